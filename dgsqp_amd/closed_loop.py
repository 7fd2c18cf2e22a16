"""The feedback rule between two steps of a closed-loop (receding-horizon) run, on the host.

This is the documented mirror of what ``dg_closed_loop_kernel`` (csrc/dgsqp_closed_loop.h) does between two solves of one chain and
of what ``DGSQP.step()`` does for a single scenario (reference DGSQP.py:283-297):

* the plant is the game's own discrete model: the next state is stage 1 of the prediction, plus an optional disturbance (one fp64 add);
* the next warm start is the solution shifted by one stage per agent with the last row repeated --
  ``np.vstack((u_pred[1:], u_pred[-1]))`` -- unless the solve ended 'diverged' or 'qp_fail': then the warm start it started from is kept.

Everything here is exact data movement apart from that one add, so device and host agree bit for bit.

A closed-loop launch may instead run a plant of its own (``PlantModel``, ``dgsqp_set_plant``; reference
DGSQP/dynamics/dynamics_simulator.py:11-40): the game's model class with its own vehicle parameters and integrator, several simulation
steps per control step, every input channel behind a delay line.  ``plant_feedback`` is the documented mirror of that rule
(``dev_plant_feedback``, csrc/dgsqp_closed_loop.h); its delay lines are data movement again, the integration is the caller's."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _ffi
from .dynamics import INTEGRATORS, DynamicBicycleConfig, KinematicBicycleConfig

DIVERGED, QP_FAIL = 3, 4        # include/dgsqp.h: the exit codes after which step() does not shift the warm start
NUA = 2                         # every vehicle model has two inputs (DGSQP_NUA)


def shift_warm_start(u_am: np.ndarray, N: int, num_ua_d) -> np.ndarray:
    """``u_am`` [..., n] agent-major (agent a: N rows of ``num_ua_d[a]`` inputs) -> the same layout with every agent's rows moved up
    by one stage and its last row repeated."""
    u_am = np.asarray(u_am, dtype=np.float64)
    if u_am.shape[-1] != N * int(sum(num_ua_d)):
        raise ValueError(f'u_am has {u_am.shape[-1]} entries per scenario, expected {N * int(sum(num_ua_d))}')
    parts, si = [], 0
    for nu in num_ua_d:
        blk = u_am[..., si:si + N * nu].reshape(*u_am.shape[:-1], N, nu)
        parts.append(np.concatenate((blk[..., 1:, :], blk[..., -1:, :]), axis=-2).reshape(*u_am.shape[:-1], N * nu))
        si += N * nu
    return np.concatenate(parts, axis=-1)


def feedback(x_pred: np.ndarray, u_am: np.ndarray, status, u_ws_prev: np.ndarray, w=None, num_ua_d=None):
    """One feedback step for a batch (or a single scenario: no leading axis).

    ``x_pred`` [..., N+1, n_q] prediction of the solve, ``u_am`` [..., n] its solution (agent-major), ``status`` [...] its exit code,
    ``u_ws_prev`` [..., n] the warm start it started from, ``w`` [..., n_q] disturbance or None.  ``num_ua_d``: inputs per agent
    (default: two each).  Returns ``(q_next [..., n_q], u_ws_next [..., n], finite [...])``; a chain whose ``finite`` is False ends."""
    x_pred = np.asarray(x_pred, dtype=np.float64)
    u_am = np.asarray(u_am, dtype=np.float64)
    u_ws_prev = np.asarray(u_ws_prev, dtype=np.float64)
    status = np.asarray(status)
    N = x_pred.shape[-2] - 1
    if num_ua_d is None:
        num_ua_d = [NUA] * (u_am.shape[-1] // (N * NUA))
    q_next = x_pred[..., 1, :].copy()
    if w is not None:
        q_next = q_next + np.asarray(w, dtype=np.float64)
    keep = (status == DIVERGED) | (status == QP_FAIL)
    u_ws_next = np.where(keep[..., None], u_ws_prev, shift_warm_start(u_am, N, num_ua_d))
    return q_next, u_ws_next, np.isfinite(q_next).all(axis=-1)


def config_model_id(config) -> int:
    """Model class (DGSQP_MODEL_*) a dynamics config belongs to: the bicycle configs name theirs, every other ``DynamicsConfig`` is what
    the unicycle is built from (dynamics.CasadiKinematicUnicycle)."""
    if isinstance(config, DynamicBicycleConfig):
        return 1
    return 0 if isinstance(config, KinematicBicycleConfig) else 2


@dataclass
class PlantModel:
    """The plant of ``DGSQP.step_batch(..., plant=...)``: same model class, state layout and track as the game's agents, but its own

    * ``dynamics_configs``: one config per agent (vehicle parameters, tyre model, driven wheels, slip formula), or None for the game's;
    * ``method`` ('euler' | 'rk2' | 'rk3' | 'rk4') and ``M`` sub-steps per simulation step, None for the game's ('euler' takes one
      step per simulation step, as the game's model does);
    * ``sim_steps`` S simulation steps of length dt / S per control step;
    * input delay per agent and channel, [M][2] (or one value for all): ``delay_steps`` in simulation steps, or ``delay`` in seconds,
      converted as the reference's simulator does: ``int(d / (dt / S))``.  At most ``_ffi.MAX_DELAY`` steps.

    A plant PER CHAIN (``dgsqp_set_plant_ensemble``; ``perturbed_configs`` draws one): ``per_chain_configs`` [B][M], chain b's vehicles,
    and ``per_chain_delay_steps`` [B][M][2] (or ``per_chain_delay`` in seconds, converted as ``delay``), chain b's delays; B must be the
    batch size of the call.  Method, ``M`` and ``sim_steps`` are shared by all chains.  With per-chain delays alone every chain keeps
    the vehicles of ``dynamics_configs`` (or the game's)."""
    dynamics_configs: Optional[Sequence] = None
    method: Optional[str] = None
    M: Optional[int] = None
    sim_steps: int = 1
    delay_steps: Optional[Sequence] = None
    delay: Optional[Sequence] = None
    per_chain_configs: Optional[Sequence] = None
    per_chain_delay_steps: Optional[Sequence] = None
    per_chain_delay: Optional[Sequence] = None

    def _delay_steps(self, steps, seconds, shape: tuple, dt: float, what: str) -> np.ndarray:
        if steps is not None and seconds is not None:
            raise ValueError(f'give {what}_steps or {what}, not both')
        if seconds is not None:
            sec = np.broadcast_to(np.asarray(seconds, dtype=float), shape)
            d = np.array([int(v / (dt / self.sim_steps)) for v in sec.reshape(-1)], dtype=np.int64).reshape(shape)
        elif steps is not None:
            raw = np.broadcast_to(np.asarray(steps), shape)
            d = raw.astype(np.int64)
            if not np.array_equal(d, raw):
                raise ValueError(f'{what}_steps must be whole numbers of simulation steps')
        else:
            d = np.zeros(shape, np.int64)
        if (d < 0).any() or (d > _ffi.MAX_DELAY).any():
            raise ValueError(f'input delays must be 0 .. {_ffi.MAX_DELAY} simulation steps, got {d.tolist()}')
        return d

    def steps_of_delay(self, n_agents: int, dt: float) -> np.ndarray:
        """[n_agents, 2] delays in simulation steps."""
        return self._delay_steps(self.delay_steps, self.delay, (n_agents, NUA), dt, 'delay')

    @property
    def per_chain(self) -> bool:
        return self.per_chain_configs is not None or self.per_chain_delay_steps is not None or self.per_chain_delay is not None

    def lower_ensemble(self, problem: _ffi.ProblemT, B: int):
        """``(vehicles, delay)`` for ``dgsqp_set_plant_ensemble`` with a batch of ``B`` chains: a ctypes array of B * M ``dgsqp_vehicle_t``
        and an int32 array [B, M, 2] or None (host only); ``ValueError`` for what the library would refuse."""
        from .solver import fill_vehicle
        n_agents = int(problem.M)
        if int(self.sim_steps) != self.sim_steps or self.sim_steps < 1:
            raise ValueError(f'sim_steps must be a whole number >= 1, got {self.sim_steps}')
        vehicles = (_ffi.VehicleT * (B * n_agents))()
        if self.per_chain_configs is not None:
            if len(self.per_chain_configs) != B or any(len(row) != n_agents for row in self.per_chain_configs):
                raise ValueError(f'per_chain_configs must be [B][M] = [{B}][{n_agents}] configs')
            for b, row in enumerate(self.per_chain_configs):
                for a, cfg in enumerate(row):
                    if config_model_id(cfg) != problem.agents[a].model:
                        raise ValueError(f'per-chain plant config [{b}][{a}] is of model class {config_model_id(cfg)}, the game\'s agent is of '
                                         f'class {problem.agents[a].model}: a plant keeps the game\'s model class and state layout')
                    fill_vehicle(vehicles[b * n_agents + a], config_model_id(cfg), cfg)
        else:                       # per-chain delays alone: every chain has the shared plant's vehicles
            base = self.lower(problem)
            src = problem.agents if base.use_game_agents else base.agents
            for a in range(n_agents):
                one = _ffi.VehicleT.from_buffer_copy(bytes(src[a])[:C.sizeof(_ffi.VehicleT)])
                for b in range(B):
                    vehicles[b * n_agents + a] = one
        delay = None
        if self.per_chain_delay_steps is not None or self.per_chain_delay is not None:
            for given in (self.per_chain_delay_steps, self.per_chain_delay):
                if given is not None and np.shape(given) != (B, n_agents, NUA):
                    raise ValueError(f'per-chain delays must be [B][M][2] = {(B, n_agents, NUA)}, got {np.shape(given)}')
            delay = np.ascontiguousarray(self._delay_steps(self.per_chain_delay_steps, self.per_chain_delay, (B, n_agents, NUA), float(problem.dt),
                                                           'per_chain_delay'), dtype=np.int32)
        return vehicles, delay

    def lower(self, problem: _ffi.ProblemT) -> _ffi.PlantT:
        """``dgsqp_plant_t`` for the game ``problem`` (host only); ``ValueError`` for what the library would refuse."""
        from .solver import fill_vehicle
        n_agents = int(problem.M)
        if int(self.sim_steps) != self.sim_steps or self.sim_steps < 1:
            raise ValueError(f'sim_steps must be a whole number >= 1, got {self.sim_steps}')
        pt = _ffi.PlantT()
        pt.sim_steps = int(self.sim_steps)
        if self.method is None:
            pt.integrator = problem.integrator
        elif self.method in INTEGRATORS:
            pt.integrator = INTEGRATORS[self.method]
        else:
            raise ValueError(f'Discretization method of {self.method} not recognized')
        pt.substeps = int(problem.substeps if self.M is None else self.M)
        if pt.substeps < 1:
            raise ValueError(f'M must be at least 1, got {self.M}')
        for a, row in enumerate(self.steps_of_delay(n_agents, float(problem.dt))):
            for j in range(NUA):
                pt.delay[a][j] = int(row[j])
        pt.use_game_agents = int(self.dynamics_configs is None)
        if self.dynamics_configs is not None:
            if len(self.dynamics_configs) != n_agents:
                raise ValueError(f'Number of agents: {n_agents}, but {len(self.dynamics_configs)} plant configs were provided')
            for a, cfg in enumerate(self.dynamics_configs):
                if config_model_id(cfg) != problem.agents[a].model:
                    raise ValueError(f'plant config {a} is of model class {config_model_id(cfg)}, the game\'s agent is of class '
                                     f'{problem.agents[a].model}: a plant keeps the game\'s model class and state layout')
                fill_vehicle(pt.agents[a], config_model_id(cfg), cfg)
        return pt


def new_lines(delay_steps, lead=()) -> list:
    """Empty (zero) delay lines: one array [*lead, d] per input channel of the joint input, oldest entry first; ``delay_steps`` [n_u] (or
    [M][2], flattened agent after agent)."""
    return [np.zeros(tuple(lead) + (int(d),)) for d in np.asarray(delay_steps).reshape(-1)]


def plant_feedback(fd, q: np.ndarray, u_new: np.ndarray, lines: list, sim_steps: int = 1, w=None):
    """One control step of the plant for a batch (or a single scenario: no leading axis) -- the host mirror of ``dev_plant_feedback``.

    For each of the ``sim_steps`` simulation steps: a channel whose line is not empty integrates under the line's oldest entry and
    ``u_new`` is then appended to the line; a channel with an empty line (d = 0) integrates under ``u_new``; the state advances by
    ``fd(q, u) -> q_next``, ONE simulation step (length dt / sim_steps) of the caller's choice.  After the last step ``w`` is added.
    ``lines`` (``new_lines``) are updated in place: they persist from control step to control step and start as zeros.
    Returns ``(q_next [..., n_q], u_used [..., sim_steps, n_u], finite [...])``."""
    q = np.asarray(q, dtype=np.float64)
    u_new = np.asarray(u_new, dtype=np.float64)
    if len(lines) != u_new.shape[-1]:
        raise ValueError(f'{len(lines)} delay lines for {u_new.shape[-1]} input channels')
    used = []
    for _ in range(int(sim_steps)):
        u = u_new.copy()
        for ch, line in enumerate(lines):
            if line.shape[-1] > 0:
                u[..., ch] = line[..., 0]
                line[..., :-1] = line[..., 1:].copy()
                line[..., -1] = u_new[..., ch]
        used.append(u)
        q = np.asarray(fd(q, u), dtype=np.float64)
    if w is not None:
        q = q + np.asarray(w, dtype=np.float64)
    return q, np.stack(used, axis=-2), np.isfinite(q).all(axis=-1)


def perturbed_configs(configs: Sequence, spread: dict, B: int, seed: int) -> list:
    """An ensemble of vehicles for ``PlantModel(per_chain_configs=...)``: [B][M] copies of ``configs`` (one dynamics config per agent) in
    which every field named by ``spread`` (field -> relative half-width s) holds

        nominal * (1 + s * (2 U - 1)),     U = sampler.uniform(seed, b, k),

    the counter-based uniform of ``sampler.py`` keyed by the seed, the chain b and k = a * len(spread) + (index of the field in
    ``spread``'s order) -- so chain b's vehicle does not depend on B, and s = 0 returns the nominal value bit for bit."""
    import copy
    from . import sampler
    fields = list(spread)
    for f, s in spread.items():
        if not 0.0 <= float(s) < 1.0:
            raise ValueError(f'spread of {f} must be a relative half-width in [0, 1), got {s}')
        for a, c in enumerate(configs):
            if not hasattr(c, f):
                raise ValueError(f'config {a} has no field {f}')
    out = [[copy.deepcopy(c) for c in configs] for _ in range(int(B))]
    chains = np.arange(int(B))
    for a, c in enumerate(configs):
        for i, f in enumerate(fields):
            U = sampler.uniform(int(seed), chains, a * len(fields) + i)
            vals = float(getattr(c, f)) * (1.0 + float(spread[f]) * (2.0 * U - 1.0))
            for b in range(int(B)):
                setattr(out[b][a], f, float(vals[b]))
    return out


def monitor(z: np.ndarray, radii, st_lb, st_ub, qoff):
    """The safety monitor of one control step for a batch (or a single scenario: no leading axes) -- the host mirror of what
    ``dgsqp_set_monitor`` records.  ``z`` [..., S, n_q]: the joint state after each of the S simulation steps (the last one with the
    disturbance added: it is q[t+1]); ``radii`` [M]; ``st_lb``, ``st_ub`` [n_q] the game's state bounds (+-inf: absent); ``qoff`` [M+1]
    where each agent's state block starts.  Returns ``(clearance [...], box_excess [...], first_hit [...])``:

    * clearance: min over j and pairs i < k of sqrt(dx^2 + dy^2) - (radius_i + radius_k), positions = the first two entries of each
      block; +inf for M = 1;
    * box_excess: max over j and entries with a finite bound of max(z - st_ub, st_lb - z); -inf when there is none;
    * both NaN when an entry of ``z`` is not finite;
    * first_hit: the smallest j whose pairwise clearance is < 0, or -1."""
    z = np.asarray(z, dtype=np.float64)
    radii = np.asarray(radii, dtype=np.float64)
    lb, ub = np.asarray(st_lb, dtype=np.float64), np.asarray(st_ub, dtype=np.float64)
    M = len(radii)
    lead = z.shape[:-2]
    per_step = np.full(z.shape[:-1], np.inf)                            # [..., S] clearance of each simulation step
    for i in range(M):
        for k in range(i + 1, M):
            dx, dy = z[..., qoff[i]] - z[..., qoff[k]], z[..., qoff[i] + 1] - z[..., qoff[k] + 1]
            per_step = np.minimum(per_step, np.sqrt(dx * dx + dy * dy) - (radii[i] + radii[k]))
    clearance = per_step.min(axis=-1)
    box = np.full(lead, -np.inf)
    with np.errstate(invalid='ignore'):
        for i in range(z.shape[-1]):
            if np.isfinite(ub[i]):
                box = np.maximum(box, (z[..., i] - ub[i]).max(axis=-1))
            if np.isfinite(lb[i]):
                box = np.maximum(box, (lb[i] - z[..., i]).max(axis=-1))
        hit = per_step < 0
    first = np.where(hit.any(axis=-1), hit.argmax(axis=-1), -1)
    bad = ~np.isfinite(z).all(axis=(-1, -2))
    return np.where(bad, np.nan, clearance), np.where(bad, np.nan, box), first
