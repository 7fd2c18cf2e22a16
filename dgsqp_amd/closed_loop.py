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
(``dev_plant_feedback``, csrc/dgsqp_closed_loop.h); its delay lines are data movement again, the integration is the caller's.

A launch with a plant may also choose, per agent and per chain, who produces the command that enters the plant (``Drivers``,
``dgsqp_set_drivers``): the game, the reference's PID lane follower run closed-loop on the true state, or a replayed sequence.
``pid_driver_step`` and ``drive`` are the documented mirrors of that choice (``dev_pid_law`` in csrc/dgsqp_pid.h, the drivers overload of
``dev_plant_feedback``); the command they return is what ``plant_feedback`` takes as ``u_new``.

A launch may carry the command of step t into solve t + 1 as the input before its stage 0 (``step_batch(..., u_prev=True)``,
``dgsqp_set_closed_loop_u_prev``): ``next_u_prev`` is the mirror of that rule.

A launch with a plant may hold a plan across control steps (``PlanHold``, ``dgsqp_set_plan_hold``): a planning rate below the control
rate, and the next stage of the last accepted plan as the command after a failed solve.  ``hold_step`` is the mirror of that rule.

A plant may be of ANOTHER model class than the game's agent (``PlantModel(own_class=True)``, ``dgsqp_set_cross_plant``): it keeps a state
``z`` of its own and the game sees the projection ``project_state`` of it; ``lift_state`` is the default ``z0``.  A 'track' driver follows
the game's plan on such a plant: ``track_reference`` is the reference it steers towards, ``drive`` / ``pid_driver_step`` the law."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _ffi
from .dynamics import INTEGRATORS, DynamicBicycleConfig, KinematicBicycleConfig, rk_step

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


def config_model_id(config, game_model: Optional[int] = None) -> int:
    """Model class (DGSQP_MODEL_*) a dynamics config belongs to: the bicycle configs name theirs, every other ``DynamicsConfig`` is what
    the two unicycles are built from (dynamics.CasadiKinematicUnicycle, class 2, and the Frenet point mass
    dynamics.CasadiKinematicUnicycleCombined, class 3).  Such a config does not say which; ``game_model``, the class of the game's
    agent it is a plant for, decides between the two, and it is class 2 where that is a bicycle (which then refuses it) or not given."""
    if isinstance(config, DynamicBicycleConfig):
        return 1
    if isinstance(config, KinematicBicycleConfig):
        return 0
    return 3 if game_model == 3 else 2


MODEL_NQ = {0: 6, 1: 8, 2: 4, 3: 6}     # states per model class (dg_model_nq)
SIX_OF_EIGHT = (0, 1, 2, 5, 6, 7)       # [x, y, v, e_psi, s, e_y] of [x, y, vx, vy, w, e_psi, s, e_y]
CROSS_PAIRS = ((0, 1), (3, 0), (3, 1))  # (game class, plant class) besides the same class: the table in include/dgsqp.h


def cross_projection(game_class: int, plant_class: int) -> tuple:
    """Which entries of a plant agent's state block the game's agent sees; ``ValueError`` for a pair outside the table."""
    g, p = int(game_class), int(plant_class)
    if g not in MODEL_NQ or p not in MODEL_NQ or (g != p and (g, p) not in CROSS_PAIRS):
        raise ValueError(f'a game agent of model class {g} on a plant of class {p} is not a supported pair (same class, 0 -> 1, 3 -> 0, 3 -> 1)')
    return SIX_OF_EIGHT if MODEL_NQ[p] == 8 and MODEL_NQ[g] == 6 else tuple(range(MODEL_NQ[g]))


def _blocks(classes):
    return np.concatenate(([0], np.cumsum([MODEL_NQ[int(c)] for c in classes])))


def project_state(game_classes, plant_classes, z) -> np.ndarray:
    """``q = p(z)``: ``z`` [..., n_z] (the plant agents' blocks, agent after agent) -> [..., n_q] in the game's layout.  Data movement."""
    z = np.asarray(z, dtype=np.float64)
    zoff = _blocks(plant_classes)
    if len(game_classes) != len(plant_classes) or z.shape[-1] != zoff[-1]:
        raise ValueError(f'z has {z.shape[-1]} entries per chain, the plant classes {list(plant_classes)} have {zoff[-1]}')
    return np.concatenate([z[..., [zoff[a] + i for i in cross_projection(g, p)]] for a, (g, p) in enumerate(zip(game_classes, plant_classes))], axis=-1)


def lift_state(game_classes, plant_classes, x0) -> np.ndarray:
    """A plant state whose projection is ``x0`` [..., n_q]: the entries the game does not see (vy, w) are zero."""
    x0 = np.asarray(x0, dtype=np.float64)
    qoff, zoff = _blocks(game_classes), _blocks(plant_classes)
    if len(game_classes) != len(plant_classes) or x0.shape[-1] != qoff[-1]:
        raise ValueError(f'x0 has {x0.shape[-1]} entries per chain, the game classes {list(game_classes)} have {qoff[-1]}')
    z = np.zeros(x0.shape[:-1] + (int(zoff[-1]),))
    for a, (g, p) in enumerate(zip(game_classes, plant_classes)):
        z[..., [zoff[a] + i for i in cross_projection(g, p)]] = x0[..., qoff[a]:qoff[a + 1]]
    return z


def track_reference(model, q_agent, g, method: Optional[str] = None, dt: Optional[float] = None, M: Optional[int] = None) -> np.ndarray:
    """The state a 'track' driver steers towards: one step of the discrete model of the GAME's agent (``model``: a numpy model of
    ``dynamics``) from ``q_agent`` -- the projection of the plant agent's true state -- under the game's command ``g``.  ``method``, ``dt``
    and ``M`` are the joint model's (a game discretises every agent with them); by default the model's own, and the result is then
    ``model.fd(q_agent, g)`` where the model has one.  The references are entries 2 (v), last (lateral) and e_psi of the result."""
    method = model.model_config.discretization_method if method is None else method
    return rk_step(lambda z: model.fc(z, g), q_agent, method, float(model.dt if dt is None else dt), int(model.M if M is None else M))


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
    the vehicles of ``dynamics_configs`` (or the game's).

    ``own_class=True``: the configs may be of ANOTHER model class than the game's agents (``dgsqp_set_cross_plant``; the pairs of
    ``cross_projection``): the plant then keeps a state of its own, ``step_batch`` takes ``z0`` and returns ``z``."""
    dynamics_configs: Optional[Sequence] = None
    method: Optional[str] = None
    M: Optional[int] = None
    sim_steps: int = 1
    delay_steps: Optional[Sequence] = None
    delay: Optional[Sequence] = None
    per_chain_configs: Optional[Sequence] = None
    per_chain_delay_steps: Optional[Sequence] = None
    per_chain_delay: Optional[Sequence] = None
    own_class: bool = False

    def plant_classes(self, problem: _ffi.ProblemT) -> list:
        """The model class of each plant agent: its config's, or the game's where there is none."""
        game = [int(problem.agents[a].model) for a in range(int(problem.M))]
        if self.dynamics_configs is None:
            return game
        return [config_model_id(c, g) for c, g in zip(self.dynamics_configs, game)]

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
        classes = self.plant_classes(problem) if self.own_class else None
        if self.per_chain_configs is not None:
            if len(self.per_chain_configs) != B or any(len(row) != n_agents for row in self.per_chain_configs):
                raise ValueError(f'per_chain_configs must be [B][M] = [{B}][{n_agents}] configs')
            for b, row in enumerate(self.per_chain_configs):
                for a, cfg in enumerate(row):
                    mid = config_model_id(cfg, problem.agents[a].model)
                    if self.own_class and mid != classes[a]:
                        raise ValueError(f'per-chain plant config [{b}][{a}] is of model class {mid}, the plant\'s agent is of class {classes[a]}')
                    if not self.own_class and mid != problem.agents[a].model:
                        raise ValueError(f'per-chain plant config [{b}][{a}] is of model class {mid}, the game\'s agent is of '
                                         f'class {problem.agents[a].model}: a plant keeps the game\'s model class and state layout')
                    fill_vehicle(vehicles[b * n_agents + a], mid, cfg)
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
        """``dgsqp_plant_t`` for the game ``problem`` (host only) -- with ``own_class`` what ``dgsqp_set_cross_plant`` takes --; ``ValueError``
        for what the library would refuse."""
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
                mid = config_model_id(cfg, problem.agents[a].model)
                if self.own_class:
                    cross_projection(problem.agents[a].model, mid)
                elif mid != problem.agents[a].model:
                    raise ValueError(f'plant config {a} is of model class {mid}, the game\'s agent is of class '
                                     f'{problem.agents[a].model}: a plant keeps the game\'s model class and state layout')
                fill_vehicle(pt.agents[a], mid, cfg)
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


DRIVER_KINDS = {'game': _ffi.DRIVER_GAME, 'pid': _ffi.DRIVER_PID, 'replay': _ffi.DRIVER_REPLAY, 'track': _ffi.DRIVER_TRACK}
UNICYCLE = 2                    # DGSQP_MODEL_UNICYCLE: no e_y / e_psi, so no lane follower


@dataclass
class PidGains:
    """The lane follower of ``dgsqp_pid_t`` (defaults: what the warm-start PID runs with): speed P gain, steering PI gains on
    ``ey_gain (e_y - lat_ref) + e_psi``, the integrator clamp, and per input (u_a, u_steer) the magnitude limit and the largest change
    per control step."""
    kp_v: float = 1.0
    kp_s: float = 1.0
    ki_s: float = 0.005
    ey_gain: float = 5.0
    ei_max: float = 100.0
    u_max: Sequence = (2.1, 0.436)
    du_max: Sequence = (10.0, 4.5)

    def fill(self, out: _ffi.PidT):
        out.kp_v, out.kp_s, out.ki_s, out.ey_gain, out.ei_max = float(self.kp_v), float(self.kp_s), float(self.ki_s), float(self.ey_gain), float(self.ei_max)
        for j in range(NUA):
            out.u_max[j], out.du_max[j] = float(self.u_max[j]), float(self.du_max[j])
        out.substeps = 1            # (not read by the driver: the plant integrates)


def _kind_id(k) -> int:
    if isinstance(k, str):
        if k not in DRIVER_KINDS:
            raise ValueError(f"driver kind {k!r} not recognized: 'game', 'pid', 'replay' or 'track'")
        return DRIVER_KINDS[k]
    if int(k) != k or int(k) not in DRIVER_KINDS.values():
        raise ValueError(f'driver kind {k!r} not recognized: 0 (game), 1 (pid), 2 (replay) or 3 (track)')
    return int(k)


@dataclass
class Drivers:
    """Who produces the command that enters each agent's plant in ``DGSQP.step_batch(..., drivers=...)`` (``dgsqp_set_drivers``):

    * ``kinds`` [M]: 'game' (stage 0 of the game's solution, as without drivers), 'pid' (the lane follower ``pid`` run closed-loop on the
      TRUE state; 6- and 8-state models only), 'replay' (``u_replay``) or 'track' (the lane follower towards ``track_reference`` of the game's
      command; only with ``PlantModel(own_class=True)``), or the numbers 0 .. 3;
    * ``pid``: one ``PidGains`` for all agents or one per agent (default: ``PidGains()``);
    * ``per_chain_kinds`` [B][M]: the kinds of every chain, in place of ``kinds``;
    * ``refs`` [B][M][2]: (v_ref, lat_ref) of the PID agents per chain; None: (v, e_y) of the chain's x0, as the warm-start PID does;
    * ``u_replay`` [B][T][n_u]: the commands of the 'replay' agents (joint inputs, agent after agent; other agents' entries are not read).

    The solves do not change and the warm start stays the shifted joint solution: the game's belief about everybody."""
    kinds: Optional[Sequence] = None
    pid: object = None
    per_chain_kinds: Optional[Sequence] = None
    refs: Optional[Sequence] = None
    u_replay: Optional[Sequence] = None

    def gains(self, n_agents: int) -> list:
        """One ``PidGains`` per agent."""
        if self.pid is None:
            return [PidGains() for _ in range(n_agents)]
        if isinstance(self.pid, PidGains):
            return [self.pid] * n_agents
        if len(self.pid) != n_agents or not all(isinstance(p, PidGains) for p in self.pid):
            raise ValueError(f'pid must be one PidGains or one per agent ({n_agents})')
        return list(self.pid)

    def lower(self, problem: _ffi.ProblemT, B: int, T: int, plant_classes=None):
        """``plant_classes``: the classes of a cross plant's agents (``PlantModel.plant_classes``), None without one.
        ``(drivers, kind, ref, u_replay)`` for ``dgsqp_set_drivers`` with a launch of ``B`` chains and ``T`` steps: a ``DriversT``, an
        int32 array [B, M] or None, a float64 array [B, M, 2] or None and a float64 array [T, B, n_u] (step-major, as the library takes
        it) or None (host only); ``ValueError`` for what the library would refuse."""
        M = int(problem.M)
        n_u = M * NUA
        if int(T) < 1:
            raise ValueError(f'drivers: T must be at least 1, got {T}')
        if int(B) < 0:
            raise ValueError('drivers: B must not be negative')
        kinds = [_ffi.DRIVER_GAME] * M if self.kinds is None else [_kind_id(k) for k in self.kinds]
        if len(kinds) != M:
            raise ValueError(f'Number of agents: {M}, but {len(kinds)} driver kinds were provided')
        per_chain = None
        if self.per_chain_kinds is not None:
            if np.shape(self.per_chain_kinds) != (B, M):
                raise ValueError(f'per_chain_kinds must be [B][M] = {(B, M)}, got {np.shape(self.per_chain_kinds)}')
            per_chain = np.array([[_kind_id(k) for k in row] for row in self.per_chain_kinds], dtype=np.int32).reshape(B, M)
        every = np.array([kinds], dtype=np.int32) if per_chain is None else np.concatenate((np.array([kinds], dtype=np.int32), per_chain))
        for a in range(M):
            if (every[:, a] == _ffi.DRIVER_PID).any() and problem.agents[a].model == UNICYCLE:
                raise ValueError(f'PID driver for agent {a}, a unicycle: the lane follower needs e_y and e_psi (the 6- and 8-state models)')
            if (every[:, a] == _ffi.DRIVER_TRACK).any():
                if plant_classes is None:
                    raise ValueError(f"driver kind 'track' (3) of agent {a} not recognized without a plant of its own class: PlantModel(own_class=True)")
                if problem.agents[a].model == UNICYCLE:
                    raise ValueError(f"'track' driver for agent {a}, a unicycle: the lane follower needs e_y and e_psi (the 6- and 8-state models)")
            if plant_classes is not None and problem.agents[a].model == 3 and plant_classes[a] != 3 and (every[1 if per_chain is not None else 0:, a] == _ffi.DRIVER_GAME).any():
                raise ValueError(f"drivers: agent {a} is a point mass (inputs Fx, wz) on a bicycle plant (acceleration, steering): a 'game' driver "
                                 "cannot command it; use 'track', 'pid' or 'replay'")
        ref = None
        if self.refs is not None:
            ref = np.ascontiguousarray(self.refs, dtype=np.float64)
            if ref.shape != (B, M, 2):
                raise ValueError(f'refs must be [B][M][2] = {(B, M, 2)}, got {ref.shape}')
        rep = None
        if self.u_replay is not None:
            rep = np.asarray(self.u_replay, dtype=np.float64)
            if rep.shape != (B, T, n_u):
                raise ValueError(f'u_replay must be [B, steps, n_u] = {(B, T, n_u)}, got {rep.shape}')
            rep = np.ascontiguousarray(rep.transpose(1, 0, 2))
        elif (every == _ffi.DRIVER_REPLAY).any():
            raise ValueError("a 'replay' driver needs u_replay")
        dt = _ffi.DriversT()
        for a, g in enumerate(self.gains(M)):
            dt.kind[a] = kinds[a]
            g.fill(dt.pid[a])
        return dt, per_chain, ref, rep


def new_pid_state(lead=()) -> np.ndarray:
    """The lane follower's state when a chain starts: [*lead, 3] zeros (integrator, previous u_a, previous u_steer)."""
    return np.zeros(tuple(lead) + (3,))


def pid_driver_step(pid: PidGains, q_agent, ref, state, dt: float, epsi_ref: float = 0.0):
    """One control step of the PID driver for one agent -- the host mirror of ``dev_pid_law``: the operations of ``pid.PID.solve`` in its
    order, with Kd = 0, symmetric limits and u_ref = 0.  ``q_agent`` [n_qa] the agent's TRUE state (6- or 8-state model: v at 2, e_psi at 3
    or 5, e_y last), ``ref`` (v_ref, lat_ref), ``state`` [3] (integrator, previous u_a, previous u_steer), ``dt`` the control step.
    ``epsi_ref`` (a 'track' driver's): the law sees ``e_psi - epsi_ref`` in place of ``e_psi``.
    Returns ``(u [2], state [3])``; ``state`` itself is not changed."""
    q_agent = np.asarray(q_agent, dtype=np.float64)
    if q_agent.shape[-1] not in (6, 8):
        raise ValueError(f'the lane follower needs e_y and e_psi: a 6- or 8-state agent, got {q_agent.shape[-1]} states')
    v, epsi, ey = float(q_agent[2]), float(q_agent[5 if q_agent.shape[-1] == 8 else 3]), float(q_agent[-1])
    if epsi_ref:
        epsi = epsi - float(epsi_ref)
    ei, up0, up1 = (float(x) for x in state)
    ua = -(pid.kp_v * (v - float(ref[0])))
    e = pid.ey_gain * (ey - float(ref[1])) + epsi
    ei = min(max(ei + e * dt, -pid.ei_max), pid.ei_max)
    us = -(pid.kp_s * e + pid.ki_s * ei)
    ua = min(max(min(max(ua - up0, -pid.du_max[0]), pid.du_max[0]) + up0, -pid.u_max[0]), pid.u_max[0])
    us = min(max(min(max(us - up1, -pid.du_max[1]), pid.du_max[1]) + up1, -pid.u_max[1]), pid.u_max[1])
    return np.array([ua, us]), np.array([ei, ua, us])


def drive(kinds, u_game, q, gains, refs, states, dt: float, qoff, u_replay=None, track_refs=None):
    """The commands of one control step of one chain -- the host mirror of the drivers overload of ``dev_plant_feedback``.  Per agent a:
    kind 0 takes ``u_game[2a:2a+2]`` (stage 0 of the solution), kind 1 ``pid_driver_step(gains[a], q[qoff[a]:qoff[a+1]], refs[a],
    states[a], dt)``, kind 2 ``u_replay[2a:2a+2]``.  ``kinds`` [M], ``u_game`` [n_u], ``q`` [n_q] the TRUE state, ``refs`` [M, 2],
    ``states`` [M, 3].  With a cross plant ``q`` is the PLANT's state z and ``qoff`` its blocks; kind 3 ('track') is
    ``pid_driver_step(gains[a], z_a, track_refs[a][:2], states[a], dt, epsi_ref=track_refs[a][2])`` with ``track_refs`` [M, 3] =
    (v_ref, lat_ref, epsi_ref) from ``track_reference``.  Returns ``(u_cmd [n_u], states [M, 3])``; only PID and track agents' states
    change (in the returned copy)."""
    u_game = np.asarray(u_game, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    states = np.array(states, dtype=np.float64)
    u_cmd = u_game.copy()
    for a, k in enumerate(kinds):
        k = _kind_id(k)
        if k == _ffi.DRIVER_PID:
            u_cmd[NUA * a:NUA * a + NUA], states[a] = pid_driver_step(gains[a], q[qoff[a]:qoff[a + 1]], refs[a], states[a], dt)
        elif k == _ffi.DRIVER_TRACK:
            if track_refs is None:
                raise ValueError("driver kind 'track' (3) not recognized without track_refs (closed_loop.track_reference of the game's command)")
            r = np.asarray(track_refs, dtype=np.float64)[a]
            u_cmd[NUA * a:NUA * a + NUA], states[a] = pid_driver_step(gains[a], q[qoff[a]:qoff[a + 1]], r[:2], states[a], dt, epsi_ref=r[2])
        elif k == _ffi.DRIVER_REPLAY:
            if u_replay is None:
                raise ValueError("a 'replay' driver needs u_replay")
            u_cmd[NUA * a:NUA * a + NUA] = np.asarray(u_replay, dtype=np.float64)[NUA * a:NUA * a + NUA]
    return u_cmd, states


REFERENCE_FAIL_MASK = (1 << DIVERGED) | (1 << QP_FAIL)      # the statuses after which step() keeps its warm start (DGSQP.py:293-295)
CONVERGED_FAIL_MASK = 0b111100                              # every status but the two converged ones: 2 .. 5
ON_FAIL = {'reference': _ffi.HOLD_REFERENCE, 'hold': _ffi.HOLD_HOLD}


@dataclass
class PlanHold:
    """Holding a plan across control steps in ``DGSQP.step_batch(..., hold=...)`` (``dgsqp_set_plan_hold``): a chain holds a plan -- its
    warm start -- and consumes it stage by stage until a newer one is accepted.

    * ``replan_every`` R, 1 .. N: a chain solves, and once a solve is accepted follows that plan for R control steps before the next;
    * ``on_fail``: what a chain applies after a failed solve -- 'reference': stage 0 of the failed iterate, keeping the warm start
      unshifted (``DGSQP.step()``, the default); 'hold': the next stage of the plan it holds, and the solve is retried at the next step;
    * ``accept``: which solves count as failed -- 'reference': 'diverged' and 'qp_fail'; 'converged': every status but the two converged
      ones; or a mask with bit s set when status s (0 .. 5) is a failure.

    The rule of one step is ``hold_step``.  The defaults are, bit for bit, the launch without ``hold``."""
    replan_every: int = 1
    on_fail: str = 'reference'
    accept: object = 'reference'

    def __post_init__(self):
        if isinstance(self.replan_every, bool) or int(self.replan_every) != self.replan_every or self.replan_every < 1:
            raise ValueError(f'replan_every must be a whole number >= 1, got {self.replan_every!r}')
        if self.on_fail not in ON_FAIL:
            raise ValueError(f"on_fail {self.on_fail!r} not recognized: 'reference' or 'hold'")
        self.mask           # (validates accept)

    @property
    def mask(self) -> int:
        """The fail mask: bit s set when status s counts as a failed solve."""
        if isinstance(self.accept, str):
            if self.accept not in ('reference', 'converged'):
                raise ValueError(f"accept {self.accept!r} not recognized: 'reference', 'converged' or a mask of the statuses 0 .. 5")
            return REFERENCE_FAIL_MASK if self.accept == 'reference' else CONVERGED_FAIL_MASK
        if isinstance(self.accept, bool) or int(self.accept) != self.accept or not 0 <= int(self.accept) < 64:
            raise ValueError(f'accept as a mask holds bits 0 .. 5 (one per status), got {self.accept!r}')
        return int(self.accept)

    def lower(self, problem: _ffi.ProblemT) -> _ffi.HoldT:
        """``dgsqp_hold_t`` for the game ``problem`` (host only); ``ValueError`` for what the library would refuse."""
        if int(self.replan_every) > int(problem.N):
            raise ValueError(f'replan_every must be 1 .. N = {int(problem.N)}, got {self.replan_every}')
        ht = _ffi.HoldT()
        ht.replan_every, ht.on_fail, ht.fail_mask, ht.reserved = int(self.replan_every), ON_FAIL[self.on_fail], self.mask, 0
        return ht


def hold_step(status, u_t, u_ws_t, age: int, due: bool, hold: PlanHold, N: int, num_ua_d):
    """One control step of one chain that holds a plan -- the host mirror of ``dev_hold_due``, the hold overload of ``dev_plant_feedback``
    and ``dev_hold_next`` (csrc/dgsqp_closed_loop.h; the table in include/dgsqp.h).  ``status``: the exit code of the step's solve, or
    None on a held step (no solve: exactly when ``due`` is False); ``u_t`` [n] the solve's iterate (agent-major; not read on a held step,
    may be None), ``u_ws_t`` [n] the warm start the chain holds; ``age``, ``due`` the chain's state before the step (0, True when it
    starts).  Returns ``(u_game [n_u], u_ws_next [n], age, due, plan_stage)``:

    * due, status not in the mask: stage 0 of ``u_t``; ``shift(u_t)``; age 1, due = (1 >= R); plan_stage 0
    * due, failed, 'reference':    stage 0 of ``u_t``; ``u_ws_t`` unshifted; age and due unchanged; plan_stage 0
    * due, failed, 'hold':         stage 0 of ``u_ws_t``; ``shift(u_ws_t)``; age + 1, due stays; plan_stage = age before
    * not due (held):              stage 0 of ``u_ws_t``; ``shift(u_ws_t)``; age + 1, due = (age >= R); plan_stage = age before

    Pure data movement: device and host agree bit for bit."""
    if (status is None) == bool(due):
        raise ValueError('a chain solves exactly when a plan is due: status is None on a held step and only there')
    R = int(hold.replan_every)
    u_ws_t = np.asarray(u_ws_t, dtype=np.float64)
    first = np.cumsum([0] + [N * int(nu) for nu in num_ua_d])       # where each agent's rows start
    stage0 = lambda u: np.concatenate([u[first[a]:first[a] + int(nu)] for a, nu in enumerate(num_ua_d)])
    failed = status is not None and 0 <= int(status) <= 5 and bool((hold.mask >> int(status)) & 1)
    if status is not None and not failed:
        u_t = np.asarray(u_t, dtype=np.float64)
        return stage0(u_t), shift_warm_start(u_t, N, num_ua_d), 1, 1 >= R, 0
    if failed and hold.on_fail == 'reference':
        return stage0(np.asarray(u_t, dtype=np.float64)), u_ws_t.copy(), int(age), bool(due), 0
    new_age = int(age) + 1
    return stage0(u_ws_t), shift_warm_start(u_ws_t, N, num_ua_d), new_age, bool(due) if failed else new_age >= R, int(age)


def next_u_prev(u_t_stage0, u_cmd=None, kinds=None) -> np.ndarray:
    """The input a chain's next solve takes as applied before its stage 0 (``step_batch(..., u_prev=...)``,
    ``dgsqp_set_closed_loop_u_prev``) -- the host mirror of the carry in ``dg_closed_loop_kernel``: per agent, the command that entered that
    agent's plant at this step.  ``u_t_stage0`` [..., n_u] is stage 0 of the solve's solution as returned (``u_applied``; also after
    'diverged' / 'qp_fail', the feedback applies it then as well); ``u_cmd`` [..., n_u] the commands of a launch with drivers (``drive``), which
    then take its place: a PID or replay agent's own command is what the game sees as that agent's previous input.  With delay lines this
    is the value appended to the line, not the delayed one the plant integrated under.  ``kinds`` [M] (with ``u_cmd``): a 'track' agent's command
    is in the plant's units, so its entries take the GAME's command ``u_t_stage0`` (u_game).  Pure data movement: a copy."""
    src = np.asarray(u_t_stage0 if u_cmd is None else u_cmd, dtype=np.float64)
    if u_cmd is not None and src.shape != np.shape(u_t_stage0):
        raise ValueError(f'u_cmd has shape {src.shape}, stage 0 of the solution {np.shape(u_t_stage0)}')
    out = src.copy()
    if u_cmd is not None and kinds is not None:
        for a, k in enumerate(kinds):
            if _kind_id(k) == _ffi.DRIVER_TRACK:
                out[..., NUA * a:NUA * a + NUA] = np.asarray(u_t_stage0, dtype=np.float64)[..., NUA * a:NUA * a + NUA]
    return out
