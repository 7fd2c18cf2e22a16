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
      converted as the reference's simulator does: ``int(d / (dt / S))``.  At most ``_ffi.MAX_DELAY`` steps."""
    dynamics_configs: Optional[Sequence] = None
    method: Optional[str] = None
    M: Optional[int] = None
    sim_steps: int = 1
    delay_steps: Optional[Sequence] = None
    delay: Optional[Sequence] = None

    def steps_of_delay(self, n_agents: int, dt: float) -> np.ndarray:
        """[n_agents, 2] delays in simulation steps."""
        if self.delay_steps is not None and self.delay is not None:
            raise ValueError('give delay_steps or delay, not both')
        if self.delay is not None:
            sec = np.broadcast_to(np.asarray(self.delay, dtype=float), (n_agents, NUA))
            d = np.array([[int(v / (dt / self.sim_steps)) for v in row] for row in sec], dtype=np.int64).reshape(n_agents, NUA)
        elif self.delay_steps is not None:
            raw = np.broadcast_to(np.asarray(self.delay_steps), (n_agents, NUA))
            d = raw.astype(np.int64)
            if not np.array_equal(d, raw):
                raise ValueError('delay_steps must be whole numbers of simulation steps')
        else:
            d = np.zeros((n_agents, NUA), np.int64)
        if (d < 0).any() or (d > _ffi.MAX_DELAY).any():
            raise ValueError(f'input delays must be 0 .. {_ffi.MAX_DELAY} simulation steps, got {d.tolist()}')
        return d

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
