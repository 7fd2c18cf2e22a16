"""LTV-MPC reference tracker (reference DGSQP/solvers/CA_LTV_MPC.py, ``qp_interface='casadi'``) on the device.

``CA_LTV_MPC(dynamics, costs, constraints, bounds, params)`` has the reference's surface -- ``set_warm_start``, ``solve``, ``step``,
``get_prediction``, ``q_pred`` / ``u_pred`` / ``du_pred`` -- over one launch of ``dg_mpc_kernel`` (csrc/dgsqp_mpc.h);
``solve_batch`` runs many scenarios at once; ``mpc_batch(solver, agent, ...)`` (``DGSQP.mpc_batch``) runs it for one agent of an existing
game's handle.  CasADi functions cannot cross the C-ABI, so cost and constraints are declarative records that cover what the reference's
three callers build (scripts/race/car{1,2}_tracking_controller_setup.py, comparison_study_*/warm_start*.py):

    TrackingCost        0.5 (q - q_ref_k)' diag(state_weight) (q - q_ref_k) at stages 0..N (+ terminal_linear' q_N),
                        0.5 u' diag(input_weight) u, 0.5 du' diag(rate_weight) du
    SoftStateBounds     comes from ``CALTVMPCParams.soft_state_bound_*`` (one soft state)
    ObstacleAvoidance   (2 r)^2 - |(x, y) - p_obs_k|^2 <= 0 at stages 1..N
    TrackEdgeRows       e_y - left_width(s) <= 0 and -right_width(s) - e_y <= 0 at stages 1..N, the track's width functions
                        (comparison_study_f1/warm_start.py:112-118); hard rows, linearised about D like the obstacle row

Two stated deviations: the QP is solved exactly where the reference calls OSQP with polish
(``rate_weight > 0`` is required, so the minimiser is unique); ``state_scaling`` is accepted and ignored -- a change of variables that does
not move the exact minimiser (only the reference's ``1e-10 I`` term moves with it).  ``input_scaling`` is accepted as what it is in the
reference: with ``Tu = 1 / input_scaling`` the reference leaves ``u_{k+1} = u_k + dt du`` unscaled (CA_LTV_MPC.py:396-405), so its QP variable
is ``du' = Tu du`` and its rate cost and rate box are in those units.  That is an exact change of variables of the rate channel, lowered on
the host: the record carries ``w_du Tu^2`` and ``du_lb / Tu``, ``du_ub / Tu``; the caller's ``du_ws`` is divided by ``Tu`` and the returned
``du_pred`` multiplied by it, so ``du_ws`` / ``du_pred`` are in the reference's units; the input cost and the input box are not touched (again
only the ``1e-10 I`` term moves).  ``host_scaling`` does that step; ``check_params`` checks what is left for the device and still refuses
``input_scaling`` itself.  ``q_ref`` must be continuous in ``s`` along the horizon (no wrap at
the start line): the caller's duty, as in the reference, whose ``wrapped_state_idxs`` unwrapping is refused here along with ``delay``,
``soft_constraint_*``, other QP interfaces, code generation, ``reg != 0`` and rate-constraint functions.  A ``u_prev`` beyond an input bound
by more than 1e-12 (relative to max(1, |bound|)) makes every QP infeasible, as in the reference, where ``u_{-1}`` is fixed and bounded;
closer than that -- what the tracker's own saturated output can be -- it is moved onto the bound."""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _ffi
from .solver_types import CALTVMPCParams
from .types import VehiclePrediction, VehicleState


@dataclass
class TrackingCost:
    state_weight: Sequence[float]
    input_weight: Sequence[float] = (0.0, 0.0)
    rate_weight: Sequence[float] = (1.0, 1.0)
    terminal_linear: Optional[Sequence[float]] = None       # c_N (the race demo: -1.0 on s)


@dataclass
class SoftStateBounds:
    idxs: Sequence[int]
    quad: Sequence[float]
    lin: Sequence[float]


@dataclass
class ObstacleAvoidance:
    r: float


@dataclass
class TrackEdgeRows:
    """The track's edges as state constraints of the tracker (margin 0, as the study has them).  Needs a model with (s, e_y) on a track with a
    width table (every spline track; an arc track after ``set_width_table``): the library refuses the rest ("mpc: ...")."""


def check_params(params: CALTVMPCParams) -> None:
    """Everything the device does not implement is refused here, before anything reaches the library.  ``input_scaling`` is among it: the
    callers pass the parameters through ``host_scaling`` first, which lowers it on the host."""
    if params.delay is not None:
        raise NotImplementedError('CA_LTV_MPC: delay (input delay buffers) is not supported')
    if params.wrapped_state_idxs is not None or params.wrapped_state_periods is not None:
        raise NotImplementedError('CA_LTV_MPC: wrapped_state_idxs (state unwrapping) is not supported: pass a q_ref that is continuous in s')
    if params.soft_constraint_idxs is not None or params.soft_constraint_quad is not None or params.soft_constraint_lin is not None:
        raise NotImplementedError('CA_LTV_MPC: soft_constraint_* is not supported (soft_state_bound_* is)')
    if params.qp_interface != 'casadi':
        raise NotImplementedError(f"CA_LTV_MPC: qp_interface {params.qp_interface!r} is not supported (only 'casadi')")
    if params.code_gen or params.jit:
        raise NotImplementedError('CA_LTV_MPC: code_gen / jit are not supported (the solver is a compiled HIP kernel)')
    if params.reg != 0:
        raise NotImplementedError('CA_LTV_MPC: reg != 0 is not supported')
    if params.input_scaling is not None:
        raise NotImplementedError('CA_LTV_MPC: input_scaling is no option of the device record: it is a change of variables of the rate channel '
                                  'that the host applies first (ltv_mpc.host_scaling, as CA_LTV_MPC and mpc_batch do); check the parameters '
                                  'it returns')
    v = params.state_scaling
    if v is not None and not (np.all(np.isfinite(v)) and np.all(np.asarray(v, float) > 0)):
        raise ValueError('CA_LTV_MPC: state_scaling must be positive')


def host_scaling(params: CALTVMPCParams):
    """The host's share of the parameters: ``(device_params, Tu)``.  ``input_scaling`` is taken out -- ``Tu = 1 / input_scaling`` is the factor
    of the rate channel's change of variables that ``lower`` and ``solve_batch`` apply -- and ``device_params`` is what ``check_params``
    sees; ``Tu`` is None without ``input_scaling``."""
    v = params.input_scaling
    if v is None:
        return params, None
    if len(v) != _ffi.NUA:
        raise ValueError('CA_LTV_MPC: input_scaling needs one entry per input')
    if not (np.all(np.isfinite(v)) and np.all(np.asarray(v, float) > 0)):
        raise ValueError('CA_LTV_MPC: input_scaling must be positive')
    return dataclasses.replace(params, input_scaling=None), rate_scale(v)


def rate_scale(input_scaling) -> Optional[np.ndarray]:
    """``Tu = 1 / input_scaling`` (CA_LTV_MPC.py:121), or None: the factor between the reference's rate variable ``du' = Tu du`` and ``du``."""
    return None if input_scaling is None else 1.0 / np.asarray(input_scaling, np.float64)


def lower(agent: int, n_q: int, cost: TrackingCost, soft: Optional[SoftStateBounds], obstacle: Optional[ObstacleAvoidance],
          q_ub, q_lb, u_ub, u_lb, du_ub, du_lb, N: int, qp_iters: int, damping: float, zero_du: bool = False,
          input_scaling=None, track_edges: Optional[TrackEdgeRows] = None) -> _ffi.MpcT:
    """The dgsqp_mpc_t record (validated again by dgsqp_set_mpc).  ``input_scaling``: the rate cost and the rate box are the reference's, in
    its scaled rate ``du' = Tu du``; the record states them for ``du``: ``w_du Tu^2``, ``du_lb / Tu``, ``du_ub / Tu``."""
    if len(cost.state_weight) != n_q:
        raise ValueError(f'TrackingCost.state_weight needs {n_q} entries')
    if cost.terminal_linear is not None and len(cost.terminal_linear) != n_q:
        raise ValueError(f'TrackingCost.terminal_linear needs {n_q} entries')
    if len(cost.input_weight) != _ffi.NUA or len(cost.rate_weight) != _ffi.NUA:
        raise ValueError('TrackingCost.input_weight / rate_weight need one entry per input')
    if not all(float(w) > 0 for w in cost.rate_weight):
        raise ValueError('TrackingCost.rate_weight must be positive for every channel (the QP is solved exactly and must be strictly convex)')
    m = _ffi.MpcT()
    m.agent, m.N, m.qp_iters, m.zero_du, m.damping = int(agent), int(N), int(qp_iters), int(bool(zero_du)), float(damping)
    for i in range(_ffi.MAX_NQA):
        m.w_q[i] = float(cost.state_weight[i]) if i < n_q else 0.0
        m.c_N[i] = float(cost.terminal_linear[i]) if (cost.terminal_linear is not None and i < n_q) else 0.0
        m.q_ub[i] = float(q_ub[i]) if i < n_q else np.inf
        m.q_lb[i] = float(q_lb[i]) if i < n_q else -np.inf
    Tu = rate_scale(input_scaling)
    for j in range(_ffi.NUA):
        t = 1.0 if Tu is None else float(Tu[j])
        m.w_u[j], m.w_du[j] = float(cost.input_weight[j]), float(cost.rate_weight[j]) * t * t
        m.u_ub[j], m.u_lb[j], m.du_ub[j], m.du_lb[j] = float(u_ub[j]), float(u_lb[j]), float(du_ub[j]) / t, float(du_lb[j]) / t
    if soft is not None:
        if not (len(soft.idxs) == len(soft.quad) == len(soft.lin)):
            raise ValueError('soft state bounds: idxs, quad and lin must have the same length')
        if len(soft.idxs) > 1:
            raise NotImplementedError('CA_LTV_MPC: one soft state bound is supported (with more, the reference writes the rows of '
                                      'different states on top of one another, CA_LTV_MPC.py:519-533)')
        m.n_soft = len(soft.idxs)
        for i, (j, qd, ln) in enumerate(zip(soft.idxs, soft.quad, soft.lin)):
            m.soft_idx[i], m.soft_quad[i], m.soft_lin[i] = int(j), float(qd), float(ln)
    m.obs_r = float(obstacle.r) if obstacle is not None else 0.0
    if track_edges is not None and not isinstance(track_edges, TrackEdgeRows):
        raise TypeError('track_edges must be None or a TrackEdgeRows record')
    m.edge_rows = 1 if track_edges is not None else 0
    return m


def _check(lib, h, rc: int, what: str) -> None:
    if rc != 0:
        msg = lib.dgsqp_last_error(h)
        err = {_ffi.E_TOO_LARGE: MemoryError}.get(rc, ValueError if rc == _ffi.E_ARG else RuntimeError)
        raise err(f'{what} failed ({rc}): {msg.decode() if msg else ""}')


def mpc_dims(lib, h) -> dict:
    """n, the row table (kind, stage, index, sign) in the order of the logged multipliers, len_D, n_q of the tracker set on handle h."""
    d = _ffi.MpcDimsT()
    _check(lib, h, lib.dgsqp_mpc_dims(h, C.byref(d), None, 0), 'dgsqp_mpc_dims')
    rows = (_ffi.MpcRowT * max(1, d.n_rows))()
    _check(lib, h, lib.dgsqp_mpc_dims(h, C.byref(d), rows, d.n_rows), 'dgsqp_mpc_dims')
    table = np.array([(r.kind, r.stage, r.index, r.sign) for r in rows[:d.n_rows]], dtype=np.int32).reshape(-1, 4)
    return dict(n=d.n, n_rows=d.n_rows, len_D=d.len_D, n_q=d.n_q, lds_bytes=d.lds_bytes, workspace_bytes=d.workspace_bytes, rows=table)


def run_batch(lib, h, record: _ffi.MpcT, n_q: int, q0, u_ws, du_ws, q_ref, p_obs=None, log: bool = False) -> dict:
    """dgsqp_set_mpc + dgsqp_mpc_batch (+ the log) on handle h.  q0 [B, n_q], u_ws [B, N+1, 2] (row 0 = u_prev), du_ws [B, N, 2],
    q_ref [B, N+1, n_q], p_obs [B, N, 2]."""
    N, nu = int(record.N), _ffi.NUA
    q0 = np.ascontiguousarray(q0, np.float64)
    B = q0.shape[0]
    shapes = dict(q0=(B, n_q), u_ws=(B, N + 1, nu), du_ws=(B, N, nu), q_ref=(B, N + 1, n_q))
    arrs = dict(q0=q0, u_ws=np.ascontiguousarray(u_ws, np.float64), du_ws=np.ascontiguousarray(du_ws, np.float64),
                q_ref=np.ascontiguousarray(q_ref, np.float64))
    for k, shp in shapes.items():
        if arrs[k].shape != shp:
            raise ValueError(f'{k} must have shape {shp}, got {arrs[k].shape}')
    if record.obs_r > 0:
        if p_obs is None:
            raise ValueError('an obstacle row needs p_obs [B, N, 2]')
        p_obs = np.ascontiguousarray(p_obs, np.float64)
        if p_obs.shape != (B, N, 2):
            raise ValueError(f'p_obs must have shape {(B, N, 2)}, got {p_obs.shape}')
    else:
        p_obs = None
    _check(lib, h, lib.dgsqp_set_mpc(h, C.byref(record)), 'dgsqp_set_mpc')
    _check(lib, h, lib.dgsqp_set_mpc_log(h, int(bool(log))), 'dgsqp_set_mpc_log')
    out = dict(q_pred=np.zeros((B, N + 1, n_q)), u_pred=np.zeros((B, N, nu)), du_pred=np.zeros((B, N, nu)),
               status=np.zeros(B, np.int32), qp_steps=np.zeros(B, np.int32))
    tm = _ffi.TimingT()
    rc = lib.dgsqp_mpc_batch(h, B, _ffi.dptr(arrs['q0']), _ffi.dptr(arrs['u_ws']), _ffi.dptr(arrs['du_ws']), _ffi.dptr(arrs['q_ref']),
                             _ffi.dptr(p_obs), _ffi.dptr(out['q_pred']), _ffi.dptr(out['u_pred']), _ffi.dptr(out['du_pred']),
                             _ffi.iptr(out['status']), _ffi.iptr(out['qp_steps']), C.byref(tm))
    _check(lib, h, rc, 'dgsqp_mpc_batch')
    out['success'] = out['status'] == 0
    out['timing'] = dict(h2d_ms=tm.h2d_ms, kernel_ms=tm.kernel_ms, d2h_ms=tm.d2h_ms, total_ms=tm.total_ms, grid=tm.grid, block=tm.block)
    if log and B > 0:
        d = mpc_dims(lib, h)
        it = int(record.qp_iters)
        out['log_D'] = np.zeros((B, it, d['len_D']))
        out['log_D_bar'] = np.zeros((B, it, d['len_D']))
        out['log_lam'] = np.zeros((B, it, d['n_rows']))
        _check(lib, h, lib.dgsqp_fetch_mpc_log(h, _ffi.dptr(out['log_D']), _ffi.dptr(out['log_D_bar']), _ffi.dptr(out['log_lam']), B),
               'dgsqp_fetch_mpc_log')
        out['dims'] = d
    return out


def mpc_batch(solver, agent: int, cost: TrackingCost, bounds: dict, q0, u_ws, du_ws, q_ref, p_obs=None, N: Optional[int] = None,
              qp_iters: int = 2, damping: float = 0.75, soft: Optional[SoftStateBounds] = None,
              obstacle: Optional[ObstacleAvoidance] = None, zero_du: bool = False, log: bool = False, input_scaling=None,
              track_edges: Optional[TrackEdgeRows] = None) -> dict:
    """The tracker for agent ``agent`` of the game of ``solver`` (a ``DGSQP``): its model, vehicle, integrator, dt and track.  ``bounds``:
    ``qu_ub``, ``qu_lb``, ``du_ub``, ``du_lb`` as ``VehicleState`` (the reference's dict).  ``input_scaling`` as in ``CALTVMPCParams``:
    ``du_ws`` and ``du_pred`` are then the reference's scaled rates."""
    mdl = solver.joint_dynamics.dynamics_models[agent] if 0 <= int(agent) < solver.M else None
    if mdl is None:
        raise ValueError(f'agent {agent} is outside the game\'s 0..{solver.M - 1}')
    q_ub, u_ub = mdl.state2qu(bounds['qu_ub'])
    q_lb, u_lb = mdl.state2qu(bounds['qu_lb'])
    _, du_ub = mdl.state2qu(bounds['du_ub'])
    _, du_lb = mdl.state2qu(bounds['du_lb'])
    rec = lower(agent, mdl.n_q, cost, soft, obstacle, q_ub, q_lb, u_ub, u_lb, du_ub, du_lb, solver.N if N is None else N, qp_iters, damping, zero_du,
                input_scaling=input_scaling, track_edges=track_edges)
    Tu = rate_scale(input_scaling)
    out = run_batch(solver._lib, solver._h, rec, mdl.n_q, q0, u_ws, du_ws if Tu is None else np.asarray(du_ws, np.float64) / Tu, q_ref, p_obs, log=log)
    if Tu is not None:
        out['du_pred'] = out['du_pred'] * Tu
    return out


def shift_warm_start(u_pred: np.ndarray, du_pred: np.ndarray):
    """step()'s warm start for the next call (CA_LTV_MPC.py:219-222): u_ws [N+1, n_u] whose row 0 -- the next u_prev -- is the input
    just applied, du_ws shifted by one stage; both repeat their last row."""
    return np.vstack((u_pred, u_pred[-1])), np.vstack((du_pred[1:], du_pred[-1]))


class CA_LTV_MPC:
    """The reference's class surface.  ``costs``: a ``TrackingCost``; ``constraints``: ``None``, an ``ObstacleAvoidance`` or a dict with
    the keys ``'obstacle'`` and ``'track_edges'`` (a ``TrackEdgeRows``); ``bounds``: the reference's dict of ``VehicleState`` (``qu_ub``, ``qu_lb``, ``du_ub``, ``du_lb``).
    ``parameters`` of ``solve`` / ``step`` / ``set_warm_start`` is the reference's ``P`` tail: ``q_ref.ravel()`` ([N+1, n_q]) followed by
    ``p_obs.ravel()`` ([N, 2]) when there is an obstacle row."""

    def __init__(self, dynamics, costs: TrackingCost, constraints, bounds: dict, control_params: CALTVMPCParams = None, print_method=print,
                 device: int = 0, workgroups_per_cu: int = 1):
        params = control_params if control_params is not None else CALTVMPCParams()
        check_params(host_scaling(params)[0])
        self.track_edges = None
        if isinstance(constraints, dict):
            if constraints.get('rate') is not None and any(c is not None for c in np.atleast_1d(np.asarray(constraints['rate'], dtype=object))):
                raise NotImplementedError('CA_LTV_MPC: rate-constraint functions are not supported (the rate box is)')
            extra = set(constraints) - {'obstacle', 'rate', 'state_input', 'track_edges'}
            if extra:
                raise NotImplementedError(f'CA_LTV_MPC: unknown constraint entries {sorted(extra)}')
            si = constraints.get('state_input')
            if si is not None and any(c is not None for c in np.atleast_1d(np.asarray(si, dtype=object))):
                raise NotImplementedError("CA_LTV_MPC: 'state_input' functions are not supported: pass ObstacleAvoidance under 'obstacle', "
                                          "TrackEdgeRows under 'track_edges'")
            track_edges = constraints.get('track_edges')
            if track_edges is not None and not isinstance(track_edges, TrackEdgeRows):
                raise NotImplementedError("CA_LTV_MPC: 'track_edges' must be None or a TrackEdgeRows record")
            if track_edges is not None and not (hasattr(dynamics, 's_idx') and hasattr(dynamics, 'ey_idx')):
                raise ValueError('CA_LTV_MPC: TrackEdgeRows needs a model with (s, e_y)')
            if track_edges is not None and (getattr(dynamics, 'track', None) is None or dynamics.track.width_table() is None):
                raise ValueError('CA_LTV_MPC: TrackEdgeRows needs a track with a width table (a spline track, or set_width_table)')
            self.track_edges = track_edges
            constraints = constraints.get('obstacle')
        if constraints is not None and not isinstance(constraints, ObstacleAvoidance):
            raise NotImplementedError('CA_LTV_MPC: constraints must be None or an ObstacleAvoidance record')
        if not isinstance(costs, TrackingCost):
            raise NotImplementedError('CA_LTV_MPC: costs must be a TrackingCost record (CasADi functions cannot be lowered)')
        self.dynamics, self.dt, self.costs, self.constraints = dynamics, dynamics.dt, costs, constraints
        self.print_method = (lambda s: None) if print_method is None else print_method
        self.n_u, self.n_q = dynamics.n_u, dynamics.n_q
        self.n_z = self.n_q + self.n_u
        self.N, self.damping, self.qp_iters = int(params.N), float(params.damping), int(params.qp_iters)
        self.params = params
        self.soft = None
        if params.soft_state_bound_idxs is not None:
            self.soft = SoftStateBounds(list(params.soft_state_bound_idxs), list(params.soft_state_bound_quad), list(params.soft_state_bound_lin))
        self.state_ub, self.input_ub = dynamics.state2qu(bounds['qu_ub'])
        self.state_lb, self.input_lb = dynamics.state2qu(bounds['qu_lb'])
        _, self.input_rate_ub = dynamics.state2qu(bounds['du_ub'])
        _, self.input_rate_lb = dynamics.state2qu(bounds['du_lb'])
        self._record(self.qp_iters, self.damping, False)          # every refusal of the record, before a handle exists
        self._solver = self._one_agent_solver(dynamics, bounds, device, workgroups_per_cu)
        self.q_pred = np.zeros((self.N + 1, self.n_q))
        self.u_pred = np.zeros((self.N, self.n_u))
        self.du_pred = np.zeros((self.N, self.n_u))
        self.u_prev = np.zeros(self.n_u)
        self.u_ws = np.zeros((self.N + 1, self.n_u))
        self.du_ws = np.zeros((self.N, self.n_u))
        self.initialized = False
        self.t = 0
        self.state_input_prediction = None

    def _one_agent_solver(self, dynamics, bounds, device, workgroups_per_cu):
        """A one-agent game around ``dynamics``, built with the package's own constructors: the handle the tracker runs on."""
        from .dynamics import CasadiDecoupledMultiAgentDynamicsModel, MultiAgentModelConfig
        from .game import RacingCost
        from .solver import DGSQP
        from .solver_types import DGSQPParams
        cfg = dynamics.model_config
        joint = CasadiDecoupledMultiAgentDynamicsModel(dynamics.t0, [dynamics], MultiAgentModelConfig(
            dt=cfg.dt, discretization_method=cfg.discretization_method, M=cfg.M, use_mx=True, code_gen=False, verbose=False))
        cost = RacingCost(input_weight=(1.0, 1.0), input_rate_weight=(1.0, 1.0), comp_weights=(1.0, 0.0), comp_type='atan',
                          blocking_weight=0, obs_weight=0, obs_r=0.0)
        return DGSQP(joint, [cost], [None], None, dict(ub=[bounds['qu_ub']], lb=[bounds['qu_lb']]),
                     DGSQPParams(dt=cfg.dt, N=min(self.N, 8)), print_method=None, device=device, workgroups_per_cu=workgroups_per_cu)

    def _record(self, qp_iters: int, damping: float, zero_du: bool) -> _ffi.MpcT:
        return lower(0, self.n_q, self.costs, self.soft, self.constraints, self.state_ub, self.state_lb, self.input_ub, self.input_lb,
                     self.input_rate_ub, self.input_rate_lb, self.N, qp_iters, damping, zero_du, input_scaling=self.params.input_scaling,
                     track_edges=self.track_edges)

    def initialize(self) -> None:
        return

    def _split(self, parameters):
        p = np.asarray(parameters, np.float64).ravel()
        nq = (self.N + 1) * self.n_q
        want = nq + (2 * self.N if self.constraints is not None else 0)
        if p.size != want:
            raise ValueError(f'parameters must hold q_ref.ravel() ({nq})' + (f' and p_obs.ravel() ({2 * self.N})' if self.constraints is not None else '')
                             + f': got {p.size}')
        return p[:nq].reshape(1, self.N + 1, self.n_q), (p[nq:].reshape(1, self.N, 2) if self.constraints is not None else None)

    def solve_batch(self, q0, u_ws, du_ws, q_ref, p_obs=None, log: bool = False, qp_iters: Optional[int] = None,
                    damping: Optional[float] = None, zero_du: bool = False) -> dict:
        """Many scenarios in one launch: q0 [B, n_q], u_ws [B, N+1, n_u] (row 0 = u_prev), du_ws [B, N, n_u], q_ref [B, N+1, n_q],
        p_obs [B, N, 2].  Returns q_pred, u_pred, du_pred, status (0 or 4 = 'qp_fail': the outputs are then the warm start), success,
        qp_steps, timing."""
        rec = self._record(self.qp_iters if qp_iters is None else qp_iters, self.damping if damping is None else damping, zero_du)
        Tu = rate_scale(self.params.input_scaling)
        if Tu is None:
            return run_batch(self._solver._lib, self._solver._h, rec, self.n_q, q0, u_ws, du_ws, q_ref, p_obs, log=log)
        # du_ws and du_pred are the reference's scaled rates du' = Tu du; the device works in du
        out = run_batch(self._solver._lib, self._solver._h, rec, self.n_q, q0, u_ws, np.asarray(du_ws, np.float64) / Tu, q_ref, p_obs, log=log)
        out['du_pred'] = out['du_pred'] * Tu
        return out

    def set_warm_start(self, u_ws: np.ndarray, du_ws: np.ndarray, state: VehicleState = None, parameters: np.ndarray = np.array([]),
                       l_ws: np.ndarray = None) -> None:
        self.u_ws = np.asarray(u_ws, np.float64)
        self.u_prev = self.u_ws[0]
        self.du_ws = np.asarray(du_ws, np.float64)
        if l_ws is not None:
            self.l_ws = l_ws
        # (the reference sets ``initalized`` -- misspelt -- so this loop runs on every call that passes a state, CA_LTV_MPC.py:166, :203)
        if not self.initialized and state:
            q0, _ = self.dynamics.state2qu(state)
            q_ref, p_obs = self._split(parameters)
            out = self.solve_batch(q0[None], self.u_ws[None], self.du_ws[None], q_ref, p_obs, qp_iters=2, damping=0.5, zero_du=True)
            if not out['success'][0]:
                self.print_method('QP returned qp_fail')
            self.q_pred = out['q_pred'][0]
            self.u_ws = np.vstack((self.u_ws[:1], out['u_pred'][0]))
            self.du_ws = out['du_pred'][0]
            self.u_pred = self.u_ws[1:]
            self.du_pred = self.du_ws
            self.initalized = True

    def solve(self, state: VehicleState, parameters: np.ndarray = np.array([])) -> bool:
        q0, _ = self.dynamics.state2qu(state)
        q_ref, p_obs = self._split(parameters)
        out = self.solve_batch(q0[None], self.u_ws[None], self.du_ws[None], q_ref, p_obs)
        success = bool(out['success'][0])
        if not success:
            self.print_method('Warning: QP returned qp_fail')
        self.q_pred, self.u_pred, self.du_pred = out['q_pred'][0], out['u_pred'][0], out['du_pred'][0]
        return success

    def step(self, vehicle_state: VehicleState, parameters: np.ndarray = np.array([])) -> None:
        self.t = vehicle_state.t
        self.solve(vehicle_state, parameters)
        u = self.u_pred[0]
        self.dynamics.qu2state(vehicle_state, None, u)
        u_ws, du_ws = shift_warm_start(self.u_pred, self.du_pred)
        self.set_warm_start(u_ws, du_ws)

    def get_prediction(self) -> VehiclePrediction:
        if self.state_input_prediction is None:
            self.state_input_prediction = VehiclePrediction()
        self.state_input_prediction.t = self.t
        self.dynamics.qu2prediction(self.state_input_prediction, self.q_pred, self.u_pred)
        return self.state_input_prediction
