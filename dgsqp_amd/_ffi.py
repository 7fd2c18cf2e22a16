"""ctypes mirror of include/dgsqp.h and the loader of the HIP library.

There is deliberately no CPU fallback: if ``libdgsqp_hip.so`` is missing or
cannot be loaded, ``load_library()`` raises."""
from __future__ import annotations

import ctypes as C
import os
import pathlib

MAX_KNOTS = 1152
MAX_AGENTS = 6
MAX_SEGS = 16
MAX_NQA = 8
MAX_LANES = 2
NUA = 2
# DGSQP_MODEL_*: vehicle model ids (include/dgsqp.h)
MODEL_KIN_BICYCLE, MODEL_DYN_BICYCLE, MODEL_UNICYCLE, MODEL_UNICYCLE_COMBINED = 0, 1, 2, 3
MAX_DELAY = 16       # DGSQP_MAX_DELAY: longest input delay line of a closed-loop plant, in simulation steps

STATUS_MSG = ['conv_abs_tol', 'conv_rel_tol', 'max_it', 'diverged', 'qp_fail', 'time_limit']
NOT_RUN = -1         # DGSQP_NOT_RUN: a closed-loop step that never ran (step_batch reports it as 'not_run')
HELD = -2            # DGSQP_HELD: a closed-loop step that followed the plan it held and did not solve ('held')
STATUS_NAMES = {**dict(enumerate(STATUS_MSG)), NOT_RUN: 'not_run', HELD: 'held'}

dbl2 = C.c_double * NUA


class LaneT(C.Structure):
    _fields_ = [('brk', C.c_double), ('n_lo', dbl2), ('n_hi', dbl2), ('anchor', dbl2), ('r', C.c_double)]


class AgentT(C.Structure):
    _fields_ = [
        ('model', C.c_int32), ('tire_model', C.c_int32), ('drive_wheels', C.c_int32), ('simple_slip', C.c_int32),
        ('L_f', C.c_double), ('L_r', C.c_double), ('mass', C.c_double), ('I_z', C.c_double), ('gravity', C.c_double),
        ('c_dr', C.c_double), ('c_da', C.c_double), ('c_s', C.c_double), ('c_r', C.c_double), ('p_r', C.c_double),
        ('pac_Bf', C.c_double), ('pac_Br', C.c_double), ('pac_Cf', C.c_double), ('pac_Cr', C.c_double),
        ('pac_Df', C.c_double), ('pac_Dr', C.c_double), ('lin_Bf', C.c_double), ('lin_Br', C.c_double),
        ('w_in', dbl2), ('w_rate', dbl2), ('w_prog', C.c_double), ('w_comp', C.c_double),
        ('comp_type', C.c_int32), ('_pad0', C.c_int32),
        ('w_block', C.c_double), ('w_obs', C.c_double), ('obs_cost_r', C.c_double),
        ('has_rate', C.c_int32), ('_pad1', C.c_int32),
        ('rate_ub', dbl2), ('rate_lb', dbl2), ('in_ub', dbl2), ('in_lb', dbl2),
        ('st_ub', C.c_double * MAX_NQA), ('st_lb', C.c_double * MAX_NQA),
        ('radius', C.c_double),
        ('w_goal', C.c_double * MAX_NQA), ('goal', C.c_double * MAX_NQA), ('goal_term_mult', C.c_double),
        ('n_lane', C.c_int32), ('_pad2', C.c_int32), ('lane', LaneT * MAX_LANES),
        ('edge_rows', C.c_int32), ('_pad3', C.c_int32), ('edge_margin', C.c_double),
    ]


class ProblemT(C.Structure):
    _fields_ = [
        ('M', C.c_int32), ('N', C.c_int32), ('integrator', C.c_int32), ('substeps', C.c_int32),
        ('dt', C.c_double),
        ('n_segs', C.c_int32), ('obstacle_rows', C.c_int32),
        ('track_L', C.c_double),
        ('seg_s', C.c_double * (MAX_SEGS + 1)), ('seg_curv', C.c_double * MAX_SEGS),
        ('seg_ang', C.c_double * (MAX_SEGS + 1)),
        ('agents', AgentT * MAX_AGENTS),
        ('track_kind', C.c_int32), ('n_knots', C.c_int32), ('spline', C.c_uint64),     # const double*: kept as an integer so that the POD stays copyable / picklable
        ('n_width', C.c_int32), ('_pad_w', C.c_int32), ('widths', C.c_uint64),         # track width table [n_width][3] (knot, left, right); 0: none
    ]


class ParamsT(C.Structure):
    _fields_ = [
        ('beta', C.c_double), ('tau', C.c_double), ('p_tol', C.c_double), ('d_tol', C.c_double), ('reg', C.c_double),
        ('line_search_iters', C.c_int32), ('nonmono_ls', C.c_int32), ('sqp_iters', C.c_int32),
        ('merit_function', C.c_int32), ('rel_tol_req', C.c_int32), ('lsqr_iter_lim', C.c_int32),
        ('lsqr_atol', C.c_double), ('lsqr_btol', C.c_double),
        ('qp_warm_start', C.c_int32), ('hessian_bfgs', C.c_int32),
        ('eig_floor', C.c_double), ('time_limit', C.c_double),
        ('snap_active_bounds', C.c_int32), ('variant', C.c_int32),
        ('nms', C.c_int32), ('nms_frequency', C.c_int32), ('nms_memory_size', C.c_int32), ('merit_decrease_condition', C.c_int32),
        ('qp_method', C.c_int32), ('osqp_rho_carry', C.c_int32), ('mixed_precision', C.c_int32), ('reserved_', C.c_int32),
        ('reg_decay', C.c_double), ('delta_decay', C.c_double), ('merit_decrease', C.c_double), ('merit_parameter', C.c_double),
    ]


class PlantT(C.Structure):
    """dgsqp_plant_t: the plant of closed-loop launches (closed_loop.PlantModel lowers to it)."""
    _fields_ = [('integrator', C.c_int32), ('substeps', C.c_int32), ('sim_steps', C.c_int32), ('use_game_agents', C.c_int32),
                ('delay', (C.c_int32 * NUA) * MAX_AGENTS), ('agents', AgentT * MAX_AGENTS)]


class VehicleT(C.Structure):
    """dgsqp_vehicle_t: the vehicle fields of dgsqp_agent_t (model .. lin_Br), one per chain and agent of a plant ensemble."""
    _fields_ = AgentT._fields_[:22]


class PidT(C.Structure):
    _fields_ = [
        ('kp_v', C.c_double), ('kp_s', C.c_double), ('ki_s', C.c_double), ('ey_gain', C.c_double), ('ei_max', C.c_double),
        ('u_max', C.c_double * 2), ('du_max', C.c_double * 2), ('substeps', C.c_int32), ('reserved_', C.c_int32),
    ]


class DriversT(C.Structure):
    """dgsqp_drivers_t: who produces each agent's command in closed-loop launches (closed_loop.Drivers lowers to it)."""
    _fields_ = [('kind', C.c_int32 * MAX_AGENTS), ('pid', PidT * MAX_AGENTS)]


DRIVER_GAME, DRIVER_PID, DRIVER_REPLAY, DRIVER_TRACK = 0, 1, 2, 3        # DGSQP_DRIVER_*


class HoldT(C.Structure):
    """dgsqp_hold_t: the planning rate and the fallback of closed-loop launches that hold a plan (closed_loop.PlanHold lowers to it)."""
    _fields_ = [('replan_every', C.c_int32), ('on_fail', C.c_int32), ('fail_mask', C.c_uint32), ('reserved', C.c_int32)]


HOLD_REFERENCE, HOLD_HOLD = 0, 1                        # DGSQP_HOLD_*


class StatRecordT(C.Structure):
    _fields_ = [('status', C.c_int32), ('iters', C.c_int32), ('qp_solves', C.c_int32), ('rank', C.c_int32),
                ('p_feas', C.c_double), ('comp', C.c_double), ('stat', C.c_double), ('cost', C.c_double * MAX_AGENTS)]


class DimsT(C.Structure):
    _fields_ = [('M', C.c_int32), ('N', C.c_int32), ('n_q', C.c_int32), ('n_u', C.c_int32), ('n', C.c_int32),
                ('n_c', C.c_int32), ('n_dense', C.c_int32), ('lds_bytes', C.c_int32),
                ('workspace_bytes', C.c_int64), ('layout', C.c_int32), ('reserved_', C.c_int32)]


class TimingT(C.Structure):
    _fields_ = [('h2d_ms', C.c_double), ('kernel_ms', C.c_double), ('d2h_ms', C.c_double), ('total_ms', C.c_double),
                ('grid', C.c_int32), ('block', C.c_int32)]


class MpcT(C.Structure):
    """dgsqp_mpc_t: the reference tracker's record (ltv_mpc.CA_LTV_MPC lowers to it)."""
    _fields_ = [('agent', C.c_int32), ('N', C.c_int32), ('qp_iters', C.c_int32), ('zero_du', C.c_int32), ('damping', C.c_double),
                ('w_q', C.c_double * MAX_NQA), ('c_N', C.c_double * MAX_NQA), ('w_u', dbl2), ('w_du', dbl2),
                ('q_ub', C.c_double * MAX_NQA), ('q_lb', C.c_double * MAX_NQA), ('u_ub', dbl2), ('u_lb', dbl2), ('du_ub', dbl2), ('du_lb', dbl2),
                ('n_soft', C.c_int32), ('edge_rows', C.c_int32), ('soft_idx', C.c_int32 * MAX_NQA),
                ('soft_quad', C.c_double * MAX_NQA), ('soft_lin', C.c_double * MAX_NQA), ('obs_r', C.c_double)]


class MpcRowT(C.Structure):
    _fields_ = [('kind', C.c_int32), ('stage', C.c_int32), ('index', C.c_int32), ('sign', C.c_int32)]


class MpcDimsT(C.Structure):
    _fields_ = [('n', C.c_int32), ('n_rows', C.c_int32), ('len_D', C.c_int32), ('n_q', C.c_int32), ('lds_bytes', C.c_int32),
                ('reserved_', C.c_int32), ('workspace_bytes', C.c_int64)]


RL_COLS = 9          # DGSQP_RL_COLS: columns of the raceline table (x, y, psi, v_long, v_tran, psidot, e_psi, s, e_y)


class RacelineWsT(C.Structure):
    """dgsqp_raceline_ws_t: the warm-start program of warm_start_dynamic.py (montecarlo.raceline_ws lowers to it)."""
    _fields_ = [('mpc', MpcT), ('u_init', C.c_double), ('du_init', C.c_double), ('init_iters', C.c_int32), ('reserved_', C.c_int32),
                ('init_damping', C.c_double)]


class RacelineSamplerT(C.Structure):
    """dgsqp_raceline_sampler_t: the placement of monte_carlo_sampler_dynamic.py (sampler.raceline_sampler_spec fills it)."""
    _fields_ = [('n_key', C.c_int32), ('reserved_', C.c_int32), ('seed', C.c_uint64), ('half_width', C.c_double), ('obs_d', C.c_double),
                ('collision_d', C.c_double), ('key_pts', (C.c_double * 6) * (MAX_SEGS + 1))]


class RacelineSplineSamplerT(C.Structure):
    """dgsqp_raceline_spline_sampler_t: the placement of comparison_study_f1/monte_carlo_sampler.py (sampler.raceline_spline_sampler_spec)."""
    _fields_ = [('seed', C.c_uint64), ('s_lo', C.c_double), ('s_hi', C.c_double), ('gap_lo', C.c_double), ('gap_hi', C.c_double),
                ('ey_clip', C.c_double), ('collision_d', C.c_double)]


class TrackFrameT(C.Structure):
    """dgsqp_track_frame_t: the track of the batched frame transforms (tracks.track_frame_spec fills it); n_key = 0: the handle's spline."""
    _fields_ = [('n_key', C.c_int32), ('_pad', C.c_int32), ('half_width', C.c_double), ('slack', C.c_double),
                ('key_pts', (C.c_double * 6) * (MAX_SEGS + 1))]


MPC_ROW_RATE, MPC_ROW_SLACK, MPC_ROW_INPUT, MPC_ROW_STATE, MPC_ROW_SOFT, MPC_ROW_OBS, MPC_ROW_EDGE = range(7)     # DGSQP_MPC_ROW_*
MPC_NMAX = 128                                                                                      # DGSQP_MPC_NMAX
E_ARG, E_DEVICE, E_NOMEM, E_TOO_LARGE = -1, -2, -3, -4                                              # DGSQP_E_*

_PD = C.POINTER(C.c_double)
_PI = C.POINTER(C.c_int32)
_PF = C.POINTER(C.c_float)
_PU64 = C.POINTER(C.c_uint64)
_H = C.c_void_p
_TM = C.POINTER(TimingT)

# The C-ABI of include/dgsqp.h, stated once: name -> (restype, argtypes).  load_library applies it; EXPORTED_SYMBOLS is its key list.
SIGNATURES = {
    'dgsqp_create': (C.c_int, [C.POINTER(ProblemT), C.POINTER(ParamsT), C.c_int, C.POINTER(_H)]),
    'dgsqp_destroy': (None, [_H]),
    'dgsqp_dims': (C.c_int, [_H, C.POINTER(DimsT)]),
    'dgsqp_plan': (C.c_int, [C.POINTER(ProblemT), C.POINTER(ParamsT), C.POINTER(DimsT), C.c_char_p, C.c_int]),
    'dgsqp_last_error': (C.c_char_p, [_H]),
    'dgsqp_backend_info': (C.c_int, [C.c_char_p, C.c_int]),
    'dgsqp_solve_batch': (C.c_int, [_H, C.c_int64, _PD, _PD, _PD, _PD, _PD, _PI, _PI, _PI, _PD, _PD, _TM]),
    'dgsqp_solve_batch_f32': (C.c_int, [_H, C.c_int64, _PF, _PF, _PF, _PF, _PF, _PI, _PI, _PI, _PF, _PF, _TM]),
    'dgsqp_closed_loop_batch': (C.c_int, [_H, C.c_int64, C.c_int32, _PD, _PD, _PD, _PD, _PD, _PD, _PD, _PD, _PI, _PI, _PI, _PD, _PD, _PI, _TM]),
    'dgsqp_set_plant': (C.c_int, [_H, C.POINTER(PlantT)]),
    'dgsqp_fetch_u_plant': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_set_plant_ensemble': (C.c_int, [_H, C.c_int64, C.POINTER(VehicleT), _PI]),
    'dgsqp_set_estimate_noise': (C.c_int, [_H, C.c_int32, C.c_int64, _PD]),
    'dgsqp_fetch_q_est': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_set_monitor': (C.c_int, [_H, C.c_int]),
    'dgsqp_fetch_monitor': (C.c_int, [_H, _PD, _PD, _PI]),
    'dgsqp_set_drivers': (C.c_int, [_H, C.POINTER(DriversT), C.c_int32, C.c_int64, _PI, _PD, _PD]),
    'dgsqp_fetch_u_cmd': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_set_plan_hold': (C.c_int, [_H, C.POINTER(HoldT)]),
    'dgsqp_fetch_plan_hold': (C.c_int, [_H, _PD, _PI, C.c_int64]),
    'dgsqp_set_cross_plant': (C.c_int, [_H, C.POINTER(PlantT), C.c_int64, _PD]),
    'dgsqp_fetch_plant_state': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_fetch_track_ref': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_set_u_prev': (C.c_int, [_H, C.c_int64, _PD]),
    'dgsqp_set_closed_loop_u_prev': (C.c_int, [_H, C.c_int, C.c_int64, _PD]),
    'dgsqp_fetch_u_prev': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_stage_inputs': (C.c_int, [_H, C.c_int64, _PD, _PD]),
    'dgsqp_solve_staged': (C.c_int, [_H, _TM]),
    'dgsqp_launch_staged': (C.c_int, [_H]),
    'dgsqp_launch_staged_group': (C.c_int, [C.POINTER(_H), C.c_int]),
    'dgsqp_draining': (C.c_int, [_H]),
    'dgsqp_finished': (C.c_int, [_H]),
    'dgsqp_wait': (C.c_int, [_H, _TM]),
    'dgsqp_synchronize': (C.c_int, [_H]),
    'dgsqp_fetch_results': (C.c_int, [_H, _PD, _PD, _PD, _PI, _PI, _PI, _PD, _PD]),
    'dgsqp_evaluate_batch': (C.c_int, [_H, C.c_int64, _PD, _PD, _PD, _PD, _PD, _PD, _PD, _PD, _PD]),
    'dgsqp_qp_batch': (C.c_int, [_H, C.c_int64, _PD, _PD, _PD, _PD, _PD, _PD, _PI]),
    'dgsqp_qp_batch_info': (C.c_int, [_H, C.c_int64, _PD, _PD, _PD, _PD, _PD, _PD, _PI, _PD]),
    'dgsqp_pid_warm_start_batch': (C.c_int, [_H, C.c_int64, _PD, C.POINTER(PidT), _PD, _PD, _PI]),
    'dgsqp_sample_batch': (C.c_int, [_H, C.c_int64, C.c_void_p, C.POINTER(PidT), _PD, _PD, C.POINTER(C.c_int64), C.c_int]),
    'dgsqp_set_trace': (C.c_int, [_H, C.c_int]),
    'dgsqp_fetch_trace': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_set_iterate_log': (C.c_int, [_H, C.c_int]),
    'dgsqp_fetch_iterate_log': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_set_cooperative': (C.c_int, [_H, C.c_int]),
    'dgsqp_coop_stats': (C.c_int, [_H, _PU64]),
    'dgsqp_osqp_counters': (C.c_int, [_H, _PU64, C.c_int]),
    'dgsqp_set_deferral': (C.c_int, [_H, C.c_int32, C.c_double]),
    'dgsqp_reserve_deferral': (C.c_int, [_H, C.c_int64]),
    'dgsqp_deferral_stats': (C.c_int, [_H, _PU64]),
    'dgsqp_deferral_log': (C.c_int, [_H, _PU64, C.c_int64]),
    'dgsqp_comm_unique_id': (C.c_int, [C.c_char_p]),
    'dgsqp_comm_init': (C.c_int, [_H, C.c_char_p, C.c_int, C.c_int]),
    'dgsqp_comm_destroy': (C.c_int, [_H]),
    'dgsqp_gather_stats': (C.c_int, [_H, C.c_int64, C.c_void_p]),
    'dgsqp_comm_barrier': (C.c_int, [_H]),
    'dgsqp_comm_allreduce_max': (C.c_int, [_H, _PD, C.c_int]),
    'dgsqp_set_mpc': (C.c_int, [_H, C.POINTER(MpcT)]),
    'dgsqp_mpc_dims': (C.c_int, [_H, C.POINTER(MpcDimsT), C.POINTER(MpcRowT), C.c_int64]),
    'dgsqp_mpc_batch': (C.c_int, [_H, C.c_int64, _PD, _PD, _PD, _PD, _PD, _PD, _PD, _PD, _PI, _PI, _TM]),
    'dgsqp_set_mpc_log': (C.c_int, [_H, C.c_int]),
    'dgsqp_fetch_mpc_log': (C.c_int, [_H, _PD, _PD, _PD, C.c_int64]),
    'dgsqp_set_raceline': (C.c_int, [_H, C.c_int64, _PD, _PD]),
    'dgsqp_raceline_warm_start_batch': (C.c_int, [_H, C.c_int64, _PD, C.POINTER(RacelineWsT), _PD, _PI]),
    'dgsqp_fetch_raceline_ref': (C.c_int, [_H, _PD, C.c_int64]),
    'dgsqp_sample_raceline_batch': (C.c_int, [_H, C.c_int64, C.POINTER(RacelineSamplerT), C.POINTER(RacelineWsT), _PD, _PD,
                                              C.POINTER(C.c_int64), C.c_int]),
    'dgsqp_set_raceline_clip': (C.c_int, [_H, C.c_int, C.c_double]),
    'dgsqp_sample_raceline_spline_batch': (C.c_int, [_H, C.c_int64, C.POINTER(RacelineSplineSamplerT), C.POINTER(RacelineWsT), _PD, _PD,
                                                     C.POINTER(C.c_int64), C.c_int]),
    'dgsqp_local_to_global_batch': (C.c_int, [_H, C.c_int64, C.POINTER(TrackFrameT), _PD, _PD]),
    'dgsqp_global_to_local_batch': (C.c_int, [_H, C.c_int64, C.POINTER(TrackFrameT), _PD, _PD, _PD, _PI]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)

_LIB = None
_LIBS = {}          # workgroups per CU -> CDLL (1: the product build; 2: libdgsqp_hip_b256.so, 256-thread workgroups and half the LDS arena)


def library_path(workgroups_per_cu: int = 1) -> pathlib.Path:
    env = os.environ.get('DGSQP_HIP_LIB')
    if env:
        return pathlib.Path(env)
    name = {1: 'libdgsqp_hip.so', 2: 'libdgsqp_hip_b256.so'}[int(workgroups_per_cu)]
    return pathlib.Path(__file__).resolve().parent / 'csrc' / name


def load_library(workgroups_per_cu: int = 1) -> C.CDLL:
    """Load the HIP solver library; raise loudly if it is absent (no CPU fallback).  ``workgroups_per_cu=2`` loads the build with
    256-thread workgroups, two per CU (row N1: large batches of n <= 64 games; the two libraries can live in one process)."""
    global _LIB
    if int(workgroups_per_cu) not in (1, 2):
        raise ValueError('workgroups_per_cu: 1 (the product build) or 2 (libdgsqp_hip_b256.so)')
    if int(workgroups_per_cu) in _LIBS:
        return _LIBS[int(workgroups_per_cu)]
    path = library_path(workgroups_per_cu)
    if not path.exists():
        raise RuntimeError(f'HIP solver library {path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           f'(hipcc --offload-arch=gfx950). There is no CPU fallback.')
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIBS[int(workgroups_per_cu)] = lib
    if int(workgroups_per_cu) == 1:
        _LIB = lib
    return lib


def dptr(a):
    return None if a is None else a.ctypes.data_as(_PD)


def iptr(a):
    return None if a is None else a.ctypes.data_as(_PI)
