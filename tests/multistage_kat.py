"""Shared helper of the multi-stage known-answer tests (tests/golden/multistage_<case>.npz, written by tools/make_multistage_kats.py:
x, g, q, G, Q of ``_evaluate`` from plain 60-digit functions of the input sequence and central differences -- independent of oracle/
and of dgsqp_amd/csrc).  Loads a fixture, builds the game of the case from the package's public constructors, asserts that this game
has exactly the parameters the answers were computed with, and compares an evaluation with the answers.

Bars (relative to the largest entry of each array): the project's own -- oracle 1e-12, device 1e-11 --
or 64 x the fixture's sensitivity of the quantity where that is larger (the sensitivity is the relative change of the exact answer
under 2^-53 relative perturbations of x0 and u: the floor of ANY fp64 evaluation, computed from the reference side alone); x
elementwise at rtol 1e-13, atol 1e-14 as in test_one_stage_game_hessian_from_sympy_tensors."""
import dataclasses
import pathlib

import numpy as np

GOLD = pathlib.Path(__file__).resolve().parent / 'golden'

SMALL_CASES = ('kin2_euler_N3', 'kin2_rk4_N4', 'kin3_euler_N3', 'dyn2_rk4m3_N3', 'dyn2_rk4m10_N2', 'dyn2_rk3_N3', 'dyn2_rk2_lin_N3', 'uni3_merge_N3')
DIRECTIONAL_CASES = {'kin3_N20_dir': 1, 'kin3_N25_dir': 2}          # case -> the device layout it is there for (1 big, 2 XL)
CASES = SMALL_CASES + tuple(DIRECTIONAL_CASES)

ORACLE_BAR, DEVICE_BAR, X_RTOL, X_ATOL = 1e-12, 1e-11, 1e-13, 1e-14


def _with_integrator(base, method, substeps, **over):
    from dgsqp_amd.dynamics import CasadiDecoupledMultiAgentDynamicsModel
    models = [type(m)(0, dataclasses.replace(m.model_config, discretization_method=method, M=substeps, **over), track=base.track)
              for m in base.joint_model.dynamics_models]
    joint = CasadiDecoupledMultiAgentDynamicsModel(0, models, dataclasses.replace(base.joint_model.model_config, discretization_method=method, M=substeps))
    return dataclasses.replace(base, joint_model=joint)


def build_game(case):
    from dgsqp_amd.game import RacingCost
    from dgsqp_amd.montecarlo import dynamic_racing_game, kinematic_racing_game, merge_game
    if case == 'kin2_euler_N3':
        return kinematic_racing_game('curve', N=3)
    if case == 'kin2_rk4_N4':
        g = _with_integrator(kinematic_racing_game('chicane', N=4), 'rk4', 2)
        cost = lambda: RacingCost(input_weight=(1.0, 1.0), input_rate_weight=(1.0, 1.0), comp_weights=(10.0, 5.0), comp_type='linear',
                                  blocking_weight=0.7, obs_weight=3.0, obs_r=0.9)
        return dataclasses.replace(g, costs=[cost(), cost()])
    if case == 'kin3_euler_N3':
        return kinematic_racing_game('curve', N=3, M=3)
    if case == 'dyn2_rk4m3_N3':
        return dynamic_racing_game(N=3, rk4_substeps=3)
    if case == 'dyn2_rk4m10_N2':
        return dynamic_racing_game(N=2, rk4_substeps=10)
    if case == 'dyn2_rk3_N3':
        return _with_integrator(dynamic_racing_game(N=3, rk4_substeps=4), 'rk3', 4)
    if case == 'dyn2_rk2_lin_N3':
        return _with_integrator(dynamic_racing_game(N=3, rk4_substeps=2), 'rk2', 2, tire_model='linear', simple_slip=True, drive_wheels='rear')
    if case == 'uni3_merge_N3':
        return merge_game(N=3, M=3)
    if case in DIRECTIONAL_CASES:
        return kinematic_racing_game('curve', N={'kin3_N20_dir': 20, 'kin3_N25_dir': 25}[case], M=3)
    raise ValueError(case)


_VEHICLE_FIELDS = {'wheel_dist_front': 'L_f', 'wheel_dist_rear': 'L_r', 'mass': 'mass', 'drag_coefficient': 'c_dr', 'damping_coefficient': 'c_da',
                   'slip_coefficient': 'c_s', 'rolling_resistance': 'c_r', 'rolling_resistance_exponent': 'p_r', 'yaw_inertia': 'I_z', 'gravity': 'gravity',
                   'simple_slip': 'simple_slip', 'tire_model': 'tire_model', 'drive_wheels': 'drive_wheels', 'pacejka_b_front': 'pac_Bf',
                   'pacejka_b_rear': 'pac_Br', 'pacejka_c_front': 'pac_Cf', 'pacejka_c_rear': 'pac_Cr', 'pacejka_d_front': 'pac_Df',
                   'pacejka_d_rear': 'pac_Dr', 'linear_bf': 'lin_Bf', 'linear_br': 'lin_Br'}
_CODES = {'tire_model': {'pacejka': 0, 'linear': 1}, 'drive_wheels': {'all': 0, 'rear': 1}}
_NQ = {'kin': 6, 'dyn': 8, 'uni': 4}


def assert_same_parameters(kat, P):
    """Every ``p_*`` entry of the fixture against the problem record the package builds for the device and the oracle, exactly."""
    from dgsqp_amd.dynamics import INTEGRATORS
    same = lambda got, want, what: np.testing.assert_array_equal(np.asarray(got, float), np.asarray(want, float), err_msg=what)
    seen = set()

    def take(key):
        seen.add(key)
        v = kat[key]
        return v.item() if v.ndim == 0 else v
    M = take('p_M')
    assert (P.M, P.N, P.dt, P.substeps, P.obstacle_rows) == (M, take('p_N'), take('p_dt'), take('p_substeps'), take('p_obstacle_rows'))
    assert P.integrator == INTEGRATORS[take('p_method')]
    if take('p_has_track'):
        n = len(take('p_track_seg_curv'))
        assert P.n_segs == n and P.track_L == take('p_track_L') and P.track_kind == 0
        same(P.seg_s[:n + 1], kat['p_track_seg_s'], 'seg_s'); same(P.seg_curv[:n], kat['p_track_seg_curv'], 'seg_curv')
        same(P.seg_ang[:n + 1], take('p_track_seg_ang'), 'seg_ang'); seen.add('p_track_seg_s')
    for a in range(M):
        A, pre = P.agents[a], f'p_a{a}_'
        model = take(pre + 'model')
        nq = _NQ[model]
        assert A.model == {'kin': 0, 'dyn': 1, 'uni': 2}[model]
        for name, field in _VEHICLE_FIELDS.items():
            if pre + 'vehicle_' + name in kat.files:
                want = take(pre + 'vehicle_' + name)
                assert getattr(A, field) == _CODES.get(name, {}).get(want, want), (a, name, getattr(A, field), want)
        same(A.w_in, take(pre + 'cost_input_weight'), 'w_in'); same(A.w_rate, take(pre + 'cost_input_rate_weight'), 'w_rate')
        if take(pre + 'cost_kind') == 'goal':
            same(A.w_goal[:nq], take(pre + 'cost_state_weight'), 'w_goal'); same(A.goal[:nq], take(pre + 'cost_goal'), 'goal')
            assert A.goal_term_mult == take(pre + 'cost_terminal_multiplier')
            assert (A.w_prog, A.w_comp, A.w_block, A.w_obs) == (0, 0, 0, 0)
        else:
            same([A.w_prog, A.w_comp], take(pre + 'cost_comp_weights'), 'comp_weights')
            assert A.comp_type == {'atan': 0, 'linear': 1}[take(pre + 'cost_comp_type')]
            assert (A.w_block, A.w_obs, A.obs_cost_r) == (take(pre + 'cost_blocking_weight'), take(pre + 'cost_obs_weight'), take(pre + 'cost_obs_r'))
            assert not any(A.w_goal)
        assert A.has_rate == take(pre + 'has_rate')
        if A.has_rate:
            same([A.rate_ub, A.rate_lb], take(pre + 'rate'), 'rate')
        assert A.n_lane == take(pre + 'n_lane')
        for j in range(A.n_lane):
            ln = A.lane[j]
            same([ln.brk, ln.r, *ln.n_lo, *ln.n_hi, *ln.anchor], take(pre + f'lane{j}'), f'lane {j}')
        same(A.in_ub, take(pre + 'in_ub'), 'in_ub'); same(A.in_lb, take(pre + 'in_lb'), 'in_lb')
        same(A.st_ub[:nq], take(pre + 'st_ub'), 'st_ub'); same(A.st_lb[:nq], take(pre + 'st_lb'), 'st_lb')
        assert A.radius == take(pre + 'radius')
    left = {k for k in kat.files if k.startswith('p_')} - seen
    assert not left, f'parameters of the fixture that nothing was compared with: {sorted(left)}'


def load(case):
    """(fixture, Game, problem record) of a case, the parameters checked."""
    from dgsqp_amd.solver import build_problem
    kat = np.load(GOLD / f'multistage_{case}.npz')
    g = build_game(case)
    P = build_problem(*g.solver_args())
    assert_same_parameters(kat, P)
    for k in kat.files:
        if k.startswith('acc_'):
            assert kat[k] <= 1e-18, (k, float(kat[k]))          # the fixture's own accuracy record (60 against 90 digits)
    assert kat['margin'] > 1e-3                                 # distance of every evaluated state to a breakpoint
    return kat, g, P


def assert_layout(case, g, P):
    """The two directional cases exist for the big and the XL layout: ``plan`` must choose them."""
    from dgsqp_amd.solver import build_params, plan
    assert plan(P, build_params(g.params, qp_method='active_set'))['layout'] == DIRECTIONAL_CASES[case]


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def bar(kat, key, project_bar):
    return max(project_bar, 64.0 * float(kat['sens_' + key]))


def compare(kat, b, ev, project_bar, tag):
    """One scenario's evaluation (dict with x, g, q, G, Q) against the fixture; returns {key: relative error}.  Prints every figure
    before it asserts (pytest -s)."""
    errs = {}
    x = np.asarray(ev['x']).reshape(kat['x'][b].shape)
    pairs = [('g', ev['g'], kat['g'][b]), ('q', ev['q'], kat['q'][b])]
    if 'Q' in kat.files:
        pairs += [('G', ev['G'], kat['G'][b]), ('Q', ev['Q'], kat['Q'][b])]
    else:
        v = kat['v']
        pairs += [('Gv', np.stack([ev['G'] @ w for w in v]), kat['Gv'][b]), ('Qv', np.stack([ev['Q'] @ w for w in v]), kat['Qv'][b])]
    errs['x'] = rel(x, kat['x'][b])
    for key, got, want in pairs:
        errs[key] = rel(np.asarray(got).reshape(want.shape), want)
    print(f'{tag} scenario {b}: ' + ', '.join(f'{k} {e:.2e}' for k, e in errs.items()))
    np.testing.assert_allclose(x, kat['x'][b], rtol=max(X_RTOL, 64.0 * float(kat['sens_x'])), atol=X_ATOL, err_msg=f'{tag} scenario {b} x')
    for key, _, _ in pairs:
        assert errs[key] < bar(kat, key, project_bar), (tag, b, key, errs[key], bar(kat, key, project_bar))
    return errs
