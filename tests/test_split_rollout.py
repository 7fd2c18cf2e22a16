"""The dynamic-bicycle rollout split into a velocity chain and a pose chain on two wavefronts (csrc/dgsqp_eval.h:
dev_rollout_dyn), on a real MI355X.

(a) parity of ``evaluate_batch`` with the oracle at the 1e-12 bar of tests/test_gpu.py::test_evaluate_parity, at points where
    the chains leave their fast paths: slip angles beyond atan(7/16), heading errors beyond 0.78 rad, a step across a track-segment
    boundary, a step across the lap seam (the test asserts that the inputs do that), for rk4, rk3 and rk2;
(b) the hand-off between the two wavefronts is deterministic: repeated evaluations and repeated solves are bit-identical;
(c) the fused pass, the multi-trajectory line-search rollouts and the plain rollout agree: the trajectory a solve returns is
    ``evaluate_batch``'s at the returned inputs, to the bit;
(d) the same three at a short horizon (N = 4), where the hand-off ring is deeper than the whole rollout of a stage.

(e) slip angles that are exactly zero: atan2(0, vx) in the rollout's and the Taylor pass's tyre chains.

The single-wavefront mode of dev_rollout_dyn (DYN_BOTH), taken when dyn_ring_setup finds no room for one evaluation of every lane
pair, is reached by no game this package builds (see the docstring of test_short_horizon_dynamic_game); it is run directly and
compared bit for bit with the split modes in tests/test_device_math.py::test_single_wavefront_rollout_is_the_split_one."""
import numpy as np
import pytest

from conftest import agent_major

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def _dyn_game(method, N, substeps):
    """dynamic_racing_game (exact_dynamic) under another integrator of the reference (dynamics_models.py:188-219)."""
    from dgsqp_amd import montecarlo as mc
    if method == 'rk4':
        return mc.dynamic_racing_game(N=N, rk4_substeps=substeps)
    track = mc._track('curve', 45, 1.0)
    cfg = lambda: mc.DynamicBicycleConfig(dt=0.1, model_name='dynamic_bicycle', noise=False, discretization_method=method, simple_slip=False,
                                          tire_model='pacejka', mass=2.2187, yaw_inertia=0.02723, wheel_friction=0.9, pacejka_b_front=5.0,
                                          pacejka_b_rear=5.0, pacejka_c_front=2.28, pacejka_c_rear=2.28, M=substeps)
    models = [mc.CasadiDynamicBicycleCombined(0, cfg(), track=track) for _ in range(2)]
    joint = mc.CasadiDecoupledMultiAgentDynamicsModel(0, models, mc.MultiAgentModelConfig(
        dt=0.1, discretization_method=method, use_mx=False, code_gen=False, verbose=False, compute_hessians=True, M=substeps))
    params = mc.DGSQPParams(solver_name='DGSQP', dt=0.1, N=N, reg=1e-3, nonmono_ls=True, line_search_iters=50, sqp_iters=50, p_tol=1e-3,
                            d_tol=1e-3, beta=0.01, tau=0.5, verbose=False)
    cost = lambda: mc.RacingCost(input_weight=(1.0, 1.0), input_rate_weight=(1.0, 1.0), comp_weights=(1.0, 5.0), comp_type='linear')
    return mc.Game(joint, [cost(), cost()], [None, None], mc.CollisionAvoidance([0.23, 0.23]), mc._bounds(1.0, 2), params, track, 1.0, 0.46,
                   name=f'dyn_{method}')


def _games():
    from dgsqp_amd import montecarlo as mc
    return {'dyn_curve_N25': lambda: mc.dynamic_racing_game(N=25, rk4_substeps=10),
            'dyn_curve_N15': lambda: mc.dynamic_racing_game(N=15, rk4_substeps=4, game_def='curve'),
            'dyn_rk3_N10': lambda: _dyn_game('rk3', 10, 4), 'dyn_rk2_N10': lambda: _dyn_game('rk2', 10, 4)}


def _slow_branch_points(g, P, s):
    """Four scenarios (q = [x, y, vx, vy, w, e_psi, s, e_y] per car): 0 a car sliding sideways, 1 a car across the track, 2 a car just
    before the first segment boundary, 3 a car just before the end of the lap."""
    from dgsqp_amd.montecarlo import sample_scenarios
    x0, u_tm = sample_scenarios(g, 4, seed=31)
    u = agent_major(u_tm)
    x0 = x0.copy()
    x0[0, 2:5] = (1.5, 0.8, 0.0)                # rear slip angle atan2(0.8, 1.5) = 0.49 rad
    x0[1, 8 + 5] = 0.9                          # e_psi of car 2
    x0[2, 2], x0[2, 6] = 1.5, P.seg_s[1] - 0.05
    x0[3, 8 + 2], x0[3, 8 + 6] = 1.5, P.track_L - 0.05
    return x0, u


@pytest.mark.parametrize('name', ['dyn_curve_N25', 'dyn_curve_N15', 'dyn_rk3_N10', 'dyn_rk2_N10'])
def test_evaluate_parity_on_the_slow_branches(oracle, name):
    from dgsqp_amd.solver import DGSQP, build_problem
    g = _games()[name]()
    P = build_problem(*g.solver_args())
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    x0, u = _slow_branch_points(g, P, s)
    rng = np.random.default_rng(1)
    l = np.maximum(0, rng.standard_normal((len(x0), s.n_c_total)))
    ev = s.evaluate_batch(x0, u, l)
    ref = [oracle.evaluate(P, x0[b], u[b], l[b], 1) for b in range(len(x0))]
    # the inputs do what they are here for (read off the ORACLE's trajectories)
    x = np.array([o['x'] for o in ref]).reshape(len(x0), s.N + 1, 2, 8)
    L_r = P.agents[0].L_r
    slip = np.abs(np.arctan2(x[0, :, 0, 3] - x[0, :, 0, 4] * L_r, x[0, :, 0, 2])).max()
    assert slip > np.arctan(7.0 / 16.0), slip
    assert np.abs(x[1, :, 1, 5]).max() > 0.78
    sa = x[2, :, 0, 6]
    assert sa[0] < P.seg_s[1] <= sa[1], (sa[:2], P.seg_s[1])
    sb = x[3, :, 1, 6]
    assert sb[0] < P.track_L <= sb[1], (sb[:2], P.track_L)
    for b in range(len(x0)):
        for key in ('x', 'q', 'g', 'G', 'Q'):
            err = rel(ev[key][b], ref[b][key])
            print(name, 'scenario', b, key, f'{err:.2e}')
            assert err < 1e-12, (key, b, err)


def test_hand_off_is_deterministic():
    from dgsqp_amd.montecarlo import dynamic_racing_game, sample_scenarios
    from dgsqp_amd.solver import DGSQP
    g = dynamic_racing_game(N=25, rk4_substeps=10)
    s = DGSQP(*g.solver_args(), print_method=None)
    x0, u_tm = sample_scenarios(g, 256, seed=32)
    u = agent_major(u_tm)
    ev = [s.evaluate_batch(x0[:64], u[:64]) for _ in range(3)]
    for e in ev[1:]:
        for key in ('x', 'q', 'g', 'G', 'Q'):
            assert np.array_equal(e[key].view(np.int64), ev[0][key].view(np.int64)), key
    r1, r2 = s.solve_batch(x0, u_tm), s.solve_batch(x0, u_tm)
    for key in ('status', 'num_iters', 'qp_solves'):
        assert np.array_equal(r1[key], r2[key]), key
    for key in ('u', 'l', 'x'):
        assert np.array_equal(r1[key].view(np.int64), r2[key].view(np.int64)), key


def test_solve_trajectory_is_the_evaluated_one():
    """The solve's trajectory comes out of the fused pass or a line-search block (K concurrent trajectories), evaluate_batch's out
    of a fused pass of its own: the same chain arithmetic on other lanes.  Compared on the scenarios that ended converged."""
    from dgsqp_amd.montecarlo import dynamic_racing_game, sample_scenarios
    from dgsqp_amd.solver import DGSQP
    g = dynamic_racing_game(N=25, rk4_substeps=10)
    s = DGSQP(*g.solver_args(), print_method=None)
    x0, u_tm = sample_scenarios(g, 64, seed=33)
    res = s.solve_batch(x0, u_tm)
    ok = (res['status'] <= 1) & np.isfinite(res['u']).all(axis=1)
    assert ok.sum() >= 32
    ev = s.evaluate_batch(x0[ok], res['u'][ok])
    xs = np.ascontiguousarray(res['x'][ok]).reshape(ev['x'].shape)
    assert np.array_equal(xs.view(np.int64), ev['x'].view(np.int64)), np.abs(xs - ev['x']).max()


@pytest.mark.parametrize('method', ['rk4', 'rk3'])
def test_short_horizon_dynamic_game(oracle, method):
    """dynamic_racing_game at N = 4, rk4 and rk3: (a) evaluate_batch against the oracle at 1e-12, repeated solves bit-identical, (c) the
    trajectory a solve returns is evaluate_batch's at the returned inputs, to the bit.

    This game was meant to drive the line search's blocks of K concurrent trial trajectories into the single-wavefront mode of
    dev_rollout_dyn (DYN_BOTH: dyn_ring_setup's depth (N + 1) nq / (3 K M) < 1 needs K >= 14 at N = 4, M = 2).  It does NOT: the
    layout (dgsqp_layout.h, ls_spec) only grants K > 0 where the QP scratch reaches beyond the evaluation arrays by whole trajectories,
    and a host-side print of ls_spec gives 0 for every two-car dynamic game at N = 1 .. 5 (rk4, rk3, v2 parameters, the 'curve'
    definition; active-set and OSQP QP) -- 15 at N = 25, 16 at N = 15.  With K = 0 every trial is a single-trajectory rollout
    (depth 13): the split modes, as are the fused passes of the solve and of evaluate_batch.  So every part of this test runs the
    split modes at a short horizon and (c) compares split with split; DYN_BOTH is covered by
    tests/test_device_math.py::test_single_wavefront_rollout_is_the_split_one, which calls it through the probe library."""
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP, build_problem
    g = _dyn_game(method, 4, 4)
    P = build_problem(*g.solver_args())
    x0, u_tm = sample_scenarios(g, 64, seed=34)
    u = agent_major(u_tm)
    # (a) evaluate_batch against the oracle
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    rng = np.random.default_rng(2)
    l = np.maximum(0, rng.standard_normal((4, s.n_c_total)))
    ev = s.evaluate_batch(x0[:4], u[:4], l)
    for b in range(4):
        ref = oracle.evaluate(P, x0[b], u[b], l[b], 1)
        for key in ('x', 'q', 'g', 'G', 'Q'):
            err = rel(ev[key][b], ref[key])
            print(method, 'scenario', b, key, f'{err:.2e}')
            assert err < 1e-12, (key, b, err)
    # repeated solves are bit-identical
    s = DGSQP(*g.solver_args(), print_method=None)
    r1, r2 = s.solve_batch(x0, u_tm), s.solve_batch(x0, u_tm)
    for key in ('status', 'num_iters', 'qp_solves'):
        assert np.array_equal(r1[key], r2[key]), key
    for key in ('u', 'l', 'x'):
        assert np.array_equal(r1[key].view(np.int64), r2[key].view(np.int64)), key
    # (c) the returned trajectory is evaluate_batch's at the returned inputs
    ok = (r1['status'] <= 1) & np.isfinite(r1['u']).all(axis=1)
    print(method, 'converged', int(ok.sum()), 'of', len(ok), 'iterations', r1['num_iters'][ok].min(), '..', r1['num_iters'][ok].max())
    assert ok.sum() >= 32
    assert r1['num_iters'][ok].max() >= 1
    ev = s.evaluate_batch(x0[ok], r1['u'][ok])
    xs = np.ascontiguousarray(r1['x'][ok]).reshape(ev['x'].shape)
    assert np.array_equal(xs.view(np.int64), ev['x'].view(np.int64)), np.abs(xs - ev['x']).max()


def test_zero_slip_angles(oracle):
    """atan2(0, vx): dynamic_racing_game at N = 4, rk4 with 4 substeps, evaluate_batch against the oracle at 1e-12.
    Scenario 0: car 1 is exactly at rest laterally (vy = w = 0, vx > 0) and never steers, so both of its slip angles are atan2(0, vx)
    at every f_c evaluation of the horizon (vx = 0 itself is not admissible: the Taylor pass divides by vx).  Scenario 1: car 1 starts with
    vy + w L_f = 0 exactly (front slip angle atan2(0, vx) at the first evaluation) at vx = 2, the sampler's lowest speed."""
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP, build_problem
    N = 4
    g = _dyn_game('rk4', N, 4)
    P = build_problem(*g.solver_args())
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    x0, u_tm = sample_scenarios(g, 2, seed=35)
    u = agent_major(u_tm)
    x0 = x0.copy()
    assert x0[0, 2] > 0 and x0[0, 3] == 0 and x0[0, 4] == 0
    u[0, 1:2 * N:2] = 0.0                          # steering of car 1, every stage
    L_f = P.agents[0].L_f
    x0[1, 2], x0[1, 3], x0[1, 4] = 2.0, -0.5 * L_f, 0.5
    assert x0[1, 3] + x0[1, 4] * L_f == 0.0 and 0.5 * L_f == float(np.float64(0.5) * np.float64(L_f))
    u[1, 1] = 0.0                                  # no steering in the first stage: the front wheel frame is the body frame there
    rng = np.random.default_rng(3)
    l = np.maximum(0, rng.standard_normal((2, s.n_c_total)))
    ev = s.evaluate_batch(x0, u, l)
    ref = [oracle.evaluate(P, x0[b], u[b], l[b], 1) for b in range(2)]
    xr = np.asarray(ref[0]['x']).reshape(N + 1, 2, 8)
    assert (xr[:, 0, 3] == 0).all() and (xr[:, 0, 4] == 0).all() and (xr[:, 0, 2] > 0).all()
    for b in range(2):
        for key in ('x', 'q', 'g', 'G', 'Q'):
            err = rel(ev[key][b], ref[b][key])
            print('zero slip angle, scenario', b, key, f'{err:.2e}')
            assert err < 1e-12, (key, b, err)
