"""Closed-loop batches on the device: DGSQP.step_batch (dgsqp_closed_loop_batch, csrc/dgsqp_closed_loop.h).

The check is the same in every case (its helpers are those of tests/closed_loop_checks.py) -- TEACHER FORCING: every (state, warm start)
pair a chain went through is stacked into ONE ``solve_batch`` call on the same solver, and u, l, x, cond, cost, status, num_iters and qp_solves of that call must equal the closed-loop
records bit for bit: every closed-loop step is the very solve the product already performs, whatever path the chain took.  Separately the
feedback between two steps is checked exactly against the host mirror ``dgsqp_amd.closed_loop.feedback``."""
import numpy as np
import pytest

from closed_loop_checks import COUNTS, DOUBLES, check_feedback, same, scenarios, solver_of, teacher_force      # noqa: F401  (solver_of is a fixture)
from conftest import agent_major

pytestmark = pytest.mark.gpu


def run_and_check(s, x0, u_tm, T, w=None):
    res = s.step_batch(x0, u_tm, T, disturbance=w, keep_predictions=True)
    check_feedback(s, res, x0, s._to_agent_major(np.asarray(u_tm, float)), w)
    teacher_force(s, res)
    return res


def test_basic_chain_with_disturbance(games, solver_of):
    """Case 1: kb_curve_N10 (n = 40, LDS layout), B = 6, T = 4, disturbance 1e-3 N(0, 1)."""
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 6, 41)
    w = 1e-3 * np.random.default_rng(5).standard_normal((6, 4, s.n_q))
    res = run_and_check(s, x0, u_tm, 4, w)
    assert (res['steps_done'] == 4).all() and s.dims.layout == 0
    assert not same(res['q'][:, 1], res['x'][:, 0, 1])            # the disturbance really entered
    # without keep_predictions: the same chain, no x / l
    lean = s.step_batch(x0, u_tm, 4, disturbance=w)
    assert 'x' not in lean and 'l' not in lean
    for key in ('q', 'u_ws', 'u', 'cond', 'cost', 'u_applied') + COUNTS + ('steps_done',):
        assert same(lean[key], res[key]), key


def test_chain_goes_on_after_a_failed_qp(games):
    """Case 2: scenario 1 starts with car 2 one metre outside the track (test_step_keeps_the_warm_start_after_a_failed_qp): its step 0 is
    'qp_fail', the warm start is kept, the chain goes on."""
    from dgsqp_amd.solver import DGSQP
    g = games['kb_curve_N10'][0]
    s = DGSQP(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    xa, ua = scenarios(g, 1, 31)
    xb, ub = scenarios(g, 2, 37)
    x0, u_tm = np.stack([xb[0], xa[0], xb[1]]), np.stack([ub[0], ua[0], ub[1]])
    x0[1, 11] = g.half_width + 1.0                    # e_y of car 2
    res = run_and_check(s, x0, u_tm, 3)
    assert res['msg'][1][0] == 'qp_fail' and res['status'][1, 0] == 4 and not res['converged'][1, 0]
    assert same(res['u_ws'][1, 1], res['u_ws'][1, 0])
    assert (res['steps_done'] == 3).all() and (res['status'] >= 0).all()
    assert not same(res['u_ws'][0, 1], res['u_ws'][0, 0])         # (the others shift)


def test_early_stop_on_a_non_finite_state(games, solver_of):
    """Case 3: disturbance[1, 1, :] = nan ends chain 1 after two steps; the other chains do not notice."""
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 3, 43)
    w = np.zeros((3, 4, s.n_q))
    clean = run_and_check(s, x0, u_tm, 4, w)
    w[1, 1, :] = np.nan
    res = run_and_check(s, x0, u_tm, 4, w)
    assert res['steps_done'].tolist() == [4, 2, 4] and clean['steps_done'].tolist() == [4, 4, 4]
    assert res['msg'][1][2:] == ['not_run', 'not_run'] and (res['status'][1, 2:] == -1).all()
    for key in DOUBLES:
        assert np.isnan(res[key][1, 2:]).all(), key
    assert np.isnan(res['q'][1, 2:]).all() and np.isnan(res['u_ws'][1, 2:]).all()
    for key in DOUBLES + COUNTS + ('q', 'u_ws', 'u_applied'):
        assert same(res[key][[0, 2]], clean[key][[0, 2]]), key
        assert same(res[key][1, :2], clean[key][1, :2]), key          # ... and chain 1 itself up to its end


def test_more_chains_than_workgroups(games, solver_of):
    """Case 4: B = 600 > the grid: a workgroup starts a second chain after finishing a first; state carried over between chains would
    show as a difference from solve_batch (which, at 1,800 scenarios, also runs cooperatively and defers)."""
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 600, 47)
    res = s.step_batch(x0, u_tm, 3, keep_predictions=True)
    check_feedback(s, res, x0, agent_major(u_tm))
    assert teacher_force(s, res) == 1800


@pytest.mark.parametrize('name', ['dyn_curve_N15', 'merge_N8'])
def test_other_vehicle_models(games, solver_of, name):
    """Case 5: dynamic bicycle (8 states per car) and unicycle (3 cars)."""
    s = solver_of(name)
    x0, u_tm = scenarios(games[name][0], 4, 53)
    run_and_check(s, x0, u_tm, 3)


def test_v2(games):
    """Case 6: DG-SQP v2 (the kinematic game of test_dgsqp_v2_matches_oracle) through DGSQPV2."""
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver_types import DGSQPV2Params
    from dgsqp_amd.solver_v2 import DGSQP as DGSQPV2
    g = mc.kinematic_racing_game('curve', N=12)
    g.params = DGSQPV2Params(dt=0.1, N=12)
    g.params.time_limit = None
    s = DGSQPV2(*g.solver_args(), print_method=None, lsqr_tol=1e-13)
    assert s._cparams.variant == 1
    x0, u_tm = scenarios(g, 3, 2)
    res = run_and_check(s, x0, u_tm, 3)
    assert (res['num_iters'][:, 0] > 20).all()                    # v2 really iterates


@pytest.mark.parametrize('case,qp_method', [('kin3_N20_dir', None), ('kin3_N25_dir', None), ('kin3_N20_dir', 'osqp')])
def test_big_and_xl_layouts(case, qp_method):
    """Case 7: the three-car kinematic games of tests/multistage_kat.py: n = 120 (big layout) and n = 150 (XL), one of them with OSQP."""
    import multistage_kat as mk
    from dgsqp_amd.solver import DGSQP, build_params, build_problem, plan
    g = mk.build_game(case)
    layout = plan(build_problem(*g.solver_args()), build_params(g.params, qp_method=qp_method))['layout']
    assert layout == mk.DIRECTIONAL_CASES[case] == {'kin3_N20_dir': 1, 'kin3_N25_dir': 2}[case]
    s = DGSQP(*g.solver_args(), print_method=None, qp_method=qp_method)
    assert s.dims.layout == layout and s.n == {'kin3_N20_dir': 120, 'kin3_N25_dir': 150}[case]
    x0, u_tm = scenarios(g, 2, 59)
    run_and_check(s, x0, u_tm, 2)


def test_half_arena_build(games, solver_of):
    """Case 8: libdgsqp_hip_b256.so (256-thread workgroups, two per CU)."""
    s = solver_of('kb_chicane_N15', workgroups_per_cu=2)
    x0, u_tm = scenarios(games['kb_chicane_N15'][0], 4, 61)
    run_and_check(s, x0, u_tm, 3)


def test_coexistence_with_solve_batch_and_its_logs(games, solver_of):
    """Case 9: solve_batch, step_batch, the same solve_batch: identical results; an event / iterate log setting made before step_batch
    neither breaks it nor is lost for the following solve_batch."""
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 5, 67)
    par = s._cparams
    s.set_trace((par.sqp_iters + 1) * (16 + 6 * par.line_search_iters))          # (the capacities DGSQP.solve() uses)
    s.set_iterate_log(par.sqp_iters + 2)
    try:
        a = s.solve_batch(x0, u_tm)
        tr_a, it_a = s.fetch_trace(5), s.fetch_iterate_log(5)
        res = s.step_batch(x0, u_tm, 2, keep_predictions=True)
        b = s.solve_batch(x0, u_tm)
        tr_b, it_b = s.fetch_trace(5), s.fetch_iterate_log(5)
    finally:
        s.set_trace(0)
        s.set_iterate_log(0)
    for key in DOUBLES + COUNTS:
        assert same(a[key], b[key]), key
        assert same(res[key][:, 0], a[key]), key                  # step 0 is that very solve
    assert all(len(t) > 0 for t in tr_b) and all(len(u) > 1 for u, _ in it_b)
    assert all(same(p, q) for p, q in zip(tr_a, tr_b))
    assert all(same(ua, ub) and same(la, lb) for (ua, la), (ub, lb) in zip(it_a, it_b))
    check_feedback(s, res, x0, agent_major(u_tm))
    teacher_force(s, res)


def test_one_step_is_one_solve_batch(games, solver_of):
    """Case 10."""
    from dgsqp_amd import closed_loop
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 7, 71)
    ref = s.solve_batch(x0, u_tm)
    res = s.step_batch(x0, u_tm, 1, keep_predictions=True)
    for key in DOUBLES + COUNTS:
        assert same(res[key][:, 0], ref[key]), key
    want = np.where(np.isin(ref['status'], (3, 4))[:, None], agent_major(u_tm), closed_loop.shift_warm_start(ref['u'], s.N, s.num_ua_d))
    assert same(res['u_ws'][:, 1], want) and same(res['q'][:, 1], ref['x'][:, 1]) and (res['steps_done'] == 1).all()
    check_feedback(s, res, x0, agent_major(u_tm))


def test_argument_errors(games, solver_of):
    """Case 11."""
    from dgsqp_amd import _ffi
    s = solver_of('kb_curve_N10')
    x0, u_tm = scenarios(games['kb_curve_N10'][0], 2, 73)
    with pytest.raises(ValueError):
        s.step_batch(x0, u_tm, 0)
    with pytest.raises(ValueError):
        s.step_batch(x0, u_tm, 2, disturbance=np.zeros((2, 3, s.n_q)))
    with pytest.raises(ValueError):
        s.step_batch(x0, u_tm, 2, disturbance=np.zeros((2, 2, s.n_q + 1)))
    with pytest.raises(RuntimeError):
        s.step_batch(x0, u_tm[:, :-1], 2)
    with pytest.raises(RuntimeError):
        s.step_batch(x0[:, :-1], u_tm, 2)
    empty = s.step_batch(np.zeros((0, s.n_q)), np.zeros((0, s.N, s.n_u)), 3, keep_predictions=True)
    assert empty['q'].shape == (0, 4, s.n_q) and empty['u_applied'].shape == (0, 3, s.n_u) and empty['x'].shape == (0, 3, s.N + 1, s.n_q)
    assert empty['status'].shape == (0, 3) and empty['steps_done'].shape == (0,) and empty['msg'] == []
    # the C-ABI itself: T < 1, B < 0 and a NULL required pointer are argument errors with a message
    u_am, q_buf = agent_major(u_tm), np.empty((2, 2, s.n_q))
    call = lambda B, T, q_out: s._lib.dgsqp_closed_loop_batch(s._h, B, T, _ffi.dptr(x0), _ffi.dptr(u_am), None, q_out, *([None] * 11))
    q_out = _ffi.dptr(q_buf)
    for B, T, qo in ((2, 0, q_out), (-1, 1, q_out), (2, 1, None)):
        assert call(B, T, qo) == -1 and s._lib.dgsqp_last_error(s._h)
    assert call(0, 1, None) == 0
