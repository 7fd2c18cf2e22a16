"""Track-edge rows of the LTV-MPC tracker on the device (dgsqp_mpc_t.edge_rows, csrc/dgsqp_mpc.h), teacher-forced with the helpers and at
the bars of tests/test_ltv_mpc.py: the numpy QP of tests/ltv_mpc_checks.py gains the two rows per stage (tests/track_width_checks.py),
linearised about the device's own logged D.  Kinematic bicycle, euler, N = 3: on the F1 spline at a narrow place, and on the curve track
with a sloped four-piece table; in each batch a car starts near an edge heading outwards with a reference beyond it, so that an edge row
is active (asserted from the helper's own answer).  Then: edge_rows = 0 on a handle with a table is today's tracker bit for bit, the
refusals through the raw ABI, the 256-thread build, and the raceline warm-start program against its host-loop composition with the rows on."""
import ctypes as C

import numpy as np
import pytest

import ltv_mpc_checks as chk
import test_ltv_mpc as base
import track_frame_checks as tf
import track_width_checks as tw

pytestmark = pytest.mark.gpu

N = 3
EDGE = tw.EDGE
ARC_TABLE = ([0.0, 0.25, 0.6, 1.3], [1.0, 0.9, 0.72, 0.95, 1.0], [0.8, 0.7, 0.75, 0.6, 0.9])      # knots (the track length closes them), left, right


def f1_game():
    from dgsqp_amd import montecarlo as mc
    return mc.f1_racing_game(N=6)


def arc_game():
    """The curve track with a four-piece table: slopes between -0.51 and +0.33, left != right."""
    from dgsqp_amd import montecarlo as mc
    g = mc.kinematic_racing_game('curve', N=10)
    k, l, r = ARC_TABLE
    g.track.set_width_table(k + [g.track.track_length], l, r)
    return g


def edge_case(g, s_at, ey_frac, ey_ref, epsi0, seed):
    """Three scenarios of test_ltv_mpc.scenario moved to s_at, each car at ey_frac of the width on that side, heading epsi0, reference e_y ey_ref."""
    q0, u_ws, du_ws, q_ref, idx = base.scenario('kin', 3, N, seed=seed)
    V, S, EY = idx
    q0[:, S] += s_at
    q_ref[:, :, S] += np.asarray(s_at, float)[:, None]
    for b in range(3):
        w = g.track.left_width(q0[b, S]) if ey_frac[b] > 0 else g.track.right_width(q0[b, S])
        q0[b, EY], q0[b, 3] = ey_frac[b] * w, epsi0[b]
        q_ref[b, :, EY] = ey_ref[b]
    return q0, u_ws, du_ws, q_ref, idx


CASES = {'f1': (f1_game, [478.0, 479.5, 62.0], [0.9, -0.9, 0.93], [0.9, -0.9, 1.6], [0.2, -0.2, 0.2], 41),
         'arc': (arc_game, [0.0, 0.0, 0.0], [0.9, -0.9, 0.88], [1.2, -1.2, 1.2], [0.2, -0.2, 0.2], 43)}


def solve(which, monkeypatch, oracle, want_active, **solver_kw):
    from dgsqp_amd import ltv_mpc
    from dgsqp_amd.solver import DGSQP, build_problem
    make, s_at, frac, ref, epsi, seed = CASES[which]
    g = make()
    solver, P = DGSQP(*g.solver_args(), print_method=None, **solver_kw), build_problem(*g.solver_args())
    mdl = solver.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = edge_case(g, s_at, frac, ref, epsi, seed)
    bounds = base.wide_bounds(mdl, idx, u=(2.0, 0.436), du=(10.0, 4.5))
    kw = dict(N=N, track_edges=ltv_mpc.TrackEdgeRows())
    rec, out = base.run(solver, 0, base.weights('kin', idx), bounds, q0, u_ws, du_ws, q_ref, **kw)
    rec.edge_rows = 1                                    # (base.run lowers the record without the rows; mpc_batch lowered it with them)
    rows = out['dims']['rows']
    assert [tuple(r) for r in rows[-2 * N:]] == [(EDGE, k, 0, sg) for k in range(1, N + 1) for sg in (-1, 1)]
    assert (rows[:-2 * N, 0] != EDGE).all() and (out['status'] == 0).all()
    with tw.edge_rows(monkeypatch, g.track):
        seen = base.teacher_forced(oracle, solver, P, 0, out, rec, q0, u_ws, q_ref, None)
    active = {(kind, sign) for kind, _, sign in seen if kind == EDGE}
    print(which, 'edge rows seen active (kind, sign):', sorted(active))
    assert active >= want_active
    return g, solver, (q0, u_ws, du_ws, q_ref, idx), bounds, out


def test_f1_spline_narrow_place(monkeypatch, oracle):
    """s ~ 478 m, where the left edge is 0.59 m from the centre line (the constant half width is 0.70 m): the left row of stage 3 is active."""
    g, *_ = solve('f1', monkeypatch, oracle, {(EDGE, 1)})
    assert g.track.left_width(478.3) < 0.6 < g.track.half_width


def test_arc_track_with_a_sloped_table(monkeypatch, oracle):
    """Both sides: a right row and a left row are active, on pieces of different slope."""
    solve('arc', monkeypatch, oracle, {(EDGE, 1), (EDGE, -1)})


def test_256_thread_build(monkeypatch, oracle):
    g, solver, data, bounds, out = solve('arc', monkeypatch, oracle, {(EDGE, 1), (EDGE, -1)}, workgroups_per_cu=2)
    assert out['timing']['block'] == 256


def test_without_the_rows_nothing_changes():
    """edge_rows = 0 on a handle that carries a table against a handle of the same game without one: the tracker's outputs and its log,
    bit for bit; and with the rows on, but no car near an edge, the QPs are the same up to the larger row table."""
    from dgsqp_amd import ltv_mpc
    from dgsqp_amd.solver import DGSQP
    g1, g0 = arc_game(), arc_game()
    g0.track.clear_width_table()
    s1, s0 = DGSQP(*g1.solver_args(), print_method=None), DGSQP(*g0.solver_args(), print_method=None)
    assert (s1._problem.n_width, s0._problem.n_width) == (5, 0)
    mdl = s1.joint_dynamics.dynamics_models[0]
    q0, u_ws, du_ws, q_ref, idx = base.scenario('kin', 4, N, seed=5)
    bounds = base.wide_bounds(mdl, idx, ey=0.9)
    outs = [s.mpc_batch(0, base.weights('kin', idx), bounds, q0, u_ws, du_ws, q_ref, N=N, log=True) for s in (s1, s0)]
    for key in ('q_pred', 'u_pred', 'du_pred', 'log_D', 'log_D_bar', 'log_lam'):
        assert np.array_equal(base.bits(outs[0][key]), base.bits(outs[1][key])), key
    assert np.array_equal(outs[0]['status'], outs[1]['status']) and np.array_equal(outs[0]['qp_steps'], outs[1]['qp_steps'])
    assert outs[0]['dims']['lds_bytes'] == outs[1]['dims']['lds_bytes'] and np.array_equal(outs[0]['dims']['rows'], outs[1]['dims']['rows'])
    on = s1.mpc_batch(0, base.weights('kin', idx), bounds, q0, u_ws, du_ws, q_ref, N=N, log=True, track_edges=ltv_mpc.TrackEdgeRows())
    assert on['dims']['n_rows'] == outs[0]['dims']['n_rows'] + 2 * N and on['dims']['lds_bytes'] >= outs[0]['dims']['lds_bytes'] + 8 * 4 * N
    assert (on['log_lam'][:, :, -2 * N:] == 0).all()                 # nobody is near an edge: the rows stay inactive ...
    assert np.abs(on['q_pred'] - outs[0]['q_pred']).max() < 1e-12    # ... and the minimiser is the same


def test_refusals_through_the_raw_abi():
    from dgsqp_amd import _ffi, ltv_mpc, montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g1, g0 = arc_game(), mc.kinematic_racing_game('curve', N=10)
    s1, s0 = DGSQP(*g1.solver_args(), print_method=None), DGSQP(*g0.solver_args(), print_method=None)
    q0, u_ws, du_ws, q_ref, idx = base.scenario('kin', 1, N, seed=1)
    cost = base.weights('kin', idx)
    INF = base.INF

    def rec(edge_rows, n_q=6, cost=cost):
        r = ltv_mpc.lower(0, n_q, cost, None, None, INF * np.ones(n_q), -INF * np.ones(n_q), (1, 1), (-1, -1), (1, 1), (-1, -1), N, 2, 0.75)
        r.edge_rows = edge_rows
        return r

    def refused(s, r, word):
        assert s._lib.dgsqp_set_mpc(s._h, C.byref(r)) == _ffi.E_ARG
        msg = s._lib.dgsqp_last_error(s._h).decode()
        assert msg.startswith('mpc: ') and word in msg, msg
    assert s1._lib.dgsqp_set_mpc(s1._h, C.byref(rec(1))) == 0
    refused(s1, rec(2), 'edge_rows must be 0 or 1')
    refused(s1, rec(-1), 'edge_rows must be 0 or 1')
    refused(s0, rec(1), 'without a width table')
    assert s0._lib.dgsqp_set_mpc(s0._h, C.byref(rec(0))) == 0
    with pytest.raises(ValueError, match='mpc: edge_rows on a handle without a width table'):
        s0.mpc_batch(0, cost, base.wide_bounds(s0.joint_dynamics.dynamics_models[0], idx), q0, u_ws, du_ws, q_ref, N=N, track_edges=ltv_mpc.TrackEdgeRows())
    from dgsqp_amd.solver import build_problem
    merge = mc.merge_game(N=4)                                  # unicycles, no track: the handle gets a table over its placeholder length
    lib = s1._lib
    P = build_problem(*merge.solver_args())
    tab = np.array([[0.0, 1.0, 1.0], [P.track_L, 1.0, 1.0]])
    P.n_width, P.widths = 2, tab.ctypes.data
    h = C.c_void_p()
    assert lib.dgsqp_create(C.byref(P), C.byref(s1._cparams), 0, C.byref(h)) == 0, lib.dgsqp_last_error(None)
    try:
        w4 = ltv_mpc.TrackingCost(state_weight=np.ones(4), input_weight=(1e-2, 1e-2), rate_weight=(0.1, 1.0))
        assert lib.dgsqp_set_mpc(h, C.byref(rec(1, n_q=4, cost=w4))) == _ffi.E_ARG
        msg = lib.dgsqp_last_error(h).decode()
        assert msg.startswith('mpc: ') and 'unicycle' in msg, msg
        assert lib.dgsqp_set_mpc(h, C.byref(rec(0, n_q=4, cost=w4))) == 0
    finally:
        lib.dgsqp_destroy(h)


def test_raceline_program_with_the_rows_on():
    """dgsqp_raceline_warm_start_batch with the study tracker's edge rows (study_tracker(track_constraints=True): the e_y box open, the rows
    in its place) against the host-loop composition of tests/raceline_checks.py -- two CA_LTV_MPC.solve_batch calls per car with the same
    record --, bit for bit; the dynamic F1 game, N = 6.  Six states around the narrow place at s ~ 478 m on the line, and six at the wide
    place at s ~ 63 m (left width 1.35 m and more) with both cars 0.9 m left of the centre line: inside the track, outside the constant
    box of +-0.596 m -- there the program with the rows succeeds and the program with the box cannot (its QPs are infeasible)."""
    import raceline_checks as rc
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    rl = tf.f1_raceline()
    g = mc.f1_racing_game(N=6, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=rl, edges='track')
    s = DGSQP(*g.solver_args(), print_method=None)
    s.set_raceline(rl)
    tracker = mc.study_tracker(g)
    assert tracker['track_edges'] is not None and tracker['bounds']['qu_ub'].p.x_tran == 1e9
    W = mc.raceline_ws(g)
    assert W.mpc.edge_rows == 1
    B = 12
    wide = np.arange(B) >= 6
    sa = np.concatenate((np.linspace(474.0, 482.0, 6), np.linspace(62.0, 63.5, 6)))
    x0 = np.zeros((B, 16))
    for a in range(2):
        sc = sa + 0.8 * a
        r = rl.eval(rl.s2t(sc))
        assert (g.track.left_width(sc[wide]) > 1.3).all() and g.half_width < 0.6
        x0[:, 8 * a + 2], x0[:, 8 * a + 5], x0[:, 8 * a + 6], x0[:, 8 * a + 7] = r[:, 3], r[:, 6], sc, np.where(wide, 0.9, r[:, 8])
    dev = s.raceline_warm_start_batch(x0, W)
    q_ref = s.fetch_raceline_ref(B)
    mpc = rc.lowered_tracker(g, tracker)
    mpc.track_edges = tracker['track_edges']
    host_u, host_ok = rc.host_loop(g, tracker, mpc, x0, q_ref)
    print(f'ok with the rows: {dev["ok"].astype(int).tolist()}')
    assert np.array_equal(dev['ok'], host_ok)
    assert np.array_equal(base.bits(dev['u_ws'][dev['ok']]), base.bits(host_u[host_ok]))
    assert dev['ok'][wide].all()
    g_box = mc.f1_racing_game(N=6, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=rl)
    box = s.raceline_warm_start_batch(x0, mc.raceline_ws(g_box))
    print(f'ok with the box:  {box["ok"].astype(int).tolist()}')
    assert not box['ok'][wide].any()
