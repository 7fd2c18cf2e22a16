"""Track-edge rows in the game (game.TrackEdges, dgsqp_agent_t.edge_rows) on the device.  No oracle: oracle/ has no edge rows.
  * constant table == box: a table of constant width W and margin m against the same game with e_y in +-(W - m): g and G of the matched
    rows and q bit for bit (the slope is exactly 0.0); Q at 1e-13 relative to its largest entry -- the costate source adds the two
    multipliers of a state in another order (right, left against upper, lower), so bits are not promised there.  On the LDS layout, the big
    layout, the XL layout (n = 136) and the 256-thread build.
  * a sloped four-piece table: g against numpy on the returned trajectory (1e-14), the edge rows of G against central differences of g and Q
    against central differences of q + G'l over u.  Bars 1e-6 / 1e-5 relative to the largest entry: with h = 1e-6 the truncation term
    h^2 f''' / 6 is ~1e-11 and the rounding term eps |f| / h ~1e-9 on entries of size 1 .. 10, two orders under the bars; the stages stay 1e-3 m
    from every knot (asserted), so no difference straddles a change of slope.
  * solves on the F1 track, edges='track', dynamic N = 10, 16 scenarios from the raceline front end at the narrow place: converged solves keep
    every edge value under p_tol (recomputed in numpy from the returned x), and two launches agree bit for bit."""
import os

import numpy as np
import pytest

import track_frame_checks as tf
import track_width_checks as tw

pytestmark = pytest.mark.gpu

TABLE = ([0.0, 0.25, 0.6, 1.3], [1.0, 0.9, 0.72, 0.95, 1.0], [0.8, 0.7, 0.75, 0.6, 0.9])


def inputs(s, B, seed):
    rng = np.random.default_rng(seed)
    M = s.M
    nqa = s.n_q // M
    x0 = np.zeros((B, s.n_q))
    for a in range(M):
        o = a * nqa
        x0[:, o + 2], x0[:, o + nqa - 2], x0[:, o + nqa - 1] = 1.5 + 0.3 * rng.random(B), 0.12 + 0.3 * rng.random(B) + 0.45 * a, 0.3 * (rng.random(B) - 0.5)
        x0[:, o + nqa - 3] = 0.1 * (rng.random(B) - 0.5)
        x0[:, o], x0[:, o + 1] = x0[:, o + nqa - 2], x0[:, o + nqa - 1]
    u = np.concatenate([np.stack([0.5 * rng.standard_normal((B, s.N)), 0.1 * rng.standard_normal((B, s.N))], axis=2).reshape(B, -1) for _ in range(M)], axis=1)
    return x0, u


@pytest.mark.parametrize('layout', ['lds', 'big', 'xl', 'v2', 'b256'])
def test_constant_table_equals_box(layout):
    """lds: two cars, kinematic N = 4.  big / xl: the three-car N = 20 / 25 games of the directional fixtures (kin3_N20_dir, kin3_N25_dir),
    evaluation only.  v2: the lds game under DG-SQP v2 (DGSQPV2Params, solver_v2.DGSQP).  b256: the lds game on the 256-thread build."""
    from dgsqp_amd.solver import DGSQP, plan
    N, M = {'big': (20, 3), 'xl': (25, 3)}.get(layout, (4, 2))
    W, m = 0.9, 0.1
    kw = dict(workgroups_per_cu=2) if layout == 'b256' else {}
    ge, gb = tw.edge_game(N=N, table=([0.0], [W, W], [W, W]), margin=m, M=M), tw.edge_game(N=N, box=W, margin=m, M=M)
    cls = DGSQP
    if layout == 'v2':
        from dgsqp_amd.solver_types import DGSQPV2Params
        from dgsqp_amd.solver_v2 import DGSQP as cls
        ge.params, gb.params = DGSQPV2Params(dt=0.1, N=N), DGSQPV2Params(dt=0.1, N=N)
    se, sb = cls(*ge.solver_args(), print_method=None, **kw), cls(*gb.solver_args(), print_method=None, **kw)
    want = {'big': 1, 'xl': 2}.get(layout, 0)
    assert plan(se._problem, se._cparams)['layout'] == want and plan(sb._problem, sb._cparams)['layout'] == want
    assert se._cparams.variant == (1 if layout == 'v2' else 0)
    re_, rb = tw.row_table(se._problem), tw.row_table(sb._problem)
    assert len(re_) == se.n_c_total == len(rb)
    eyi = se.n_q // M - 1
    match = {('edge_l', k, a, 1): ('st_ub', k, a, eyi) for k in range(1, N + 1) for a in range(M)}
    match.update({('edge_r', k, a, 0): ('st_lb', k, a, eyi) for k in range(1, N + 1) for a in range(M)})
    where = {r: i for i, r in enumerate(rb)}
    perm = np.array([where[match.get(r, r)] for r in re_])
    assert sorted(perm) == list(range(len(rb)))
    B = 3
    x0, u = inputs(se, B, 7)
    lb = np.random.default_rng(8).random((B, len(rb)))
    oe, ob = se.evaluate_batch(x0, u, lb[:, perm]), sb.evaluate_batch(x0, u, lb)
    assert np.array_equal(oe['x'], ob['x']) and np.array_equal(oe['q'], ob['q'])
    assert np.array_equal(oe['g'], ob['g'][:, perm]) and np.array_equal(oe['G'], ob['G'][:, perm])
    dQ = np.abs(oe['Q'] - ob['Q']).max() / np.abs(ob['Q']).max()
    print(f'{layout}: Q differs by {dQ:.2e} relative to its largest entry; bit-identical: {np.array_equal(oe["Q"], ob["Q"])}')
    assert dQ <= 1e-13


@pytest.mark.parametrize('case', list(tw.KAT_CASES))
def test_exact_fixtures(case):
    """evaluate_batch on kin2_edges_euler_N3 / dyn2_edges_rk4m3_N3 against tests/golden/multistage_<case>.npz (tools/make_track_edge_kats.py:
    the rollout, the costs and the rows -- the edge rows among them -- as plain 60-digit functions, differenced): x at rtol 1e-13, g, G, q, Q at
    multistage_kat.DEVICE_BAR or 64 x the fixture's sensitivity (the helper's own rule).  Every edge row carries a multiplier; the stages
    fall into at least two pieces of the four-piece table, 1e-3 m from every knot (asserted by the tool)."""
    import multistage_kat as mk
    from dgsqp_amd.solver import DGSQP
    kat, g, P = tw.load_edge_case(case)
    assert (kat['l'][:, kat['edge_rows']] >= 0.1).all()
    s = DGSQP(*g.solver_args(), print_method=None)
    assert (s.n, s.n_c_total) == (kat['u'].shape[1], kat['l'].shape[1])
    ev = s.evaluate_batch(kat['x0'], kat['u'], kat['l'])
    worst = {}
    for b in range(len(kat['x0'])):
        for k, e in mk.compare(kat, b, {key: ev[key][b] for key in ('x', 'g', 'q', 'G', 'Q')}, mk.DEVICE_BAR, f'{case} device').items():
            worst[k] = max(worst.get(k, 0.0), e)
    print(f'{case}: device vs fixture, maxima ' + ', '.join(f'{k} {e:.2e}' for k, e in worst.items()))


@pytest.mark.parametrize('kind', ['kin', 'dyn'])
def test_sloped_table_against_numpy_and_differences(kind):
    from dgsqp_amd.solver import DGSQP
    N, m = 3, 0.05
    g = tw.edge_game(kind=kind, N=N, table=TABLE, margin=m)
    s = DGSQP(*g.solver_args(), print_method=None)
    rows = tw.row_table(s._problem)
    assert len(rows) == s.n_c_total
    B = 2
    x0, u = inputs(s, B, 3)
    l = 0.2 + np.random.default_rng(4).random((B, len(rows)))
    o = s.evaluate_batch(x0, u, l)
    nqa = s.n_q // 2
    x = o['x'].reshape(B, N + 1, 2, nqa)
    sk, ey = x[..., nqa - 2], x[..., nqa - 1]
    t = g.track
    kn = t.width_table()[:, 0]
    assert np.abs(t._sbar(sk[:, 1:])[..., None] - kn).min() > 1e-3
    pieces = {int(i) for i in np.searchsorted(kn, t._sbar(sk[:, 1:]).ravel(), side='right') - 1}
    assert len(pieces) >= 2, pieces
    ie = [i for i, r in enumerate(rows) if r[0].startswith('edge')]
    for i in ie:
        typ, k, a, _ = rows[i]
        want = -(t.right_width(sk[:, k, a]) - m) - ey[:, k, a] if typ == 'edge_r' else ey[:, k, a] - (t.left_width(sk[:, k, a]) - m)
        assert np.abs(o['g'][:, i] - want).max() <= 1e-14
    h = 1e-6
    Gfd, Qfd = np.zeros_like(o['G']), np.zeros_like(o['Q'])
    for c in range(s.n):
        up, um = u.copy(), u.copy()
        up[:, c] += h; um[:, c] -= h
        p, q = s.evaluate_batch(x0, up, l), s.evaluate_batch(x0, um, l)
        Gfd[:, :, c] = (p['g'] - q['g']) / (2 * h)
        Lp, Lm = p['q'] + np.einsum('brc,br->bc', p['G'], l), q['q'] + np.einsum('brc,br->bc', q['G'], l)
        Qfd[:, :, c] = (Lp - Lm) / (2 * h)
    dG = np.abs(o['G'][:, ie] - Gfd[:, ie]).max() / np.abs(o['G']).max()
    dQ = np.abs(o['Q'] - Qfd).max() / np.abs(o['Q']).max()
    print(f'{kind}: edge rows of G against differences {dG:.2e}, Q against differences {dQ:.2e}; |G edge| max {np.abs(o["G"][:, ie]).max():.3f}')
    assert np.abs(o['G'][:, ie]).max() > 1e-3 and dG <= 1e-6 and dQ <= 1e-5


def test_solves_respect_the_edges(oracle):
    """The window s in [472, 484] m is where the track is narrowest (0.54 m; the constant bound is 0.596 m).  Precondition, asserted: the host
    rollout (the CPU oracle's dynamics) of at least one warm start crosses w - margin."""
    import closed_loop_checks as clc
    import ltv_mpc_checks as chk
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=10, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=tf.f1_raceline(), s_range=(472, 484), edges='track')
    s = DGSQP(*g.solver_args(), print_method=None)
    rows = tw.row_table(s._problem)
    assert len(rows) == s.n_c_total and sum(r[0].startswith('edge') for r in rows) == 40 and not any(r[0].startswith('st_') for r in rows)
    batch = s.sample_raceline_batch(g, 16, seed=2)
    t = g.track
    edge_max = lambda x: max((-(t.right_width(x[..., 6]) - 0.1) - x[..., 7]).max(), (x[..., 7] - (t.left_width(x[..., 6]) - 0.1)).max())
    crossing = 0
    for b in range(16):
        for a in range(2):
            q = chk.rollout(chk.oracle_dyn(oracle, s._problem, a), batch['x0'][b, 8 * a:8 * a + 8], batch['u_ws'][b, :, 2 * a:2 * a + 2])
            crossing += bool(edge_max(q[1:]) > 0)
    print(f'{crossing} of 32 warm-start rollouts cross w - margin')
    assert crossing >= 1
    r1, r2 = s.solve_batch(batch['x0'], batch['u_ws']), s.solve_batch(batch['x0'], batch['u_ws'])
    for key in ('status', 'num_iters', 'qp_solves'):
        assert np.array_equal(r1[key], r2[key]), key
    for key in ('u', 'l', 'x'):
        assert np.array_equal(r1[key], r2[key], equal_nan=True), key
    conv = r1['converged']
    print(f'converged {int(conv.sum())} of 16; status {r1["status"].tolist()}')
    assert conv.any()
    worst = edge_max(r1['x'][conv].reshape(-1, 11, 2, 8)[:, 1:])
    ie = [i for i, r in enumerate(rows) if r[0].startswith('edge')]
    lmax = r1['l'][conv][:, ie].max()
    print(f'largest edge value over the converged solves {worst:.3e} (p_tol {g.params.p_tol}); largest edge multiplier {lmax:.3e}')
    assert worst <= g.params.p_tol
    assert lmax > 1e-6
    # three closed-loop steps, teacher-forced: every step is the solve_batch solve from the state and warm start it started from
    res = s.step_batch(batch['x0'], batch['u_ws'], 3, keep_predictions=True)
    clc.check_feedback(s, res, batch['x0'], s._to_agent_major(np.asarray(batch['u_ws'], float)))
    n = clc.teacher_force(s, res)
    print(f'{n} closed-loop steps teacher-forced')
    assert n >= 16
