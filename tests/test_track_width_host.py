"""Track width functions on the host: ``left_width(s)`` / ``right_width(s)`` / ``width_slopes(s)`` of the track classes against numpy's own
interpolation, the explicit table of arc tracks and its refusals, the width table in ``dgsqp_problem_t`` (layout, what ``build_problem``
passes, what ``dgsqp_plan`` refuses), and the numpy mirror of the F1 study's e_y clip.  No GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import track_frame_checks as tf


def f1_table(track):
    return track.knots - track.knots[0], track.left_width_points, track.right_width_points


def test_f1_widths_against_numpy_interp():
    """1,000 points from -1.3 L to 2.4 L (negative s and s > L included): the value against np.interp on the wrapped s to 1e-15, the slope
    against the table's divided differences exactly, and a knot belongs to the piece on its right."""
    t = tf.f1_track()
    k, l, r = f1_table(t)
    L = t.track_length
    assert len(k) == 1103 and k[0] == 0.0 and k[-1] == L
    print(f'left {l.min():.4f} .. {l.max():.4f}, right {r.min():.4f} .. {r.max():.4f}, half_width {t.half_width:.4f}')
    assert abs(min(l.min(), r.min()) - 0.54) < 0.01 and abs(max(l.max(), r.max()) - 1.40) < 0.01
    s = np.random.default_rng(0).uniform(-1.3 * L, 2.4 * L, 1000)
    assert (s < 0).sum() > 100 and (s > L).sum() > 100
    sb = np.fmod(np.fmod(s, L) + L, L)
    for fn, w in ((t.left_width, l), (t.right_width, r)):
        err = np.abs(fn(s) - np.interp(sb, k, w)).max()
        print(f'{fn.__name__}: max |value - np.interp| {err:.2e}')
        assert err <= 1e-15
    i = np.searchsorted(k, sb, side='right') - 1
    assert (i >= 0).all() and (i <= len(k) - 2).all()
    dl, dr = t.width_slopes(s)
    assert np.array_equal(dl, (l[i + 1] - l[i]) / (k[i + 1] - k[i])) and np.array_equal(dr, (r[i + 1] - r[i]) / (k[i + 1] - k[i]))
    # at a knot: the value is the table's, the slope is the piece's that starts there; just before it, the piece's that ends there
    # (the wrap (s mod L + L) mod L rounds, so this is checked at the knots the wrap returns unchanged, and there are plenty)
    at = [j for j in range(1, len(k) - 1) if t._sbar(k[j]) == k[j]]
    assert len(at) >= 100
    for j in at:
        assert t.left_width(k[j]) == l[j] and t.right_width(k[j]) == r[j]
        assert t.width_slopes(k[j])[0] == (l[j + 1] - l[j]) / (k[j + 1] - k[j])
    before = [j for j in at if t._sbar(np.nextafter(k[j], 0.0)) < k[j]]
    assert len(before) >= 10
    for j in before:
        assert t.width_slopes(np.nextafter(k[j], 0.0))[0] == (l[j] - l[j - 1]) / (k[j] - k[j - 1])
    assert t.left_width(0.0) == l[0] and t.left_width(L) == l[0] and t.left_width(-L) == l[0]          # wrapped
    assert isinstance(float(t.left_width(3.0)), float) and t.left_width(np.array([1.0, 2.0])).shape == (2,)
    # in the study's window, s in [60, 80] m, the left edge alone moves between 0.63 m and 1.40 m (half_width: 0.696 m)
    w = t.left_width(np.linspace(60, 80, 2001))
    assert abs(w.min() - 0.631) < 0.005 and abs(w.max() - 1.403) < 0.005


def test_arc_tracks_constant_widths_and_an_explicit_table():
    tracks = tf.arc_tracks()
    t = tracks['curve']
    L = t.track_length
    s = np.linspace(-L, 2 * L, 50)
    assert t.width_table() is None
    assert np.array_equal(t.left_width(s), np.full(50, t.half_width)) and np.array_equal(t.right_width(s), np.full(50, t.half_width))
    assert t.left_width(1.0) == t.half_width and all((v == 0).all() for v in t.width_slopes(s))
    k = np.array([0.0, 0.3 * L, 0.45 * L, 0.8 * L, L])
    l, r = np.array([1.0, 0.8, 0.83, 1.1, 0.9]), np.array([0.7, 0.9, 0.85, 0.6, 0.75])
    assert t.set_width_table(k, l, r) is t
    assert np.array_equal(t.width_table(), np.stack([k, l, r], axis=1)) and t.width_table().flags.c_contiguous
    sb = np.fmod(np.fmod(s, L) + L, L)
    assert np.abs(t.left_width(s) - np.interp(sb, k, l)).max() <= 1e-15 and np.abs(t.right_width(s) - np.interp(sb, k, r)).max() <= 1e-15
    dl, dr = t.width_slopes(np.array([0.1 * L, 0.4 * L, 0.9 * L - 3 * L]))
    assert np.array_equal(dl, [(l[1] - l[0]) / (k[1] - k[0]), (l[2] - l[1]) / (k[2] - k[1]), (l[4] - l[3]) / (k[4] - k[3])])
    assert np.array_equal(dr, [(r[1] - r[0]) / (k[1] - k[0]), (r[2] - r[1]) / (k[2] - k[1]), (r[4] - r[3]) / (k[4] - k[3])])
    k[1] = 99.0                                     # the track keeps a copy
    assert t.width_table()[1, 0] == 0.3 * L


def test_set_width_table_refusals():
    from dgsqp_amd import _ffi
    t = tf.arc_tracks()['curve']
    L = t.track_length
    k, w = np.array([0.0, 0.5 * L, L]), np.array([1.0, 0.9, 1.0])
    for knots, left, right, word in (
            (k + 0.1, w, w, 'from 0 to the track length'), (np.array([0.0, 0.5 * L, 0.99 * L]), w, w, 'from 0 to the track length'),
            (np.array([0.0, 0.5 * L, 0.5 * L, L]), np.ones(4), np.ones(4), 'increase strictly'),
            (np.array([0.0, 0.6 * L, 0.5 * L, L]), np.ones(4), np.ones(4), 'increase strictly'),
            (k, np.array([1.0, 0.0, 1.0]), w, 'positive'), (k, w, np.array([1.0, -0.2, 1.0]), 'positive'),
            (k, np.array([1.0, np.nan, 1.0]), w, 'non-finite'), (np.array([0.0, np.inf, L]), w, w, 'non-finite'),
            (k, w[:2], w, 'one length'), (k[:1], w[:1], w[:1], 'one length'), (k.reshape(1, 3), w, w, 'one length'),
            (np.linspace(0, L, _ffi.MAX_KNOTS + 1), np.ones(_ffi.MAX_KNOTS + 1), np.ones(_ffi.MAX_KNOTS + 1), 'limit')):
        with pytest.raises(ValueError, match='width table: .*' + word):
            t.set_width_table(knots, left, right)
    assert t.width_table() is None                                  # nothing was kept
    t.set_width_table(np.linspace(0, L, _ffi.MAX_KNOTS), np.ones(_ffi.MAX_KNOTS), np.ones(_ffi.MAX_KNOTS))


def test_struct_layouts(tmp_path):
    """The records against the header, from a compiled C program: dgsqp_agent_t grew by the 16 appended bytes of the edge rows, dgsqp_problem_t by
    six times that and by the 16 bytes of the appended table fields; the tracker's and the sampler's records keep their sizes."""
    from dgsqp_amd import _ffi
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dgsqp.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(dgsqp_agent_t), '
           'sizeof(dgsqp_problem_t), sizeof(dgsqp_mpc_t), sizeof(dgsqp_raceline_spline_sampler_t), offsetof(dgsqp_problem_t, spline), '
           'offsetof(dgsqp_problem_t, n_width), offsetof(dgsqp_problem_t, widths));return 0;}\n')
    exe = tmp_path / 'sizes'
    subprocess.run(['gcc', '-x', 'c', '-', '-I', str(tf.ROOT / 'include'), '-o', str(exe)], input=src.encode(), check=True)
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P = _ffi.ProblemT
    assert sizes == [ctypes.sizeof(_ffi.AgentT), ctypes.sizeof(P), ctypes.sizeof(_ffi.MpcT), ctypes.sizeof(_ffi.RacelineSplineSamplerT),
                     P.spline.offset, P.n_width.offset, P.widths.offset]
    assert sizes == [736, 4888, 552, 56, 4864, 4872, 4880]          # (the agent record: 720 + edge_rows, _pad3, edge_margin)


def test_build_problem_passes_the_table():
    """The F1 track always has one; an arc track after set_width_table; every other game passes n_width = 0.  The record of f1_racing_game()
    is, before the appended fields, byte for byte the record of the same game without a table."""
    from dgsqp_amd import _ffi, montecarlo as mc
    from dgsqp_amd.solver import build_problem, plan, build_params
    g = mc.f1_racing_game()
    P = build_problem(*g.solver_args())
    assert P.n_width == 1103 and P.widths == P._widths_keepalive.ctypes.data
    k, l, r = f1_table(g.track)
    assert np.array_equal(P._widths_keepalive, np.stack([k, l, r], axis=1)) and P._widths_keepalive.flags.c_contiguous
    assert P.track_L == k[-1]
    d = plan(P, build_params(g.params))
    g0 = mc.f1_racing_game()
    g0.track.clear_width_table()
    P0 = build_problem(*g0.solver_args())
    assert P0.n_width == 0 and P0.widths == 0
    cut, ptr = _ffi.ProblemT.n_width.offset, _ffi.ProblemT.spline.offset
    assert bytes(P)[:ptr] == bytes(P0)[:ptr] and cut == ptr + 8          # (between them: the address of the spline table)
    assert plan(P0, build_params(g0.params)) == d                        # the plan does not depend on the table
    arc = mc.kinematic_racing_game('curve', N=4)
    assert build_problem(*arc.solver_args()).n_width == 0
    L = arc.track.track_length
    arc.track.set_width_table([0.0, 0.4 * L, L], [1.0, 0.8, 1.0], [0.9, 1.0, 0.9])
    Pa = build_problem(*arc.solver_args())
    assert Pa.n_width == 3 and np.array_equal(Pa._widths_keepalive[:, 0], [0.0, 0.4 * L, L])
    assert bytes(Pa)[:cut] == bytes(build_problem(*mc.kinematic_racing_game('curve', N=4).solver_args()))[:cut]
    assert build_problem(*mc.merge_game(N=4).solver_args()).n_width == 0          # a game without a track


def test_plan_refuses_a_bad_table():
    """dgsqp_plan validates the table as dgsqp_create does: every refusal with its 'widths: ' message."""
    from dgsqp_amd import _ffi, montecarlo as mc
    from dgsqp_amd.solver import build_problem, plan, build_params
    g = mc.kinematic_racing_game('curve', N=4)
    L = g.track.track_length
    par = build_params(g.params)
    good = np.array([[0.0, 1.0, 0.9], [0.4 * L, 0.8, 1.0], [L, 1.0, 0.9]])

    def refused(table, word, n=None):
        P = build_problem(*g.solver_args())
        tab = np.ascontiguousarray(table, dtype=float) if table is not None else None
        P.n_width, P.widths = (len(tab) if n is None else n), (tab.ctypes.data if tab is not None else 0)
        with pytest.raises(ValueError, match=r'\(-1\): widths: .*' + word):
            plan(P, par)
    P = build_problem(*g.solver_args())
    P.n_width, P.widths = 3, good.ctypes.data
    plan(P, par)
    refused(good, 'n_width', n=1)
    refused(good, 'n_width', n=-3)
    refused(good, 'n_width', n=_ffi.MAX_KNOTS + 1)
    refused(None, 'without a table', n=3)
    for i, j, v, word in ((0, 0, 0.1, 'from 0 to track_L'), (2, 0, 0.999 * L, 'from 0 to track_L'), (1, 0, 0.0, 'increase strictly'),
                          (1, 0, np.nan, 'non-finite'), (1, 2, np.inf, 'non-finite'), (0, 1, 0.0, 'positive'), (2, 2, -1.0, 'positive')):
        bad = good.copy()
        bad[i, j] = v
        refused(bad, word)
    refused(np.array([[0.0, 1, 1], [0.5 * L, 1, 1], [0.5 * L, 1, 1], [L, 1, 1]]), 'increase strictly')


def clip_game(clip='track', **kw):
    from dgsqp_amd import montecarlo as mc
    return mc.f1_racing_game(N=10, model='dynamic', rk4_substeps=2, sampler='raceline', raceline=kw.pop('raceline', None) or tf.f1_raceline(),
                             s_range=(60, 80), edges=clip, **kw)


def test_sampler_mirror_clip():
    """sampler.place_raceline on the B = 300, seed 11 batch of the study's window.  Default: the draws of the constant clip, restated here
    from the uniforms.  edges='track': every e_y lies within 0.9 x the widths at its own s, the draws differ from the constant
    clip's only in e_y (and the positions made from it), and some draw sits ON a scaled width that is not 0.9 x half_width."""
    from dgsqp_amd import sampler as smp
    rl = tf.f1_raceline()
    g0, g1 = clip_game('constant', raceline=rl), clip_game('track', raceline=rl)
    assert (g0.clip_widths, g1.clip_widths) == (False, True) and smp.raceline_clip(g0) == (0, 0.0) and smp.raceline_clip(g1) == (1, 0.9)
    assert ctypes.sizeof(smp.raceline_spline_sampler_spec(g1, 11)) == 56
    cand = np.arange(300, dtype=np.uint64)
    x0, m0 = smp.place_raceline(g0, 11, cand)
    x1, m1 = smp.place_raceline(g1, 11, cand)
    t, lim = g0.track, 0.9 * g0.half_width
    n_on_width = 0
    for a in range(2):
        s, ey0, ey1 = x0[:, 8 * a + 6], x0[:, 8 * a + 7], x1[:, 8 * a + 7]
        raw = rl.eval(rl.s2t(s))[:, 8] + (2 * smp.uniform(11, cand, 3 * a + 1) - 1)
        assert np.array_equal(ey0, np.maximum(np.minimum(raw, lim), -lim))                  # today's law
        hi, lo = 0.9 * t.left_width(s), -0.9 * t.right_width(s)
        assert np.array_equal(ey1, np.maximum(np.minimum(raw, hi), lo)) and (ey1 <= hi).all() and (ey1 >= lo).all()
        on = ((ey1 == hi) & (np.abs(hi - lim) > 1e-3)) | ((ey1 == lo) & (np.abs(lo + lim) > 1e-3))
        n_on_width += int(on.sum())
        same = [8 * a + c for c in (2, 3, 4, 5, 6)]
        assert np.array_equal(x0[:, same], x1[:, same])
        print(f'car {a + 1}: {int((ey0 != ey1).sum())} of 300 draws change, {int(on.sum())} sit on a scaled width; widths seen '
              f'{t.left_width(s).min():.3f} .. {t.left_width(s).max():.3f} (left), {t.right_width(s).min():.3f} .. {t.right_width(s).max():.3f} (right)')
    assert n_on_width >= 1
    assert not np.array_equal(m0, m1)


def test_python_side_refusals():
    from dgsqp_amd import montecarlo as mc
    with pytest.raises(ValueError, match='edges'):
        mc.f1_racing_game(N=5, edges='widths')
    assert mc.f1_racing_game(N=5).clip_widths is False
    # the sequential host sampler follows the same switch
    rl = tf.f1_raceline()
    g1 = clip_game('track', raceline=rl)
    t = g1.track
    rng = np.random.default_rng(0)
    for _ in range(50):
        x, _ = mc.place_raceline_sequential(g1, rng)
        for a in range(2):
            s, ey = x[8 * a + 6], x[8 * a + 7]
            assert -0.9 * t.right_width(s) <= ey <= 0.9 * t.left_width(s)


def test_tracker_edge_rows_python_surface():
    """ltv_mpc.TrackEdgeRows lowers to dgsqp_mpc_t.edge_rows (the field that was reserved_: the record keeps its 552 bytes), the study tracker
    with track_constraints opens its e_y box and carries the record, raceline_ws passes it on, and what cannot work raises before a handle
    exists."""
    from dgsqp_amd import _ffi, ltv_mpc, montecarlo as mc
    assert _ffi.MPC_ROW_EDGE == 6 and 'DGSQP_MPC_ROW_EDGE = 6' in (tf.ROOT / 'include' / 'dgsqp.h').read_text()
    assert _ffi.MpcT.edge_rows.offset == _ffi.MpcT.n_soft.offset + 4 and _ffi.MpcT.edge_rows.size == 4
    cost = ltv_mpc.TrackingCost(state_weight=np.ones(6))
    args = (np.ones(6), -np.ones(6), (1, 1), (-1, -1), (1, 1), (-1, -1), 3, 2, 0.75)
    assert ltv_mpc.lower(0, 6, cost, None, None, *args).edge_rows == 0
    assert ltv_mpc.lower(0, 6, cost, None, None, *args, track_edges=ltv_mpc.TrackEdgeRows()).edge_rows == 1
    with pytest.raises(TypeError, match='TrackEdgeRows'):
        ltv_mpc.lower(0, 6, cost, None, None, *args, track_edges=True)
    rl = tf.f1_raceline()
    g0 = mc.f1_racing_game(N=5, model='dynamic', sampler='raceline', raceline=rl)
    g1 = mc.f1_racing_game(N=5, model='dynamic', sampler='raceline', raceline=rl, edges='track')
    assert (g0.clip_widths, g0.tracker_edges, g1.clip_widths, g1.tracker_edges) == (False, False, True, True)
    t0, t1 = mc.study_tracker(g0), mc.study_tracker(g1)
    assert t0['track_edges'] is None and (t0['bounds']['qu_ub'].p.x_tran, t0['bounds']['qu_lb'].p.x_tran) == (g0.half_width, -g0.half_width)
    assert isinstance(t1['track_edges'], ltv_mpc.TrackEdgeRows) and (t1['bounds']['qu_ub'].p.x_tran, t1['bounds']['qu_lb'].p.x_tran) == (1e9, -1e9)
    assert isinstance(mc.study_tracker(g0, track_constraints=True)['track_edges'], ltv_mpc.TrackEdgeRows)
    assert mc.study_tracker(g1, track_constraints=False)['track_edges'] is None
    W0, W1 = mc.raceline_ws(g0), mc.raceline_ws(g1)
    assert (W0.mpc.edge_rows, W1.mpc.edge_rows) == (0, 1) and abs(W1.mpc.q_ub[7]) >= 1e9 and W0.mpc.q_ub[7] == g0.half_width
    for name, *_ in _ffi.MpcT._fields_:          # nothing else in the record moves
        if name not in ('edge_rows', 'q_ub', 'q_lb'):
            a, b = getattr(W0.mpc, name), getattr(W1.mpc, name)
            assert (list(a) == list(b)) if hasattr(a, '__len__') else a == b, name
    # the BARC study on an arc track: constant widths, no table -- the rows have nothing to read
    import raceline_checks as rc
    barc = rc.dynamic_game()
    with pytest.raises(ValueError, match='width table'):
        mc.study_tracker(barc, track_constraints=True)
    # the class surface
    mdl = g1.joint_model.dynamics_models[0]
    bounds = t1['bounds']
    with pytest.raises(NotImplementedError, match='track_edges'):
        ltv_mpc.CA_LTV_MPC(mdl, t1['cost'], {'track_edges': 0.5}, bounds, t1['params'], print_method=None)
    with pytest.raises(ValueError, match='width table'):
        ltv_mpc.CA_LTV_MPC(barc.joint_model.dynamics_models[0], t1['cost'], {'track_edges': ltv_mpc.TrackEdgeRows()}, bounds, t1['params'], print_method=None)
    with pytest.raises(NotImplementedError, match='unknown constraint entries'):
        ltv_mpc.CA_LTV_MPC(mdl, t1['cost'], {'edges': None}, bounds, t1['params'], print_method=None)


def test_game_edge_rows_lowering_order_and_refusals():
    """game.TrackEdges through build_problem: the appended agent fields, the host row count against dgsqp_plan, the (type, stage, agent)
    order of the edge rows of a two-car N = 3 game, f1_racing_game(edges=...), and every refusal before the library."""
    import track_width_checks as tw
    from dgsqp_amd import _ffi, montecarlo as mc
    from dgsqp_amd.game import InputRateLimits, LaneBoundaries, TrackEdges, constraint_records
    from dgsqp_amd.solver import build_params, build_problem, plan, problem_dims
    g = tw.edge_game(N=3, table=([0.0, 0.4], [1.0, 0.8, 0.9], [0.9, 0.7, 0.9]), margin=0.1)
    P = build_problem(*g.solver_args())
    assert [(P.agents[a].edge_rows, P.agents[a].edge_margin, P.agents[a].has_rate) for a in range(2)] == [(1, 0.1, 1)] * 2
    assert _ffi.AgentT.edge_rows.offset == 720 and _ffi.AgentT.edge_margin.offset == 728
    rows = tw.row_table(P)
    d = plan(P, build_params(g.params))
    assert len(rows) == problem_dims(P)[3] == d['n_c']
    per_stage = {k: [(t, a) for t, kk, a, _ in rows if kk == k and t != 'obs'] for k in range(4)}
    assert [r for r in per_stage[0] if r[0].startswith('edge')] == []                       # x_0 is fixed
    for k in (1, 2):
        want = []
        for a in range(2):
            want += [('rate_ub', a), ('rate_lb', a)] * 2 + [('edge_r', a), ('edge_l', a)] + [('in_ub', a)] * 2 + [('in_lb', a)] * 2
        assert per_stage[k] == want, per_stage[k]
    assert per_stage[3] == [('edge_r', 0), ('edge_l', 0), ('edge_r', 1), ('edge_l', 1)]
    box = tw.edge_game(N=3, box=0.9, margin=0.1)
    dbox = plan(build_problem(*box.solver_args()), build_params(box.params))
    assert d['n_c'] == dbox['n_c'] and d['n_dense'] == dbox['n_dense'] + 2 * 3          # two dense gradients per (agent, stage) where the box has one
    # the F1 game
    f0, f1 = mc.f1_racing_game(N=5), mc.f1_racing_game(N=5, edges='track')
    assert isinstance(f0.agent_constraints[0], InputRateLimits) and [type(r) for r in f1.agent_constraints[0]] == [InputRateLimits, TrackEdges]
    assert f1.agent_constraints[1][1].margin == 0.1 and (f1.clip_widths, f1.tracker_edges) == (False, False)      # (the circuit sampler reads no widths)
    P1 = build_problem(*f1.solver_args())
    assert P1.agents[0].edge_rows == 1 and P1.agents[0].st_ub[5] == np.inf and build_problem(*f0.solver_args()).agents[0].edge_rows == 0
    with pytest.raises(ValueError, match="edges"):
        mc.f1_racing_game(N=5, edges='yes')
    # refusals
    arc = mc.kinematic_racing_game('curve', N=3)
    arc.agent_constraints = [[InputRateLimits(), TrackEdges(0.1)], InputRateLimits()]
    with pytest.raises(ValueError, match='TrackEdges: the track has no width table'):
        build_problem(*arc.solver_args())
    merge = mc.merge_game(N=3)
    merge.agent_constraints = [TrackEdges()] + list(merge.agent_constraints[1:])
    with pytest.raises(ValueError, match='TrackEdges: agent 0 has no'):
        build_problem(*merge.solver_args())
    g.agent_constraints = [[TrackEdges(0.1), TrackEdges(0.2)], None]
    with pytest.raises(ValueError, match='at most one record of each kind'):
        build_problem(*g.solver_args())
    g.agent_constraints = [[TrackEdges(np.nan)], None]
    with pytest.raises(ValueError, match='margin must be finite'):
        build_problem(*g.solver_args())
    with pytest.raises(TypeError, match='unknown record'):
        constraint_records([3.0])
    g.agent_constraints = [[InputRateLimits(), LaneBoundaries([])], None]
    with pytest.raises(ValueError, match='exclude one another'):
        build_problem(*g.solver_args())
    # the library's own refusals (dgsqp_plan): a game without a table, a bad flag
    P2 = build_problem(*tw.edge_game(N=3, table=([0.0], [1.0, 1.0], [1.0, 1.0])).solver_args())
    P2.n_width = 0
    with pytest.raises(ValueError, match='edge rows: the game has no width table'):
        plan(P2, build_params(g.params))
    P.agents[1].edge_rows = 2
    with pytest.raises(ValueError, match='edge rows: edge_rows must be 0 or 1'):
        plan(P, build_params(g.params))


def test_edge_fixtures_and_the_generator_on_a_constant_table():
    """The two fixtures with edge rows load (every parameter against the record build_problem makes, the positions of the edge rows, the
    accuracy record, the breakpoint margin, a multiplier on every edge row, at least two pieces of the table).  And the generator itself:
    tools/make_track_edge_kats.py on the committed kin2_euler_N3 case with a CONSTANT table W = 1.5 and margin 0.5 (W - margin = 1.0, the
    half width of that case, both exact in binary) in place of the e_y box reproduces the parent generator's g (matched rows), q, G and Q
    to 1e-17 of the largest entry, on the unrounded values (hi + lo): scenario 0 in full, scenario 1 x, g, q."""
    import sys
    import track_width_checks as tw
    sys.path.insert(0, str(tf.ROOT / 'tools'))
    import make_track_edge_kats as gen
    base = gen.base
    for case in tw.KAT_CASES:
        kat, g, P = tw.load_edge_case(case)
        assert (kat['l'][:, kat['edge_rows']] >= 0.1).all() and len(kat['edge_rows']) == 12
        nqa = kat['x'].shape[2] // 2
        sb = kat['x'][:, 1:, [nqa - 2, 2 * nqa - 2]]
        kn = kat['p_track_widths'][:, 0]
        assert len({int(i) for i in (np.searchsorted(kn, sb, side='right') - 1).ravel()}) >= 2 and np.abs(sb[..., None] - kn).min() >= 1e-3
        slopes = np.diff(kat['p_track_widths'][:, 1:], axis=0) / np.diff(kn)[:, None]
        assert len(kn) == 5 and np.abs(slopes).max() <= 0.3 and not np.array_equal(kat['p_track_widths'][:, 1], kat['p_track_widths'][:, 2])
    par = np.load(tf.ROOT / 'tests' / 'golden' / 'multistage_kin2_euler_N3.npz')
    spec = base.unflatten_spec(par)
    W, m = 1.5, 0.5
    L = spec['track']['L']
    edges = gen.with_edges(spec, [[0.0, W, W], [L, W, W]], m)
    ie = gen.edge_row_index(edges)
    # rows of the parent: the e_y boxes of stage k sit at the end of each agent's block; match them through the package's own row table
    from dgsqp_amd import montecarlo as mc
    from dgsqp_amd.solver import build_problem
    import multistage_kat as mk
    rb = tw.row_table(build_problem(*mk.build_game('kin2_euler_N3').solver_args()))
    ge = tw.build_edge_case('kin2_edges_euler_N3', table=np.array([[0.0, W, W], [L, W, W]]), margin=m)
    re_ = tw.row_table(build_problem(*ge.solver_args()))
    assert [i for i, r in enumerate(re_) if r[0].startswith('edge')] == ie
    match = {('edge_l', k, a, 1): ('st_ub', k, a, 5) for k in range(1, 4) for a in range(2)}
    match.update({('edge_r', k, a, 0): ('st_lb', k, a, 5) for k in range(1, 4) for a in range(2)})
    perm = np.array([rb.index(match.get(r, r)) for r in re_])
    assert sorted(perm) == list(range(len(rb)))
    tot = lambda v: v[0].astype(np.longdouble) + v[1]
    for b, full in ((0, True), (1, False)):
        want, mg0 = base.answers(spec, par['x0'][b], par['u'][b], par['l'][b], 60, 20, full=full)
        got, mg1 = gen.base.answers(edges, par['x0'][b], par['u'][b], par['l'][b][perm], 60, 20, full=full)
        assert mg1[0] > 1e-3
        for k in ('x', 'g', 'q') + (('G', 'Q') if full else ()):
            w = tot(want[k])[perm] if k in ('g', 'G') else tot(want[k])
            err = float(np.abs(tot(got[k]) - w).max() / np.abs(w).max())
            print(f'scenario {b} {k}: {err:.1e} of the largest entry')
            assert err <= 1e-17, (b, k, err)
