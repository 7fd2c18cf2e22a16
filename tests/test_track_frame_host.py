"""Track-frame transforms, the host side (no GPU): the numpy mirrors of csrc/dgsqp_track_frame.h -- round trips on the F1 spline and on
the arc tracks, the seams, the TUM raceline loader on the study's file, and the refusals that need no device."""
import ctypes

import numpy as np
import pytest

import track_frame_checks as tf


def test_mirror_round_trip_f1():
    """2,000 seeded points: Frenet -> global -> Frenet at the bars of track_frame_checks."""
    from dgsqp_amd import tracks
    t = tf.f1_track()
    assert t.circuit
    cl = tf.round_trip_points(t)
    xy = tracks.local_to_global_batch(t, cl)
    got, resid, status = tracks.global_to_local_batch(t, xy)
    tf.assert_round_trip(t, cl, got, resid, status, 'F1 mirror')
    # the batch helper against the scalar method (hypot against sqrt of the sum: the last place), one point and many through the methods
    ref = np.array([t.local_to_global(tuple(c)) for c in cl[:64]])
    assert np.abs(xy[:64] - ref).max() <= 1e-13
    one = t.global_to_local(tuple(xy[5]))
    assert isinstance(one, tuple) and one == tuple(got[5])
    assert np.array_equal(t.global_to_local(xy[:7]), got[:7])


def test_seams():
    """K_i -+ 1e-9 for the first, a middle and the last piece and s in {0, 1e-9, L - 1e-9}, e_y = -+0.3: the bars of the round trip.  At the
    start line the table has a kink of 8.66e-7 rad, and the points on its inner side have two foot points: see
    track_frame_checks.assert_round_trip for what is asserted there (measured: (L - 1e-9, -0.3) comes back as s = 2.59e-7, the closer one).
    The points at the middle seams and on the outer side of the kink meet every bar."""
    from dgsqp_amd import tracks
    t = tf.f1_track()
    cl = tf.seam_points(t)
    assert len(cl) == 26
    got, resid, status = tracks.global_to_local_batch(t, tracks.local_to_global_batch(t, cl))
    tf.assert_round_trip(t, cl, got, resid, status, 'F1 seams', start_line_kink=True)
    outer = (tf.circ(cl[:, 0], t.track_length) <= 1e-6) & (cl[:, 1] > 0)          # e_y = +0.3 is the outer side: one foot point
    assert outer.sum() == 7 and tf.circ(got[outer, 0] - cl[outer, 0], t.track_length).max() <= tf.BAR_S


@pytest.mark.parametrize('name', ['L_track_barc', 'chicane', 'curve'])
def test_arc_tracks(name):
    from dgsqp_amd import tracks
    t = tf.arc_tracks()[name]
    cl = tf.round_trip_points(t, n=256, seed=1, ey_frac=1.0)
    xy = tracks.local_to_global_batch(t, cl)
    ref = np.array([t.local_to_global(tuple(c)) for c in cl])
    assert np.abs(xy - ref).max() <= 1e-13                       # the vectorised restatement of the scalar method
    got, resid, status = tracks.global_to_local_batch(t, xy)
    tf.assert_round_trip(t, cl, got, resid, status, name)
    far = (xy[0, 0] + 10 * t.track_width, xy[0, 1] + 10 * t.track_width, 0.0)
    assert t.global_to_local(far) is None
    many = t.global_to_local(np.array([far, xy[1]]))
    assert np.isnan(many[0]).all() and np.array_equal(many[1], got[1])
    assert tracks.global_to_local_batch(t, np.array([far]))[2].tolist() == [2]
    # exactly on a key point (the last one of a circuit is, to rounding, the first: segment 1 comes first in the order and takes it)
    for i in (0, 1, t.key_pts.shape[0] - 2):
        s, ey, _ = t.global_to_local((t.key_pts[i, 0], t.key_pts[i, 1], 0.2))
        assert ey == 0.0 and s == t.key_pts[i, 3]


def test_typed_and_non_finite():
    from dgsqp_amd import tracks
    from dgsqp_amd.types import OrientationEuler, ParametricPose, Position, VehicleState
    for t in (tf.f1_track(), tf.arc_tracks()['L_track_barc']):
        st = VehicleState(p=ParametricPose(s=3.0, x_tran=0.2, e_psi=0.1))
        t.local_to_global_typed(st)
        back = VehicleState(x=Position(x=st.x.x, y=st.x.y), e=OrientationEuler(psi=st.e.psi))
        t.global_to_local_typed(back)
        assert abs(back.p.s - 3.0) <= tf.BAR_S and abs(back.p.x_tran - 0.2) <= tf.BAR_EY and abs(back.p.e_psi - 0.1) <= tf.BAR_EPSI
        xy = tracks.local_to_global_batch(t, tf.round_trip_points(t, n=8))
        bad = xy.copy()
        bad[2, 0], bad[5, 2] = np.nan, np.inf
        cl, resid, status = tracks.global_to_local_batch(t, bad)
        ref = tracks.global_to_local_batch(t, xy)
        assert status.tolist() == [0, 0, 1, 0, 0, 1, 0, 0] and np.isnan(cl[[2, 5]]).all() and np.isnan(resid[[2, 5]]).all()
        keep = [0, 1, 3, 4, 6, 7]
        assert np.array_equal(cl[keep], ref[0][keep]) and np.array_equal(resid[keep], ref[1][keep])


def test_tum_loader_on_the_fixture():
    from dgsqp_amd import tracks
    from DGSQP.tracks.track_lib import load_tum_raceline
    assert load_tum_raceline is tracks.load_tum_raceline
    raceline, s2t, lap_mat = load_tum_raceline(tf.TUM_FIXTURE, tf.F1, tenth_scale=True)
    R = raceline.table
    L = tf.f1_track().track_length
    assert lap_mat.shape == (2721, 9) and R.T.shape == (2 * 2721 - 1,) and R.cols.shape == (2 * 2721 - 1, 9)
    assert (np.diff(R.T) > 0).all() and (np.diff(R.cols[:, 7]) > 0).all()
    raw = tracks.global_to_local_batch(tf.f1_track(), lap_mat[:, :3])[0][:, 0]           # the projections before the + L rule
    assert int((np.diff(raw) < 0).sum()) == 1
    assert np.array_equal(lap_mat[:, 7], np.where(np.arange(2721) > int(np.argmax(np.diff(raw) < 0)), raw + L, raw))
    assert np.array_equal(R.cols[2721:, 7], lap_mat[1:, 7] + L)
    assert np.abs(s2t(lap_mat[:, 7]) - R.lap_T).max() <= 1e-9
    assert np.abs(R.projection_resid).max() <= 1e-10 and (R.projection_status == 0).all()
    print(f'max |e_y| of the line {np.abs(lap_mat[:, 8]).max():.6f}, v {lap_mat[:, 3].min():.3f} .. {lap_mat[:, 3].max():.3f} m/s, lap time {R.lap_T[-1]:.3f} s')
    assert abs(np.abs(lap_mat[:, 8]).max() - 0.7708) <= 1e-3
    # columns: x, y scaled by 0.1, psi + pi / 2, v = vx / 10; T the cumulative sum of ds_file / v
    import gzip
    import hashlib
    raw = gzip.open(tf.TUM_FIXTURE).read()          # the study's traj_race_cl.csv byte for byte, kept gzipped (233,019 B of text otherwise)
    assert len(raw) == 233019 and hashlib.sha256(raw).hexdigest() == 'c4039b044496f7373b4e2240cb886419f54edaaa3476cb59b6a5b652b3abb360'
    row = np.array([float(v) for v in raw.decode().splitlines()[3].split(';')])
    assert np.allclose(lap_mat[0, :4], [0.1 * row[1], 0.1 * row[2], row[3] + np.pi / 2, 0.1 * row[5]], rtol=0, atol=1e-15)
    assert abs(R.lap_T[1] - 0.1 * 1.9998958 / lap_mat[0, 3]) <= 1e-12
    v = np.array(raceline(0.5 * R.lap_T[-1]))
    assert v.shape == (9,) and np.array_equal(v, R.eval(0.5 * R.lap_T[-1]))
    half = tracks.load_tum_raceline(tf.TUM_FIXTURE, tf.F1, tenth_scale=True, time_scale=2.0)[0].table
    assert np.allclose(half.lap_mat[:, 3], lap_mat[:, 3] / 2, rtol=1e-15) and np.allclose(half.lap_T, 2 * R.lap_T, rtol=1e-12)
    with pytest.raises(NotImplementedError):
        tracks.load_tum_raceline(tf.TUM_FIXTURE, tf.F1, tenth_scale=True, segment=[60, 80])
    with pytest.raises(NotImplementedError):
        tracks.load_tum_raceline(tf.TUM_FIXTURE, tf.F1, tenth_scale=True, resample_resolution=10)


def test_python_side_refusals_and_surface():
    from dgsqp_amd import _ffi, montecarlo as mc, sampler as smp, tracks
    g = mc.f1_racing_game(N=5)
    spec = smp.sampler_spec(g, 3)
    assert (spec.kind, spec.n_key) == (smp.CIRCUIT, 0)
    for kind in ('first_segment', 'independent'):
        g.sampler = 'first_segment'
        if kind == 'independent':
            g = mc.f1_racing_game(N=5, M=3)
            g.sampler = 'first_segment'
        with pytest.raises(ValueError, match="spline track .*'circuit'"):
            smp.sampler_spec(g, 3)
    barc = mc.barc_racing_game(N=5)
    with pytest.raises(ValueError, match='spline track'):
        smp.raceline_spline_sampler_spec(barc, 1)
    with pytest.raises(ValueError):
        mc.f1_racing_game(N=5, sampler='first_segment')
    with pytest.raises(ValueError, match='raceline='):
        mc.f1_racing_game(N=5, sampler='raceline')
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError, match=r'\[n, 3\]'):
            tracks.local_to_global_batch(g.track, bad)
        with pytest.raises(ValueError, match=r'\[n, 3\]'):
            tracks.global_to_local_batch(g.track, bad)
    with pytest.raises(ValueError):
        g.track.global_to_local((1.0, 2.0))
    # the records and the C-ABI
    assert ctypes.sizeof(_ffi.TrackFrameT) == 8 + 16 + 8 * 6 * (_ffi.MAX_SEGS + 1) and ctypes.sizeof(_ffi.RacelineSplineSamplerT) == 56
    T = tracks.track_frame_spec(g.track)
    assert T.n_key == 0 and T.half_width == g.track.half_width and T.slack == g.track.slack
    T = tracks.track_frame_spec(barc.track)
    assert T.n_key == barc.track.key_pts.shape[0] and T.key_pts[3][3] == barc.track.key_pts[3, 3]
    header = (tf.ROOT / 'include' / 'dgsqp.h').read_text()
    for name in ('dgsqp_local_to_global_batch', 'dgsqp_global_to_local_batch', 'dgsqp_sample_raceline_spline_batch'):
        assert name in _ffi.SIGNATURES and name in _ffi.EXPORTED_SYMBOLS and f'int {name}(' in header, name
    # the F1 study's defaults
    rl = tf.f1_raceline()
    g = mc.f1_racing_game(N=5, model='dynamic', sampler='raceline', raceline=rl)
    S = smp.raceline_spline_sampler_spec(g, 7)
    assert (S.seed, S.s_lo, S.s_hi, S.gap_lo, S.gap_hi) == (7, 0.0, g.track.track_length - 10.0, 0.0, 3 * 0.56)
    assert S.ey_clip == 0.9 * g.half_width and S.collision_d == 2 * np.sqrt(0.28 ** 2 + 0.1 ** 2)
    g = mc.f1_racing_game(N=5, model='dynamic', sampler='raceline', raceline=rl, s_range=(60, 80))
    S = smp.raceline_spline_sampler_spec(g, 7)
    assert (S.s_lo, S.s_hi) == (60.0, 80.0)
    t = mc.study_tracker(g)
    p = t['params']
    assert list(p.state_scaling) == [100, 100, 7, np.pi / 2, g.track.track_length, 1.0] and list(p.input_scaling) == [2, 0.45]
    assert (p.damping, p.qp_iters, p.N) == (0.75, 5, 5)
    b = t['bounds']
    assert (b['du_ub'].u.u_a, b['du_ub'].u.u_steer, b['du_lb'].u.u_a, b['du_lb'].u.u_steer) == (20.0, 4.5, -20.0, -4.5)
    assert (b['qu_ub'].p.x_tran, b['qu_lb'].p.x_tran) == (g.half_width, -g.half_width)
    assert (b['qu_lb'].v.v_long, b['qu_ub'].v.v_long, b['qu_ub'].v.v_tran, b['qu_ub'].w.w_psi, b['qu_ub'].u.u_a, b['qu_ub'].u.u_steer) == (0.1, 5, 2, 10, 2.0, 0.436)
    # the mirror's placement: car 2 ahead of car 1 inside the gap, e_y clipped
    x0, margin = smp.place_raceline(g, 7, np.arange(256))
    gap = x0[:, 14] - x0[:, 6]
    assert x0.shape == (256, 16) and margin.shape == (256,) and (gap >= 0).all() and (gap <= 3 * 0.56).all()
    assert (x0[:, 6] >= 60.0).all() and (x0[:, 6] <= 80.0).all() and (np.abs(x0[:, [7, 15]]) <= S.ey_clip).all()
