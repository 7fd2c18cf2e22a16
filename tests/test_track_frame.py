"""Track-frame transforms on the device (csrc/dgsqp_track_frame.h) against their numpy mirrors (dgsqp_amd/tracks.py): Frenet -> global
and global -> Frenet on the F1 spline and on arc tracks, the seams, non-finite inputs, the 256-thread build and the C-side refusals."""
import ctypes as C

import numpy as np
import pytest

import track_frame_checks as tf

pytestmark = pytest.mark.gpu

BAR_MIRROR = 1e-11          # device against mirror: the polynomial part runs the same operations (the figure printed is usually 0)


@pytest.fixture(scope='module')
def f1():
    """f1_racing_game(N=5) on a handle, 257 of the host test's round-trip points, their global poses and the mirror's projections."""
    from dgsqp_amd import montecarlo as mc, tracks
    from dgsqp_amd.solver import DGSQP
    g = mc.f1_racing_game(N=5)
    s = DGSQP(*g.solver_args(), print_method=None)
    cl = np.ascontiguousarray(tf.round_trip_points(g.track)[:257])
    xy = tracks.local_to_global_batch(g.track, cl)
    return g, s, cl, xy, tracks.global_to_local_batch(g.track, xy)


def psi_bar(track, cl):
    """tests/test_device_math.py holds atan2 to 2.5 ulp; psi = atan2(y', x') + e_psi adds one rounding of a sum whose terms may differ."""
    theta = track.lookup(cl[:, 0])[1]
    return 2.5 * np.spacing(np.abs(theta)) + np.spacing(np.abs(theta) + np.abs(cl[:, 2]))


def against_mirror(dev, mirror, tag):
    (cl, resid, status), (mcl, mresid, mstatus) = dev, mirror
    d = np.abs(cl - mcl).max(axis=0) if len(cl) else np.zeros(3)
    dr = np.abs(resid - mresid).max() if len(cl) else 0.0
    print(f'{tag}: device against mirror |ds| {d[0]:.2e}, |de_y| {d[1]:.2e}, |de_psi| {d[2]:.2e}, |dresid| {dr:.2e}')
    assert np.array_equal(status, mstatus)
    assert d.max() <= BAR_MIRROR and dr <= BAR_MIRROR


@pytest.mark.parametrize('n', [0, 1, 257])
def test_device_against_mirror(f1, n):
    """n = 257: the tail of a second 256-lane block.  local_to_global: coordinates are below 2^7 m, a handful of roundings of at most
    2^-46 m each: |dx|, |dy| <= 1e-12 (the mirror runs the same operations: usually 0); psi at ``psi_bar``.  global_to_local: s, e_y
    (and e_psi, resid) against the mirror at 1e-11, against the truth at the host bars, status identical."""
    g, s, cl, xy, mirror = f1
    dev_xy = s.local_to_global_batch(cl[:n])
    assert dev_xy.shape == (n, 3)
    dev = s.global_to_local_batch(xy[:n])
    assert dev[0].shape == (n, 3) and dev[1].shape == (n,) and dev[2].shape == (n,) and dev[2].dtype == np.int32
    if n == 0:
        return
    dxy = np.abs(dev_xy - xy[:n])
    print(f'n = {n}: local_to_global |dx| {dxy[:, 0].max():.2e}, |dy| {dxy[:, 1].max():.2e}, |dpsi| {dxy[:, 2].max():.2e}')
    assert dxy[:, :2].max() <= 1e-12 and (dxy[:, 2] <= psi_bar(g.track, cl[:n])).all()
    against_mirror(dev, tuple(a[:n] for a in mirror), f'n = {n}')
    tf.assert_round_trip(g.track, cl[:n], *dev, f'device n = {n}')


def test_seams_and_wrap(f1):
    from dgsqp_amd import tracks
    g, s = f1[:2]
    cl = tf.seam_points(g.track)
    xy = tracks.local_to_global_batch(g.track, cl)
    assert np.abs(s.local_to_global_batch(cl)[:, :2] - xy[:, :2]).max() <= 1e-12
    dev = s.global_to_local_batch(xy)
    against_mirror(dev, tracks.global_to_local_batch(g.track, xy), 'seams')
    tf.assert_round_trip(g.track, cl, *dev, 'device seams', start_line_kink=True)
    # s outside [0, L) is wrapped by local_to_global: two laps on, one lap back
    L = g.track.track_length
    far = cl.copy()
    far[::2, 0] += 2 * L
    far[1::2, 0] -= L
    assert np.abs(s.local_to_global_batch(far)[:, :2] - tracks.local_to_global_batch(g.track, far)[:, :2]).max() <= 1e-12
    assert np.abs(s.local_to_global_batch(far)[:, :2] - xy[:, :2]).max() <= 1e-9


def test_non_finite_inputs(f1):
    """Lanes 3 and 200 of 257 carry NaN and +inf: status 1 and NaN outputs there, every other lane bit for bit what the run without them
    gives; an off-track point keeps its values and gets status 2."""
    g, s, cl, xy, _ = f1
    ref = s.global_to_local_batch(xy)
    bad = xy.copy()
    bad[3, 0], bad[200, 1] = np.nan, np.inf
    got = s.global_to_local_batch(bad)
    keep = np.ones(257, bool)
    keep[[3, 200]] = False
    assert got[2][[3, 200]].tolist() == [1, 1] and np.isnan(got[0][[3, 200]]).all() and np.isnan(got[1][[3, 200]]).all()
    assert np.array_equal(tf.bits(got[0][keep]), tf.bits(ref[0][keep])) and np.array_equal(tf.bits(got[1][keep]), tf.bits(ref[1][keep]))
    assert np.array_equal(got[2][keep], ref[2][keep])
    bad = xy[:4].copy()
    bad[1, 2] = -np.inf
    assert s.global_to_local_batch(bad)[2].tolist() == [0, 1, 0, 0]
    cl_bad = cl[:4].copy()
    cl_bad[2, 0] = np.nan
    out = s.local_to_global_batch(cl_bad)
    assert np.isnan(out[2]).all() and np.array_equal(tf.bits(out[[0, 1, 3]]), tf.bits(s.local_to_global_batch(cl[:4])[[0, 1, 3]]))
    off = cl[:3].copy()
    off[1, 1] = g.track.half_width + g.track.slack + 0.5
    from dgsqp_amd import tracks
    c, _, st = s.global_to_local_batch(tracks.local_to_global_batch(g.track, off))
    assert st.tolist() == [0, 2, 0] and abs(c[1, 1] - off[1, 1]) <= tf.BAR_EY


@pytest.mark.parametrize('name', ['L_track_barc', 'chicane', 'curve'])
def test_arc_tracks(name):
    """n = 64 through the device on a handle whose game runs on an arc track; the key points travel in the call.  sin / cos / atan2 are
    the two maths libraries': 1e-11 against the mirror (coordinates of a few metres, a few ulp each), the host bars against the truth.
    The last point is 10 track widths away: status 2, NaN outputs."""
    from dgsqp_amd import montecarlo as mc, tracks
    from dgsqp_amd.solver import DGSQP
    t = tf.arc_tracks()[name]
    g = mc.barc_racing_game(N=5) if name == 'L_track_barc' else mc.kinematic_racing_game(name, N=5)
    s = DGSQP(*g.solver_args(), print_method=None)
    cl = np.ascontiguousarray(tf.round_trip_points(t, n=64, seed=1, ey_frac=1.0))
    xy = tracks.local_to_global_batch(t, cl)
    dev_xy = s.local_to_global_batch(cl, track=t)
    d = np.abs(dev_xy - xy).max(axis=0)
    print(f'{name}: local_to_global |dx| {d[0]:.2e}, |dy| {d[1]:.2e}, |dpsi| {d[2]:.2e}')
    assert d.max() <= 1e-12
    xy[63, :2] += 10 * t.track_width
    dev = s.global_to_local_batch(xy, track=t)
    mirror = tracks.global_to_local_batch(t, xy)
    assert dev[2].tolist() == [0] * 63 + [2] and np.isnan(dev[0][63]).all() and np.isnan(dev[1][63])
    against_mirror(tuple(a[:63] for a in dev), tuple(a[:63] for a in mirror), name)
    tf.assert_round_trip(t, cl[:63], *(a[:63] for a in dev), f'device {name}')
    kp = t.key_pts
    on = s.global_to_local_batch(np.array([[kp[1, 0], kp[1, 1], 0.2]]), track=t)
    assert on[2][0] == 0 and on[0][0, 1] == 0.0 and on[0][0, 0] == kp[1, 3]
    if name == 'L_track_barc':          # without track=: the game's own
        assert np.array_equal(tf.bits(s.global_to_local_batch(xy)[0][:63]), tf.bits(dev[0][:63]))


def test_256_thread_build(f1):
    from dgsqp_amd.solver import DGSQP
    g, s, cl, xy, _ = f1
    b = DGSQP(*g.solver_args(), print_method=None, workgroups_per_cu=2)
    for name in ('dgsqp_local_to_global_batch', 'dgsqp_global_to_local_batch', 'dgsqp_sample_raceline_spline_batch'):
        assert hasattr(b._lib, name)
    assert np.array_equal(tf.bits(b.local_to_global_batch(cl)), tf.bits(s.local_to_global_batch(cl)))
    one, two = s.global_to_local_batch(xy), b.global_to_local_batch(xy)
    assert np.array_equal(tf.bits(one[0]), tf.bits(two[0])) and np.array_equal(tf.bits(one[1]), tf.bits(two[1])) and np.array_equal(one[2], two[2])


def test_c_side_refusals(f1):
    from dgsqp_amd import _ffi, montecarlo as mc, sampler as smp, tracks
    from dgsqp_amd.solver import DGSQP
    g, s, cl, xy, _ = f1
    lib, P = s._lib, _ffi.dptr
    out, res, st = np.empty((4, 3)), np.empty(4), np.empty(4, np.int32)
    a = np.ascontiguousarray(xy[:4])

    def refused(rc, handle, word=''):
        msg = handle._lib.dgsqp_last_error(handle._h).decode()
        assert rc == _ffi.E_ARG and msg.startswith('track frame: ') and word in msg, (rc, msg)
    T = tracks.track_frame_spec(g.track)
    refused(lib.dgsqp_local_to_global_batch(s._h, -1, C.byref(T), P(a), P(out)), s, 'n < 0')
    refused(lib.dgsqp_global_to_local_batch(s._h, -1, C.byref(T), P(a), P(out), P(res), _ffi.iptr(st)), s, 'n < 0')
    refused(lib.dgsqp_local_to_global_batch(s._h, 4, None, P(a), P(out)), s, 'NULL')
    refused(lib.dgsqp_local_to_global_batch(s._h, 4, C.byref(T), None, P(out)), s, 'NULL')
    refused(lib.dgsqp_local_to_global_batch(s._h, 4, C.byref(T), P(a), None), s, 'NULL')
    refused(lib.dgsqp_global_to_local_batch(s._h, 4, C.byref(T), None, P(out), P(res), _ffi.iptr(st)), s, 'NULL')
    refused(lib.dgsqp_global_to_local_batch(s._h, 4, C.byref(T), P(a), None, P(res), _ffi.iptr(st)), s, 'NULL')
    refused(lib.dgsqp_global_to_local_batch(s._h, 4, C.byref(T), P(a), P(out), P(res), None), s, 'status')
    assert lib.dgsqp_global_to_local_batch(s._h, 4, C.byref(T), P(a), P(out), None, _ffi.iptr(st)) == 0          # resid may be NULL
    assert lib.dgsqp_global_to_local_batch(s._h, 0, C.byref(T), P(a), P(out), None, _ffi.iptr(st)) == 0
    bg = mc.barc_racing_game(N=5)
    arc = DGSQP(*bg.solver_args(), print_method=None)
    A = tracks.track_frame_spec(bg.track)
    refused(lib.dgsqp_local_to_global_batch(s._h, 4, C.byref(A), P(a), P(out)), s, 'spline-track handle')
    refused(lib.dgsqp_global_to_local_batch(s._h, 4, C.byref(A), P(a), P(out), P(res), _ffi.iptr(st)), s, 'spline-track handle')
    refused(lib.dgsqp_local_to_global_batch(arc._h, 4, C.byref(T), P(a), P(out)), arc, 'n_key = 0')
    refused(lib.dgsqp_global_to_local_batch(arc._h, 4, C.byref(T), P(a), P(out), P(res), _ffi.iptr(st)), arc, 'n_key = 0')
    for n_key in (1, _ffi.MAX_SEGS + 2, -3):
        A = tracks.track_frame_spec(bg.track)
        A.n_key = n_key
        refused(lib.dgsqp_global_to_local_batch(arc._h, 4, C.byref(A), P(a), P(out), P(res), _ffi.iptr(st)), arc, 'n_key = ')
    A = tracks.track_frame_spec(bg.track)
    A.key_pts[2][1] = np.nan
    refused(lib.dgsqp_local_to_global_batch(arc._h, 4, C.byref(A), P(a), P(out)), arc, 'key point [2][1]')
    A = tracks.track_frame_spec(bg.track)
    A.key_pts[A.n_key - 1][3] = 0.0
    refused(lib.dgsqp_local_to_global_batch(arc._h, 4, C.byref(A), P(a), P(out)), arc, 'track length')
    A = tracks.track_frame_spec(bg.track)
    A.slack = np.inf
    refused(lib.dgsqp_global_to_local_batch(arc._h, 4, C.byref(A), P(a), P(out), P(res), _ffi.iptr(st)), arc, 'slack')
    with pytest.raises(ValueError, match='track frame: '):
        s.global_to_local_batch(xy[:4], track=bg.track)
    # the handles are fine after every refusal
    assert (s.global_to_local_batch(xy[:4])[2] == 0).all() and (arc.global_to_local_batch(tracks.local_to_global_batch(bg.track, cl[:4] * [0.01, 0.3, 1]))[2] == 0).all()
    # the sampler's entries: the kinds that need seg0_len, the wrong track kind
    spec = smp.sampler_spec(g, 1)
    pid = _ffi.PidT()
    pid.substeps = 10
    for kind in (smp.FIRST_SEGMENT, smp.INDEPENDENT):
        spec.kind = kind
        assert lib.dgsqp_sample_batch(s._h, 4, C.byref(spec), C.byref(pid), None, None, None, 0) == _ffi.E_ARG
        assert lib.dgsqp_last_error(s._h).decode().startswith('sampler: a spline track takes the circuit sampler only')
    spec.kind = smp.CIRCUIT
    assert lib.dgsqp_sample_batch(arc._h, 4, C.byref(spec), C.byref(pid), None, None, None, 0) == _ffi.E_ARG          # n_key = 0 on an arc-track handle
    assert lib.dgsqp_last_error(arc._h).decode() == 'bad sampler description'
