"""Test infrastructure of the track-frame transforms and the spline-track front ends (tests/test_track_frame_host.py, test_track_frame.py,
test_spline_sampler.py, test_f1_raceline.py): the seeded points, the seam points, the bars and the fixture.  The product never imports this."""
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
TUM_FIXTURE = ROOT / 'tests' / 'golden' / 'f1_traj_race_cl.csv.gz'
F1 = 'f1_austin_tenth_scale'

# Round-trip bars.  A prototype of exactly the projection's definition measured, on 20,000 seeded points of the F1 track, no wrong piece,
# |ds| 2.3e-13 and |de_y| 3.0e-14: the bars leave more than 100 x over that.
BAR_S, BAR_EY, BAR_EPSI, BAR_RESID = 1e-10, 1e-11, 1e-11, 1e-10


def f1_track():
    from dgsqp_amd.tracks import get_track
    return get_track(F1)


def round_trip_points(track, n=2000, seed=0, ey_frac=0.9):
    """Seeded Frenet points: s in [0, L), |e_y| <= ey_frac half_width, e_psi in +-0.5."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n) * track.track_length, (2 * rng.random(n) - 1) * ey_frac * track.half_width, rng.random(n) - 0.5], axis=1)


def seam_points(track):
    """K_i -+ 1e-9 for the first, a middle and the last piece, and s in {0, 1e-9, L - 1e-9}, each with e_y = -+0.3."""
    kn = track.knots - track.knots[0]
    L = track.track_length
    n = len(kn)
    s = []
    for i in (0, 1, n // 2, n - 2, n - 1):
        s += [kn[i] - 1e-9, kn[i] + 1e-9]
    s += [0.0, 1e-9, L - 1e-9]
    s = np.fmod(np.fmod(np.array(s), L) + L, L)
    return np.array([[si, ey, 0.1] for si in s for ey in (-0.3, 0.3)])


def circ(ds, L):
    ds = np.abs(ds)
    return np.minimum(ds, np.abs(L - ds))


def assert_round_trip(track, cl, got, resid, status, tag='', start_line_kink=False):
    """got = global_to_local(local_to_global(cl)) at the host bars.

    ``start_line_kink``: the F1 table is an interpolating spline with free ends, so its two ends meet in position (3e-16 m) but not in
    direction: the tangent turns by 8.66e-7 rad at the start line.  A point within |e_y| x 8.66e-7 m of the start line on the inner side of
    that kink has TWO foot points, one on the last piece and one on the first, and the one on the first piece is the closer by about
    1e-13 m -- measured: the point made from (L - 1e-9, -0.3) projects to s = 2.59e-7 with g = -5.7e-14, e_y = -0.3 to 1e-11 and e_psi off
    by exactly the kink.  That is the closest point (what the reference's NLP, started at waypoint 0, minimises), not the arclength the
    point was made from.  For the points made within 1e-6 m of the start line the check is therefore the one that does not depend on
    which of the two is named: status, residual and |de_y| at the same bars, the answer no farther from the point than the arclength it was
    made from, and mapping the answer back gives the point to 1e-11 m; every other point is held to all the bars."""
    from dgsqp_amd.tracks import local_to_global_batch
    L = track.track_length
    ds = circ(got[:, 0] - cl[:, 0], L) if track.circuit else np.abs(got[:, 0] - cl[:, 0])
    dey, dep = np.abs(got[:, 1] - cl[:, 1]), np.abs(got[:, 2] - cl[:, 2])
    at_line = np.zeros(len(cl), bool)
    if start_line_kink:
        at_line = circ(cl[:, 0], L) <= 1e-6
        p, back = local_to_global_batch(track, cl), local_to_global_batch(track, got)
        dp = np.abs(back[at_line] - p[at_line])
        other = at_line & ((ds > BAR_S) | (dep > BAR_EPSI))
        print(f'{tag}: {int(at_line.sum())} points at the start line, {int(other.sum())} of them answered with the other foot point '
              f'(|ds| up to {ds[at_line].max():.2e}, |de_psi| up to {dep[at_line].max():.2e}); mapped back |dp| {dp.max():.2e}')
        assert dp.max() <= 1e-11
        assert (np.abs(got[at_line, 1]) <= np.abs(cl[at_line, 1]) + 1e-12).all()
        assert (ds[at_line] <= 1e-6).all() and (dep[at_line] <= 1e-6).all()
    rest = ~at_line
    print(f'{tag}: n {len(cl)}, |ds| {ds[rest].max():.2e}, |de_y| {dey.max():.2e}, |de_psi| {dep[rest].max():.2e}, |resid| {np.abs(resid).max():.2e}, '
          f'status {np.unique(status).tolist()}')
    assert (status == 0).all()
    assert dey.max() <= BAR_EY and np.abs(resid).max() <= BAR_RESID
    assert ds[rest].max() <= BAR_S and dep[rest].max() <= BAR_EPSI


def arc_tracks():
    from dgsqp_amd.montecarlo import _track
    from dgsqp_amd.tracks import get_track
    return {'L_track_barc': get_track('L_track_barc'), 'chicane': _track('chicane', 45, 1.0), 'curve': _track('curve', 45, 1.0)}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def f1_raceline(time_scale=1.0):
    from dgsqp_amd.montecarlo import Raceline
    return Raceline.from_tum(TUM_FIXTURE, F1, tenth_scale=True, time_scale=time_scale)
