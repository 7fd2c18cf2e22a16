"""Track geometry entering the hot path.

Only what ``DGSQP.solve()`` and the Monte-Carlo samplers need from the
reference track classes:

* key points of a radius/arc-length centre line
  (reference DGSQP/tracks/radius_arclength_track.py:361-408),
* the two lookup tables behind ``get_curvature_casadi_fn`` /
  ``get_tangent_angle_casadi_fn`` (:199-225) -- exported as plain arrays that
  the HIP kernels evaluate with CasADi's ``pw_const`` / ``pw_lin`` semantics,
* ``local_to_global`` (:752-807) used by the initial-condition samplers, and ``global_to_local`` (:644-743; on a spline the
  foot point the reference's NLP finds) -- both also for batches, as the numpy mirrors of csrc/dgsqp_track_frame.h,
* the three parametrised shapes of DGSQP/tracks/track_lib.py:14-87 and the
  ``L_track_barc`` circuit.

Plotting is not on the path.
"""
from __future__ import annotations

import numpy as np


def _wrap(theta: float) -> float:
    if theta < -np.pi:
        return 2 * np.pi + theta
    if theta > np.pi:
        return theta - 2 * np.pi
    return theta


class _WidthFunctions:
    """``left_width(s)`` / ``right_width(s)`` of a track: the reference's ``pw_lin(sbar, s_waypoints, width)`` on the wrapped arclength
    (DGSQP/tracks/casadi_bspline_track.py:61-64) over a table of knots -- the numpy mirror of dev_track_width (csrc/dgsqp_track_width.h):
    piece i is the largest one with K_i <= sbar, the value is ``w_i + (w_{i+1} - w_i) / (K_{i+1} - K_i) * (sbar - K_i)``, every operation
    rounded once.  A track without a table has constant widths ``half_width`` (radius_arclength_track.py:57)."""
    _width_table = None

    def set_width_table(self, knots, left, right):
        """An explicit table: ``knots`` from 0 to the track length, strictly increasing, positive widths at every knot."""
        from . import _ffi
        k, l, r = (np.array(v, dtype=float) for v in (knots, left, right))
        if k.ndim != 1 or l.shape != k.shape or r.shape != k.shape or k.size < 2:
            raise ValueError('width table: knots, left and right are three vectors of one length, at least 2')
        if k.size > _ffi.MAX_KNOTS:
            raise ValueError('width table: %d knots, limit is %d' % (k.size, _ffi.MAX_KNOTS))
        if not (np.isfinite(k).all() and np.isfinite(l).all() and np.isfinite(r).all()):
            raise ValueError('width table: a non-finite entry')
        if k[0] != 0.0 or k[-1] != self.track_length:
            raise ValueError('width table: the knots must run from 0 to the track length %r' % self.track_length)
        if not (np.diff(k) > 0).all():
            raise ValueError('width table: the knots must increase strictly')
        if not ((l > 0).all() and (r > 0).all()):
            raise ValueError('width table: the widths must be positive')
        self._width_table = (k, l, r)
        return self

    def clear_width_table(self):
        """Back to constant widths ``half_width``: ``build_problem`` then passes no table (n_width = 0)."""
        self._width_table = None
        return self

    def width_table(self):
        """[n, 3] rows (knot, left, right) as the C-ABI takes them (dgsqp_problem_t.widths), or None for constant widths."""
        if self._width_table is None:
            return None
        return np.ascontiguousarray(np.stack(self._width_table, axis=1))

    def _width_piece(self, s):
        k = self._width_table[0]
        sb = self._sbar(np.asarray(s, dtype=float))
        i = np.clip(np.searchsorted(k, sb, side='right') - 1, 0, len(k) - 2)
        return i, sb - k[i], k[i + 1] - k[i]

    def _width(self, s, col):
        if self._width_table is None:
            return np.full(np.shape(s), float(self.half_width))[()]
        w = self._width_table[col]
        i, t, dk = self._width_piece(s)
        return (w[i + 1] - w[i]) / dk * t + w[i]

    def left_width(self, s):
        return self._width(s, 1)

    def right_width(self, s):
        return self._width(s, 2)

    def width_slopes(self, s):
        """(d left_width / ds, d right_width / ds): the slope of the piece with K_i <= sbar < K_{i+1} (right-continuous at a knot)."""
        if self._width_table is None:
            z = np.zeros(np.shape(s))[()]
            return z, z
        _, l, r = self._width_table
        i, _, dk = self._width_piece(s)
        return (l[i + 1] - l[i]) / dk, (r[i + 1] - r[i]) / dk


class RadiusArclengthTrack(_WidthFunctions):
    """Centre line made of constant-curvature segments ``cl_segs[i] = [length, signed radius]``
    (radius 0 = straight)."""

    def __init__(self, track_width=None, slack=None, cl_segs=None):
        self.track_width = track_width
        self.slack = slack
        self.cl_segs = None if cl_segs is None else np.asarray(cl_segs, dtype=float)
        self.key_pts = None
        self.track_length = None
        self.half_width = None
        self.n_segs = None
        self.circuit = False
        self.phase_out = False

    def initialize(self, track_width=None, slack=None, cl_segs=None, init_pos=(0, 0, 0)):
        if track_width is not None:
            self.track_width = float(track_width)
        if slack is not None:
            self.slack = float(slack)
        if cl_segs is not None:
            self.cl_segs = np.asarray(cl_segs, dtype=float)
        self.half_width = self.track_width / 2
        self.n_segs = self.cl_segs.shape[0]
        self.key_pts = self.get_track_key_pts(self.cl_segs, init_pos)
        self.track_length = float(self.key_pts[-1, 3])
        self.circuit = bool(np.isclose(self.key_pts[0, 0], self.key_pts[-1, 0])
                            and np.isclose(self.key_pts[0, 1], self.key_pts[-1, 1]))
        return self

    @staticmethod
    def get_track_key_pts(cl_segs, init_pos):
        """Rows ``[x, y, psi, cumulative s, segment length, signed curvature]``; row i>0
        describes the END of segment i-1 (radius_arclength_track.py:361-408)."""
        n = cl_segs.shape[0]
        kp = np.zeros((n + 1, 6))
        kp[0, :3] = init_pos
        for i in range(1, n + 1):
            x0, y0, psi0, s0 = kp[i - 1, :4]
            length, r = cl_segs[i - 1]
            if r == 0:
                psi, curv = psi0, 0.0
                x = x0 + length * np.cos(psi0)
                y = y0 + length * np.sin(psi0)
            else:
                xc = x0 - r * np.sin(psi0)
                yc = y0 + r * np.cos(psi0)
                theta = length / r
                x = xc + r * np.sin(psi0 + theta)
                y = yc - r * np.cos(psi0 + theta)
                curv = 1 / r
                psi = _wrap(psi0 + theta)
            kp[i] = [x, y, psi, s0 + length, length, curv]
        return kp

    # ---- tables consumed by the solver (radius_arclength_track.py:199-225) -------------------
    def tables(self):
        """Return ``(L, seg_s[n+1], seg_curv[n], seg_ang[n+1])``:
        curvature(s) = pw_const(sbar, seg_s[1:-1], seg_curv), tangent(s) = pw_lin(sbar, seg_s, seg_ang)."""
        seg_s = self.key_pts[:, 3].copy()
        seg_curv = self.key_pts[1:, 5].copy()
        seg_len = self.key_pts[:, 4]
        curv = self.key_pts[:, 5]
        ang = np.zeros(self.key_pts.shape[0] + 1)
        for i in range(self.key_pts.shape[0]):
            ang[i + 1] = ang[i] if curv[i] == 0 else ang[i] + seg_len[i] * curv[i]
        return self.track_length, seg_s, seg_curv, ang[1:].copy()

    def _sbar(self, s):
        L = self.track_length
        return np.fmod(np.fmod(s, L) + L, L)

    def get_curvature(self, s):
        """Numeric value of the CasADi curvature function (pw_const semantics)."""
        _, seg_s, seg_curv, _ = self.tables()
        sb = self._sbar(s)
        c = seg_curv[0]
        for i in range(len(seg_curv) - 1):
            c = c + (seg_curv[i + 1] - seg_curv[i]) * float(sb >= seg_s[i + 1])
        return c

    def get_tangent_angle(self, s):
        """Numeric value of the CasADi tangent-angle function (pw_lin semantics)."""
        _, seg_s, _, ang = self.tables()
        sb = self._sbar(s)

        def lseg(i):
            return ang[i] + (ang[i + 1] - ang[i]) / (seg_s[i + 1] - seg_s[i]) * (sb - seg_s[i])
        r = lseg(0)
        for i in range(len(seg_s) - 2):
            if sb >= seg_s[i + 1]:
                r = r + (lseg(i + 1) - lseg(i))
        return r

    def get_halfwidth(self, s):
        return self.half_width

    kind = 'arcs'

    def lookup(self, s):
        """Vectorised (curvature, tangent angle) at arclength s."""
        L, seg_s, seg_curv, ang = self.tables()
        sb = np.fmod(np.fmod(s, L) + L, L)
        idx = np.clip(np.searchsorted(seg_s, sb, side='right') - 1, 0, len(seg_curv) - 1)
        slope = (ang[idx + 1] - ang[idx]) / (seg_s[idx + 1] - seg_s[idx])
        return seg_curv[idx], ang[idx] + slope * (sb - seg_s[idx])

    # ---- Frenet -> global (radius_arclength_track.py:752-807) --------------------------------
    def local_to_global(self, cl_coord):
        s, e_y, e_psi = cl_coord
        L = self.track_length
        while s < 0:
            s += L
        while s >= L:
            s -= L
        kp = self.key_pts
        i0 = np.where(s >= kp[:, 3])[0][-1]
        i1 = i0 + 1
        x_s, y_s, psi_s = kp[i0, 0], kp[i0, 1], kp[i0, 2]
        x_f, y_f, psi_f, curv_f = kp[i1, 0], kp[i1, 1], kp[i1, 2], kp[i1, 5]
        seg_len = kp[i1, 4]
        d = s - kp[i0, 3]
        if curv_f == 0:
            x = x_s + (x_f - x_s) * d / seg_len + e_y * np.cos(psi_f + np.pi / 2)
            y = y_s + (y_f - y_s) * d / seg_len + e_y * np.sin(psi_f + np.pi / 2)
            psi = _wrap(psi_f + e_psi)
        else:
            r = 1 / curv_f
            sgn = 1 if r >= 0 else -1
            xc = x_s + abs(r) * np.cos(psi_s + sgn * np.pi / 2)
            yc = y_s + abs(r) * np.sin(psi_s + sgn * np.pi / 2)
            span = d / abs(r)
            psi_d = _wrap(psi_s + sgn * span)
            ang_norm = _wrap(psi_s + sgn * np.pi / 2)
            ang = -(1 if ang_norm >= 0 else -1) * (np.pi - abs(ang_norm))
            x = xc + (abs(r) - sgn * e_y) * np.cos(ang + sgn * span)
            y = yc + (abs(r) - sgn * e_y) * np.sin(ang + sgn * span)
            psi = _wrap(psi_d + e_psi)
        return x, y, psi

    def local_to_global_typed(self, state):
        x, y, psi = self.local_to_global((state.p.s, state.p.x_tran, state.p.e_psi))
        state.x.x, state.x.y, state.e.psi = x, y, psi

    # ---- global -> Frenet (radius_arclength_track.py:644-743) --------------------------------
    def global_to_local(self, xy_coord):
        """One point ``(x, y, psi)`` -> ``(s, e_y, e_psi)``, or ``None`` when no segment takes it, as the reference; an array [n, 3] ->
        [n, 3] with NaN rows for such points (``global_to_local_batch`` also gives their status)."""
        return _global_to_local(self, xy_coord)

    def global_to_local_typed(self, state):
        return _global_to_local_typed(self, state)


class StraightTrack(RadiusArclengthTrack):
    def __init__(self, length, width, slack, phase_out=False):
        segs = [[length, 0], [10, 0]] if phase_out else [[length, 0]]
        super().__init__(width, slack, np.array(segs, dtype=float))
        self.phase_out = phase_out
        self.initialize()
        self.circuit = False


class CurveTrack(RadiusArclengthTrack):
    """straight - arc - straight (track_lib.py:27-52)."""

    def __init__(self, enter_straight_length, curve_length, curve_swept_angle, exit_straight_length,
                 width, slack, phase_out=False, ccw=True):
        sgn = 1 if ccw else -1
        segs = [[enter_straight_length, 0], [curve_length, sgn * curve_length / curve_swept_angle],
                [exit_straight_length, 0]]
        if phase_out:
            segs.append([10, 0])
        super().__init__(width, slack, np.array(segs, dtype=float))
        self.phase_out = phase_out
        self.initialize()
        self.circuit = False


class ChicaneTrack(RadiusArclengthTrack):
    """straight - arc - straight - opposite arc - straight (track_lib.py:54-87)."""

    def __init__(self, enter_straight_length, curve1_length, curve1_swept_angle, mid_straight_length,
                 curve2_length, curve2_swept_angle, exit_straight_length, width, slack,
                 phase_out=False, mirror=False):
        s1, s2 = (1, -1) if mirror else (-1, 1)
        segs = [[enter_straight_length, 0], [curve1_length, s1 * curve1_length / curve1_swept_angle],
                [mid_straight_length, 0], [curve2_length, s2 * curve2_length / curve2_swept_angle],
                [exit_straight_length, 0]]
        if phase_out:
            segs.append([10, 0])
        super().__init__(width, slack, np.array(segs, dtype=float))
        self.phase_out = phase_out
        self.initialize()
        self.circuit = False


# L_track_barc circuit: the numbers of DGSQP/tracks/track_data/L_track_barc.npz
# (cl_segs, track_width, slack) -- data, not code; tests/test_tracks.py checks closure and
# the cumulative lengths quoted in SURVEY.md Appendix B.
_TRACK_DATA = {
    'L_track_barc': dict(
        track_width=1.1, slack=0.3,
        cl_segs=[[2.251, 0.0], [3.620685533262237, 1.1525], [0.9009999999999999, 0.0],
                 [1.6024753617155325, -1.0201675], [0.15000000000000002, 0.0],
                 [3.858449119267546, 1.2281825], [2.25454, 0.0], [1.9173571933848375, 1.2206275],
                 [0.9059049999999997, 0.0]]),
}


class CubicSplineTrack(_WidthFunctions):
    """Centre line given by cubic-spline interpolants x(s), y(s) through arclength-tagged waypoints -- the reference's
    ``CasadiBSplineTrack`` (DGSQP/tracks/casadi_bspline_track.py:10-71) as the solver sees it:
    curvature = (x'y'' - y'x'') / (x'^2 + y'^2)^1.5 (:122-135), tangent angle = atan2(y', x') (:137-149),
    ``sbar = fmod(fmod(s, L) + L, L)``.  The interpolant is held as one cubic per waypoint interval (ascending powers of
    ``s - s_i``); the table is produced by tools/make_f1_table.py with scipy's ``make_interp_spline(k=3)`` -- CasADi's
    ``interpolant('bspline')`` satisfies the same interpolation conditions, its end conditions may differ (stated deviation)."""
    kind = 'spline'

    def __init__(self, knots, cx, cy, left_width, right_width, slack):
        self.knots = np.asarray(knots, float)
        self.cx, self.cy = np.asarray(cx, float), np.asarray(cy, float)
        self.left_width_points, self.right_width_points = np.asarray(left_width, float), np.asarray(right_width, float)
        self.track_width = float(np.mean(self.left_width_points + self.right_width_points))      # casadi_bspline_track.py:20-21
        self.half_width = self.track_width / 2
        self.slack = slack
        self.track_length = float(self.knots[-1] - self.knots[0])
        self.circuit = bool(np.allclose([self.cx[0, 0], self.cy[0, 0]], self._xy(self.knots[-1] - 1e-12), atol=1e-6))
        self.set_width_table(self.knots - self.knots[0], self.left_width_points, self.right_width_points)       # the measured edges

    def _sbar(self, s):
        L = self.track_length
        return np.fmod(np.fmod(s, L) + L, L)

    def _piece(self, sb):
        i = np.clip(np.searchsorted(self.knots, sb, side='right') - 1, 0, len(self.knots) - 2)
        return i, sb - self.knots[i]

    def _xy(self, s):
        i, t = self._piece(self._sbar(np.asarray(s, float)))
        return (((self.cx[i, 3] * t + self.cx[i, 2]) * t + self.cx[i, 1]) * t + self.cx[i, 0],
                ((self.cy[i, 3] * t + self.cy[i, 2]) * t + self.cy[i, 1]) * t + self.cy[i, 0])

    def _derivs(self, s):
        i, t = self._piece(self._sbar(np.asarray(s, float)))
        dx = (3 * self.cx[i, 3] * t + 2 * self.cx[i, 2]) * t + self.cx[i, 1]
        dy = (3 * self.cy[i, 3] * t + 2 * self.cy[i, 2]) * t + self.cy[i, 1]
        return dx, dy, 6 * self.cx[i, 3] * t + 2 * self.cx[i, 2], 6 * self.cy[i, 3] * t + 2 * self.cy[i, 2]

    def lookup(self, s):
        """Vectorised (curvature, tangent angle) at arclength s."""
        dx, dy, ddx, ddy = self._derivs(s)
        return (dx * ddy - dy * ddx) / np.power(dx ** 2 + dy ** 2, 1.5), np.arctan2(dy, dx)

    def get_curvature(self, s):
        return float(self.lookup(s)[0])

    def get_tangent_angle(self, s):
        return float(self.lookup(s)[1])

    def get_halfwidth(self, s):
        return self.half_width

    def local_to_global(self, cl_coord):
        """casadi_bspline_track.py:151-170: centre-line point plus e_y along the left normal, heading = tangent + e_psi."""
        s, e_y, e_psi = cl_coord
        x, y = self._xy(s)
        dx, dy, _, _ = self._derivs(s)
        nrm = np.hypot(dx, dy)
        return float(x - e_y * dy / nrm), float(y + e_y * dx / nrm), float(np.arctan2(dy, dx) + e_psi)

    def local_to_global_typed(self, state):
        x, y, psi = self.local_to_global((state.p.s, state.p.x_tran, state.p.e_psi))
        state.x.x, state.x.y, state.e.psi = x, y, psi

    def global_to_local(self, xy_coord):
        """One point ``(x, y, psi)`` -> ``(s, e_y, e_psi)``; an array [n, 3] -> [n, 3].  The foot point of ``global_to_local_batch``: the
        reference (casadi_bspline_track.py:106-112, :172-186) reaches it with an NLP started at the closest waypoint."""
        return _global_to_local(self, xy_coord)

    def global_to_local_typed(self, state):
        return _global_to_local_typed(self, state)

    def _frame(self, sb):
        """c, c', c'' at sbar in [0, L] -- the arithmetic of tf_eval (csrc/dgsqp_track_frame.h), on the table ``spline_table`` hands over."""
        kn = self.knots - self.knots[0]
        i = np.clip(np.searchsorted(kn, sb, side='right') - 1, 0, len(kn) - 2)
        t = sb - kn[i]
        cx, cy = self.cx[i], self.cy[i]
        return (((cx[:, 3] * t + cx[:, 2]) * t + cx[:, 1]) * t + cx[:, 0], ((cy[:, 3] * t + cy[:, 2]) * t + cy[:, 1]) * t + cy[:, 0],
                (3 * cx[:, 3] * t + 2 * cx[:, 2]) * t + cx[:, 1], (3 * cy[:, 3] * t + 2 * cy[:, 2]) * t + cy[:, 1],
                6 * cx[:, 3] * t + 2 * cx[:, 2], 6 * cy[:, 3] * t + 2 * cy[:, 2])

    def spline_table(self):
        """[knots (n), x coefficients (n-1) x 4, y coefficients (n-1) x 4] as the C-ABI takes it (dgsqp_problem_t.spline)."""
        return np.ascontiguousarray(np.concatenate([self.knots - self.knots[0], self.cx.ravel(), self.cy.ravel()]))


_SPLINE_TRACKS = {'f1_austin_tenth_scale': 'f1_austin_tenth_scale_spline.npz'}


def get_track(name: str):
    key = name[:-4] if name.endswith('.npz') else name
    if key in _SPLINE_TRACKS:
        import pathlib
        d = np.load(pathlib.Path(__file__).resolve().parent / 'track_data' / _SPLINE_TRACKS[key])
        return CubicSplineTrack(d['knots'], d['cx'], d['cy'], d['left_width'], d['right_width'], float(d['slack']))
    if key not in _TRACK_DATA:
        raise ValueError('Chosen Track is unavailable: %s\n Available Tracks: %s' % (name, sorted(_TRACK_DATA)))
    d = _TRACK_DATA[key]
    return RadiusArclengthTrack().initialize(d['track_width'], d['slack'], np.array(d['cl_segs'], dtype=float))


def load_mpclab_raceline(file_path, track_name, time_scale=1.0):
    """Reference DGSQP/tracks/track_lib.py:124-143: the reference's triple ``(raceline, s2t, raceline_mat)``.  ``raceline(t)`` returns the
    nine interpolated columns (x, y, psi, v_long, v_tran, psidot, e_psi, s, e_y) of the two-lap table -- a list of nine values, as the
    CasADi function does, each of ``t``'s shape --, ``s2t(s)`` the table's time at arclength ``s``; ``raceline_mat`` is the one-lap
    table [n, 9].  Both callables are the numpy look-ups of ``montecarlo.Raceline`` (``raceline.table`` is that object): linear, and
    continued linearly outside the table."""
    from .montecarlo import Raceline
    rl = Raceline.from_file(file_path, track_name, time_scale)

    def raceline(t):
        v = rl.eval(t)
        return [v[..., c] for c in range(v.shape[-1])]

    def s2t(s):
        return rl.s2t(s)
    raceline.table = s2t.table = rl
    return raceline, s2t, rl.lap_mat


# ---- batched track-frame transforms: the numpy mirror of csrc/dgsqp_track_frame.h ----
def _wrap_pi(a):
    """Into (-pi, pi] (tf_wrap_pi)."""
    return a - 2 * np.pi * np.ceil((a - np.pi) / (2 * np.pi))


def _wrap_once(a):
    """``_wrap`` for arrays."""
    return np.where(a < -np.pi, 2 * np.pi + a, np.where(a > np.pi, a - 2 * np.pi, a))


def _points(a, what):
    a = np.asarray(a, dtype=float)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f'{what} must be [n, 3]')
    return a


def track_frame_spec(track):
    """The C-ABI description of ``track`` for the batched transforms (include/dgsqp.h: dgsqp_track_frame_t); n_key = 0: the handle's spline."""
    from . import _ffi
    T = _ffi.TrackFrameT()
    T.half_width, T.slack = float(track.track_width) / 2, float(track.slack)
    if track.kind == 'spline':
        return T
    kp = np.asarray(track.key_pts, dtype=float)
    if kp.shape[0] > _ffi.MAX_SEGS + 1:
        raise ValueError('track frame: arc tracks of at most %d segments' % _ffi.MAX_SEGS)
    T.n_key = kp.shape[0]
    for i in range(kp.shape[0]):
        for j in range(6):
            T.key_pts[i][j] = float(kp[i, j])
    return T


def local_to_global_batch(track, cl):
    """Frenet ``cl`` [n, 3] = (s, e_y, e_psi) -> [n, 3] = (x, y, psi): ``track.local_to_global`` for every row, vectorised -- the arithmetic of
    dev_spline_local_to_global / dev_arc_local_to_global.  A row whose s is not finite gives NaN."""
    cl = _points(cl, 'cl')
    out = np.full(cl.shape, np.nan)
    m = np.isfinite(cl[:, 0])
    s, ey, epsi = cl[m, 0], cl[m, 1], cl[m, 2]
    L = track.track_length
    sb = np.fmod(np.fmod(s, L) + L, L)
    if track.kind == 'spline':
        x, y, dx, dy, _, _ = track._frame(sb)
        nrm = np.sqrt(dx * dx + dy * dy)          # (as the device: x, y carry its bits; the scalar method's hypot may differ in the last place)
        out[m] = np.stack([x - ey * dy / nrm, y + ey * dx / nrm, np.arctan2(dy, dx) + epsi], axis=1)
        return out
    kp = track.key_pts
    i0 = np.clip(np.searchsorted(kp[:, 3], sb, side='right') - 1, 0, kp.shape[0] - 2)
    i1 = i0 + 1
    xs, ys, psis = kp[i0, 0], kp[i0, 1], kp[i0, 2]
    xf, yf, psif, curv, seg = kp[i1, 0], kp[i1, 1], kp[i1, 2], kp[i1, 5], kp[i1, 4]
    d = sb - kp[i0, 3]
    hp = np.pi / 2
    with np.errstate(divide='ignore', invalid='ignore'):
        r = 1 / curv
        sgn = np.where(r >= 0, 1.0, -1.0)
        ar = np.abs(r)
        xc, yc = xs + ar * np.cos(psis + sgn * hp), ys + ar * np.sin(psis + sgn * hp)
        span = d / ar
        an = _wrap_once(psis + sgn * hp)
        ang = -np.where(an >= 0, 1.0, -1.0) * (np.pi - np.abs(an))
        xa, ya = xc + (ar - sgn * ey) * np.cos(ang + sgn * span), yc + (ar - sgn * ey) * np.sin(ang + sgn * span)
        psia = _wrap_once(_wrap_once(psis + sgn * span) + epsi)
    st = curv == 0
    out[m] = np.stack([np.where(st, xs + (xf - xs) * d / seg + ey * np.cos(psif + hp), xa),
                       np.where(st, ys + (yf - ys) * d / seg + ey * np.sin(psif + hp), ya),
                       np.where(st, _wrap_once(psif + epsi), psia)], axis=1)
    return out


def _project_spline(track, px, py, psi):
    """dev_spline_project for finite points: the piece whose start is closest, 30 Newton steps on g(s) = (c(s) - p) . c'(s) clipped to
    [K_j - 1.5 D, K_j + 1.5 D], no early exit."""
    kn = track.knots - track.knots[0]
    L = track.track_length
    x0, y0 = track.cx[:, 0], track.cy[:, 0]
    j = np.empty(len(px), dtype=np.int64)
    for a in range(0, len(px), 4096):                       # (the distance table of a chunk: 4096 x pieces)
        ax, ay = x0[None, :] - px[a:a + 4096, None], y0[None, :] - py[a:a + 4096, None]
        j[a:a + 4096] = np.argmin(ax * ax + ay * ay, axis=1)
    delta = kn[1] - kn[0]
    lo, hi = kn[j] - 1.5 * delta, kn[j] + 1.5 * delta
    s = kn[j].copy()

    def at(s):
        sb = np.fmod(np.fmod(s, L) + L, L) if track.circuit else np.fmin(np.fmax(s, 0.0), L)
        x, y, dx, dy, ddx, ddy = track._frame(sb)
        ex, ey = x - px, y - py
        return sb, x, y, dx, dy, ddx, ddy, ex, ey, ex * dx + ey * dy
    for _ in range(30):
        _, _, _, dx, dy, ddx, ddy, ex, ey, g = at(s)
        h = (dx * dx + dy * dy) + (ex * ddx + ey * ddy)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            step = np.where(h > 0.0, -(g / h), np.where(g > 0.0, -0.1, np.where(g < 0.0, 0.1, 0.0)))
        s = np.fmax(np.fmin(s + step, hi), lo)
    sb, x, y, dx, dy, _, _, _, _, g = at(s)
    nrm = np.sqrt(dx * dx + dy * dy)
    return sb, ((py - y) * dx - (px - x) * dy) / nrm, _wrap_pi(psi - np.arctan2(dy, dx)), g


def _project_arcs(track, px, py, psi):
    """dev_arc_project for finite points: the segments in order, the first whose span contains the foot point with |e_y| within half the track
    width plus the slack.  Returns s, e_y, e_psi (NaN where no segment takes the point) and found [n]."""
    kp = track.key_pts
    lim = track.track_width / 2 + track.slack
    hp = np.pi / 2
    n = len(px)
    s_out, ey_out, ep_out = (np.full(n, np.nan) for _ in range(3))
    found = np.zeros(n, bool)
    for i in range(1, kp.shape[0]):
        xs, ys, psis = kp[i - 1, :3]
        xf, yf, psif = kp[i, :3]
        curv, seg = kp[i, 5], kp[i, 4]
        at_s = (px == xs) & (py == ys)
        at_f = ~at_s & (px == xf) & (py == yf)
        if curv == 0:
            wx, wy, vx, vy, ux, uy = xf - xs, yf - ys, px - xs, py - ys, px - xf, py - yf
            dot = wx * vx + wy * vy
            lw = np.sqrt(wx * wx + wy * wy)
            ey = (wx * vy - wy * vx) / lw
            ok = (dot >= 0.0) & (-(wx * ux + wy * uy) >= 0.0) & (np.abs(ey) <= lim)
            s = kp[i - 1, 3] + dot / lw
            ref = np.full(n, psis)
        else:
            r = 1 / curv
            dr = 1.0 if r > 0 else -1.0
            ar = abs(r)
            xc, yc = xs + ar * np.cos(psis + dr * hp), ys + ar * np.sin(psis + dr * hp)
            ax, ay, bx, by = xs - xc, ys - yc, px - xc, py - yc
            cur = np.arctan2(ax * by - ay * bx, ax * bx + ay * by)
            ey = -dr * (np.sqrt(bx * bx + by * by) - ar)
            ok = (cur * dr > 0.0) & (abs(seg / r) >= np.abs(cur)) & (np.abs(ey) <= lim)
            s = kp[i - 1, 3] + np.abs(cur) * ar
            ref = psis + cur
        s = np.where(at_s, kp[i - 1, 3], np.where(at_f, kp[i, 3], s))
        ey = np.where(at_s | at_f, 0.0, ey)
        ref = np.where(at_s, psis, np.where(at_f, psif, ref))
        take = ~found & (at_s | at_f | ok)
        s_out[take], ey_out[take], ep_out[take] = s[take], ey[take], _wrap_pi(psi - ref)[take]
        found |= take
    return s_out, ey_out, ep_out, found


def global_to_local_batch(track, xy):
    """Global poses ``xy`` [n, 3] = (x, y, psi) -> (cl [n, 3] = (s, e_y, e_psi), resid [n], status [n] int32): the numpy mirror of
    ``dgsqp_global_to_local_batch``.  status 0: fine; 1: an input is not finite (NaN outputs); 2: off the track -- on a spline
    |e_y| > half_width + slack with the values still returned, on arcs no segment takes the point (NaN outputs).  resid: the final
    g = (c(s) - p) . c'(s) on a spline, 0 on arcs."""
    xy = _points(xy, 'xy')
    n = xy.shape[0]
    cl, resid, status = np.full((n, 3), np.nan), np.full(n, np.nan), np.ones(n, np.int32)
    m = np.isfinite(xy).all(axis=1)
    if not m.any():
        return cl, resid, status
    px, py, psi = xy[m, 0], xy[m, 1], xy[m, 2]
    if track.kind == 'spline':
        s, ey, ep, g = _project_spline(track, px, py, psi)
        cl[m], resid[m] = np.stack([s, ey, ep], axis=1), g
        status[m] = np.where(np.abs(ey) > track.track_width / 2 + track.slack, 2, 0)
    else:
        s, ey, ep, found = _project_arcs(track, px, py, psi)
        cl[m], resid[m] = np.stack([s, ey, ep], axis=1), np.where(found, 0.0, np.nan)
        status[m] = np.where(found, 0, 2)
    return cl, resid, status


def _global_to_local(track, xy_coord):
    xy = np.asarray(xy_coord, dtype=float)
    if xy.ndim == 1:
        if xy.shape[0] != 3:
            raise ValueError('xy_coord: (x, y, psi)')
        cl, _, status = global_to_local_batch(track, xy[None, :])
        if track.kind == 'arcs' and status[0] == 2:
            return None
        return float(cl[0, 0]), float(cl[0, 1]), float(cl[0, 2])
    return global_to_local_batch(track, xy)[0]


def _global_to_local_typed(track, state):
    cl = _global_to_local(track, (state.x.x, state.x.y, state.e.psi))
    if cl is None:
        return -1
    state.p.s, state.p.x_tran, state.p.e_psi = cl
    return 0


def load_tum_raceline(file_path, track_name, tenth_scale=False, time_scale=1.0, segment=None, resample_resolution=None, solver=None):
    """Reference DGSQP/tracks/track_lib.py:145-213, its ``segment=None`` branch: the triple of ``load_mpclab_raceline`` from a TUM raceline file
    (``;``-separated rows s, x, y, psi, kappa, vx, ax).  Every row is projected onto the centre line -- with the numpy mirror, or on the device
    with ``solver=`` a ``DGSQP`` on that track.  ``segment=`` / ``resample_resolution=`` (the study's track segment) are not built."""
    if segment is not None or resample_resolution is not None:
        raise NotImplementedError('load_tum_raceline: segment= / resample_resolution= (a raceline on a track segment) are not built; '
                                  'the F1 game takes the window as s_range=')
    from .montecarlo import Raceline
    rl = Raceline.from_tum(file_path, track_name, tenth_scale=tenth_scale, time_scale=time_scale, solver=solver)

    def raceline(t):
        v = rl.eval(t)
        return [v[..., c] for c in range(v.shape[-1])]

    def s2t(s):
        return rl.s2t(s)
    raceline.table = s2t.table = rl
    return raceline, s2t, rl.lap_mat
