// Track-frame transforms on the device (include/dgsqp.h: dgsqp_local_to_global_batch, dgsqp_global_to_local_batch) and the placement
// kernel of the circuit sampler on a spline track.  Thin kernels: one lane per point, grid-stride loops.
//   dev_spline_local_to_global   CasadiBSplineTrack.local_to_global (casadi_bspline_track.py:151-170): centre-line point plus e_y along the
//                                left normal, heading atan2(y', x') + e_psi, on the handle's table dg_prob.spl
//   dev_spline_project           global -> Frenet on that table.  The reference starts an NLP from the closest waypoint; this is the
//                                deterministic statement of the same foot point: the piece j whose start point is closest, then 30 Newton
//                                steps on g(s) = (c(s) - p) . c'(s) inside [K_j - 1.5 D, K_j + 1.5 D], D = K_1 - K_0 (no early exit)
//   dev_arc_local_to_global      dg_local_to_global (dgsqp_sampler.h) plus the heading of radius_arclength_track.py:752-807
//   dev_arc_project              the rule of radius_arclength_track.py:644-743: the first segment, in order, whose span contains the foot
//                                point with |e_y| <= track_width / 2 + slack
// Every operation the numpy mirror (dgsqp_amd/tracks.py) restates is rounded once (no fused multiply-add), so the polynomial part --
// piece, Newton iterates, s, e_y on a spline -- carries the mirror's bits; atan2 / sin / cos are the two maths libraries'.
// Status of a projection: 0 fine; 1 an input is not finite (outputs NaN, no table is indexed); 2 off the track (spline: |e_y| > half_width
// + slack, values still returned; arcs: no segment takes the point, outputs NaN).
#pragma once

struct TfPoint { double x, y, dx, dy, ddx, ddy; };

__device__ inline double tf_sbar(double s, double L) { return fmod(fmod(s, L) + L, L); }
// into (-pi, pi]
__device__ inline double tf_wrap_pi(double a) {
#pragma clang fp contract(off)
  const double pi = 3.141592653589793, twopi = 6.283185307179586;
  return a - twopi * ceil((a - pi) / twopi);
}
// tracks._wrap: one step towards [-pi, pi]
__device__ inline double tf_wrap_once(double a) {
#pragma clang fp contract(off)
  const double pi = 3.141592653589793;
  if (a < -pi) return 2 * pi + a;
  if (a > pi) return a - 2 * pi;
  return a;
}
// the cubic piece of a finite sbar: the largest i with K_i <= sbar, clamped to 0 .. n_knots - 2 (waypoints are close to equispaced: a
// proportional guess, then a walk)
__device__ inline int tf_piece(double sbar) {
  const int nk = dg_prob.P.n_knots;
  const double* kn = dg_prob.spl;
  int i = (int)(sbar * dg_prob.inv_track_L * (double)(nk - 1));
  i = i < 0 ? 0 : (i > nk - 2 ? nk - 2 : i);
  while (i > 0 && sbar < kn[i]) i--;
  while (i < nk - 2 && sbar >= kn[i + 1]) i++;
  return i;
}
// c, c', c'' at a finite sbar in [0, L]
__device__ inline void tf_eval(double sbar, TfPoint& q) {
#pragma clang fp contract(off)
  const int nk = dg_prob.P.n_knots;
  const int i = tf_piece(sbar);
  const double t = sbar - dg_prob.spl[i];
  const double* cx = dg_prob.spl + nk + 4 * i;
  const double* cy = dg_prob.spl + nk + 4 * (nk - 1) + 4 * i;
  q.x = ((cx[3] * t + cx[2]) * t + cx[1]) * t + cx[0];
  q.y = ((cy[3] * t + cy[2]) * t + cy[1]) * t + cy[0];
  q.dx = (3 * cx[3] * t + 2 * cx[2]) * t + cx[1];
  q.dy = (3 * cy[3] * t + 2 * cy[2]) * t + cy[1];
  q.ddx = 6 * cx[3] * t + 2 * cx[2];
  q.ddy = 6 * cy[3] * t + 2 * cy[2];
}

__device__ inline void dev_spline_local_to_global(double s, double ey, double epsi, double* x, double* y, double* psi) {
#pragma clang fp contract(off)
  if (!__builtin_isfinite(s)) { *x = *y = *psi = __builtin_nan(""); return; }       // (no table is indexed with it)
  TfPoint q;
  tf_eval(tf_sbar(s, dg_prob.P.track_L), q);
  const double nrm = sqrt(q.dx * q.dx + q.dy * q.dy);
  *x = q.x - ey * q.dy / nrm;
  *y = q.y + ey * q.dx / nrm;
  *psi = atan2(q.dy, q.dx) + epsi;
}

__device__ inline int dev_spline_project(int circuit, double lim, double px, double py, double psi, double* s_out, double* ey_out,
                                         double* epsi_out, double* resid) {
#pragma clang fp contract(off)
  if (!(__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(psi))) {
    *s_out = *ey_out = *epsi_out = *resid = __builtin_nan("");
    return 1;
  }
  const int nk = dg_prob.P.n_knots;
  const double* kn = dg_prob.spl;
  const double* cx = dg_prob.spl + nk;
  const double* cy = dg_prob.spl + nk + 4 * (nk - 1);
  // coarse start: the loop index is the same in every lane, so the table is read with wave-uniform loads
  int j = 0;
  double best = 0.0;
  for (int i = 0; i < nk - 1; i++) {
    const double ax = cx[4 * i] - px, ay = cy[4 * i] - py;
    const double d2 = ax * ax + ay * ay;
    if (i == 0 || d2 < best) { best = d2; j = i; }
  }
  const double L = dg_prob.P.track_L, delta = kn[1] - kn[0];
  const double lo = kn[j] - 1.5 * delta, hi = kn[j] + 1.5 * delta;
  double s = kn[j];
  TfPoint q;
  for (int it = 0; it <= 30; it++) {
    const double sb = circuit ? tf_sbar(s, L) : fmin(fmax(s, 0.0), L);
    tf_eval(sb, q);
    const double ex = q.x - px, ey = q.y - py;
    const double g = ex * q.dx + ey * q.dy;
    if (it == 30) {            // the 31st evaluation is the result's
      const double nrm = sqrt(q.dx * q.dx + q.dy * q.dy);
      *s_out = sb;
      *ey_out = ((py - q.y) * q.dx - (px - q.x) * q.dy) / nrm;
      *epsi_out = tf_wrap_pi(psi - atan2(q.dy, q.dx));
      *resid = g;
      break;
    }
    const double h = (q.dx * q.dx + q.dy * q.dy) + (ex * q.ddx + ey * q.ddy);
    const double step = h > 0.0 ? -(g / h) : (g > 0.0 ? -0.1 : (g < 0.0 ? 0.1 : 0.0));
    s = fmax(fmin(s + step, hi), lo);
  }
  return fabs(*ey_out) > lim ? 2 : 0;
}

// T carries the key points for dg_local_to_global; s is wrapped with fmod first, so that function's own wrap loops have nothing to do
// (they would not end for a huge s)
__device__ inline void dev_arc_local_to_global(const dgsqp_sampler_t& T, double s, double ey, double epsi, double* x, double* y, double* psi) {
#pragma clang fp contract(off)
  if (!__builtin_isfinite(s)) { *x = *y = *psi = __builtin_nan(""); return; }
  const double L = T.key_pts[T.n_key - 1][3];
  s = tf_sbar(s, L);
  dg_local_to_global(T, s, ey, x, y);
  int i0 = 0;
  for (int i = 0; i < T.n_key - 1; i++) if (s >= T.key_pts[i][3]) i0 = i;
  const double curv = T.key_pts[i0 + 1][5];
  if (curv == 0.0) *psi = tf_wrap_once(T.key_pts[i0 + 1][2] + epsi);
  else {
    const double r = 1.0 / curv, sgn = r >= 0 ? 1.0 : -1.0;
    const double span = (s - T.key_pts[i0][3]) / fabs(r);
    *psi = tf_wrap_once(tf_wrap_once(T.key_pts[i0][2] + sgn * span) + epsi);
  }
}

__device__ inline int dev_arc_project(const dgsqp_track_frame_t& F, double px, double py, double psi, double* s_out, double* ey_out,
                                      double* epsi_out, double* resid) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  *s_out = *ey_out = *epsi_out = *resid = nan;
  if (!(__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(psi))) return 1;
  const double lim = F.half_width + F.slack, hp = 1.5707963267948966;
  for (int i = 1; i < F.n_key; i++) {
    const double xs = F.key_pts[i - 1][0], ys = F.key_pts[i - 1][1], psis = F.key_pts[i - 1][2];
    const double xf = F.key_pts[i][0], yf = F.key_pts[i][1], psif = F.key_pts[i][2], curv = F.key_pts[i][5], len = F.key_pts[i][4];
    double s, ey, ref;
    if (px == xs && py == ys) { s = F.key_pts[i - 1][3]; ey = 0.0; ref = psis; }
    else if (px == xf && py == yf) { s = F.key_pts[i][3]; ey = 0.0; ref = psif; }
    else if (curv == 0.0) {
      const double wx = xf - xs, wy = yf - ys, vx = px - xs, vy = py - ys, ux = px - xf, uy = py - yf;
      const double dot = wx * vx + wy * vy;
      if (!(dot >= 0.0 && -(wx * ux + wy * uy) >= 0.0)) continue;          // the foot point is not between the segment's ends
      const double lw = sqrt(wx * wx + wy * wy);
      ey = (wx * vy - wy * vx) / lw;
      if (!(fabs(ey) <= lim)) continue;
      s = F.key_pts[i - 1][3] + dot / lw;
      ref = psis;
    } else {
      const double r = 1.0 / curv, dir = r > 0 ? 1.0 : -1.0, ar = fabs(r);
      const double xc = xs + ar * cos(psis + dir * hp), yc = ys + ar * sin(psis + dir * hp);
      const double ax = xs - xc, ay = ys - yc, bx = px - xc, by = py - yc;
      const double cur = atan2(ax * by - ay * bx, ax * bx + ay * by);
      if (!(cur * dir > 0.0 && fabs(len / r) >= fabs(cur))) continue;     // swept the segment's way, and not past its end
      ey = -dir * (sqrt(bx * bx + by * by) - ar);
      if (!(fabs(ey) <= lim)) continue;
      s = F.key_pts[i - 1][3] + fabs(cur) * ar;
      ref = psis + cur;
    }
    *s_out = s; *ey_out = ey; *epsi_out = tf_wrap_pi(psi - ref); *resid = 0.0;
    return 0;
  }
  return 2;
}

// cl [n][3] (s, e_y, e_psi) -> xy [n][3] (x, y, psi)
__global__ void dg_spline_l2g_kernel(int64_t n, const double* __restrict__ cl, double* __restrict__ xy) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dev_spline_local_to_global(cl[3 * i], cl[3 * i + 1], cl[3 * i + 2], xy + 3 * i, xy + 3 * i + 1, xy + 3 * i + 2);
}
__global__ void dg_arc_l2g_kernel(int64_t n, dgsqp_sampler_t T, const double* __restrict__ cl, double* __restrict__ xy) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dev_arc_local_to_global(T, cl[3 * i], cl[3 * i + 1], cl[3 * i + 2], xy + 3 * i, xy + 3 * i + 1, xy + 3 * i + 2);
}
// xy [n][3] -> cl [n][3], resid [n] (may be null), status [n]
__global__ void dg_spline_project_kernel(int64_t n, int circuit, double lim, const double* __restrict__ xy, double* __restrict__ cl,
                                         double* __restrict__ resid, int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double r;
    status[i] = dev_spline_project(circuit, lim, xy[3 * i], xy[3 * i + 1], xy[3 * i + 2], cl + 3 * i, cl + 3 * i + 1, cl + 3 * i + 2, &r);
    if (resid) resid[i] = r;
  }
}
__global__ void dg_arc_project_kernel(int64_t n, dgsqp_track_frame_t F, const double* __restrict__ xy, double* __restrict__ cl,
                                      double* __restrict__ resid, int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double r;
    status[i] = dev_arc_project(F, xy[3 * i], xy[3 * i + 1], xy[3 * i + 2], cl + 3 * i, cl + 3 * i + 1, cl + 3 * i + 2, &r);
    if (resid) resid[i] = r;
  }
}

// The placement of scripts/comparison_study_f1/monte_carlo_sampler.py:25-55 on the handle's spline track: car 2 starts AHEAD of car 1, the
// arclength range is limited; six uniforms per candidate in the script's order (s1, e_y1, v1, gap, e_y2, v2).  e_y is clipped to +-ey_clip or,
// with clip_widths, to [-clip_scale right_width(s), clip_scale left_width(s)] (dgsqp_track_width.h).  One lane per candidate ->
// q0[cand][n_q], collide[cand] (1: the two cars overlap).
__global__ void dg_raceline_place_spline_kernel(int64_t n, unsigned long long c0, dgsqp_raceline_spline_sampler_t S, int clip_widths, double clip_scale, DgRaceline R,
                                                double* __restrict__ q0, int32_t* __restrict__ collide) {
  const DgProb& D = dg_prob;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
    const unsigned long long c = c0 + (unsigned long long)i;
    double* q = q0 + i * D.nq;
    for (int t = 0; t < D.nq; t++) q[t] = 0.0;
    double px[2], py[2];
    const double s1 = S.s_lo + (S.s_hi - S.s_lo) * dg_uniform(S.seed, c, 0);
    for (int a = 0; a < 2; a++) {
      const double s = a == 0 ? s1 : s1 + S.gap_lo + (S.gap_hi - S.gap_lo) * dg_uniform(S.seed, c, 3);
      double r[DGSQP_RL_COLS], psi;
      rl_eval(R, rl_s2t(R, s), r);
      double hi = S.ey_clip, lo = -S.ey_clip;
      if (clip_widths) {      // the study's clip: the track's width functions at the car's own s
        double wL, dwL, wR, dwR;
        dev_track_width(s, &wL, &dwL, &wR, &dwR);
        hi = clip_scale * wL; lo = -(clip_scale * wR);
      }
      const double ey = fmax(fmin(r[8] + (2 * dg_uniform(S.seed, c, 3 * a + 1) - 1), hi), lo);
      const double v = r[3] + (1.5 * dg_uniform(S.seed, c, 3 * a + 2) - 0.75);
      dev_spline_local_to_global(s, ey, 0.0, &px[a], &py[a], &psi);
      double* qa = q + D.qoff[a];
      const int nqa = D.nqa[a];
      qa[0] = px[a]; qa[1] = py[a]; qa[2] = v; qa[nqa - 3] = r[6]; qa[nqa - 2] = s; qa[nqa - 1] = ey;
    }
    const double dx = px[0] - px[1], dy = py[0] - py[1];
    collide[i] = (S.collision_d * S.collision_d - (dx * dx + dy * dy) >= 0.0) ? 1 : 0;
  }
}

// The circuit law of dg_sample_place_kernel (DGSQP_comp_monte_carlo.py:365-382) on the handle's spline track: L = track_L, positions
// by dev_spline_local_to_global.  One lane per candidate -> q0[cand][n_q], ok[cand] = 1.
__global__ void dg_sample_place_spline_kernel(int64_t n, unsigned long long c0, dgsqp_sampler_t S, double* __restrict__ q0, int32_t* __restrict__ ok) {
  const DgProb& D = dg_prob;
  const double pi = 3.141592653589793;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
    const unsigned long long c = c0 + (unsigned long long)i;
    double* q = q0 + i * D.nq;
    for (int t = 0; t < D.nq; t++) q[t] = 0.0;
    auto U = [&](int k) { return dg_uniform(S.seed, c, k); };
    auto put = [&](int a, double s, double ey, double v, double epsi) {   // Frenet-frame bicycles: [x, y, v, (..), e_psi, s, e_y]
      double x, y, psi;
      dev_spline_local_to_global(s, ey, 0.0, &x, &y, &psi);
      double* qa = q + D.qoff[a];
      const int nqa = D.nqa[a];
      qa[0] = x; qa[1] = y; qa[2] = v; qa[nqa == 8 ? 5 : 3] = epsi; qa[nqa - 2] = s; qa[nqa - 1] = ey;
    };
    const double s1 = D.P.track_L * U(0), v1 = 2.0 + (U(2) - 0.5);
    put(0, s1, S.half_width * (2 * U(1) - 1), v1, 5.0 * (2 * U(3) - 1) * pi / 180);
    for (int a = 1; a < D.M; a++)
      put(a, s1 + 1.2 * S.obs_d * (2 * U(4 * a) - 1), S.half_width * (2 * U(4 * a + 1) - 1), (1 + 0.25 * (2 * U(4 * a + 2) - 1)) * v1, 5.0 * (2 * U(4 * a + 3) - 1) * pi / 180);
    ok[i] = 1;
  }
}
