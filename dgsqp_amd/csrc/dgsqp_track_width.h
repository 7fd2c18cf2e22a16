// Track width functions on the device (include/dgsqp.h: dgsqp_problem_t.widths): the reference's
//   left_width(s) = pw_lin(sbar, s_waypoints, left_width),  sbar = fmod(fmod(s, L) + L, L)      (casadi_bspline_track.py:61-64)
// and right_width likewise, on the handle's table dg_prob.wid = [n_width][3] rows (knot, left, right) in global memory next to the spline
// table.  Piece i is the largest one with K_i <= sbar, clamped to 0 .. n_width - 2 (right-continuous at a knot); value and slope are
//   w = (w_{i+1} - w_i) / (K_{i+1} - K_i) * (sbar - K_i) + w_i,   w' = (w_{i+1} - w_i) / (K_{i+1} - K_i)
// with every operation rounded once (no fused multiply-add), so they carry the bits of the numpy mirror (tracks._WidthFunctions).
#pragma once

// the piece of a finite sbar: bisection on the knots, at most ceil(log2 n_width) steps whatever their spacing
__device__ inline int tw_piece(double sbar) {
  const double* tab = dg_prob.wid;
  int lo = 0, hi = dg_prob.P.n_width - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (sbar >= tab[3 * mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// (w_L, w_L', w_R, w_R') at arclength s; NaN when s is not finite (no table is indexed with it).  The handle has a table (n_width >= 2):
// the callers' entry points have checked that.
__device__ inline void dev_track_width(double s, double* wL, double* dwL, double* wR, double* dwR) {
#pragma clang fp contract(off)
  if (!__builtin_isfinite(s)) { *wL = *dwL = *wR = *dwR = __builtin_nan(""); return; }
  const double sbar = fmod(fmod(s, dg_prob.P.track_L) + dg_prob.P.track_L, dg_prob.P.track_L);
  const int i = tw_piece(sbar);
  const double* r0 = dg_prob.wid + 3 * i;
  const double* r1 = r0 + 3;
  const double t = sbar - r0[0], dk = r1[0] - r0[0];
  *dwL = (r1[1] - r0[1]) / dk;
  *dwR = (r1[2] - r0[2]) / dk;
  *wL = *dwL * t + r0[1];
  *wR = *dwR * t + r0[2];
}
