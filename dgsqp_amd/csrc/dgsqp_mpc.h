// LTV-MPC reference tracker (DGSQP/solvers/CA_LTV_MPC.py, casadi branch) on the device: dg_mpc_kernel.
//
// One workgroup carries one scenario of one agent through all QP iterations.  The equalities of the reference's QP -- the initial
// condition and z_{k+1} = A_k z_k + B_k du_k + g_k, linearised at (q_k, u_{k-1}) of the current decision vector D -- are eliminated on
// the device: the QP is solved in x = (du_0 .. du_{N-1}, s_ub, s_lb), n = N n_u + 2 n_soft <= 128.
//
// What lives where.  LDS (behind the game's persistent vectors and the track tables, at DgLds.scr): the packed lower triangle of the
// condensed Hessian, overwritten by its Cholesky factor L and then by J = L^-1 (n (n + 1) / 2 doubles: 66 KB at n = 128); D, D_bar,
// (q0, u_prev); the QP's n-vectors, active list and row flags.  Global scratch of the workgroup (about 0.8 MB at n = 128: served by
// L2 / MALL for small n, HBM traffic at the limit): A_k | B_k, f_d, g_k, the
// affine trajectory, the sensitivities S_k = dq_k / dx [N][n_q][n], and the active-set factor: the orthonormal basis Qm of the active
// rows' images J a_i (n x n) and the inverse triangular factor Rinv (J A_W' = Qm R).
//
// The QP is a dense dual active-set method (Goldfarb-Idnani) over rows `sign * value <= sign * bound` of seven kinds (dgsqp.h,
// DGSQP_MPC_ROW_*): unit rows (rate boxes, slack signs), cumulative-sum rows (input boxes, u_k = u_prev + dt sum_{j<=k} du_j) and
// dense rows (state boxes, soft-bound rows, obstacle rows, track-edge rows: rows of S_k).  Box rows whose bound has magnitude >= 1e9 are not generated
// (the host builds the table): they cannot be active.  Every sum runs in a fixed order and nothing is accumulated with atomics: two runs
// of a batch agree bit for bit.  An infeasible QP, a non-finite value or a Hessian that is not positive definite ends the solve with
// DGSQP_QP_FAIL.
//
// Track-edge rows (edge_rows = 1): e_y - left_width(s) <= 0 and -right_width(s) - e_y <= 0 at stages 1..N, linearised about D as the obstacle
// row is.  The width functions are looked up once per QP, not per row and column: mpc_condense fills one record (w_L, w_L', w_R, w_R')
// per stage at the s of D, one lane per stage, into LDS (o_wid, 4 N doubles); rows and gradients read it behind the barriers that follow.
#pragma once

namespace dg_mpc {

#define DG_MPC_UTOL 1e-12   // a u_prev this close (relative to max(1, |bound|)) beyond an input bound counts as on it

struct DgMpcDev {
  dgsqp_mpc_t c;
  int nqa, nz, n, ns, nrows, lenD, mdl, spl, max_steps, pad_;
  double dt, omd;                     // the game's dt; 1 - damping
  // LDS offsets (doubles)
  int o_J, o_g, o_y, o_x, o_a, o_d, o_z, o_w, o_r, o_lam, o_act, o_D, o_Db, o_P0, o_flag, o_wid, o_end;
  // scratch offsets (doubles) of one workgroup
  int64_t ws_AB, ws_f, ws_gk, ws_qbar, ws_S, ws_Qm, ws_Ri, ws_doubles;
  const dgsqp_mpc_row_t* rows;
  const double *q0, *u_ws, *du_ws, *q_ref, *p_obs;
  double *q_pred, *u_pred, *du_pred, *ws, *logD, *logDb, *loglam;
  int32_t *status, *qp_steps;
};

// The warm start's rollout, one lane.  It runs dev_fd in the first-order Taylor type with a zero direction (the value part is the same
// arithmetic): the degree-0 dev_fd is the solver's rollout, and a second caller of that instantiation changes how the compiler inlines
// it there (dev_rollout_multi came out different), while the first-order one is only reached through dev_fd_t by the derivative items.
template <int MDL, bool SPL>
__device__ __noinline__ void mpc_rollout(const DgMpcDev& M, lptr Dl) {
  typedef Ty<1> T;
  constexpr int NQA = dg_model_nq(MDL);
  const dgsqp_problem_t& P = dg_prob.P;
  const dgsqp_agent_t& ag = P.agents[M.c.agent];
  const int nz = NQA + DGSQP_NUA;
  T q[NQA], qn[NQA], u[DGSQP_NUA];
#pragma unroll
  for (int i = 0; i < NQA; i++) { q[i].c[0] = Dl[i]; q[i].c[1] = 0.0; }
  for (int k = 0; k < M.c.N; k++) {
    for (int j = 0; j < DGSQP_NUA; j++) { u[j].c[0] = Dl[(k + 1) * nz + NQA + j]; u[j].c[1] = 0.0; }
    dev_fd<1, MDL, SPL>(P, ag, q, u, qn);
#pragma unroll
    for (int i = 0; i < NQA; i++) { q[i].c[0] = qn[i].c[0]; q[i].c[1] = 0.0; Dl[(k + 1) * nz + i] = qn[i].c[0]; }
  }
}
// column `dir` of [A_k | B_k] = [fAd fBd](q_k, u_{k-1}) (and f_d itself from direction 0): dev_fd in first-order Taylor arithmetic
template <int MDL, bool SPL>
__device__ __noinline__ void mpc_lin_item(const DgMpcDev& M, clptr Dl, gptr ws, int k, int dir) {
  typedef Ty<1> T;
  constexpr int NQA = dg_model_nq(MDL);
  const dgsqp_problem_t& P = dg_prob.P;
  const dgsqp_agent_t& ag = P.agents[M.c.agent];
  const int nz = NQA + DGSQP_NUA;
  T q[NQA], out[NQA], u[DGSQP_NUA];
#pragma unroll
  for (int i = 0; i < NQA; i++) { q[i].c[0] = Dl[k * nz + i]; q[i].c[1] = i == dir ? 1.0 : 0.0; }
#pragma unroll
  for (int j = 0; j < DGSQP_NUA; j++) { u[j].c[0] = Dl[k * nz + NQA + j]; u[j].c[1] = NQA + j == dir ? 1.0 : 0.0; }
  dev_fd<1, MDL, SPL>(P, ag, q, u, out);
  gptr AB = ws + M.ws_AB + (int64_t)k * NQA * nz;
  for (int o = 0; o < NQA; o++) AB[o * nz + dir] = out[o].c[1];
  if (dir == 0) {
    gptr f = ws + M.ws_f + k * NQA;
    for (int o = 0; o < NQA; o++) f[o] = out[o].c[0];
  }
}
__device__ inline void mpc_rollout_any(const DgMpcDev& M, lptr Dl) {
  dev_with_model(M.mdl, M.spl, [&](auto m) { mpc_rollout<decltype(m)::MDL, decltype(m)::SPL>(M, Dl); });
}
__device__ inline void mpc_lin_any(const DgMpcDev& M, clptr Dl, gptr ws, int k, int dir) {
  dev_with_model(M.mdl, M.spl, [&](auto m) { mpc_lin_item<decltype(m)::MDL, decltype(m)::SPL>(M, Dl, ws, k, dir); });
}

__device__ inline int tri(int i) { return i * (i + 1) / 2; }

// Linearisation about D, sensitivities, the condensed Hessian (packed, LDS) and gradient.  Block-cooperative.
__device__ __noinline__ void mpc_condense(const DgMpcDev& M, gptr ws, int64_t b) {
  const int N = M.c.N, nq = M.nqa, nz = M.nz, n = M.n, ns = M.ns, ndu = N * DGSQP_NUA;
  clptr Dl = LP(M.o_D);
  clptr P0 = LP(M.o_P0);
  // A_k | B_k and f_d at (q_k, u_{k-1}), k < N
  for (int it = TID; it < N * nz; it += NT) mpc_lin_any(M, Dl, ws, it / nz, it % nz);
  if (M.c.edge_rows) {      // the track's widths and their slopes at s_k of D, k = 1..N (record k - 1)
    lptr wid = LP(M.o_wid);
    for (int k = TID; k < N; k += NT) {
      double wL, dwL, wR, dwR;
      dev_track_width(Dl[(k + 1) * nz + nq - 2], &wL, &dwL, &wR, &dwR);
      wid[4 * k] = wL; wid[4 * k + 1] = dwL; wid[4 * k + 2] = wR; wid[4 * k + 3] = dwR;
    }
  }
  __syncthreads();
  gptr AB = ws + M.ws_AB, gk = ws + M.ws_gk, qbar = ws + M.ws_qbar, S = ws + M.ws_S;
  cgptr f = ws + M.ws_f;
  for (int it = TID; it < N * nq; it += NT) {
    const int k = it / nq, i = it % nq;
    double s = f[it];
    for (int j = 0; j < nz; j++) s -= AB[(k * nq + i) * nz + j] * Dl[k * nz + j];
    gk[it] = s;
  }
  __syncthreads();
  // S_k (k = 1..N, stored at k - 1) one lane per column, and the affine trajectory (x = 0) on lane n
  for (int col = TID; col <= n; col += NT) {
    double v[DGSQP_MAX_NQA], w[DGSQP_MAX_NQA];
    const bool aff = col == n;
    const int sc = col / DGSQP_NUA, cc = col % DGSQP_NUA;       // a du column: its stage and channel
#pragma unroll
    for (int i = 0; i < DGSQP_MAX_NQA; i++) v[i] = aff && i < nq ? P0[i] : 0.0;
    if (aff) for (int i = 0; i < nq; i++) qbar[i] = P0[i];
    for (int k = 0; k < N; k++) {
      cgptr A = AB + (int64_t)k * nq * nz;
      // d u_{k} / d x: dt on the du columns of the stages <= k; the affine part carries u_prev
      const bool on = !aff && col < ndu && sc <= k;
#pragma unroll
      for (int i = 0; i < DGSQP_MAX_NQA; i++) {
        double s = 0.0;
        if (i < nq) {
          for (int j = 0; j < nq; j++) s += A[i * nz + j] * v[j];
          if (on) s += A[i * nz + nq + cc] * M.dt;
          if (aff) { s += A[i * nz + nq] * P0[nq]; s += A[i * nz + nq + 1] * P0[nq + 1]; s += gk[k * nq + i]; }
        }
        w[i] = s;
      }
#pragma unroll
      for (int i = 0; i < DGSQP_MAX_NQA; i++) v[i] = w[i];
      if (aff) { for (int i = 0; i < nq; i++) qbar[(k + 1) * nq + i] = v[i]; }
      else for (int i = 0; i < nq; i++) S[((int64_t)k * nq + i) * n + col] = v[i];
    }
  }
  __syncthreads();
  // H_c, packed lower triangle
  lptr H = LP(M.o_J);
  const int npk = tri(n);
  for (int t = TID; t < npk; t += NT) {
    int i = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (tri(i + 1) <= t) i++;
    while (tri(i) > t) i--;
    const int j = t - tri(i);      // j <= i
    double s = 0.0;
    if (i < ndu) {
      const int si = i / DGSQP_NUA, ci = i % DGSQP_NUA, cj = j % DGSQP_NUA;
      for (int k = si; k < N; k++)       // S_{k+1}: columns of the stages <= k
        for (int r = 0; r < nq; r++) s += S[((int64_t)k * nq + r) * n + i] * (M.c.w_q[r] + 1e-10) * S[((int64_t)k * nq + r) * n + j];
      if (ci == cj) s += M.dt * M.dt * (M.c.w_u[ci] + 1e-10) * (double)(N - si);
      if (i == j) s += M.c.w_du[ci];
    } else if (i == j) s = 2.0 * M.c.soft_quad[(i - ndu) % ns];
    H[t] = s;
  }
  lptr g = LP(M.o_g);
  const double* qref = M.q_ref + b * (int64_t)(N + 1) * nq;
  for (int i = TID; i < n; i += NT) {
    double s = 0.0;
    if (i < ndu) {
      const int si = i / DGSQP_NUA, ci = i % DGSQP_NUA;
      for (int k = si; k < N; k++)
        for (int r = 0; r < nq; r++) {
          const double lin = -M.c.w_q[r] * qref[(k + 1) * nq + r] + (k + 1 == N ? M.c.c_N[r] : 0.0);
          s += S[((int64_t)k * nq + r) * n + i] * ((M.c.w_q[r] + 1e-10) * qbar[(k + 1) * nq + r] + lin);
        }
      s += M.dt * (M.c.w_u[ci] + 1e-10) * P0[nq + ci] * (double)(N - si);
    } else s = M.c.soft_lin[(i - ndu) % ns];
    g[i] = s;
  }
  __syncthreads();
}

// H (packed, LDS) -> L -> J = L^-1, in place.  Returns false when H is not positive definite (uniform).
__device__ __noinline__ bool mpc_factor(const DgMpcDev& M) {
  const int n = M.n;
  lptr H = LP(M.o_J);
  bool ok = true;
  for (int j = 0; j < n; j++) {
    const double hjj = H[tri(j) + j];
    if (!(hjj > 0.0) || !isfinite(hjj)) { ok = false; break; }     // uniform: every lane reads the same word
    const double d = sqrt(hjj);
    __syncthreads();
    for (int i = j + TID; i < n; i += NT) H[tri(i) + j] = i == j ? d : H[tri(i) + j] / d;
    __syncthreads();
    for (int i = j + 1 + TID; i < n; i += NT) {
      const double lij = H[tri(i) + j];
      for (int k = j + 1; k <= i; k++) H[tri(i) + k] -= lij * H[tri(k) + j];
    }
    __syncthreads();
  }
  __syncthreads();
  if (!ok) return false;
  for (int j = n - 1; j >= 0; j--) {
    const double ijj = 1.0 / H[tri(j) + j];
    double s[(DGSQP_MPC_NMAX + NT - 1) / NT];
    int c = 0;
    for (int i = j + 1 + TID; i < n; i += NT, c++) {
      double t = 0.0;
      for (int k = j + 1; k <= i; k++) t += H[tri(i) + k] * H[tri(k) + j];
      s[c] = -t * ijj;
    }
    __syncthreads();
    c = 0;
    for (int i = j + 1 + TID; i < n; i += NT, c++) H[tri(i) + j] = s[c];
    if (TID == 0) H[tri(j) + j] = ijj;
    __syncthreads();
  }
  return true;
}

// out = J in (lower triangular product), out' = J' in
__device__ inline void mpc_J_mul(const DgMpcDev& M, clptr in, lptr out) {
  clptr J = LP(M.o_J);
  for (int i = TID; i < M.n; i += NT) {
    double s = 0.0;
    for (int j = 0; j <= i; j++) s += J[tri(i) + j] * in[j];
    out[i] = s;
  }
  __syncthreads();
}
__device__ inline void mpc_Jt_mul(const DgMpcDev& M, clptr in, lptr out) {
  clptr J = LP(M.o_J);
  for (int j = TID; j < M.n; j += NT) {
    double s = 0.0;
    for (int i = j; i < M.n; i++) s += J[tri(i) + j] * in[i];
    out[j] = s;
  }
  __syncthreads();
}

// D_bar of the condensed point x: du and slacks, the inputs by their running sum, the states by the linearised dynamics
__device__ __noinline__ void mpc_expand(const DgMpcDev& M, gptr ws) {
  const int N = M.c.N, nq = M.nqa, nz = M.nz, n = M.n;
  clptr x = LP(M.o_x), P0 = LP(M.o_P0);
  lptr Db = LP(M.o_Db);
  for (int i = TID; i < n; i += NT) Db[(N + 1) * nz + i] = x[i];
  if (TID < nz) Db[TID] = P0[TID];
  if (TID < DGSQP_NUA) {
    double v = P0[nq + TID];
    for (int k = 0; k < N; k++) { v += M.dt * x[k * DGSQP_NUA + TID]; Db[(k + 1) * nz + nq + TID] = v; }
  }
  __syncthreads();
  cgptr AB = ws + M.ws_AB, gk = ws + M.ws_gk;
  for (int k = 0; k < N; k++) {
    if (TID < nq) {
      cgptr A = AB + ((int64_t)k * nq + TID) * nz;
      double s = gk[k * nq + TID];
      for (int j = 0; j < nq; j++) s += A[j] * Db[k * nz + j];
      s += A[nq] * Db[(k + 1) * nz + nq];
      s += A[nq + 1] * Db[(k + 1) * nz + nq + 1];
      Db[(k + 1) * nz + TID] = s;
    }
    __syncthreads();
  }
}

// sign * value - sign * bound of row R at D_bar (> 0: violated)
__device__ inline double mpc_row_res(const DgMpcDev& M, const dgsqp_mpc_row_t R, int64_t b) {
  const int N = M.c.N, nq = M.nqa, nz = M.nz, ns = M.ns;
  clptr Db = LP(M.o_Db), Dl = LP(M.o_D);
  const int sb = (N + 1) * nz + N * DGSQP_NUA;
  switch (R.kind) {
    case DGSQP_MPC_ROW_RATE: { const double v = Db[(N + 1) * nz + R.stage * DGSQP_NUA + R.index]; return R.sign > 0 ? v - M.c.du_ub[R.index] : M.c.du_lb[R.index] - v; }
    case DGSQP_MPC_ROW_SLACK: return -Db[sb + R.index];
    case DGSQP_MPC_ROW_INPUT: { const double v = Db[R.stage * nz + nq + R.index]; return R.sign > 0 ? v - M.c.u_ub[R.index] : M.c.u_lb[R.index] - v; }
    case DGSQP_MPC_ROW_STATE: { const double v = Db[R.stage * nz + R.index]; return R.sign > 0 ? v - M.c.q_ub[R.index] : M.c.q_lb[R.index] - v; }
    case DGSQP_MPC_ROW_SOFT: {
      const int j = M.c.soft_idx[R.index];
      const double v = Db[R.stage * nz + j];
      return R.sign > 0 ? v - Db[sb + R.index] - M.c.q_ub[j] : M.c.q_lb[j] - v - Db[sb + ns + R.index];
    }
    case DGSQP_MPC_ROW_EDGE: {      // c(q_bar) + grad c (q - q_bar); left (+1): c = e_y - w_L(s), right (-1): c = -w_R(s) - e_y
      clptr w = LP(M.o_wid) + 4 * (R.stage - 1);
      const double s0 = Dl[R.stage * nz + nq - 2], e0 = Dl[R.stage * nz + nq - 1];
      const double ds = Db[R.stage * nz + nq - 2] - s0, de = Db[R.stage * nz + nq - 1] - e0;
      return R.sign > 0 ? (e0 - w[0]) - w[1] * ds + de : (-w[2] - e0) - w[3] * ds - de;
    }
    default: {
      const double* p = M.p_obs + (b * N + (R.stage - 1)) * 2;
      const double x0 = Dl[R.stage * nz], y0 = Dl[R.stage * nz + 1], dx = x0 - p[0], dy = y0 - p[1];
      const double C = 4.0 * M.c.obs_r * M.c.obs_r - (dx * dx + dy * dy);
      return C - 2.0 * dx * (Db[R.stage * nz] - x0) - 2.0 * dy * (Db[R.stage * nz + 1] - y0);
    }
  }
}
// the row's gradient in x, into a[n].  Block-cooperative.
__device__ inline void mpc_row_grad(const DgMpcDev& M, gptr ws, const dgsqp_mpc_row_t R, int64_t b, lptr a) {
  const int N = M.c.N, nq = M.nqa, nz = M.nz, n = M.n, ns = M.ns, ndu = N * DGSQP_NUA;
  cgptr S = ws + M.ws_S;
  clptr Dl = LP(M.o_D);
  const double sg = (double)R.sign;
  for (int col = TID; col < n; col += NT) {
    double v = 0.0;
    const int sc = col / DGSQP_NUA, cc = col % DGSQP_NUA;
    switch (R.kind) {
      case DGSQP_MPC_ROW_RATE: v = col == R.stage * DGSQP_NUA + R.index ? sg : 0.0; break;
      case DGSQP_MPC_ROW_SLACK: v = col == ndu + R.index ? -1.0 : 0.0; break;
      case DGSQP_MPC_ROW_INPUT: v = col < ndu && cc == R.index && sc < R.stage ? sg * M.dt : 0.0; break;
      case DGSQP_MPC_ROW_STATE: v = sg * S[((int64_t)(R.stage - 1) * nq + R.index) * n + col]; break;
      case DGSQP_MPC_ROW_SOFT:
        v = sg * S[((int64_t)(R.stage - 1) * nq + M.c.soft_idx[R.index]) * n + col];
        if (col == ndu + (R.sign > 0 ? 0 : ns) + R.index) v = -1.0;
        break;
      case DGSQP_MPC_ROW_EDGE: {
        clptr w = LP(M.o_wid) + 4 * (R.stage - 1);
        v = sg * S[((int64_t)(R.stage - 1) * nq + nq - 1) * n + col] - (R.sign > 0 ? w[1] : w[3]) * S[((int64_t)(R.stage - 1) * nq + nq - 2) * n + col];
        break;
      }
      default: {
        const double* p = M.p_obs + (b * N + (R.stage - 1)) * 2;
        const double dx = Dl[R.stage * nz] - p[0], dy = Dl[R.stage * nz + 1] - p[1];
        v = -2.0 * (dx * S[((int64_t)(R.stage - 1) * nq) * n + col] + dy * S[((int64_t)(R.stage - 1) * nq + 1) * n + col]);
      }
    }
    a[col] = v;
  }
  __syncthreads();
}

// With the gradient of a row in a[]: d = J a, w = Qm' d over the first cnt basis vectors (Gram-Schmidt, two passes), z = d - Qm w,
// r = Rinv w.  Returns |z|^2; dd = |d|^2.
__device__ __noinline__ double mpc_project(const DgMpcDev& M, gptr ws, int cnt, double& dd) {
  const int n = M.n;
  cgptr Qm = ws + M.ws_Qm, Ri = ws + M.ws_Ri;
  lptr d = LP(M.o_d), z = LP(M.o_z), w = LP(M.o_w), r = LP(M.o_r), red = LP(dg_prob.L.red);
  mpc_J_mul(M, LP(M.o_a), d);
  for (int pass = 0; pass < 2; pass++) {
    clptr src = pass ? z : d;
    double wi[(DGSQP_MPC_NMAX + NT - 1) / NT];
    int c = 0;
    for (int i = TID; i < cnt; i += NT, c++) {
      double s = 0.0;
      for (int j = 0; j < n; j++) s += Qm[(int64_t)i * n + j] * src[j];
      wi[c] = s;
    }
    c = 0;
    for (int i = TID; i < cnt; i += NT, c++) r[i] = wi[c];       // r: this pass's coefficients
    __syncthreads();
    for (int j = TID; j < n; j += NT) {
      double s = src[j];
      for (int i = 0; i < cnt; i++) s -= r[i] * Qm[(int64_t)i * n + j];
      z[j] = s;
    }
    for (int i = TID; i < cnt; i += NT) w[i] = pass ? w[i] + r[i] : r[i];
    __syncthreads();
  }
  double pd = 0.0, pz = 0.0;
  for (int j = TID; j < n; j += NT) { pd += d[j] * d[j]; pz += z[j] * z[j]; }
  dd = block_sum(pd, red);
  const double zz = block_sum(pz, red);
  for (int i = TID; i < cnt; i += NT) {
    double s = 0.0;
    for (int c = i; c < cnt; c++) s += Ri[(int64_t)c * n + i] * w[c];
    r[i] = s;
  }
  __syncthreads();
  return zz;
}
// the projected row becomes basis vector cnt: Qm[cnt] = z / rho, column cnt of Rinv = (-r / rho, 1 / rho)
__device__ inline void mpc_append(const DgMpcDev& M, gptr ws, int cnt, double zz) {
  const int n = M.n;
  gptr Qm = ws + M.ws_Qm, Ri = ws + M.ws_Ri;
  clptr z = LP(M.o_z), r = LP(M.o_r);
  const double irho = 1.0 / sqrt(zz);
  for (int j = TID; j < n; j += NT) Qm[(int64_t)cnt * n + j] = z[j] * irho;
  for (int i = TID; i <= cnt; i += NT) Ri[(int64_t)cnt * n + i] = i == cnt ? irho : -r[i] * irho;
  __threadfence_block();
  __syncthreads();
}

// One QP at the current D: fills D_bar (LDS) and, with a log, the multipliers.  Returns false on failure.  All branches are uniform:
// every decision is taken on values that block reductions hand to all lanes, or that all lanes read from the same LDS words.
__device__ __noinline__ bool mpc_qp(const DgMpcDev& M, gptr ws, int64_t b, double* loglam, int& steps) {
  const int n = M.n, nrows = M.nrows;
  lptr g = LP(M.o_g), y = LP(M.o_y), x = LP(M.o_x), a = LP(M.o_a), z = LP(M.o_z), r = LP(M.o_r), lam = LP(M.o_lam), red = LP(dg_prob.L.red);
  int* act = (int*)(dg_lds + M.o_act);
  int* flag = (int*)(dg_lds + M.o_flag);
  // u_{-1} is fixed by the initial condition AND bounded by the input box: still outside it after mpc_scenario's clamp, the QP is infeasible
  // (uniform: every lane reads the same words)
  for (int j = 0; j < DGSQP_NUA; j++) {
    const double up = LP(M.o_P0)[M.nqa + j];
    if ((fabs(M.c.u_ub[j]) < 1e9 && up > M.c.u_ub[j]) || (fabs(M.c.u_lb[j]) < 1e9 && up < M.c.u_lb[j]) || !isfinite(up)) return false;
  }
  mpc_condense(M, ws, b);
  if (!mpc_factor(M)) return false;
  for (int i = TID; i < nrows; i += NT) flag[i] = 0;
  mpc_J_mul(M, g, y);
  for (int i = TID; i < n; i += NT) y[i] = -y[i];
  __syncthreads();
  mpc_Jt_mul(M, y, x);
  int q = 0;
  bool ok = false;
  for (int it = 0; it < M.max_steps; it++) {
    mpc_expand(M, ws);
    double v = INFINITY;
    int idx = 0x7fffffff;
    bool bad = false;
    for (int rr = TID; rr < nrows; rr += NT) {
      if (flag[rr]) continue;
      const double res = mpc_row_res(M, M.rows[rr], b);
      if (!isfinite(res)) bad = true;
      argmin_pick(v, idx, -res, rr);
    }
    if (__syncthreads_or(bad ? 1 : 0)) break;
    double vout; int p;
    block_argmin(v, idx, red, vout, p);
    if (!(-vout > 1e-13)) { ok = true; break; }
    steps++;
    const dgsqp_mpc_row_t Rp = M.rows[p];
    double lam_p = 0.0;
    bool added = false, fail = false;
    for (int inner = 0; inner <= n + 1; inner++) {
      mpc_row_grad(M, ws, Rp, b, a);
      double dd;
      const double zz = mpc_project(M, ws, q, dd);
      const double res_p = mpc_row_res(M, Rp, b);
      double t1 = INFINITY; int j1 = 0x7fffffff;
      for (int i = TID; i < q; i += NT)
        if (r[i] > 0.0) argmin_pick(t1, j1, lam[i] / r[i], i);
      double t1o; int j1o;
      block_argmin(t1, j1, red, t1o, j1o);
      const bool dep = !(zz > 1e-24 * dd) || q >= n;
      const double t2 = dep ? INFINITY : res_p / zz;
      if (!(t1o < INFINITY) && dep) { fail = true; break; }      // no step keeps the duals feasible: the QP is infeasible
      if (!isfinite(zz) || !isfinite(dd)) { fail = true; break; }
      const double t = fmin(t1o, t2);
      __syncthreads();
      for (int i = TID; i < q; i += NT) lam[i] -= t * r[i];
      if (!dep) for (int i = TID; i < n; i += NT) y[i] -= t * z[i];
      lam_p += t;
      __syncthreads();
      if (!dep) mpc_Jt_mul(M, y, x);
      if (t2 <= t1o) {      // full step: the row joins the active set
        mpc_append(M, ws, q, zz);
        if (TID == 0) { act[q] = p; lam[q] = lam_p; flag[p] = 1; }
        __syncthreads();
        q++;
        added = true;
        break;
      }
      // partial step: row j1o leaves, the factor is rebuilt from its position on
      steps++;
      const int dropped = act[j1o];
      int an = 0; double ln = 0.0;
      if (TID >= j1o && TID + 1 < q) { an = act[TID + 1]; ln = lam[TID + 1]; }
      __syncthreads();
      if (TID >= j1o && TID + 1 < q) { act[TID] = an; lam[TID] = ln; }
      if (TID == 0) flag[dropped] = 0;
      __syncthreads();
      q--;
      for (int i = j1o; i < q; i++) {
        mpc_row_grad(M, ws, M.rows[act[i]], b, a);
        double dd2;
        const double zz2 = mpc_project(M, ws, i, dd2);
        if (!(zz2 > 1e-24 * dd2)) { fail = true; break; }
        mpc_append(M, ws, i, zz2);
      }
      if (fail) break;
      mpc_expand(M, ws);
    }
    if (fail || !added) break;
  }
  if (!ok) return false;
  // one refinement of the active rows' residuals: y -= Qm Rinv' rho, lam += Rinv Rinv' rho
  if (q > 0) {
    cgptr Qm = ws + M.ws_Qm, Ri = ws + M.ws_Ri;
    lptr w = LP(M.o_w);
    for (int i = TID; i < q; i += NT) r[i] = mpc_row_res(M, M.rows[act[i]], b);
    __syncthreads();
    for (int c = TID; c < q; c += NT) {
      double s = 0.0;
      for (int i = 0; i <= c; i++) s += Ri[(int64_t)c * n + i] * r[i];
      w[c] = s;
    }
    __syncthreads();
    for (int j = TID; j < n; j += NT) {
      double s = y[j];
      for (int c = 0; c < q; c++) s -= w[c] * Qm[(int64_t)c * n + j];
      y[j] = s;
    }
    for (int i = TID; i < q; i += NT) {
      double s = lam[i];
      for (int c = i; c < q; c++) s += Ri[(int64_t)c * n + i] * w[c];
      lam[i] = s;
    }
    __syncthreads();
    mpc_Jt_mul(M, y, x);
    mpc_expand(M, ws);
  }
  if (loglam) {
    for (int i = TID; i < nrows; i += NT) loglam[i] = 0.0;
    __syncthreads();
    for (int i = TID; i < q; i += NT) loglam[act[i]] = lam[i];
  }
  __syncthreads();
  return true;
}

__device__ inline void mpc_scenario(const DgMpcDev& M, gptr ws, int64_t b) {
  const int N = M.c.N, nq = M.nqa, nz = M.nz, lenD = M.lenD, ndu = N * DGSQP_NUA;
  lptr Dl = LP(M.o_D), Db = LP(M.o_Db), P0 = LP(M.o_P0);
  const double* uws = M.u_ws + b * (int64_t)(N + 1) * DGSQP_NUA;
  const double* duws = M.du_ws + b * (int64_t)ndu;
  for (int t = TID; t < (N + 1) * DGSQP_NUA; t += NT) Dl[(t / DGSQP_NUA) * nz + nq + t % DGSQP_NUA] = uws[t];
  for (int t = TID; t < lenD - (N + 1) * nz; t += NT) Dl[(N + 1) * nz + t] = t < ndu ? duws[t] : 0.0;
  if (TID < nq) Dl[TID] = M.q0[b * nq + TID];
  __syncthreads();
  if (TID < nz) {
    // (q0, u_prev) of the initial condition.  u_{-1} is also bounded by the input box (CA_LTV_MPC.py:742-743).  An input the tracker itself
    // returned at its bound comes back as u_prev a few ulp or a row tolerance beyond it (rows are accepted up to 1e-13, the damped update
    // rounds once more): within DG_MPC_UTOL max(1, |bound|) of a bound u_prev is moved onto it, farther outside the QP is infeasible
    double v = Dl[TID];
    if (TID >= nq) {
      const double ub = M.c.u_ub[TID - nq], lb = M.c.u_lb[TID - nq];
      if (fabs(ub) < 1e9 && v > ub && v <= ub + DG_MPC_UTOL * fmax(1.0, fabs(ub))) v = ub;
      if (fabs(lb) < 1e9 && v < lb && v >= lb - DG_MPC_UTOL * fmax(1.0, fabs(lb))) v = lb;
    }
    P0[TID] = v;
  }
  if (TID == 0) mpc_rollout_any(M, Dl);
  __syncthreads();
  // the fallback of a failed QP: the warm start
  double* qp = M.q_pred ? M.q_pred + b * (int64_t)(N + 1) * nq : nullptr;
  double* up = M.u_pred ? M.u_pred + b * (int64_t)ndu : nullptr;
  double* dp = M.du_pred ? M.du_pred + b * (int64_t)ndu : nullptr;
  if (qp) for (int t = TID; t < (N + 1) * nq; t += NT) qp[t] = Dl[(t / nq) * nz + t % nq];
  if (up) for (int t = TID; t < ndu; t += NT) up[t] = uws[DGSQP_NUA + t];
  if (dp) for (int t = TID; t < ndu; t += NT) dp[t] = duws[t];
  int steps = 0;
  bool ok = true;
  const int iters = M.c.qp_iters;
  for (int it = 0; it < iters; it++) {
    double* lD = M.logD ? M.logD + (b * iters + it) * (int64_t)lenD : nullptr;
    double* lB = M.logDb ? M.logDb + (b * iters + it) * (int64_t)lenD : nullptr;
    double* lL = M.loglam ? M.loglam + (b * iters + it) * (int64_t)M.nrows : nullptr;
    if (lD) for (int t = TID; t < lenD; t += NT) lD[t] = ok ? (double)Dl[t] : NAN;
    if (ok) ok = mpc_qp(M, ws, b, lL, steps);
    if (!ok) {
      if (lB) for (int t = TID; t < lenD; t += NT) lB[t] = NAN;
      if (lL) for (int t = TID; t < M.nrows; t += NT) lL[t] = NAN;
      continue;
    }
    if (lB) for (int t = TID; t < lenD; t += NT) lB[t] = Db[t];
    // D <- damping D + (1 - damping) D_bar, each product and the sum rounded once; slacks (zero_du: and du) to zero
    for (int t = TID; t < lenD; t += NT) {
#pragma clang fp contract(off)
      const double v = M.c.damping * Dl[t] + M.omd * Db[t];
      const bool zero = t >= (N + 1) * nz + ndu || (M.c.zero_du && t >= (N + 1) * nz);
      Dl[t] = zero ? 0.0 : v;
    }
    __syncthreads();
  }
  if (ok || M.c.zero_du) {
    if (qp) for (int t = TID; t < (N + 1) * nq; t += NT) qp[t] = Dl[(t / nq) * nz + t % nq];
    if (up) for (int t = TID; t < ndu; t += NT) up[t] = Dl[(t / DGSQP_NUA + 1) * nz + nq + t % DGSQP_NUA];
    if (dp) for (int t = TID; t < ndu; t += NT) dp[t] = Dl[(N + 1) * nz + t];
  }
  if (TID == 0) {
    if (M.status) M.status[b] = ok ? 0 : DGSQP_QP_FAIL;
    if (M.qp_steps) M.qp_steps[b] = steps;
  }
  __syncthreads();
}

// The grid is smaller than the batch: workgroup g takes scenarios g, g + grid, ...  Nothing of a scenario survives in LDS or scratch
// for the next: every word read is written first.
__global__ void __launch_bounds__(DG_BLOCK)
dg_mpc_kernel(int64_t B, const DgMpcDev* __restrict__ Mp) {
  const DgMpcDev& M = *Mp;
  dev_load_tables();
  gptr ws = (gptr)M.ws + (int64_t)blockIdx.x * M.ws_doubles;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();
    mpc_scenario(M, ws, b);
  }
}

}  // namespace dg_mpc
