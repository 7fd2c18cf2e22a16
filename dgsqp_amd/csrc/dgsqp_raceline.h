// Raceline warm starts: the front end of scripts/comparison_study_barc/monte_carlo_main.py on the device (include/dgsqp.h).
//   the table        track_lib.load_mpclab_raceline: knots T [n] and nine columns (x, y, psi, v_long, v_tran, psidot, e_psi, s, e_y)
//   rl_s2t, rl_eval  its two look-ups
//   dg_raceline_ref_kernel, dg_ws_chain_kernel, dg_ws_assemble_kernel   the pieces of warm_start_dynamic.py:145-165 around the two launches
//                    of dg_mpc_kernel (which is not touched)
//   dg_raceline_place_kernel   the placement of monte_carlo_sampler_dynamic.py:27-57
// Interpolation, both look-ups: the segment [x0, x1] with x0 <= x < x1 is found by binary search (the study's table has 4,401 knots),
// and the value is   y0 + (y1 - y0) * ((x - x0) / (x1 - x0))   in exactly that operation order, every operation rounded once (no
// fused multiply-add), so that the numpy mirror (montecarlo.Raceline) computes the same bits.  Below the first knot the first segment
// and above the last knot the last segment are continued linearly by the same formula.
#pragma once

struct DgRaceline {
  int n;                   // knots
  const double* T;         // [n]
  const double* cols;      // [n][DGSQP_RL_COLS]
};

// largest i in 0 .. n - 2 with X[i stride] <= x (0 when there is none): the segment the formula runs on
__device__ inline int rl_segment(const double* X, int stride, int n, double x) {
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (x >= X[(int64_t)mid * stride]) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ inline double rl_lerp(double x, double x0, double x1, double y0, double y1) {
#pragma clang fp contract(off)
  const double w = (x - x0) / (x1 - x0);
  const double d = (y1 - y0) * w;
  return y0 + d;
}
__device__ inline double rl_s2t(const DgRaceline& R, double s) {
  const double* S = R.cols + 7;
  const int i = rl_segment(S, DGSQP_RL_COLS, R.n, s);
  return rl_lerp(s, S[(int64_t)i * DGSQP_RL_COLS], S[(int64_t)(i + 1) * DGSQP_RL_COLS], R.T[i], R.T[i + 1]);
}
__device__ inline void rl_eval(const DgRaceline& R, double t, double* out /* [DGSQP_RL_COLS] */) {
  const int i = rl_segment(R.T, 1, R.n, t);
  const double t0 = R.T[i], t1 = R.T[i + 1];
  const double* r0 = R.cols + (int64_t)i * DGSQP_RL_COLS;
  const double* r1 = r0 + DGSQP_RL_COLS;
  for (int c = 0; c < DGSQP_RL_COLS; c++) out[c] = rl_lerp(t, t0, t1, r0[c], r1[c]);
}

// The tracker's inputs for every agent, one lane per (scenario, agent, stage k = 0..N): warm_start_dynamic.py:148-155.
//   q0a   [M][B][n_qa]          the agent's own state (the tracker's q0)
//   q_ref [M][B][N+1][n_qa]     agent after agent: each agent's block is what dg_mpc_kernel reads
//   u_ws  [B][N+1][n_u], du_ws [B][N][n_u]   the constants of warm_start_dynamic.py:156-157 (the same for every agent)
// Every agent has n_qa states and a Frenet-frame bicycle model (the host checks it).
__global__ void dg_raceline_ref_kernel(int64_t B, DgRaceline R, const double* __restrict__ x0, double u_init, double du_init,
                                       double* __restrict__ q0a, double* __restrict__ q_ref, double* __restrict__ u_ws, double* __restrict__ du_ws) {
  const DgProb& D = dg_prob;
  const int N = D.N, M = D.M, nqa = D.nqa[0];
  const int64_t lanes = B * M * (N + 1);
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < lanes; it += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
    const int k = (int)(it % (N + 1));
    const int a = (int)((it / (N + 1)) % M);
    const int64_t b = it / ((int64_t)(N + 1) * M);
    const double* q = x0 + b * D.nq + D.qoff[a];
    const double s0 = q[nqa - 2], ey0 = q[nqa - 1], v0 = q[2];
    double r[DGSQP_RL_COLS];
    const double t0 = rl_s2t(R, s0);
    rl_eval(R, t0, r);
    const double offset = ey0 - r[8];
    const double scaling = v0 / r[3];
    const double tk = t0 + D.P.dt * (double)k * scaling;
    rl_eval(R, tk, r);
    double* o = q_ref + (((int64_t)a * B + b) * (N + 1) + k) * nqa;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[3] * scaling;
    if (nqa == 8) { o[3] = r[4] * scaling; o[4] = r[5] * scaling; }
    o[nqa - 3] = r[6]; o[nqa - 2] = r[7]; o[nqa - 1] = r[8] + offset;
    if (k == 0) {
      double* oq = q0a + ((int64_t)a * B + b) * nqa;
      for (int i = 0; i < nqa; i++) oq[i] = q[i];
    }
    if (a == 0) {
      for (int j = 0; j < DGSQP_NUA; j++) {
        u_ws[(b * (N + 1) + k) * DGSQP_NUA + j] = u_init;
        if (k < N) du_ws[(b * N + k) * DGSQP_NUA + j] = du_init;
      }
    }
  }
}

// CA_LTV_MPC.set_warm_start after its loop (CA_LTV_MPC.py:198-201): u_ws <- (u_ws[0], u_pred), du_ws <- du_pred.  One lane per
// (scenario, stage, input).
__global__ void dg_ws_chain_kernel(int64_t B, int N, const double* __restrict__ u_ws, const double* __restrict__ u_pred,
                                   const double* __restrict__ du_pred, double* __restrict__ u_ws2, double* __restrict__ du_ws2) {
  const int64_t per = (int64_t)(N + 1) * DGSQP_NUA, lanes = B * per;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < lanes; it += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = it / per;
    const int t = (int)(it % per);
    if (t < DGSQP_NUA) { u_ws2[it] = u_ws[it]; continue; }
    const int64_t src = b * (int64_t)N * DGSQP_NUA + (t - DGSQP_NUA);
    u_ws2[it] = u_pred[src];
    du_ws2[src] = du_pred[src];
  }
}

// The agent's u_pred [B][N][n_u] into the game's agent-major u_ws [B][n]; ok[b] = (first agent ? 1 : ok[b]) & (status[b] == 0).
__global__ void dg_ws_assemble_kernel(int64_t B, int N, int n, int agent, const double* __restrict__ u_pred, const int32_t* __restrict__ status,
                                      double* __restrict__ u_out, int32_t* __restrict__ ok) {
  const int64_t per = (int64_t)N * DGSQP_NUA, lanes = B * per;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < lanes; it += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = it / per;
    const int t = (int)(it % per);
    u_out[b * n + (int64_t)agent * per + t] = u_pred[it];
    if (t == 0) ok[b] = ((agent == 0) ? 1 : ok[b]) & (status[b] == 0 ? 1 : 0);
  }
}

// one lane per candidate: monte_carlo_sampler_dynamic.py:27-57 -> q0[cand][n_q], collide[cand] (1: the two cars overlap).  T carries the
// track's key points for dg_local_to_global.
__global__ void dg_raceline_place_kernel(int64_t n, unsigned long long c0, dgsqp_raceline_sampler_t S, dgsqp_sampler_t T, DgRaceline R,
                                         double* __restrict__ q0, int32_t* __restrict__ collide) {
  const DgProb& D = dg_prob;
  const double L = S.key_pts[S.n_key - 1][3], lim = 0.9 * S.half_width;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
    const unsigned long long c = c0 + (unsigned long long)i;
    double* q = q0 + i * D.nq;
    for (int t = 0; t < D.nq; t++) q[t] = 0.0;
    double px[2], py[2];
    const double s1 = L * dg_uniform(S.seed, c, 0);
    for (int a = 0; a < 2; a++) {
      const double s = a == 0 ? s1 : s1 + 1.2 * S.obs_d * (2 * dg_uniform(S.seed, c, 3) - 1);
      double r[DGSQP_RL_COLS];
      rl_eval(R, rl_s2t(R, s), r);
      const double ey = fmax(fmin(r[8] + (2 * dg_uniform(S.seed, c, 3 * a + 1) - 1), lim), -lim);
      const double v = r[3] + (1.5 * dg_uniform(S.seed, c, 3 * a + 2) - 0.75);
      dg_local_to_global(T, s, ey, &px[a], &py[a]);
      double* qa = q + D.qoff[a];
      const int nqa = D.nqa[a];
      qa[0] = px[a]; qa[1] = py[a]; qa[2] = v; qa[nqa - 3] = r[6]; qa[nqa - 2] = s; qa[nqa - 1] = ey;
    }
    const double dx = px[0] - px[1], dy = py[0] - py[1];
    collide[i] = (S.collision_d * S.collision_d - (dx * dx + dy * dy) >= 0.0) ? 1 : 0;
  }
}
