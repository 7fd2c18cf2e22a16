// Closed-loop (receding-horizon) batches in one launch: one workgroup carries one scenario through all T steps of DGSQP.step()
// (DGSQP.py:283-297), so that a launch is bounded by its longest CHAIN and no intermediate state leaves the device.
// Included by dgsqp_api.hip after dg_solve_kernel; host mirror of the feedback rule: dgsqp_amd/closed_loop.py.
#pragma once

// Step-major buffers of one closed-loop launch.  q and uws are FED BACK: the workgroup writes slice t + 1 and its own next solve
// reads it, so they are plain pointers -- never const, never __restrict__ -- and every slice has an address of its own.
struct DgClosedLoop {
  int T;
  double* q;             // [T+1][B][nq]   slice 0 = x0, slice t + 1 = state the plant reached after step t
  double* uws;           // [T+1][B][n]    slice t = warm start step t started from (agent-major)
  const double* w;       // [T][B][nq]     disturbance added to the plant's next state, or null (only ever read)
  SolveOutPtrs O;        // records of step 0; step t sits t * B * stride further on (O.l may be null)
  int64_t x_step;        // doubles between the prediction slices of consecutive steps: B (N+1) nq, or 0 when the caller keeps no
                         // predictions (one [B][N+1][nq] slice, reused by every step: x_t[b][1] has to exist somewhere)
  int32_t* steps_done;   // [B]
};

// Per ticket b, for t = 0 .. T-1: solve from (q[t][b], uws[t][b]) exactly as dg_solve_kernel would, then
//   q[t+1][b]   = x_t[b][1] (+ w[t][b])                          the game's own discrete model is the plant
//   uws[t+1][b] = shift(u_t[b]), or uws[t][b] after 'diverged' / 'qp_fail'   (DGSQP.py:293-295)
// shift, per agent: row k takes row k + 1, the last row is repeated (np.vstack((u_pred[1:], u_pred[-1]))).
// A non-finite q[t+1][b] ends the chain: steps_done[b] = t + 1, and no solve starts from such a state (q[t+1][b] keeps that state,
// uws[t+1][b] is not written).  The records of steps that never ran keep what the host filled them with before the launch
// (status DGSQP_NOT_RUN, zero counts, NaN).
// No cooperative line search, no deferral, no event or iterate log: a chain's next solve depends on its last one.
__global__ void __launch_bounds__(DG_BLOCK, 2)
dg_closed_loop_kernel(int64_t B, DgClosedLoop cl, double* __restrict__ ws_all, unsigned long long* __restrict__ ticket) {
  Ctx c;
  c.coop = nullptr; c.coop_payload = nullptr; c.coop_total = 0; c.coop_start = 0; c.coop_verify = 0; c.coop_window = 0; c.coop_helpers = 0;
  c.park = DgPark{};
  c.ticket = ticket;
  c.trace = nullptr; c.trace_cap = 0; c.itlog = nullptr; c.itlog_cap = 0;
  c.ws = (gptr)ws_all + (int64_t)blockIdx.x * dg_prob.ws_doubles;
  const int n = dg_prob.n, nq = dg_prob.nq, nc = dg_prob.nc, N = dg_prob.N;
  const int64_t nx = (int64_t)(N + 1) * nq;
  dev_load_tables();
  if (TID == 0) dg_lds[dg_prob.L.scal + DG_COOP_FLIP] = 0.0;
  while (true) {
    __syncthreads();
    if (TID == 0) dg_lds[dg_prob.L.scal + 63] = (double)atomicAdd(ticket, 1ULL);
    __syncthreads();
    const int64_t b = (int64_t)dg_lds[dg_prob.L.scal + 63];
    if (b >= B) break;
    int t = 0;
    while (t < cl.T) {
      const int64_t tb = (int64_t)t * B;        // records of step t start tb scenarios after those of step 0
      double* uws_t = cl.uws + (tb + b) * n;
      SolveOutPtrs O = cl.O;
      O.u += tb * n; if (O.l) O.l += tb * nc; O.x += (int64_t)t * cl.x_step; O.cond += tb * 3; O.cost += tb * dg_prob.M;
      O.status += tb; O.iters += tb; O.qp_solves += tb;
      c.x0 = (cgptr)(cl.q + (tb + b) * nq);
      if (dg_prob.par.variant == DGSQP_VARIANT_V2) dev_solve_v2(c, (cgptr)uws_t, b, O);
      else dev_solve(c, (cgptr)uws_t, b, O);
      // feedback.  The solve's records were stored by other lanes of this workgroup: fence + barrier before they are read back.
      __threadfence_block();
      __syncthreads();
      const int status = O.status[b];
      const bool keep = status == DGSQP_DIVERGED || status == DGSQP_QP_FAIL;
      const double* x1 = O.x + b * nx + nq;                 // stage 1 of the final iterate's rollout
      const double* u_t = O.u + b * n;
      const double* w_t = cl.w ? cl.w + (tb + b) * nq : nullptr;
      double* q_next = cl.q + (tb + B + b) * nq;
      double* uws_next = cl.uws + (tb + B + b) * n;
      int bad = 0;
      for (int i = TID; i < nq; i += NT) {
        double v = x1[i];
        if (w_t) v = v + w_t[i];
        q_next[i] = v;
        bad |= !isfinite(v);
      }
      t++;
      if (__syncthreads_or(bad)) break;                     // the chain ends: q[t] shows why, its warm start is never written
      for (int i = TID; i < n; i += NT) {
        const int k = (i % (N * DGSQP_NUA)) / DGSQP_NUA;    // agent-major: agent a holds rows k = 0 .. N-1 of DGSQP_NUA inputs
        uws_next[i] = keep ? uws_t[i] : u_t[k + 1 < N ? i + DGSQP_NUA : i];
      }
      // the next dev_solve of this workgroup reads q_next / uws_next through ordinary loads
      __threadfence_block();
      __syncthreads();
    }
    if (TID == 0) cl.steps_done[b] = t;
  }
}
