// C-ABI of the MI355X batched DG-SQP solver (include/dgsqp.h) and its kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o libdgsqp_hip.so dgsqp_api.hip
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <thread>
#include <vector>
#include <mutex>
#include <algorithm>

#include "dgsqp_solve.h"
#include "dgsqp_xl.h"
#include "dgsqp_osqp_xl.h"
#include "dgsqp_solve_v2.h"


// one staged batch of a grouped launch: its inputs and its outputs
// (up, up_stride: the batch's u_prev as dg_solve_kernel takes it)
struct DgBatch { const double* x0; const double* u_ws; SolveOutPtrs O; const double* up; int64_t up_stride; };
#define DG_GROUP_MAX 64

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// Persistent solve kernel: each workgroup pulls scenarios from a device-wide ticket counter, so that
// scenarios with long SQP runs (iteration counts vary 1..50+) do not serialise a static partition.
__global__ void __launch_bounds__(DG_BLOCK, 2)
dg_solve_kernel(const DgProb* __restrict__ D, int64_t B, const double* __restrict__ x0, const double* __restrict__ u_ws,
                SolveOutPtrs O, double* __restrict__ ws_all, unsigned long long* __restrict__ ticket,
                double* __restrict__ trace, int trace_cap, unsigned int* __restrict__ drained,
                double* __restrict__ itlog, int itlog_cap, const DgBatch* __restrict__ group, int group_n,
                DgCoop* coop, double* coop_payload, int coop_start, int coop_verify, int coop_window, int coop_helpers, DgPark park,
                const double* __restrict__ up, int64_t up_stride) {
  // up: scenario b's u_prev is the n_u doubles at up + b * up_stride -- [B][n_u] with stride n_u (dgsqp_set_u_prev), or the handle's n_u
  // zeros with stride 0
  Ctx c;
  c.coop = coop;
  c.park = park;
  if (!coop) c.park.entries = nullptr;
  c.ticket = ticket;
  c.coop_start = coop_start; c.coop_verify = coop_verify; c.coop_window = coop_window; c.coop_helpers = coop_helpers;
  c.coop_payload = coop ? coop_payload + (size_t)blockIdx.x * 2 * (2 * dg_prob.n + 2 * dg_prob.nc) : nullptr;
  c.coop_total = (unsigned long long)(B * (group ? group_n : 1));
  c.trace_cap = trace_cap;
  c.itlog_cap = itlog_cap;
  c.ws = (gptr)ws_all + (int64_t)blockIdx.x * dg_prob.ws_doubles;
#ifdef DG_PROF
  const long long wg_t0 = clock64();
  const unsigned long long wall0 = wall_clock64();
#endif
  dev_load_tables();
  if (TID == 0) dg_lds[dg_prob.L.scal + DG_COOP_FLIP] = 0.0;
  if (coop && TID == 0) { unsigned long long zero = 0ull; __hip_atomic_compare_exchange_strong(&coop->t_first, &zero, wall_clock64(), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  while (true) {
    __syncthreads();
    if (TID == 0) dg_lds[dg_prob.L.scal + 63] = (double)atomicAdd(ticket, 1ULL);
    __syncthreads();
    int64_t b = (int64_t)dg_lds[dg_prob.L.scal + 63];
    const DgParkEntry* resume = nullptr;
    if (b >= B * (group ? group_n : 1)) {
      // the queue is empty: from now on this launch only drains.  Tell the host (mapped, fine-grained memory) so that it
      // can start the next independent batch on the compute units that become free.
      if (drained && TID == 0) { __hip_atomic_store(drained, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
      if (!coop) break;
      // cooperative launches: resume a deferred scenario, the one that has cost the most so far first; with none waiting, stay and
      // evaluate line-search trials for the workgroups that are still solving (until a deferred scenario turns up or the launch ends)
      const long long slot = dev_park_pop(c);
      if (slot < 0) {
        if (dev_coop_help(c)) continue;
        break;
      }
      dev_park_load(c, (unsigned int)slot);
      resume = &c.park.entries[slot];
      b = (int64_t)resume->ticket;
      if (TID == 0) c.park.entries[slot].t_resume = wall_clock64() - AT_LOAD(&coop->t_first);
    }
    const int64_t tk = b;
    if (group) {        // grouped launch (dgsqp_launch_staged_group): ticket -> (staged batch, scenario); every batch has its own buffers
      const int64_t gi = b / B;
      b -= gi * B;
      x0 = group[gi].x0; u_ws = group[gi].u_ws; O = group[gi].O; up = group[gi].up; up_stride = group[gi].up_stride;
    }
    c.x0 = (cgptr)x0 + b * dg_prob.nq;
    c.up = (cgptr)up + b * up_stride;
    c.trace = trace ? (gptr)trace + b * (int64_t)(1 + 2 * trace_cap) : nullptr;
    if (c.trace && TID == 0 && !resume) c.trace[0] = 0.0;
    c.itlog = itlog ? (gptr)itlog + b * (1 + (int64_t)itlog_cap * (dg_prob.n + dg_prob.nc)) : nullptr;
#ifdef DG_PROF
    const long long sc_t0 = clock64();
#endif
    bool deferred = false;
    int its = 0;
    const unsigned long long ticks0 = c.park.entries ? dev_bcast_u64(TID == 0 ? wall_clock64() : 0ull) : 0ull;
    if (dg_prob.par.variant == DGSQP_VARIANT_V2) deferred = dev_solve_v2(c, (cgptr)u_ws + b * dg_prob.n, b, O, resume, (long long)tk, ticks0, &its);
    else deferred = dev_solve(c, (cgptr)u_ws + b * dg_prob.n, b, O, resume, (long long)tk, ticks0, &its);
    if (resume && TID == 0) {
      DgParkEntry* e = &c.park.entries[resume - c.park.entries];
      e->t_done = wall_clock64() - AT_LOAD(&coop->t_first); e->final_its = its; e->final_qps = O.qp_solves ? O.qp_solves[b] : 0;
    }
    if (coop && !deferred && TID == 0) {
      __threadfence();
      if (!resume && c.park.entries) {
        __hip_atomic_fetch_add(&coop->done_ticks, wall_clock64() - ticks0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&coop->done_fresh, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __hip_atomic_fetch_add(&coop->done_iters, (unsigned long long)its, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&coop->finished, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
#ifdef DG_PROF
    if (TID == 0 && tk < 16384) dg_prof_scn[tk] = (resume ? dg_prof_scn[tk] : 0ull) + (unsigned long long)(clock64() - sc_t0);
#endif
  }
#ifdef DG_PROF
  if (TID == 0) {
    atomicAdd(&dg_prof[2 * PH_WGTOTAL], (unsigned long long)(clock64() - wg_t0));
    atomicAdd(&dg_prof[2 * PH_WGTOTAL + 1], 1ULL);
    atomicMax(&dg_prof[2 * PH_WGMAX], (unsigned long long)(clock64() - wg_t0));
    atomicMax(&dg_prof[2 * PH_WGMAX + 1], (unsigned long long)(wall_clock64() - wall0));
  }
#endif
}

#include "dgsqp_closed_loop.h"
#include "dgsqp_pid.h"
#include "dgsqp_sampler.h"
#include "dgsqp_track_width.h"
#include "dgsqp_mpc.h"
#include "dgsqp_raceline.h"
#include "dgsqp_track_frame.h"

// Test hook: one _evaluate(hessian=True) (+ dual init) per scenario, results expanded to dense arrays.
__global__ void __launch_bounds__(DG_BLOCK, 2)
dg_evaluate_kernel(const DgProb* __restrict__ D, int64_t B, const double* __restrict__ x0, const double* __restrict__ u,
                   const double* __restrict__ l, double* q, double* g, double* G, double* Q, double* x, double* l0,
                   double* __restrict__ ws_all, const double* __restrict__ up, int64_t up_stride) {
  Ctx c;
  c.coop = nullptr; c.coop_payload = nullptr; c.coop_total = 0; c.coop_start = 0; c.coop_verify = 0; c.coop_window = 0; c.coop_helpers = 0;
  c.ws = (gptr)ws_all + (int64_t)blockIdx.x * dg_prob.ws_doubles;
  c.trace = nullptr; c.trace_cap = 0; c.itlog = nullptr; c.itlog_cap = 0;
  const DgLds& L = dg_prob.L;
  const int n = dg_prob.n, nc = dg_prob.nc;
  dev_load_tables();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    c.x0 = (cgptr)x0 + b * dg_prob.nq;
    c.up = (cgptr)up + b * up_stride;
    __syncthreads();
    if (TID == 0) { dg_lds[L.scal + DG_XVALID] = 0.0; dg_lds[L.scal + DG_REG] = dg_prob.par.reg; dg_lds[L.scal + DG_OSQP_RHO] = 0.1; }
    for (int i = TID; i < n; i += NT) dg_lds[L.u + i] = u[b * n + i];
    for (int r = TID; r < nc; r += NT) dg_lds[L.l + r] = l ? l[b * nc + r] : 0.0;
    __syncthreads();
    dev_evaluate(c, LP(L.u), 0.0, nullptr, true);
    if (q) for (int i = TID; i < n; i += NT) q[b * n + i] = dg_lds[L.q + i];
    if (g) for (int r = TID; r < nc; r += NT) g[b * nc + r] = dg_lds[L.g + r];
    if (x) for (int i = TID; i < (dg_prob.N + 1) * dg_prob.nq; i += NT) x[b * (int64_t)(dg_prob.N + 1) * dg_prob.nq + i] = dg_lds[L.e_x + i];
    if (G)
      for (int64_t t = TID; t < (int64_t)nc * n; t += NT)
        G[b * (int64_t)nc * n + t] = dg_prob.gd_global ? g_row_coef<cgptr>(dg_prob, dev_gd_global(c), (int)(t / n), (int)(t % n))
                                                          : g_row_coef<clptr>(dg_prob, LP(L.gd), (int)(t / n), (int)(t % n));
    if (Q) {
      cgptr Qg = c.ws + dg_prob.ws_q;
      for (int t = TID; t < n * n; t += NT) Q[b * (int64_t)n * n + t] = Qg[t];
    }
    if (l0) {
      dev_dual_init(c);
      for (int r = TID; r < nc; r += NT) l0[b * nc + r] = dg_lds[L.l + r];
    }
    __syncthreads();
  }
}

// Test hook: _solve_qp at the linearisation point (u, l).
__global__ void __launch_bounds__(DG_BLOCK, 2)
dg_qp_kernel(const DgProb* __restrict__ D, int64_t B, const double* __restrict__ x0, const double* __restrict__ u,
             const double* __restrict__ l, double* du, double* lhat, double* Qpd, int32_t* flag, double* info8, double* __restrict__ ws_all,
             const double* __restrict__ up, int64_t up_stride) {
  Ctx c;
  c.coop = nullptr; c.coop_payload = nullptr; c.coop_total = 0; c.coop_start = 0; c.coop_verify = 0; c.coop_window = 0; c.coop_helpers = 0;
  c.ws = (gptr)ws_all + (int64_t)blockIdx.x * dg_prob.ws_doubles;
  c.trace = nullptr; c.trace_cap = 0; c.itlog = nullptr; c.itlog_cap = 0;
  const DgLds& L = dg_prob.L;
  const int n = dg_prob.n, nc = dg_prob.nc;
  dev_load_tables();
  // The saved active set is deliberately NOT cleared between the scenarios one workgroup handles: with more scenarios
  // than workgroups every QP after the first is warm-started from an unrelated problem's active set (tests use this).
  if (TID == 0) { dg_lds[L.scal + DG_QP_NPREV] = 0.0; dg_lds[L.scal + DG_PSD_PD] = 0.0; }
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    c.x0 = (cgptr)x0 + b * dg_prob.nq;
    c.up = (cgptr)up + b * up_stride;
    __syncthreads();
    if (TID == 0) { dg_lds[L.scal + DG_XVALID] = 0.0; dg_lds[L.scal + DG_REG] = dg_prob.par.reg; dg_lds[L.scal + DG_OSQP_RHO] = 0.1; }
    for (int i = TID; i < n; i += NT) dg_lds[L.u + i] = u[b * n + i];
    for (int r = TID; r < nc; r += NT) dg_lds[L.l + r] = l[b * nc + r];
    __syncthreads();
    const int f = dev_linearize_and_qp(c, true, nullptr, Qpd ? (gptr)Qpd + b * (int64_t)n * n : nullptr);
    if (du) for (int i = TID; i < n; i += NT) du[b * n + i] = dg_lds[L.o_du + i];
    if (lhat) for (int r = TID; r < nc; r += NT) lhat[b * nc + r] = dg_lds[L.o_lhat + r];
    if (flag && TID == 0) flag[b] = f;
    if (info8 && TID < 8) info8[b * 8 + TID] = dg_prob.osqp ? dg_lds[L.scal + DG_OSQP_INFO + TID] : 0.0;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// The per-scenario arrays of a solve, stated once: every host function that allocates, fills, hands out or copies them walks this
// table.  The eight records from DG_U on are in the order of the C-ABI's result parameters (include/dgsqp.h).
enum DgRec { DG_Q, DG_UWS, DG_W, DG_U, DG_L, DG_X, DG_STATUS, DG_ITERS, DG_QPS, DG_COND, DG_COST, DG_DONE, DG_REC_COUNT };
// `fill` is the byte a closed-loop launch leaves where a step never ran: every byte 0xff is NaN in a double and DGSQP_NOT_RUN (-1) in a
// status; counts are zero.  The kernel writes each slice it reaches once, on top of this.
struct DgRecDesc { size_t elem, per; int fill; };      // bytes of an element, elements per scenario, fill byte
struct DgRecTable {
  DgRecDesc d[DG_REC_COUNT];
  const DgRecDesc& operator[](int r) const { return d[r]; }
  size_t bytes(int r) const { return d[r].elem * d[r].per; }      // of one scenario
};
// built once per handle, in dgsqp_create
static DgRecTable rec_table(const DgProb& D) {
  const size_t dbl = sizeof(double), i32 = sizeof(int32_t);
  return DgRecTable{{
      /* DG_Q      initial state (closed loop: the chain of states)   */ {dbl, (size_t)D.nq, 0xff},
      /* DG_UWS    warm start, agent-major (closed loop: per step)    */ {dbl, (size_t)D.n, 0xff},
      /* DG_W      closed loop only: disturbance of the plant         */ {dbl, (size_t)D.nq, 0xff},
      /* DG_U      */ {dbl, (size_t)D.n, 0xff},
      /* DG_L      */ {dbl, (size_t)D.nc, 0xff},
      /* DG_X      */ {dbl, (size_t)(D.N + 1) * D.nq, 0xff},
      /* DG_STATUS */ {i32, 1, 0xff},
      /* DG_ITERS  */ {i32, 1, 0},
      /* DG_QPS    */ {i32, 1, 0},
      /* DG_COND   p_feas, comp, stat                                 */ {dbl, 3, 0xff},
      /* DG_COST   */ {dbl, (size_t)D.M, 0xff},
      /* DG_DONE   closed loop only: steps a chain ran                */ {i32, 1, 0}}};
}
// scenarios of each record that one use of a buffer set holds (0: that record is not part of it)
struct DgRecCount { int64_t n[DG_REC_COUNT]; };
// a staged batch: B of everything a plain solve reads and writes
static DgRecCount rec_count_batch(int64_t B) {
  DgRecCount c;
  for (int r = 0; r < DG_REC_COUNT; r++) c.n[r] = (r == DG_W || r == DG_DONE) ? 0 : B;
  return c;
}
// Device buffers over the table.  Every buffer grows exactly to what is asked of it and never shrinks.
struct DgRecords {
  void* p[DG_REC_COUNT] = {};
  size_t bytes[DG_REC_COUNT] = {};
  double* dbl(int r) const { return (double*)p[r]; }
  // a record that is not part of this use is a null pointer to the kernels, whatever an earlier use left allocated
  SolveOutPtrs out(const DgRecCount& c) const {
    auto at = [&](int r) { return c.n[r] ? p[r] : nullptr; };
    return SolveOutPtrs{(double*)at(DG_U), (double*)at(DG_L), (double*)at(DG_X), (double*)at(DG_COND), (double*)at(DG_COST),
                        (int32_t*)at(DG_STATUS), (int32_t*)at(DG_ITERS), (int32_t*)at(DG_QPS)};
  }
};
// the eight result parameters of the C-ABI, in its order, as a table of host pointers (null: not wanted)
static void rec_host_table(void* dst[DG_REC_COUNT], void* u, void* l, void* x, void* status, void* iters, void* qp_solves, void* cond, void* cost) {
  for (int r = 0; r < DG_REC_COUNT; r++) dst[r] = nullptr;
  dst[DG_U] = u; dst[DG_L] = l; dst[DG_X] = x; dst[DG_STATUS] = status; dst[DG_ITERS] = iters; dst[DG_QPS] = qp_solves; dst[DG_COND] = cond; dst[DG_COST] = cost;
}

// Event trace and iterate log of a single launch: one scenario's slice is a count followed by `cap` entries.
struct DgLog {
  bool iterates;              // entries are iterates (u, l) -- n + n_c doubles -- and not (code, value) pairs
  double* buf = nullptr;
  int cap = 0;                // entries per scenario (0: off)
  int64_t held = 0;           // scenarios the buffer holds
  int64_t launch_B = 0;       // scenarios of the launch that filled it
  int64_t doubles(const DgProb& D) const { return 1 + (int64_t)cap * (iterates ? D.n + D.nc : 2); }
};

// The settings of closed-loop launches (dgsqp_set_plant and, on top of a plant, dgsqp_set_plant_ensemble, dgsqp_set_estimate_noise,
// dgsqp_set_monitor, dgsqp_set_drivers, dgsqp_set_plan_hold).  Every device buffer they need is one entry of DgSide, stated once here: what a setter uploads,
// what a launch sizes per workgroup, and the records a launch leaves behind for a dgsqp_fetch_*.  Every buffer grows exactly to what is
// asked of it and never shrinks.
enum DgSideBuf {
  SB_PLANT, SB_LINES, SB_U_PLANT,                             // the plant: one dgsqp_plant_t; delay lines per workgroup; u_plant [T][B][S][nu]
  SB_VEHICLES, SB_DELAY, SB_WG_PLANT,                         // the ensemble: [B][M] dgsqp_vehicle_t, [B][M][DGSQP_NUA] int32; one dgsqp_plant_t per workgroup
  SB_V, SB_Q_EST,                                             // estimate noise: v and q_est [T][B][nq]
  SB_MON_SCRATCH, SB_CLEARANCE, SB_BOX_EXCESS, SB_HIT_STEP,   // the monitor: [grid][S][M][3]; clearance and box_excess [T][B], hit_step [B] int32
  SB_KIND, SB_PID, SB_REF, SB_U_REPLAY,                       // the drivers: [B][M] int32, [DGSQP_MAX_AGENTS] dgsqp_pid_t, [B][M][2], [T][B][nu]
  SB_U_CMD, SB_PID_STATE,                                     // ... u_cmd [T][B][nu]; per workgroup: [grid][M][3]
  SB_U_GAME, SB_PLAN_STAGE, SB_HOLD_STATE,                    // the held plan: u_game [T][B][nu], plan_stage [T][B] int32; per workgroup: [grid][2] int32
  SB_U_PREV,                                                  // the carried input (dgsqp_set_closed_loop_u_prev): u_prev [T][B][nu]
  SB_X_GAME, SB_X_LIFT, SB_Z, SB_TRACK_REF,                   // the cross plant: the game as a dgsqp_plant_t; the game with bounds in the plant's layout; z [T+1][B][nz], track_ref [T][B][M][3]
  DG_SIDE_COUNT
};
struct DgBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
struct DgSide {
  DgBuf b[DG_SIDE_COUNT];
  int64_t left[DG_SIDE_COUNT] = {};   // a record: elements the last launch that filled it left behind (0: none yet)
  template <class T> T* at(int i) const { return (T*)b[i].p; }
};
// what is set, and for which launch shape: the plant; the further settings on top of it; the drivers; the held plan
struct DgPlantState {
  bool set = false;
  dgsqp_plant_t host;                 // resolved: agents[] hold the game's records when the plant uses the game's parameters
};
struct DgEnsembleState {
  int64_t B = 0;                      // chains of the plant ensemble (0: off)
  bool has_delay = false;
  int32_t est_T = 0;                  // estimate noise: its shape (0: off)
  int64_t est_B = 0;
  int monitor = 0;                    // 0 off, 1 record, 2 record and stop
  bool any() const { return B > 0 || est_T > 0 || monitor != 0; }
};
struct DgDriversState {
  bool set = false;
  int32_t T = 0;                      // the launch shape the arrays were given for
  int64_t B = 0;
  bool has_ref = false, has_replay = false;
  std::vector<int32_t> kinds;         // [B][M] as uploaded (a cross-plant launch checks them against its pairs)
};
struct DgHoldState {
  bool set = false;
  dgsqp_hold_t host;
};
// a plant of another model class (dgsqp_set_cross_plant): plant.set holds as well while it is set, plant.host is its resolved record
struct DgCrossState {
  bool set = false;
  int64_t B = 0;                      // chains z0 was given for
  int mdl[DGSQP_MAX_AGENTS] = {}, nz[DGSQP_MAX_AGENTS] = {}, zoff[DGSQP_MAX_AGENTS] = {}, nz_all = 0;
  int8_t proj[DGSQP_MAX_AGENTS][DGSQP_MAX_NQA] = {};
  std::vector<double> z0;             // [B][nz_all]
};

// u_{-1}, the input applied before stage 0 (Ctx.up).  dgsqp_set_u_prev keeps a host copy; staging a batch captures it in a device buffer of
// the handle's own, so a later set does not reach a batch that is already staged.  A kernel is handed (pointer, stride between scenarios):
// the captured [B][n_u] with stride n_u, or `zero` -- n_u zeros, allocated with the handle -- with stride 0.
struct DgUPrevState {
  std::vector<double> host;           // [B][n_u] as set (sticky)
  int64_t B = 0;                      // 0: off
  DgBuf staged;                       // what the staged batch captured ...
  int64_t staged_stride = 0;          // ... n_u, or 0: the staged batch runs from `zero`
  double* zero = nullptr;
  const double* ptr() const { return staged_stride ? (const double*)staged.p : zero; }
  int cl_mode = 0;                    // closed loop (dgsqp_set_closed_loop_u_prev): 0 off, 1 carry
  int64_t cl_B = 0;                   // chains u_prev0 was given for (0: none, every chain starts from zeros)
  std::vector<double> cl_host;        // u_prev0 [cl_B][n_u]
};

// The tracker of dgsqp_set_mpc: the resolved device record (pointers are filled per launch), its row table and the log of the last launch.
struct DgMpcState {
  bool set = false;
  dg_mpc::DgMpcDev dev;
  std::vector<dgsqp_mpc_row_t> rows;
  bool log_on = false;
  double *logD = nullptr, *logDb = nullptr, *loglam = nullptr;    // device, of the last logged launch
  int64_t log_B = 0;
  int log_iters = 0, log_lenD = 0, log_rows = 0;
};

// The raceline of dgsqp_set_raceline (device copy of the table) and the reference trajectories of the last warm-start program.
struct DgRacelineState {
  DgRaceline dev{0, nullptr, nullptr};
  double* T = nullptr;                 // device [n]
  double* cols = nullptr;              // device [n][DGSQP_RL_COLS]
  double* qref = nullptr;              // device [M][B][N+1][n_qa] of the last program (dgsqp_fetch_raceline_ref)
  size_t qref_cap = 0;                 // doubles allocated
  int64_t ref_B = 0;
};

struct dgsqp_comm_state;
struct dgsqp_solver {
  int device = 0;
  DgProb hp;
  DgProb* dp = nullptr;
  hipStream_t stream = nullptr;          // the handle's own: staging, result copies, the synchronous hooks and closed-loop launches
  hipStream_t launch_stream = nullptr;   // what the handle's launch in flight (or its last one) runs on: a pool stream (launch_solve) or `stream`
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int num_cu = 0, wg_per_cu = 1, max_grid = 0, launched_grid = 0;
  size_t lds_bytes = 0;
  double* ws = nullptr;
  size_t ws_groups = 0;
  unsigned long long* ticket = nullptr;
  unsigned int* drained_host = nullptr;   // mapped host memory: 1 once the last launch has handed out its last scenario
  unsigned int* drained_dev = nullptr;
  DgRecTable rec;                         // the record table of this handle's game
  int64_t B = 0;                          // staged batch: its size ...
  DgRecords staged;                       // ... and its arrays
  DgRecords closed;                       // closed-loop launches (dgsqp_closed_loop_batch): step-major arrays
  DgLog trace{false}, itlog{true};
  DgPlantState plant;                      // closed-loop settings ...
  DgEnsembleState ens;
  DgDriversState drv;
  DgHoldState hold;
  DgCrossState cross;
  DgSide side;                             // ... and their device buffers
  DgUPrevState up;                         // the input before stage 0: plain solves and hooks, and closed-loop carry
  DgMpcState mpc;                          // the reference tracker (dgsqp_set_mpc)
  DgRacelineState rl;                      // the raceline (dgsqp_set_raceline)
  int rl_clip_widths = 0;                  // e_y clip of the spline-track raceline sampler (dgsqp_set_raceline_clip)
  double rl_clip_scale = 0.0;
  bool in_flight = false;       // a solve launch has been enqueued and not yet waited for
  dgsqp_solver* group_leader = nullptr;   // set while this handle's batch is being solved by another handle's grouped launch
  DgBatch* d_group = nullptr;             // leader: device table of the group's batches (DG_GROUP_MAX entries)
  DgBatch* group_host = nullptr;          // ... and its pinned host image (the source of an asynchronous copy)
  unsigned long long launch_gen = 0;      // leader: counts its launches; members remember the generation they belong to
  unsigned long long group_gen = 0;       // member: launch_gen of the leader's launch that solves this handle's batch
  float last_ms = 0.0f;                   // kernel time of the last completed launch that solved this handle's batch (HIP events)
  DgCoop* d_coop = nullptr;           // cooperative line search: job slots (2 per workgroup) ...
  double* d_coop_payload = nullptr;   // ... and the base points their owners publish
  size_t coop_bytes = 0;
  int coop_mode = 1;                  // 0 off, 1 synchronous calls only (nothing else is waiting for the compute units), 2 every launch
  bool coop_next_sync = false;        // (set by the synchronous entry points around their launch)
  size_t park_last_cap = 0;           // deferral of long scenarios: slots the handle's last launch could use (0: it did not defer)
  int defer_min_it = 8;               // 0: off
  double defer_factor = 2.0;
  bool defer_requested = false;       // dgsqp_set_deferral was called (DG-SQP v2 is only deferred on request)
  dgsqp_comm_state* comm = nullptr;   // RCCL communicator + record buffers (dgsqp_comm.h), owned by the handle
  std::string err;
};
static thread_local std::string g_create_err;

#define HIPCHK(h, call)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
      return DGSQP_E_DEVICE;                                                                 \
    }                                                                                        \
  } while (0)

#include "dgsqp_comm.h"

static void mpc_log_free(dgsqp_solver* h);

static void rec_free(DgRecords& S) {
  for (int r = 0; r < DG_REC_COUNT; r++) { if (S.p[r]) (void)hipFree(S.p[r]); S.p[r] = nullptr; S.bytes[r] = 0; }
}
static int rec_reserve(dgsqp_solver* h, DgRecords& S, const DgRecCount& c) {
  for (int r = 0; r < DG_REC_COUNT; r++) {
    const size_t want = (size_t)c.n[r] * h->rec.bytes(r);
    if (want <= S.bytes[r]) continue;
    if (S.p[r]) (void)hipFree(S.p[r]);
    S.p[r] = nullptr; S.bytes[r] = 0;
    HIPCHK(h, hipMalloc(&S.p[r], want));
    S.bytes[r] = want;
  }
  return DGSQP_OK;
}
// each record's fill byte over its scenarios from keep.n[r] on, in table order on h's stream
static int rec_fill(dgsqp_solver* h, const DgRecords& S, const DgRecCount& c, const DgRecCount& keep) {
  for (int r = 0; r < DG_REC_COUNT; r++) {
    const size_t one = h->rec.bytes(r);
    if (c.n[r] > keep.n[r]) HIPCHK(h, hipMemsetAsync((char*)S.p[r] + (size_t)keep.n[r] * one, h->rec[r].fill, (size_t)(c.n[r] - keep.n[r]) * one, h->stream));
  }
  return DGSQP_OK;
}
// c.n[r] scenarios of every record with a pointer in `host`, to the device or back, in table order on h's stream (no synchronise)
static int rec_copy(dgsqp_solver* h, const DgRecords& S, const DgRecCount& c, void* const host[DG_REC_COUNT], hipMemcpyKind kind) {
  for (int r = 0; r < DG_REC_COUNT; r++) {
    if (!host[r] || c.n[r] == 0) continue;
    const size_t bytes = (size_t)c.n[r] * h->rec.bytes(r);
    if (kind == hipMemcpyHostToDevice) HIPCHK(h, hipMemcpyAsync(S.p[r], host[r], bytes, kind, h->stream));
    else HIPCHK(h, hipMemcpyAsync(host[r], S.p[r], bytes, kind, h->stream));
  }
  return DGSQP_OK;
}
static int ensure_ws(dgsqp_solver* h, size_t groups) {
  if (groups <= h->ws_groups) return DGSQP_OK;
  if (h->ws) (void)hipFree(h->ws);
  h->ws = nullptr; h->ws_groups = 0;
  HIPCHK(h, hipMalloc(&h->ws, sizeof(double) * groups * (size_t)h->hp.ws_doubles));
  h->ws_groups = groups;
  return DGSQP_OK;
}
// The kernels read the game from the __constant__ symbol dg_prob, one per device and process.  Handles of DIFFERENT games
// (or parameters) may coexist: the registry below remembers which description the symbol of each device holds and which
// handles have a launch in flight.  A launch whose description differs from the resident one first waits for every launch
// in flight on that device (they would otherwise read the new constants), then uploads its own; launches of the same
// description skip the upload and overlap freely (bench.py --pipeline).
namespace {
std::mutex g_reg_mutex;
struct DgResident { bool valid = false; std::vector<unsigned char> bytes; };
DgResident g_resident[64];
std::vector<dgsqp_solver*> g_handles;
// Deferral of long scenarios: ONE pool of slots per device, taken by the cooperative launch that defers (such launches run when
// nothing else waits for the compute units; a second one that finds the pool busy simply does not defer).  Allocated at the first
// deferring launch on the device -- 4,096 slots or what 16 GB hold -- and kept: no launch pays for an allocation of its own.
struct DgParkPool {
  DgParkEntry* entries = nullptr;
  double* store = nullptr;
  size_t slots = 0, slot_doubles = 0;
  dgsqp_solver* owner = nullptr;            // handle whose launch uses the pool ...
  unsigned long long owner_gen = 0;         // ... and which of its launches
};
DgParkPool g_park[64];
// Launch streams: dg_solve_kernel launches do not run on their handles' streams but on a small pool of streams per device, taken
// round robin in launch order.  The runtime spreads streams over GPU_MAX_HW_QUEUES hardware queues (4 unless set) in creation order,
// and a kernel waits for everything before it in its hardware queue: with one stream per handle, which launches shared a queue --
// and then ran one after the other, tail included -- depended on which handles led them.  The pool is created before the first
// handle's stream of the device, so its K = min(queues, 8) streams sit on different queues; launch j shares a stream with launch
// j - K alone.  It lives while the device has a handle.
struct DgLaunchStreams {
  std::vector<hipStream_t> streams;
  unsigned long long next = 0;      // launches handed a stream so far
};
DgLaunchStreams g_launch_streams[64];
}  // namespace
static int launch_stream_count() {
  const char* e = getenv("GPU_MAX_HW_QUEUES");
  char* end = nullptr;
  const long q = e ? strtol(e, &end, 10) : 0;
  return (int)std::min<long>(e && end != e && *end == '\0' && q >= 1 ? q : 4, 8);
}
// Call with g_reg_mutex held and the device current.  The pool of h's device, created on demand.
static int ensure_launch_streams(dgsqp_solver* h) {
  DgLaunchStreams& pool = g_launch_streams[h->device & 63];
  for (int k = (int)pool.streams.size(), K = launch_stream_count(); k < K; k++) {
    hipStream_t s = nullptr;
    HIPCHK(h, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    pool.streams.push_back(s);
  }
  return DGSQP_OK;
}
// the stream the handle's solve in flight runs on: its own launch's, or the leader's for a member of a grouped launch
static hipStream_t active_stream(const dgsqp_solver* h) { return (h->group_leader ? h->group_leader : h)->launch_stream; }
// kernel time of h's completed launch (events ev[0], ev[1] of the stream it ran on)
static void record_last_ms(dgsqp_solver* h, dgsqp_solver* leader) {
  float ms = 0.0f;
  if (h->launched_grid > 0 && hipEventElapsedTime(&ms, leader->ev[0], leader->ev[1]) == hipSuccess) h->last_ms = ms;
}
// The members of a grouped launch led by L whose kernel has completed (L's launch stream is synchronised): they leave the group
// with the kernel time of THAT launch.  Called before L's events are re-recorded by its next launch, so that a member's
// later dgsqp_wait / dgsqp_finished never looks at the events of an unrelated kernel.
static void release_members(dgsqp_solver* L) {
  for (dgsqp_solver* o : g_handles)
    if (o->group_leader == L && o->group_gen == L->launch_gen) { record_last_ms(o, L); o->in_flight = false; o->group_leader = nullptr; }
}
static int wait_idle(dgsqp_solver* h) {
  if (h->in_flight) {
    dgsqp_solver* L = h->group_leader ? h->group_leader : h;
    HIPCHK(h, hipStreamSynchronize(L->launch_stream));
    record_last_ms(h, L);
    h->in_flight = false;
    h->group_leader = nullptr;
  }
  return DGSQP_OK;
}
// Call with g_reg_mutex held and keep it until the kernel that needs the constants has been enqueued and the handle is
// marked in flight: from then on a launch of a different game waits for that kernel before it overwrites the symbol.
static int upload_problem(dgsqp_solver* h) {
  DgResident& r = g_resident[h->device & 63];
  if (r.valid && r.bytes.size() == sizeof(DgProb) && memcmp(r.bytes.data(), &h->hp, sizeof(DgProb)) == 0) return DGSQP_OK;
  for (dgsqp_solver* o : g_handles)
    if (o->device == h->device && o->in_flight) {
      if (hipStreamSynchronize(active_stream(o)) != hipSuccess) { h->err = "hipStreamSynchronize of a launch in flight failed"; return DGSQP_E_DEVICE; }
      // (o stays marked in flight: its owner still has to collect it with dgsqp_wait)
    }
  HIPCHK(h, hipMemcpyToSymbolAsync(HIP_SYMBOL(dg_prob), &h->hp, sizeof(DgProb), 0, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  r.bytes.assign((const unsigned char*)&h->hp, (const unsigned char*)&h->hp + sizeof(DgProb));
  r.valid = true;
  return DGSQP_OK;
}
// Cooperative line search for the launch about to be enqueued?  Helpers keep their compute units until the launch's last
// scenario is done: right when nothing else waits for them (synchronous calls), wrong in a pipeline of launches -- the caller
// says so (dgsqp_set_cooperative).  Needs the whole grid resident (it is: at most one workgroup per compute unit).
// (development knobs: DGSQP_COOP_START = rejected trials after which a line search is offered to helpers, default 2;
//  DGSQP_COOP_VERIFY = 1: owners re-evaluate every helper value and count differing bits -- dgsqp_coop_stats)
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static double env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
static int coop_start_trials() { return std::max(1, env_int("DGSQP_COOP_START", 2)); }
static int coop_window_trials() { return std::max(1, env_int("DGSQP_COOP_WINDOW", 64)); }
static int coop_max_helpers() { return std::max(1, env_int("DGSQP_COOP_HELPERS", 64)); }
static int coop_verify_mode() { return env_int("DGSQP_COOP_VERIFY", 0) != 0; }
static bool coop_for_launch(dgsqp_solver* h, int grid) {
  if (!h->d_coop || grid > h->num_cu * 2 + 2 || h->trace.cap > 0) return false;
  // (development knob DGSQP_COOP_MIN_CHAIN: only for games whose rollout is a dependent chain of at least that many evaluations of f_c,
  // N x substeps x stages.  With all idle workgroups helping, the euler games lost -- 409 -> 450 ms --; with the helpers capped at 64
  // they gain as well -- 362 -> 345 ms --, so the default is 0.)
  const dgsqp_problem_t& P = h->hp.P;
  const int stages = P.integrator == DGSQP_INT_RK4 ? 4 : (P.integrator == DGSQP_INT_RK3 ? 3 : (P.integrator == DGSQP_INT_RK2 ? 2 : 1));
  const int chain = P.N * (P.integrator == DGSQP_INT_EULER ? 1 : P.substeps * stages);
  if (chain < env_int("DGSQP_COOP_MIN_CHAIN", 0)) return false;
  return h->coop_mode == 2 || (h->coop_mode == 1 && h->coop_next_sync);
}
// Deferral of long scenarios for the cooperative launch about to be enqueued on `stream` (DgPark, dgsqp_device.h): a quarter of
// the launch's scenarios may be deferred at a time (bounded by 16 GB of slots).  Off for launches that give every scenario its own
// workgroup and while logs are recorded; DG-SQP v2 only after an explicit dgsqp_set_deferral (round 4).  (development knobs: DGSQP_DEFER = 0 switches it off, DGSQP_DEFER_MIN_IT,
// DGSQP_DEFER_FACTOR override dgsqp_set_deferral.)
static int park_for_launch(dgsqp_solver* h, hipStream_t stream, bool coop, int grid, int64_t total, DgPark* out) {
  memset(out, 0, sizeof(*out));
  h->park_last_cap = 0;
  int min_it = h->defer_min_it;
  double factor = h->defer_factor;
  // qp_method OSQP on the LDS path: what a scenario costs is set by its ADMM iterations, not by its SQP iterations -- "twice the mean
  // iteration count" sets aside scenarios that are not long, and their state copies and late resumes cost more than the tail they
  // save (20 batches of configs[1] in one launch, profiles/r06_osqp_deferral_sweep.txt: 4,410 scen/s at factor 2, 4,914 without deferral,
  // 5,337 at factor 4, 5,108 at 6; the exact QP has its optimum at 2: 11,739 against 11,105 at 3 and 10,129 without)
  if (h->hp.osqp && h->hp.big != 2 && !h->defer_requested) factor = 4.0;
  const int time_mode = env_int("DGSQP_DEFER_TIME", 0) != 0;
  if (env_int("DGSQP_DEFER", 1) == 0) min_it = 0;
  min_it = env_int("DGSQP_DEFER_MIN_IT", min_it);
  factor = env_double("DGSQP_DEFER_FACTOR", factor);
  if (!coop || min_it <= 0 || total <= (int64_t)grid || h->trace.cap > 0 || h->itlog.cap > 0) return DGSQP_OK;
  // DG-SQP v2: only when the caller asked for it (dgsqp_set_deferral).  Nearly every v2 scenario runs ~375 iterations and a few run
  // thousands: setting those aside delays exactly the solves that decide the launch's length (48 batches of 512 as 8 x 3 launches:
  // 409 scen/s without, 367 with; as one launch 404 / 411).
  if (h->hp.par.variant == DGSQP_VARIANT_V2 && !h->defer_requested) return DGSQP_OK;
  const size_t slot = (size_t)h->hp.L.total + (size_t)h->hp.ws_doubles;
  const double frac = env_double("DGSQP_DEFER_CAP_FRAC", 0.25);
  size_t cap = (size_t)((double)total * (frac > 0.0 && frac <= 1.0 ? frac : 0.25) + 1.0);
  DgParkPool& pool = g_park[h->device & 63];      // (g_reg_mutex is held by the launch functions)
  if (pool.owner && pool.owner != h && pool.owner->in_flight && pool.owner->launch_gen == pool.owner_gen) return DGSQP_OK;   // busy: no deferral
  // The pool holds what this launch may defer (a quarter of its scenarios) and grows geometrically when a larger launch comes along; its
  // size is bounded by DGSQP_DEFER_POOL_BYTES (default 16 GiB; 0 switches deferral off).  It is only ever re-allocated while no launch uses it.
  size_t limit_bytes = (size_t)16 << 30;
  { const char* e = getenv("DGSQP_DEFER_POOL_BYTES"); if (e) limit_bytes = (size_t)strtoull(e, nullptr, 10); }
  const size_t max_slots = limit_bytes / (slot * sizeof(double));
  if (cap > max_slots) cap = max_slots;
  if (cap < 1) return DGSQP_OK;
  if (pool.slots < cap || pool.slot_doubles < slot) {
    size_t slots = pool.slot_doubles == slot ? 2 * pool.slots : 0;
    if (slots < cap) slots = cap;
    if (slots < 64) slots = 64;
    if (slots > max_slots) slots = max_slots;
    if (pool.entries) (void)hipFree(pool.entries);
    if (pool.store) (void)hipFree(pool.store);
    pool = DgParkPool();
    HIPCHK(h, hipMalloc((void**)&pool.entries, sizeof(DgParkEntry) * slots));
    if (hipMalloc((void**)&pool.store, sizeof(double) * slot * slots) != hipSuccess) {      // no room: solve without deferral
      (void)hipGetLastError();
      (void)hipFree(pool.entries); pool.entries = nullptr;
      return DGSQP_OK;
    }
    pool.slots = slots; pool.slot_doubles = slot;
  }
  if (cap > pool.slots) cap = pool.slots;
  HIPCHK(h, hipMemsetAsync(pool.entries, 0, sizeof(DgParkEntry) * cap, stream));
  pool.owner = h; pool.owner_gen = h->launch_gen + 1;      // (the launch about to be enqueued)
  h->park_last_cap = cap;
  out->entries = pool.entries; out->store = pool.store; out->cap = (unsigned int)cap;
  out->min_it = min_it; out->factor_x16 = (int)(factor * 16.0 + 0.5); out->slot_doubles = slot;
  out->time_mode = time_mode;
  return DGSQP_OK;
}
static int grid_for(dgsqp_solver* h, int64_t B) {
  int64_t g = (int64_t)h->max_grid;
  if (B < g) g = B;
  if (g < 1) g = 1;
  return (int)g;
}

// helpers for the two test hooks: temporary device buffers
struct TmpBuf {
  std::vector<void*> ptrs;
  ~TmpBuf() { for (void* p : ptrs) (void)hipFree(p); }
  template <class T> T* alloc(size_t count) { void* p = nullptr; if (hipMalloc(&p, sizeof(T) * (count ? count : 1)) != hipSuccess) return nullptr; ptrs.push_back(p); return (T*)p; }
};

// one mapping from dg_build()'s message to the ABI's error code, shared by dgsqp_create and dgsqp_plan
static int build_error_code(const std::string& msg) {
  const bool too_large = msg.find("LDS") != std::string::npos || msg.find("too many") != std::string::npos || msg.find("not supported yet") != std::string::npos;
  return too_large ? DGSQP_E_TOO_LARGE : DGSQP_E_ARG;
}

// what dgsqp_dims and dgsqp_plan report about a built game
static void fill_dims(const DgProb& D, dgsqp_dims_t* out) {
  memset(out, 0, sizeof(*out));
  out->M = D.M; out->N = D.N; out->n_q = D.nq; out->n_u = D.nu; out->n = D.n; out->n_c = D.nc;
  out->n_dense = D.ndense; out->lds_bytes = D.L.total * 8; out->workspace_bytes = D.ws_doubles * (int64_t)sizeof(double);
  out->layout = D.big;
}

// every entry point that is about to use the handle's buffers for B scenarios: no launch in flight, scratch for the grid of B
static int idle_with_ws(dgsqp_solver* h, int64_t B) {
  const int rc = wait_idle(h);
  return rc ? rc : ensure_ws(h, (size_t)grid_for(h, B));
}

// What every launch that re-records ev[0] / ev[1] begins with.  Takes g_reg_mutex: the caller keeps `lock` until its kernel is
// enqueued and the handle marked in flight (upload_problem's contract).  The handle is idle (its callers waited for its last launch),
// and the host waits here for what is queued on the handle's OWN stream -- staging copies, the sampler, the fp32 widening, log
// set-up --, so the kernel may go to any stream; no launch stream is waited for: that would stall the host behind an older launch.
static int begin_launch(dgsqp_solver* h, std::unique_lock<std::mutex>& lock) {
  lock = std::unique_lock<std::mutex>(g_reg_mutex);
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "hipStreamSynchronize failed"; return DGSQP_E_DEVICE; }
  release_members(h);        // (members of an earlier grouped launch led by h: that kernel is done, its events are about to be reused)
  return upload_problem(h);
}

// The synchronous test hooks, between "inputs are on the device" and "kernels finished": `enqueue` puts the hook's kernels on h's stream
// while the registry is locked; the lock goes once the handle is marked in flight (a launch of another game then waits for them).
template <class F>
static int run_sync(dgsqp_solver* h, F enqueue) {
  {
    std::unique_lock<std::mutex> game_lock(g_reg_mutex);
    { const int rc = upload_problem(h); if (rc) return rc; }
    { const int rc = enqueue(); if (rc) return rc; }
    h->launch_stream = h->stream;
    h->in_flight = true;       // (the sampler's enqueue waits for every round itself: for that hook this mark and the wait below do nothing)
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->in_flight = false;
  return DGSQP_OK;
}

// ---- the two logs (DgLog) ----
// the buffer for a launch of B scenarios, or null while the log is off
static int log_for_launch(dgsqp_solver* h, DgLog& g, int64_t B, double** out) {
  *out = nullptr;
  if (g.cap <= 0) return DGSQP_OK;
  if (g.held < B) {
    if (g.buf) (void)hipFree(g.buf);
    g.buf = nullptr; g.held = 0;
    HIPCHK(h, hipMalloc(&g.buf, sizeof(double) * B * (size_t)g.doubles(h->hp)));
    g.held = B;
  }
  g.launch_B = B;
  *out = g.buf;
  return DGSQP_OK;
}
static int log_set(dgsqp_solver* h, DgLog& g, int cap) {
  if (cap < 0) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  g.cap = cap;
  g.held = g.launch_B = 0;
  if (g.buf) { (void)hipFree(g.buf); g.buf = nullptr; }
  return DGSQP_OK;
}
static int log_fetch(dgsqp_solver* h, DgLog& g, double* out, int64_t capacity_doubles, const char* none, const char* too_small) {
  if (!out || g.cap <= 0 || !g.buf || g.launch_B <= 0) { h->err = none; return DGSQP_E_ARG; }
  const int64_t need = g.launch_B * g.doubles(h->hp);
  if (capacity_doubles < need) { h->err = std::string(too_small) + std::to_string(need) + " doubles"; return DGSQP_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  HIPCHK(h, hipMemcpy(out, g.buf, sizeof(double) * need, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

// ---- the settings of closed-loop launches and their side buffers (DgSide) ----
static int side_reserve(dgsqp_solver* h, int i, size_t bytes) {
  DgBuf& b = h->side.b[i];
  if (bytes <= b.bytes) return DGSQP_OK;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr; b.bytes = 0;
  HIPCHK(h, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return DGSQP_OK;
}
// what a setter hands the device: reserve, then a synchronous copy
static int side_upload(dgsqp_solver* h, int i, const void* src, size_t bytes) {
  { const int rc = side_reserve(h, i, bytes); if (rc) return rc; }
  HIPCHK(h, hipMemcpy(h->side.b[i].p, src, bytes, hipMemcpyHostToDevice));
  return DGSQP_OK;
}
// A record a launch leaves behind for its dgsqp_fetch_*: `count` elements of `elem` bytes, every byte 0xff on h's stream (NaN, hit_step -1)
// for the kernel to write on top of.  The count is zero while anything can still fail.
static int side_record(dgsqp_solver* h, int i, int64_t count, size_t elem) {
  h->side.left[i] = 0;
  { const int rc = side_reserve(h, i, (size_t)count * elem); if (rc) return rc; }
  HIPCHK(h, hipMemsetAsync(h->side.b[i].p, 0xff, (size_t)count * elem, h->stream));
  h->side.left[i] = count;
  return DGSQP_OK;
}
// What every dgsqp_fetch_* of such records does: all of `what` as the last launch that filled them left them.  `name`: the records are
// doubles and `capacity` of them fit behind each pointer (null: the caller's arrays have the launch's shape).
struct DgFetch { int buf; void* out; size_t elem; };
static int side_fetch(dgsqp_solver* h, std::initializer_list<DgFetch> what, const char* none, const char* null_out, const char* name, int64_t capacity) {
  const DgSide& S = h->side;
  for (const DgFetch& f : what) if (S.left[f.buf] <= 0) { h->err = none; return DGSQP_E_ARG; }
  for (const DgFetch& f : what) if (!f.out) { h->err = null_out; return DGSQP_E_ARG; }
  for (const DgFetch& f : what)
    if (name && capacity < S.left[f.buf]) { h->err = std::string(name) + " buffer too small: need " + std::to_string(S.left[f.buf]) + " doubles"; return DGSQP_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  for (const DgFetch& f : what) HIPCHK(h, hipMemcpy(f.out, S.b[f.buf].p, f.elem * (size_t)S.left[f.buf], hipMemcpyDeviceToHost));
  return DGSQP_OK;
}
// what every dgsqp_set_* of these settings begins with: a handle, its device, no launch in flight
static int setter_begin(dgsqp_solver* h) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  return wait_idle(h);
}
static int refuse(dgsqp_solver* h, const char* setting, const std::string& m) { h->err = setting + m; return DGSQP_E_ARG; }
// every setting on top of the plant is refused without one
static int need_plant(dgsqp_solver* h, const char* setting) {
  return h->plant.set ? DGSQP_OK : refuse(h, setting, "no plant set (dgsqp_set_plant first; the identity plant will do)");
}
// The two checks the plant and the ensemble share, of `who` (an agent, or a chain's agent): "" or what is wrong.
static std::string delay_fault(const std::string& who, int j, int32_t d) {
  if (d >= 0 && d <= DGSQP_MAX_DELAY) return "";
  return "delay of " + who + ", input " + std::to_string(j) + " is " + std::to_string(d) + " simulation steps, allowed 0 .. " + std::to_string(DGSQP_MAX_DELAY);
}
static std::string model_fault(const std::string& who, int model, int game_model) {
  if (model == game_model) return "";
  return who + " is of model class " + std::to_string(model) + ", the game's is " + std::to_string(game_model);
}

// Per setting: what a launch of T steps and B chains must find (the order of these checks in dgsqp_closed_loop_batch decides which message
// a caller sees), and what a launch of `grid` workgroups hands the kernel -- per-workgroup buffers sized, records filled on h's stream.
static int further_check_plant(dgsqp_solver* h) {
  const DgEnsembleState& E = h->ens;
  if (!E.any() || h->plant.set) return DGSQP_OK;
  return refuse(h, E.B > 0 ? "plant ensemble" : E.est_T > 0 ? "estimate noise" : "monitor", ": no plant set for this launch");
}
static int drivers_check_launch(dgsqp_solver* h, int32_t T, int64_t B) {
  const DgDriversState& R = h->drv;
  if (!R.set) return DGSQP_OK;
  if (!h->plant.set) return refuse(h, "drivers: ", "no plant set for this launch");
  if (!h->cross.set)
    for (const int32_t k : R.kinds)
      if (k == DGSQP_DRIVER_TRACK) return refuse(h, "drivers: ", "a TRACK driver is set and no cross plant for this launch");
  if (R.T != T || R.B != B)
    return refuse(h, "drivers: ", "launch of T = " + std::to_string(T) + ", B = " + std::to_string(B) + ", the drivers were set for T = " + std::to_string(R.T) + ", B = " + std::to_string(R.B));
  return DGSQP_OK;
}
static int hold_check_launch(dgsqp_solver* h) {
  return !h->hold.set || h->plant.set ? DGSQP_OK : refuse(h, "plan hold: ", "no plant set for this launch");
}
static int further_check_launch(dgsqp_solver* h, int32_t T, int64_t B) {
  const DgEnsembleState& E = h->ens;
  if (E.B > 0 && E.B != B) return refuse(h, "plant ensemble: ", "launch of B = " + std::to_string(B) + " chains, the ensemble holds " + std::to_string(E.B));
  if (E.est_T > 0 && (E.est_T != T || E.est_B != B))
    return refuse(h, "estimate noise: ", "launch of T = " + std::to_string(T) + ", B = " + std::to_string(B) + ", the noise was set for T = " + std::to_string(E.est_T) + ", B = " + std::to_string(E.est_B));
  return DGSQP_OK;
}
// Every launch with a plant fills all four parts of the one pack: the feedback touches every per-workgroup buffer whatever is set.
// `wanted` false: the caller asked for no record of that part; its pointers stay null, the kernel skips the stores, and what an earlier
// launch left behind stays fetchable.
// the plant: delay lines per workgroup (the kernel clears them when a chain starts) and the u_plant record
static int plant_for_launch(dgsqp_solver* h, int grid, int64_t B, int64_t TB, DgPlantPack* pk) {
  const DgSide& S = h->side;
  { const int rc = side_reserve(h, SB_LINES, sizeof(double) * (size_t)grid * DGSQP_MAX_AGENTS * DGSQP_NUA * DGSQP_MAX_DELAY); if (rc) return rc; }
  { const int rc = side_record(h, SB_U_PLANT, TB * h->plant.host.sim_steps * h->hp.nu, sizeof(double)); if (rc) return rc; }
  pk->B = B; pk->P = S.at<const dgsqp_plant_t>(SB_PLANT); pk->lines = S.at<double>(SB_LINES); pk->u_plant = S.at<double>(SB_U_PLANT);
  return DGSQP_OK;
}
// the further settings, whichever are on (the others stay null and zero)
static int further_for_launch(dgsqp_solver* h, int grid, int64_t B, int64_t TB, DgPlantPack* pk) {
  const DgEnsembleState& E = h->ens;
  DgSide& S = h->side;
  if (E.B > 0) {
    if (sizeof(dgsqp_plant_t) * (size_t)grid > S.b[SB_WG_PLANT].bytes) {
      { const int rc = side_reserve(h, SB_WG_PLANT, sizeof(dgsqp_plant_t) * (size_t)grid); if (rc) return rc; }
      HIPCHK(h, hipMemsetAsync(S.b[SB_WG_PLANT].p, 0, S.b[SB_WG_PLANT].bytes, h->stream));
    }
    pk->vehicles = S.at<const dgsqp_vehicle_t>(SB_VEHICLES); pk->delay = E.has_delay ? S.at<const int32_t>(SB_DELAY) : nullptr; pk->wg_plant = S.at<dgsqp_plant_t>(SB_WG_PLANT);
  }
  if (E.est_T > 0) {
    { const int rc = side_record(h, SB_Q_EST, TB * h->hp.nq, sizeof(double)); if (rc) return rc; }
    pk->v = S.at<const double>(SB_V); pk->q_est = S.at<double>(SB_Q_EST);
  }
  if (E.monitor) {
    S.left[SB_CLEARANCE] = S.left[SB_BOX_EXCESS] = S.left[SB_HIT_STEP] = 0;      // one record in three arrays: none of it while any can fail
    { const int rc = side_reserve(h, SB_MON_SCRATCH, sizeof(double) * (size_t)grid * h->plant.host.sim_steps * h->hp.M * 3); if (rc) return rc; }
    { const int rc = side_record(h, SB_CLEARANCE, TB, sizeof(double)); if (rc) return rc; }
    { const int rc = side_record(h, SB_BOX_EXCESS, TB, sizeof(double)); if (rc) return rc; }
    { const int rc = side_record(h, SB_HIT_STEP, B, sizeof(int32_t)); if (rc) return rc; }
    pk->monitor = E.monitor; pk->mon_scratch = S.at<double>(SB_MON_SCRATCH); pk->clearance = S.at<double>(SB_CLEARANCE); pk->box_excess = S.at<double>(SB_BOX_EXCESS);
    pk->hit_step = S.at<int32_t>(SB_HIT_STEP);
  }
  return DGSQP_OK;
}
// the drivers: the per-workgroup PID state (the kernel writes before it reads it) and, when `wanted`, the u_cmd record.  A launch without
// drivers of the caller's runs with every agent of every chain on DGSQP_DRIVER_GAME: the kinds are built here (all-GAME is the launch
// without drivers, bit for bit); gains, references and replay are never read then.
static int drivers_for_launch(dgsqp_solver* h, int grid, int64_t B, int64_t TB, DgPlantPack* pk) {
  DgDriversState& R = h->drv;
  DgSide& S = h->side;
  const bool wanted = R.set || h->hold.set || h->cross.set;      // u_cmd null: every agent is GAME under the default hold, which is what the carry relies on
  if (!R.set) {
    static_assert(DGSQP_DRIVER_GAME == 0, "all-GAME kinds are a buffer of zero bytes");
    R.has_ref = R.has_replay = false;
    { const int rc = side_reserve(h, SB_KIND, sizeof(int32_t) * (size_t)B * h->hp.M); if (rc) return rc; }
    { const int rc = side_reserve(h, SB_PID, sizeof(dgsqp_pid_t) * DGSQP_MAX_AGENTS); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(S.b[SB_KIND].p, 0, sizeof(int32_t) * (size_t)B * h->hp.M, h->stream));
  }
  { const int rc = side_reserve(h, SB_PID_STATE, sizeof(double) * (size_t)grid * h->hp.M * 3); if (rc) return rc; }
  if (wanted) {
    S.left[SB_U_CMD] = 0;
    { const int rc = side_record(h, SB_U_CMD, TB * h->hp.nu, sizeof(double)); if (rc) return rc; }
    pk->u_cmd = S.at<double>(SB_U_CMD);
  }
  pk->kind = S.at<const int32_t>(SB_KIND); pk->pid = S.at<const dgsqp_pid_t>(SB_PID);
  pk->ref = R.has_ref ? S.at<const double>(SB_REF) : nullptr; pk->u_replay = R.has_replay ? S.at<const double>(SB_U_REPLAY) : nullptr;
  pk->pid_state = S.at<double>(SB_PID_STATE);
  return DGSQP_OK;
}
// the held plan: the per-workgroup (age, due) (the kernel writes before it reads it) and, when `wanted`, the u_game and plan_stage records.
// A launch without a hold of the caller's: R = 1 with the reference's rule, which is the launch without the setting, bit for bit.
static int hold_for_launch(dgsqp_solver* h, int grid, int64_t TB, DgPlantPack* pk) {
  DgSide& S = h->side;
  const bool wanted = h->hold.set || h->cross.set;
  { const int rc = side_reserve(h, SB_HOLD_STATE, sizeof(int32_t) * (size_t)grid * 2); if (rc) return rc; }
  if (wanted) {
    S.left[SB_U_GAME] = S.left[SB_PLAN_STAGE] = 0;      // one record in two arrays: none of it while either can fail
    { const int rc = side_record(h, SB_U_GAME, TB * h->hp.nu, sizeof(double)); if (rc) return rc; }
    { const int rc = side_record(h, SB_PLAN_STAGE, TB, sizeof(int32_t)); if (rc) return rc; }
    pk->u_game = S.at<double>(SB_U_GAME); pk->plan_stage = S.at<int32_t>(SB_PLAN_STAGE);
  }
  const dgsqp_hold_t off{1, DGSQP_HOLD_REFERENCE, (1u << DGSQP_DIVERGED) | (1u << DGSQP_QP_FAIL), 0};
  const dgsqp_hold_t& H = h->hold.set ? h->hold.host : off;
  pk->replan_every = H.replan_every; pk->on_fail = H.on_fail; pk->fail_mask = H.fail_mask;
  pk->state = S.at<int32_t>(SB_HOLD_STATE);
  return DGSQP_OK;
}
// The cross plant.  Before the launch: its shape, x0 = p(z0) bit for bit, no disturbance, and a GAME driver only where the game's inputs
// mean what the plant's do.  For the launch, in the pack's cross part: the z record with z0 in slice 0, and track_ref.
static int cross_check_launch(dgsqp_solver* h, int64_t B, const double* x0, const double* w) {
  const DgCrossState& X = h->cross;
  const DgProb& D = h->hp;
  if (!X.set) return DGSQP_OK;
  if (w) return refuse(h, "cross plant: ", "a disturbance w is in the game's layout and has no place in the plant's state z: pass NULL");
  if (B != X.B) return refuse(h, "cross plant: ", "launch of B = " + std::to_string(B) + " chains, z0 was set for " + std::to_string(X.B));
  for (int64_t b = 0; b < B; b++)
    for (int a = 0; a < D.M; a++)
      for (int i = 0; i < D.nqa[a]; i++)
        if (memcmp(&x0[b * D.nq + D.qoff[a] + i], &X.z0[b * X.nz_all + X.zoff[a] + X.proj[a][i]], sizeof(double)) != 0)
          return refuse(h, "cross plant: ", "x0 of chain " + std::to_string(b) + ", agent " + std::to_string(a) + ", entry " + std::to_string(i) + " is not the projection of z0 (bit for bit)");
  for (int a = 0; a < D.M; a++) {
    if (D.mdl[a] != DGSQP_MODEL_UNICYCLE_COMBINED || X.mdl[a] == DGSQP_MODEL_UNICYCLE_COMBINED) continue;
    for (int64_t b = 0; b < B; b++)
      if (!h->drv.set || h->drv.kinds[(size_t)b * D.M + a] == DGSQP_DRIVER_GAME)
        return refuse(h, "drivers: ", "agent " + std::to_string(a) + " is a point mass (inputs Fx, wz) on a bicycle plant (acceleration, steering): a GAME driver cannot command it" +
                      (h->drv.set ? " (chain " + std::to_string(b) + ")" : " (no drivers set: every agent is GAME)") + "; use TRACK, PID or REPLAY");
  }
  return DGSQP_OK;
}
static int cross_for_launch(dgsqp_solver* h, int64_t B, int32_t T, DgCrossPack* xp) {
  const DgCrossState& X = h->cross;
  DgSide& S = h->side;
  S.left[SB_Z] = S.left[SB_TRACK_REF] = 0;
  { const int rc = side_record(h, SB_Z, ((int64_t)T + 1) * B * X.nz_all, sizeof(double)); if (rc) return rc; }
  { const int rc = side_record(h, SB_TRACK_REF, (int64_t)T * B * h->hp.M * 3, sizeof(double)); if (rc) return rc; }
  HIPCHK(h, hipMemcpyAsync(S.b[SB_Z].p, X.z0.data(), sizeof(double) * X.z0.size(), hipMemcpyHostToDevice, h->stream));
  for (int a = 0; a < DGSQP_MAX_AGENTS; a++) { xp->mdl[a] = X.mdl[a]; xp->nz[a] = X.nz[a]; xp->zoff[a] = X.zoff[a]; }
  xp->nz_all = X.nz_all;
  memcpy(xp->proj, X.proj, sizeof(xp->proj));
  xp->lift = S.at<const dgsqp_problem_t>(SB_X_LIFT); xp->game = S.at<const dgsqp_plant_t>(SB_X_GAME);
  xp->z = S.at<double>(SB_Z); xp->track_ref = S.at<double>(SB_TRACK_REF);
  return DGSQP_OK;
}
// the one launch of dg_closed_loop_kernel, instantiated for the argument pack the settings call for (none: no plant)
template <class... PLANT>
static void launch_closed_loop(dgsqp_solver* h, int grid, int64_t B, const DgClosedLoop& cl, const PLANT&... pd) {
  hipLaunchKernelGGL(dg_closed_loop_kernel<PLANT...>, dim3(grid), dim3(DG_BLOCK), h->lds_bytes, h->stream, B, cl, h->ws, h->ticket, pd...);
}

// The one launch of dg_solve_kernel: L's staged batch, or -- with `group`, the host image of `count` batches of L->B scenarios each,
// L's first -- all of them behind one ticket queue.  `total` scenarios in all.  Leaves L marked in flight.  Everything it enqueues goes
// to the next launch stream of the device's pool, which L records: waits, queries and timing follow that record.
static int launch_solve(dgsqp_solver* L, int64_t total, const DgBatch* group, int count) {
  const int grid = grid_for(L, total);
  std::unique_lock<std::mutex> game_lock;
  { const int rc = begin_launch(L, game_lock); if (rc) return rc; }
  { const int rc = ensure_launch_streams(L); if (rc) return rc; }
  DgLaunchStreams& pool = g_launch_streams[L->device & 63];
  const hipStream_t stream = pool.streams[pool.next % pool.streams.size()];
  double *trace = nullptr, *itlog = nullptr;      // (a grouped launch has neither: its caller refuses handles that record logs)
  { const int rc = log_for_launch(L, L->trace, total, &trace); if (rc) return rc; }
  { const int rc = log_for_launch(L, L->itlog, total, &itlog); if (rc) return rc; }
  if (group) HIPCHK(L, hipMemcpyAsync(L->d_group, group, sizeof(DgBatch) * count, hipMemcpyHostToDevice, stream));
  HIPCHK(L, hipMemsetAsync(L->ticket, 0, sizeof(unsigned long long), stream));
  const bool coop = coop_for_launch(L, grid);
  if (coop) HIPCHK(L, hipMemsetAsync(L->d_coop, 0, L->coop_bytes, stream));
  DgPark park;
  { const int rc = park_for_launch(L, stream, coop, grid, total, &park); if (rc) return rc; }
  HIPCHK(L, hipEventRecord(L->ev[0], stream));
  *L->drained_host = 0u;
  hipLaunchKernelGGL(dg_solve_kernel, dim3(grid), dim3(DG_BLOCK), L->lds_bytes, stream, L->dp, L->B, L->staged.dbl(DG_Q), L->staged.dbl(DG_UWS),
                     L->staged.out(rec_count_batch(L->B)), L->ws, L->ticket, trace, L->trace.cap, L->drained_dev, itlog, L->itlog.cap,
                     group ? (const DgBatch*)L->d_group : (const DgBatch*)nullptr, group ? count : 0,
                     coop ? L->d_coop : (DgCoop*)nullptr, L->d_coop_payload, coop_start_trials(), coop_verify_mode(), coop_window_trials(), coop_max_helpers(), park,
                     L->up.ptr(), L->up.staged_stride);
  HIPCHK(L, hipGetLastError());
  pool.next++;
  L->launch_stream = stream;
  L->launch_gen++;
  L->launched_grid = grid;
  L->in_flight = true;       // (only now: an error return above leaves the handle idle)
  HIPCHK(L, hipEventRecord(L->ev[1], stream));
  return DGSQP_OK;
}

extern "C" {

int dgsqp_backend_info(char* buf, int buflen) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    snprintf(buf, buflen, "no HIP device");
    return DGSQP_E_DEVICE;
  }
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) return DGSQP_E_DEVICE;
  snprintf(buf, buflen, "%s arch=%s CUs=%d LDS/WG=%zu devices=%d", p.name, p.gcnArchName, p.multiProcessorCount, (size_t)p.sharedMemPerBlock, ndev);
  return DGSQP_OK;
}

int dgsqp_create(const dgsqp_problem_t* prob, const dgsqp_params_t* par, int device, dgsqp_handle_t* out) {
  if (!prob || !par || !out) { g_create_err = "null argument"; return DGSQP_E_ARG; }
  dgsqp_solver* h = new dgsqp_solver();
  std::string msg = dg_build(*prob, *par, h->hp);
  if (!msg.empty()) {
    g_create_err = msg;
    delete h;
    return build_error_code(msg);
  }
  h->rec = rec_table(h->hp);
  if (DG_BLOCK != 512 && (h->hp.big == 2 || h->hp.classic_qp || h->hp.osqp)) {
    // the -DDG_BLOCK=256 build (two workgroups per CU, row N1): explicit-inverse layouts (n <= 128) with the active-set QP only
    g_create_err = "too large: this build (DG_BLOCK = 256, two workgroups per CU) holds the LDS-resident and big explicit-inverse layouts with the active-set QP only";
    delete h;
    return DGSQP_E_TOO_LARGE;
  }
  auto fail = [&](const std::string& m) { g_create_err = m; dgsqp_destroy(h); return DGSQP_E_DEVICE; };
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail("device index out of range");
  h->device = device;
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) return fail("hipGetDeviceProperties failed");
  h->num_cu = p.multiProcessorCount;
  h->lds_bytes = (size_t)h->hp.L.total * sizeof(double);
  int rc_pool;      // (the launch streams first: they get hardware queues of their own before the handles' streams share them out)
  { std::lock_guard<std::mutex> lk(g_reg_mutex); rc_pool = ensure_launch_streams(h); }
  if (rc_pool != DGSQP_OK) return fail("hipStreamCreate (launch streams) failed");
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
  h->launch_stream = h->stream;
  for (auto& e : h->ev) if (hipEventCreate(&e) != hipSuccess) return fail("hipEventCreate failed");
  if (hipMalloc(&h->dp, sizeof(DgProb)) != hipSuccess) return fail("hipMalloc(problem) failed");
  if (hipMemcpy(h->dp, &h->hp, sizeof(DgProb), hipMemcpyHostToDevice) != hipSuccess) return fail("hipMemcpy(problem) failed");
  if (hipMalloc(&h->ticket, sizeof(unsigned long long)) != hipSuccess) return fail("hipMalloc(ticket) failed");
  if (hipMalloc((void**)&h->up.zero, sizeof(double) * h->hp.nu) != hipSuccess || hipMemset(h->up.zero, 0, sizeof(double) * h->hp.nu) != hipSuccess) return fail("hipMalloc(u_prev zeros) failed");
  if (hipHostMalloc((void**)&h->drained_host, sizeof(unsigned int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return fail("hipHostMalloc(flag) failed");
  *h->drained_host = 1u;
  if (hipHostGetDevicePointer((void**)&h->drained_dev, h->drained_host, 0) != hipSuccess) return fail("hipHostGetDevicePointer failed");
  h->coop_bytes = sizeof(DgCoop) + sizeof(DgCoopJob) * 2 * (size_t)(h->num_cu * 2 + 2);
  if (hipMalloc((void**)&h->d_coop, h->coop_bytes) != hipSuccess) return fail("hipMalloc(coop) failed");
  if (hipMalloc((void**)&h->d_coop_payload, sizeof(double) * 2 * (2 * (size_t)h->hp.n + 2 * (size_t)h->hp.nc) * (size_t)(h->num_cu * 2 + 2)) != hipSuccess) return fail("hipMalloc(coop payload) failed");
  const void* kernels[] = {(const void*)dg_solve_kernel, (const void*)dg_evaluate_kernel, (const void*)dg_qp_kernel, (const void*)dg_closed_loop_kernel<>,
                           (const void*)dg_closed_loop_kernel<DgPlantPack>, (const void*)dg_closed_loop_kernel<DgCrossPack>};
  for (const void* k : kernels) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes);
    if (e != hipSuccess) return fail(std::string("hipFuncSetAttribute(dynamic LDS): ") + hipGetErrorString(e));
  }
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, dg_solve_kernel, DG_BLOCK, h->lds_bytes) != hipSuccess || occ < 1) occ = 1;
  h->wg_per_cu = occ;
  h->max_grid = h->num_cu * occ;
  { std::lock_guard<std::mutex> lk(g_reg_mutex); g_handles.push_back(h); }
  *out = h;
  return DGSQP_OK;
}

void dgsqp_destroy(dgsqp_handle_t h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->in_flight && active_stream(h)) (void)hipStreamSynchronize(active_stream(h));      // the launch in flight first: nothing it uses is freed under it
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  { std::lock_guard<std::mutex> lk(g_reg_mutex); for (dgsqp_solver* o : g_handles) if (o->group_leader == h) { o->group_leader = nullptr; o->in_flight = false; } }
  if (h->d_group) (void)hipFree(h->d_group);
  if (h->group_host) (void)hipHostFree(h->group_host);
  if (h->comm) (void)dgsqp_comm_destroy(h);
  { std::lock_guard<std::mutex> lk(g_reg_mutex); g_handles.erase(std::remove(g_handles.begin(), g_handles.end(), h), g_handles.end()); }
  rec_free(h->staged);
  rec_free(h->closed);
  if (h->ws) (void)hipFree(h->ws);
  if (h->dp) (void)hipFree(h->dp);
  if (h->ticket) (void)hipFree(h->ticket);
  if (h->up.zero) (void)hipFree(h->up.zero);
  if (h->up.staged.p) (void)hipFree(h->up.staged.p);
  if (h->d_coop) (void)hipFree(h->d_coop);
  if (h->d_coop_payload) (void)hipFree(h->d_coop_payload);
  mpc_log_free(h);
  if (h->rl.T) (void)hipFree(h->rl.T);
  if (h->rl.cols) (void)hipFree(h->rl.cols);
  if (h->rl.qref) (void)hipFree(h->rl.qref);
  {
    std::lock_guard<std::mutex> lk(g_reg_mutex);
    DgParkPool& pool = g_park[h->device & 63];
    if (pool.owner == h) pool.owner = nullptr;
    // last handle of the device: its launch streams go as well (none has work left: every handle waited for its launch above)
    if (std::none_of(g_handles.begin(), g_handles.end(), [&](const dgsqp_solver* o) { return o->device == h->device; })) {
      DgLaunchStreams& ls = g_launch_streams[h->device & 63];
      for (hipStream_t s : ls.streams) (void)hipStreamDestroy(s);
      ls = DgLaunchStreams();
    }
    if (g_handles.empty()) {          // last handle of the process: the pools go as well
      for (DgParkPool& pl : g_park) {
        if (pl.entries || pl.store) {
          // (the pool's memory belongs to the device it was allocated on)
          if (pl.entries) (void)hipFree(pl.entries);
          if (pl.store) (void)hipFree(pl.store);
          pl = DgParkPool();
        }
      }
    }
  }
  if (h->drained_host) (void)hipHostFree(h->drained_host);
  if (h->trace.buf) (void)hipFree(h->trace.buf);
  if (h->itlog.buf) (void)hipFree(h->itlog.buf);
  for (DgBuf& b : h->side.b) if (b.p) (void)hipFree(b.p);
  for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int dgsqp_dims(dgsqp_handle_t h, dgsqp_dims_t* out) {
  if (!h || !out) return DGSQP_E_ARG;
  fill_dims(h->hp, out);
  return DGSQP_OK;
}

int dgsqp_plan(const dgsqp_problem_t* prob, const dgsqp_params_t* par, dgsqp_dims_t* out, char* msg, int msglen) {
  if (!prob || !par || !out) return DGSQP_E_ARG;
  static DgProb D;     // ~100 KB: not on the stack (single-threaded helper, like dgsqp_create)
  const std::string err = dg_build(*prob, *par, D);
  if (msg && msglen > 0) snprintf(msg, msglen, "%s", err.c_str());
  fill_dims(D, out);
  if (!err.empty()) return build_error_code(err);
  return DGSQP_OK;
}

const char* dgsqp_last_error(dgsqp_handle_t h) { return h ? h->err.c_str() : g_create_err.c_str(); }

// what dgsqp_stage_inputs, the fp32 boundary and the sampler begin with: the handle idle, then staged arrays and scratch for B scenarios
static int stage_begin(dgsqp_solver* h, int64_t B) {
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }            // the buffers below belong to the launch in flight, if any
  h->up.staged_stride = 0;          // (a batch staged without dgsqp_set_u_prev's array -- the sampler's -- runs from zeros)
  if (B == 0) return DGSQP_OK;
  int rc = rec_reserve(h, h->staged, rec_count_batch(B));
  if (!rc) rc = ensure_ws(h, (size_t)grid_for(h, B));
  if (rc) h->B = 0;        // (some staged buffers may be gone: nothing is staged any more)
  return rc;
}

// dgsqp_set_u_prev and the entry points it applies to.  A call of another batch size is refused before it touches anything.
static int u_prev_check(dgsqp_solver* h, int64_t B) {
  if (h->up.B == 0 || B == 0 || h->up.B == B) return DGSQP_OK;
  return refuse(h, "u_prev: ", "set for B = " + std::to_string(h->up.B) + " scenarios, this call has B = " + std::to_string(B) + " (dgsqp_set_u_prev with the new batch, or with B = 0 to switch it off)");
}
// after stage_begin: the staged batch captures the array (copy on h's stream, which every launch waits for)
static int u_prev_stage(dgsqp_solver* h, int64_t B) {
  if (h->up.B == 0 || h->up.B != B) return DGSQP_OK;
  const size_t bytes = sizeof(double) * (size_t)B * h->hp.nu;
  DgBuf& b = h->up.staged;
  if (bytes > b.bytes) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.bytes = 0;
    HIPCHK(h, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
  }
  HIPCHK(h, hipMemcpyAsync(b.p, h->up.host.data(), bytes, hipMemcpyHostToDevice, h->stream));
  h->up.staged_stride = h->hp.nu;
  return DGSQP_OK;
}
// the two synchronous hooks: the array (set for exactly this B) in a temporary buffer of the call, or the handle's zeros
static int u_prev_hook(dgsqp_solver* h, int64_t B, TmpBuf& tb, const double** up, int64_t* stride) {
  *up = h->up.zero; *stride = 0;
  if (h->up.B == 0 || h->up.B != B) return DGSQP_OK;
  double* d = tb.alloc<double>((size_t)B * h->hp.nu);
  if (!d) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(d, h->up.host.data(), sizeof(double) * (size_t)B * h->hp.nu, hipMemcpyHostToDevice));
  *up = d; *stride = h->hp.nu;
  return DGSQP_OK;
}
// both setters refuse entries that are not finite
static int64_t first_non_finite(const double* v, int64_t count) {
  for (int64_t i = 0; i < count; i++) if (!std::isfinite(v[i])) return i;
  return -1;
}

int dgsqp_set_u_prev(dgsqp_handle_t h, int64_t B, const double* u_prev) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgUPrevState& U = h->up;
  if (!u_prev && B == 0) { U.B = 0; U.host.clear(); return DGSQP_OK; }
  if (!u_prev || B <= 0) return refuse(h, "u_prev: ", "needs B > 0 scenarios and an array [B][n_u] (NULL with B = 0 switches it off)");
  const int nu = h->hp.nu;
  const int64_t bad = first_non_finite(u_prev, B * nu);
  if (bad >= 0) return refuse(h, "u_prev: ", "entry [" + std::to_string(bad / nu) + "][" + std::to_string(bad % nu) + "] is not finite");
  U.host.assign(u_prev, u_prev + B * nu);
  U.B = B;
  return DGSQP_OK;
}

int dgsqp_set_closed_loop_u_prev(dgsqp_handle_t h, int mode, int64_t B, const double* u_prev0) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgUPrevState& U = h->up;
  if (mode == 0) { U.cl_mode = 0; U.cl_B = 0; U.cl_host.clear(); return DGSQP_OK; }
  if (mode != 1) return refuse(h, "closed-loop u_prev: ", "mode must be 0 (off) or 1 (carry), got " + std::to_string(mode));
  if (B < 0) return refuse(h, "closed-loop u_prev: ", "B must not be negative");
  const int nu = h->hp.nu;
  if (u_prev0) {
    const int64_t bad = first_non_finite(u_prev0, B * nu);
    if (bad >= 0) return refuse(h, "closed-loop u_prev: ", "u_prev0 entry [" + std::to_string(bad / nu) + "][" + std::to_string(bad % nu) + "] is not finite");
    U.cl_host.assign(u_prev0, u_prev0 + B * nu);
    U.cl_B = B;
  } else { U.cl_host.clear(); U.cl_B = 0; }
  U.cl_mode = 1;
  return DGSQP_OK;
}
int dgsqp_fetch_u_prev(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  const char* none = "no closed-loop launch that carries u_prev has run";
  return h ? side_fetch(h, {{SB_U_PREV, out, sizeof(double)}}, none, none, "u_prev", capacity_doubles) : DGSQP_E_ARG;
}

int dgsqp_stage_inputs(dgsqp_handle_t h, int64_t B, const double* x0, const double* u_ws) {
  if (!h || B < 0 || (B > 0 && (!x0 || !u_ws))) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  int rc = u_prev_check(h, B);
  if (rc) return rc;
  rc = stage_begin(h, B);
  if (rc) return rc;
  h->B = B;
  if (B == 0) return DGSQP_OK;
  if ((rc = u_prev_stage(h, B))) return rc;
  void* in[DG_REC_COUNT] = {};
  in[DG_Q] = (void*)x0; in[DG_UWS] = (void*)u_ws;
  if ((rc = rec_copy(h, h->staged, rec_count_batch(B), in, hipMemcpyHostToDevice))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DGSQP_OK;
}

int dgsqp_launch_staged(dgsqp_handle_t h) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  { int rcw = wait_idle(h); if (rcw) return rcw; }     // one launch in flight per handle
  h->launched_grid = 0;
  if (h->B == 0) return DGSQP_OK;
  return launch_solve(h, h->B, nullptr, 0);
}

int dgsqp_launch_staged_group(const dgsqp_handle_t* hs, int count) {
  if (!hs || count < 1 || count > DG_GROUP_MAX || !hs[0]) return DGSQP_E_ARG;
  dgsqp_solver* L = hs[0];
  if (count == 1) return dgsqp_launch_staged(L);
  HIPCHK(L, hipSetDevice(L->device));
  for (int i = 0; i < count; i++) {
    dgsqp_solver* h = hs[i];
    if (!h) { L->err = "null handle in the group"; return DGSQP_E_ARG; }
    for (int j = 0; j < i; j++) if (hs[j] == h) { L->err = "a handle appears twice in the group"; return DGSQP_E_ARG; }
    if (h->device != L->device || h->B != L->B || L->B <= 0 || memcmp(&h->hp, &L->hp, sizeof(DgProb)) != 0) {
      L->err = "grouped launch: every handle must hold a staged batch of the same size, of the same game, on the same device"; return DGSQP_E_ARG;
    }
    if (h->trace.cap > 0 || h->itlog.cap > 0) { L->err = "grouped launch: event / iterate logs are per single launch"; return DGSQP_E_ARG; }
    const int rcw = wait_idle(h);
    if (rcw) return rcw;
  }
  { const int rce = ensure_ws(L, (size_t)grid_for(L, L->B * count)); if (rce) return rce; }
  if (!L->d_group) HIPCHK(L, hipMalloc(&L->d_group, sizeof(DgBatch) * DG_GROUP_MAX));
  if (!L->group_host) HIPCHK(L, hipHostMalloc((void**)&L->group_host, sizeof(DgBatch) * DG_GROUP_MAX, hipHostMallocDefault));
  for (int i = 0; i < count; i++) L->group_host[i] = DgBatch{hs[i]->staged.dbl(DG_Q), hs[i]->staged.dbl(DG_UWS), hs[i]->staged.out(rec_count_batch(L->B)), hs[i]->up.ptr(), hs[i]->up.staged_stride};
  const int rc = launch_solve(L, L->B * count, L->group_host, count);
  // (every handle was idle above: the leader is in flight exactly when the kernel was enqueued, and then so are the members' batches)
  if (L->in_flight)
    for (int i = 0; i < count; i++) { hs[i]->launched_grid = L->launched_grid; hs[i]->in_flight = true; hs[i]->group_leader = i == 0 ? nullptr : L; hs[i]->group_gen = L->launch_gen; }
  return rc;
}

int dgsqp_draining(dgsqp_handle_t h) {
  if (!h) return 1;
  const dgsqp_solver* L = h->group_leader ? h->group_leader : h;
  return h->launched_grid == 0 || __atomic_load_n(L->drained_host, __ATOMIC_RELAXED) != 0u;
}

int dgsqp_finished(dgsqp_handle_t h) {
  if (!h || !h->in_flight || h->launched_grid == 0) return 1;
  if (hipSetDevice(h->device) != hipSuccess) return 1;
  return hipEventQuery((h->group_leader ? h->group_leader : h)->ev[1]) != hipErrorNotReady;      // (a member whose leader has moved on was released: not in flight)
}

int dgsqp_wait(dgsqp_handle_t h, dgsqp_timing_t* tm) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (tm) memset(tm, 0, sizeof(*tm));
  { const int rc = wait_idle(h); if (rc) return rc; }           // (a member of a grouped launch waits for, and reports, the group's kernel)
  if (tm && h->launched_grid > 0) { tm->kernel_ms = h->last_ms; tm->total_ms = h->last_ms; tm->grid = h->launched_grid; tm->block = DG_BLOCK; }
  return DGSQP_OK;
}

int dgsqp_solve_staged(dgsqp_handle_t h, dgsqp_timing_t* tm) {
  if (!h) return DGSQP_E_ARG;
  h->coop_next_sync = true;          // the caller waits for this launch: idle workgroups help with its line searches
  const int rc = dgsqp_launch_staged(h);
  h->coop_next_sync = false;
  if (rc != DGSQP_OK) return rc;
  return dgsqp_wait(h, tm);
}

int dgsqp_set_cooperative(dgsqp_handle_t h, int mode) {
  if (!h || mode < 0 || mode > 2) return DGSQP_E_ARG;
  h->coop_mode = mode;
  return DGSQP_OK;
}

int dgsqp_set_deferral(dgsqp_handle_t h, int min_iters, double factor) {
  if (!h || min_iters < 0 || !(factor >= 0.0) || factor > 1000.0) return DGSQP_E_ARG;
  h->defer_min_it = min_iters;
  h->defer_factor = factor;
  h->defer_requested = true;
  return DGSQP_OK;
}

int dgsqp_reserve_deferral(dgsqp_handle_t h, int64_t scenarios) {
  if (!h || scenarios < 1) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(g_reg_mutex);
  { const int rcw = wait_idle(h); if (rcw) return rcw; }
  DgParkPool& pool = g_park[h->device & 63];
  dgsqp_solver* const owner = pool.owner;
  const unsigned long long owner_gen = pool.owner_gen;
  DgPark unused;
  const int rc = park_for_launch(h, h->stream, true, h->max_grid, scenarios, &unused);      // (sizes the device's pool exactly as that launch would)
  h->park_last_cap = 0;
  // no launch follows: the pool must not look taken by this handle's NEXT launch (a plain one would make other handles' cooperative
  // launches find it "busy" and run without deferral).  A re-allocation reset the owner anyway; otherwise put back what was there.
  if (g_park[h->device & 63].owner == h) { g_park[h->device & 63].owner = owner == h ? nullptr : owner; g_park[h->device & 63].owner_gen = owner == h ? 0 : owner_gen; }
  return rc;
}

int dgsqp_deferral_stats(dgsqp_handle_t h, uint64_t* out2) {
  if (!h || !out2 || !h->d_coop) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  DgCoop hdr;
  HIPCHK(h, hipMemcpy(&hdr, h->d_coop, sizeof(DgCoop) - sizeof(DgCoopJob), hipMemcpyDeviceToHost));
  out2[0] = hdr.park_pushed < h->park_last_cap ? hdr.park_pushed : (uint64_t)h->park_last_cap;
  out2[1] = hdr.park_resumed;
  return DGSQP_OK;
}

int dgsqp_deferral_log(dgsqp_handle_t h, uint64_t* out, int64_t cap_rows) {
  if (!h || !out || cap_rows < 0) return -1;
  if (hipSetDevice(h->device) != hipSuccess || wait_idle(h) != DGSQP_OK) return 0;
  std::lock_guard<std::mutex> lk(g_reg_mutex);
  const DgParkPool& pool = g_park[h->device & 63];
  if (!pool.entries || pool.owner != h) return 0;        // (another launch has used the device's pool since)
  uint64_t st[2];
  if (dgsqp_deferral_stats(h, st) != DGSQP_OK) return -1;
  const int64_t n = (int64_t)st[0] < cap_rows ? (int64_t)st[0] : cap_rows;
  std::vector<DgParkEntry> e((size_t)n);
  if (n > 0 && hipMemcpy(e.data(), pool.entries, sizeof(DgParkEntry) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (int64_t i = 0; i < n; i++) {
    uint64_t* r = out + 11 * i;
    memcpy(r + 8, e[i].cond, sizeof(double) * 3);
    r[0] = (uint64_t)e[i].ticket; r[1] = (uint64_t)e[i].sqp_it; r[2] = (uint64_t)e[i].total_qp; r[3] = e[i].key;
    r[4] = e[i].t_park; r[5] = e[i].t_resume; r[6] = e[i].t_done; r[7] = ((uint64_t)(uint32_t)e[i].final_qps << 32) | (uint32_t)e[i].final_its;
  }
  return (int)n;
}

int dgsqp_coop_stats(dgsqp_handle_t h, uint64_t* out4 /* six values */) {
  if (!h || !out4 || !h->d_coop) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  DgCoop hdr;
  HIPCHK(h, hipMemcpy(&hdr, h->d_coop, sizeof(DgCoop) - sizeof(DgCoopJob), hipMemcpyDeviceToHost));
  out4[0] = hdr.helped; out4[1] = hdr.helper_regs; out4[2] = hdr.finished; out4[3] = hdr.idle;
  out4[4] = hdr.used; out4[5] = hdr.mismatches;
  return DGSQP_OK;
}

int dgsqp_osqp_counters(dgsqp_handle_t h, uint64_t* out2, int reset) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  if (out2) {
    unsigned long long v[2] = {0ull, 0ull};
    HIPCHK(h, hipMemcpyFromSymbol(v, HIP_SYMBOL(dg_osqp_count), sizeof v));
    out2[0] = v[0]; out2[1] = v[1];
  }
  if (reset) {
    const unsigned long long z[2] = {0ull, 0ull};
    HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(dg_osqp_count), z, sizeof z));
  }
  return DGSQP_OK;
}

int dgsqp_fetch_results(dgsqp_handle_t h, double* u_out, double* l_out, double* x_out, int32_t* status, int32_t* iters,
                        int32_t* qp_solves, double* cond, double* cost) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->B == 0) return DGSQP_OK;
  { const int rcw = wait_idle(h); if (rcw) return rcw; }      // (a member of a grouped launch was solved on its leader's stream)
  void* dst[DG_REC_COUNT];
  rec_host_table(dst, u_out, l_out, x_out, status, iters, qp_solves, cond, cost);
  { const int rc = rec_copy(h, h->staged, rec_count_batch(h->B), dst, hipMemcpyDeviceToHost); if (rc) return rc; }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DGSQP_OK;
}

int dgsqp_solve_batch(dgsqp_handle_t h, int64_t B, const double* x0, const double* u_ws, double* u_out, double* l_out,
                      double* x_out, int32_t* status, int32_t* iters, int32_t* qp_solves, double* cond, double* cost,
                      dgsqp_timing_t* tm) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  int rc = dgsqp_stage_inputs(h, B, x0, u_ws);
  if (rc) return rc;
  dgsqp_timing_t t2;
  rc = dgsqp_solve_staged(h, &t2);
  if (rc) return rc;
  rc = dgsqp_fetch_results(h, u_out, l_out, x_out, status, iters, qp_solves, cond, cost);
  if (rc) return rc;
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (tm) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    *tm = t2;
    tm->total_ms = ms;
  }
  return DGSQP_OK;
}

int dgsqp_set_plant(dgsqp_handle_t h, const dgsqp_plant_t* plant) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgPlantState& S = h->plant;
  if (h->cross.set) { h->cross.set = false; S.set = false; }      // (a cross plant's record is not a plant of the game's class)
  if (!plant) { S.set = false; return DGSQP_OK; }
  auto bad = [&](const std::string& m) { return refuse(h, "plant: ", m); };
  const int integ = plant->integrator;
  if (integ != DGSQP_INT_EULER && integ != DGSQP_INT_RK4 && integ != DGSQP_INT_RK3 && integ != DGSQP_INT_RK2) return bad("unknown integrator " + std::to_string(integ));
  if (plant->substeps < 1) return bad("substeps must be at least 1, got " + std::to_string(plant->substeps));
  if (plant->sim_steps < 1) return bad("sim_steps must be at least 1, got " + std::to_string(plant->sim_steps));
  const dgsqp_problem_t& P = h->hp.P;
  for (int a = 0; a < P.M; a++) {
    const std::string who = "agent " + std::to_string(a);
    for (int j = 0; j < DGSQP_NUA; j++) { const std::string m = delay_fault(who, j, plant->delay[a][j]); if (!m.empty()) return bad(m); }
    if (!plant->use_game_agents) { const std::string m = model_fault(who, plant->agents[a].model, P.agents[a].model); if (!m.empty()) return bad(m); }
  }
  S.host = *plant;
  if (plant->use_game_agents) memcpy(S.host.agents, P.agents, sizeof(P.agents));
  { const int rc = side_upload(h, SB_PLANT, &S.host, sizeof(dgsqp_plant_t)); if (rc) return rc; }
  S.set = true;
  return DGSQP_OK;
}
int dgsqp_fetch_u_plant(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  const char* none = "no closed-loop launch with a plant has run";
  return h ? side_fetch(h, {{SB_U_PLANT, out, sizeof(double)}}, none, none, "u_plant", capacity_doubles) : DGSQP_E_ARG;
}

// the pairs (game class -> plant class) of the table in include/dgsqp.h
static bool cross_pair_ok(int game, int plant) {
  if (game == plant) return game >= DGSQP_MODEL_KIN_BICYCLE && game <= DGSQP_MODEL_UNICYCLE_COMBINED;
  if (plant == DGSQP_MODEL_DYN_BICYCLE) return game == DGSQP_MODEL_KIN_BICYCLE || game == DGSQP_MODEL_UNICYCLE_COMBINED;
  return game == DGSQP_MODEL_UNICYCLE_COMBINED && plant == DGSQP_MODEL_KIN_BICYCLE;
}
int dgsqp_set_cross_plant(dgsqp_handle_t h, const dgsqp_plant_t* plant, int64_t B, const double* z0) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgCrossState& X = h->cross;
  if (!plant) { if (X.set) { X.set = false; h->plant.set = false; } return DGSQP_OK; }
  auto bad = [&](const std::string& m) { return refuse(h, "cross plant: ", m); };
  const int integ = plant->integrator;
  if (integ != DGSQP_INT_EULER && integ != DGSQP_INT_RK4 && integ != DGSQP_INT_RK3 && integ != DGSQP_INT_RK2) return bad("unknown integrator " + std::to_string(integ));
  if (plant->substeps < 1) return bad("substeps must be at least 1, got " + std::to_string(plant->substeps));
  if (plant->sim_steps < 1) return bad("sim_steps must be at least 1, got " + std::to_string(plant->sim_steps));
  if (B < 1 || !z0) return bad("z0 [B][n_z] is needed, with B >= 1");
  const DgProb& D = h->hp;
  const dgsqp_problem_t& P = D.P;
  DgCrossState N;
  for (int a = 0; a < P.M; a++) {
    const std::string who = "agent " + std::to_string(a);
    for (int j = 0; j < DGSQP_NUA; j++) { const std::string m = delay_fault(who, j, plant->delay[a][j]); if (!m.empty()) return bad(m); }
    const int gm = P.agents[a].model, pm = plant->use_game_agents ? gm : plant->agents[a].model;
    if (!cross_pair_ok(gm, pm))
      return bad(who + ": a game agent of model class " + std::to_string(gm) + " on a plant of class " + std::to_string(pm) + " is not a supported pair (same class, 0 -> 1, 3 -> 0, 3 -> 1)");
    N.mdl[a] = pm; N.nz[a] = dg_model_nq(pm); N.zoff[a] = N.nz_all; N.nz_all += N.nz[a];
    for (int i = 0; i < D.nqa[a]; i++) N.proj[a][i] = (int8_t)(N.nz[a] == D.nqa[a] || i < 3 ? i : i + 2);      // 6 of 8: [0, 1, 2, 5, 6, 7]
  }
  N.B = B;
  N.z0.assign(z0, z0 + (size_t)B * N.nz_all);
  DgPlantState& S = h->plant;
  S.set = false; X.set = false;
  S.host = *plant;
  if (plant->use_game_agents) memcpy(S.host.agents, P.agents, sizeof(P.agents));
  { const int rc = side_upload(h, SB_PLANT, &S.host, sizeof(dgsqp_plant_t)); if (rc) return rc; }
  // the game as a plant (the reference of a TRACK driver is one step of it), and the game with its bounds in the plant's layout
  {
    std::vector<dgsqp_plant_t> g(1);
    memset(g.data(), 0, sizeof(dgsqp_plant_t));
    g[0].integrator = P.integrator; g[0].substeps = P.substeps; g[0].sim_steps = 1; g[0].use_game_agents = 1;
    memcpy(g[0].agents, P.agents, sizeof(P.agents));
    { const int rc = side_upload(h, SB_X_GAME, g.data(), sizeof(dgsqp_plant_t)); if (rc) return rc; }
    std::vector<dgsqp_problem_t> lift(1, P);
    for (int a = 0; a < P.M; a++) {
      dgsqp_agent_t& A = lift[0].agents[a];
      for (int i = 0; i < DGSQP_MAX_NQA; i++) { A.st_ub[i] = INFINITY; A.st_lb[i] = -INFINITY; }
      for (int i = 0; i < D.nqa[a]; i++) { A.st_ub[N.proj[a][i]] = P.agents[a].st_ub[i]; A.st_lb[N.proj[a][i]] = P.agents[a].st_lb[i]; }
    }
    { const int rc = side_upload(h, SB_X_LIFT, lift.data(), sizeof(dgsqp_problem_t)); if (rc) return rc; }
  }
  X = std::move(N);
  X.set = true; S.set = true;
  return DGSQP_OK;
}
int dgsqp_fetch_plant_state(dgsqp_handle_t h, double* z, int64_t capacity_doubles) {
  const char* none = "no closed-loop launch with a cross plant has run";
  return h ? side_fetch(h, {{SB_Z, z, sizeof(double)}}, none, none, "z", capacity_doubles) : DGSQP_E_ARG;
}
int dgsqp_fetch_track_ref(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  const char* none = "no closed-loop launch with a cross plant has run";
  return h ? side_fetch(h, {{SB_TRACK_REF, out, sizeof(double)}}, none, none, "track_ref", capacity_doubles) : DGSQP_E_ARG;
}

int dgsqp_set_plant_ensemble(dgsqp_handle_t h, int64_t B, const dgsqp_vehicle_t* vehicles, const int32_t* delay) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgEnsembleState& E = h->ens;
  if (!vehicles || B == 0) { E.B = 0; return DGSQP_OK; }
  auto bad = [&](const std::string& m) { return refuse(h, "plant ensemble: ", m); };
  { const int rc = need_plant(h, "plant ensemble: "); if (rc) return rc; }
  if (B < 0) return bad("B must not be negative");
  const int M = h->hp.P.M;
  for (int64_t b = 0; b < B; b++)
    for (int a = 0; a < M; a++) {
      const std::string who = "chain " + std::to_string(b) + ", agent " + std::to_string(a);
      if (h->cross.set) {
        if (vehicles[b * M + a].model != h->cross.mdl[a])
          return bad("vehicle of " + who + " is of model class " + std::to_string(vehicles[b * M + a].model) + ", the cross plant's agent is of class " + std::to_string(h->cross.mdl[a]));
      }
      else { const std::string m = model_fault("vehicle of " + who, vehicles[b * M + a].model, h->hp.P.agents[a].model); if (!m.empty()) return bad(m); }
      for (int j = 0; delay && j < DGSQP_NUA; j++) { const std::string m = delay_fault(who, j, delay[(b * M + a) * DGSQP_NUA + j]); if (!m.empty()) return bad(m); }
    }
  E.B = 0;
  { const int rc = side_upload(h, SB_VEHICLES, vehicles, sizeof(dgsqp_vehicle_t) * (size_t)B * M); if (rc) return rc; }
  if (delay) { const int rc = side_upload(h, SB_DELAY, delay, sizeof(int32_t) * (size_t)B * M * DGSQP_NUA); if (rc) return rc; }
  E.has_delay = delay != nullptr;
  E.B = B;
  return DGSQP_OK;
}
int dgsqp_set_estimate_noise(dgsqp_handle_t h, int32_t T, int64_t B, const double* v) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgEnsembleState& E = h->ens;
  if (!v || T == 0 || B == 0) { E.est_T = 0; E.est_B = 0; return DGSQP_OK; }
  { const int rc = need_plant(h, "estimate noise: "); if (rc) return rc; }
  if (T < 0 || B < 0) return refuse(h, "estimate noise: ", "T and B must not be negative");
  E.est_T = 0; E.est_B = 0;
  { const int rc = side_upload(h, SB_V, v, sizeof(double) * (size_t)T * (size_t)B * h->hp.nq); if (rc) return rc; }
  E.est_T = T; E.est_B = B;
  return DGSQP_OK;
}
int dgsqp_fetch_q_est(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  const char* none = "no closed-loop launch with state estimates has run";
  return h ? side_fetch(h, {{SB_Q_EST, out, sizeof(double)}}, none, none, "q_est", capacity_doubles) : DGSQP_E_ARG;
}
int dgsqp_set_monitor(dgsqp_handle_t h, int mode) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  if (mode == 0) { h->ens.monitor = 0; return DGSQP_OK; }
  if (mode != 1 && mode != 2) return refuse(h, "monitor: ", "mode must be 0 (off), 1 (record) or 2 (record and stop), got " + std::to_string(mode));
  { const int rc = need_plant(h, "monitor: "); if (rc) return rc; }
  h->ens.monitor = mode;
  return DGSQP_OK;
}
int dgsqp_fetch_monitor(dgsqp_handle_t h, double* clearance, double* box_excess, int32_t* hit_step) {
  if (!h) return DGSQP_E_ARG;
  return side_fetch(h, {{SB_CLEARANCE, clearance, sizeof(double)}, {SB_BOX_EXCESS, box_excess, sizeof(double)}, {SB_HIT_STEP, hit_step, sizeof(int32_t)}},
                    "no closed-loop launch with the monitor on has run", "monitor: null argument", nullptr, 0);
}

int dgsqp_set_drivers(dgsqp_handle_t h, const dgsqp_drivers_t* d, int32_t T, int64_t B, const int32_t* kind, const double* ref, const double* u_replay) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgDriversState& R = h->drv;
  if (!d) { R.set = false; return DGSQP_OK; }
  auto bad = [&](const std::string& m) { return refuse(h, "drivers: ", m); };
  { const int rc = need_plant(h, "drivers: "); if (rc) return rc; }
  if (T < 1) return bad("T must be at least 1, got " + std::to_string(T));
  if (B < 0) return bad("B must not be negative");
  const dgsqp_problem_t& P = h->hp.P;
  const int M = P.M;
  // the kinds of every chain: d->kind where the caller gives none per chain; both are checked, whichever the launch will read
  std::vector<int32_t> kinds((size_t)B * M);
  bool replay = false;
  auto check = [&](int32_t k, int a, const std::string& where) -> int {
    if (k == DGSQP_DRIVER_TRACK && h->cross.set) {
      if (P.agents[a].model == DGSQP_MODEL_UNICYCLE)
        return bad("TRACK driver for " + where + ", a unicycle: the lane follower needs e_y and e_psi (the 6- and 8-state models)");
      return DGSQP_OK;
    }
    if (k == DGSQP_DRIVER_TRACK) return bad("kind of " + where + " is 3 (track): a TRACK driver needs a cross plant (dgsqp_set_cross_plant; the identity cross plant will do)");
    if (k != DGSQP_DRIVER_GAME && k != DGSQP_DRIVER_PID && k != DGSQP_DRIVER_REPLAY)
      return bad("kind of " + where + " is " + std::to_string(k) + ", allowed 0 (game), 1 (PID), 2 (replay)");
    if (k == DGSQP_DRIVER_PID && P.agents[a].model == DGSQP_MODEL_UNICYCLE)
      return bad("PID driver for " + where + ", a unicycle: the lane follower needs e_y and e_psi (the 6- and 8-state models)");
    replay = replay || k == DGSQP_DRIVER_REPLAY;
    return DGSQP_OK;
  };
  for (int a = 0; a < M; a++) { const int rc = check(d->kind[a], a, "agent " + std::to_string(a)); if (rc) return rc; }
  for (int64_t b = 0; b < B; b++)
    for (int a = 0; a < M; a++) {
      const int32_t k = kind ? kind[b * M + a] : d->kind[a];
      if (kind) { const int rc = check(k, a, "chain " + std::to_string(b) + ", agent " + std::to_string(a)); if (rc) return rc; }
      kinds[(size_t)b * M + a] = k;
    }
  if (replay && !u_replay) return bad("a REPLAY driver needs u_replay");
  R.set = false;
  { const int rc = side_upload(h, SB_PID, d->pid, sizeof(d->pid)); if (rc) return rc; }
  if (B > 0) {
    { const int rc = side_upload(h, SB_KIND, kinds.data(), sizeof(int32_t) * kinds.size()); if (rc) return rc; }
    if (ref) { const int rc = side_upload(h, SB_REF, ref, sizeof(double) * (size_t)B * M * 2); if (rc) return rc; }
    if (u_replay) { const int rc = side_upload(h, SB_U_REPLAY, u_replay, sizeof(double) * (size_t)T * (size_t)B * h->hp.nu); if (rc) return rc; }
  }
  R.has_ref = ref != nullptr; R.has_replay = u_replay != nullptr;
  R.kinds = std::move(kinds);
  R.T = T; R.B = B;
  R.set = true;
  return DGSQP_OK;
}
int dgsqp_fetch_u_cmd(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  const char* none = "no closed-loop launch with drivers has run";
  return h ? side_fetch(h, {{SB_U_CMD, out, sizeof(double)}}, none, none, "u_cmd", capacity_doubles) : DGSQP_E_ARG;
}

int dgsqp_set_plan_hold(dgsqp_handle_t h, const dgsqp_hold_t* hold) {
  { const int rc = setter_begin(h); if (rc) return rc; }
  DgHoldState& S = h->hold;
  if (!hold) { S.set = false; return DGSQP_OK; }
  auto bad = [&](const std::string& m) { return refuse(h, "plan hold: ", m); };
  { const int rc = need_plant(h, "plan hold: "); if (rc) return rc; }
  const int N = h->hp.N;
  if (hold->replan_every < 1 || hold->replan_every > N) return bad("replan_every must be 1 .. N = " + std::to_string(N) + ", got " + std::to_string(hold->replan_every));
  if (hold->on_fail != DGSQP_HOLD_REFERENCE && hold->on_fail != DGSQP_HOLD_HOLD)
    return bad("on_fail must be 0 (reference) or 1 (hold), got " + std::to_string(hold->on_fail));
  if (hold->fail_mask >> 6) return bad("fail_mask has a bit above 5 set (" + std::to_string(hold->fail_mask) + "): the statuses are 0 .. 5");
  S.host = *hold;
  S.set = true;
  return DGSQP_OK;
}
int dgsqp_fetch_plan_hold(dgsqp_handle_t h, double* u_game, int32_t* plan_stage, int64_t capacity_doubles) {
  if (!h) return DGSQP_E_ARG;
  return side_fetch(h, {{SB_U_GAME, u_game, sizeof(double)}, {SB_PLAN_STAGE, plan_stage, sizeof(int32_t)}},
                    "no closed-loop launch with a plan hold has run", "plan hold: null argument", "u_game", capacity_doubles);
}

// Closed-loop batch: B chains of T receding-horizon steps in ONE launch of dg_closed_loop_kernel (dgsqp_closed_loop.h): without an
// argument pack when the handle has no plant, with a DgPlantPack when it has one (every further setting is a field of it), and with a
// DgCrossPack when the plant is a cross plant.
int dgsqp_closed_loop_batch(dgsqp_handle_t h, int64_t B, int32_t T, const double* x0, const double* u_ws, const double* w,
                            double* q_out, double* u_ws_out, double* u_out, double* l_out, double* x_out, int32_t* status,
                            int32_t* iters, int32_t* qp_solves, double* cond, double* cost, int32_t* steps_done, dgsqp_timing_t* tm) {
  if (!h) return DGSQP_E_ARG;
  if (T < 1) { h->err = "closed loop: T must be at least 1"; return DGSQP_E_ARG; }
  if (B < 0) { h->err = "closed loop: B must not be negative"; return DGSQP_E_ARG; }
  if (tm) memset(tm, 0, sizeof(*tm));
  if (B == 0) return DGSQP_OK;
  if (!x0 || !u_ws || !q_out || !u_ws_out || !u_out || !status || !iters || !qp_solves || !cond || !cost || !steps_done) {
    h->err = "closed loop: null argument (only w, l_out, x_out and timing may be NULL)"; return DGSQP_E_ARG;
  }
  const bool cross = h->cross.set;
  { const int rc = further_check_plant(h); if (rc) return rc; }
  { const int rc = drivers_check_launch(h, T, B); if (rc) return rc; }
  { const int rc = hold_check_launch(h); if (rc) return rc; }
  { const int rc = further_check_launch(h, T, B); if (rc) return rc; }
  { const int rc = cross_check_launch(h, B, x0, w); if (rc) return rc; }
  const DgUPrevState& U = h->up;
  if (U.cl_mode && U.cl_B > 0 && U.cl_B != B)
    return refuse(h, "closed-loop u_prev: ", "launch of B = " + std::to_string(B) + " chains, u_prev0 was set for " + std::to_string(U.cl_B));
  HIPCHK(h, hipSetDevice(h->device));
  // Step-major arrays: T x B of every record, one more slice of the state and warm-start chains; c = scenarios per record, keep = the
  // leading ones that are copied in and not filled.  Without x_out one [B][N+1][nq] slice serves every step, without l_out there is no l.
  const int64_t TB = (int64_t)T * B;
  DgRecCount c, keep;
  for (int r = 0; r < DG_REC_COUNT; r++) { c.n[r] = TB; keep.n[r] = 0; }
  c.n[DG_Q] = c.n[DG_UWS] = TB + B; keep.n[DG_Q] = keep.n[DG_UWS] = B;
  c.n[DG_W] = keep.n[DG_W] = w ? TB : 0;
  c.n[DG_L] = l_out ? TB : 0;
  if (!x_out) c.n[DG_X] = keep.n[DG_X] = B;
  c.n[DG_DONE] = B;
  DgRecords& S = h->closed;
  { const int rc = idle_with_ws(h, B); if (rc) return rc; }
  { const int rc = rec_reserve(h, S, c); if (rc) return rc; }
  const int grid = grid_for(h, B);
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  { const int rc = rec_fill(h, S, c, keep); if (rc) return rc; }
  void* host[DG_REC_COUNT] = {};
  host[DG_Q] = (void*)x0; host[DG_UWS] = (void*)u_ws; host[DG_W] = (void*)w;
  { const int rc = rec_copy(h, S, keep, host, hipMemcpyHostToDevice); if (rc) return rc; }
  DgClosedLoop cl;
  cl.T = T; cl.q = S.dbl(DG_Q); cl.uws = S.dbl(DG_UWS); cl.w = w ? S.dbl(DG_W) : nullptr;
  cl.O = S.out(c);
  cl.x_step = x_out ? B * (int64_t)h->rec[DG_X].per : 0;
  cl.steps_done = (int32_t*)S.p[DG_DONE];
  // the carried input: a record [T][B][nu] like u_cmd, slice 0 = u_prev0 (or zeros); without carry every solve reads the handle's zeros
  cl.up = nullptr; cl.up_zero = U.zero;
  h->side.left[SB_U_PREV] = 0;
  if (U.cl_mode) {
    const size_t slice = sizeof(double) * (size_t)B * h->hp.nu;
    { const int rc = side_record(h, SB_U_PREV, TB * h->hp.nu, sizeof(double)); if (rc) return rc; }
    cl.up = h->side.at<double>(SB_U_PREV);
    if (U.cl_B > 0) HIPCHK(h, hipMemcpyAsync(cl.up, U.cl_host.data(), slice, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(h, hipMemsetAsync(cl.up, 0, slice, h->stream));
  }
  DgCrossPack xp{};      // (its DgPlantPack part is the whole pack of a launch with a plant of the game's class)
  if (h->plant.set) {
    { const int rc = plant_for_launch(h, grid, B, TB, &xp); if (rc) return rc; }
    { const int rc = further_for_launch(h, grid, B, TB, &xp); if (rc) return rc; }
    { const int rc = drivers_for_launch(h, grid, B, TB, &xp); if (rc) return rc; }
    { const int rc = hold_for_launch(h, grid, TB, &xp); if (rc) return rc; }
    if (cross) { const int rc = cross_for_launch(h, B, T, &xp); if (rc) return rc; }
  }
  {
    std::unique_lock<std::mutex> game_lock;
    { const int rc = begin_launch(h, game_lock); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(h->ticket, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    if (cross) launch_closed_loop(h, grid, B, cl, xp);
    else if (h->plant.set) launch_closed_loop<DgPlantPack>(h, grid, B, cl, xp);
    else launch_closed_loop(h, grid, B, cl);
    HIPCHK(h, hipGetLastError());
    h->launch_stream = h->stream;
    h->in_flight = true;       // (a launch of another game waits for this kernel before it replaces the constants)
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->in_flight = false;
  rec_host_table(host, u_out, l_out, x_out, status, iters, qp_solves, cond, cost);
  host[DG_Q] = q_out; host[DG_UWS] = u_ws_out; host[DG_DONE] = steps_done;
  { const int rc = rec_copy(h, S, c, host, hipMemcpyDeviceToHost); if (rc) return rc; }
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (tm) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    tm->kernel_ms = ms;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    tm->total_ms = ms;
    tm->grid = grid; tm->block = DG_BLOCK;
  }
  return DGSQP_OK;
}

// fp32 boundary: widen / narrow on the device
__global__ void dg_widen_kernel(int64_t n, const float* __restrict__ src, double* __restrict__ dst) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (double)src[i];
}
__global__ void dg_narrow_kernel(int64_t n, const double* __restrict__ src, float* __restrict__ dst) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}

int dgsqp_solve_batch_f32(dgsqp_handle_t h, int64_t B, const float* x0, const float* u_ws, float* u_out, float* l_out,
                          float* x_out, int32_t* status, int32_t* iters, int32_t* qp_solves, float* cond, float* cost,
                          dgsqp_timing_t* tm) {
  if (!h || B < 0 || (B > 0 && (!x0 || !u_ws))) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  int rc = u_prev_check(h, B);
  if (rc) return rc;
  rc = stage_begin(h, B);
  if (rc) return rc;
  h->B = B;
  if (B == 0) return DGSQP_OK;
  if ((rc = u_prev_stage(h, B))) return rc;          // (u_prev is fp64 also at the fp32 boundary: it is a setting, not one of the call's arrays)
  const DgRecCount c = rec_count_batch(B);
  const DgRecords& S = h->staged;
  size_t big = 0;
  for (int r = 0; r < DG_REC_COUNT; r++) big = std::max(big, (size_t)c.n[r] * h->rec[r].per);
  TmpBuf tb;
  float* f = tb.alloc<float>(big);          // one single-precision staging buffer, reused for every array
  if (!f) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  const float* in[DG_REC_COUNT] = {};
  in[DG_Q] = x0; in[DG_UWS] = u_ws;
  for (int r = 0; r < DG_REC_COUNT; r++) {
    if (!in[r]) continue;
    const size_t cnt = (size_t)c.n[r] * h->rec[r].per;
    HIPCHK(h, hipMemcpyAsync(f, in[r], sizeof(float) * cnt, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(dg_widen_kernel, dim3(256), dim3(256), 0, h->stream, (int64_t)cnt, f, S.dbl(r));
    HIPCHK(h, hipGetLastError());
  }
  dgsqp_timing_t t2;
  rc = dgsqp_solve_staged(h, &t2);
  if (rc) return rc;
  void* dst[DG_REC_COUNT];
  rec_host_table(dst, u_out, l_out, x_out, status, iters, qp_solves, cond, cost);
  for (int r = 0; r < DG_REC_COUNT; r++) {      // the double records are narrowed on the device; the counts are copied as they are
    if (!dst[r] || h->rec[r].elem != sizeof(double)) continue;
    const size_t cnt = (size_t)c.n[r] * h->rec[r].per;
    hipLaunchKernelGGL(dg_narrow_kernel, dim3(256), dim3(256), 0, h->stream, (int64_t)cnt, (const double*)S.dbl(r), f);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(dst[r], f, sizeof(float) * cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));       // f is reused by the next array
    dst[r] = nullptr;
  }
  if ((rc = rec_copy(h, S, c, dst, hipMemcpyDeviceToHost))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (tm) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    *tm = t2;
    tm->total_ms = ms;
  }
  return DGSQP_OK;
}

// Diagnostic build (-DDG_PROF) only: cycles spent on each scenario of the last launch.
int dgsqp_prof_scn(unsigned long long* out, int n) {
#ifdef DG_PROF
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(dg_prof_scn), sizeof(unsigned long long) * (n < 16384 ? n : 16384)) != hipSuccess) return DGSQP_E_DEVICE;
  return 0;
#else
  (void)out; (void)n;
  return -1;
#endif
}

// Diagnostic build (-DDG_PROF) only: read and clear the per-phase cycle counters.
int dgsqp_prof_read(unsigned long long* out, int n) {
#ifdef DG_PROF
  unsigned long long tmp[PH_COUNT * 2];
  if (hipMemcpyFromSymbol(tmp, HIP_SYMBOL(dg_prof), sizeof(tmp)) != hipSuccess) return DGSQP_E_DEVICE;
  for (int i = 0; i < n && i < PH_COUNT * 2; i++) out[i] = tmp[i];
  memset(tmp, 0, sizeof(tmp));
  if (hipMemcpyToSymbol(HIP_SYMBOL(dg_prof), tmp, sizeof(tmp)) != hipSuccess) return DGSQP_E_DEVICE;
  return PH_COUNT;
#else
  (void)out; (void)n;
  return 0;
#endif
}

int dgsqp_set_trace(dgsqp_handle_t h, int pairs_per_scenario) { return h ? log_set(h, h->trace, pairs_per_scenario) : DGSQP_E_ARG; }
int dgsqp_fetch_trace(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  return h ? log_fetch(h, h->trace, out, capacity_doubles, "no trace recorded", "trace buffer too small: need ") : DGSQP_E_ARG;
}
int dgsqp_set_iterate_log(dgsqp_handle_t h, int records_per_scenario) { return h ? log_set(h, h->itlog, records_per_scenario) : DGSQP_E_ARG; }
int dgsqp_fetch_iterate_log(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  return h ? log_fetch(h, h->itlog, out, capacity_doubles, "no iterate log recorded", "iterate-log buffer too small: need ") : DGSQP_E_ARG;
}

// ---- the reference tracker (dgsqp_mpc.h) ----
static void mpc_log_free(dgsqp_solver* h) {
  DgMpcState& S = h->mpc;
  if (S.logD) (void)hipFree(S.logD);
  if (S.logDb) (void)hipFree(S.logDb);
  if (S.loglam) (void)hipFree(S.loglam);
  S.logD = S.logDb = S.loglam = nullptr;
  S.log_B = 0;
}
// Validates the record against the handle's game and lays the tracker out: the row table, the LDS arena behind DgLds.scr and the
// workgroup's scratch.  DGSQP_E_ARG / DGSQP_E_TOO_LARGE with the reason in msg.
static int mpc_plan(const DgProb& D, const dgsqp_mpc_t& c, dg_mpc::DgMpcDev& M, std::vector<dgsqp_mpc_row_t>& rows, std::string& msg) {
  auto bad = [&](const std::string& m) { msg = "mpc: " + m; return DGSQP_E_ARG; };
  if (c.agent < 0 || c.agent >= D.M) return bad("agent " + std::to_string(c.agent) + " is outside the game's 0.." + std::to_string(D.M - 1));
  if (c.N < 1) return bad("N < 1");
  if (c.qp_iters < 1) return bad("qp_iters < 1");
  if (!(c.damping >= 0.0 && c.damping <= 1.0)) return bad("damping outside [0, 1]");
  const int nq = D.nqa[c.agent], nu = DGSQP_NUA;
  if (c.n_soft < 0 || c.n_soft > 1) return bad("n_soft outside 0..1 (with more soft states the reference's rows overwrite one another)");
  for (int j = 0; j < nu; j++) {
    if (!(c.w_du[j] > 0.0) || !std::isfinite(c.w_du[j])) return bad("w_du must be positive for every channel (the QP is solved exactly: it has to be strictly convex)");
    if (!(c.w_u[j] >= 0.0) || !std::isfinite(c.w_u[j])) return bad("w_u must be finite and non-negative");
    if (std::isnan(c.u_ub[j]) || std::isnan(c.u_lb[j]) || std::isnan(c.du_ub[j]) || std::isnan(c.du_lb[j])) return bad("a bound is NaN");
  }
  for (int i = 0; i < nq; i++) {
    if (!(c.w_q[i] >= 0.0) || !std::isfinite(c.w_q[i])) return bad("w_q must be finite and non-negative");
    if (!std::isfinite(c.c_N[i])) return bad("c_N must be finite");
    if (std::isnan(c.q_ub[i]) || std::isnan(c.q_lb[i])) return bad("a bound is NaN");
  }
  for (int i = 0; i < c.n_soft; i++) {
    if (c.soft_idx[i] < 0 || c.soft_idx[i] >= nq) return bad("soft state index out of range");
    if (!(c.soft_quad[i] > 0.0) || !std::isfinite(c.soft_quad[i]) || !(c.soft_lin[i] >= 0.0) || !std::isfinite(c.soft_lin[i])) return bad("soft_quad must be positive and soft_lin non-negative");
    if (!std::isfinite(c.q_ub[c.soft_idx[i]]) || !std::isfinite(c.q_lb[c.soft_idx[i]])) return bad("a soft state needs finite bounds");
  }
  if (!(c.obs_r >= 0.0) || !std::isfinite(c.obs_r)) return bad("obs_r must be finite and non-negative");
  if (c.edge_rows != 0 && c.edge_rows != 1) return bad("edge_rows must be 0 or 1");
  if (c.edge_rows && D.P.n_width < 2) return bad("edge_rows on a handle without a width table (dgsqp_problem_t.widths)");
  if (c.edge_rows && D.mdl[c.agent] == DG_UNI) return bad("edge_rows need an agent with (s, e_y): agent " + std::to_string(c.agent) + " is a unicycle");
  const int64_t n64 = (int64_t)c.N * nu + 2 * c.n_soft;
  if (n64 > DGSQP_MPC_NMAX) { msg = "mpc: N n_u + 2 n_soft = " + std::to_string(n64) + " condensed variables exceed " + std::to_string(DGSQP_MPC_NMAX); return DGSQP_E_TOO_LARGE; }
  memset(&M, 0, sizeof M);
  M.c = c;
  const int N = c.N, n = (int)n64, ns = c.n_soft, nz = nq + nu;
  M.nqa = nq; M.nz = nz; M.n = n; M.ns = ns; M.mdl = D.mdl[c.agent]; M.spl = D.P.track_kind == DGSQP_TRACK_SPLINE;
  M.lenD = (N + 1) * nz + N * nu + 2 * ns;
  M.dt = D.P.dt; M.omd = 1.0 - c.damping;
  // rows: a bound of magnitude >= 1e9 (the reference's 1e10 "none", +-inf) generates none
  rows.clear();
  auto fin = [](double v) { return std::fabs(v) < 1e9; };
  auto is_soft = [&](int i) { for (int s = 0; s < ns; s++) if (c.soft_idx[s] == i) return true; return false; };
  for (int k = 0; k < N; k++)
    for (int j = 0; j < nu; j++) {
      if (fin(c.du_ub[j])) rows.push_back({DGSQP_MPC_ROW_RATE, k, j, 1});
      if (fin(c.du_lb[j])) rows.push_back({DGSQP_MPC_ROW_RATE, k, j, -1});
    }
  for (int i = 0; i < 2 * ns; i++) rows.push_back({DGSQP_MPC_ROW_SLACK, 0, i, -1});
  for (int k = 1; k <= N; k++)
    for (int j = 0; j < nu; j++) {
      if (fin(c.u_ub[j])) rows.push_back({DGSQP_MPC_ROW_INPUT, k, j, 1});
      if (fin(c.u_lb[j])) rows.push_back({DGSQP_MPC_ROW_INPUT, k, j, -1});
    }
  for (int k = 1; k <= N; k++)
    for (int i = 0; i < nq; i++) {
      if (is_soft(i)) continue;
      if (fin(c.q_ub[i])) rows.push_back({DGSQP_MPC_ROW_STATE, k, i, 1});
      if (fin(c.q_lb[i])) rows.push_back({DGSQP_MPC_ROW_STATE, k, i, -1});
    }
  for (int s = 0; s < ns; s++)
    for (int k = 1; k <= N; k++) { rows.push_back({DGSQP_MPC_ROW_SOFT, k, s, 1}); rows.push_back({DGSQP_MPC_ROW_SOFT, k, s, -1}); }
  if (c.obs_r > 0.0) for (int k = 1; k <= N; k++) rows.push_back({DGSQP_MPC_ROW_OBS, k, 0, 1});
  if (c.edge_rows) for (int k = 1; k <= N; k++) { rows.push_back({DGSQP_MPC_ROW_EDGE, k, 0, -1}); rows.push_back({DGSQP_MPC_ROW_EDGE, k, 0, 1}); }   // right, left
  M.nrows = (int)rows.size();
  M.max_steps = 20 * n + 2 * M.nrows + 100;
  // LDS, behind the game's persistent part (the track and atan tables f_c reads)
  int o = D.L.scr;
  auto take = [&](int cnt) { int r = o; o += (cnt + 1) & ~1; return r; };
  M.o_J = take(n * (n + 1) / 2);
  M.o_g = take(n); M.o_y = take(n); M.o_x = take(n); M.o_a = take(n); M.o_d = take(n); M.o_z = take(n); M.o_w = take(n); M.o_r = take(n); M.o_lam = take(n);
  M.o_act = take((n + 2) / 2); M.o_D = take(M.lenD); M.o_Db = take(M.lenD); M.o_P0 = take(nz); M.o_flag = take((M.nrows + 2) / 2);
  M.o_wid = c.edge_rows ? take(4 * N) : o;      // (w_L, w_L', w_R, w_R') per stage 1..N; a record without edge rows keeps its arena
  M.o_end = o;
  if ((long)o * 8 > DG_LDS_LIMIT) {
    msg = "mpc: the tracker needs " + std::to_string((long)o * 8) + " B of LDS per workgroup (limit " + std::to_string(DG_LDS_LIMIT) + "): N=" + std::to_string(N) + " n=" + std::to_string(n);
    return DGSQP_E_TOO_LARGE;
  }
  int64_t w = 0;
  auto wtake = [&](int64_t cnt) { int64_t r = w; w += (cnt + 31) / 32 * 32; return r; };
  M.ws_AB = wtake((int64_t)N * nq * nz); M.ws_f = wtake((int64_t)N * nq); M.ws_gk = wtake((int64_t)N * nq); M.ws_qbar = wtake((int64_t)(N + 1) * nq);
  M.ws_S = wtake((int64_t)N * nq * n); M.ws_Qm = wtake((int64_t)n * n); M.ws_Ri = wtake((int64_t)n * n);
  M.ws_doubles = w;
  return DGSQP_OK;
}

int dgsqp_set_mpc(dgsqp_handle_t h, const dgsqp_mpc_t* mpc) {
  if (!h) return DGSQP_E_ARG;
  if (!mpc) { h->mpc.set = false; h->mpc.rows.clear(); return DGSQP_OK; }
  dg_mpc::DgMpcDev M;
  std::vector<dgsqp_mpc_row_t> rows;
  std::string msg;
  const int rc = mpc_plan(h->hp, *mpc, M, rows, msg);
  if (rc) { h->err = msg; return rc; }
  h->mpc.dev = M;
  h->mpc.rows.swap(rows);
  h->mpc.set = true;
  return DGSQP_OK;
}

int dgsqp_mpc_dims(dgsqp_handle_t h, dgsqp_mpc_dims_t* out, dgsqp_mpc_row_t* rows, int64_t row_capacity) {
  if (!h || !out) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  if (!h->mpc.set) { h->err = "mpc: no tracker set (dgsqp_set_mpc)"; return DGSQP_E_ARG; }
  const dg_mpc::DgMpcDev& M = h->mpc.dev;
  memset(out, 0, sizeof *out);
  out->n = M.n; out->n_rows = M.nrows; out->len_D = M.lenD; out->n_q = M.nqa; out->lds_bytes = M.o_end * 8;
  out->workspace_bytes = M.ws_doubles * (int64_t)sizeof(double);
  if (rows) {
    if (row_capacity < M.nrows) { h->err = "mpc: row table too small: need " + std::to_string(M.nrows); return DGSQP_E_ARG; }
    memcpy(rows, h->mpc.rows.data(), sizeof(dgsqp_mpc_row_t) * (size_t)M.nrows);
  }
  return DGSQP_OK;
}

int dgsqp_set_mpc_log(dgsqp_handle_t h, int on) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  h->mpc.log_on = on != 0;
  mpc_log_free(h);
  return DGSQP_OK;
}

int dgsqp_fetch_mpc_log(dgsqp_handle_t h, double* D, double* D_bar, double* lam, int64_t capacity) {
  if (!h) return DGSQP_E_ARG;
  DgMpcState& S = h->mpc;
  if (!S.logD || S.log_B <= 0) { h->err = "mpc: no log recorded"; return DGSQP_E_ARG; }
  if (capacity < S.log_B) { h->err = "mpc: log buffers too small: need " + std::to_string(S.log_B) + " scenarios"; return DGSQP_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nd = (size_t)S.log_B * S.log_iters * S.log_lenD, nl = (size_t)S.log_B * S.log_iters * S.log_rows;
  if (D) HIPCHK(h, hipMemcpy(D, S.logD, sizeof(double) * nd, hipMemcpyDeviceToHost));
  if (D_bar) HIPCHK(h, hipMemcpy(D_bar, S.logDb, sizeof(double) * nd, hipMemcpyDeviceToHost));
  if (lam && nl) HIPCHK(h, hipMemcpy(lam, S.loglam, sizeof(double) * nl, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

// The tracker's launch path from device-resident buffers: dgsqp_mpc_batch between its copies in and its copies out, and the warm-start
// program of dgsqp_raceline_warm_start_batch.  M carries every device pointer but `rows`.
//   mpc_upload         the row table and the record to the device (drows, dM: the caller's), host-synchronous
//   mpc_lds_attribute  the kernel's dynamic LDS size, once before the launches of a record's layout
//   mpc_enqueue        dg_mpc_kernel on h->stream: inside run_sync's critical section (the kernel reads dg_prob)
static int mpc_grid(const dgsqp_solver* h, int64_t B) {
  const int grid = (int)std::min<int64_t>(B, (int64_t)h->num_cu * DG_WG_PER_CU);
  return grid < 1 ? 1 : grid;
}
static int mpc_upload(dgsqp_solver* h, dg_mpc::DgMpcDev& M, const std::vector<dgsqp_mpc_row_t>& rows, dgsqp_mpc_row_t* drows, dg_mpc::DgMpcDev* dM) {
  if (M.nrows) HIPCHK(h, hipMemcpy(drows, rows.data(), sizeof(dgsqp_mpc_row_t) * (size_t)M.nrows, hipMemcpyHostToDevice));
  M.rows = drows;
  HIPCHK(h, hipMemcpy(dM, &M, sizeof M, hipMemcpyHostToDevice));
  return DGSQP_OK;
}
static int mpc_lds_attribute(dgsqp_solver* h, const dg_mpc::DgMpcDev& M) {
  if (hipFuncSetAttribute((const void*)dg_mpc::dg_mpc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)M.o_end * sizeof(double))) != hipSuccess) {
    h->err = "hipFuncSetAttribute(dynamic LDS) failed for the tracker";
    return DGSQP_E_DEVICE;
  }
  return DGSQP_OK;
}
static int mpc_enqueue(dgsqp_solver* h, const dg_mpc::DgMpcDev& M, const dg_mpc::DgMpcDev* dM, int64_t B, int grid) {
  hipLaunchKernelGGL(dg_mpc::dg_mpc_kernel, dim3(grid), dim3(DG_BLOCK), (size_t)M.o_end * sizeof(double), h->stream, B, dM);
  HIPCHK(h, hipGetLastError());
  return DGSQP_OK;
}

int dgsqp_mpc_batch(dgsqp_handle_t h, int64_t B, const double* q0, const double* u_ws, const double* du_ws, const double* q_ref,
                    const double* p_obs, double* q_pred, double* u_pred, double* du_pred, int32_t* status, int32_t* qp_steps,
                    dgsqp_timing_t* timing) {
  if (!h) return DGSQP_E_ARG;
  if (!h->mpc.set) { h->err = "mpc: no tracker set (dgsqp_set_mpc)"; return DGSQP_E_ARG; }
  if (B < 0 || !q0 || !u_ws || !du_ws || !q_ref) { h->err = "mpc: bad argument"; return DGSQP_E_ARG; }
  dg_mpc::DgMpcDev M = h->mpc.dev;
  if (M.c.obs_r > 0.0 && !p_obs) { h->err = "mpc: obs_r > 0 needs p_obs"; return DGSQP_E_ARG; }
  if (timing) memset(timing, 0, sizeof *timing);
  if (B == 0) return DGSQP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  const int N = M.c.N, nq = M.nqa, nu = DGSQP_NUA;
  const auto t0 = std::chrono::steady_clock::now();
  const int grid = mpc_grid(h, B);
  TmpBuf tb;
  const size_t nQ0 = (size_t)B * nq, nU = (size_t)B * (N + 1) * nu, nDU = (size_t)B * N * nu, nQ = (size_t)B * (N + 1) * nq, nP = (size_t)B * N * 2;
  double* dq0 = tb.alloc<double>(nQ0); double* duw = tb.alloc<double>(nU); double* ddu = tb.alloc<double>(nDU); double* dqr = tb.alloc<double>(nQ);
  double* dpo = M.c.obs_r > 0.0 ? tb.alloc<double>(nP) : nullptr;
  double* oq = tb.alloc<double>(nQ); double* ou = tb.alloc<double>(nDU); double* od = tb.alloc<double>(nDU);
  int32_t* ost = tb.alloc<int32_t>(B); int32_t* osp = tb.alloc<int32_t>(B);
  double* ws = tb.alloc<double>((size_t)grid * M.ws_doubles);
  dgsqp_mpc_row_t* drows = tb.alloc<dgsqp_mpc_row_t>(M.nrows);
  dg_mpc::DgMpcDev* dM = tb.alloc<dg_mpc::DgMpcDev>(1);
  if (!dq0 || !duw || !ddu || !dqr || (M.c.obs_r > 0.0 && !dpo) || !oq || !ou || !od || !ost || !osp || !ws || !drows || !dM) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  DgMpcState& S = h->mpc;
  if (S.log_on) {
    mpc_log_free(h);
    const size_t nd = (size_t)B * M.c.qp_iters * M.lenD, nl = (size_t)B * M.c.qp_iters * (M.nrows ? M.nrows : 1);
    HIPCHK(h, hipMalloc(&S.logD, sizeof(double) * nd));
    HIPCHK(h, hipMalloc(&S.logDb, sizeof(double) * nd));
    HIPCHK(h, hipMalloc(&S.loglam, sizeof(double) * nl));
    S.log_B = B; S.log_iters = M.c.qp_iters; S.log_lenD = M.lenD; S.log_rows = M.nrows;
  }
  HIPCHK(h, hipMemcpy(dq0, q0, sizeof(double) * nQ0, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(duw, u_ws, sizeof(double) * nU, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(ddu, du_ws, sizeof(double) * nDU, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dqr, q_ref, sizeof(double) * nQ, hipMemcpyHostToDevice));
  if (dpo) HIPCHK(h, hipMemcpy(dpo, p_obs, sizeof(double) * nP, hipMemcpyHostToDevice));
  M.q0 = dq0; M.u_ws = duw; M.du_ws = ddu; M.q_ref = dqr; M.p_obs = dpo;
  M.q_pred = oq; M.u_pred = ou; M.du_pred = od; M.status = ost; M.qp_steps = osp; M.ws = ws;
  M.logD = S.log_on ? S.logD : nullptr; M.logDb = S.log_on ? S.logDb : nullptr; M.loglam = S.log_on ? S.loglam : nullptr;
  { const int rcu = mpc_upload(h, M, S.rows, drows, dM); if (rcu) return rcu; }
  const auto t1 = std::chrono::steady_clock::now();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(h, hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); h->err = "hipEventCreate failed"; return DGSQP_E_DEVICE; }
  int rc = mpc_lds_attribute(h, M);
  if (rc) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return rc; }
  rc = run_sync(h, [&]() -> int {
    HIPCHK(h, hipEventRecord(e0, h->stream));
    { const int rce = mpc_enqueue(h, M, dM, B, grid); if (rce) return rce; }
    HIPCHK(h, hipEventRecord(e1, h->stream));
    return DGSQP_OK;
  });
  float ms = 0.0f;
  if (!rc && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) ms = 0.0f;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (rc) return rc;
  const auto t2 = std::chrono::steady_clock::now();
  if (q_pred) HIPCHK(h, hipMemcpy(q_pred, oq, sizeof(double) * nQ, hipMemcpyDeviceToHost));
  if (u_pred) HIPCHK(h, hipMemcpy(u_pred, ou, sizeof(double) * nDU, hipMemcpyDeviceToHost));
  if (du_pred) HIPCHK(h, hipMemcpy(du_pred, od, sizeof(double) * nDU, hipMemcpyDeviceToHost));
  if (status) HIPCHK(h, hipMemcpy(status, ost, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  if (qp_steps) HIPCHK(h, hipMemcpy(qp_steps, osp, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  const auto t3 = std::chrono::steady_clock::now();
  if (timing) {
    auto msd = [](auto a, auto b_) { return std::chrono::duration<double, std::milli>(b_ - a).count(); };
    timing->h2d_ms = msd(t0, t1); timing->kernel_ms = ms; timing->d2h_ms = msd(t2, t3); timing->total_ms = msd(t0, t3);
    timing->grid = grid; timing->block = DG_BLOCK;
  }
  return DGSQP_OK;
}

int dgsqp_synchronize(dgsqp_handle_t h) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  // A member of a grouped launch is solved on its LEADER's stream: wait for that kernel first (and leave the group), then for
  // whatever is queued on the handle's own stream (copies, the stats gather).
  { const int rc = wait_idle(h); if (rc) return rc; }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DGSQP_OK;
}

int dgsqp_evaluate_batch(dgsqp_handle_t h, int64_t B, const double* x0, const double* u, const double* l, double* q,
                         double* g, double* G, double* Q, double* x, double* l0) {
  if (!h || B < 0 || !x0 || !u) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  if (B == 0) return DGSQP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const DgProb& D = h->hp;
  const int grid = grid_for(h, B);
  int rc = u_prev_check(h, B);
  if (rc) return rc;
  rc = idle_with_ws(h, B);
  if (rc) return rc;
  TmpBuf tb;
  const double* dup = nullptr; int64_t up_stride = 0;
  if ((rc = u_prev_hook(h, B, tb, &dup, &up_stride))) return rc;
  const size_t n = D.n, nc = D.nc, nx = (size_t)(D.N + 1) * D.nq;
  double* dx0 = tb.alloc<double>(B * D.nq); double* du = tb.alloc<double>(B * n);
  double* dl = l ? tb.alloc<double>(B * nc) : nullptr;
  double* dq = q ? tb.alloc<double>(B * n) : nullptr; double* dg = g ? tb.alloc<double>(B * nc) : nullptr;
  double* dG = G ? tb.alloc<double>(B * nc * n) : nullptr; double* dQ = Q ? tb.alloc<double>(B * n * n) : nullptr;
  double* dx = x ? tb.alloc<double>(B * nx) : nullptr; double* dl0 = l0 ? tb.alloc<double>(B * nc) : nullptr;
  if (!dx0 || !du || (l && !dl) || (q && !dq) || (g && !dg) || (G && !dG) || (Q && !dQ) || (x && !dx) || (l0 && !dl0)) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(dx0, x0, sizeof(double) * B * D.nq, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(du, u, sizeof(double) * B * n, hipMemcpyHostToDevice));
  if (l) HIPCHK(h, hipMemcpy(dl, l, sizeof(double) * B * nc, hipMemcpyHostToDevice));
  rc = run_sync(h, [&]() -> int {
    hipLaunchKernelGGL(dg_evaluate_kernel, dim3(grid), dim3(DG_BLOCK), h->lds_bytes, h->stream, h->dp, B, dx0, du, dl, dq, dg, dG, dQ, dx, dl0, h->ws, dup, up_stride);
    HIPCHK(h, hipGetLastError());
    return DGSQP_OK;
  });
  if (rc) return rc;
  if (q) HIPCHK(h, hipMemcpy(q, dq, sizeof(double) * B * n, hipMemcpyDeviceToHost));
  if (g) HIPCHK(h, hipMemcpy(g, dg, sizeof(double) * B * nc, hipMemcpyDeviceToHost));
  if (G) HIPCHK(h, hipMemcpy(G, dG, sizeof(double) * B * nc * n, hipMemcpyDeviceToHost));
  if (Q) HIPCHK(h, hipMemcpy(Q, dQ, sizeof(double) * B * n * n, hipMemcpyDeviceToHost));
  if (x) HIPCHK(h, hipMemcpy(x, dx, sizeof(double) * B * nx, hipMemcpyDeviceToHost));
  if (l0) HIPCHK(h, hipMemcpy(l0, dl0, sizeof(double) * B * nc, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

int dgsqp_pid_warm_start_batch(dgsqp_handle_t h, int64_t B, const double* q0, const dgsqp_pid_t* pid, double* u_ws,
                               double* q_ws, int32_t* collide) {
  if (!h || B < 0 || !q0 || !pid || !u_ws || pid->substeps < 1) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  if (B == 0) return DGSQP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const DgProb& D = h->hp;
  for (int a = 0; a < D.M; a++)
    if (D.mdl[a] == DG_UNI) { h->err = "the PID lane follower needs a Frenet-frame model (the merge script starts from zero inputs)"; return DGSQP_E_ARG; }
  TmpBuf tb;
  const size_t nx = (size_t)(D.N + 1) * D.nq;
  double* dq0 = tb.alloc<double>(B * D.nq); double* du = tb.alloc<double>(B * D.n);
  double* dq = (q_ws || collide) ? tb.alloc<double>(B * nx) : nullptr;
  int32_t* dc = collide ? tb.alloc<int32_t>(B) : nullptr;
  if (!dq0 || !du || ((q_ws || collide) && !dq) || (collide && !dc)) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(dq0, q0, sizeof(double) * B * D.nq, hipMemcpyHostToDevice));
  const int64_t lanes = B * D.M;
  int grid = (int)((lanes + DG_BLOCK - 1) / DG_BLOCK);
  if (grid > 4 * h->num_cu) grid = 4 * h->num_cu;
  const int rc = run_sync(h, [&]() -> int {
    hipLaunchKernelGGL(dg_pid_kernel, dim3(grid), dim3(DG_BLOCK), (size_t)D.L.scr * sizeof(double), h->stream, B, dq0, *pid, du, dq);
    HIPCHK(h, hipGetLastError());
    if (collide) {
      hipLaunchKernelGGL(dg_collide_kernel, dim3((int)((B + 255) / 256)), dim3(256), 0, h->stream, B, dq, dc);
      HIPCHK(h, hipGetLastError());
    }
    return DGSQP_OK;
  });
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(u_ws, du, sizeof(double) * B * D.n, hipMemcpyDeviceToHost));
  if (q_ws) HIPCHK(h, hipMemcpy(q_ws, dq, sizeof(double) * B * nx, hipMemcpyDeviceToHost));
  if (collide) HIPCHK(h, hipMemcpy(collide, dc, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

int dgsqp_sample_batch(dgsqp_handle_t h, int64_t B, const dgsqp_sampler_t* spec, const dgsqp_pid_t* pid, double* x0_out,
                       double* u_ws_out, int64_t* candidates, int stage) {
  if (!h || B < 0 || !spec || spec->kind < 0 || spec->kind > DGSQP_SAMPLER_MERGE) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  const DgProb& D = h->hp;
  const bool merge = spec->kind == DGSQP_SAMPLER_MERGE;
  // n_key = 0 on a spline-track handle: the cars are placed on the handle's spline (dg_sample_place_spline_kernel)
  const bool on_spline = !merge && spec->n_key == 0 && D.P.track_kind == DGSQP_TRACK_SPLINE;
  if (on_spline && spec->kind != DGSQP_SAMPLER_CIRCUIT) { h->err = "sampler: a spline track takes the circuit sampler only (first_segment / independent need seg0_len, the first segment of an arc track)"; return DGSQP_E_ARG; }
  if (!merge && (!pid || pid->substeps < 1 || (!on_spline && (spec->n_key < 2 || spec->n_key > DGSQP_MAX_SEGS + 1)))) { h->err = "bad sampler description"; return DGSQP_E_ARG; }
  if (spec->kind == DGSQP_SAMPLER_FIRST_SEGMENT && D.M != 2) { h->err = "the first-segment sampler places two cars"; return DGSQP_E_ARG; }
  for (int a = 0; a < D.M; a++)
    if ((D.mdl[a] == DG_UNI) != merge) { h->err = "sampler and vehicle model do not fit (merge: unicycles; the others: Frenet-frame models)"; return DGSQP_E_ARG; }
  if (candidates) *candidates = 0;
  if (B == 0) return DGSQP_OK;
  { const int rc = stage_begin(h, B); if (rc) return rc; }
  double *const d_x0 = h->staged.dbl(DG_Q), *const d_uws = h->staged.dbl(DG_UWS);
  const int64_t nround = std::max<int64_t>(256, std::min<int64_t>(2 * B, 1 << 16));        // candidates per round
  const size_t nx = (size_t)(D.N + 1) * D.nq;
  TmpBuf tb;
  double* dq0 = tb.alloc<double>(nround * D.nq); double* du = tb.alloc<double>(nround * D.n); double* dq = tb.alloc<double>(nround * nx);
  int32_t* dok = tb.alloc<int32_t>(nround); int32_t* dcol = tb.alloc<int32_t>(nround); int32_t* dpos = tb.alloc<int32_t>(nround); int32_t* dcnt = tb.alloc<int32_t>(1);
  if (!dq0 || !du || !dq || !dok || !dcol || !dpos || !dcnt) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  // (the rounds belong together: one critical section around all of them)
  const int rcs = run_sync(h, [&]() -> int {
    int64_t have = 0;
    unsigned long long c0 = 0;
    for (int round = 0; have < B; round++) {
      if (round > 10000) { h->err = "sampler did not produce enough collision-free scenarios"; return DGSQP_E_ARG; }
      if (on_spline) hipLaunchKernelGGL(dg_sample_place_spline_kernel, dim3((unsigned)((nround + 255) / 256)), dim3(256), 0, h->stream, nround, c0, *spec, dq0, dok);
      else hipLaunchKernelGGL(dg_sample_place_kernel, dim3((unsigned)((nround + 255) / 256)), dim3(256), 0, h->stream, nround, c0, *spec, dq0, dok);
      HIPCHK(h, hipGetLastError());
      if (merge) {
        hipLaunchKernelGGL(dg_sample_zero_rollout_kernel, dim3((unsigned)((nround * D.M + 255) / 256)), dim3(256), 0, h->stream, nround, dq0, dq);
      } else {
        int grid = (int)((nround * D.M + DG_BLOCK - 1) / DG_BLOCK);
        if (grid > 4 * h->num_cu) grid = 4 * h->num_cu;
        hipLaunchKernelGGL(dg_pid_kernel, dim3(grid), dim3(DG_BLOCK), (size_t)D.L.scr * sizeof(double), h->stream, nround, dq0, *pid, du, dq);
      }
      HIPCHK(h, hipGetLastError());
      hipLaunchKernelGGL(dg_collide_kernel, dim3((unsigned)((nround + 255) / 256)), dim3(256), 0, h->stream, nround, dq, dcol);
      hipLaunchKernelGGL(dg_sample_scan_kernel, dim3(1), dim3(1024), 0, h->stream, nround, dok, dcol, dpos, dcnt);
      hipLaunchKernelGGL(dg_sample_gather_kernel, dim3(1024), dim3(128), 0, h->stream, nround, have, B, dpos, dq0, merge ? (const double*)nullptr : du, d_x0, d_uws);
      HIPCHK(h, hipGetLastError());
      int32_t cnt = 0;
      HIPCHK(h, hipMemcpyAsync(&cnt, dcnt, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (have + cnt >= B && candidates) {
        // index after the (B - have)-th accepted candidate of this round
        std::vector<int32_t> pos((size_t)nround);
        HIPCHK(h, hipMemcpy(pos.data(), dpos, sizeof(int32_t) * nround, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < nround; i++) if (pos[i] == (int32_t)(B - have - 1)) { *candidates = (int64_t)(c0 + i + 1); break; }
      }
      have += cnt;
      c0 += (unsigned long long)nround;
    }
    return DGSQP_OK;
  });
  if (rcs) return rcs;
  if (x0_out) HIPCHK(h, hipMemcpy(x0_out, d_x0, sizeof(double) * B * D.nq, hipMemcpyDeviceToHost));
  if (u_ws_out) HIPCHK(h, hipMemcpy(u_ws_out, d_uws, sizeof(double) * B * D.n, hipMemcpyDeviceToHost));
  h->B = stage ? B : 0;          // (the staging buffers were used either way: without `stage` nothing is left staged)
  return DGSQP_OK;
}

// ---- raceline warm starts (dgsqp_raceline.h) ----
int dgsqp_set_raceline(dgsqp_handle_t h, int64_t n, const double* T, const double* cols) {
  if (!h) return DGSQP_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  DgRacelineState& S = h->rl;
  if (T && cols) {
    if (n < 2 || n > (1 << 30)) return refuse(h, "raceline: ", "n = " + std::to_string(n) + " knots (at least 2)");
    int64_t bad = first_non_finite(T, n);
    if (bad >= 0) return refuse(h, "raceline: ", "T[" + std::to_string(bad) + "] is not finite");
    bad = first_non_finite(cols, n * DGSQP_RL_COLS);
    if (bad >= 0) return refuse(h, "raceline: ", "entry [" + std::to_string(bad / DGSQP_RL_COLS) + "][" + std::to_string(bad % DGSQP_RL_COLS) + "] is not finite");
    for (int64_t i = 1; i < n; i++) {
      if (!(T[i] > T[i - 1])) return refuse(h, "raceline: ", "T is not strictly increasing at knot " + std::to_string(i));
      if (!(cols[i * DGSQP_RL_COLS + 7] > cols[(i - 1) * DGSQP_RL_COLS + 7])) return refuse(h, "raceline: ", "the s column is not strictly increasing at knot " + std::to_string(i));
    }
  }
  if (S.T) (void)hipFree(S.T);
  if (S.cols) (void)hipFree(S.cols);
  S.T = S.cols = nullptr;
  S.dev = DgRaceline{0, nullptr, nullptr};
  if (!T || !cols) return DGSQP_OK;
  HIPCHK(h, hipMalloc(&S.T, sizeof(double) * (size_t)n));
  HIPCHK(h, hipMalloc(&S.cols, sizeof(double) * (size_t)n * DGSQP_RL_COLS));
  HIPCHK(h, hipMemcpy(S.T, T, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(S.cols, cols, sizeof(double) * (size_t)n * DGSQP_RL_COLS, hipMemcpyHostToDevice));
  S.dev = DgRaceline{(int)n, S.T, S.cols};
  return DGSQP_OK;
}

// The warm-start program for `cap` scenarios at a time: the two records of every agent planned and uploaded, the buffers between the
// launches.  Everything is sized for cap scenarios; enqueue() may run for any B <= cap.
struct DgRacelineProgram {
  int64_t cap = 0;
  int grid = 1;
  dg_mpc::DgMpcDev rec[DGSQP_MAX_AGENTS][2];              // host images, device pointers filled
  dg_mpc::DgMpcDev* drec = nullptr;                       // device [M][2]
  double *q0a = nullptr, *u1 = nullptr, *du1 = nullptr, *u2 = nullptr, *du2 = nullptr, *up1 = nullptr, *dup1 = nullptr, *up2 = nullptr;
  int32_t* st2 = nullptr;
  double u_init = 0.0, du_init = 0.0;
};
static int raceline_check(dgsqp_solver* h, const dgsqp_raceline_ws_t* W) {
  const DgProb& D = h->hp;
  if (!W) return refuse(h, "raceline: ", "no warm-start description");
  if (h->rl.dev.n < 2) return refuse(h, "raceline: ", "no raceline set (dgsqp_set_raceline)");
  for (int a = 0; a < D.M; a++) {
    if (D.mdl[a] != DG_KIN && D.mdl[a] != DG_DYN) return refuse(h, "raceline: ", "agent " + std::to_string(a) + " is no Frenet-frame bicycle (the reference states are laid out for the kinematic and the dynamic bicycle)");
    if (D.mdl[a] != D.mdl[0]) return refuse(h, "raceline: ", "agents of different models");
  }
  if (W->init_iters < 1) return refuse(h, "raceline: ", "init_iters < 1");
  if (!std::isfinite(W->u_init) || !std::isfinite(W->du_init)) return refuse(h, "raceline: ", "u_init / du_init is not finite");
  return DGSQP_OK;
}
static int raceline_program(dgsqp_solver* h, const dgsqp_raceline_ws_t& W, int64_t cap, TmpBuf& tb, DgRacelineProgram& P) {
  const DgProb& D = h->hp;
  const int N = W.mpc.N, nu = DGSQP_NUA, nqa = D.nqa[0];
  if (N != D.N) return refuse(h, "raceline: ", "the tracker's N = " + std::to_string(N) + " is not the game's N = " + std::to_string(D.N) + " (its u_pred becomes the game's warm start)");
  P.cap = cap; P.grid = mpc_grid(h, cap); P.u_init = W.u_init; P.du_init = W.du_init;
  DgRacelineState& S = h->rl;
  const size_t need = (size_t)D.M * cap * (N + 1) * nqa;
  if (S.qref_cap < need) {
    if (S.qref) (void)hipFree(S.qref);
    S.qref = nullptr; S.qref_cap = 0; S.ref_B = 0;
    HIPCHK(h, hipMalloc(&S.qref, sizeof(double) * need));
    S.qref_cap = need;
  }
  const size_t nU = (size_t)cap * (N + 1) * nu, nDU = (size_t)cap * N * nu;
  P.q0a = tb.alloc<double>((size_t)D.M * cap * nqa);
  P.u1 = tb.alloc<double>(nU); P.du1 = tb.alloc<double>(nDU); P.u2 = tb.alloc<double>(nU); P.du2 = tb.alloc<double>(nDU);
  P.up1 = tb.alloc<double>(nDU); P.dup1 = tb.alloc<double>(nDU); P.up2 = tb.alloc<double>(nDU);
  P.st2 = tb.alloc<int32_t>(cap);
  P.drec = tb.alloc<dg_mpc::DgMpcDev>((size_t)D.M * 2);
  if (!P.q0a || !P.u1 || !P.du1 || !P.u2 || !P.du2 || !P.up1 || !P.dup1 || !P.up2 || !P.st2 || !P.drec) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  double* ws = nullptr;
  for (int a = 0; a < D.M; a++) {
    std::vector<dgsqp_mpc_row_t> rows;
    for (int ph = 0; ph < 2; ph++) {
      dgsqp_mpc_t c = W.mpc;
      c.agent = a;
      c.zero_du = ph == 0 ? 1 : 0;
      if (ph == 0) { c.qp_iters = W.init_iters; c.damping = W.init_damping; }
      dg_mpc::DgMpcDev& M = P.rec[a][ph];
      std::string msg;
      const int rc = mpc_plan(D, c, M, rows, msg);
      if (rc) { h->err = msg; return rc; }
      if (c.obs_r > 0.0) return refuse(h, "raceline: ", "obstacle rows are not part of the warm-start program (obs_r must be 0)");
      if (!ws) { ws = tb.alloc<double>((size_t)P.grid * M.ws_doubles); if (!ws) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; } }
      dgsqp_mpc_row_t* drows = tb.alloc<dgsqp_mpc_row_t>(M.nrows);
      if (!drows) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
      M.q0 = P.q0a + (size_t)a * cap * nqa;
      M.q_ref = S.qref + (size_t)a * cap * (N + 1) * nqa;
      M.p_obs = nullptr; M.q_pred = nullptr; M.qp_steps = nullptr; M.ws = ws;
      M.logD = M.logDb = M.loglam = nullptr;
      if (ph == 0) { M.u_ws = P.u1; M.du_ws = P.du1; M.u_pred = P.up1; M.du_pred = P.dup1; M.status = nullptr; }
      else { M.u_ws = P.u2; M.du_ws = P.du2; M.u_pred = P.up2; M.du_pred = nullptr; M.status = P.st2; }
      const int rcu = mpc_upload(h, M, rows, drows, P.drec + a * 2 + ph);
      if (rcu) return rcu;
    }
  }
  return mpc_lds_attribute(h, P.rec[0][1]);
}
// The program for B <= cap scenarios whose joint states are at d_x0 [B][n_q] (device): on h->stream, inside run_sync's critical section.
// d_u [B][n] agent-major and d_ok [B] receive the result.  The buffers are laid out for cap scenarios, so B must equal cap wherever an
// agent's block follows another's (q0a, q_ref): the callers run it with B == cap.
static int raceline_enqueue(dgsqp_solver* h, const DgRacelineProgram& P, int64_t B, const double* d_x0, double* d_u, int32_t* d_ok) {
  const DgProb& D = h->hp;
  const int N = D.N;
  auto blocks = [&](int64_t lanes) { return dim3((unsigned)std::min<int64_t>((lanes + 255) / 256, 4 * (int64_t)h->num_cu)); };
  hipLaunchKernelGGL(dg_raceline_ref_kernel, blocks(B * D.M * (N + 1)), dim3(256), 0, h->stream, B, h->rl.dev, d_x0, P.u_init, P.du_init,
                     P.q0a, h->rl.qref, P.u1, P.du1);
  HIPCHK(h, hipGetLastError());
  for (int a = 0; a < D.M; a++) {
    int rc = mpc_enqueue(h, P.rec[a][0], P.drec + a * 2, B, P.grid);
    if (rc) return rc;
    hipLaunchKernelGGL(dg_ws_chain_kernel, blocks(B * (N + 1) * DGSQP_NUA), dim3(256), 0, h->stream, B, N, (const double*)P.u1, (const double*)P.up1,
                       (const double*)P.dup1, P.u2, P.du2);
    HIPCHK(h, hipGetLastError());
    rc = mpc_enqueue(h, P.rec[a][1], P.drec + a * 2 + 1, B, P.grid);
    if (rc) return rc;
    hipLaunchKernelGGL(dg_ws_assemble_kernel, blocks(B * N * DGSQP_NUA), dim3(256), 0, h->stream, B, N, D.n, a, (const double*)P.up2,
                       (const int32_t*)P.st2, d_u, d_ok);
    HIPCHK(h, hipGetLastError());
  }
  h->rl.ref_B = B;
  return DGSQP_OK;
}

int dgsqp_raceline_warm_start_batch(dgsqp_handle_t h, int64_t B, const double* x0, const dgsqp_raceline_ws_t* W, double* u_ws_out,
                                    int32_t* ok_out) {
  if (!h) return DGSQP_E_ARG;
  if (B < 0) return refuse(h, "raceline: ", "B < 0");
  { const int rc = raceline_check(h, W); if (rc) return rc; }
  if (!x0 && h->B != B) return refuse(h, "raceline: ", "x0 = NULL needs a staged batch of B = " + std::to_string(B) + " scenarios (staged: " + std::to_string(h->B) + ")");
  if (B == 0) return DGSQP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  const DgProb& D = h->hp;
  TmpBuf tb;
  DgRacelineProgram P;
  { const int rc = raceline_program(h, *W, B, tb, P); if (rc) return rc; }
  const double* d_x0 = nullptr;
  double* d_u = nullptr;
  if (x0) {
    double* dx = tb.alloc<double>((size_t)B * D.nq);
    d_u = tb.alloc<double>((size_t)B * D.n);
    if (!dx || !d_u) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
    HIPCHK(h, hipMemcpy(dx, x0, sizeof(double) * (size_t)B * D.nq, hipMemcpyHostToDevice));
    d_x0 = dx;
  } else {
    d_x0 = h->staged.dbl(DG_Q);
    d_u = h->staged.dbl(DG_UWS);
  }
  int32_t* d_ok = tb.alloc<int32_t>(B);
  if (!d_ok) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  const int rc = run_sync(h, [&]() -> int { return raceline_enqueue(h, P, B, d_x0, d_u, d_ok); });
  if (rc) return rc;
  if (u_ws_out) HIPCHK(h, hipMemcpy(u_ws_out, d_u, sizeof(double) * (size_t)B * D.n, hipMemcpyDeviceToHost));
  if (ok_out) HIPCHK(h, hipMemcpy(ok_out, d_ok, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

int dgsqp_fetch_raceline_ref(dgsqp_handle_t h, double* out, int64_t capacity_doubles) {
  if (!h) return DGSQP_E_ARG;
  const DgProb& D = h->hp;
  DgRacelineState& S = h->rl;
  if (!S.qref || S.ref_B <= 0) return refuse(h, "raceline: ", "no reference trajectories recorded");
  const int nqa = D.nqa[0];
  const int64_t per = (int64_t)(D.N + 1) * nqa, B = S.ref_B, total = B * D.M * per;
  if (!out || capacity_doubles < total) return refuse(h, "raceline: ", "reference buffer too small: need " + std::to_string(total) + " doubles");
  HIPCHK(h, hipSetDevice(h->device));
  // device [M][B][..] (an agent's block is what the tracker reads) -> the caller's [B][M][..]
  std::vector<double> tmp((size_t)total);
  HIPCHK(h, hipMemcpy(tmp.data(), S.qref, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost));
  for (int a = 0; a < D.M; a++)
    for (int64_t b = 0; b < B; b++)
      memcpy(out + (b * D.M + a) * per, tmp.data() + ((int64_t)a * B + b) * per, sizeof(double) * (size_t)per);
  return DGSQP_OK;
}

// The rounds the two raceline samplers share: `place(nround, c0, dq0, dcol)` enqueues the placement of candidates c0 .. c0 + nround - 1,
// then the warm-start program, the scan and the gather, until B scenarios are accepted.  The callers have checked their descriptions.
extern "C++" template <class F>
int raceline_rounds(dgsqp_solver* h, int64_t B, const dgsqp_raceline_ws_t* W, F place, double* x0_out, double* u_ws_out,
                    int64_t* candidates, int stage) {
  const DgProb& D = h->hp;
  if (D.M != 2) return refuse(h, "raceline: ", "the study's sampler places two cars");
  if (candidates) *candidates = 0;
  if (B == 0) return DGSQP_OK;
  { const int rc = stage_begin(h, B); if (rc) return rc; }
  double *const d_x0 = h->staged.dbl(DG_Q), *const d_uws = h->staged.dbl(DG_UWS);
  const int64_t nround = std::max<int64_t>(256, std::min<int64_t>(2 * B, 1 << 16));        // candidates per round, as dgsqp_sample_batch
  TmpBuf tb;
  DgRacelineProgram P;
  { const int rc = raceline_program(h, *W, nround, tb, P); if (rc) { h->B = 0; return rc; } }
  double* dq0 = tb.alloc<double>(nround * D.nq); double* du = tb.alloc<double>(nround * D.n);
  int32_t* dok = tb.alloc<int32_t>(nround); int32_t* dcol = tb.alloc<int32_t>(nround); int32_t* dpos = tb.alloc<int32_t>(nround); int32_t* dcnt = tb.alloc<int32_t>(1);
  if (!dq0 || !du || !dok || !dcol || !dpos || !dcnt) { h->err = "hipMalloc failed"; h->B = 0; return DGSQP_E_NOMEM; }
  const int rcs = run_sync(h, [&]() -> int {
    int64_t have = 0;
    unsigned long long c0 = 0;
    for (int round = 0; have < B; round++) {
      if (round > 10000) { h->err = "raceline: the sampler did not produce enough scenarios"; return DGSQP_E_ARG; }
      place(nround, c0, dq0, dcol);
      HIPCHK(h, hipGetLastError());
      { const int rc = raceline_enqueue(h, P, nround, dq0, du, dok); if (rc) return rc; }
      hipLaunchKernelGGL(dg_sample_scan_kernel, dim3(1), dim3(1024), 0, h->stream, nround, dok, dcol, dpos, dcnt);
      hipLaunchKernelGGL(dg_sample_gather_kernel, dim3(1024), dim3(128), 0, h->stream, nround, have, B, dpos, dq0, (const double*)du, d_x0, d_uws);
      HIPCHK(h, hipGetLastError());
      int32_t cnt = 0;
      HIPCHK(h, hipMemcpyAsync(&cnt, dcnt, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (have + cnt >= B && candidates) {
        std::vector<int32_t> pos((size_t)nround);
        HIPCHK(h, hipMemcpy(pos.data(), dpos, sizeof(int32_t) * nround, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < nround; i++) if (pos[i] == (int32_t)(B - have - 1)) { *candidates = (int64_t)(c0 + i + 1); break; }
      }
      have += cnt;
      c0 += (unsigned long long)nround;
    }
    return DGSQP_OK;
  });
  if (rcs) { h->B = 0; return rcs; }
  if (x0_out) HIPCHK(h, hipMemcpy(x0_out, d_x0, sizeof(double) * B * D.nq, hipMemcpyDeviceToHost));
  if (u_ws_out) HIPCHK(h, hipMemcpy(u_ws_out, d_uws, sizeof(double) * B * D.n, hipMemcpyDeviceToHost));
  h->B = stage ? B : 0;
  return DGSQP_OK;
}

int dgsqp_sample_raceline_batch(dgsqp_handle_t h, int64_t B, const dgsqp_raceline_sampler_t* spec, const dgsqp_raceline_ws_t* W,
                                double* x0_out, double* u_ws_out, int64_t* candidates, int stage) {
  if (!h) return DGSQP_E_ARG;
  if (B < 0 || !spec) return refuse(h, "raceline: ", "bad argument (B < 0 or no sampler description)");
  if (spec->n_key < 2 || spec->n_key > DGSQP_MAX_SEGS + 1 || !(spec->collision_d >= 0.0) || !std::isfinite(spec->collision_d) ||
      !std::isfinite(spec->obs_d) || !std::isfinite(spec->half_width) || first_non_finite(&spec->key_pts[0][0], (int64_t)spec->n_key * 6) >= 0 ||
      !(spec->key_pts[spec->n_key - 1][3] > 0.0))          // (the placement wraps s into [0, L): L must be a positive length)
    return refuse(h, "raceline: ", "bad sampler description");
  { const int rc = raceline_check(h, W); if (rc) return rc; }
  dgsqp_sampler_t track;
  memset(&track, 0, sizeof track);
  track.n_key = spec->n_key;
  memcpy(track.key_pts, spec->key_pts, sizeof track.key_pts);
  return raceline_rounds(h, B, W, [&](int64_t nround, unsigned long long c0, double* dq0, int32_t* dcol) {
    hipLaunchKernelGGL(dg_raceline_place_kernel, dim3((unsigned)((nround + 255) / 256)), dim3(256), 0, h->stream, nround, c0, *spec, track, h->rl.dev, dq0, dcol);
  }, x0_out, u_ws_out, candidates, stage);
}

int dgsqp_sample_raceline_spline_batch(dgsqp_handle_t h, int64_t B, const dgsqp_raceline_spline_sampler_t* spec, const dgsqp_raceline_ws_t* W,
                                       double* x0_out, double* u_ws_out, int64_t* candidates, int stage) {
  if (!h) return DGSQP_E_ARG;
  if (B < 0 || !spec) return refuse(h, "raceline: ", "bad argument (B < 0 or no sampler description)");
  if (h->hp.P.track_kind != DGSQP_TRACK_SPLINE) return refuse(h, "raceline: ", "the spline-track sampler on an arc-track handle (dgsqp_sample_raceline_batch places cars on arc tracks)");
  const double v[6] = {spec->s_lo, spec->s_hi, spec->gap_lo, spec->gap_hi, spec->ey_clip, spec->collision_d};
  if (first_non_finite(v, 6) >= 0 || spec->s_hi < spec->s_lo || spec->gap_hi < spec->gap_lo || spec->ey_clip < 0.0 || spec->collision_d < 0.0)
    return refuse(h, "raceline: ", "bad sampler description");
  { const int rc = raceline_check(h, W); if (rc) return rc; }
  return raceline_rounds(h, B, W, [&](int64_t nround, unsigned long long c0, double* dq0, int32_t* dcol) {
    hipLaunchKernelGGL(dg_raceline_place_spline_kernel, dim3((unsigned)((nround + 255) / 256)), dim3(256), 0, h->stream, nround, c0, *spec, h->rl_clip_widths, h->rl_clip_scale, h->rl.dev, dq0, dcol);
  }, x0_out, u_ws_out, candidates, stage);
}

int dgsqp_set_raceline_clip(dgsqp_handle_t h, int clip_widths, double clip_scale) {
  if (!h) return DGSQP_E_ARG;
  if (clip_widths != 0 && clip_widths != 1) return refuse(h, "raceline: ", "clip_widths must be 0 or 1");
  if (clip_widths && h->hp.P.n_width < 2) return refuse(h, "raceline: ", "clip_widths = 1 on a handle without a width table (dgsqp_problem_t.widths)");
  if (clip_widths && !(std::isfinite(clip_scale) && clip_scale >= 0.0)) return refuse(h, "raceline: ", "clip_scale must be finite and not negative");
  h->rl_clip_widths = clip_widths;
  h->rl_clip_scale = clip_widths ? clip_scale : 0.0;
  return DGSQP_OK;
}

// ---- track-frame transforms (dgsqp_track_frame.h) ----
// The ends of the handle's spline meet (tracks.CubicSplineTrack.circuit): the projection wraps s; otherwise it clips to [0, L].
static bool spline_is_circuit(const DgProb& D) {
  const int nk = D.P.n_knots, i = nk - 2;
  const double* cx = D.spl + nk + 4 * i;
  const double* cy = D.spl + nk + 4 * (nk - 1) + 4 * i;
  const double t = D.spl[nk - 1] - D.spl[i];
  const double xe = ((cx[3] * t + cx[2]) * t + cx[1]) * t + cx[0], ye = ((cy[3] * t + cy[2]) * t + cy[1]) * t + cy[0];
  const double x0 = D.spl[nk], y0 = D.spl[nk + 4 * (nk - 1)];
  return fabs(x0 - xe) <= 1e-6 + 1e-5 * fabs(xe) && fabs(y0 - ye) <= 1e-6 + 1e-5 * fabs(ye);
}
static int track_frame_check(dgsqp_solver* h, int64_t n, const dgsqp_track_frame_t* t, const void* in, const void* out) {
  if (n < 0) return refuse(h, "track frame: ", "n < 0");
  if (!t || !in || !out) return refuse(h, "track frame: ", "a NULL pointer (track description, input or output)");
  const bool spline = h->hp.P.track_kind == DGSQP_TRACK_SPLINE;
  if (t->n_key == 0 && !spline) return refuse(h, "track frame: ", "n_key = 0 means the handle's spline, and this handle's track is made of arcs: give its key points");
  if (t->n_key != 0 && spline) return refuse(h, "track frame: ", "key points on a spline-track handle (n_key must be 0: the handle's spline)");
  if (!std::isfinite(t->half_width) || !std::isfinite(t->slack)) return refuse(h, "track frame: ", "half_width / slack is not finite");
  if (t->n_key != 0) {
    if (t->n_key < 2 || t->n_key > DGSQP_MAX_SEGS + 1) return refuse(h, "track frame: ", "n_key = " + std::to_string(t->n_key) + " (2 .. DGSQP_MAX_SEGS + 1 key points)");
    const int64_t bad = first_non_finite(&t->key_pts[0][0], (int64_t)t->n_key * 6);
    if (bad >= 0) return refuse(h, "track frame: ", "key point [" + std::to_string(bad / 6) + "][" + std::to_string(bad % 6) + "] is not finite");
    if (!(t->key_pts[t->n_key - 1][3] > 0.0)) return refuse(h, "track frame: ", "the track length (last key point's cumulative length) is not positive");
  }
  return DGSQP_OK;
}
static dim3 track_frame_grid(dgsqp_solver* h, int64_t n) { return dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8 * (int64_t)h->num_cu)); }

int dgsqp_local_to_global_batch(dgsqp_handle_t h, int64_t n, const dgsqp_track_frame_t* t, const double* cl, double* xy) {
  if (!h) return DGSQP_E_ARG;
  { const int rc = track_frame_check(h, n, t, cl, xy); if (rc) return rc; }
  if (n == 0) return DGSQP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  TmpBuf tb;
  double* dcl = tb.alloc<double>((size_t)n * 3); double* dxy = tb.alloc<double>((size_t)n * 3);
  if (!dcl || !dxy) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(dcl, cl, sizeof(double) * (size_t)n * 3, hipMemcpyHostToDevice));
  dgsqp_sampler_t track;
  memset(&track, 0, sizeof track);
  track.n_key = t->n_key;
  memcpy(track.key_pts, t->key_pts, sizeof track.key_pts);
  const int rc = run_sync(h, [&]() -> int {
    if (t->n_key == 0) hipLaunchKernelGGL(dg_spline_l2g_kernel, track_frame_grid(h, n), dim3(256), 0, h->stream, n, (const double*)dcl, dxy);
    else hipLaunchKernelGGL(dg_arc_l2g_kernel, track_frame_grid(h, n), dim3(256), 0, h->stream, n, track, (const double*)dcl, dxy);
    HIPCHK(h, hipGetLastError());
    return DGSQP_OK;
  });
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(xy, dxy, sizeof(double) * (size_t)n * 3, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

int dgsqp_global_to_local_batch(dgsqp_handle_t h, int64_t n, const dgsqp_track_frame_t* t, const double* xy, double* cl, double* resid,
                                int32_t* status) {
  if (!h) return DGSQP_E_ARG;
  { const int rc = track_frame_check(h, n, t, xy, cl); if (rc) return rc; }
  if (!status) return refuse(h, "track frame: ", "a NULL pointer (status)");
  if (n == 0) return DGSQP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  TmpBuf tb;
  double* dxy = tb.alloc<double>((size_t)n * 3); double* dcl = tb.alloc<double>((size_t)n * 3);
  double* dres = resid ? tb.alloc<double>((size_t)n) : nullptr;
  int32_t* dst = tb.alloc<int32_t>((size_t)n);
  if (!dxy || !dcl || (resid && !dres) || !dst) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(dxy, xy, sizeof(double) * (size_t)n * 3, hipMemcpyHostToDevice));
  const int circuit = t->n_key == 0 && spline_is_circuit(h->hp) ? 1 : 0;
  const int rc = run_sync(h, [&]() -> int {
    if (t->n_key == 0) hipLaunchKernelGGL(dg_spline_project_kernel, track_frame_grid(h, n), dim3(256), 0, h->stream, n, circuit, t->half_width + t->slack, (const double*)dxy, dcl, dres, dst);
    else hipLaunchKernelGGL(dg_arc_project_kernel, track_frame_grid(h, n), dim3(256), 0, h->stream, n, *t, (const double*)dxy, dcl, dres, dst);
    HIPCHK(h, hipGetLastError());
    return DGSQP_OK;
  });
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(cl, dcl, sizeof(double) * (size_t)n * 3, hipMemcpyDeviceToHost));
  if (resid) HIPCHK(h, hipMemcpy(resid, dres, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(status, dst, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

int dgsqp_qp_batch(dgsqp_handle_t h, int64_t B, const double* x0, const double* u, const double* l, double* du_out,
                   double* lhat, double* Qpd, int32_t* flag) {
  return dgsqp_qp_batch_info(h, B, x0, u, l, du_out, lhat, Qpd, flag, nullptr);
}

int dgsqp_qp_batch_info(dgsqp_handle_t h, int64_t B, const double* x0, const double* u, const double* l, double* du_out,
                        double* lhat, double* Qpd, int32_t* flag, double* info8) {
  if (!h || B < 0 || !x0 || !u || !l) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  if (B == 0) return DGSQP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const DgProb& D = h->hp;
  const int grid = grid_for(h, B);
  int rc = u_prev_check(h, B);
  if (rc) return rc;
  rc = idle_with_ws(h, B);
  if (rc) return rc;
  TmpBuf tb;
  const double* dup = nullptr; int64_t up_stride = 0;
  if ((rc = u_prev_hook(h, B, tb, &dup, &up_stride))) return rc;
  const size_t n = D.n, nc = D.nc;
  double* dx0 = tb.alloc<double>(B * D.nq); double* du = tb.alloc<double>(B * n); double* dl = tb.alloc<double>(B * nc);
  double* ddu = du_out ? tb.alloc<double>(B * n) : nullptr; double* dlh = lhat ? tb.alloc<double>(B * nc) : nullptr;
  double* dQ = Qpd ? tb.alloc<double>(B * n * n) : nullptr; int32_t* df = flag ? tb.alloc<int32_t>(B) : nullptr;
  double* dinfo = info8 ? tb.alloc<double>(B * 8) : nullptr;
  if (!dx0 || !du || !dl || (du_out && !ddu) || (lhat && !dlh) || (Qpd && !dQ) || (flag && !df) || (info8 && !dinfo)) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(dx0, x0, sizeof(double) * B * D.nq, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(du, u, sizeof(double) * B * n, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dl, l, sizeof(double) * B * nc, hipMemcpyHostToDevice));
  rc = run_sync(h, [&]() -> int {
    hipLaunchKernelGGL(dg_qp_kernel, dim3(grid), dim3(DG_BLOCK), h->lds_bytes, h->stream, h->dp, B, dx0, du, dl, ddu, dlh, dQ, df, dinfo, h->ws, dup, up_stride);
    HIPCHK(h, hipGetLastError());
    return DGSQP_OK;
  });
  if (rc) return rc;
  if (du_out) HIPCHK(h, hipMemcpy(du_out, ddu, sizeof(double) * B * n, hipMemcpyDeviceToHost));
  if (lhat) HIPCHK(h, hipMemcpy(lhat, dlh, sizeof(double) * B * nc, hipMemcpyDeviceToHost));
  if (Qpd) HIPCHK(h, hipMemcpy(Qpd, dQ, sizeof(double) * B * n * n, hipMemcpyDeviceToHost));
  if (flag) HIPCHK(h, hipMemcpy(flag, df, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
  if (info8) HIPCHK(h, hipMemcpy(info8, dinfo, sizeof(double) * B * 8, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

// ---- RCCL communicator owned by the handle -----------------------------------------------------------------------------
int dgsqp_comm_unique_id(char* out128) {
  if (!out128) return DGSQP_E_ARG;
  if (!g_rccl.load()) { g_create_err = g_rccl.err; return DGSQP_E_DEVICE; }
  ncclUniqueId id;
  if (g_rccl.GetUniqueId(&id) != ncclSuccess) { g_create_err = "ncclGetUniqueId failed"; return DGSQP_E_DEVICE; }
  static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
  memcpy(out128, &id, 128);
  return DGSQP_OK;
}

int dgsqp_comm_init(dgsqp_handle_t h, const char* id128, int rank, int world) {
  if (!h || !id128 || world < 1 || rank < 0 || rank >= world) { if (h) h->err = "bad argument"; return DGSQP_E_ARG; }
  if (h->comm) { h->err = "communicator already initialised"; return DGSQP_E_ARG; }
  if (!g_rccl.load()) { h->err = g_rccl.err; return DGSQP_E_DEVICE; }
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  dgsqp_comm_state* c = new dgsqp_comm_state();
  c->rank = rank; c->world = world;
  ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, id, rank);
  if (r != ncclSuccess) { h->err = std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error"); delete c; return DGSQP_E_DEVICE; }
  if (hipMalloc(&c->d_red, sizeof(double) * 64) != hipSuccess) { g_rccl.CommDestroy(c->comm); delete c; h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  h->comm = c;
  return DGSQP_OK;
}

int dgsqp_comm_destroy(dgsqp_handle_t h) {
  if (!h || !h->comm) return DGSQP_OK;
  (void)hipSetDevice(h->device);
  dgsqp_comm_state* c = h->comm;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (c->comm) (void)g_rccl.CommDestroy(c->comm);
  if (c->d_rec) (void)hipFree(c->d_rec);
  if (c->d_all) (void)hipFree(c->d_all);
  if (c->d_red) (void)hipFree(c->d_red);
  delete c;
  h->comm = nullptr;
  return DGSQP_OK;
}

int dgsqp_gather_stats(dgsqp_handle_t h, int64_t B_pad, dgsqp_stat_record_t* out) {
  if (!h || !out || !h->comm) { if (h) h->err = "dgsqp_comm_init first"; return DGSQP_E_ARG; }
  if (B_pad < h->B || B_pad <= 0) { h->err = "B_pad must be at least this rank's batch size"; return DGSQP_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  { int rc = wait_idle(h); if (rc) return rc; }
  dgsqp_comm_state* c = h->comm;
  if (c->rec_cap < B_pad) {
    if (c->d_rec) (void)hipFree(c->d_rec);
    if (c->d_all) (void)hipFree(c->d_all);
    c->d_rec = c->d_all = nullptr; c->rec_cap = 0;
    HIPCHK(h, hipMalloc(&c->d_rec, sizeof(dgsqp_stat_record_t) * B_pad));
    HIPCHK(h, hipMalloc(&c->d_all, sizeof(dgsqp_stat_record_t) * B_pad * c->world));
    c->rec_cap = B_pad;
  }
  const SolveOutPtrs O = h->staged.out(rec_count_batch(h->B));      // (the kernel takes the five arrays it packs one by one)
  hipLaunchKernelGGL(dg_pack_stats_kernel, dim3((unsigned)((B_pad + 255) / 256)), dim3(256), 0, h->stream, h->B, B_pad, h->hp.M, c->rank,
                     O.status, O.iters, O.qp_solves, O.cond, O.cost, c->d_rec);
  HIPCHK(h, hipGetLastError());
  NCCLCHK(h, g_rccl.AllGather(c->d_rec, c->d_all, sizeof(dgsqp_stat_record_t) * B_pad, ncclChar, c->comm, h->stream));
  HIPCHK(h, hipMemcpyAsync(out, c->d_all, sizeof(dgsqp_stat_record_t) * B_pad * c->world, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DGSQP_OK;
}

int dgsqp_comm_allreduce_max(dgsqp_handle_t h, double* values, int count) {
  if (!h || !values || count < 1 || count > 64 || !h->comm) { if (h) h->err = "bad argument / dgsqp_comm_init first"; return DGSQP_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  dgsqp_comm_state* c = h->comm;
  HIPCHK(h, hipMemcpyAsync(c->d_red, values, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
  NCCLCHK(h, g_rccl.AllReduce(c->d_red, c->d_red, count, ncclDouble, ncclMax, c->comm, h->stream));
  HIPCHK(h, hipMemcpyAsync(values, c->d_red, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return DGSQP_OK;
}

int dgsqp_comm_barrier(dgsqp_handle_t h) {
  double v = 0.0;
  return dgsqp_comm_allreduce_max(h, &v, 1);
}

}  // extern "C"
