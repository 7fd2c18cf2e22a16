// Closed-loop (receding-horizon) batches in one launch: one workgroup carries one scenario through all T steps of DGSQP.step()
// (DGSQP.py:283-297), so that a launch is bounded by its longest CHAIN and no intermediate state leaves the device.
// Included by dgsqp_api.hip after dg_solve_kernel; host mirror of the feedback rule: dgsqp_amd/closed_loop.py.
#pragma once
#include "dgsqp_pid.h"      // dev_pid_law, the PID driver's law

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
  double* up;            // [T][B][nu]     carry on: slice t = the input applied before solve t (slice 0 from the host); fed back like q and
                         // uws.  Null: carry off, every solve reads up_zero
  const double* up_zero; // the handle's nu zeros
};

// Everything a launch with a plant hands the kernel, in one pack: the argument of the one instantiation of dg_closed_loop_kernel that
// every launch with a plant of the game's model class runs.  A setting the caller leaves off is a null pointer, a zero, or the default the
// host layer builds (all-GAME kinds; R = 1 with the reference's rule), so a further setting is a field and a branch.  B: records are
// indexed by the CHAIN b, never by the workgroup.  Per-workgroup buffers ([grid]...) are written and read back by the same lane of the
// same workgroup (lane a for agent a), and cleared by it when a chain starts: plain pointers, like q and uws.
struct DgPlantPack {
  static constexpr bool cross = false;
  int64_t B;                          // chains of the launch
  // the plant (dgsqp_set_plant; reference DGSQP/dynamics/dynamics_simulator.py:11-40): after every step the state is advanced by S
  // simulation steps of length dt / S of a model with the plant's vehicle parameters and integrator, every input channel behind a delay line
  const dgsqp_plant_t* P;             // resolved by the host: agents[] hold the game's records when the plant uses the game's parameters
  double* lines;                      // [grid][DGSQP_MAX_AGENTS][DGSQP_NUA][DGSQP_MAX_DELAY]
  double* u_plant;                    // [T][B][S][nu]  the inputs the plant integrated under
  // a plant per chain (dgsqp_set_plant_ensemble)
  const dgsqp_vehicle_t* vehicles;    // [B][M] chain b's vehicle records, or null (every chain runs P)
  const int32_t* delay;               // [B][M][DGSQP_NUA] chain b's delays, or null (P's)
  dgsqp_plant_t* wg_plant;            // [grid] the plant of the chain a workgroup carries: filled when the chain starts (with vehicles only)
  // state estimates (dgsqp_set_estimate_noise)
  const double* v;                    // [T][B][nq] estimate noise, or null (the solves start from the true state)
  double* q_est;                      // [T][B][nq] q + v, what solve t starts from
  // the safety monitor (dgsqp_set_monitor)
  int monitor;                        // 0 off, 1 record, 2 record and stop
  double* mon_scratch;                // [grid][S][M][3] per simulation step and agent: position (2), the agent's own box excess
  double* clearance;                  // [T][B]
  double* box_excess;                 // [T][B]
  int32_t* hit_step;                  // [B], -1 until the chain's first hit
  // drivers (dgsqp_set_drivers): who produces the command entering agent a's plant at control step t of chain b -- the game, the lane
  // follower dev_pid_law closed-loop on the TRUE state, or the caller's u_replay
  const int32_t* kind;                // [B][M] DGSQP_DRIVER_*
  const dgsqp_pid_t* pid;             // [M] the gains of agent a's lane follower (read for PID and TRACK agents)
  const double* ref;                  // [B][M][2] (v_ref, lat_ref), or null: from the chain's initial state, as the warm-start PID does
  const double* u_replay;             // [T][B][nu], or null (no REPLAY agent)
  double* u_cmd;                      // [T][B][nu] the command each agent's plant received, or null (no record asked for: all-GAME, default hold)
  double* pid_state;                  // [grid][M][3] ei, previous u_a, previous u_steer
  // a held plan (dgsqp_set_plan_hold; the table in include/dgsqp.h): a chain solves only when a plan is due and otherwise consumes the
  // warm start it holds, stage by stage
  int32_t replan_every, on_fail;      // R; DGSQP_HOLD_*
  uint32_t fail_mask;                 // bit s: status s is a failed solve
  double* u_game;                     // [T][B][nu] the game's command: stage 0 of the step's solution, or of the plan it holds; or null (no record asked for)
  int32_t* plan_stage;                // [T][B] how many stages of its plan the chain had consumed before u_game[t][b]; null with u_game
  int32_t* state;                     // [grid][2] age, due: written by lane 0, read by every lane after a fence and a barrier
};

// A plant of ANOTHER model class than the game's (dgsqp_set_cross_plant), the argument of the third instantiation: the plant keeps a
// state z of its own, [T+1][B][nz_all], fed back like q by the lane that wrote it, and the game sees the projection q = p(z) -- entry i of
// agent a's block of q is entry proj[a][i] of its block of z.  `lift` is the game with every agent's state bounds moved to the plant's
// layout (+-inf on entries the game does not see): what the monitor reads when a z block is integrated; `game` is the game as a plant
// (its integrator and sub-steps, one simulation step, no delay): one step of it from p(z) under the game's command is the reference a
// TRACK driver follows.
struct DgCrossPack : DgPlantPack {
  static constexpr bool cross = true;
  int32_t mdl[DGSQP_MAX_AGENTS], nz[DGSQP_MAX_AGENTS], zoff[DGSQP_MAX_AGENTS];      // the plant agents' classes, state counts, offsets in z
  int32_t nz_all;                                                                   // their sum
  int8_t proj[DGSQP_MAX_AGENTS][DGSQP_MAX_NQA];
  const dgsqp_problem_t* lift;
  const dgsqp_plant_t* game;
  double* z;                          // [T+1][B][nz_all] slice 0 = z0, slice t + 1 = the plant's state after step t
  double* track_ref;                  // [T][B][M][3] (v_ref, lat_ref, epsi_ref) of the TRACK agents
};

// Agent a's monitor record of one simulation step, from its state block z: the position and the largest excess over the GAME's bounds
// (-inf: no finite bound; NaN: an entry of z is not finite).  One lane, no cross-lane operation.
__device__ inline void dev_monitor_store(const dgsqp_agent_t& game, int nqa, const double* z, double* rec) {
  double ex = -INFINITY;
  bool fin = true;
  for (int i = 0; i < nqa; i++) {
    fin = fin && isfinite(z[i]);
    if (isfinite(game.st_ub[i])) ex = fmax(ex, z[i] - game.st_ub[i]);
    if (isfinite(game.st_lb[i])) ex = fmax(ex, game.st_lb[i] - z[i]);
  }
  rec[0] = z[0]; rec[1] = z[1]; rec[2] = fin ? ex : NAN;
}

// S simulation steps of agent a's plant from q (in place).  Simulation step `count` (counted from the chain's start) of a channel with
// delay d > 0 integrates under entry count % d of its line -- the oldest of the last d -- and then stores u_new there (a deque of
// length d: read [0], append); d = 0 integrates under u_new.  One plant step is DEV_RK_SUBSTEP (dgsqp_device.h) on f_c with the plant's
// agent record, integrator, step length and sub-step count (euler: one step per simulation step, as the game's model).
// With a non-null `mon` ([S][M][3], the workgroup's): the agent's monitor record after every simulation step (dev_monitor_store).
template <int MDL, bool SPL>
__device__ inline void dev_plant_agent(const dgsqp_problem_t& P, const dgsqp_plant_t& pl, int a, int64_t count, const double* u_new,
                                       double* line, double* u_rec, int nu, double* qa, double* mon) {
  typedef Ty<0> T;
  const dgsqp_agent_t& ag = pl.agents[a];
  const int S = pl.sim_steps, integ = pl.integrator, nsub = integ == DGSQP_INT_EULER ? 1 : pl.substeps;
  const double h = P.dt / S / nsub;
  constexpr int NQA = dg_model_nq(MDL);
  T x[NQA], u[DGSQP_NUA];
#pragma unroll
  for (int i = 0; i < NQA; i++) x[i].c[0] = qa[i];
  for (int j = 0; j < S; j++, count++) {
    for (int ch = 0; ch < DGSQP_NUA; ch++) {
      const int d = pl.delay[a][ch];
      double v = u_new[ch];
      if (d > 0) {
        double* slot = line + ch * DGSQP_MAX_DELAY + (int)(count % d);
        v = *slot;
        *slot = u_new[ch];
      }
      u[ch].c[0] = v;
      u_rec[(int64_t)j * nu + ch] = v;
    }
    FcPre<0> pre;
    dev_fc_pre<0, MDL>(ag, u, pre);
    for (int m = 0; m < nsub; m++) DEV_RK_SUBSTEP(0, MDL, SPL, integ, P, ag, x, u, pre, h);
    if (mon) {
      double z[NQA];
#pragma unroll
      for (int i = 0; i < NQA; i++) z[i] = x[i].c[0];
      dev_monitor_store(P.agents[a], NQA, z, mon + ((int64_t)j * P.M + a) * 3);
    }
  }
#pragma unroll
  for (int i = 0; i < NQA; i++) qa[i] = x[i].c[0];
}

// dev_plant_agent for an agent of model class `mdl` on P's track (dev_with_model).  Out of line: one body (some 28 k instructions)
// serves both feedbacks and the TRACK driver's reference step.  That step so has a unicycle arm too; it is never taken there, since the
// host refuses a TRACK driver for a unicycle.
__device__ __noinline__ void dev_plant_model(int mdl, const dgsqp_problem_t& P, const dgsqp_plant_t& pl, int a, int64_t count, const double* u_new,
                                             double* line, double* u_rec, int nu, double* x, double* mon) {
  // (the command is read here, not through the closure: the compiler then still passes it in registers, as it did before the closure)
  const double c[DGSQP_NUA] = {u_new[0], u_new[1]};
  dev_with_model(mdl, P.track_kind == DGSQP_TRACK_SPLINE, [&](auto m) {
    dev_plant_agent<decltype(m)::MDL, decltype(m)::SPL>(P, pl, a, count, c, line, u_rec, nu, x, mon);
  });
}

// A held plan: which row of the table (include/dgsqp.h) step t falls under, from whether it solved and the solve's status.
enum { DG_HOLD_ACCEPT = 0, DG_HOLD_KEEP = 1, DG_HOLD_CONSUME = 2 };
__device__ inline int dev_hold_rule(const DgPlantPack& pk, int solved, int status) {
  if (!solved) return DG_HOLD_CONSUME;
  if (status < 0 || status > 5 || !((pk.fail_mask >> status) & 1u)) return DG_HOLD_ACCEPT;
  return pk.on_fail == DGSQP_HOLD_HOLD ? DG_HOLD_CONSUME : DG_HOLD_KEEP;
}

// Whether step t of the workgroup's chain solves.  (age, due) is reset where the delay lines and the PID state are (t == 0); afterwards it
// is what dev_hold_next left, behind the fence and barrier that end a step.  The same value on every lane: the branch on it is uniform.
__device__ __noinline__ int dev_hold_due(DgPlantPack pk, int t) {
  int32_t* st = pk.state + (int64_t)blockIdx.x * 2;
  if (t == 0) {
    if (TID == 0) { st[0] = 0; st[1] = 1; }
    __threadfence_block();
    __syncthreads();
  }
  return __builtin_amdgcn_readfirstlane(st[1]);
}

// The step between two solves, t of chain b; every lane of the workgroup calls it, and lane a < M works for agent a, in this order:
//   1. the game's command -- stage 0 of the solution u_t, or of the warm start uws_t the chain holds (dev_hold_rule) -- to u_game[t][b];
//      lane 0 writes plan_stage.  uws_t was written one step ago behind a fence and a barrier (or by the host), age by this very lane.
//   2. its driver's command to u_cmd[t][b]: the game's, dev_pid_law on the TRUE state of the plant's agent (also when the solves start from
//      estimates; its dt is the control step), the caller's u_replay, or with a cross plant TRACK: dev_pid_law towards one step of the
//      game's model from p(z_t) under the game's command (track_ref[t][b][a]).  The PID state is cleared where the delay lines are.
//   3. chain b's plant: with per-chain vehicles, the vehicle records and delays of CHAIN b are copied into the workgroup's own
//      dgsqp_plant_t when the chain starts -- lane a its agent's, lane 0 the shared scalars -- and read back after a fence and a barrier.
//   4. the delay lines (cleared when the chain starts) and the S simulation steps of its state block under that command, with the plant
//      agent's class (dev_plant_model); u_plant; with the monitor on, its records of the S steps to the workgroup's scratch.
//   5. q[t+1][b] = the state reached (+ w_t; the monitor's record of the last simulation step is stored again after w_t: that state is
//      q_next).  With a cross plant the block is z's: z[t+1][b], and q[t+1][b] = p(z[t+1][b]); nothing is added to z.
//   6. with the monitor on, after another fence and barrier, lane 0 reduces the pairs and writes clearance, box_excess and hit_step.
// The commands stay in the lane's registers from 1 to 4.  Returns non-zero on the lanes whose part of the next state is not finite, and
// from lane 0 (as 1: every feedback returns 0 or 1) after a hit in mode 2, which ends the chain as well.
// Out of line: the solve that is inlined next to the call keeps its register allocation.  The caller has fenced the solve's records
// (u_t); q_t and z_t were written by this very lane one step ago, or by the host.
template <class PACK>
__device__ __noinline__ int dev_plant_feedback(PACK pk, int solved, int status, const double* uws_t, int t, int64_t tb_b,
                                               const double* q_t, const double* u_t, const double* w_t, double* q_next) {
  constexpr bool X = PACK::cross;
  const DgProb& D = dg_prob;
  const int a = TID, M = D.M;
  const int64_t b = tb_b - (int64_t)t * pk.B;
  // the agent's state block s of ns entries, the slot sn of its successor, the doubles between two slices of that state, its model class,
  // and the game the plant's monitor and PID read: with a cross plant all of it is the PLANT's (z; the game through `lift`)
  const dgsqp_problem_t* G = &D.P;
  int ns = 0, mdl = 0;
  int64_t slice = 0;
  const double* s = nullptr;
  double* sn = nullptr;
  double c[DGSQP_NUA] = {};
  if (a < M) {
    ns = D.nqa[a]; mdl = D.mdl[a]; slice = pk.B * D.nq; s = q_t + D.qoff[a]; sn = q_next + D.qoff[a];
    if constexpr (X) {
      G = pk.lift; ns = pk.nz[a]; mdl = pk.mdl[a]; slice = pk.B * pk.nz_all;
      s = pk.z + tb_b * pk.nz_all + pk.zoff[a]; sn = pk.z + (tb_b + pk.B) * pk.nz_all + pk.zoff[a];
    }
    // 1. the game's command
    const int rule = dev_hold_rule(pk, solved, status);
    const double* src = rule == DG_HOLD_CONSUME ? uws_t : u_t;
    double g[DGSQP_NUA];
    for (int j = 0; j < DGSQP_NUA; j++) {
      g[j] = src[am_col(D, a, 0, j)];
      if (pk.u_game) pk.u_game[tb_b * D.nu + a * DGSQP_NUA + j] = g[j];
    }
    if (a == 0 && pk.plan_stage) pk.plan_stage[tb_b] = rule == DG_HOLD_CONSUME ? pk.state[(int64_t)blockIdx.x * 2] : 0;
    // 2. the driver's command
    const int kind = pk.kind[b * M + a];
    const bool track = X && kind == DGSQP_DRIVER_TRACK;
    double* st = pk.pid_state + ((int64_t)blockIdx.x * M + a) * 3;
    if (t == 0) { st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; }
    if (kind == DGSQP_DRIVER_PID || track) {
      const int epsi = ns == 8 ? 5 : 3, ey = ns - 1;                      // (state layout: dev_pid_agent)
      double v_ref = 0.0, lat_ref = 0.0, epsi_ref = 0.0;
      if (track) {
        if constexpr (X) {
          // one step of the GAME's discrete model from p(z_t) under g: the game as a plant has no delay (the line is never touched) and
          // one simulation step, whose input record goes to a local
          const int nqa = D.nqa[a];
          double xr[DGSQP_MAX_NQA], rec[DGSQP_NUA];
          for (int i = 0; i < DGSQP_MAX_NQA; i++) xr[i] = i < nqa ? s[pk.proj[a][i]] : 0.0;
          dev_plant_model(D.mdl[a], *G, *pk.game, a, 0, g, nullptr, rec, DGSQP_NUA, xr, nullptr);
          v_ref = xr[2]; lat_ref = xr[nqa - 1]; epsi_ref = xr[nqa == 8 ? 5 : 3];      // (the GAME's layout)
          double* tr = pk.track_ref + (tb_b * M + a) * 3;
          tr[0] = v_ref; tr[1] = lat_ref; tr[2] = epsi_ref;
        }
      } else {
        const double* s0 = s - (int64_t)t * slice;                          // the chain's initial state: slice 0
        const double* ref = pk.ref ? pk.ref + (b * M + a) * 2 : nullptr;
        v_ref = ref ? ref[0] : s0[2]; lat_ref = ref ? ref[1] : s0[ey];
      }
      double ei = st[0], up0 = st[1], up1 = st[2];
      dev_pid_law(pk.pid[a], G->dt, s[2], v_ref, s[ey], lat_ref, track ? s[epsi] - epsi_ref : s[epsi], ei, up0, up1);
      st[0] = ei; st[1] = up0; st[2] = up1;
      c[0] = up0; c[1] = up1;
    }
    else if (kind == DGSQP_DRIVER_REPLAY)
      for (int j = 0; j < DGSQP_NUA; j++) c[j] = pk.u_replay[tb_b * D.nu + a * DGSQP_NUA + j];
    else
      for (int j = 0; j < DGSQP_NUA; j++) c[j] = g[j];
    if (pk.u_cmd)
      for (int j = 0; j < DGSQP_NUA; j++) pk.u_cmd[tb_b * D.nu + a * DGSQP_NUA + j] = c[j];
  }
  // 3. the chain's plant
  const dgsqp_plant_t* pl = pk.P;
  if (pk.vehicles) {
    dgsqp_plant_t* mine = pk.wg_plant + blockIdx.x;
    if (t == 0) {
      if (a == 0) { mine->integrator = pl->integrator; mine->substeps = pl->substeps; mine->sim_steps = pl->sim_steps; mine->use_game_agents = 0; }
      if (a < M) {
        __builtin_memcpy(&mine->agents[a], &pk.vehicles[b * M + a], sizeof(dgsqp_vehicle_t));      // (the vehicle prefix of dgsqp_agent_t)
        for (int ch = 0; ch < DGSQP_NUA; ch++) mine->delay[a][ch] = pk.delay ? pk.delay[(b * M + a) * DGSQP_NUA + ch] : pl->delay[a][ch];
      }
      __threadfence_block();
      __syncthreads();
    }
    pl = mine;
  }
  const int S = pl->sim_steps;
  double* mon = pk.monitor ? pk.mon_scratch + (int64_t)blockIdx.x * S * M * 3 : nullptr;
  int bad = 0;
  if (a < M) {
    // 4. the delay lines and the S simulation steps
    double* line = pk.lines + ((int64_t)blockIdx.x * DGSQP_MAX_AGENTS + a) * (DGSQP_NUA * DGSQP_MAX_DELAY);
    if (t == 0)
      for (int i = 0; i < DGSQP_NUA * DGSQP_MAX_DELAY; i++) line[i] = 0.0;      // every chain starts with empty (zero) lines
    double x[DGSQP_MAX_NQA];
    for (int i = 0; i < DGSQP_MAX_NQA; i++) x[i] = i < ns ? s[i] : 0.0;
    double* u_rec = pk.u_plant + tb_b * S * D.nu + a * DGSQP_NUA;
    dev_plant_model(mdl, *G, *pl, a, (int64_t)t * S, c, line, u_rec, D.nu, x, mon);
    // 5. the next state
    for (int i = 0; i < DGSQP_MAX_NQA; i++)
      if (i < ns) {
        double v = x[i];
        if constexpr (!X)
          if (w_t) v = v + w_t[D.qoff[a] + i];
        sn[i] = v;
        bad |= !isfinite(v);
        x[i] = v;
      }
    if constexpr (X) {
      for (int i = 0; i < DGSQP_MAX_NQA; i++)
        if (i < D.nqa[a]) q_next[D.qoff[a] + i] = x[pk.proj[a][i]];
    }
    else if (mon) dev_monitor_store(G->agents[a], ns, x, mon + ((int64_t)(S - 1) * M + a) * 3);
  }
  if (!mon) return bad;
  // 6. the monitor
  __threadfence_block();
  __syncthreads();
  if (a == 0) {
    double cl = INFINITY, bx = -INFINITY;
    bool fin = true;
    int hit = -1;
    for (int j = 0; j < S; j++)
      for (int i = 0; i < M; i++) {
        const double* ri = mon + ((int64_t)j * M + i) * 3;
        fin = fin && ri[2] == ri[2];
        bx = fmax(bx, ri[2]);
        for (int k = i + 1; k < M; k++) {
          const double* rk = ri + (k - i) * 3;
          const double dx = ri[0] - rk[0], dy = ri[1] - rk[1];
          const double d = sqrt(dx * dx + dy * dy) - (G->agents[i].radius + G->agents[k].radius);
          cl = fmin(cl, d);
          if (d < 0.0 && hit < 0) hit = j;
        }
      }
    pk.clearance[tb_b] = fin ? cl : NAN;
    pk.box_excess[tb_b] = fin ? bx : NAN;
    if (hit >= 0) {
      if (pk.hit_step[b] < 0) pk.hit_step[b] = t * S + hit;
      if (pk.monitor == 2) bad = 1;
    }
  }
  return bad;
}

// The next warm start with a held plan and the chain's (age, due) after the step; every lane of the workgroup calls it, after the barrier
// that decided that the chain goes on (so every lane has read `due` of this step).
__device__ __noinline__ void dev_hold_next(DgPlantPack pk, int solved, int status, const double* uws_t, const double* u_t, double* uws_next) {
  const int n = dg_prob.n, N = dg_prob.N;
  const int rule = dev_hold_rule(pk, solved, status);
  const double* src = rule == DG_HOLD_ACCEPT ? u_t : uws_t;
  for (int i = TID; i < n; i += NT) {
    const int k = (i % (N * DGSQP_NUA)) / DGSQP_NUA;
    uws_next[i] = rule == DG_HOLD_KEEP ? uws_t[i] : src[k + 1 < N ? i + DGSQP_NUA : i];
  }
  if (TID == 0) {
    int32_t* st = pk.state + (int64_t)blockIdx.x * 2;
    if (rule == DG_HOLD_ACCEPT) { st[0] = 1; st[1] = 1 >= pk.replan_every; }
    else if (rule == DG_HOLD_CONSUME) {
      const int age = st[0] + 1;
      st[0] = age;
      if (!solved) st[1] = age >= pk.replan_every;
    }
  }
}

// The state solve t of chain b starts from.  With estimates: the lanes write q_est[t][b] = q[t][b] + v[t][b], and the slice is handed to
// the solve through memory (fence + barrier) like every other state; returns non-zero when it is not finite (the chain ends before
// the solve).  Out of line, as the feedback.
__device__ __noinline__ int dev_estimate(DgPlantPack pk, int64_t tb_b, const double* q_t, const double** x0) {
  if (!pk.v) { *x0 = q_t; return 0; }
  const int nq = dg_prob.nq;
  double* qe = pk.q_est + tb_b * nq;
  const double* v = pk.v + tb_b * nq;
  int bad = 0;
  for (int i = TID; i < nq; i += NT) {
    const double e = q_t[i] + v[i];
    qe[i] = e;
    bad |= !isfinite(e);
  }
  __threadfence_block();
  *x0 = qe;
  return __syncthreads_or(bad);
}

// Per ticket b, for t = 0 .. T-1: solve from (q[t][b], uws[t][b]) exactly as dg_solve_kernel would, then
//   q[t+1][b]   = x_t[b][1] (+ w[t][b])                          the game's own discrete model is the plant
//            or = plant(q[t][b], stage 0 of u_t[b]) (+ w[t][b])  with a PLANT: dev_plant_feedback
//            or = plant(q[t][b], u_cmd[t][b]) (+ w[t][b])         with DRIVERS: each agent's command is the game's, a PID's or replayed
//   uws[t+1][b] = shift(u_t[b]), or uws[t][b] after 'diverged' / 'qp_fail'   (DGSQP.py:293-295)
// shift, per agent: row k takes row k + 1, the last row is repeated (np.vstack((u_pred[1:], u_pred[-1]))).
// A non-finite q[t+1][b] ends the chain: steps_done[b] = t + 1, and no solve starts from such a state (q[t+1][b] keeps that state,
// uws[t+1][b] is not written).  The records of steps that never ran keep what the host filled them with before the launch
// (status DGSQP_NOT_RUN, zero counts, NaN).
// No cooperative line search, no deferral, no event or iterate log: a chain's next solve depends on its last one.
// PLANT is empty, one DgPlantPack or one DgCrossPack: the instantiation without a plant has the argument list it always had and holds
// nothing of the plant; with a plant, every setting on top of it is a field of the pack.  With a plant:
// A non-finite q_est[t][b] (estimates on) ends the chain BEFORE solve t: steps_done[b] = t.
// Step t solves only when a plan is due (dev_hold_due; always, with the default hold); a held step writes status DGSQP_HELD and zero
// counts, forms no estimate, and feeds stage 0 of the warm start it holds to the plant; the next warm start is dev_hold_next's.
// With a plant of ANOTHER CLASS (DgCrossPack) the plant's own state z is fed back next to q, q[t+1][b] = p(z[t+1][b]), and a chain
// ends on a non-finite entry of z[t+1][b].
// Channel j of the command that entered agent a's plant at the step whose records start tb_b scenarios in: stage 0 of the solution u_t,
// or with a plant what dev_plant_feedback stored in u_cmd.
__device__ inline double dev_command(int64_t, int a, int j, const double* u_t) { return u_t[am_col(dg_prob, a, 0, j)]; }
__device__ inline double dev_command(const DgPlantPack& pk, int64_t tb_b, int a, int j, const double* u_t) {
  return pk.u_cmd ? pk.u_cmd[tb_b * dg_prob.nu + a * DGSQP_NUA + j] : u_t[am_col(dg_prob, a, 0, j)];      // (no record asked for: every agent is GAME)
}
// a TRACK agent's command is in the plant's units: the game's rate rows are measured against the GAME's command for that agent
__device__ inline double dev_command(const DgCrossPack& xp, int64_t tb_b, int a, int j, const double*) {
  const int kind = xp.kind[(tb_b % xp.B) * dg_prob.M + a];
  return (kind == DGSQP_DRIVER_TRACK ? xp.u_game : xp.u_cmd)[tb_b * dg_prob.nu + a * DGSQP_NUA + j];
}

template <class... PLANT>
__global__ void __launch_bounds__(DG_BLOCK, 2)
dg_closed_loop_kernel(int64_t B, DgClosedLoop cl, double* __restrict__ ws_all, unsigned long long* __restrict__ ticket, PLANT... pd) {
  static_assert(sizeof...(PLANT) <= 1, "at most one plant");
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
      if constexpr (sizeof...(PLANT) != 0)
        if (!dev_hold_due(pd..., t)) {
          // a HELD step: no estimate and no solve; the plan the chain holds feeds the plant, and the step ends as every step does below
          if (TID == 0) { O.status[b] = DGSQP_HELD; O.iters[b] = 0; O.qp_solves[b] = 0; }
          int bad = dev_plant_feedback(pd..., 0, DGSQP_HELD, uws_t, t, tb + b, cl.q + (tb + b) * nq, uws_t, cl.w ? cl.w + (tb + b) * nq : nullptr,
                                       cl.q + (tb + B + b) * nq);
          t++;
          if (__syncthreads_or(bad)) break;
          dev_hold_next(pd..., 0, DGSQP_HELD, uws_t, uws_t, cl.uws + (tb + B + b) * n);
          if (cl.up && t < cl.T && TID < dg_prob.M)
            for (int j = 0; j < DGSQP_NUA; j++)
              cl.up[(tb + B + b) * dg_prob.nu + TID * DGSQP_NUA + j] = dev_command(pd..., tb + b, TID, j, uws_t);
          __threadfence_block();
          __syncthreads();
          continue;
        }
      if constexpr (sizeof...(PLANT) != 0) {
        const double* x0 = nullptr;
        if (dev_estimate(pd..., tb + b, cl.q + (tb + b) * nq, &x0)) break;
        c.x0 = (cgptr)x0;
      }
      else c.x0 = (cgptr)(cl.q + (tb + b) * nq);
      c.up = cl.up ? (cgptr)(cl.up + (tb + b) * dg_prob.nu) : (cgptr)cl.up_zero;
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
      if constexpr (sizeof...(PLANT) != 0) bad = dev_plant_feedback(pd..., 1, status, uws_t, t, tb + b, cl.q + (tb + b) * nq, u_t, w_t, q_next);
      else
        for (int i = TID; i < nq; i += NT) {
          double v = x1[i];
          if (w_t) v = v + w_t[i];
          q_next[i] = v;
          bad |= !isfinite(v);
        }
      t++;
      if (__syncthreads_or(bad)) break;                     // the chain ends: q[t] shows why, its warm start is never written
      if constexpr (sizeof...(PLANT) != 0) dev_hold_next(pd..., 1, status, uws_t, u_t, uws_next);
      else
        for (int i = TID; i < n; i += NT) {
          const int k = (i % (N * DGSQP_NUA)) / DGSQP_NUA;    // agent-major: agent a holds rows k = 0 .. N-1 of DGSQP_NUA inputs
          uws_next[i] = keep ? uws_t[i] : u_t[k + 1 < N ? i + DGSQP_NUA : i];
        }
      // carry: the command that entered each agent's plant at this step is the next solve's u_{-1} -- stage 0 of u_t as returned (also after
      // 'diverged' / 'qp_fail': the feedback applied it), or with drivers u_cmd[t][b], read back by the lane that stored it.  With delay
      // lines it is the value appended to the line, not the delayed one the plant integrated under.
      if (cl.up && t < cl.T && TID < dg_prob.M)
        for (int j = 0; j < DGSQP_NUA; j++)
          cl.up[(tb + B + b) * dg_prob.nu + TID * DGSQP_NUA + j] = dev_command(pd..., tb + b, TID, j, u_t);
      // the next dev_solve of this workgroup reads q_next / uws_next through ordinary loads
      __threadfence_block();
      __syncthreads();
    }
    if (TID == 0) cl.steps_done[b] = t;
  }
}
