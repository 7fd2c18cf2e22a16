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

// A plant of its own (dgsqp_set_plant; reference DGSQP/dynamics/dynamics_simulator.py:11-40): after every solve the state is advanced by
// S simulation steps of length dt / S of a model with the plant's vehicle parameters and integrator, every input channel behind a delay
// line.  `lines` is written and read back by the same lane of the same workgroup: a plain pointer like q and uws.
struct DgPlantDev {
  const dgsqp_plant_t* P;   // resolved by the host: agents[] hold the game's records when the plant uses the game's parameters
  double* lines;            // [grid][DGSQP_MAX_AGENTS][DGSQP_NUA][DGSQP_MAX_DELAY]  one set per workgroup, cleared when a chain starts
  double* u_plant;          // [T][B][S][nu]  the inputs the plant integrated under
};

// The further settings of a launch with a plant (dgsqp_set_plant_ensemble, dgsqp_set_estimate_noise, dgsqp_set_monitor): the pack type of
// the third instantiation of dg_closed_loop_kernel.  A launch that uses none of them is handed a DgPlantDev and runs what it always ran.
struct DgEnsembleDev {
  DgPlantDev pd;
  int64_t B;                          // chains of the launch: records are indexed by the CHAIN b, never by the workgroup
  const dgsqp_vehicle_t* vehicles;    // [B][M] chain b's vehicle records, or null (every chain runs pd.P)
  const int32_t* delay;               // [B][M][DGSQP_NUA] chain b's delays, or null (pd.P's)
  dgsqp_plant_t* wg_plant;            // [grid] the plant of the chain a workgroup carries: filled when the chain starts (with vehicles only)
  const double* v;                    // [T][B][nq] estimate noise, or null (the solves start from the true state)
  double* q_est;                      // [T][B][nq] q + v, what solve t starts from
  int monitor;                        // 0 off, 1 record, 2 record and stop
  double* mon_scratch;                // [grid][S][M][3] per simulation step and agent: position (2), the agent's own box excess
  double* clearance;                  // [T][B]
  double* box_excess;                 // [T][B]
  int32_t* hit_step;                  // [B], -1 until the chain's first hit
};

// Drivers (dgsqp_set_drivers): who produces the command entering agent a's plant at control step t of chain b -- the game (stage 0 of its
// solution), the lane follower dev_pid_law closed-loop on the TRUE state, or the caller's u_replay.  The pack of the fourth instantiation of
// dg_closed_loop_kernel; it wraps DgEnsembleDev, so the further settings combine with drivers.  cmd and pid_state are written and read by
// the same lane (lane a for agent a), like lines: plain pointers.  The NAME matters: LDS kernel ids follow the mangled kernel names, and this
// one sorts behind dg_closed_loop_kernel<DgEnsembleDev>, which so keeps its id and with it its register allocation.  To check after a rename:
// compile --offload-device-only -S before and after (same -cuid, also -DDG_BLOCK=256); that kernel's instructions must not change.
struct DgPlantDriversDev {
  DgEnsembleDev ex;
  const int32_t* kind;                // [B][M] DGSQP_DRIVER_*
  const dgsqp_pid_t* pid;             // [M] the gains of agent a's lane follower (read for PID agents)
  const double* ref;                  // [B][M][2] (v_ref, lat_ref), or null: from the chain's x0 = q[0][b], as the warm-start PID does
  const double* u_replay;             // [T][B][nu], or null (no REPLAY agent)
  double* u_cmd;                      // [T][B][nu] the command each agent's plant received
  double* cmd;                        // [grid][n] the workgroup's commands where the plant step reads stage 0 of u_t (agent-major)
  double* pid_state;                  // [grid][M][3] ei, previous u_a, previous u_steer: cleared when a chain starts
};

// A held plan (dgsqp_set_plan_hold; the table in include/dgsqp.h): a chain solves only when a plan is due and otherwise consumes the warm
// start it holds, stage by stage.  The pack of the fifth instantiation of dg_closed_loop_kernel; it wraps DgPlantDriversDev (a launch
// without drivers of the caller's runs with all-GAME kinds, which the host layer builds), so every other setting combines with it.  The
// game's command goes to u_game[t][b] and to the workgroup's gcmd, where the drivers' feedback reads stage 0 of u_t; gcmd is written and
// read by the same lane, like cmd.  state holds the chain's (age, due): written by lane 0, read by every lane after a fence and a barrier.
// The NAME (see DgPlantDriversDev): the namespace makes this instantiation sort behind ALL the others in the mangled kernel names -- a
// nested name mangles as N...E, and 'N' follows every digit and the 'E' that closes the empty pack of dg_closed_loop_kernel<> -- so every
// one of them keeps its LDS kernel id.
namespace dg_hold {
struct DgPlantDriversHoldDev {
  DgPlantDriversDev dd;
  int32_t replan_every, on_fail;      // R; DGSQP_HOLD_*
  uint32_t fail_mask;                 // bit s: status s is a failed solve
  double* u_game;                     // [T][B][nu] the game's command: stage 0 of the step's solution, or of the plan it holds
  int32_t* plan_stage;                // [T][B] how many stages of its plan the chain had consumed before u_game[t][b]
  double* gcmd;                       // [grid][n] (2 M used: read as u_t is)
  int32_t* state;                     // [grid][2] age, due: set to (0, 1) when a chain starts
};
}
using dg_hold::DgPlantDriversHoldDev;

// A plant of ANOTHER model class than the game's (dgsqp_set_cross_plant): the plant keeps a state z of its own, [T+1][B][nz], fed back
// like q by the lane that wrote it, and the game sees the projection q = p(z) -- entry i of agent a's block of q is entry proj[a][i] of
// its block of z.  The pack of the sixth instantiation of dg_closed_loop_kernel; it wraps DgPlantDriversHoldDev (the host layer builds
// all-GAME kinds and the default hold when the caller gives none), so every other setting combines with it.  `lift` is the game with
// every agent's state bounds moved to the plant's layout (+-inf on entries the game does not see): what the monitor of dev_plant_agent
// reads when it integrates a z block; `game` is the game as a plant (its integrator and sub-steps, one simulation step, no delay): one
// step of it from p(z) under the game's command is the reference a TRACK driver follows.
// The NAME (see DgPlantDriversDev, dg_hold): N9dg_xplant... sorts behind N7dg_hold..., so this instantiation is the last one.
namespace dg_xplant {
struct DgCrossPlantDev {
  dg_hold::DgPlantDriversHoldDev hd;
  int32_t mdl[DGSQP_MAX_AGENTS], nz[DGSQP_MAX_AGENTS], zoff[DGSQP_MAX_AGENTS];      // the plant agents' classes, state counts, offsets in z
  int32_t nz_all;                                                                   // their sum
  int8_t proj[DGSQP_MAX_AGENTS][DGSQP_MAX_NQA];
  const dgsqp_problem_t* lift;
  const dgsqp_plant_t* game;
  double* z;                          // [T+1][B][nz_all] slice 0 = z0, slice t + 1 = the plant's state after step t
  double* track_ref;                  // [T][B][M][3] (v_ref, lat_ref, epsi_ref) of the TRACK agents
};
}
using dg_xplant::DgCrossPlantDev;

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
// length d: read [0], append); d = 0 integrates under u_new.  One plant step is dev_fd_t's arithmetic on f_c with the plant's agent
// record, step length and sub-step count (euler: one step per simulation step, as the game's model).
// MON with a non-null `mon` ([S][M][3], the workgroup's): the agent's monitor record after every simulation step (dev_monitor_store).
template <int MDL, bool SPL, bool MON = false>
__device__ inline void dev_plant_agent(const dgsqp_problem_t& P, const dgsqp_plant_t& pl, int a, int64_t count, const double* u_new,
                                       double* line, double* u_rec, int nu, double* qa, double* mon = nullptr) {
  typedef Ty<0> T;
  const dgsqp_agent_t& ag = pl.agents[a];
  const int S = pl.sim_steps, integ = pl.integrator, nsub = integ == DGSQP_INT_EULER ? 1 : pl.substeps;
  const double hs = P.dt / S, h = hs / nsub;
  constexpr int NQA = dg_model_nq(MDL);
  T x[NQA], k1[NQA], k2[NQA], t[NQA], u[DGSQP_NUA];
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
    for (int m = 0; m < nsub; m++) {
      dev_fc<0, MDL, SPL>(P, ag, x, u, pre, k1);
      if (integ == DGSQP_INT_RK4) {
#pragma unroll
        for (int i = 0; i < NQA; i++) t[i] = x[i] + k1[i] * (h / 2);
        dev_fc<0, MDL, SPL>(P, ag, t, u, pre, k2);
#pragma unroll
        for (int i = 0; i < NQA; i++) { t[i] = x[i] + k2[i] * (h / 2); k1[i] = k1[i] + k2[i] * 2.0; }
        dev_fc<0, MDL, SPL>(P, ag, t, u, pre, k2);
#pragma unroll
        for (int i = 0; i < NQA; i++) { t[i] = x[i] + k2[i] * h; k1[i] = k1[i] + k2[i] * 2.0; }
        dev_fc<0, MDL, SPL>(P, ag, t, u, pre, k2);
#pragma unroll
        for (int i = 0; i < NQA; i++) x[i] = x[i] + (k1[i] + k2[i]) * (h / 6.0);
      } else if (integ == DGSQP_INT_RK3) {
#pragma unroll
        for (int i = 0; i < NQA; i++) { k1[i] = k1[i] * h; t[i] = x[i] + k1[i] * 0.5; }
        dev_fc<0, MDL, SPL>(P, ag, t, u, pre, k2);
#pragma unroll
        for (int i = 0; i < NQA; i++) { k2[i] = k2[i] * h; t[i] = x[i] - k1[i] + k2[i] * 2.0; }
        T k3[NQA];
        dev_fc<0, MDL, SPL>(P, ag, t, u, pre, k3);
#pragma unroll
        for (int i = 0; i < NQA; i++) x[i] = x[i] + (k1[i] + k2[i] * 4.0 + k3[i] * h) / 6.0;
      } else if (integ == DGSQP_INT_RK2) {
#pragma unroll
        for (int i = 0; i < NQA; i++) t[i] = x[i] + k1[i] * h;
        dev_fc<0, MDL, SPL>(P, ag, t, u, pre, k2);
#pragma unroll
        for (int i = 0; i < NQA; i++) x[i] = x[i] + (k1[i] + k2[i]) * (h / 2);
      } else {
#pragma unroll
        for (int i = 0; i < NQA; i++) x[i] = x[i] + k1[i] * hs;
      }
    }
    if constexpr (MON)
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

// The plant's feedback of step t of chain b on the lane of agent a = TID < M: q_next = plant(q_t, stage 0 of u_t) (+ w_t) with the plant
// `pl`.  Returns 1 when the lane's part of q_next is not finite, else 0.  `lines` and `u_plant` as in DgPlantDev, `mon` as in
// dev_plant_agent; its record of the last simulation step is stored here, after w_t: that state is q_next.
template <bool MON>
__device__ inline int dev_plant_step(const dgsqp_plant_t& pl, double* lines, double* u_plant, int t, int64_t tb_b, const double* q_t,
                                     const double* u_t, const double* w_t, double* q_next, double* mon) {
  const DgProb& D = dg_prob;
  const int a = TID;
  const int S = pl.sim_steps, nqa = D.nqa[a], qo = D.qoff[a];
  double* line = lines + ((int64_t)blockIdx.x * DGSQP_MAX_AGENTS + a) * (DGSQP_NUA * DGSQP_MAX_DELAY);
  if (t == 0)
    for (int i = 0; i < DGSQP_NUA * DGSQP_MAX_DELAY; i++) line[i] = 0.0;      // every chain starts with empty (zero) lines
  double u_new[DGSQP_NUA], qa[DGSQP_MAX_NQA];
  for (int j = 0; j < DGSQP_NUA; j++) u_new[j] = u_t[am_col(D, a, 0, j)];
  for (int i = 0; i < DGSQP_MAX_NQA; i++) qa[i] = i < nqa ? q_t[qo + i] : 0.0;
  double* u_rec = u_plant + tb_b * S * D.nu + a * DGSQP_NUA;
  const int64_t count = (int64_t)t * S;
  const int mdl = D.mdl[a];      // the plant's agent is of the game's model class (dgsqp_set_plant refuses any other)
  if (mdl == DG_UNI) dev_plant_agent<DG_UNI, false, MON>(D.P, pl, a, count, u_new, line, u_rec, D.nu, qa, mon);
  else if (mdl == DG_PM) dev_plant_agent<DG_PM, false, MON>(D.P, pl, a, count, u_new, line, u_rec, D.nu, qa, mon);
  else if (D.P.track_kind == DGSQP_TRACK_SPLINE) {
    if (mdl == DG_DYN) dev_plant_agent<DG_DYN, true, MON>(D.P, pl, a, count, u_new, line, u_rec, D.nu, qa, mon);
    else dev_plant_agent<DG_KIN, true, MON>(D.P, pl, a, count, u_new, line, u_rec, D.nu, qa, mon);
  }
  else if (mdl == DG_DYN) dev_plant_agent<DG_DYN, false, MON>(D.P, pl, a, count, u_new, line, u_rec, D.nu, qa, mon);
  else dev_plant_agent<DG_KIN, false, MON>(D.P, pl, a, count, u_new, line, u_rec, D.nu, qa, mon);
  int bad = 0;
  for (int i = 0; i < DGSQP_MAX_NQA; i++)
    if (i < nqa) {
      double v = qa[i];
      if (w_t) v = v + w_t[qo + i];
      q_next[qo + i] = v;
      bad |= !isfinite(v);
      if constexpr (MON) qa[i] = v;
    }
  if constexpr (MON)
    if (mon) dev_monitor_store(D.P.agents[a], nqa, qa, mon + ((int64_t)(S - 1) * D.M + a) * 3);
  return bad;
}

// The plant's feedback of step t of chain b, one lane per agent: q_next = plant(q_t, stage 0 of u_t) (+ w_t).  Returns non-zero on the
// lanes whose part of q_next is not finite.  Out of line: the solve that is inlined next to the call keeps its register allocation.
// The caller has fenced the solve's records (u_t); q_t was written by this very lane one step ago, or by the host.
__device__ __noinline__ int dev_plant_feedback(DgPlantDev pd, int t, int64_t tb_b, const double* q_t, const double* u_t, const double* w_t,
                                               double* q_next) {
  if (TID >= dg_prob.M) return 0;
  return dev_plant_step<false>(*pd.P, pd.lines, pd.u_plant, t, tb_b, q_t, u_t, w_t, q_next, nullptr);
}

// The same feedback with the further settings (DgEnsembleDev); every lane of the workgroup calls it.  Chain b's plant: the vehicle
// records and delays of CHAIN b, copied into the workgroup's own dgsqp_plant_t when the chain starts -- lane a its agent's, lane 0 the
// shared scalars -- exactly where the delay lines are cleared; the copy is read back after a fence and a barrier.  With the monitor on,
// lane a leaves its records of the S simulation steps in the workgroup's scratch; after another fence and barrier lane 0 reduces the
// pairs and writes clearance, box_excess and hit_step.  The return value also ends the chain (from lane 0, as 1: every
// feedback returns 0 or 1) after a hit in mode 2.
__device__ __noinline__ int dev_plant_feedback(DgEnsembleDev ex, int t, int64_t tb_b, const double* q_t, const double* u_t, const double* w_t,
                                               double* q_next) {
  const DgProb& D = dg_prob;
  const int a = TID, M = D.M;
  const int64_t b = tb_b - (int64_t)t * ex.B;
  const dgsqp_plant_t* pl = ex.pd.P;
  if (ex.vehicles) {
    dgsqp_plant_t* mine = ex.wg_plant + blockIdx.x;
    if (t == 0) {
      if (a == 0) { mine->integrator = pl->integrator; mine->substeps = pl->substeps; mine->sim_steps = pl->sim_steps; mine->use_game_agents = 0; }
      if (a < M) {
        __builtin_memcpy(&mine->agents[a], &ex.vehicles[b * M + a], sizeof(dgsqp_vehicle_t));      // (the vehicle prefix of dgsqp_agent_t)
        for (int ch = 0; ch < DGSQP_NUA; ch++) mine->delay[a][ch] = ex.delay ? ex.delay[(b * M + a) * DGSQP_NUA + ch] : pl->delay[a][ch];
      }
      __threadfence_block();
      __syncthreads();
    }
    pl = mine;
  }
  const int S = pl->sim_steps;
  double* mon = ex.monitor ? ex.mon_scratch + (int64_t)blockIdx.x * S * M * 3 : nullptr;
  int bad = 0;
  if (a < M) bad = dev_plant_step<true>(*pl, ex.pd.lines, ex.pd.u_plant, t, tb_b, q_t, u_t, w_t, q_next, mon);
  if (!mon) return bad;
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
          const double d = sqrt(dx * dx + dy * dy) - (D.P.agents[i].radius + D.P.agents[k].radius);
          cl = fmin(cl, d);
          if (d < 0.0 && hit < 0) hit = j;
        }
      }
    ex.clearance[tb_b] = fin ? cl : NAN;
    ex.box_excess[tb_b] = fin ? bx : NAN;
    if (hit >= 0) {
      if (ex.hit_step[b] < 0) ex.hit_step[b] = t * S + hit;
      if (ex.monitor == 2) bad = 1;
    }
  }
  return bad;
}

// The same feedback with drivers: lane a < M forms its agent's command, stores it to u_cmd[t][b] and to the workgroup's cmd, which is then
// handed to the feedback above in place of u_t -- everything downstream of the command (delay lines, the S simulation steps, u_plant, the
// monitor) is that function's.  The PID driver reads the TRUE state q_t, also when the solves start from estimates; its dt is the control
// step; its state is cleared where the delay lines are (t == 0), so a workgroup's next chain starts from zero like every other.
__device__ __noinline__ int dev_plant_feedback(DgPlantDriversDev dd, int t, int64_t tb_b, const double* q_t, const double* u_t, const double* w_t,
                                               double* q_next) {
  const DgProb& D = dg_prob;
  const int a = TID, M = D.M;
  double* cmd = dd.cmd + (int64_t)blockIdx.x * D.n;
  if (a < M) {
    const int64_t b = tb_b - (int64_t)t * dd.ex.B;
    const int kind = dd.kind[b * M + a];
    double* st = dd.pid_state + ((int64_t)blockIdx.x * M + a) * 3;
    if (t == 0) { st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; }
    double c[DGSQP_NUA];
    if (kind == DGSQP_DRIVER_PID) {
      const int nqa = D.nqa[a], epsi = nqa == 8 ? 5 : 3, ey = nqa - 1;        // (state layout: dev_pid_agent)
      const double* qa = q_t + D.qoff[a];
      const double* q0 = qa - (int64_t)t * dd.ex.B * D.nq;                     // the chain's x0: slice 0 of q
      const double* ref = dd.ref ? dd.ref + (b * M + a) * 2 : nullptr;
      const double v_ref = ref ? ref[0] : q0[2], lat_ref = ref ? ref[1] : q0[ey];
      double ei = st[0], up0 = st[1], up1 = st[2];
      dev_pid_law(dd.pid[a], D.P.dt, qa[2], v_ref, qa[ey], lat_ref, qa[epsi], ei, up0, up1);
      st[0] = ei; st[1] = up0; st[2] = up1;
      c[0] = up0; c[1] = up1;
    }
    else if (kind == DGSQP_DRIVER_REPLAY)
      for (int j = 0; j < DGSQP_NUA; j++) c[j] = dd.u_replay[tb_b * D.nu + a * DGSQP_NUA + j];
    else
      for (int j = 0; j < DGSQP_NUA; j++) c[j] = u_t[am_col(D, a, 0, j)];
    for (int j = 0; j < DGSQP_NUA; j++) {
      dd.u_cmd[tb_b * D.nu + a * DGSQP_NUA + j] = c[j];
      cmd[am_col(D, a, 0, j)] = c[j];
    }
  }
  return dev_plant_feedback(dd.ex, t, tb_b, q_t, cmd, w_t, q_next);
}

// A held plan: which row of the table (include/dgsqp.h) step t falls under, from whether it solved and the solve's status.
enum { DG_HOLD_ACCEPT = 0, DG_HOLD_KEEP = 1, DG_HOLD_CONSUME = 2 };
__device__ inline int dev_hold_rule(const DgPlantDriversHoldDev& hd, int solved, int status) {
  if (!solved) return DG_HOLD_CONSUME;
  if (status < 0 || status > 5 || !((hd.fail_mask >> status) & 1u)) return DG_HOLD_ACCEPT;
  return hd.on_fail == DGSQP_HOLD_HOLD ? DG_HOLD_CONSUME : DG_HOLD_KEEP;
}

// Whether step t of the workgroup's chain solves.  (age, due) is reset where the delay lines and the PID state are (t == 0); afterwards it
// is what dev_hold_next left, behind the fence and barrier that end a step.  The same value on every lane: the branch on it is uniform.
__device__ __noinline__ int dev_hold_due(DgPlantDriversHoldDev hd, int t) {
  int32_t* st = hd.state + (int64_t)blockIdx.x * 2;
  if (t == 0) {
    if (TID == 0) { st[0] = 0; st[1] = 1; }
    __threadfence_block();
    __syncthreads();
  }
  return __builtin_amdgcn_readfirstlane(st[1]);
}

// The feedback with a held plan: lane a < M stores the game's command for its agent -- stage 0 of the solution u_t, or of the warm start
// uws_t the chain holds -- to u_game[t][b] and to the workgroup's gcmd, lane 0 plan_stage; gcmd is then handed to the drivers' feedback in
// place of u_t.  uws_t was written one step ago behind a fence and a barrier (or by the host), age by this very lane.
__device__ __noinline__ int dev_plant_feedback(DgPlantDriversHoldDev hd, int solved, int status, const double* uws_t, int t, int64_t tb_b,
                                               const double* q_t, const double* u_t, const double* w_t, double* q_next) {
  const DgProb& D = dg_prob;
  const int a = TID;
  double* g = hd.gcmd + (int64_t)blockIdx.x * D.n;
  if (a < D.M) {
    const int rule = dev_hold_rule(hd, solved, status);
    const double* src = rule == DG_HOLD_CONSUME ? uws_t : u_t;
    for (int j = 0; j < DGSQP_NUA; j++) {
      const double v = src[am_col(D, a, 0, j)];
      hd.u_game[tb_b * D.nu + a * DGSQP_NUA + j] = v;
      g[am_col(D, a, 0, j)] = v;
    }
    if (a == 0) hd.plan_stage[tb_b] = rule == DG_HOLD_CONSUME ? hd.state[(int64_t)blockIdx.x * 2] : 0;
  }
  return dev_plant_feedback(hd.dd, t, tb_b, q_t, g, w_t, q_next);
}

// The next warm start with a held plan and the chain's (age, due) after the step; every lane of the workgroup calls it, after the barrier
// that decided that the chain goes on (so every lane has read `due` of this step).
__device__ __noinline__ void dev_hold_next(DgPlantDriversHoldDev hd, int solved, int status, const double* uws_t, const double* u_t, double* uws_next) {
  const int n = dg_prob.n, N = dg_prob.N;
  const int rule = dev_hold_rule(hd, solved, status);
  const double* src = rule == DG_HOLD_ACCEPT ? u_t : uws_t;
  for (int i = TID; i < n; i += NT) {
    const int k = (i % (N * DGSQP_NUA)) / DGSQP_NUA;
    uws_next[i] = rule == DG_HOLD_KEEP ? uws_t[i] : src[k + 1 < N ? i + DGSQP_NUA : i];
  }
  if (TID == 0) {
    int32_t* st = hd.state + (int64_t)blockIdx.x * 2;
    if (rule == DG_HOLD_ACCEPT) { st[0] = 1; st[1] = 1 >= hd.replan_every; }
    else if (rule == DG_HOLD_CONSUME) {
      const int age = st[0] + 1;
      st[0] = age;
      if (!solved) st[1] = age >= hd.replan_every;
    }
  }
}

// The state solve t of chain b starts from.  With estimates: the lanes write q_est[t][b] = q[t][b] + v[t][b], and the slice is handed to
// the solve through memory (fence + barrier) like every other state; returns non-zero when it is not finite (the chain ends before
// the solve).  Out of line, as the feedback.
__device__ __noinline__ int dev_estimate(DgEnsembleDev ex, int64_t tb_b, const double* q_t, const double** x0) {
  if (!ex.v) { *x0 = q_t; return 0; }
  const int nq = dg_prob.nq;
  double* qe = ex.q_est + tb_b * nq;
  const double* v = ex.v + tb_b * nq;
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

__device__ __noinline__ int dev_estimate(DgPlantDriversDev dd, int64_t tb_b, const double* q_t, const double** x0) {
  return dev_estimate(dd.ex, tb_b, q_t, x0);
}
__device__ __noinline__ int dev_estimate(DgPlantDriversHoldDev hd, int64_t tb_b, const double* q_t, const double** x0) {
  return dev_estimate(hd.dd.ex, tb_b, q_t, x0);
}

// ---- a plant of another model class (DgCrossPlantDev) ----
// One step of the GAME's discrete model for agent a from x (in place) under g: the game as a plant has no delay (the line is never
// touched) and one simulation step, whose input record goes to a local.
// P is the pack's copy of the game (`lift`: step, integrator and track are the game's; the bounds are not read here).
__device__ inline void dev_cross_game_step(const dgsqp_problem_t& P, const dgsqp_plant_t& game, int a, const double* g, double* x) {
  double rec[DGSQP_NUA];
  const int mdl = dg_prob.mdl[a];
  if (mdl == DG_PM) dev_plant_agent<DG_PM, false>(P, game, a, 0, g, nullptr, rec, DGSQP_NUA, x);
  else if (P.track_kind == DGSQP_TRACK_SPLINE) {
    if (mdl == DG_DYN) dev_plant_agent<DG_DYN, true>(P, game, a, 0, g, nullptr, rec, DGSQP_NUA, x);
    else dev_plant_agent<DG_KIN, true>(P, game, a, 0, g, nullptr, rec, DGSQP_NUA, x);
  }
  else if (mdl == DG_DYN) dev_plant_agent<DG_DYN, false>(P, game, a, 0, g, nullptr, rec, DGSQP_NUA, x);
  else dev_plant_agent<DG_KIN, false>(P, game, a, 0, g, nullptr, rec, DGSQP_NUA, x);
}

// The feedback with a plant of another class, one lane per agent; every lane of the workgroup calls it.  Lane a < M, in this order:
// the game's command (the hold overload's rule) to u_game[t][b]; its driver's command to u_cmd[t][b] -- PID and REPLAY read and command the
// PLANT's agent, TRACK is dev_pid_law towards one step of the game's model from p(z_t) under the game's command (track_ref[t][b][a]);
// the S simulation steps of its block of z with the plant's class (dev_plant_agent: delay lines, u_plant, the monitor's records against
// `lift`); z[t+1][b] and q[t+1][b] = p(z[t+1][b]).  Returns non-zero when z[t+1] is not finite (or, from lane 0, after a hit in mode 2).
// The chain's plant and the monitor's reduction are those of the DgEnsembleDev overload, restated: that function keeps its code.
__device__ __noinline__ int dev_plant_feedback(DgCrossPlantDev xp, int solved, int status, const double* uws_t, int t, int64_t tb_b,
                                               const double* q_t, const double* u_t, const double* w_t, double* q_next) {
  const DgProb& D = dg_prob;
  const DgPlantDriversHoldDev& hd = xp.hd;
  const DgPlantDriversDev& dd = hd.dd;
  const DgEnsembleDev& ex = dd.ex;
  const dgsqp_problem_t& L = *xp.lift;      // the game, read through the pack: bounds in the plant's layout, everything else the game's
  const int a = TID, M = D.M;
  const int64_t b = tb_b - (int64_t)t * ex.B;
  const dgsqp_plant_t* pl = ex.pd.P;
  if (ex.vehicles) {
    dgsqp_plant_t* mine = ex.wg_plant + blockIdx.x;
    if (t == 0) {
      if (a == 0) { mine->integrator = pl->integrator; mine->substeps = pl->substeps; mine->sim_steps = pl->sim_steps; mine->use_game_agents = 0; }
      if (a < M) {
        __builtin_memcpy(&mine->agents[a], &ex.vehicles[b * M + a], sizeof(dgsqp_vehicle_t));
        for (int ch = 0; ch < DGSQP_NUA; ch++) mine->delay[a][ch] = ex.delay ? ex.delay[(b * M + a) * DGSQP_NUA + ch] : pl->delay[a][ch];
      }
      __threadfence_block();
      __syncthreads();
    }
    pl = mine;
  }
  const int S = pl->sim_steps;
  double* mon = ex.monitor ? ex.mon_scratch + (int64_t)blockIdx.x * S * M * 3 : nullptr;
  int bad = 0;
  if (a < M) {
    const int nqa = D.nqa[a], nza = xp.nz[a];
    const int8_t* pr = xp.proj[a];
    const double* za = xp.z + tb_b * xp.nz_all + xp.zoff[a];             // written by this very lane one step ago, or by the host
    double* zn = xp.z + (tb_b + ex.B) * xp.nz_all + xp.zoff[a];
    // 1. the game's command, and the driver's
    const int rule = dev_hold_rule(hd, solved, status);
    const double* src = rule == DG_HOLD_CONSUME ? uws_t : u_t;
    double g[DGSQP_NUA], c[DGSQP_NUA];
    for (int j = 0; j < DGSQP_NUA; j++) {
      g[j] = src[am_col(D, a, 0, j)];
      hd.u_game[tb_b * D.nu + a * DGSQP_NUA + j] = g[j];
    }
    if (a == 0) hd.plan_stage[tb_b] = rule == DG_HOLD_CONSUME ? hd.state[(int64_t)blockIdx.x * 2] : 0;
    const int kind = dd.kind[b * M + a];
    double* st = dd.pid_state + ((int64_t)blockIdx.x * M + a) * 3;
    if (t == 0) { st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; }
    if (kind == DGSQP_DRIVER_PID || kind == DGSQP_DRIVER_TRACK) {
      const int epsi = nza == 8 ? 5 : 3, ey = nza - 1;                  // (the PLANT's layout)
      double v_ref, lat_ref, epsi_ref = 0.0;
      if (kind == DGSQP_DRIVER_TRACK) {
        double xr[DGSQP_MAX_NQA];
        for (int i = 0; i < DGSQP_MAX_NQA; i++) xr[i] = i < nqa ? za[pr[i]] : 0.0;
        dev_cross_game_step(L, *xp.game, a, g, xr);
        v_ref = xr[2]; lat_ref = xr[nqa - 1]; epsi_ref = xr[nqa == 8 ? 5 : 3];      // (the GAME's layout)
        double* tr = xp.track_ref + (tb_b * M + a) * 3;
        tr[0] = v_ref; tr[1] = lat_ref; tr[2] = epsi_ref;
      } else {
        const double* z0 = za - (int64_t)t * ex.B * xp.nz_all;            // the chain's z0: slice 0 of z
        const double* ref = dd.ref ? dd.ref + (b * M + a) * 2 : nullptr;
        v_ref = ref ? ref[0] : z0[2]; lat_ref = ref ? ref[1] : z0[ey];
      }
      double ei = st[0], up0 = st[1], up1 = st[2];
      dev_pid_law(dd.pid[a], L.dt, za[2], v_ref, za[ey], lat_ref, kind == DGSQP_DRIVER_TRACK ? za[epsi] - epsi_ref : za[epsi], ei, up0, up1);
      st[0] = ei; st[1] = up0; st[2] = up1;
      c[0] = up0; c[1] = up1;
    }
    else if (kind == DGSQP_DRIVER_REPLAY)
      for (int j = 0; j < DGSQP_NUA; j++) c[j] = dd.u_replay[tb_b * D.nu + a * DGSQP_NUA + j];
    else
      for (int j = 0; j < DGSQP_NUA; j++) c[j] = g[j];
    for (int j = 0; j < DGSQP_NUA; j++) dd.u_cmd[tb_b * D.nu + a * DGSQP_NUA + j] = c[j];
    // 2. the S simulation steps of the agent's block of z
    double* line = ex.pd.lines + ((int64_t)blockIdx.x * DGSQP_MAX_AGENTS + a) * (DGSQP_NUA * DGSQP_MAX_DELAY);
    if (t == 0)
      for (int i = 0; i < DGSQP_NUA * DGSQP_MAX_DELAY; i++) line[i] = 0.0;
    double zz[DGSQP_MAX_NQA];
    for (int i = 0; i < DGSQP_MAX_NQA; i++) zz[i] = i < nza ? za[i] : 0.0;
    double* u_rec = ex.pd.u_plant + tb_b * S * D.nu + a * DGSQP_NUA;
    const int64_t count = (int64_t)t * S;
    const int mdl = xp.mdl[a];
    if (mdl == DG_UNI) dev_plant_agent<DG_UNI, false, true>(L, *pl, a, count, c, line, u_rec, D.nu, zz, mon);
    else if (mdl == DG_PM) dev_plant_agent<DG_PM, false, true>(L, *pl, a, count, c, line, u_rec, D.nu, zz, mon);
    else if (L.track_kind == DGSQP_TRACK_SPLINE) {
      if (mdl == DG_DYN) dev_plant_agent<DG_DYN, true, true>(L, *pl, a, count, c, line, u_rec, D.nu, zz, mon);
      else dev_plant_agent<DG_KIN, true, true>(L, *pl, a, count, c, line, u_rec, D.nu, zz, mon);
    }
    else if (mdl == DG_DYN) dev_plant_agent<DG_DYN, false, true>(L, *pl, a, count, c, line, u_rec, D.nu, zz, mon);
    else dev_plant_agent<DG_KIN, false, true>(L, *pl, a, count, c, line, u_rec, D.nu, zz, mon);
    // 3. z[t+1] and its projection (the monitor's record of the last simulation step is dev_plant_agent's: nothing is added to z)
    for (int i = 0; i < DGSQP_MAX_NQA; i++)
      if (i < nza) { zn[i] = zz[i]; bad |= !isfinite(zz[i]); }
    for (int i = 0; i < DGSQP_MAX_NQA; i++)
      if (i < nqa) q_next[D.qoff[a] + i] = zz[pr[i]];
  }
  if (!mon) return bad;
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
          const double d = sqrt(dx * dx + dy * dy) - (L.agents[i].radius + L.agents[k].radius);
          cl = fmin(cl, d);
          if (d < 0.0 && hit < 0) hit = j;
        }
      }
    ex.clearance[tb_b] = fin ? cl : NAN;
    ex.box_excess[tb_b] = fin ? bx : NAN;
    if (hit >= 0) {
      if (ex.hit_step[b] < 0) ex.hit_step[b] = t * S + hit;
      if (ex.monitor == 2) bad = 1;
    }
  }
  return bad;
}

__device__ __noinline__ int dev_hold_due(DgCrossPlantDev xp, int t) { return dev_hold_due(xp.hd, t); }
__device__ __noinline__ void dev_hold_next(DgCrossPlantDev xp, int solved, int status, const double* uws_t, const double* u_t, double* uws_next) {
  dev_hold_next(xp.hd, solved, status, uws_t, u_t, uws_next);
}
__device__ __noinline__ int dev_estimate(DgCrossPlantDev xp, int64_t tb_b, const double* q_t, const double** x0) {
  return dev_estimate(xp.hd.dd.ex, tb_b, q_t, x0);
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
// A non-finite q_est[t][b] (DgEnsembleDev with estimates) ends the chain BEFORE solve t: steps_done[b] = t.
// With a plant of ANOTHER CLASS (DgCrossPlantDev) the plant's own state z is fed back next to q, q[t+1][b] = p(z[t+1][b]), and a chain
// ends on a non-finite entry of z[t+1][b]; everything else is the held-plan instantiation's.
// PLANT is empty, one DgPlantDev, one DgEnsembleDev, one DgPlantDriversDev, one DgPlantDriversHoldDev, or one DgCrossPlantDev: the instantiation without a plant has
// the argument list it always had and holds nothing of the plant, the one with a DgPlantDev nothing of the further settings, the one with a
// DgEnsembleDev nothing of the drivers, the one with a DgPlantDriversDev nothing of the held plan.
// With a HELD PLAN (DgPlantDriversHoldDev; the table in include/dgsqp.h) step t solves only when a plan is due (dev_hold_due); a held step
// writes status DGSQP_HELD and zero counts, forms no estimate, and feeds stage 0 of the warm start it holds to the plant; the next warm
// start is dev_hold_next's.
// Channel j of the command that entered agent a's plant at the step whose records start tb_b scenarios in: stage 0 of the solution u_t,
// or with drivers what dev_plant_feedback stored in u_cmd.
__device__ inline double dev_command(int64_t, int a, int j, const double* u_t) { return u_t[am_col(dg_prob, a, 0, j)]; }
__device__ inline double dev_command(const DgPlantDev&, int64_t, int a, int j, const double* u_t) { return u_t[am_col(dg_prob, a, 0, j)]; }
__device__ inline double dev_command(const DgEnsembleDev&, int64_t, int a, int j, const double* u_t) { return u_t[am_col(dg_prob, a, 0, j)]; }
__device__ inline double dev_command(const DgPlantDriversDev& dd, int64_t tb_b, int a, int j, const double*) { return dd.u_cmd[tb_b * dg_prob.nu + a * DGSQP_NUA + j]; }
__device__ inline double dev_command(const DgPlantDriversHoldDev& hd, int64_t tb_b, int a, int j, const double*) { return hd.dd.u_cmd[tb_b * dg_prob.nu + a * DGSQP_NUA + j]; }
// a TRACK agent's command is in the plant's units: the game's rate rows are measured against the GAME's command for that agent
__device__ inline double dev_command(const DgCrossPlantDev& xp, int64_t tb_b, int a, int j, const double*) {
  const DgPlantDriversDev& dd = xp.hd.dd;
  const int kind = dd.kind[(tb_b % dd.ex.B) * dg_prob.M + a];
  return (kind == DGSQP_DRIVER_TRACK ? xp.hd.u_game : dd.u_cmd)[tb_b * dg_prob.nu + a * DGSQP_NUA + j];
}

template <class... PLANT> struct DgHasEstimates { static constexpr bool value = false; };
template <> struct DgHasEstimates<DgEnsembleDev> { static constexpr bool value = true; };
template <> struct DgHasEstimates<DgPlantDriversDev> { static constexpr bool value = true; };
template <> struct DgHasEstimates<DgPlantDriversHoldDev> { static constexpr bool value = true; };
template <> struct DgHasEstimates<DgCrossPlantDev> { static constexpr bool value = true; };
template <class... PLANT> struct DgHoldsPlan { static constexpr bool value = false; };
template <> struct DgHoldsPlan<DgPlantDriversHoldDev> { static constexpr bool value = true; };
template <> struct DgHoldsPlan<DgCrossPlantDev> { static constexpr bool value = true; };
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
      if constexpr (DgHoldsPlan<PLANT...>::value)
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
      if constexpr (DgHasEstimates<PLANT...>::value) {
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
      if constexpr (DgHoldsPlan<PLANT...>::value) bad = dev_plant_feedback(pd..., 1, status, uws_t, t, tb + b, cl.q + (tb + b) * nq, u_t, w_t, q_next);
      else if constexpr (sizeof...(PLANT) != 0) bad = dev_plant_feedback(pd..., t, tb + b, cl.q + (tb + b) * nq, u_t, w_t, q_next);
      else
        for (int i = TID; i < nq; i += NT) {
          double v = x1[i];
          if (w_t) v = v + w_t[i];
          q_next[i] = v;
          bad |= !isfinite(v);
        }
      t++;
      if (__syncthreads_or(bad)) break;                     // the chain ends: q[t] shows why, its warm start is never written
      if constexpr (DgHoldsPlan<PLANT...>::value) dev_hold_next(pd..., 1, status, uws_t, u_t, uws_next);
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
