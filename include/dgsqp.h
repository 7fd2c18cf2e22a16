/*
 * dgsqp.h -- C-ABI of the MI355X batched Dynamic-Game-SQP solver.
 *
 * This is the drop-in boundary for ONE hot path of zhu-edward/DGSQP: the
 * Monte-Carlo SQP inner loop `DGSQP.solve()` (reference
 * DGSQP/solvers/DGSQP.py:302-507) together with everything it calls per
 * sample (`_evaluate` :509-533, `_solve_qp` :232-266, `_nearestPD`
 * :1290-1296, `_get_mu` :559-585, `_line_search_3` :1057-1081,
 * `_watchdog_line_search_4` :1174-1288).
 *
 * The reference is pure Python; its "FFI" for this path is the set of CasADi
 * `Function.__call__`s and the `ca.conic` call made from `solve()`.  A
 * maintainer binds this library with `ctypes.CDLL`.
 * Only plain pointers, fixed-width integers and doubles cross the boundary.
 *
 * Because CasADi Function objects cannot cross a C boundary, the symbolic
 * game (dynamics / costs / constraints built by
 * scripts/DGSQP_*_monte_carlo_*.py) is passed as a declarative POD
 * description, `dgsqp_problem_t`.
 */
#ifndef DGSQP_H
#define DGSQP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGSQP_MAX_AGENTS 6
#define DGSQP_MAX_SEGS 16
#define DGSQP_MAX_NQA 8 /* largest per-agent state (dynamic bicycle) */
#define DGSQP_NUA 2     /* every vehicle model of the path has 2 inputs */

/* dynamics model ids (reference: DGSQP/dynamics/dynamics_models.py) */
enum {
  DGSQP_MODEL_KIN_BICYCLE = 0, /* CasadiKinematicBicycleCombined :997  */
  DGSQP_MODEL_DYN_BICYCLE = 1, /* CasadiDynamicBicycleCombined   :1945 */
  DGSQP_MODEL_UNICYCLE = 2,    /* CasadiKinematicUnicycle        :306 : state [x, y, v, psi], input [F, omega] */
  /* CasadiKinematicUnicycleCombined :491 : a point mass in the track's Frenet frame, state [x, y, v, e_psi, s, x_tran], input
     [Fx, wz].  Reads mass and c_da only (:536-541).  Arc tracks only.  Six states in the kinematic bicycle's order. */
  DGSQP_MODEL_UNICYCLE_COMBINED = 3,
};
#define DGSQP_MAX_LANES 2 /* lane half-plane rows per agent and stage */
/* discretisation (dynamics_models.py:88-125, :188-219) */
enum { DGSQP_INT_EULER = 0, DGSQP_INT_RK4 = 1, DGSQP_INT_RK3 = 2, DGSQP_INT_RK2 = 3 };
/* terminal competition cost shape */
enum { DGSQP_COMP_ATAN = 0, DGSQP_COMP_LINEAR = 1 };
/* merit function (DGSQP.py:971-978) */
enum { DGSQP_MERIT_STAT_L1 = 0, DGSQP_MERIT_STAT = 1, DGSQP_MERIT_SUM_OBJ_L1 = 2 /* DG-SQP v2 only (DGSQP_v2.py:1161-1164) */ };

/* per-scenario exit codes == reference `msg` strings (DGSQP.py:388,396,408,458,466,471) */
enum {
  DGSQP_CONV_ABS_TOL = 0,
  DGSQP_CONV_REL_TOL = 1,
  DGSQP_MAX_IT = 2,
  DGSQP_DIVERGED = 3,
  DGSQP_QP_FAIL = 4,
  DGSQP_TIME_LIMIT = 5
};

/* library error codes */
enum {
  DGSQP_OK = 0,
  DGSQP_E_ARG = -1,      /* bad argument / unsupported problem */
  DGSQP_E_DEVICE = -2,   /* HIP error, no GPU, or kernel image missing */
  DGSQP_E_NOMEM = -3,
  DGSQP_E_TOO_LARGE = -4 /* problem exceeds the compiled LDS/workspace limits */
};

/*
 * One agent: vehicle model (model_types.py:34-105), cost weights
 * (scripts/DGSQP_ALGAMES_monte_carlo_chicane.py:111-122,223-277) and
 * constraint data (:80-109,282-293).
 */
typedef struct {
  int32_t model;        /* DGSQP_MODEL_* */
  int32_t tire_model;   /* 0 pacejka, 1 linear   (dynamics_models.py:2022-2029) */
  int32_t drive_wheels; /* 0 all, 1 rear         (dynamics_models.py:2036-2041) */
  int32_t simple_slip;  /* dynamics_models.py:2015-2020 */
  double L_f, L_r, mass, I_z, gravity;
  double c_dr, c_da, c_s, c_r, p_r; /* drag, damping, slip, rolling resistance (+exponent) */
  double pac_Bf, pac_Br, pac_Cf, pac_Cr, pac_Df, pac_Dr;
  double lin_Bf, lin_Br;

  /* stage cost 1/2 sum w_in u^2 + 1/2 sum w_rate (u-u_prev)^2 */
  double w_in[DGSQP_NUA];
  double w_rate[DGSQP_NUA];
  /* terminal cost  -w_prog*s_a + w_comp * sum_{b!=a} comp(s_b - s_a) */
  double w_prog, w_comp;
  int32_t comp_type; /* DGSQP_COMP_* */
  int32_t _pad0;
  /* stage+terminal state costs (ablation script :229-230):
     1/2 w_block sum_b (ey_a-ey_b)^2 + 1/2 w_obs sum_b max(0, d_ab-|p_a-p_b|)^2 */
  double w_block, w_obs, obs_cost_r;

  /* constraints */
  int32_t has_rate; /* 4 rate rows per stage, order [u0 ub, u0 lb, u1 ub, u1 lb] */
  int32_t _pad1;
  double rate_ub[DGSQP_NUA], rate_lb[DGSQP_NUA]; /* per second; multiplied by dt inside */
  double in_ub[DGSQP_NUA], in_lb[DGSQP_NUA];     /* +-inf = absent (DGSQP.py:145-148) */
  double st_ub[DGSQP_MAX_NQA], st_lb[DGSQP_MAX_NQA];
  double radius; /* obstacle row for pair (i,j): (r_i+r_j)^2 - |p_i-p_j|^2 <= 0 */

  /* goal-tracking state cost (scripts/DGSQP_merge_monte_carlo.py:253-261): stage 1/2 sum_i w_goal[i] (q_i - goal[i])^2 at
     k = 0..N-1, goal_term_mult times that at k = N.  Weights may sit on the positions and the last two states. */
  double w_goal[DGSQP_MAX_NQA], goal[DGSQP_MAX_NQA];
  double goal_term_mult;
  /* lane half-planes (merge.py:66-74, :316-318), rows at every stage k = 0..N placed where the rate rows would be:
       n(p_x)^T (p - anchor) + r n^T n <= 0,   n(p_x) = n_lo + (n_hi - n_lo) [p_x >= brk]   (CasADi pw_const)        */
  int32_t n_lane;
  int32_t _pad2;
  struct {
    double brk;          /* +inf: constant normal n_lo */
    double n_lo[2], n_hi[2];
    double anchor[2];
    double r;
  } lane[DGSQP_MAX_LANES];
  /* track-edge rows (edge_rows = 1; needs a game with a width table, dgsqp_problem_t.widths, and a model with (s, e_y): both
     bicycles and the Frenet point mass): two rows at every stage k = 1..N (x_0 is fixed), in the reference's order vertcat(right, left),
       right  -(right_width(s_k) - edge_margin) - e_y,k <= 0        left  e_y,k - (left_width(s_k) - edge_margin) <= 0
     placed among the agent's rows of stage k after its rate rows (and lane rows) and before its input and state boxes.  Gradient over
     (s, e_y): (-+w'(sbar), -+1), w' the slope of the table's piece; no second derivative of their own (the multiplier reaches Q through
     the costate).  Each row has a dense gradient of its own: two per (agent, stage) where an e_y box costs one. */
  int32_t edge_rows;
  int32_t _pad3;
  double edge_margin;
} dgsqp_agent_t;

/*
 * The game.  Track tables follow
 * DGSQP/tracks/radius_arclength_track.py:199-225 exactly:
 *   curvature(s) = pw_const(sbar, seg_s[1..n_segs-1], seg_curv[0..n_segs-1])
 *   tangent(s)   = pw_lin  (sbar, seg_s[0..n_segs],   seg_ang[0..n_segs])
 *   sbar = fmod(fmod(s, L) + L, L)
 */
typedef struct {
  int32_t M;          /* agents */
  int32_t N;          /* horizon */
  int32_t integrator; /* DGSQP_INT_* of the JOINT model (dynamics_models.py:2482-2530) */
  int32_t substeps;   /* RK sub-steps per dt ("M" in DynamicsConfig) */
  double dt;
  int32_t n_segs;
  int32_t obstacle_rows; /* 1: shared obstacle rows for every pair at k=1..N */
  double track_L;
  double seg_s[DGSQP_MAX_SEGS + 1];
  double seg_curv[DGSQP_MAX_SEGS];
  double seg_ang[DGSQP_MAX_SEGS + 1];
  dgsqp_agent_t agents[DGSQP_MAX_AGENTS];
  /* centre line of the Frenet-frame models.  DGSQP_TRACK_ARCS: the segment tables above (RadiusArclengthTrack: curvature
     piecewise constant, tangent piecewise linear, radius_arclength_track.py:199-225).  DGSQP_TRACK_SPLINE: cubic-spline
     interpolants x(s), y(s) (CasadiBSplineTrack, casadi_bspline_track.py:56-71): curvature (x'y'' - y'x'')/(x'^2 + y'^2)^1.5
     (:122-135), tangent atan2(y', x') (:137-149), s wrapped into [0, track_L).  spline = [n_knots] knots (first one 0), then
     [n_knots-1][4] coefficients of x and [n_knots-1][4] of y in ascending powers of (s - knot_i); caller-owned, copied by
     dgsqp_create (n_knots <= DGSQP_MAX_KNOTS). */
  int32_t track_kind;
  int32_t n_knots;
  const double* spline;
  /* Track width functions (CasadiBSplineTrack.left_width / right_width, casadi_bspline_track.py:61-64):
       left_width(s) = pw_lin(sbar, knot, left), right_width(s) = pw_lin(sbar, knot, right), sbar as above,
     the half widths to the left (e_y > 0) and to the right of the centre line.  widths = [n_width][3] rows (knot, left, right);
     caller-owned, copied by dgsqp_create like spline.  n_width = 0: no table (nothing reads the pointer).  Otherwise dgsqp_create /
     dgsqp_plan refuse (DGSQP_E_ARG, message starting "widths: "): n_width outside 2 .. DGSQP_MAX_KNOTS, a NULL pointer, a non-finite
     entry, knot[0] != 0, knot[n_width-1] != track_L, knots that do not increase strictly, a width that is not positive.  Either track
     kind may carry one.  Read by the spline-track raceline sampler (dgsqp_set_raceline_clip) and by the tracker's edge rows
     (dgsqp_mpc_t.edge_rows) and by the game's track-edge rows (dgsqp_agent_t.edge_rows). */
  int32_t n_width;
  int32_t _pad_w;
  const double* widths;
} dgsqp_problem_t;

#define DGSQP_TRACK_ARCS 0
#define DGSQP_TRACK_SPLINE 1
#define DGSQP_MAX_KNOTS 1152
#define DGSQP_VARIANT_V1 0
#define DGSQP_VARIANT_V2 1
#define DGSQP_QP_ACTIVE_SET 0
#define DGSQP_QP_OSQP 1
#define DGSQP_DECREASE_ARMIJO 0
#define DGSQP_DECREASE_MAX 1
/* DGSQPParams (solver_types.py:91-127), numeric subset used by solve() */
typedef struct {
  double beta, tau, p_tol, d_tol, reg;
  int32_t line_search_iters;
  int32_t nonmono_ls;
  int32_t sqp_iters;
  int32_t merit_function; /* DGSQP_MERIT_* */
  int32_t rel_tol_req;    /* 3 (DGSQP.py:56) */
  int32_t lsqr_iter_lim;  /* 0 => 2*n_c (scipy default, DGSQP.py:324) */
  double lsqr_atol, lsqr_btol; /* scipy 1.15 defaults 1e-6 */
  int32_t qp_warm_start;  /* implementation knob (not in DGSQPParams): 1 = start each QP's active-set search from the
                             previous QP's final active set (same minimiser, shorter path); 0 = cold start */
  int32_t hessian_bfgs;   /* DGSQPParams.hessian_approximation: 0 'none' (exact game Hessian every iteration), 1 'bfgs' (damped BFGS
                             update of the projected Hessian after the first iteration, DGSQP.py:353-364, :535-557) */
  double eig_floor;       /* value _nearestPD gives to the negative eigenvalues; the reference uses 1e-10 (DGSQP.py:1293).
                             <= 0 selects 1e-10, which is also what the host mirror passes by default.  With reg = 0 that
                             leaves a Hessian with condition 1e12 (solved by the classical J = L^-T active-set kernels);
                             a larger floor (e.g. 1e-6) is an explicit opt-in that keeps such games on the faster
                             explicit-inverse kernels. */
  double time_limit;      /* DGSQPParams.time_limit: wall-clock seconds per solve() after which the scenario ends with DGSQP_TIME_LIMIT
                             (checked at the end of every SQP iteration, DGSQP.py:470, and inside the watchdog's relaxed steps,
                             :1243-1247); < 0: none (the reference's None -> inf, DGSQP.py:64-67); 0 ends the solve after its
                             first iteration, as in the reference.  Counted from the moment a workgroup starts the scenario
                             (before the dual start, DGSQP.py:304), not from the launch of the batch. */
  int32_t snap_active_bounds; /* implementation knob, default 0 = literal.  1: after each QP put du exactly on the input bounds
                             whose multiplier is positive.  An exact QP solver leaves them at +-1 ulp, OSQP's polish at ~1e-12
                             (sign random); the rows are linear, the next iterate inherits that residual and _get_mu switches
                             on the sign of sum(g - s) with threshold 0 (DGSQP.py:559-585) -- a coin flip in the reference
                             itself; 1 makes it deterministic (mu = 0 when nothing else is violated). */
  int32_t variant;        /* DGSQP_VARIANT_V1: DGSQP/solvers/DGSQP.py (the fields above).  DGSQP_VARIANT_V2: DGSQP/solvers/DGSQP_v2.py
                             :322-720 -- d-step / m-step non-monotone strategy with checkpoints, decaying regularisation, merit
                             memory; p_tol/d_tol, reg (= reg_init), tau, line_search_iters, sqp_iters (counts m-steps), rel_tol_req
                             (10), time_limit and the LSQR / QP knobs above keep their meaning; beta and nonmono_ls are unused */
  /* DGSQPV2Params (solver_types.py:130-175) */
  int32_t nms;                       /* non-monotone strategy on (d-steps / m-steps) */
  int32_t nms_frequency;             /* m-step at the latest after this many d-steps (nms_mstep_frequency) */
  int32_t nms_memory_size;           /* length of the merit memory (<= 16) */
  int32_t merit_decrease_condition;  /* DGSQP_DECREASE_ARMIJO / DGSQP_DECREASE_MAX (DGSQP_v2.py:731-737) */
  int32_t qp_method;                 /* how _solve_qp (DGSQP.py:232-266) is computed.  DGSQP_QP_ACTIVE_SET (0, default): the exact KKT point of
                                        the strictly convex QP -- dual active-set method + polish -- i.e. what OSQP(polish=True) returns when its
                                        polish succeeds.  DGSQP_QP_OSQP (1): OSQP's own arithmetic as the reference runs it through CasADi's
                                        conic plugin (DGSQP.py:183-201, :246-249): Ruiz equilibration, ADMM to eps 1e-3, adaptive rho, polish
                                        accepted on residuals alone -- the iterate the reference's loop actually continues from (1e-3 .. 1e-6
                                        off the exact KKT point, occasionally negative multipliers); every size up to 320 unknowns.  A primal /
                                        dual infeasible QP ends the solve with DGSQP_QP_FAIL wherever it occurs (the reference's NaN step raises
                                        in _get_mu one iteration later, DGSQP.py:566-585) */
  int32_t osqp_rho_carry;            /* qp_method = DGSQP_QP_OSQP only.  0 (default): every OSQP call starts at rho = 0.1, as the CPU restatements
                                        the parity tests compare with do.  1: a call starts from the rho the previous call of the same solve()
                                        ended with -- inside CasADi's conic plugin the OSQP workspace persists and keeps its adapted rho
                                        (SURVEY.md parity hazard 7); the first call of a solve starts at 0.1 */
  int32_t mixed_precision;           /* 0 (default): fp64 storage and arithmetic throughout.  1: qp_method = DGSQP_QP_OSQP on the XL layout
                                        (n > 128: BASELINE configs[2], [3], [4], which name fp32) keeps the explicit K^-1 of the ADMM iteration in
                                        fp32 -- fp64 accumulation; the iteration is memory-bound and K^-1 is 60 % of the bytes it streams --;
                                        factorisations, residual checks, the polish and every other kernel stay fp64 -- and so does K^-1 when
                                        reg < 1e-4 (measured: at reg = 0 the flat directions of the projected Hessian drown in the rounding and
                                        the six-car merge of configs[4] loses half its converged solves, so the switch leaves that game in fp64).
                                        At reg = 1e-3 a QP whose polish succeeds in both returns the fp64 kernel's point to 1e-6 (the polish is
                                        fp64); ADMM iteration counts are no longer bit-comparable with the fp64 restatements, and along a whole
                                        solve only the solvable three-car game keeps its converged set (20 vs 21 of 24) -- on the chaotic F1 game
                                        single paths differ and only the statistics agree (256 scenarios: 44.9 % vs 47.3 % converged) */
  int32_t reserved_;
  double reg_decay;                  /* reg <- reg * reg_decay after every m-step / line-search step */
  double delta_decay;                /* gamma: d-step radius decay */
  double merit_decrease;             /* sigma */
  double merit_parameter;            /* mu; < 0: adaptive (DGSQPV2Params.merit_parameter = None, _get_mu DGSQP_v2.py:665-690) */
} dgsqp_params_t;

/* PID lane follower used for the Monte-Carlo warm start (DGSQP/solvers/PID.py through
   scripts/DGSQP_ALGAMES_monte_carlo_chicane.py:411-447) */
typedef struct {
  double kp_v;        /* speed P gain (1) */
  double kp_s, ki_s;  /* steering PI gains (1, 0.005) on  ey_gain (e_y - e_y0) + e_psi */
  double ey_gain;     /* 5 */
  double ei_max;      /* integrator clamp (100) */
  double u_max[2];    /* |u_a|, |u_steer| saturation */
  double du_max[2];   /* per-step change saturation, applied before the magnitude saturation */
  int32_t substeps;   /* rk4 sub-steps of the plant per dt (10) */
  int32_t reserved_;
} dgsqp_pid_t;

typedef struct {
  int32_t M, N, n_q, n_u, n, n_c; /* n = N*n_u decision vars, n_c inequality rows */
  int32_t n_dense;                /* distinct dense constraint gradients */
  int32_t lds_bytes;              /* dynamic LDS per scenario workgroup */
  int64_t workspace_bytes;        /* HBM scratch per resident workgroup */
  int32_t layout;                 /* 0 LDS-resident, 1 big (P and reflectors in the L2 scratch), 2 XL (n > 128, generic kernels) */
  int32_t reserved_;
} dgsqp_dims_t;

typedef struct {
  double h2d_ms, kernel_ms, d2h_ms, total_ms; /* HIP-event times of the last call */
  int32_t grid, block;
} dgsqp_timing_t;

/* Fixed 88-byte per-scenario record of the ONE collective of a sharded Monte-Carlo batch: what the
   convergence statistics need (process_data_curve.py:44-53).  cost holds every agent's cost (DGSQP_MAX_AGENTS slots). */
typedef struct {
  int32_t status, iters, qp_solves, rank;
  double p_feas, comp, stat;
  double cost[DGSQP_MAX_AGENTS];   /* f_J of every agent (DGSQP.py:492); zeros beyond M */
} dgsqp_stat_record_t;

typedef struct dgsqp_solver* dgsqp_handle_t;

/* Build a solver for one game on one HIP device (one process per GPU).
   Replaces DGSQP.__init__/_build_solver (DGSQP.py:26-230, :587-1030). */
int dgsqp_create(const dgsqp_problem_t* prob, const dgsqp_params_t* par, int device,
                 dgsqp_handle_t* out);
void dgsqp_destroy(dgsqp_handle_t h);
int dgsqp_dims(dgsqp_handle_t h, dgsqp_dims_t* out);
/* What dgsqp_create would build for this game -- dimensions, LDS / scratch need and the layout chosen -- without touching a
   device (host only).  Returns DGSQP_E_TOO_LARGE / DGSQP_E_ARG with the reason in msg when the game is not supported. */
int dgsqp_plan(const dgsqp_problem_t* prob, const dgsqp_params_t* par, dgsqp_dims_t* out, char* msg, int msglen);
const char* dgsqp_last_error(dgsqp_handle_t h); /* h may be NULL: last create() error */
int dgsqp_backend_info(char* buf, int buflen);  /* device name / arch / CU count */

/*
 * Solve B independent scenarios == B calls of DGSQP.solve() (DGSQP.py:302-507).
 * All arrays are caller-owned, C-contiguous host memory.
 *   x0     [B][n_q]          joint initial state (state2q, dynamics_models.py:2554-2561)
 *   u_ws   [B][n]            agent-major warm start (set_warm_start, DGSQP.py:271-281)
 *   u_out  [B][n]            agent-major solution
 *   l_out  [B][n_c]          multipliers (l_pred)
 *   x_out  [B][(N+1)*n_q]    q_pred
 *   status [B] DGSQP_* code, iters [B] num_iters, qp_solves [B]
 *   cond   [B][3]            p_feas, comp, stat of the last iteration (DGSQP.py:376-379)
 *   cost   [B][M]            f_J at the solution (DGSQP.py:492)
 * Any output pointer may be NULL.
 */
int dgsqp_solve_batch(dgsqp_handle_t h, int64_t B, const double* x0, const double* u_ws,
                      double* u_out, double* l_out, double* x_out, int32_t* status,
                      int32_t* iters, int32_t* qp_solves, double* cond, double* cost,
                      dgsqp_timing_t* timing);

/* The same call with single-precision arrays at the boundary ("double / float selected by dtype"): x0, u_ws
   are widened to fp64 on the device, the solve runs in fp64 -- there are no fp32 arithmetic kernels -- and u, l, x, cond,
   cost are rounded to fp32 on the way out.  Halves the HBM / PCIe bytes of the batch, changes nothing else: on inputs that are
   exactly representable in fp32 the integer outputs equal those of dgsqp_solve_batch. */
int dgsqp_solve_batch_f32(dgsqp_handle_t h, int64_t B, const float* x0, const float* u_ws,
                          float* u_out, float* l_out, float* x_out, int32_t* status,
                          int32_t* iters, int32_t* qp_solves, float* cond, float* cost,
                          dgsqp_timing_t* timing);

/*
 * Closed-loop (receding-horizon) batch: B independent chains of T calls of DGSQP.step() (DGSQP.py:283-297) in ONE launch.  One
 * workgroup carries one scenario through all T steps, so the launch ends with its longest chain, not T times with its slowest
 * scenario, and no intermediate state crosses the host.  Step t of scenario b is the very solve dgsqp_solve_batch performs from
 * (q[t][b], u_ws[t][b]) -- bit for bit --; between steps
 *   q[t+1][b]    = x_t[b][1] (+ w[t][b])          the plant is the game's own discrete model plus the optional disturbance w
 *                                                 (or the plant of dgsqp_set_plant, below)
 *   u_ws[t+1][b] = u_t[b] shifted by one stage per agent, last row repeated; after DGSQP_DIVERGED / DGSQP_QP_FAIL: u_ws[t][b] again
 * A non-finite q[t+1][b] ends chain b: steps_done[b] = t + 1 (otherwise T) and no solve starts from such a state.  Records of steps
 * that never ran hold status DGSQP_NOT_RUN, iters = qp_solves = 0 and NaN in every double, their q / u_ws slices included
 * (q[steps_done[b]][b] keeps the non-finite state that ended the chain; no warm start is written for it).
 * Arrays are step-major, caller-owned host memory; w, l_out, x_out and timing may be NULL.  The call is synchronous.  Event log,
 * iterate log, cooperative line search and deferral do not apply to closed-loop launches (a chain's next solve depends on its last
 * one); their settings are left as they are for the next dgsqp_solve_batch.  T < 1, B < 0 or a NULL required pointer: DGSQP_E_ARG.
 */
#define DGSQP_NOT_RUN (-1)
int dgsqp_closed_loop_batch(dgsqp_handle_t h, int64_t B, int32_t T,
    const double* x0,      /* [B][n_q] */
    const double* u_ws,    /* [B][n], agent-major */
    const double* w,       /* [T][B][n_q] or NULL */
    double* q_out,         /* [T+1][B][n_q]; slice 0 = x0 */
    double* u_ws_out,      /* [T+1][B][n]; slice t = the warm start step t started from */
    double* u_out,         /* [T][B][n] */
    double* l_out,         /* [T][B][n_c] or NULL */
    double* x_out,         /* [T][B][N+1][n_q] or NULL */
    int32_t* status, int32_t* iters, int32_t* qp_solves,   /* [T][B] */
    double* cond,          /* [T][B][3] */
    double* cost,          /* [T][B][M] */
    int32_t* steps_done,   /* [B] */
    dgsqp_timing_t* timing);

/*
 * A plant of its own for closed-loop launches (reference DGSQP/dynamics/dynamics_simulator.py:11-40: the simulator steps a model
 * built from its own dynamics_config, several simulation steps per control step, every input channel behind a delay line).  With a
 * plant set, q[t+1][b] is no longer stage 1 of the prediction: the state q[t][b] is advanced by sim_steps simulation steps of
 * length dt / sim_steps of the plant's model -- the game's model class, state layout and track; vehicle parameters, tyre model,
 * driven wheels and slip formula of its own -- under u_new = stage 0 of u_t[b].  Simulation step j of a channel with delay d > 0
 * integrates under the oldest entry of that channel's line (d entries, zeros when the chain starts, kept from control step to control
 * step) and then appends u_new; d = 0 integrates under u_new.  One simulation step is `substeps` steps of `integrator` on the
 * continuous model (DGSQP_INT_EULER takes one step, as the game's model does).  After the sim_steps steps w[t][b] is added as
 * before; the end-of-chain rule, steps_done, the warm-start shift and every solve are unchanged (step t still is, bit for bit, the
 * solve dgsqp_solve_batch performs from (q[t][b], u_ws[t][b])).
 */
#define DGSQP_MAX_DELAY 16
typedef struct {
  int32_t integrator;      /* DGSQP_INT_* */
  int32_t substeps;        /* >= 1 */
  int32_t sim_steps;       /* >= 1 */
  int32_t use_game_agents; /* 1: the game's vehicle parameters (agents[] is not read) */
  int32_t delay[DGSQP_MAX_AGENTS][DGSQP_NUA]; /* simulation steps, 0 .. DGSQP_MAX_DELAY; entries beyond M are not read */
  dgsqp_agent_t agents[DGSQP_MAX_AGENTS];     /* only the vehicle fields (model .. lin_Br) are read; model must equal the game's */
} dgsqp_plant_t;
/* The plant of the handle's SUBSEQUENT closed-loop launches (copied); NULL: the game's own discrete model again.  Nothing else is
   affected.  DGSQP_E_ARG with the reason in dgsqp_last_error: unknown integrator, substeps < 1, sim_steps < 1, a delay outside
   0 .. DGSQP_MAX_DELAY, an agent of another model class than the game's. */
int dgsqp_set_plant(dgsqp_handle_t h, const dgsqp_plant_t* plant);
/* The inputs the plant integrated under in the handle's last closed-loop launch with a plant: out [T][B][sim_steps][n_u] (n_u joint
   inputs, agent after agent); NaN where a step never ran.  capacity_doubles = what out can hold (DGSQP_E_ARG when it is too small or
   when no such launch has run). */
int dgsqp_fetch_u_plant(dgsqp_handle_t h, double* out, int64_t capacity_doubles);

/*
 * Three more settings of closed-loop launches WITH A PLANT SET (robustness studies over a distribution of vehicles).  Each has a setter
 * for the handle's SUBSEQUENT closed-loop launches (NULL / 0 switches it off again) and, where it records something, a fetcher for what
 * the last such launch left behind.  dgsqp_set_plant(h, plant) of the identity plant (use_game_agents = 1, sim_steps = 1, the game's
 * integrator, no delay) is enough; switching any of them on, or launching with one of them on, while no plant is set is DGSQP_E_ARG.
 * A launch that uses none of them runs the kernels it always ran; dgsqp_solve_batch is never affected.
 */
/* The vehicle fields model .. lin_Br of dgsqp_agent_t: its first 160 bytes, field for field. */
typedef struct {
  int32_t model, tire_model, drive_wheels, simple_slip;
  double L_f, L_r, mass, I_z, gravity;
  double c_dr, c_da, c_s, c_r, p_r;
  double pac_Bf, pac_Br, pac_Cf, pac_Cr, pac_Df, pac_Dr;
  double lin_Bf, lin_Br;
} dgsqp_vehicle_t;
#ifdef __cplusplus
static_assert(sizeof(dgsqp_vehicle_t) == 160 && offsetof(dgsqp_agent_t, w_in) == sizeof(dgsqp_vehicle_t) &&
              offsetof(dgsqp_vehicle_t, model) == offsetof(dgsqp_agent_t, model) && offsetof(dgsqp_vehicle_t, simple_slip) == offsetof(dgsqp_agent_t, simple_slip) &&
              offsetof(dgsqp_vehicle_t, L_f) == offsetof(dgsqp_agent_t, L_f) && offsetof(dgsqp_vehicle_t, gravity) == offsetof(dgsqp_agent_t, gravity) &&
              offsetof(dgsqp_vehicle_t, c_dr) == offsetof(dgsqp_agent_t, c_dr) && offsetof(dgsqp_vehicle_t, p_r) == offsetof(dgsqp_agent_t, p_r) &&
              offsetof(dgsqp_vehicle_t, pac_Bf) == offsetof(dgsqp_agent_t, pac_Bf) && offsetof(dgsqp_vehicle_t, pac_Dr) == offsetof(dgsqp_agent_t, pac_Dr) &&
              offsetof(dgsqp_vehicle_t, lin_Bf) == offsetof(dgsqp_agent_t, lin_Bf) && offsetof(dgsqp_vehicle_t, lin_Br) == offsetof(dgsqp_agent_t, lin_Br),
              "dgsqp_vehicle_t is the vehicle prefix of dgsqp_agent_t");
#else
_Static_assert(sizeof(dgsqp_vehicle_t) == 160 && offsetof(dgsqp_agent_t, w_in) == sizeof(dgsqp_vehicle_t) &&
               offsetof(dgsqp_vehicle_t, L_f) == offsetof(dgsqp_agent_t, L_f) && offsetof(dgsqp_vehicle_t, lin_Br) == offsetof(dgsqp_agent_t, lin_Br),
               "dgsqp_vehicle_t is the vehicle prefix of dgsqp_agent_t");
#endif
/* A plant PER CHAIN: chain b of a launch of exactly B chains integrates with vehicles[b][a] in place of the plant's agents[a] and, when
   delay is given, with delay[b][a][channel] in place of the plant's delay.  Integrator, substeps and sim_steps stay those of
   dgsqp_set_plant, so u_plant keeps its shape; delay lines start empty for every chain as before.  Both arrays are copied.
   vehicles = NULL or B = 0: off.  DGSQP_E_ARG, message starting "plant ensemble: ": no plant set, B < 0, a vehicle of another model
   class than the game's agent, a delay outside 0 .. DGSQP_MAX_DELAY; and, from dgsqp_closed_loop_batch, a launch whose B differs. */
int dgsqp_set_plant_ensemble(dgsqp_handle_t h, int64_t B, const dgsqp_vehicle_t* vehicles /* [B][M] */, const int32_t* delay /* [B][M][DGSQP_NUA] or NULL */);
/* State estimates: solve t of chain b starts from q_est[t][b] = q[t][b] + v[t][b] (one fp64 add per entry) and not from q[t][b]; the plant
   goes on advancing the TRUE q[t][b], and every solve still is, bit for bit, the one dgsqp_solve_batch performs from (q_est[t][b],
   u_ws[t][b]).  A non-finite q_est[t][b] ends chain b BEFORE that solve: steps_done[b] = t (0 is possible) and the slice keeps the value.
   v is copied; v = NULL or T = 0 or B = 0: off.  DGSQP_E_ARG: no plant set; from dgsqp_closed_loop_batch, a launch whose T or B differs.
   dgsqp_fetch_q_est: q_est [T][B][n_q] of the last launch with estimates, NaN where a step never started. */
int dgsqp_set_estimate_noise(dgsqp_handle_t h, int32_t T, int64_t B, const double* v /* [T][B][n_q] */);
int dgsqp_fetch_q_est(dgsqp_handle_t h, double* out /* [T][B][n_q] */, int64_t capacity_doubles);
/* Safety monitor of what happens BETWEEN control steps.  mode 0 off, 1 record, 2 record and stop.  For a control step t of chain b that
   ran, let z_0 .. z_{S-1} be the joint states after each of the S = sim_steps simulation steps, z_{S-1} with w[t][b] added (it is
   q[t+1][b]).  Then
     clearance[t][b]  = min over j and pairs i < k of sqrt(dx^2 + dy^2) - (radius_i + radius_k), (dx, dy) the difference of the first two
                        entries of the two agents' state blocks (the positions the obstacle rows read); +inf for M = 1;
     box_excess[t][b] = max over j, agents and state entries with a finite bound of max(z - st_ub, st_lb - z), with the GAME's bounds;
                        -inf when no entry has one (track-edge rows are not read: a game that bounds e_y by dgsqp_agent_t.edge_rows has no
                        e_y entry here);
   both NaN for a step that never ran and for a step with a non-finite entry in one of its z_j;
     hit_step[b]      = the smallest t * S + j whose pairwise clearance is < 0, or -1.
   In mode 2 chain b ends after the control step of its first hit: steps_done[b] = t + 1, q[t+1][b] is kept, u_ws[t+1][b] is not written
   (as after a non-finite state).  DGSQP_E_ARG: a mode other than 0, 1, 2; no plant set.
   dgsqp_fetch_monitor: the records of the last launch with the monitor on; clearance, box_excess [T][B], hit_step [B], none may be NULL. */
int dgsqp_set_monitor(dgsqp_handle_t h, int mode);
int dgsqp_fetch_monitor(dgsqp_handle_t h, double* clearance, double* box_excess, int32_t* hit_step);

/*
 * Drivers: who produces the command that enters agent a's plant at control step t of chain b (closed-loop launches WITH A PLANT SET).
 * Without drivers every agent applies stage 0 of the joint game solution: self-play.  With them the ego car can apply its part of the
 * solution while the others are driven by a lane follower or by a recorded drive (the reference's closed-loop script drives its cars by
 * their own controllers: scripts/race/race_main.py).  Everything downstream of the command is unchanged: it passes through the agent's
 * delay lines, is held for the sim_steps simulation steps, and u_plant records what was integrated.  The solves do not change: solve t
 * still is, bit for bit, the dgsqp_solve_batch solve from (q[t][b] or q_est[t][b], u_ws[t][b]), and the warm start still is the shifted
 * JOINT solution -- the game's belief about everybody, drivers included.
 *   DGSQP_DRIVER_GAME    stage 0 of the game's solution, as without drivers.
 *   DGSQP_DRIVER_PID     the lane follower of dgsqp_pid_t run closed-loop on the TRUE state q[t][b], also when the solves start from
 *                        estimates: speed P control on v - v_ref, steering PI control on ey_gain (e_y - lat_ref) + e_psi; rate
 *                        saturation first, against the agent's previous command, then magnitude.  The law's dt is the control step.  The
 *                        integrator and the previous command persist along the chain and start at 0 for every chain.  `substeps` is
 *                        not read.  For the 6- and 8-state models only (the unicycle has no e_y / e_psi).
 *   DGSQP_DRIVER_REPLAY  u_replay[t][b] of that agent.  A non-finite entry makes the next state non-finite and ends that chain.
 *   DGSQP_DRIVER_TRACK   with a cross plant only (dgsqp_set_cross_plant, below): the lane follower tracks the game's plan.
 */
enum { DGSQP_DRIVER_GAME = 0, DGSQP_DRIVER_PID = 1, DGSQP_DRIVER_REPLAY = 2, DGSQP_DRIVER_TRACK = 3 };
typedef struct {
  int32_t kind[DGSQP_MAX_AGENTS];     /* DGSQP_DRIVER_*; entries beyond M are not read */
  dgsqp_pid_t pid[DGSQP_MAX_AGENTS];  /* read for PID agents */
} dgsqp_drivers_t;
/* The drivers of the handle's SUBSEQUENT closed-loop launches of exactly T steps and B chains; every array is copied.  d = NULL: off.
   kind: the kinds per chain, or NULL for d->kind in every chain.  ref: (v_ref, lat_ref) per chain and agent for the PID agents, or NULL
   for (v, e_y) of the chain's x0, as the warm-start PID takes them.  u_replay: joint inputs, agent after agent; only the entries of
   REPLAY agents are read.  DGSQP_E_ARG, message starting "drivers: ": no plant set, a kind outside 0 .. 2 (in d or in kind), PID for a
   unicycle agent, a REPLAY kind anywhere without u_replay, T < 1 or B < 0; and, from dgsqp_closed_loop_batch, a launch whose T or B
   differs.  dgsqp_solve_batch and launches without drivers are not affected.
   dgsqp_fetch_u_cmd: the commands of the last launch with drivers, [T][B][n_u]; NaN where a step never ran; for a GAME agent stage 0 of
   u.  capacity_doubles = what out can hold (DGSQP_E_ARG when it is too small or when no such launch has run). */
int dgsqp_set_drivers(dgsqp_handle_t h, const dgsqp_drivers_t* d, int32_t T, int64_t B,
                      const int32_t* kind     /* [B][M] or NULL: d->kind for every chain */,
                      const double*  ref      /* [B][M][2] or NULL: from x0 */,
                      const double*  u_replay /* [T][B][n_u] or NULL; only REPLAY agents' entries are read */);
int dgsqp_fetch_u_cmd(dgsqp_handle_t h, double* out /* [T][B][n_u] */, int64_t capacity_doubles);

/*
 * The input before stage 0.  The stage-0 rate rows  -/+ (u_0 - u_prev) <= dt rate  and the stage-0 rate cost  1/2 w_rate (u_0 - u_prev)^2
 * of a solve are measured against u_prev, the joint input applied before the scenario's first stage: n_u doubles in the order of
 * u_pred[0] (agent a's two inputs at 2 a).  Without a setting u_prev = 0, the reference's solve() (DGSQP.py:305-308).
 *
 * dgsqp_set_u_prev: sticky, like dgsqp_set_plant; the array is copied.  It applies to the handle's SUBSEQUENT dgsqp_solve_batch,
 * dgsqp_solve_batch_f32, dgsqp_stage_inputs (captured when staging: a later set does not reach a batch that is already staged, and every
 * handle of a pipeline or a grouped launch keeps its own), dgsqp_evaluate_batch and dgsqp_qp_batch(_info) of exactly B scenarios; such a
 * call with another B returns DGSQP_E_ARG (message starting "u_prev: ").  A batch staged by dgsqp_sample_batch runs from zeros.
 * u_prev = NULL with B = 0: off.  An entry that is not finite is refused (DGSQP_E_ARG).  Closed-loop launches ignore it.
 *
 * dgsqp_set_closed_loop_u_prev, mode 1 (carry): solve t of chain b of the handle's SUBSEQUENT closed-loop launches runs with
 * u_prev[t][b], where u_prev[0][b] = u_prev0[b] (NULL: zeros; otherwise the launch must have exactly B chains) and u_prev[t+1][b] is,
 * per agent, the command that entered that agent's plant at step t: stage 0 of u[t][b] as returned -- also after 'diverged' and
 * 'qp_fail', the feedback applies it then as well --, or with drivers u_cmd[t][b]; with delay lines the value appended to the line, not
 * the delayed one the plant integrated under.  Mode 0: off.  It needs no plant.  dgsqp_solve_batch ignores it.  DGSQP_E_ARG, message
 * starting "closed-loop u_prev: ": another mode, B < 0, an entry of u_prev0 that is not finite; and, from dgsqp_closed_loop_batch, a
 * launch whose B differs from a u_prev0's.
 * dgsqp_fetch_u_prev: u_prev of the last launch that carried, [T][B][n_u]; NaN where it was never written (the steps after a chain's
 * end).  capacity_doubles = what out can hold (DGSQP_E_ARG when it is too small or when no such launch has run).
 */
int dgsqp_set_u_prev(dgsqp_handle_t h, int64_t B, const double* u_prev /* [B][n_u], or NULL with B = 0: off */);
int dgsqp_set_closed_loop_u_prev(dgsqp_handle_t h, int mode /* 0 off, 1 carry */, int64_t B, const double* u_prev0 /* [B][n_u] or NULL = zeros */);
int dgsqp_fetch_u_prev(dgsqp_handle_t h, double* out /* [T][B][n_u] */, int64_t capacity_doubles);

/*
 * Holding a plan across control steps (closed-loop launches WITH A PLANT SET): a planning rate below the control rate, and a defined
 * command when a solve fails (the reference's closed-loop script solves once and follows that solution for many control steps:
 * scripts/race/race_main.py:495-578).  A chain holds a plan and consumes it stage by stage until a newer one is accepted.  The held plan
 * is the warm-start chain itself: stage 0 of u_ws[t][b] is the next unconsumed stage of the last accepted plan, one more shift consumes it.
 *
 * replan_every = R (1 <= R <= N), on_fail (DGSQP_HOLD_REFERENCE, DGSQP_HOLD_HOLD) and fail_mask: bit s set when status s counts as a
 * failed solve (bits 0 .. 5 only; the reference's list is (1 << DGSQP_DIVERGED) | (1 << DGSQP_QP_FAIL)).  Per chain: age (int) and due
 * (bool), age = 0 and due = true at t = 0.  Step t, with ws = u_ws[t][b] and u_t the solve's iterate:
 *
 *   case                                  u_game[t][b]   u_ws[t+1][b]     age, due after                  records of step t
 *   due, status not in fail_mask          stage 0 of u_t shift(u_t)       age = 1, due = (1 >= R)         the solve's; plan_stage = 0
 *   due, failed, DGSQP_HOLD_REFERENCE     stage 0 of u_t ws (unshifted)   unchanged (due stays)           the solve's; plan_stage = 0
 *   due, failed, DGSQP_HOLD_HOLD          stage 0 of ws  shift(ws)        age += 1 (due stays)            the solve's; plan_stage = age before
 *   not due (held step, no solve)         stage 0 of ws  shift(ws)        age += 1, due = (age >= R)      status DGSQP_HELD, iters = qp_solves = 0,
 *                                                                                                         every double NaN; plan_stage = age before
 *
 * shift is the per-agent shift with the last row repeated, so a plan older than N stages repeats its last row.  u_game takes the place of
 * stage 0 of u_t in everything downstream, which is unchanged: drivers (a GAME agent receives u_game; PID and REPLAY agents are
 * untouched), delay lines, simulation steps, u_plant, monitor, disturbance, the end-of-chain rules and the u_prev carry (u_prev takes
 * the command that entered the plant).  With estimates q_est[t][b] is formed and checked only on steps that solve: on a held step the
 * noise is not read, q_est[t][b] stays NaN and a non-finite entry there does not end the chain.  Steps that never ran keep
 * DGSQP_NOT_RUN and plan_stage = -1.  R = 1 with DGSQP_HOLD_REFERENCE and the reference's mask is, record for record and bit for bit,
 * the launch without the setting.
 */
#define DGSQP_HELD (-2)
#define DGSQP_HOLD_REFERENCE 0
#define DGSQP_HOLD_HOLD 1
typedef struct {
  int32_t replan_every;   /* R: 1 .. N */
  int32_t on_fail;        /* DGSQP_HOLD_* */
  uint32_t fail_mask;     /* bit s: status s is a failed solve; bits 0 .. 5 */
  int32_t reserved;
} dgsqp_hold_t;
/* The setting of the handle's SUBSEQUENT closed-loop launches (copied); NULL: off.  DGSQP_E_ARG, message starting "plan hold: ": no
   plant set, replan_every outside 1 .. N, an unknown on_fail, a mask bit above 5; and, from dgsqp_closed_loop_batch, a launch without a
   plant.  dgsqp_solve_batch and launches without the setting are not affected.
   dgsqp_fetch_plan_hold: u_game [T][B][n_u] (NaN where a step never ran) and plan_stage [T][B] (-1 there) of the last launch with the
   setting; capacity_doubles = what u_game can hold (DGSQP_E_ARG when it is too small, when a pointer is NULL or when no such launch has
   run). */
int dgsqp_set_plan_hold(dgsqp_handle_t h, const dgsqp_hold_t* hold);
int dgsqp_fetch_plan_hold(dgsqp_handle_t h, double* u_game /* [T][B][n_u] */, int32_t* plan_stage /* [T][B] */, int64_t capacity_doubles);

/*
 * A plant of ANOTHER MODEL CLASS than the game's (the reference's race demo plans with a point-mass game and drives a dynamic bicycle with
 * Pacejka tyres: scripts/race/race_main.py:438-456, 586-597).  The plant keeps a state z of its own, [T+1][B][n_z], n_z the sum of the
 * plant agents' state counts, and the game sees the projection q = p(z), agent by agent:
 *
 *   game -> plant                                     projection
 *   same class (all four classes)                     identity
 *   kinematic bicycle (0) -> dynamic bicycle (1)      z[[0,1,2,5,6,7]]
 *   Frenet point mass (3) -> kinematic bicycle (0)    identity
 *   Frenet point mass (3) -> dynamic bicycle (1)      z[[0,1,2,5,6,7]]
 *
 * (8 states [x, y, vx, vy, w, e_psi, s, e_y]; 6 states [x, y, v, e_psi, s, e_y], the point mass [x, y, v, e_psi, s, x_tran];
 * race_main.py:533-541 maps between them in the same way.)  Every other pair is refused; agents of one game may use different pairs.
 *
 * dgsqp_set_cross_plant: sticky like dgsqp_set_plant, every array is copied.  plant->agents[a].model may be any class of the table;
 * use_game_agents = 1: every agent keeps the game's class and record.  z0 [B][n_z] is slice 0 of z.  It counts as "a plant is set" for the
 * ensemble, estimate, monitor, drivers, hold and u_prev settings; dgsqp_set_plant(h, ...) and dgsqp_set_cross_plant(h, NULL, 0, NULL)
 * clear it.  DGSQP_E_ARG, message starting "cross plant: ": what dgsqp_set_plant refuses, a pair outside the table, B < 1, z0 = NULL.
 *
 * dgsqp_closed_loop_batch with a cross plant set: x0 must equal p(z0) bit for bit and B must be z0's, w must be NULL (a disturbance in
 * the game's layout has no place in z), else DGSQP_E_ARG ("cross plant: ...").  Step t: z[t+1][b] is z[t][b] advanced by the plant as
 * under dgsqp_set_plant (u_plant, delay lines, sim_steps, integrator and sub-steps work exactly as there) and q[t+1][b] = p(z[t+1][b]).
 * Every solve still is, bit for bit, the dgsqp_solve_batch solve from (q[t][b] or q_est[t][b], u_ws[t][b]); q_est = p(z) + v, the noise
 * stays in the game's layout.  A chain ends on a non-finite entry of z[t+1][b] (the projection drops vy and w).  The monitor reads the
 * projected states after each simulation step: positions, and the game's bounds on the entries the game sees.
 * dgsqp_set_plant_ensemble compares each vehicle's class with the PLANT's agent class.
 *
 * Drivers on a cross plant.  GAME needs inputs of the same meaning: same-class pairs and 0 -> 1; a point-mass agent (Fx, wz) on a bicycle
 * plant (acceleration, steering) with a GAME driver is refused when the launch starts -- a launch without drivers included, all agents
 * are GAME then -- with a message starting "drivers: " that names the agent.  PID and REPLAY read and command the PLANT's agent (e_psi at
 * 5 and e_y at 7 of an 8-state block; with ref = NULL the references come from z0).  DGSQP_DRIVER_TRACK is accepted only while a cross
 * plant is set (the identity cross plant will do), for 6- and 8-state agents.  With g = u_game[t][b] of agent a (stage 0 of the solution,
 * or of the held plan):
 *   x_ref = one step of the GAME's discrete model for agent a from p_a(z[t][b]) -- the TRUE state -- under g (the game's integrator,
 *           sub-steps and dt);
 *   the command is the PID law with v_ref = x_ref[v], lat_ref = x_ref[last] and the heading error e_psi - x_ref[e_psi] in place of
 *   e_psi; v, e_y and e_psi are the plant agent's.  Integrator and previous command persist and are reset per chain, as for PID.
 * With the u_prev carry a TRACK agent's u_prev[t+1] takes u_game[t] (the game's rate rows are in the game's units), every other kind
 * u_cmd[t] as before.
 *
 * dgsqp_fetch_plant_state: z [T+1][B][n_z] of the last launch with a cross plant; slice 0 is z0, the state that ended a chain is kept,
 * slices of steps that never ran hold NaN.  dgsqp_fetch_track_ref: [T][B][M][3] (v_ref, lat_ref, epsi_ref) of that launch; NaN for
 * agents that are not TRACK and for steps that never ran.  capacity_doubles = what the array can hold (DGSQP_E_ARG when it is too small
 * or when no such launch has run).  Launches without a cross plant run the kernels they always ran.
 */
int dgsqp_set_cross_plant(dgsqp_handle_t h, const dgsqp_plant_t* plant, int64_t B, const double* z0 /* [B][n_z] */);
int dgsqp_fetch_plant_state(dgsqp_handle_t h, double* z /* [T+1][B][n_z] */, int64_t capacity_doubles);
int dgsqp_fetch_track_ref(dgsqp_handle_t h, double* out /* [T][B][M][3] */, int64_t capacity_doubles);

/*
 * Device-resident variant used by bench.py: inputs are staged once with
 * dgsqp_stage_inputs(); dgsqp_solve_staged() runs only the solve kernel on
 * the handle's stream; dgsqp_fetch_results() copies results back.
 */
int dgsqp_stage_inputs(dgsqp_handle_t h, int64_t B, const double* x0, const double* u_ws);
int dgsqp_solve_staged(dgsqp_handle_t h, dgsqp_timing_t* timing);
/* Asynchronous halves of dgsqp_solve_staged(): enqueue the solve on one of the device's launch streams / wait for it.  Independent
   batches held by different handles of the SAME game (same dgsqp_problem_t and dgsqp_params_t) can be in flight together:
   the workgroups of the later launch take over the compute units as the earlier launch drains its slowest scenarios.
   Handles of DIFFERENT games are safe too, but serialised: such a launch first waits for the launches in flight on the
   device (the kernels read the game from one per-device constant block). */
int dgsqp_launch_staged(dgsqp_handle_t h);
int dgsqp_wait(dgsqp_handle_t h, dgsqp_timing_t* timing);
/* ONE launch over the staged batches of `count` handles (same game, same batch size, same device; at most 64): the scenarios of all
   of them share one ticket queue, every batch keeps its own input and output buffers, results are bit-identical to separate
   launches.  A launch ends with its slowest scenario, so few long launches keep the compute units busier than many short ones.
   Launches run on K = min(GPU_MAX_HW_QUEUES, 8) launch streams per device (4 queues unless the variable is set), taken round robin
   in launch order whichever handles lead: up to K launches in flight overlap, launch j queues behind launch j - K alone.  hs[0]
   leads: its workspace and events are used; every handle of the group is in flight until ITS dgsqp_wait / dgsqp_fetch_results
   (which wait for the group's kernel).
   Event and iterate logs are not available in grouped launches. */
int dgsqp_launch_staged_group(const dgsqp_handle_t* hs, int count);
/* Cooperative line search.  A launch ends with its slowest scenario (dozens of failing 50-trial line searches) while most
   workgroups have long run out of scenarios.  In a cooperative launch those workgroups stay and evaluate line-search trial points
   for the ones still solving (the very same device code: results are bit-identical to a non-cooperative launch); they keep their
   compute units until the launch's last scenario is done.  mode 0: never; 1 (default): in the synchronous calls only
   (dgsqp_solve_batch, dgsqp_solve_staged -- nothing else is waiting for the compute units); 2: every launch of this handle, also
   the asynchronous ones -- for the LAST launch of a pipeline.  The leader's setting governs a grouped launch. */
int dgsqp_set_cooperative(dgsqp_handle_t h, int mode);
/* Diagnostic: counters of the handle's last cooperative launch -- out6 = {trials evaluated by helpers, times a workgroup entered
   the helper loop (at most coop_helpers of them evaluate trials at any moment, the others sleep), scenarios finished, helpers still registered (0 after the launch), helper values the owners consumed, helper values
   whose bits differed from the owner's own evaluation (verify mode, environment DGSQP_COOP_VERIFY=1; must be 0)}. */
int dgsqp_coop_stats(dgsqp_handle_t h, uint64_t* out6);
/* qp_method = DGSQP_QP_OSQP: {QP calls, ADMM iterations} of every solve on h's DEVICE since the last reset (waits for h's launches; callers
   that want a clean count let the device's other handles finish first).  out2 may be NULL (reset only).  Nothing in the reference: OSQP
   reports `info.iter` per call; this is the sum bench.py divides to price the ADMM work it measures (mean iterations per QP). */
int dgsqp_osqp_counters(dgsqp_handle_t h, uint64_t* out2, int reset);
/* Deferral of long scenarios (cooperative launches; scheduling only, results are bit-identical).  Nothing in a scenario's inputs
   tells how long its solve will run; its own history does.  A scenario still iterating after max(min_iters, factor x the mean
   iteration count of the launch's finished scenarios) SQP iterations is set aside while fresh scenarios remain in the queue -- its
   workgroup stores the LDS arena and its scratch in a slot and takes the next ticket -- and resumed from that image once the queue
   is empty, the scenarios that have cost the most so far first.  The long solves of a launch's last batches thereby run while the
   chip still has other work.  Defaults: min_iters 8, factor 2.0; min_iters 0 switches it off.  Never applied while logs are recorded or in
   non-cooperative launches; DG-SQP v1 solves with a wall-clock limit (dgsqp_params_t.time_limit >= 0) are never deferred either.
   DG-SQP v2 solves can be deferred too, but only after an explicit dgsqp_set_deferral (measured: it does not pay for v2's length
   distribution); its study always sets a limit (600 s): the time a scenario spends set aside does not count towards it.  The slots
   (LDS image + scratch image per scenario: 0.65 MB for the 2-agent N = 25 games, up to 4 MB for the XL layouts) are one pool per
   device: sized for what the launch may defer (a quarter of its scenarios; 257 slots = 0.17 GB for a 1,024-scenario batch, 3.4 GB for
   a group of 20), grown geometrically by later, larger launches, never beyond DGSQP_DEFER_POOL_BYTES (environment; default 16 GiB,
   0 = no deferral), kept until the process's last handle is destroyed; a cooperative launch that finds the pool in use by another
   launch in flight simply does not defer.  Nothing is
   deferred before 32 scenarios of the launch have finished nor when fewer than two rounds of fresh scenarios remain. */
int dgsqp_set_deferral(dgsqp_handle_t h, int32_t min_iters, double factor);
/* Sizes the device's deferral pool now for a cooperative launch of `scenarios` scenarios of h's game (what that launch would do itself
   on entry: a hipFree + hipMalloc of up to several GB when the pool has to grow -- 1 to 100 ms that a caller may not want inside a
   timed or latency-critical region).  Nothing in the reference. */
int dgsqp_reserve_deferral(dgsqp_handle_t h, int64_t scenarios);
/* Diagnostic: out2 = {scenarios deferred, scenarios resumed} of the handle's last cooperative launch (equal after the launch). */
int dgsqp_deferral_stats(dgsqp_handle_t h, uint64_t* out2);
/* Diagnostic: one row of 11 values per deferred scenario of the handle's last cooperative launch, at most cap_rows rows --
   {ticket, SQP iterations and QP solves when it was set aside, 100 MHz ticks it had cost by then (the resume order's key), ticks since
   the launch's start when it was set aside / resumed / finished, (QP solves << 32) | iterations at the end, and -- as the bits of three doubles -- the convergence measures (constraint violation,
   complementarity, stationarity) of its last iteration before it was set aside}.  Returns the number of
   rows written, negative on error. */
int dgsqp_deferral_log(dgsqp_handle_t h, uint64_t* out, int64_t cap_rows);
/* 1 once the handle's last launch has handed out its last scenario (it only drains from then on, compute units are
   becoming free) or when nothing is in flight; 0 while scenarios are still queued.  Polled by bench.py to start the next
   independent batch on another handle at exactly that moment. */
int dgsqp_draining(dgsqp_handle_t h);
/* 1 once the launch of dgsqp_launch_staged has completed (or nothing is in flight), 0 while it runs; never blocks.  A batch ends
   with its slowest scenario: a caller that keeps several launches in flight retires whichever has finished, not the oldest. */
int dgsqp_finished(dgsqp_handle_t h);
int dgsqp_fetch_results(dgsqp_handle_t h, double* u_out, double* l_out, double* x_out,
                        int32_t* status, int32_t* iters, int32_t* qp_solves, double* cond,
                        double* cost);

/*
 * Test hook == one DGSQP._evaluate(u, l, x0, up=0, hessian=True) per scenario
 * (DGSQP.py:509-533) plus the dual initialisation of DGSQP.py:320-327.
 *   l   [B][n_c] multipliers used for Q (may be NULL => zeros)
 *   q   [B][n], g [B][n_c], G [B][n_c][n] dense row-major, Q [B][n][n] (raw,
 *   unsymmetrised), x [B][(N+1)*n_q], l0 [B][n_c] = max(0,-lsqr(GG^T, Gq)).
 */
int dgsqp_evaluate_batch(dgsqp_handle_t h, int64_t B, const double* x0, const double* u,
                         const double* l, double* q, double* g, double* G, double* Q,
                         double* x, double* l0);

/*
 * Test hook == DGSQP._solve_qp(Q, q, G, g) (DGSQP.py:232-266) on the game's
 * own constraint structure: evaluates at (u, l), PSD-projects Q (+reg) and
 * solves the QP.  du [B][n], lhat [B][n_c], Qpd [B][n][n] (projected +
 * regularised Hessian), flag [B] (0 ok, 1 infeasible / failed).
 */
int dgsqp_qp_batch(dgsqp_handle_t h, int64_t B, const double* x0, const double* u,
                   const double* l, double* du, double* lhat, double* Qpd, int32_t* flag);
/* The same hook with OSQP's diagnostics when the handle runs qp_method = DGSQP_QP_OSQP (zeros otherwise): info8 [B][8] = {OSQP status
   (1 solved, 2 solved inaccurate, -2 iteration limit, -3 primal infeasible, -4 dual infeasible, -10 non-finite data), ADMM iterations,
   polish (1 accepted, -1 rejected, 0 not attempted), final rho, rho updates, active rows handed to the polish, primal and dual residual
   of the ADMM iterate} -- what tests compare with the CPU restatements of OSQP (oracle/osqp.hpp, oracle/osqp_restate.py). */
int dgsqp_qp_batch_info(dgsqp_handle_t h, int64_t B, const double* x0, const double* u,
                        const double* l, double* du, double* lhat, double* Qpd, int32_t* flag, double* info8);

/* Warm start of a Monte-Carlo batch (row (f) of the hot-path scope): for every scenario and agent roll the PID lane follower
   out from q0[B][n_q] over the horizon with the agent's own continuous model (rk4).  u_ws[B][n] agent-major (what
   dgsqp_solve_batch takes); q_ws[B][(N+1) n_q] and collide[B] (1 = some pair closer than r_i + r_j at some stage,
   check_collision chicane.py:38-43) are optional.  Replaces the per-sample loop chicane.py:411-447 / curve.py:440-467. */
int dgsqp_pid_warm_start_batch(dgsqp_handle_t h, int64_t B, const double* q0, const dgsqp_pid_t* pid, double* u_ws,
                               double* q_ws, int32_t* collide);

/*
 * Rejection samplers of the Monte-Carlo scripts on the device (row (f) of the hot-path scope): random placement, PID warm start
 * (zero inputs for the merge), collision check along the warm start, accepted candidates kept in candidate order.  The random
 * numbers are counter-based (Philox4x32-10): uniform k of candidate c depends on (seed, c, k) only, so the host mirror
 * (dgsqp_amd/sampler.py) reproduces the stream bit for bit whatever the round sizes.
 *   DGSQP_SAMPLER_FIRST_SEGMENT  scripts/DGSQP_ALGAMES_monte_carlo_chicane.py:384-404, _curve.py (two cars)
 *   DGSQP_SAMPLER_INDEPENDENT    scripts/DGSQP_monte_carlo_agents.py:262-308 (M cars)
 *   DGSQP_SAMPLER_CIRCUIT        scripts/DGSQP_comp_monte_carlo.py:365-382 (M cars on a closed track)
 *   DGSQP_SAMPLER_MERGE          scripts/DGSQP_merge_monte_carlo.py:429-473 (unicycles, zero warm start)
 * key_pts: the arc track's key points (x, y, psi, cumulative length, segment length, signed curvature of the segment ENDING
 * there), n_key = segments + 1 (radius_arclength_track.py:361-408).  n_key = 0 on a spline-track handle: the CIRCUIT sampler places
 * the cars on the handle's spline (the other kinds need seg0_len and are refused).
 */
enum { DGSQP_SAMPLER_FIRST_SEGMENT = 0, DGSQP_SAMPLER_INDEPENDENT = 1, DGSQP_SAMPLER_CIRCUIT = 2, DGSQP_SAMPLER_MERGE = 3 };
typedef struct {
  int32_t kind;
  int32_t n_key;
  uint64_t seed;
  double half_width;   /* placement range of e_y */
  double obs_d;        /* obstacle distance of the relative placements */
  double seg0_len;     /* length of the first track segment */
  double x_nom[DGSQP_MAX_AGENTS];   /* merge: nominal x of every car (merge.py:430,443,456) */
  double key_pts[DGSQP_MAX_SEGS + 1][6];
} dgsqp_sampler_t;
/* Draw until B scenarios are accepted: x0_out [B][n_q], u_ws_out [B][n] agent-major (host, either may be NULL).  stage != 0: the
   batch also becomes the handle's staged input (as after dgsqp_stage_inputs) -- sampling, solve and statistics never leave the
   device.  *candidates (may be NULL) = candidates consumed, i.e. the index after the last accepted one. */
int dgsqp_sample_batch(dgsqp_handle_t h, int64_t B, const dgsqp_sampler_t* spec, const dgsqp_pid_t* pid, double* x0_out,
                       double* u_ws_out, int64_t* candidates, int stage);

/*
 * Test hook: event log of the SQP state machine (convergence measures, merit values, step lengths,
 * watchdog branches) of every scenario of the next solve calls; compared event-by-event with the
 * oracle's log.  Layout per scenario: [count, (code, value) x pairs_per_scenario].  0 disables.
 */
int dgsqp_set_trace(dgsqp_handle_t h, int pairs_per_scenario);
/* out: [B_launch][1 + 2 * pairs_per_scenario] of the last launch; capacity_doubles = what out can hold (DGSQP_E_ARG when it
   is too small).  A count above pairs_per_scenario means that scenario's log was truncated. */
int dgsqp_fetch_trace(dgsqp_handle_t h, double* out, int64_t capacity_doubles);

/* Iterate log for solve()'s iter_data / init (DGSQP.py:328, :386-451): per scenario [count, records x (n + n_c)], record 0 =
   (u_ws, dual start l), record i = (u, l) at the end of SQP iteration i (or at the exit test that ended the solve).
   0 disables (default: Monte-Carlo batches only keep the final iterates). */
int dgsqp_set_iterate_log(dgsqp_handle_t h, int records_per_scenario);
int dgsqp_fetch_iterate_log(dgsqp_handle_t h, double* out, int64_t capacity_doubles);

/* Wait for everything enqueued on the handle's stream (what a caller without a HIP runtime of its own uses as a fence). */
int dgsqp_synchronize(dgsqp_handle_t h);

/*
 * LTV-MPC reference tracker (DGSQP/solvers/CA_LTV_MPC.py, qp_interface 'casadi'), batched: row (f9) of the hot-path scope.  One agent
 * of the handle's game (its model, vehicle, integrator, dt and track) follows per-scenario reference trajectories: rollout of the warm
 * start, then qp_iters times { QP of the cost's Gauss-Newton model and the dynamics linearised at (q_k, u_{k-1}) about the current
 * decision vector D; D <- damping D + (1 - damping) D_bar; slacks (zero_du: and du) <- 0 }.  The QP is solved exactly (dense dual
 * active set on the condensed problem), where the reference calls OSQP.
 *   D = [(q_0, u_-1), ..., (q_N, u_N-1), du_0 .. du_N-1, s_ub, s_lb]      len_D = (N + 1)(n_q + n_u) + N n_u + 2 n_soft
 *   cost   sum_{k=0..N} 0.5 (q_k - q_ref_k)' diag(w_q) (q_k - q_ref_k) + c_N' q_N + sum_{k=0..N} 0.5 u_{k-1}' diag(w_u) u_{k-1}
 *          + sum_{k<N} 0.5 du_k' diag(w_du) du_k + soft_quad s^2 + soft_lin s        (+ the reference's 1e-10 I on every (q, u) block)
 *   boxes  u_lb <= u_{k-1} <= u_ub (k = 0..N), q_lb <= q_k <= q_ub (k = 1..N), du_lb <= du_k <= du_ub; a bound of magnitude >= 1e9
 *          generates no row.  The bounds of a soft state are lifted: q_k[j] <= q_ub[j] + s_ub, q_k[j] >= q_lb[j] - s_lb, s >= 0 (one
 *          slack pair over the horizon; n_soft <= 1: with more, the reference's rows of different states overwrite one another).
 *   obs_r > 0: one row per stage k = 1..N, (2 obs_r)^2 - |(x, y)_k - p_obs_k|^2 <= 0, linearised about D.
 *   edge_rows = 1: two hard rows per stage k = 1..N, the track's edges as the F1 study's tracker has them (comparison_study_f1/
 *          warm_start.py:112-118, its 'state_input' constraints, vertcat(right, left)):
 *            right  -right_width(s_k) - e_y,k <= 0        left  e_y,k - left_width(s_k) <= 0
 *          with the width functions of the handle's table (dgsqp_problem_t.widths), linearised about D as the obstacle row is: value
 *          c(q_bar_k) + grad c (q_k - q_bar_k), grad c over (s, e_y) = (-w'(s_bar), +-1), w' the slope of the table's piece.
 * zero_du != 0 is the loop of set_warm_start (CA_LTV_MPC.py:174-197): du of D is zeroed after every iteration, and a failed QP leaves
 * the current D as the result.  Otherwise a failed QP (status DGSQP_QP_FAIL) returns the warm start: q_ws, u_ws[1:], du_ws.
 * A u_prev (= u_ws[0]) more than 1e-12 max(1, |bound|) beyond an input bound makes every QP infeasible, as in the reference, where u_-1 is
 * both fixed and bounded; closer than that (a saturated input this tracker returned, fed back) it is moved onto the bound.
 */
typedef struct {
  int32_t agent, N, qp_iters, zero_du;
  double damping;
  double w_q[DGSQP_MAX_NQA], c_N[DGSQP_MAX_NQA], w_u[DGSQP_NUA], w_du[DGSQP_NUA];   /* w_du > 0: the QP is strictly convex */
  double q_ub[DGSQP_MAX_NQA], q_lb[DGSQP_MAX_NQA], u_ub[DGSQP_NUA], u_lb[DGSQP_NUA], du_ub[DGSQP_NUA], du_lb[DGSQP_NUA];
  int32_t n_soft;
  int32_t edge_rows;                                                                 /* 0, or 1: track-edge rows (this field was reserved_) */
  int32_t soft_idx[DGSQP_MAX_NQA];                   /* entries past n_soft (<= 1 today) are reserved: room for more soft states */
  double soft_quad[DGSQP_MAX_NQA], soft_lin[DGSQP_MAX_NQA];
  double obs_r;                                                                      /* 0: no obstacle rows */
} dgsqp_mpc_t;
/* rows of the condensed QP, x = (du_0 .. du_N-1, s_ub, s_lb): sign * value <= sign * bound */
enum { DGSQP_MPC_ROW_RATE = 0,   /* du_stage[index] */
       DGSQP_MPC_ROW_SLACK = 1,  /* slack index (0 .. 2 n_soft - 1), sign -1: s >= 0 */
       DGSQP_MPC_ROW_INPUT = 2,  /* u of block `stage` (1..N), i.e. u_{stage-1}[index] */
       DGSQP_MPC_ROW_STATE = 3,  /* q_stage[index] */
       DGSQP_MPC_ROW_SOFT = 4,   /* soft state `index` (slot) at `stage`: sign +1 the upper row, -1 the lower */
       DGSQP_MPC_ROW_OBS = 5,    /* obstacle row of `stage` */
       DGSQP_MPC_ROW_EDGE = 6 }; /* track-edge row of `stage`: sign +1 the left edge, -1 the right; after the obstacle rows, right before left */
typedef struct { int32_t kind, stage, index, sign; } dgsqp_mpc_row_t;
typedef struct { int32_t n, n_rows, len_D, n_q, lds_bytes, reserved_; int64_t workspace_bytes; } dgsqp_mpc_dims_t;
#define DGSQP_MPC_NMAX 128   /* condensed variables: N n_u + 2 n_soft */
/* Validated and copied; NULL clears it.  DGSQP_E_ARG, message starting "mpc: ": agent out of range, N < 1, qp_iters < 1, damping outside
   [0, 1], w_du <= 0, a negative weight, n_soft outside 0..1 or its index out of range, obs_r < 0, a non-finite entry, edge_rows outside
   0..1, edge_rows = 1 on a handle without a width table or for a unicycle agent.
   DGSQP_E_TOO_LARGE: N n_u + 2 n_soft > DGSQP_MPC_NMAX, or the workgroup's LDS arena cannot hold it (the 256-thread build has half). */
int dgsqp_set_mpc(dgsqp_handle_t h, const dgsqp_mpc_t* mpc);
/* rows: the row table in the order of the multipliers of dgsqp_fetch_mpc_log (may be NULL); row_capacity = what it can hold. */
int dgsqp_mpc_dims(dgsqp_handle_t h, dgsqp_mpc_dims_t* out, dgsqp_mpc_row_t* rows, int64_t row_capacity);
/* q0 [B][n_q] (n_q of the agent), u_ws [B][N+1][n_u] (row 0 = u_prev), du_ws [B][N][n_u], q_ref [B][N+1][n_q], p_obs [B][N][2] (stage
   1..N; required when obs_r > 0, else ignored); out: q_pred [B][N+1][n_q], u_pred [B][N][n_u], du_pred [B][N][n_u], status [B] (0 or
   DGSQP_QP_FAIL), qp_steps [B] (active-set steps of all QPs), each may be NULL. */
int dgsqp_mpc_batch(dgsqp_handle_t h, int64_t B, const double* q0, const double* u_ws, const double* du_ws, const double* q_ref,
                    const double* p_obs, double* q_pred, double* u_pred, double* du_pred, int32_t* status, int32_t* qp_steps,
                    dgsqp_timing_t* timing);
/* Test hook: per-iteration log of the next dgsqp_mpc_batch calls: D before the iteration, D_bar, the multipliers of the rows.  An
   iteration that did not run (after a failed QP) and a failed QP's D_bar / multipliers are NaN. */
int dgsqp_set_mpc_log(dgsqp_handle_t h, int on);
/* D, D_bar [B][qp_iters][len_D], lam [B][qp_iters][n_rows] of the last launch; capacity = scenarios each array can hold. */
int dgsqp_fetch_mpc_log(dgsqp_handle_t h, double* D, double* D_bar, double* lam, int64_t capacity);

/*
 * Raceline warm starts: the front end of scripts/comparison_study_barc/monte_carlo_main.py (monte_carlo_sampler_dynamic.py,
 * warm_start_dynamic.py) on the device.
 *
 * The raceline is the two-lap, time-parametrised table of track_lib.load_mpclab_raceline: n knots T (strictly increasing) and nine
 * columns (x, y, psi, v_long, v_tran, psidot, e_psi, s, e_y), s strictly increasing.  Two look-ups (csrc/dgsqp_raceline.h): s2t(s),
 * linear interpolation of T over the s column, and raceline(t), linear over T; both find their segment by binary search and continue
 * the first / last segment linearly outside the table (what CasADi's 'linear' interpolant is understood to do: a stated definition).
 * dgsqp_set_raceline validates and copies the table to the device; T = NULL or cols = NULL clears it.  DGSQP_E_ARG, message starting
 * "raceline: ": n < 2, a non-finite entry, T or the s column not strictly increasing.
 */
#define DGSQP_RL_COLS 9
int dgsqp_set_raceline(dgsqp_handle_t h, int64_t n, const double* T /* [n] */, const double* cols /* [n][9] */);

/*
 * The warm-start program of warm_start_dynamic.py:145-165 for every agent of a batch, stream-ordered on the device:
 *   reference   t0 = s2t(s_0), offset = e_y0 - raceline(t0)[8], scaling = v_long0 / raceline(t0)[3], t_k = t0 + dt k scaling,
 *               q_ref_k = raceline(t_k)[3:] with the three velocities multiplied by scaling and e_y shifted by offset, laid out for the
 *               agent's model: dynamic bicycle (x, y, v_long, v_tran, psidot, e_psi, s, e_y), kinematic bicycle (x, y, v_long, e_psi,
 *               s, e_y); x, y come from the raceline (give them zero weight).  Unicycle models are refused.
 *   phase 1     the tracker (dg_mpc_kernel) with zero_du, init_iters iterations and init_damping from u_ws = u_init, du_ws = du_init:
 *               the loop of CA_LTV_MPC.set_warm_start; its status is ignored, as the reference ignores it
 *   chain       u_ws <- (u_ws[0], u_pred), du_ws <- du_pred
 *   phase 2     the tracker with the template's qp_iters and damping: CA_LTV_MPC.solve
 *   assemble    u_pred of phase 2 into the game's agent-major u_ws; ok &= (status == 0)
 * mpc.agent and mpc.zero_du are ignored; the record is planned per agent (what dgsqp_set_mpc refuses is refused here, message starting
 * "mpc: ").  The handle's own tracker setting (dgsqp_set_mpc) is not touched.
 */
typedef struct {
  dgsqp_mpc_t mpc;
  double u_init, du_init;   /* warm_start_dynamic.py:156-157: 0.01 */
  int32_t init_iters, reserved_;
  double init_damping;      /* CA_LTV_MPC.py:174-197: 2 iterations, damping 0.5 */
} dgsqp_raceline_ws_t;
/* x0 [B][n_q] (host), or NULL: the handle's staged batch of B scenarios, whose staged u_ws then receives the result
   (dgsqp_solve_staged may follow).  u_ws_out [B][n] agent-major, ok_out [B] (1: every agent's phase 2 succeeded); each may be NULL.
   DGSQP_E_ARG, message starting "raceline: ": no raceline set, a unicycle agent, agents of different models, B < 0, x0 = NULL without a
   staged batch of that size. */
int dgsqp_raceline_warm_start_batch(dgsqp_handle_t h, int64_t B, const double* x0, const dgsqp_raceline_ws_t* ws, double* u_ws_out,
                                    int32_t* ok_out);
/* Test hook: q_ref [B][M][N+1][n_qa] of the last dgsqp_raceline_warm_start_batch (of the last round of dgsqp_sample_raceline_batch);
   capacity_doubles = what out can hold (DGSQP_E_ARG when it is too small or when no such call has run). */
int dgsqp_fetch_raceline_ref(dgsqp_handle_t h, double* out, int64_t capacity_doubles);

/*
 * The sampler of monte_carlo_sampler_dynamic.py:27-57 (two cars), in the rounds of dgsqp_sample_batch with the same counter-based
 * uniforms, six per candidate: s1 = L u0, e_y1 = clip(raceline e_y + (2 u1 - 1), -+0.9 half_width), v1 = raceline v_long + (1.5 u2 - 0.75),
 * e_psi1 = the raceline's; s2 = s1 + 1.2 obs_d (2 u3 - 1) and the rest likewise from the raceline at s2 with u4, u5.  A candidate is
 * rejected when collision_d^2 - |p1 - p2|^2 >= 0, or when the warm-start program reports ok = 0 (the study redraws both).
 */
typedef struct {
  int32_t n_key, reserved_;
  uint64_t seed;
  double half_width, obs_d;
  double collision_d;       /* r1 + r2; the study: 2 sqrt((0.37 / 2)^2 + (0.195 / 2)^2) */
  double key_pts[DGSQP_MAX_SEGS + 1][6];
} dgsqp_raceline_sampler_t;
/* x0_out, u_ws_out, candidates, stage: as dgsqp_sample_batch. */
int dgsqp_sample_raceline_batch(dgsqp_handle_t h, int64_t B, const dgsqp_raceline_sampler_t* spec, const dgsqp_raceline_ws_t* ws,
                                double* x0_out, double* u_ws_out, int64_t* candidates, int stage);

/*
 * The sampler of scripts/comparison_study_f1/monte_carlo_sampler.py:25-55 on a spline-track handle (two cars), in the same rounds with the
 * same uniforms: s1 = s_lo + (s_hi - s_lo) u0; s2 = s1 + gap_lo + (gap_hi - gap_lo) u3 (car 2 starts ahead of car 1); per car
 * e_y = clip(raceline e_y + (2 u - 1), -+ey_clip), v = raceline v_long + (1.5 u - 0.75), e_psi = the raceline's (u1, u2 for car 1; u4, u5
 * for car 2).  ey_clip is one constant bound.  After dgsqp_set_raceline_clip with clip_widths = 1: the study's clip with the track's width functions
 * (monte_carlo_sampler.py:29,38; clip_scale = 0.9 there), each car at its own s:
 *   e_y = max(min(raceline e_y + (2 u - 1), clip_scale left_width(s)), -clip_scale right_width(s))
 * from the handle's width table (dgsqp_problem_t.widths, csrc/dgsqp_track_width.h); ey_clip is ignored.  Rejection as
 * dgsqp_sample_raceline_batch.  DGSQP_E_ARG, message starting "raceline: ": an arc-track handle, a non-finite entry, s_hi < s_lo,
 * gap_hi < gap_lo, ey_clip < 0, collision_d < 0, and what dgsqp_sample_raceline_batch refuses.
 */
typedef struct {
  uint64_t seed;
  double s_lo, s_hi, gap_lo, gap_hi, ey_clip, collision_d;
} dgsqp_raceline_spline_sampler_t;
int dgsqp_sample_raceline_spline_batch(dgsqp_handle_t h, int64_t B, const dgsqp_raceline_spline_sampler_t* spec, const dgsqp_raceline_ws_t* ws,
                                       double* x0_out, double* u_ws_out, int64_t* candidates, int stage);
/* The e_y clip of the handle's SUBSEQUENT dgsqp_sample_raceline_spline_batch calls (sticky, like dgsqp_set_plant; the record above keeps
   its 56 bytes).  clip_widths = 0 (the state of a new handle): the constant ey_clip; clip_scale is not read.  clip_widths = 1: the width
   functions as above.  DGSQP_E_ARG, message starting "raceline: ": clip_widths outside 0 .. 1, clip_widths = 1 on a handle without a width
   table or with a clip_scale that is negative or not finite; the setting in force is kept then. */
int dgsqp_set_raceline_clip(dgsqp_handle_t h, int clip_widths, double clip_scale);

/*
 * Track-frame transforms for batches of points (csrc/dgsqp_track_frame.h), one lane per point, on the handle's stream.
 *   n_key = 0   the handle's spline track (dgsqp_problem_t.spline): Frenet -> global is CasadiBSplineTrack.local_to_global; global ->
 *               Frenet is the foot point reached from the closest piece start K_j by 30 Newton steps on g(s) = (c(s) - p) . c'(s), clipped
 *               to [K_j - 1.5 D, K_j + 1.5 D] with D = K_1 - K_0 (the reference starts an NLP from the closest waypoint); a table whose ends
 *               do not meet is not wrapped: s is clipped to [0, L]
 *   n_key > 0   an arc track given by its key points (as dgsqp_sampler_t.key_pts; the handle's problem does not hold them):
 *               radius_arclength_track.py:752-807 and :644-743
 * half_width, slack: a projection with |e_y| > half_width + slack is off the track.
 * cl [n][3] = (s, e_y, e_psi), xy [n][3] = (x, y, psi).  status [n]: 0 fine; 1 an input is not finite (outputs NaN); 2 off the track
 * (spline: the values are still returned; arcs: no segment takes the point, outputs NaN).  resid [n] (may be NULL): the final g on a
 * spline, 0 on arcs.  n = 0: DGSQP_OK.  DGSQP_E_ARG, message starting "track frame: ": n < 0, a NULL pointer, n_key = 0 on an arc-track
 * handle, n_key > 0 on a spline-track handle, n_key outside 2 .. DGSQP_MAX_SEGS + 1, a non-finite entry, a track length that is not positive.
 */
typedef struct {
  int32_t n_key;
  int32_t _pad;
  double half_width, slack;
  double key_pts[DGSQP_MAX_SEGS + 1][6];
} dgsqp_track_frame_t;
int dgsqp_local_to_global_batch(dgsqp_handle_t h, int64_t n, const dgsqp_track_frame_t* t, const double* cl /* [n][3] s, e_y, e_psi */,
                                double* xy /* [n][3] x, y, psi */);
int dgsqp_global_to_local_batch(dgsqp_handle_t h, int64_t n, const dgsqp_track_frame_t* t, const double* xy, double* cl,
                                double* resid /* may be NULL */, int32_t* status);


/*
 * Multi-GPU (one process per GPU, scenarios sharded, no data-path collective): the library owns the RCCL communicator.
 *   dgsqp_comm_unique_id   rank 0: 128-byte ncclUniqueId to hand to the other ranks (file, socket, environment ...)
 *   dgsqp_comm_init        every rank: ncclCommInitRank on the handle's device (collective call)
 *   dgsqp_gather_stats     the ONE collective per batch: ncclAllGather over xGMI of the 88-byte records of the handle's last solve.
 *                          B_pad = the largest shard (shards may differ by one scenario); out[world * B_pad] in rank order, padding
 *                          rows carry status -1.  Every rank receives all records.
 *   dgsqp_comm_barrier, dgsqp_comm_allreduce_max   fences / max-over-ranks of small host vectors for benchmark timing
 * world = 1 works without any peer (and is what the single-GPU test exercises).
 */
int dgsqp_comm_unique_id(char* out128);
int dgsqp_comm_init(dgsqp_handle_t h, const char* id128, int rank, int world);
int dgsqp_comm_destroy(dgsqp_handle_t h);
int dgsqp_gather_stats(dgsqp_handle_t h, int64_t B_pad, dgsqp_stat_record_t* out);
int dgsqp_comm_barrier(dgsqp_handle_t h);
int dgsqp_comm_allreduce_max(dgsqp_handle_t h, double* values, int count);

#ifdef __cplusplus
}
#endif
#endif /* DGSQP_H */
