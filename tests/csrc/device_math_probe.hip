// Test infrastructure, never loaded by the product: one-workgroup kernels that apply ONE device primitive of csrc/dgsqp_device.h or
// csrc/dgsqp_eval.h elementwise to arrays in global memory (tests/test_device_math.py, helper tests/device_math_probe.py).
//
// This translation unit includes the product's own dgsqp_api.hip (found through -I, so that the same probe can be built against
// another revision of the headers): the handle comes from dgsqp_create, the constant block dg_prob from upload_problem, the atan and
// track tables from dev_load_tables -- nothing of them is restated here.
//
// Lane i of wavefront w handles element DG_BLOCK * pass + 64 * w + i: every aligned group of 64 consecutive elements shares one
// wavefront (the wave-uniform fast paths of the roll_* functions and the wave reductions see exactly that group).  The element
// count is a multiple of 64 (DG_BLOCK for the block reductions), so every wavefront that works has all of its lanes active.
#include "dgsqp_api.hip"

enum {
  PR_RCP = 0, PR_SINCOS, PR_TAN, PR_ATAN, PR_ATAN2, PR_ROLL_ATAN, PR_ROLL_ATAN2, PR_ROLL_SIN, PR_ROLL_SINCOS,
  PR_TY_RECIP, PR_TY_MUL, PR_TY_DIV, PR_TY_SINCOS, PR_TY_TAN, PR_TY_ATAN, PR_TY_ATAN2, PR_TY_SQRT, PR_TY_POW, PR_TY_ABS,
  PR_WRAP_S, PR_TRACK, PR_TRACK_SPLINE,
  PR_WAVE_SUM, PR_WAVE_MAX, PR_WAVE_ARGMIN, PR_BLOCK_SUM, PR_BLOCK_MAX, PR_BLOCK_ARGMIN,
  PR_COUNT
};
// planes of n doubles each op reads and writes (the host entry point checks the caller's buffers against these)
static const int pr_nin[PR_COUNT] = {1, 1, 1, 1, 2, 1, 2, 1, 1, 3, 6, 6, 3, 3, 3, 6, 3, 3, 3, 1, 3, 3, 1, 1, 2, 1, 1, 2};
static const int pr_nout[PR_COUNT] = {1, 2, 1, 1, 1, 1, 1, 1, 2, 3, 3, 3, 6, 3, 3, 3, 3, 3, 3, 1, 4, 6, 1, 1, 2, 1, 1, 2};

typedef Ty<2> T2;
__device__ inline T2 pr_ld(const double* in, int64_t n, int plane, int64_t e) {
  T2 r;
  r.c[0] = in[plane * n + e]; r.c[1] = in[(plane + 1) * n + e]; r.c[2] = in[(plane + 2) * n + e];
  return r;
}
__device__ inline void pr_st(double* out, int64_t n, int plane, int64_t e, const T2& v) {
  out[plane * n + e] = v.c[0]; out[(plane + 1) * n + e] = v.c[1]; out[(plane + 2) * n + e] = v.c[2];
}

__global__ void __launch_bounds__(DG_BLOCK)
dg_probe_kernel(int op, int64_t n, const double* __restrict__ in, double* __restrict__ out, double p) {
  dev_load_tables();
  const DgProb& D = dg_prob;
  if (op >= PR_BLOCK_SUM) {      // every thread takes part in every pass (barriers inside)
    lptr red = LP(D.L.red);
    for (int64_t base = 0; base < n; base += DG_BLOCK) {
      const int64_t e = base + TID;
      const double v = in[e];
      if (op == PR_BLOCK_SUM) out[e] = block_sum(v, red);
      else if (op == PR_BLOCK_MAX) out[e] = block_max(v, red);
      else {
        double vo; int io;
        block_argmin(v, (int)in[n + e], red, vo, io);
        out[e] = vo; out[n + e] = (double)io;
      }
      __syncthreads();
    }
    return;
  }
  for (int64_t e = TID; e < n; e += DG_BLOCK) {
    const double a = in[e];
    switch (op) {      // uniform
      case PR_RCP: out[e] = fast_rcp(a); break;
      case PR_SINCOS: { double s, c; dev_sincos(a, s, c); out[e] = s; out[n + e] = c; } break;
      case PR_TAN: out[e] = dev_tan(a); break;
      case PR_ATAN: out[e] = dev_atan(a); break;
      case PR_ATAN2: out[e] = dev_atan2(a, in[n + e]); break;
      case PR_ROLL_ATAN: out[e] = roll_atan(a); break;
      case PR_ROLL_ATAN2: out[e] = roll_atan2(a, in[n + e]); break;
      case PR_ROLL_SIN: out[e] = roll_sin(a); break;
      case PR_ROLL_SINCOS: { double s, c; roll_sincos(a, s, c); out[e] = s; out[n + e] = c; } break;
      case PR_TY_RECIP: pr_st(out, n, 0, e, ty_recip(pr_ld(in, n, 0, e))); break;
      case PR_TY_MUL: pr_st(out, n, 0, e, pr_ld(in, n, 0, e) * pr_ld(in, n, 3, e)); break;
      case PR_TY_DIV: pr_st(out, n, 0, e, pr_ld(in, n, 0, e) / pr_ld(in, n, 3, e)); break;
      case PR_TY_SINCOS: { T2 s, c; ty_sincos(pr_ld(in, n, 0, e), s, c); pr_st(out, n, 0, e, s); pr_st(out, n, 3, e, c); } break;
      case PR_TY_TAN: pr_st(out, n, 0, e, ty_tan(pr_ld(in, n, 0, e))); break;
      case PR_TY_ATAN: pr_st(out, n, 0, e, ty_atan(pr_ld(in, n, 0, e))); break;
      case PR_TY_ATAN2: pr_st(out, n, 0, e, ty_atan2(pr_ld(in, n, 0, e), pr_ld(in, n, 3, e))); break;
      case PR_TY_SQRT: pr_st(out, n, 0, e, ty_sqrt(pr_ld(in, n, 0, e))); break;
      case PR_TY_POW: pr_st(out, n, 0, e, ty_pow(pr_ld(in, n, 0, e), p)); break;
      case PR_TY_ABS: pr_st(out, n, 0, e, ty_abs(pr_ld(in, n, 0, e))); break;
      case PR_WRAP_S: out[e] = wrap_s(a, D.P.track_L, D.inv_track_L); break;
      case PR_TRACK: { double curv; T2 psi; dev_track<2>(D.P, pr_ld(in, n, 0, e), curv, psi); out[e] = curv; pr_st(out, n, 1, e, psi); } break;
      case PR_TRACK_SPLINE: { T2 curv, psi; dev_track_spline<2>(D.P, pr_ld(in, n, 0, e), curv, psi); pr_st(out, n, 0, e, curv); pr_st(out, n, 3, e, psi); } break;
      case PR_WAVE_SUM: out[e] = wave_sum(a); break;
      case PR_WAVE_MAX: out[e] = wave_max(a); break;
      case PR_WAVE_ARGMIN: { double v = a; int idx = (int)in[n + e]; wave_argmin(v, idx); out[e] = v; out[n + e] = (double)idx; } break;
      default: break;
    }
  }
}

// The single-wavefront rollout of the dynamic bicycle (dev_rollout_dyn<DYN_BOTH>) on lanes < 2 M of wavefront 0, inputs in LDS where
// dev_evaluate keeps them.  No ring, no progress word: nothing in this mode waits.
// u sits in L.u, du in L.e_ue and the trajectory in L.e_x side by side (dev_evaluate itself keeps only the stepped input, in e_ue): this
// relies on dgsqp_layout.h handing out disjoint ranges for the three in every layout -- take(n) for L.u in the persistent part of the
// arena, take((N + 1) n_q) for L.e_x and take(n) for L.e_ue behind L.scr, unconditionally.
__global__ void __launch_bounds__(DG_BLOCK)
dg_probe_rollout_both_kernel(const double* __restrict__ x0, const double* __restrict__ u, const double* __restrict__ du, double alpha,
                             double* __restrict__ x) {
  dev_load_tables();
  const DgProb& D = dg_prob;
  const DgLds& L = D.L;
  lptr ub = LP(L.u), dub = LP(L.e_ue), xs = LP(L.e_x);
  for (int i = TID; i < D.n; i += NT) { ub[i] = u[i]; dub[i] = du ? du[i] : 0.0; }
  for (int i = TID; i < D.nq; i += NT) xs[i] = x0[i];
  __syncthreads();
  DynRing R;
  R.buf = nullptr; R.vprog = nullptr; R.pprog = nullptr; R.mask = 0; R.stride = 0; R.off = 0;      // not read in this mode
  const int lane = TID & 63;
  if (TID < 64 && lane < 2 * D.M)
    dev_rollout_dyn<DYN_BOTH>(D, lane >> 1, lane & 1, R, ub, du ? (clptr)dub : (clptr)nullptr, alpha, xs, nullptr);
  __syncthreads();
  for (int i = TID; i < (D.N + 1) * D.nq; i += NT) x[i] = xs[i];
}

static int probe_prepare(dgsqp_solver* h, const void* kernel) {
  HIPCHK(h, hipSetDevice(h->device));
  { const int rc = wait_idle(h); if (rc) return rc; }
  HIPCHK(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
  return DGSQP_OK;
}

extern "C" {

int dgsqp_probe_block(void) { return DG_BLOCK; }

// in: nin planes of n doubles, out: nout planes of n doubles (host memory); n a multiple of 64 (of DG_BLOCK for the block reductions)
int dgsqp_probe_run(dgsqp_handle_t h, int op, int64_t n, int nin, const double* in, int nout, double* out, double p) {
  if (!h || !in || !out) return DGSQP_E_ARG;
  if (op < 0 || op >= PR_COUNT || nin != pr_nin[op] || nout != pr_nout[op] || n <= 0 || n % (op >= PR_BLOCK_SUM ? DG_BLOCK : 64) != 0) {
    h->err = "probe: bad op, plane count or element count"; return DGSQP_E_ARG;
  }
  const bool spline = h->hp.P.track_kind == DGSQP_TRACK_SPLINE;
  if ((op == PR_TRACK_SPLINE && !spline) || (op == PR_TRACK && spline)) { h->err = "probe: track kind of the handle does not fit the op"; return DGSQP_E_ARG; }
  { const int rc = probe_prepare(h, (const void*)dg_probe_kernel); if (rc) return rc; }
  TmpBuf tb;
  double* din = tb.alloc<double>((size_t)nin * n);
  double* dout = tb.alloc<double>((size_t)nout * n);
  if (!din || !dout) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(din, in, sizeof(double) * nin * n, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemset(dout, 0, sizeof(double) * nout * n));
  std::unique_lock<std::mutex> game_lock(g_reg_mutex);
  { const int rc = upload_problem(h); if (rc) return rc; }
  hipLaunchKernelGGL(dg_probe_kernel, dim3(1), dim3(DG_BLOCK), h->lds_bytes, h->stream, op, n, din, dout, p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, dout, sizeof(double) * nout * n, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

// x[(N + 1) n_q] = dev_rollout_dyn<DYN_BOTH> from x0[n_q] under the inputs u[n] (agent-major), or fma(alpha, du, u) where du is given
int dgsqp_probe_rollout_both(dgsqp_handle_t h, const double* x0, const double* u, const double* du, double alpha, double* x) {
  if (!h || !x0 || !u || !x) return DGSQP_E_ARG;
  const DgProb& D = h->hp;
  bool ok = D.P.track_kind == DGSQP_TRACK_ARCS && 2 * D.M <= 64;
  for (int a = 0; a < D.M; a++) ok = ok && D.nqa[a] == 8;
  if (!ok) { h->err = "probe: the pair rollout needs dynamic bicycles on an arc track"; return DGSQP_E_ARG; }
  { const int rc = probe_prepare(h, (const void*)dg_probe_rollout_both_kernel); if (rc) return rc; }
  TmpBuf tb;
  const size_t nx = (size_t)(D.N + 1) * D.nq;
  double* dx0 = tb.alloc<double>(D.nq); double* du_ = tb.alloc<double>(D.n); double* ddu = du ? tb.alloc<double>(D.n) : nullptr;
  double* dx = tb.alloc<double>(nx);
  if (!dx0 || !du_ || (du && !ddu) || !dx) { h->err = "hipMalloc failed"; return DGSQP_E_NOMEM; }
  HIPCHK(h, hipMemcpy(dx0, x0, sizeof(double) * D.nq, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(du_, u, sizeof(double) * D.n, hipMemcpyHostToDevice));
  if (du) HIPCHK(h, hipMemcpy(ddu, du, sizeof(double) * D.n, hipMemcpyHostToDevice));
  std::unique_lock<std::mutex> game_lock(g_reg_mutex);
  { const int rc = upload_problem(h); if (rc) return rc; }
  hipLaunchKernelGGL(dg_probe_rollout_both_kernel, dim3(1), dim3(DG_BLOCK), h->lds_bytes, h->stream, dx0, du_, ddu, alpha, dx);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(x, dx, sizeof(double) * nx, hipMemcpyDeviceToHost));
  return DGSQP_OK;
}

}  // extern "C"
