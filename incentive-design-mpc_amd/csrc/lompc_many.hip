// lompc_many.hip — lompc_solve_many: K unrelated LoMPC QPs, each with its own prices
// (lmbd, lmbd_r, gamma), in one launch.
//
// Replaces a Python loop of LoMPC.solve_lompc (chargingstation/lompc.py:137-156) over QPs that
// share nothing: the reference's own timing harness draws fresh lmbd, lmbd_r and gamma for every
// solve (test/test_lompc.py:30-40), and per-EV (personalised) incentives are exactly this batch.
//
//   k_many        one 64-lane wave per QP (lane t = stage t), MANY_WAVES waves per workgroup so the
//                 box table is built once per workgroup: the QP's stage data from its price vector
//                 as k_central forms it, lqw::wave_solve from k_central's cold working set (or, with
//                 LOMPC_MANY_WARM, the fp64 PDAS straight from the caller's working set), the
//                 outputs in wave form, coalesced row store of w, lane-0 stores of the scalars.
//   k_many_close  one thread: counts[0] = K - (repaired + failed + invalid).
//
// The call keeps no state: it reads neither the context's parameter sets nor its mode and leaves
// the status rows of lompc_last_status alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lompc_ctx.hpp"
#include "lompc_wave.hpp"

#define MANY_WAVES 4                 // waves (QPs) per workgroup
#define MANY_CHUNK (1ll << 24)       // QPs per launch (grid x block stays below 2^32 threads)

struct ManyArgs {
  int64_t K;            // QPs of the whole call
  int64_t j0;           // first QP of this launch
  int64_t lmbd_stride;  // doubles between price vectors (0: one shared vector)
  const double* lmbd;
  const double* lmbd_r;  // or null (= 0)
  const double* gamma;
  const double* w_ref;   // or null
  uint8_t* ws;           // [K][LQ_STB] or null
  double* w;
  double* cost;
  double* w0;
  double* price0;
  double* err;
  int8_t* status;
  unsigned long long* counts;  // [4] or null
};

struct ManyOut {
  double cost, err, price0;
};

// Cost (lompc.py:155, incl. c0 and the PWL term), A_bar error (price_solver.py:191-192, :207) and
// price0 (lompc.py:164-170) of the QP held by the wave (lane t = w_t): the wave form of lq_outputs
// with the stage data in registers.  One prefix scan for y = A w and A (w - w_ref), one for the four
// sums.  l0: (lmbd1_0, lmbd2_0, lmbd3_0).  Result on every lane.
__device__ __forceinline__ ManyOut many_outputs(const QPConst& q, const lqw::WaveSet& ws, double gamma, double c0,
                                                const double (&l0)[3], double lr, double w, double wr,
                                                bool want_err) {
  const int N = ws.N;
  const bool act = ws.lane < N;
  lqw::Aff<2> h = lqw::Aff<2>::identity();
  if (act) {
    h.B[0] = w;
    h.B[1] = w - wr;
  }
  const lqw::Aff<2> Y = lqw::wave_scan(h, N);
  const double y = Y.B[0], ey = Y.B[1];
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // smooth terms, PWL, (A dw)^2, dw^2
  if (act) {
    v[0] = 0.5 * q.c * y * y - q.c * gamma * y + w * fma(0.5 * ws.d_nat, w, ws.e_nat);
    if (!q.ev_small) v[1] = lq_pwl(w * q.inv_wmax);
    v[2] = ey * ey;
    v[3] = (w - wr) * (w - wr);
  }
  lqw::wave_totals(v, N);
  const double tw = q.theta * q.w_max;
  ManyOut o;
  o.cost = v[0] + c0 + (q.ev_small ? 0.0 : tw * tw * v[1]);
  o.err = want_err ? sqrt(v[2] + (lr / q.delta) * v[3]) : 0.0;  // kappa = lmbd_r / delta, price_solver.py:191
  const double w0 = lqw::readlane_d(w, 0);
  o.price0 = q.theta * (w0 * l0[0] + (q.w_max - w0) * l0[1]) + q.q_scale * w0 * w0 * l0[2] +
             q.theta * q.theta * w0 * w0 * lr;
  return o;
}

// lqw::wave_solve from a caller's working set: no fp32 search (as wave_solve_path(..., warm = true)),
// the fp64 PDAS from s, the KKT certificate, the primal active set if needed.  nit as wave_solve's.
__device__ __forceinline__ bool many_solve_warm(const QPConst& q, const lqw::WaveSet& ws, double gamma, int& s,
                                                double& w, double& r, int* nit) {
  int n64 = 0;
  bool ok = lqw::wave_pdas(q, ws, gamma, s, w, r, min(4 * ws.N + 8, LQ_PDAS_CAP), &n64);
  *nit = n64;
  if (ok) ok = lqw::wave_kkt(q, ws, s, w, r) <= q.tol_cert;
  if (!ok) {
    *nit += 65536;
    ok = lqw::wave_primal_as(q, ws, gamma, s, w, r, 16 * ws.N + 32, true);
    if (ok) ok = lqw::wave_kkt(q, ws, s, w, r) <= q.tol_cert;
  }
  const Box b = lq_box(ws.lane < ws.N ? s : 0);
  w = fmin(fmax(w, b.lo), b.hi);
  return ok;
}

template <bool WARM>
__global__ __launch_bounds__(64 * MANY_WAVES) void k_many(QPConst q, ManyArgs a) {
  lq_tab_init(q);
  const int lane = threadIdx.x & 63;
  const int N = q.N;
  const int64_t j = a.j0 + (int64_t)blockIdx.x * MANY_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (j >= a.K) return;  // (wave-uniform, behind the workgroup's only barrier)
  const bool act = lane < N;
  const double* L = a.lmbd + j * a.lmbd_stride;
  const double lr = a.lmbd_r ? a.lmbd_r[j] : 0.0;
  const double g = a.gamma[j];
  double l1 = 0.0, l2 = 0.0, l3 = 0.0;
  if (act) {
    l1 = L[lane];
    l2 = L[N + lane];
    l3 = L[2 * N + lane];
  }
  const double wr = (a.w_ref && act) ? a.w_ref[j * N + lane] : 0.0;
  int sl = act ? 1 : 0;  // k_central's cold working set
  if (WARM && act) sl = min((int)a.ws[j * LQ_STB + lane], 2 * q.m);
  const bool bad = act && !(l1 >= 0.0 && l2 >= 0.0 && l3 >= 0.0);
  const bool valid = !__any(bad) && (lr >= 0.0) && (g >= 0.0) && (g <= q.y_max);
  if (!valid) {  // row and every requested scalar NaN
    if (a.w && act) a.w[j * N + lane] = NAN;
    if (a.ws) a.ws[j * LQ_STB + lane] = (uint8_t)(act ? 1 : 0);
    if (lane == 0) {
      if (a.cost) a.cost[j] = NAN;
      if (a.w0) a.w0[j] = NAN;
      if (a.price0) a.price0[j] = NAN;
      if (a.err) a.err[j] = NAN;
      if (a.status) a.status[j] = LOMPC_QP_INVALID;
      if (a.counts) atomicAdd(a.counts + LOMPC_QP_INVALID, 1ull);
    }
    return;
  }
  // stage data as k_central forms it (lompc.py:105, :126-133)
  const double tt = q.theta * q.theta;
  lqw::WaveSet ws;
  ws.N = N;
  ws.lane = lane;
  ws.d_nat = act ? 2.0 * lr * tt + 2.0 * q.q_scale * l3 + q.dsmall : 0.0;
  ws.e_nat = act ? q.theta * (l1 - l2) : 0.0;
  const double c0 = q.theta * q.w_max * lqw::wave_sum(l2, N);  // lompc.py:128
  const double l0[3] = {lqw::readlane_d(l1, 0), lqw::readlane_d(l2, 0), lqw::readlane_d(l3, 0)};
  double w = 0.0, r = 0.0;
  int nit = 0;
  const bool ok = WARM ? many_solve_warm(q, ws, g, sl, w, r, &nit) : lqw::wave_solve(q, ws, g, sl, w, r, &nit);
  const int st = !ok ? LOMPC_QP_FAILED : (nit >= 65536 ? LOMPC_QP_REPAIRED : LOMPC_QP_OK);
  if (a.w && act) a.w[j * N + lane] = w;
  if (a.ws) a.ws[j * LQ_STB + lane] = (uint8_t)(act ? sl : 0);
  const bool scalars = a.cost || a.price0 || a.err;
  ManyOut o{0.0, 0.0, 0.0};
  if (scalars) o = many_outputs(q, ws, g, c0, l0, lr, w, wr, a.err != nullptr);
  if (lane == 0) {
    if (a.cost) a.cost[j] = o.cost;
    if (a.w0) a.w0[j] = w;
    if (a.price0) a.price0[j] = o.price0;
    if (a.err) a.err[j] = o.err;
    if (a.status) a.status[j] = (int8_t)st;
    if (a.counts && st != LOMPC_QP_OK) atomicAdd(a.counts + st, 1ull);
  }
}

__global__ void k_many_close(unsigned long long* counts, int64_t K) {
  counts[LOMPC_QP_OK] =
      (unsigned long long)K - counts[LOMPC_QP_REPAIRED] - counts[LOMPC_QP_FAILED] - counts[LOMPC_QP_INVALID];
}

extern "C" int lompc_solve_many(lompc_ctx* c, int64_t K, const double* lmbd, int64_t lmbd_stride,
                                const double* lmbd_r, const double* gamma, const double* w_ref, uint8_t* ws,
                                int flags, double* w, double* cost, double* w0, double* price0, double* err,
                                int8_t* status, int64_t* counts, void* stream) {
  if (!c) return LOMPC_ERR_INVALID_ARG;
  if (K < 0) return fail_arg(c, "solve_many: K >= 0 required");
  if (!lmbd || !gamma) return fail_arg(c, "solve_many: lmbd and gamma required");
  if (lmbd_stride != 0 && lmbd_stride < 3 * (int64_t)c->N)
    return fail_arg(c, "solve_many: lmbd_stride is 0 (one shared price vector) or at least 3N");
  if (flags & ~LOMPC_MANY_WARM) return fail_arg(c, "solve_many: unknown flag");
  if ((flags & LOMPC_MANY_WARM) && !ws) return fail_arg(c, "solve_many: LOMPC_MANY_WARM needs ws");
  if (err && !w_ref) return fail_arg(c, "solve_many: err needs w_ref");
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  if (counts) HIPCHK(c, hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st));
  ManyArgs a{};
  a.K = K;
  a.lmbd_stride = lmbd_stride;
  a.lmbd = lmbd;
  a.lmbd_r = lmbd_r;
  a.gamma = gamma;
  a.w_ref = w_ref;
  a.ws = ws;
  a.w = w;
  a.cost = cost;
  a.w0 = w0;
  a.price0 = price0;
  a.err = err;
  a.status = status;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  for (int64_t j0 = 0; j0 < K; j0 += MANY_CHUNK) {
    a.j0 = j0;
    const int64_t n = std::min<int64_t>(MANY_CHUNK, K - j0);
    const dim3 grid((unsigned)((n + MANY_WAVES - 1) / MANY_WAVES)), block(64 * MANY_WAVES);
    if (flags & LOMPC_MANY_WARM)
      hipLaunchKernelGGL(k_many<true>, grid, block, 0, st, c->q, a);
    else
      hipLaunchKernelGGL(k_many<false>, grid, block, 0, st, c->q, a);
    HIPCHK(c, hipGetLastError());
  }
  if (counts && K > 0) {
    hipLaunchKernelGGL(k_many_close, dim3(1), dim3(1), 0, st, a.counts, K);
    HIPCHK(c, hipGetLastError());
  }
  return LOMPC_OK;
}
