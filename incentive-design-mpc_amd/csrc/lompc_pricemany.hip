// lompc_pricemany.hip — lompc_price_step_many: the price-gradient step of PriceSolver
// (price_solver.py:216-246) for K unrelated QPs, each with its own w, w_ref, prices and lmbd_r, in
// one launch, with the loop's convergence test (price_solver.py:125) fused in front of it.
//
// The other half of a per-EV (personalised) price iteration beside lompc_solve_many: the host-driven
// loop is {k_many, k_price_steps} per iteration, nothing crosses the bus but the 32-byte tally.
//
//   k_price_steps        one 64-lane wave per QP (lane t = stage t), STEPS_WAVES waves per workgroup:
//                        the step of loop_step_core (lompc_loopstep.hpp) — PriceQPW::init with the QP's
//                        own kappa, q = -Q lmbd - (phi(w) - phi(w_ref)), nnqp_wave from lmbd's free
//                        set, the decrease from the certificate's multipliers.  No LDS, no barrier;
//                        coalesced row stores, lane-0 stores of the scalars.
//   k_price_steps_close  one thread: counts[RUNNING] = K - (converged + failed + invalid).
//
// The call keeps no state: the A_bar factor is computed per QP and nothing is read from or written
// to the context beyond its constants.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lompc_ctx.hpp"
#include "lompc_pricewave.hpp"

#define STEPS_WAVES 4                 // waves (QPs) per workgroup
#define STEPS_CHUNK (1ll << 24)       // QPs per launch (grid x block stays below 2^32 threads)

struct StepsArgs {
  int64_t K;            // QPs of the whole call
  int64_t j0;           // first QP of this launch
  int64_t lmbd_stride;  // doubles between price vectors read (>= r)
  int64_t next_stride;  // doubles between price vectors written (>= 3N)
  int N, r;
  double theta, w_max, m, delta, eps_reg, tol;
  const double* w;
  const double* w_ref;
  const double* lmbd;
  const double* lmbd_r;  // or null (= 0)
  const double* err;     // or null (no convergence test)
  double* lmbd_next;
  double* dec;           // or null
  int8_t* state;         // or null (every QP running)
  int32_t* iters;        // or null
  unsigned long long* counts;  // [4] or null
};

__global__ __launch_bounds__(64 * STEPS_WAVES) void k_price_steps(StepsArgs a) {
  const int lane = threadIdx.x & 63;
  const int N = a.N, nb = a.r / N;
  const int64_t j = a.j0 + (int64_t)blockIdx.x * STEPS_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (j >= a.K) return;  // (wave-uniform)
  const bool act = lane < N;
  // the whole row before any store: lmbd_next may be lmbd (in place)
  const double* L = a.lmbd + j * a.lmbd_stride;
  double lm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) lm[k] = (act && k < nb) ? L[k * N + lane] : 0.0;
  double* X = a.lmbd_next + j * a.next_stride;
  const int st_in = a.state ? (int)a.state[j] : LOMPC_STEP_RUNNING;
  if (st_in != LOMPC_STEP_RUNNING) {  // frozen: the prices as they are, nothing else moves
    if (act) {
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k * N + lane] = lm[k];
    }
    if (lane == 0) {
      if (a.dec) a.dec[j] = 0.0;
      if (a.counts)
        atomicAdd(a.counts + ((st_in >= LOMPC_STEP_CONVERGED && st_in <= LOMPC_STEP_INVALID) ? st_in : LOMPC_STEP_INVALID),
                  1ull);
    }
    return;
  }
  const double wk = act ? a.w[j * N + lane] : 0.0;
  const double wr = act ? a.w_ref[j * N + lane] : 0.0;
  const double lr = a.lmbd_r ? a.lmbd_r[j] : 0.0;
  const double e = a.err ? a.err[j] : 0.0;
  bool bad = !(wk == wk) || !(wr == wr);
#pragma unroll
  for (int k = 0; k < 3; ++k) bad = bad || !(lm[k] >= 0.0);
  const bool valid = !__any(bad) && (lr >= 0.0) && (e == e);
  int st = LOMPC_STEP_RUNNING;
  double x[3] = {lm[0], lm[1], lm[2]};
  double dec = 0.0;
  if (!valid) {
    st = LOMPC_STEP_INVALID;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = k < nb ? NAN : 0.0;
    dec = NAN;
  } else if (a.err && e <= a.tol) {  // price_solver.py:125
    st = LOMPC_STEP_CONVERGED;
  } else {
    // the price-gradient step at (w, lmbd): loop_step_core's, with the factor of this QP's A_bar
    lqp::PriceQPW P;
    P.init(N, a.r, a.theta, a.w_max, a.m, lr / a.delta, a.eps_reg, wk);
    const double q_s = 3.0 * a.theta / (4.0 * a.w_max);
    double Ql[3], q[3];
    P.mulQ(lm, Ql);
    const double dw = wk - wr;
    const double dphi[3] = {a.theta * dw, -a.theta * dw, q_s * (wk * wk - wr * wr)};
    double qmax = 0.0, dual = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      q[k] = P.has(k) ? -Ql[k] - dphi[k] : 0.0;
      qmax = fmax(qmax, fabs(q[k]));
      dual += P.has(k) ? lm[k] * fma(0.5, Ql[k], q[k]) : 0.0;
    }
    qmax = lqw::wave_max(qmax, 64);
    dual = lqw::wave_sum(dual, 64);
    double z[3] = {0.0, 0.0, 0.0}, mu[3];
    if (lqp::nnqp_wave(P, q, lm, z, 1e-11 * (1.0 + qmax), mu)) {
      double cn = 0.0;  // 1/2 x'Qx + q'x with Qx = mu - q from the certificate
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        cn += P.has(k) ? z[k] * fma(0.5, mu[k] - q[k], q[k]) : 0.0;
        x[k] = P.has(k) ? z[k] : 0.0;
      }
      dec = dual - lqw::wave_sum(cn, 64);
    } else {  // no certified point: the prices stay
      st = LOMPC_STEP_FAILED;
      dec = NAN;
    }
  }
  if (act) {
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k * N + lane] = x[k];
  }
  if (lane == 0) {
    if (a.dec) a.dec[j] = dec;
    if (st == LOMPC_STEP_RUNNING) {
      if (a.iters) a.iters[j] += 1;
    } else {
      if (a.state) a.state[j] = (int8_t)st;
      if (a.counts) atomicAdd(a.counts + st, 1ull);
    }
  }
}

__global__ void k_price_steps_close(unsigned long long* counts, int64_t K) {
  counts[LOMPC_STEP_RUNNING] = (unsigned long long)K - counts[LOMPC_STEP_CONVERGED] - counts[LOMPC_STEP_FAILED] -
                               counts[LOMPC_STEP_INVALID];
}

extern "C" int lompc_price_step_many(lompc_ctx* c, int64_t K, int r, double eps_reg, const double* w,
                                     const double* w_ref, const double* lmbd, int64_t lmbd_stride,
                                     const double* lmbd_r, const double* err, double tol, double* lmbd_next,
                                     int64_t next_stride, double* dec, int8_t* state, int32_t* iters,
                                     int64_t* counts, void* stream) {
  if (!c) return LOMPC_ERR_INVALID_ARG;
  const int N = c->N;
  if (K < 0) return fail_arg(c, "price_step_many: K >= 0 required");
  if (!w || !w_ref || !lmbd || !lmbd_next) return fail_arg(c, "price_step_many: w, w_ref, lmbd and lmbd_next required");
  if (r != 2 * N && r != 3 * N) return fail_arg(c, "price_step_many: r is 2N or 3N");
  if (!(eps_reg > 0.0)) return fail_arg(c, "price_step_many: eps_reg > 0 required");
  if (lmbd_stride < r) return fail_arg(c, "price_step_many: lmbd_stride is at least r");
  if (next_stride < 3 * (int64_t)N) return fail_arg(c, "price_step_many: next_stride is at least 3N");
  if (K > 0 && !(lmbd_next == lmbd && next_stride == lmbd_stride)) {  // in place, or fully disjoint
    const double* le = lmbd + (K - 1) * lmbd_stride + r;
    const double* ne = lmbd_next + (K - 1) * next_stride + 3 * (int64_t)N;
    if (lmbd_next < le && lmbd < ne)
      return fail_arg(c, "price_step_many: lmbd_next overlaps lmbd (allowed: exactly in place, or disjoint)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
  if (counts) HIPCHK(c, hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st));
  StepsArgs a{};
  a.K = K;
  a.lmbd_stride = lmbd_stride;
  a.next_stride = next_stride;
  a.N = N;
  a.r = r;
  a.theta = c->q.theta;
  a.w_max = c->q.w_max;
  a.m = c->q.c;  // 2 delta theta^2, lompc.py:71
  a.delta = c->q.delta;
  a.eps_reg = eps_reg;
  a.tol = tol;
  a.w = w;
  a.w_ref = w_ref;
  a.lmbd = lmbd;
  a.lmbd_r = lmbd_r;
  a.err = err;
  a.lmbd_next = lmbd_next;
  a.dec = dec;
  a.state = state;
  a.iters = iters;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  for (int64_t j0 = 0; j0 < K; j0 += STEPS_CHUNK) {
    a.j0 = j0;
    const int64_t n = std::min<int64_t>(STEPS_CHUNK, K - j0);
    const dim3 grid((unsigned)((n + STEPS_WAVES - 1) / STEPS_WAVES)), block(64 * STEPS_WAVES);
    hipLaunchKernelGGL(k_price_steps, grid, block, 0, st, a);
    HIPCHK(c, hipGetLastError());
  }
  if (counts && K > 0) {
    hipLaunchKernelGGL(k_price_steps_close, dim3(1), dim3(1), 0, st, a.counts, K);
    HIPCHK(c, hipGetLastError());
  }
  return LOMPC_OK;
}
