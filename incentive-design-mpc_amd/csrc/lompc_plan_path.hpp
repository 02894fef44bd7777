// lompc_plan_path.hpp — the plan's path side: the write-through stores, the LDS index helpers, the sets'
// constants, the gamma-window kernels (k_plan_window, k_plan_window_sorted), PathArgs, path_cell and k_path.
// Plain text of lompc_plan.hip, included by it alone, inside its kernel namespace and before
// lompc_plan_eval.hpp; the order of the declarations is the order the kernels were generated in.

typedef unsigned int lq_v4u __attribute__((ext_vector_type(4)));
typedef unsigned int lq_v2u __attribute__((ext_vector_type(2)));

// write-through (sc1) stores: the outputs leave no dirty lines in the XCD's L2, so the kernel
// boundary behind k_eval has no L2 writeback to wait for (MI355X_MICROARCH.md, price list)
#ifndef LQ_ROW_AUX
#define LQ_ROW_AUX 16  // the row stores' cache policy bits (16: sc1, write-through); diagnostic builds vary it
#endif
__device__ __forceinline__ void st_wt16(__amdgpu_buffer_rsrc_t rs, int off, double x, double y) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(lq_v4u, make_double2(x, y)), rs, off, 0, LQ_ROW_AUX);
}
__device__ __forceinline__ void st_wt8b(__amdgpu_buffer_rsrc_t rs, int off, double x) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(lq_v2u, x), rs, off, 0, LQ_ROW_AUX);
}
__device__ __forceinline__ void st_wt8(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per-EV scalar outputs (cost, w0): 8-B write-through stores are one fabric write each (2.7x the
// per-byte time of 16-B ones, MI355X_MICROARCH.md); EV_PLAIN (diagnostic builds) stores them plain
#ifndef LQ_EV_PLAIN
#define LQ_EV_PLAIN 0
#endif
__device__ __forceinline__ void st_ev8(double* p, double v) {
  if (LQ_EV_PLAIN) *p = v;
  else st_wt8(p, v);
}

__device__ __forceinline__ void st_wt4(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_eval: double2 per LDS piece row (padding shifts consecutive rows across the banks)
__host__ __device__ constexpr int eval_row_stride(int N) { return N + 1; }
// k_eval: LDS double of coefficient j of piece k; the record's four 16-B quarters are permuted
// by bits 2..3 of k, so lanes reading quarter q of different pieces spread over all 64 banks
// (records are 64 B: unswizzled, quarter q of every piece falls on one of 4 bank slots)
__device__ __forceinline__ int cfx(const int k, const int j) {
  return k * 8 + ((((j >> 1) ^ (k >> 2)) & 3) << 1) + (j & 1);
}
static_assert((LQ_PPL & (LQ_PPL - 1)) == 0, "k_eval's piece-end transpose needs a power-of-two LQ_PPL");

__device__ __forceinline__ double clampw(double x, double wmax) { return fmin(fmax(x, 0.0), wmax); }

// ---------------------------------------------------------------- plan kernel
// the constants of set s's EV type: the context index from the kernel arguments and wave-uniform,
// so every field is a scalar (constant-cache) load instead of a vector load with a full memory
// round trip
// (the table is read-only for the whole launch: the constant address space lets the compiler use
// scalar loads although the kernels store to other global memory)
typedef const __attribute__((address_space(4))) QPConst QPConstK;
__device__ __forceinline__ const QPConst& set_consts(const QPConst* qd, const CtxEnds& ce, int s) {
  s = __builtin_amdgcn_readfirstlane(s);
  int k = 0;
#pragma unroll
  for (int j = 0; j + 1 < LQ_PLAN_MAX_CTX; ++j) k += s >= ce.end[j] ? 1 : 0;
  QPConstK* p = (QPConstK*)(uintptr_t)qd + k;
  return *(const QPConst*)p;
}

struct WindowArgs {
  const QPConst* qd;
  CtxEnds ce;
  const int4* blk;         // k_eval's block map: (set, begin, end)
  const int* blk_prefix;   // [S+1] first block of each set
  const double* gamma;
  unsigned long long* acc; // [S][3], zero on entry and on exit
  double* window;
  int S, nblk;
};

// per set: [lo, hi] = range of its valid gamma, widened by 1e-7 y_max (a zero-width set still
// gets cells of positive width), clipped to [0, y_max]; no valid EV -> [0, y_max].
// One workgroup per k_eval block (>= one per CU): a block folds its EVs, then merges into its
// set's accumulators with integer atomics (the bits of a non-negative double order like the
// double, so min/max are exact and the result does not depend on the order); the set's last
// block writes the window and zeroes the accumulators for the next launch.  One extra workgroup
// (the last) writes the windows of the empty sets, which have no blocks.
// the window from the set's smallest / largest valid gamma (any: there is one)
__device__ __forceinline__ void window_store(double* window, int s, double ym, bool any, double lo, double hi) {
  const double mg = 1e-7 * ym;
  double wlo = 0.0, whi = ym;
  if (any) {
    wlo = fmin(fmax(lo - mg, 0.0), ym);
    whi = fmin(fmax(hi + mg, wlo + mg), ym);
    if (!(whi > wlo)) wlo = fmax(whi - 2.0 * mg, 0.0);
  }
  window[2 * s] = wlo;
  window[2 * s + 1] = whi;
}

__global__ __launch_bounds__(256) void k_plan_window(WindowArgs a) {
  __shared__ double smin[4], smax[4];
  __shared__ int last;
  if ((int)blockIdx.x == a.nblk) {
    for (int s = threadIdx.x; s < a.S; s += 256)
      if (a.blk_prefix[s + 1] == a.blk_prefix[s]) {
        int k = 0;  // (s differs per lane: no scalar set_consts)
        for (int j = 0; j + 1 < LQ_PLAN_MAX_CTX; ++j) k += s >= a.ce.end[j] ? 1 : 0;
        a.window[2 * s] = 0.0;
        a.window[2 * s + 1] = a.qd[k].y_max;
      }
    return;
  }
  const int4 bk = a.blk[blockIdx.x];
  const int s = bk.x;
  const double ym = set_consts(a.qd, a.ce, s).y_max;
  double lo = INFINITY, hi = -INFINITY;
  for (int i = bk.y + (int)threadIdx.x; i < bk.z; i += 256) {
    const double g = a.gamma[i];
    if (g >= 0.0 && g <= ym) {
      lo = fmin(lo, g);
      hi = fmax(hi, g);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o));
    hi = fmax(hi, __shfl_xor(hi, o));
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smin[wv] = lo;
    smax[wv] = hi;
  }
  __syncthreads();
  unsigned long long* acc = a.acc + 3 * s;
  if (threadIdx.x == 0) {
    lo = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
    hi = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    if (lo <= hi) {  // + 0.0: -0.0 -> +0.0, whose bits order with the positive doubles
      atomicMax(&acc[0], ~(unsigned long long)__double_as_longlong(lo + 0.0));
      atomicMax(&acc[1], (unsigned long long)__double_as_longlong(hi + 0.0));
    }
    __threadfence();
    const unsigned long long nb = (unsigned long long)(a.blk_prefix[s + 1] - a.blk_prefix[s]);
    last = atomicAdd(&acc[2], 1ull) == nb - 1;
  }
  __syncthreads();
  if (!last || threadIdx.x != 0) return;
  __threadfence();
  const unsigned long long blo = atomicExch(&acc[0], 0ull), bhi = atomicExch(&acc[1], 0ull);
  atomicExch(&acc[2], 0ull);
  window_store(a.window, s, ym, blo != 0, __longlong_as_double((long long)~blo), __longlong_as_double((long long)bhi));
}

// gamma-sorted plans (LOMPC_PLAN_SORTED_GAMMA): one wave per set.  An ascending set whose first and
// last gamma are valid has its valid range at its ends — the same window as k_plan_window's in one
// load round instead of a pass over the set and one atomic per block (a set whose ends are not both
// valid is folded by the wave, as k_plan_window does; an unsorted set is reported failed by k_agg).
__global__ __launch_bounds__(64) void k_plan_window_sorted(WindowArgs a, const int64_t* __restrict__ set_off) {
  const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
  const double ym = set_consts(a.qd, a.ce, s).y_max;
  const int64_t s0 = set_off[s], s1 = set_off[s + 1];
  if (s1 == s0) {
    if (lane == 0) window_store(a.window, s, ym, false, 0.0, 0.0);
    return;
  }
  const double g0 = a.gamma[s0], g1 = a.gamma[s1 - 1];
  const bool v0 = g0 >= 0.0 && g0 <= ym, v1 = g1 >= 0.0 && g1 <= ym;
  double lo = g0, hi = g1;
  if (!(v0 && v1)) {
    lo = INFINITY;
    hi = -INFINITY;
    for (int64_t i = s0 + lane; i < s1; i += 64) {
      const double g = a.gamma[i];
      if (g >= 0.0 && g <= ym) {
        lo = fmin(lo, g);
        hi = fmax(hi, g);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fmin(lo, __shfl_xor(lo, o));
      hi = fmax(hi, __shfl_xor(hi, o));
    }
  }
  if (lane == 0) window_store(a.window, s, ym, lo <= hi, lo + 0.0, hi + 0.0);
}

// cell of a valid gamma in a set's window (k_eval), the same arithmetic as k_path's cell bounds
__device__ __forceinline__ int cell_of(double g, double lo, double inv_h, int G) {
  const double x = (g - lo) * inv_h;
  return x <= 0.0 ? 0 : (x >= (double)(G - 1) ? G - 1 : (int)x);
}

// ---------------------------------------------------------------- k_path
struct PathArgs {
  int S, G, N, flags;
  const QPConst* qd;
  CtxEnds ce;
  const double* window;
  const double* lmbd;    // [S][3N]
  const double* lmbd_r;  // [S]
  const double* w_ref;   // [S][N] or null
  uint8_t* ws;           // [S*G][64] warm-start working sets or null
  // per cell
  int* t_cnt;            // [S*G]             certified pieces of the cell (0: none)
  double* t_lo;          // [S*G]             coverage start
  uint8_t* t_sl;         // [S*G][64]         working set at the cell start (repairs)
  // per cell LQ_PPL piece slots, the first t_cnt used (ascending gamma)
  double* t_ge;          // [S][G*PPL]        gamma at each piece's end
  double* t_cf;          // [S][G*PPL][8]     K0 K1 K2 (cost) F0 F1 F2 (err^2) a_0 b_0
  double2* t_ab;         // [S][G*PPL][N]     (a_t, b_t)
  int* errflag;
  const int* skip;       // device-resident price loop: nonzero = the loop has finished, run nothing
};

// price loads: plain, or (COH) device-coherent sc1 loads past this CU's L1 — the persistent price
// loop (k_loop_run) re-reads prices that another workgroup of the same launch wrote through (sc1)
template <bool COH>
__device__ __forceinline__ double ld_price(const double* p) {
  if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}

// per-stage data of set s from its prices (lompc.py:92-135 in standard form)
// (bad: a negative or NaN price on this lane's stage)
template <bool COH = false>
__device__ __forceinline__ void load_set(const QPConst& q, const double* __restrict__ L, double lr, int N,
                                         int lane, lqw::WaveSet& ws, double& l2, bool& bad) {
  const double tt = q.theta * q.theta;
  ws.N = N;
  ws.lane = lane;
  l2 = 0.0;
  bad = false;
  if (lane < N) {
    const double l1 = ld_price<COH>(L + lane), l3 = ld_price<COH>(L + 2 * N + lane);
    l2 = ld_price<COH>(L + N + lane);
    bad = !(l1 >= 0.0 && l2 >= 0.0 && l3 >= 0.0);
    ws.d_nat = 2.0 * lr * tt + 2.0 * q.q_scale * l3 + q.dsmall;
    ws.e_nat = q.theta * (l1 - l2);
  } else {
    ws.d_nat = ws.e_nat = 0.0;
  }
}

// load_set with the set's prices already in registers (lane t < N: prices t, N + t, 2N + t)
__device__ __forceinline__ void load_set_regs(const QPConst& q, double l1, double l2v, double l3, double lr, int N,
                                              int lane, lqw::WaveSet& ws, double& l2, bool& bad) {
  const double tt = q.theta * q.theta;
  ws.N = N;
  ws.lane = lane;
  l2 = 0.0;
  bad = false;
  if (lane < N) {
    l2 = l2v;
    bad = !(l1 >= 0.0 && l2 >= 0.0 && l3 >= 0.0);
    ws.d_nat = 2.0 * lr * tt + 2.0 * q.q_scale * l3 + q.dsmall;
    ws.e_nat = q.theta * (l1 - l2);
  } else {
    ws.d_nat = ws.e_nat = 0.0;
  }
}

// One (set, gamma cell) path by one wave (blk = s * G + cell); the wave's workgroup has
// initialised the box table for the set's constants (lq_tab_init).  Every piece goes straight
// to the cell's fixed slots with write-through stores (visible to any XCD once they complete).
// NT: the horizon as a compile-time constant (0: a.N at run time) — the scans' row / bank steps
// become straight-line code, so independent chains can be interleaved
template <int NT = 0, bool INIT_TAB = false, bool COH = false, bool PREG = false>
__device__ __forceinline__ void path_cell(const PathArgs& a, const int blk, double p1 = 0.0, double p2 = 0.0,
                                          double p3 = 0.0, double wr_in = 0.0, int* ws_io = nullptr) {
  // (PREG: the set's prices p1..p3, the lane's w_ref wr_in and the cell's stored working set *ws_io
  // in registers — k_loop_run2's later calls; the working set still stored for the next loop)
  const int G = a.G;
  const int s = __builtin_amdgcn_readfirstlane(blk / G);
  const int cell = blk - s * G;
  const int lane = (int)threadIdx.x & 63;
  const int N = NT ? NT : a.N;
  const double* __restrict__ L = a.lmbd + (size_t)s * 3 * N;
  const double lr = a.lmbd_r[s];
  const double wr_nat = PREG ? wr_in : (a.w_ref && lane < N) ? a.w_ref[(size_t)s * N + lane] : 0.0;
  const double wlo = a.window[2 * s], whi = a.window[2 * s + 1];
  const QPConst& q = set_consts(a.qd, a.ce, s);  // scalar loads, no register copy
  LQ_STAMP(0);
  lqw::WaveSet ws;
  double l2;
  bool bad;
  if constexpr (PREG) load_set_regs(q, p1, p2, p3, lr, N, lane, ws, l2, bad);
  else load_set<COH>(q, L, lr, N, lane, ws, l2, bad);
  if (INIT_TAB) lq_tab_init(q);  // (after the price loads are issued: the barrier overlaps them)
  if (bad || (lane == 0 && !(lr >= 0.0))) atomicOr(a.errflag, 1);
  const double c0 = q.theta * q.w_max * lqw::wave_sum(l2, N);  // lompc.py:128
  const double kappa = lr / q.delta;                            // price_solver.py:191
  double Ywr;
  {
    lqw::Sums<1> y;
    y.v[0] = wr_nat;
    Ywr = lqw::wave_scan(y, N).v[0];
  }
  const double h = (whi - wlo) / (double)G;
  const double mg = 1e-13 * q.y_max;  // cells overlap by a rounding margin
  const double glo = fmax((cell == 0 ? wlo : fma((double)cell, h, wlo)) - mg, 0.0);
  const double ghi = fmin((cell == G - 1 ? whi : fma((double)(cell + 1), h, wlo)) + mg, q.y_max);
  LQ_STAMP(1);
  int npc = 0;
  int sl0 = lane < N ? 1 : 0;
  if (!(a.flags & LOMPC_PLAN_DIAG_REPAIR)) {
    int sl = sl0;
    bool warm = false;
    if (a.ws) {
      const int v = (PREG && ws_io) ? *ws_io : a.ws[(size_t)blk * 64 + lane];
      sl = (lane < N && v >= 0 && v <= 2 * q.m) ? v : sl0;
      warm = LQ_WARM_FP64 && __all(lane >= N || v <= 2 * q.m);  // (a stored set on every stage: wave-uniform)
    }
    lqw::StageSol<2> sol;
    bool has_sol = false;
#ifdef LOMPC_STAMPS
    int nit = 0;
    const bool solved = lqw::wave_solve_path(q, ws, glo, sl, sol, has_sol, &nit, warm);
    if (lane == 0 && blk < 32768) g_stamps[blk * 8 + 4] = nit;
#else
    const bool solved = lqw::wave_solve_path(q, ws, glo, sl, sol, has_sol, nullptr, warm);
#endif
    LQ_STAMP(2);
    if (solved) {
      sl0 = sl;
      if (a.ws) a.ws[(size_t)blk * 64 + lane] = (uint8_t)sl;
      if (ws_io) *ws_io = (int)(uint8_t)sl;
      const size_t sb = (size_t)blk * LQ_PPL;  // the cell's fixed piece slots
      // ---- parametric active-set tracking of w*(gamma) on [glo, ghi]
      double gcur = glo;
      int last = -1;
      const int max_iter = 4 * LQ_PPL + 16;
      const double ee = ws.e_nat;
      if (!has_sol) sol = lqw::solve_stage<2>(q, ws, 0.0, sl);  // (else the start's solve is reused)
      Box bxn = lq_box(lane < N ? sl : 0);  // the working set's boxes (carried: read with its solve)
      for (int it = 0; it < max_iter && npc < LQ_PPL; ++it) {
#ifdef LOMPC_STAMPS
        if (lane == 0 && blk < 32768) g_stamps[blk * 8 + 5] = it + 1;
#endif
        const double av = sol.w[0], bv = sol.w[1], r0 = sol.r[0], r1 = sol.r[1];
        double gc = INFINITY;
        int ns = sl;
        const bool act = lane < N;
        const Box bx = bxn;
        if (act) {
          if (sl & 1) {  // free: w(gamma) = a + b gamma leaves [lo, hi]
            if (bv > 0.0) { gc = (bx.hi - av) / bv; ns = sl + 1; }
            else if (bv < 0.0) { gc = (bx.lo - av) / bv; ns = sl - 1; }
          } else {       // fixed: v(gamma) = -r0 - r1 gamma leaves [slo, shi]
            if (r1 < 0.0) { gc = -(bx.shi + r0) / r1; ns = sl + 1; }
            else if (r1 > 0.0) { gc = -(bx.slo + r0) / r1; ns = sl - 1; }
          }
          if (!(gc == gc)) gc = INFINITY;  // NaN guard
          if (lane == last && gc <= gcur) gc = INFINITY;
          gc = fmax(gc, gcur);
        }
        double best = gc;
        int bj = lane;
        lqw::wave_argmin(best, bj, N);
        if (!(best < ghi)) {
          best = ghi;
          bj = -1;
        }
        const bool final_piece = (bj < 0) || (npc == LQ_PPL - 1);
        const bool emit = best > gcur || final_piece;  // (wave-uniform)
        // The next working set (the switch at the breakpoint) and its sub-problem solve do not
        // depend on this piece's certificate and quadratics: all of them in one basic block, so
        // the scheduler interleaves the independent DPP-scan chains (the next solve is wasted
        // work, not latency, when this piece is the last).
        const int bns = lqw::readlane_i(ns, bj < 0 ? 0 : bj);  // (bj wave-uniform: from a ballot)
        const int sln = lane == bj ? bns : sl;
        lqw::StageSol<2> nsol;
        double res;
        double t[6];
        auto piece = [&]() {
          // KKT certificate at the piece's end; its start is the previous certified end (same w
          // and r, only the switched coordinate's box changed and it contains the value)
          // (the gradient from the prefix sums of a and b, which the cost quadratics need anyway:
          // y = Ya + gamma Yb, Z = sum_{i<=t} y_i = Za + gamma Zb — two 2-value scans instead of
          // wave_kkt_point's two affine scans over w; the same point up to rounding)
          const double wz = fmin(fmax(fma(bv, best, av), bx.lo), bx.hi);
          lqw::Sums<2> pf;
          pf.v[0] = act ? av : 0.0;
          pf.v[1] = act ? bv : 0.0;
          pf = lqw::wave_scan(pf, N);
          const double Ya = pf.v[0], Yb = pf.v[1];
          {
            lqw::Sums<2> zf;
            zf.v[0] = act ? Ya : 0.0;
            zf.v[1] = act ? Yb : 0.0;
            zf = lqw::wave_scan(zf, N);
            const double y = fma(best, Yb, Ya), Z = fma(best, zf.v[1], zf.v[0]);
            const double Zt = lqw::readlane_d(Z, N - 1);
            const double rr = q.c * (Zt - Z + y - (double)(N - lane) * best) + ws.d_nat * wz + ws.e_nat;
            res = lqw::wave_max(act ? lq_resid(q, bx, wz, rr) : 0.0, N);
          }
          const double Ea = Ya - Ywr, da = av - wr_nat;
          const double dd = ws.d_nat, cc = q.c;
          const double sg = (sl & 1) ? bx.slo : 0.0;  // PWL slope of a free coordinate
          const double wmid = fma(bv, 0.5 * (gcur + best), av);
          const double tw = q.theta * q.w_max;
          // PWL value at w = 0 of its linear piece (large EVs; small EVs have no PWL term)
          const double icpt = q.ev_small ? 0.0 : fma(-sg, wmid, tw * tw * lq_pwl(wmid * q.inv_wmax));
          t[0] = fma(0.5 * cc, Ya * Ya, fma(av, fma(0.5 * dd, av, ee + sg), icpt));
          t[1] = fma(cc, fma(Ya, Yb, -Ya), bv * fma(dd, av, ee + sg));
          t[2] = fma(0.5 * cc, Yb * Yb, fma(-cc, Yb, 0.5 * dd * bv * bv));
          t[3] = fma(Ea, Ea, kappa * da * da);
          t[4] = 2.0 * fma(Ea, Yb, kappa * da * bv);
          t[5] = fma(Yb, Yb, kappa * bv * bv);
#pragma unroll
          for (int k = 0; k < 6; ++k) t[k] = act ? t[k] : 0.0;
          lqw::wave_totals(t, N);
        };
        if (bj >= 0) {  // (wave-uniform) the next solve beside this piece's certificate
          bxn = lq_box(act ? sln : 0);
          nsol = lqw::solve_stage<2>(q, ws, bxn, 0.0, sln);
          piece();
        } else {
          piece();
        }
        if (emit) {
          if (!(res <= q.tol_cert)) break;  // coverage ends at gcur
          if (lane < N) {
            double* dst = reinterpret_cast<double*>(a.t_ab + (sb + npc) * N + lane);
            st_wt8(dst, av);
            st_wt8(dst + 1, bv);
          }
          const double a0 = lqw::readlane_d(av, 0), b0v = lqw::readlane_d(bv, 0);
          if (lane < 8) {
            double v = t[0] + c0;
#pragma unroll
            for (int k = 1; k < 6; ++k) v = lane == k ? t[k] : v;
            v = lane == 6 ? a0 : (lane == 7 ? b0v : v);
            st_wt8(a.t_cf + (sb + npc) * 8 + lane, v);
          }
          if (lane == 0) st_wt8(a.t_ge + sb + npc, best);
          ++npc;
        }
        if (bj < 0) break;
        sl = sln;
        sol = nsol;
        gcur = best;
        last = bj;
      }
    }
  }
  a.t_sl[(size_t)blk * 64 + lane] = (uint8_t)sl0;
  if (lane == 0) {
    __hip_atomic_store(a.t_cnt + blk, npc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    st_wt8(a.t_lo + blk, glo);
  }
  LQ_STAMP(3);
#ifdef LOMPC_STAMPS
  if (lane == 0 && blk < 65536) g_stamps[blk * 8 + 6] = npc;
#endif
}

template <int NT>
__global__ __launch_bounds__(64) void k_path(PathArgs a) {
  if (a.skip && *a.skip) return;
  path_cell<NT, true>(a, (int)blockIdx.x);
}

// forward (defined with k_finalize below)
struct FinalArgs;
template <int NT>
__global__ __launch_bounds__(64) void k_path_fin(PathArgs a, FinalArgs r);

typedef void (*PathKernel)(PathArgs);
typedef void (*PathKernel2)(PathArgs, FinalArgs);
PathKernel path_kernel(int N) {
  switch (N) {
    case 12: return k_path<12>;
    case 16: return k_path<16>;
    case 24: return k_path<24>;
    case 48: return k_path<48>;
    default: return k_path<0>;
  }
}
