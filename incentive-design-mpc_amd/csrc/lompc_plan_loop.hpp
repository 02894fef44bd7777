// lompc_plan_loop.hpp — the device-resident price loop's kernels: k_loop_iter (one launch per iteration),
// the persistent k_loop_run, k_loop_run2 and k_loop_runs (LoopJob), the LQ_LSTAMP stamps and the dispatchers.
// Plain text of lompc_plan.hip, included by it alone, inside its kernel namespace after lompc_agg.hpp (the
// loop kernels call its aggregation) and lompc_scalar.hpp.

// ---------------------------------------------------------------- k_loop_iter
// One iteration of the device-resident price loop over gamma-sorted sets (lompc_loop.hip) in ONE
// launch, one wave per (set, cell) as k_path: the wave tracks its cell's path (path_cell), then
// aggregates the same cell from the tables it has just written (agg_cell, coherent loads) into a
// cell record (write-through).  The last of the S * G cells to arrive closes both sets from their
// records in cell order (agg_finish: k_agg's arithmetic — the same bits for G <= LQ_AGG_W, where
// k_agg's wave c holds cell c; G <= LQ_LOOP_G) and runs the loop step (lompc_loopstep.hpp) on the
// closed outputs in its registers.  The unfused form's three launches (k_path, k_agg, k_loop_step) and two kernel
// boundaries become one launch and one arrival counter (ctl[1]).
constexpr int LQ_LOOP_G = 16;  // k_loop_iter: at most this many cells per set (its closing's records in registers)
constexpr int LQ_LOOP_G2 = 32;  // k_loop_run2: at most this many (its closing reads the records 16 at a time)

#ifdef LOMPC_STAMPS
// diagnostic build: per k_loop_iter wave (blk < 64) the phases' s_memrealtime ticks summed over the
// launches: [0] path, [1] aggregation, [2] record + arrival, [3] both sets' closing, [4] loop step,
// [5] launches, [6] closings, [7] steps; sub-phases of [3] and [4]: [10] the records' load round,
// [8] the step's inputs and error metric, [9] the price QP (scripts/loop_stamps.py)
#define LQ_LSTAMP(k)                                                                                 \
  do {                                                                                               \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                 \
    const long long t__ = __builtin_amdgcn_s_memrealtime();                                          \
    if (lane == 0 && blk < 64) {                                                                     \
      __hip_atomic_fetch_add(g_lstamps + blk * 16 + (k), (unsigned long long)(t__ - tl__), __ATOMIC_RELAXED, \
                             __HIP_MEMORY_SCOPE_AGENT);                                              \
      if ((k) == 0 || (k) == 3 || (k) == 4)                                                          \
        __hip_atomic_fetch_add(g_lstamps + blk * 16 + 5 + ((k) >= 3 ? (k) - 2 : 0), 1ull, __ATOMIC_RELAXED, \
                               __HIP_MEMORY_SCOPE_AGENT);                                            \
    }                                                                                                \
    tl__ = t__;                                                                                      \
  } while (0)
#else
#define LQ_LSTAMP(k)
#endif

template <int NT>
__global__ __launch_bounds__(64) void k_loop_iter(PathArgs pa, AggArgs ga, StepArgs sa, double* rec, int m) {
  constexpr int S = 2;  // (lq_loop_fusable: the loop's two sets)
  if (sa.ctl[0]) return;  // finished: a call enqueued ahead of the convergence (every workgroup)
  const int blk = (int)blockIdx.x, lane = (int)threadIdx.x, G = pa.G;
  const int s = blk / G, c = blk - s * G;
#ifdef LOMPC_STAMPS
  long long tl__ = __builtin_amdgcn_s_memrealtime();
#endif
  StepIn in;
  step_prices(sa, lane, in);  // (every wave: the one that runs the step has them when it arrives last)
  // the sets' sizes and order flags for the closing, loaded now (scalar loads are otherwise issued
  // at their first use: a memory round on the closing's critical path)
  int cl_n[S], cl_v[S], cl_ok[S];
#pragma unroll
  for (int t = 0; t < S; ++t) {
    const int4 si = ga.sinfo[t];
    cl_n[t] = (int)(ga.set_off[t + 1] - ga.set_off[t]);
    cl_v[t] = si.x;
    cl_ok[t] = si.y;
    asm volatile("" : "+v"(cl_n[t]), "+v"(cl_v[t]), "+v"(cl_ok[t]));  // (held in VGPRs: SGPRs are scarce here)
  }
  path_cell<NT, true>(pa, blk);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the cell's tables have reached L2
  LQ_LSTAMP(0);
  {
    const AggSet z = agg_set_init<NT>(ga, s);
    AggPart ap;
    if (z.order_ok) agg_cell<NT, true>(ga, z, s, c, agg_cell_range(z, c), lane, ap);
    LQ_LSTAMP(1);
    const AggRec x = agg_wave_record(ap);
    double* rc = rec + (size_t)blk * LQ_AGG_REC;
    if (lane < z.N) st_wt8(rc + lane, ap.accw);
    if (lane < 5) st_wt8(rc + LOMPC_MAX_N + lane, x.pick(lane));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int old = 0;
  if (lane == 0) {
    old = __hip_atomic_fetch_add(sa.ctl + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == S * G - 1) __hip_atomic_store(sa.ctl + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  LQ_LSTAMP(2);
  if (lqw::readlane_i(old, 0) != S * G - 1) return;
  // the last arriver: every record of both sets in flight at once (one memory round), each set
  // closed in cell order, then the loop step on the closed outputs
  AggSet zs[S];  // (agg_finish reads N and the sizes / order flags loaded at the start)
#pragma unroll
  for (int t = 0; t < S; ++t) {
    zs[t].N = NT ? NT : ga.N;
    zs[t].n_s = cl_n[t];
    zs[t].si = make_int4(cl_v[t], cl_ok[t], 0, 0);
    zs[t].order_ok = cl_ok[t] != 0;
  }
  const int N = zs[0].N;
  // (records k >= G read the zero record past the S * G real ones: no per-load branch or mask)
  double rw[S][LQ_LOOP_G], rx[S][LQ_LOOP_G];
  const int tl = min(lane, N - 1), xl = min(lane, 4);
#pragma unroll
  for (int t = 0; t < S; ++t)
#pragma unroll
    for (int k = 0; k < LQ_LOOP_G; ++k) {
      const double* rk = rec + (size_t)(k < G ? t * G + k : S * G) * LQ_AGG_REC;
      rw[t][k] = ld_t<true>(rk + tl);
      rx[t][k] = ld_t<true>(rk + LOMPC_MAX_N + xl);
    }
  LQ_LSTAMP(10);
  AggSetOut o[S];
#pragma unroll
  for (int t = 0; t < S; ++t)
    o[t] = agg_finish<false, true, LQ_LOOP_G>(ga, zs[t], t, lane, G, [&](int k) { return rw[t][k]; },
                             [&](int k) { return rx[t][k]; });
  LQ_LSTAMP(3);
  in.s0 = o[0].sumw;
  in.wk = o[1].sumw;
  in.emax = lqw::readlane_d(o[0].stat, LOMPC_STAT_MAX_ERR);
  in.cost_c = lqw::readlane_d(o[1].stat, LOMPC_STAT_SUM_COST);
  in.n_inv = lqw::readlane_d(o[0].stat, LOMPC_STAT_N_INVALID) + lqw::readlane_d(o[1].stat, LOMPC_STAT_N_INVALID);
  in.n_fail = lqw::readlane_d(o[0].stat, LOMPC_STAT_N_FAILED) + lqw::readlane_d(o[1].stat, LOMPC_STAT_N_FAILED);
#ifdef LOMPC_STAMPS
  loop_step_core(sa, m, lane, in, [&](int k) { LQ_LSTAMP(k); });
#else
  loop_step_core(sa, m, lane, in);
#endif
  LQ_LSTAMP(4);
}

// ---------------------------------------------------------------- k_loop_run
// The WHOLE device-resident price loop as ONE launch (persistent): the S * G waves of k_loop_iter
// run call after call.  Call m is k_loop_iter's body; the last arriver's step writes the next prices,
// the loop state and (m = 0) the A_bar factor write-through (sc1), drains them, and publishes the
// generation word ctl[2] = m + 1; every other wave polls ctl[2] (lane 0, sc1 loads, s_sleep backoff)
// and then re-reads everything the step wrote with sc1 loads (prices in the path, the aggregation and
// the step; the loop state and factor in step_prices) — MI355X_MICROARCH.md's valid hand-off form:
// sc1 payload drained before an sc1 flag, sc1 polls, sc1 payload loads.  The finishing step sets
// ctl[0] before its generation, so every wave leaves at the next call's top.  No launch boundary and
// no per-launch setup between calls (k_loop_iter: one launch per call, 1.5-1.7 us apart).  Bounded
// spins: a wave that waits LQ_RUN_SPINS polls without a new generation sets ctl[3] and ctl[0] and
// leaves (the host reports the timeout).  Same arithmetic as k_loop_iter: the same bits.
#ifndef LQ_RUN_SPINS
#define LQ_RUN_SPINS (1 << 22)  // ~ seconds of polls (a call takes ~15 us)
#endif
template <int NT>
__global__ __launch_bounds__(64) void k_loop_run(PathArgs pa, AggArgs ga, StepArgs sa, double* rec) {
  constexpr int S = 2;  // (lq_loop_fusable: the loop's two sets)
  const int blk = (int)blockIdx.x, lane = (int)threadIdx.x, G = pa.G;
  const int s = blk / G, c = blk - s * G;
  int cl_n[S], cl_v[S], cl_ok[S];  // (the sets' sizes and order flags: constant over the loop)
#pragma unroll
  for (int t = 0; t < S; ++t) {
    const int4 si = ga.sinfo[t];
    cl_n[t] = (int)(ga.set_off[t + 1] - ga.set_off[t]);
    cl_v[t] = si.x;
    cl_ok[t] = si.y;
    asm volatile("" : "+v"(cl_n[t]), "+v"(cl_v[t]), "+v"(cl_ok[t]));
  }
  for (int m = 0; m <= sa.max_iter; ++m) {
    if (m > 0) {  // call m - 1's step has published the prices of call m
      int ok = 1;
      if (lane == 0) {
        int spins = 0;
        while (__hip_atomic_load(sa.ctl + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < m) {
          __builtin_amdgcn_s_sleep(2);
          if (++spins >= LQ_RUN_SPINS) {
            ok = 0;
            break;
          }
        }
        if (!ok) {
          __hip_atomic_store(sa.ctl + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(sa.ctl + 0, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (!lqw::readlane_i(ok, 0)) return;
    }
    if (__hip_atomic_load(sa.ctl + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // finished
    StepIn in;
    step_prices<true>(sa, lane, in);
    path_cell<NT, true, true>(pa, blk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the cell's tables have reached L2
    {
      const AggSet z = agg_set_init<NT, true>(ga, s);
      AggPart ap;
      if (z.order_ok) agg_cell<NT, true, true>(ga, z, s, c, agg_cell_range(z, c), lane, ap);
      const AggRec x = agg_wave_record(ap);
      double* rc = rec + (size_t)blk * LQ_AGG_REC;
      if (lane < z.N) st_wt8(rc + lane, ap.accw);
      if (lane < 5) st_wt8(rc + LOMPC_MAX_N + lane, x.pick(lane));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int old = 0;
    if (lane == 0) {
      old = __hip_atomic_fetch_add(sa.ctl + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == S * G - 1) __hip_atomic_store(sa.ctl + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lqw::readlane_i(old, 0) != S * G - 1) continue;
    // the last arriver: both sets closed from the records (one memory round), then the loop step
    AggSet zs[S];
#pragma unroll
    for (int t = 0; t < S; ++t) {
      zs[t].N = NT ? NT : ga.N;
      zs[t].n_s = cl_n[t];
      zs[t].si = make_int4(cl_v[t], cl_ok[t], 0, 0);
      zs[t].order_ok = cl_ok[t] != 0;
    }
    const int N = zs[0].N;
    double rw[S][LQ_LOOP_G], rx[S][LQ_LOOP_G];
    const int tl = min(lane, N - 1), xl = min(lane, 4);
#pragma unroll
    for (int t = 0; t < S; ++t)
#pragma unroll
      for (int k = 0; k < LQ_LOOP_G; ++k) {
        const double* rk = rec + (size_t)(k < G ? t * G + k : S * G) * LQ_AGG_REC;
        rw[t][k] = ld_t<true>(rk + tl);
        rx[t][k] = ld_t<true>(rk + LOMPC_MAX_N + xl);
      }
    AggSetOut o[S];
#pragma unroll
    for (int t = 0; t < S; ++t)
      o[t] = agg_finish<false, true, LQ_LOOP_G>(ga, zs[t], t, lane, G, [&](int k) { return rw[t][k]; },
                                               [&](int k) { return rx[t][k]; });
    in.s0 = o[0].sumw;
    in.wk = o[1].sumw;
    in.emax = lqw::readlane_d(o[0].stat, LOMPC_STAT_MAX_ERR);
    in.cost_c = lqw::readlane_d(o[1].stat, LOMPC_STAT_SUM_COST);
    in.n_inv = lqw::readlane_d(o[0].stat, LOMPC_STAT_N_INVALID) + lqw::readlane_d(o[1].stat, LOMPC_STAT_N_INVALID);
    in.n_fail = lqw::readlane_d(o[0].stat, LOMPC_STAT_N_FAILED) + lqw::readlane_d(o[1].stat, LOMPC_STAT_N_FAILED);
    // the step releases call m + 1 as soon as its prices and loop state (sc1) have left this wave —
    // before its host-memory writes, which then overlap call m + 1 (a finishing step releases nothing:
    // its ctl[0] and `done` end the loop, and the waves leave at the next call's top)
    bool released = false;
    const auto release = [&]() {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(sa.ctl + 2, m + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      released = true;
    };
    loop_step_core(sa, m, lane, in, NoStamp{}, release);
    if (!released) {  // (finished: the waiting waves find ctl[0] behind this generation)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(sa.ctl + 2, m + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// k_loop_run, redundant form (LQ_LOOP_REDUNDANT): no hand-off of the step's results.  Every wave
// arrives on a monotonic counter (ctl[1]) after writing its cell record (write-through, drained),
// waits until all S * G waves of the call have arrived, loads every record (sc1) and runs the SAME
// closing and loop step as every other wave — the same instructions on the same records in the same
// order, so the same bits in every wave — and goes straight on to the next call with the prices, the
// loop state and the A_bar factor in its registers (the path and the aggregation take the prices from
// registers: no memory round between the step and the next path).  Wave 0 alone writes: the set
// outputs, the stats and tallies, the prices / state / factor to memory and the host results.  The
// records alternate between two buffers by call parity (a wave may write call m + 1's record while a
// slower wave still reads call m's: never call m + 2's, which needs every wave's call m + 1 arrival).
// The same arithmetic as k_loop_run and k_loop_iter: the same bits.
// The body is the text of lompc_looprun2_body.hpp, which k_loop_runs (below) includes too.
#ifndef LQ_LOOP_REDUNDANT
#define LQ_LOOP_REDUNDANT 1
#endif
template <int NT>
__global__ __launch_bounds__(64) void k_loop_run2(PathArgs pa, AggArgs ga, StepArgs sa, double* rec) {
  constexpr int S = 2;
  const int blk = (int)blockIdx.x, lane = (int)threadIdx.x, G = pa.G;
#include "lompc_looprun2_body.hpp"
}

// ---------------------------------------------------------------- k_loop_runs
// L independent price loops in ONE persistent launch (lompc_price_loops): L * S * G one-wave
// workgroups, workgroup b the wave blk = b - j * S * G of loop j = b / (S * G).  The wave takes loop j's
// record — what k_loop_run2 gets as kernel arguments — from the job array (wave-uniform scalar loads
// from constant memory, as kernel arguments are) and runs k_loop_run2's body on it
// (lompc_looprun2_body.hpp).  No object is shared between loops: each record names its own plan's arrival counter, cell records, zero record, loop state,
// pinned results and price buffer, so a loop's waves wait for that loop's S * G arrivals alone, and a
// loop that ends (converged, capped, failed, expired spin) leaves while the others go on.  The host
// launches no more loops than are resident at once (lq_loop_runs_places).
struct LoopJob {
  PathArgs pa;
  AggArgs ga;
  StepArgs sa;
  double* rec;
};
static_assert(sizeof(LoopJob) % 4 == 0, "LoopJob is copied by words");

template <int NT>
__global__ __launch_bounds__(64) void k_loop_runs(const LoopJob* jobs, int waves) {
  // (waves = S * G of every loop of the launch; the quotient comes out of the vector ALU: made scalar again)
  const int b = (int)blockIdx.x, j = __builtin_amdgcn_readfirstlane(b / waves);
  typedef const __attribute__((address_space(4))) unsigned int* cwords;
  cwords src = (cwords)(reinterpret_cast<const unsigned int*>(jobs + j));
  union U {
    LoopJob job;
    unsigned int w[sizeof(LoopJob) / 4];
    __device__ U() {}
  } u;
#pragma unroll
  for (int k = 0; k < (int)(sizeof(LoopJob) / 4); ++k) u.w[k] = src[k];
  const PathArgs& pa = u.job.pa;
  const AggArgs& ga = u.job.ga;
  const StepArgs& sa = u.job.sa;
  double* const rec = u.job.rec;
  constexpr int S = 2;
  const int blk = b - j * waves, lane = (int)threadIdx.x, G = pa.G;
#include "lompc_looprun2_body.hpp"
}

typedef void (*LoopRunKernel)(PathArgs, AggArgs, StepArgs, double*);
LoopRunKernel loop_run_kernel(int N) {
  if (LQ_LOOP_REDUNDANT) switch (N) {
      case 12: return k_loop_run2<12>;
      case 16: return k_loop_run2<16>;
      case 24: return k_loop_run2<24>;
      case 48: return k_loop_run2<48>;
      default: return k_loop_run2<0>;
    }
  switch (N) {
    case 12: return k_loop_run<12>;
    case 16: return k_loop_run<16>;
    case 24: return k_loop_run<24>;
    case 48: return k_loop_run<48>;
    default: return k_loop_run<0>;
  }
}

typedef void (*LoopIterKernel)(PathArgs, AggArgs, StepArgs, double*, int);
LoopIterKernel loop_iter_kernel(int N) {
  switch (N) {
    case 12: return k_loop_iter<12>;
    case 16: return k_loop_iter<16>;
    case 24: return k_loop_iter<24>;
    case 48: return k_loop_iter<48>;
    default: return k_loop_iter<0>;
  }
}
