// lompc_plan.hip — the PATH engine: a fixed EV batch (one price loop / one time step) solved
// at new prices every price iteration.
//
// Hot path replaced: LoMPC.solve_lompc (chargingstation/lompc.py:137-156) called once per EV
// from PriceSolver._get_w_err (price_solver.py:203-209) and PriceSolver.get_w0_price0
// (price_solver.py:280-283).  Within one parameter set (an (EV type, partition) price vector)
// every EV solves the same QP except gamma_i = y_max - y0_i (price_solver.py:202, :281), so
// w*(gamma) is a continuous piecewise-affine path with a handful of breakpoints over the
// set's gamma range.
//
// Plan (once per batch, lompc_plan_create): per-set gamma window [lo, hi] (range of the set's
// valid gamma, k_plan_window) cut into G cells; the block map of k_eval (256 consecutive EVs of
// one set per workgroup).
//
// Run (every price iteration, lompc_plan_run), three launches for ALL EV types of the plan:
//   k_path    one 64-lane wave per (set, cell), lane t = horizon stage t: exact solve at the
//             cell start (fp32 working-set search + fp64 PDAS, KKT-certified), then parametric
//             active-set tracking of w*(gamma) across the cell; every piece w = a + b gamma is
//             KKT-certified at its end (the residual is convex along an affine piece, so both
//             ends certify the whole piece) and stored with the cost and the squared A_bar
//             error as quadratics in gamma.  Latency-bound: wave-parallel DPP scans.
//   k_eval    256 EVs of one set per workgroup in the caller's order: the set's pieces staged
//             in LDS (a few KB), per EV (lane = EV) its piece, cost, w0, status, price0, A_bar
//             error; the w rows (lane = stage) as contiguous 16-B write-through stores; EVs no
//             certified piece covers listed for k_finalize; per-workgroup sums in a fixed
//             order.  HBM-bound: 8(N+2) B per EV.
//   k_finalize one workgroup per set: deterministic sum / max of its workgroups' records, and the
//             individual certified re-solve of any EV k_eval listed (no certified piece covers it).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "lompc_ctx.hpp"
#include "lompc_loopstep.hpp"
#include "lompc_wave.hpp"

#ifdef LOMPC_STAMPS
// diagnostic build only (scripts/kstamps.py): per-wave s_memtime at k_path's and k_eval's phase
// boundaries (k_eval: workgroup b at g_stamps[(32768 + b) * 8 + k]); LOMPC_STAMPS_RT: the
// device-wide 100 MHz s_memrealtime instead (comparable across XCDs: launch timelines)
#ifdef LOMPC_STAMPS_RT
#define __builtin_amdgcn_s_memtime __builtin_amdgcn_s_memrealtime
#endif
__device__ long long g_stamps[65536 * 8];
__device__ long long g_wstart[32768 * 8];          // k_eval: start of wave w of workgroup b at [b * 8 + w]
__device__ unsigned long long g_lstamps[64 * 16];  // k_loop_iter's phase sums (LQ_LSTAMP)
#define LQ_WSTART()                                                                              \
  do {                                                                                           \
    const long long t__ = __builtin_amdgcn_s_memtime();                                          \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 32768) g_wstart[blockIdx.x * 8 + (threadIdx.x >> 6)] = t__; \
  } while (0)
#define LQ_STAMPE(k)                                                                        \
  do {                                                                                      \
    const long long t__ = __builtin_amdgcn_s_memtime();                                     \
    if (threadIdx.x == 0 && blockIdx.x < 32768) g_stamps[(32768 + blockIdx.x) * 8 + (k)] = t__; \
  } while (0)
#define LQ_STAMPW(k)                                                                        \
  do {                                                                                      \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                        \
    LQ_STAMPE(k);                                                                           \
  } while (0)
#define LQ_STAMP(k)                                                                         \
  do {                                                                                      \
    const long long t__ = __builtin_amdgcn_s_memtime();                                     \
    if ((threadIdx.x & 63) == 0 && blk < 65536) g_stamps[blk * 8 + (k)] = t__;              \
  } while (0)
#else
#define LQ_STAMP(k)
#define LQ_STAMPE(k)
#define LQ_STAMPW(k)
#define LQ_WSTART()
#endif

#ifndef EVAL_WAVES
#define EVAL_WAVES 8  // k_eval: waves per workgroup (16: 16.1 us, 8: 14.8 us, 4: 16.2 us at config 3)
#endif
#ifndef EVAL_RU
#define EVAL_RU 2  // k_eval: row store instructions per software-pipelined batch (2: k_evals 11.17 vs 11.70 us
                   // per run with 4, 11.68 with 3 — the same rows in the same order, so the same bits)
#endif
#ifndef EVAL_MIN_WAVES
#define EVAL_MIN_WAVES ((2 * EVAL_WAVES + 3) / 4)  // k_eval: waves per SIMD for two workgroups per CU
#endif
#define EVAL_EVS (64 * EVAL_WAVES)         // k_eval: threads per workgroup
#ifndef EVAL_PASSES
#define EVAL_PASSES 2                      // k_eval: EVs per thread, at most
#endif
#ifndef LQ_EVAL_WV_SCALAR
#define LQ_EVAL_WV_SCALAR 1  // eval_block: the wave index as a scalar (0: as the compiler derives it from threadIdx)
#endif
#ifndef LQ_EVALS_KARGS
#define LQ_EVALS_KARGS 1  // k_evals: its arguments re-read from the kernel argument segment in every run (0: held in
                          // scalar registers across the runs' loop, which spills them to vector lanes)
#endif
#define EVAL_MAXB (EVAL_EVS * EVAL_PASSES)  // k_eval: EVs per workgroup, at most
#ifndef LQ_PIECE_CAP
#define LQ_PIECE_CAP 128                   // k_eval: piece slots of one set staged in LDS (more: re-solved)
#endif
#define LQ_GMAX 1024                       // max cells per set
#ifndef LQ_EVAL_OUT_AFTER_ROWS
#define LQ_EVAL_OUT_AFTER_ROWS 1  // k_eval / k_step / k_evals: a pass's scalar outputs after its rows
#endif
#ifndef LQ_DIAG_NOLOOKUP
#define LQ_DIAG_NOLOOKUP 0  // diagnostic timing builds: every valid EV takes its cell's first piece (wrong results)
#endif
#ifndef LQ_DIAG_NOROWLDS
#define LQ_DIAG_NOROWLDS 0  // diagnostic timing builds: the rows' values without their LDS reads (wrong results)
#endif
#ifndef LQ_STEP_CELLS
#define LQ_STEP_CELLS 4                    // k_step: path cells per workgroup, one per wave (<= EVAL_WAVES; 4: one per
                                           // SIMD — 19.2 us per step vs 22.4 with 8, 19.9 with 2, profiles/r03_v5)
#endif
#ifndef LQ_STEP_PRIO
#define LQ_STEP_PRIO 1                     // k_step: path waves at raised issue priority
#endif
#ifndef LQ_WARM_FP64
#define LQ_WARM_FP64 1                     // k_path with a warm start: fp64 PDAS straight from the stored set
#endif
#define LQ_DROP_OFF 0x7fff0000             // k_eval: a store offset past any w descriptor's range (dropped)

namespace {

// the device code: plain text in this order (the order the kernels are generated in); the host code follows
#include "lompc_plan_path.hpp"
#include "lompc_plan_eval.hpp"
#include "lompc_agg.hpp"
#include "lompc_scalar.hpp"
#include "lompc_plan_loop.hpp"

// ---------------------------------------------------------------- host helpers

// capacities of the buffers a re-targeted plan (lompc_plan_update) may outgrow: 1/4 headroom, and at
// least double the previous capacity, so a batch whose size wanders from call to call (a station's
// partitions, step to step: EVs move between charge-level partitions) reallocates O(log) times, not
// at every new high (hipMalloc / hipHostMalloc took 50-470 us per re-targeted plan in the station's
// staging, scripts/stage_profile.py)
int64_t with_slack(int64_t n, int64_t cap) { return std::max(n + n / 4 + 16, 2 * cap); }
constexpr int LQ_RESERVE_CELLS = 16;  // lompc_plan_reserve: cell-indexed buffers sized for this many cells per set (pick_cells' most)

#ifndef LQ_WIDE_ALPHA
#define LQ_WIDE_ALPHA 0.85  // EVs of a second-dispatch-round k_eval / k_evals block relative to a first-round one
#endif
// The k_eval block map of a batch: every set in near-equal blocks of <= maxb EVs (at least 256),
// `target` blocks in all, set-major (blocks[b] = (set, first EV, end EV); pre[s] = set s's first block).
// weighted (one dispatch round of persistent or single launches, more blocks than CUs): the blocks of
// the later dispatch round (index >= n_cu) get LQ_WIDE_ALPHA of the EVs of the first round's — a CU's
// second-dispatched workgroup runs ~13 % slower than its first (younger waves: the SIMDs' issue
// arbitration favours the older workgroup; scripts/evals_stamps.py), and a launch ends
// with its slowest workgroup.  Each set takes the blocks whose weights cover its share of the batch,
// and inside a set the EVs split in proportion to the weights.  A map only: the same QPs and per-EV
// arithmetic, the per-set sums combine per-block records in block order.
void block_map(const int64_t* off, int64_t S, int64_t B, int64_t maxb, int64_t target, int n_cu, bool weighted,
               std::vector<int4>& blks, std::vector<int>& pre) {
  blks.clear();
  pre.assign((size_t)S + 1, 0);
  auto blocks_of = [&](int64_t m) -> int64_t {
    if (m <= 0) return 0;
    const int64_t lo = (m + maxb - 1) / maxb, hi = (m + 255) / 256;
    return std::max<int64_t>(lo, std::min<int64_t>(hi, m * target / std::max<int64_t>(B, 1)));
  };
  int64_t nblk = 0;
  for (int64_t s = 0; s < S; ++s) nblk += blocks_of(off[s + 1] - off[s]);
  if (weighted && LQ_WIDE_ALPHA < 1.0 && nblk > (int64_t)n_cu && B > 0) {
    std::vector<double> wc((size_t)nblk + 1, 0.0);
    for (int64_t k = 0; k < nblk; ++k) wc[k + 1] = wc[k] + (k < (int64_t)n_cu ? 1.0 : LQ_WIDE_ALPHA);
    std::vector<int64_t> lo_of((size_t)S);
    int64_t need_after = 0;  // blocks the later non-empty sets need at least
    for (int64_t t = 0; t < S; ++t) {
      const int64_t m = off[t + 1] - off[t];
      lo_of[t] = m > 0 ? (m + maxb - 1) / maxb : 0;
      need_after += lo_of[t];
    }
    auto wt = [&](int64_t k) { return k < nblk ? wc[k] : wc[nblk] + (double)(k - nblk) * LQ_WIDE_ALPHA; };
    int64_t b = 0;
    for (int64_t s = 0; s < S; ++s) {
      const int64_t o = off[s], m = off[s + 1] - o;
      need_after -= lo_of[s];
      int64_t nb = lo_of[s];
      if (m > 0) {
        const double tgt = wc[nblk] * (double)off[s + 1] / (double)B;  // the set's cumulative weight
        const int64_t hi = std::min<int64_t>((m + 255) / 256, nblk - b - need_after);
        while (nb < hi && b + nb < nblk && wc[b + nb] + 0.5 * (wc[b + nb + 1] - wc[b + nb]) < tgt) ++nb;
      }
      auto fits = [&](int64_t n) {  // every block of the set within maxb EVs (the kernels' LDS rows)
        const double ws_ = wt(b + n) - wt(b);
        for (int64_t k = 0; k < n; ++k)
          if ((double)m * (wt(b + k + 1) - wt(b + k)) / ws_ > (double)(maxb - 2)) return false;
        return true;
      };
      while (m > 0 && nb < m && !fits(nb)) ++nb;
      const double w0 = wt(b), ws = wt(b + nb) - w0;
      for (int64_t k = 0; k < nb; ++k) {
        const int64_t e0 = o + (int64_t)((double)m * (wt(b + k) - w0) / ws);
        const int64_t e1 = k + 1 == nb ? o + m : o + (int64_t)((double)m * (wt(b + k + 1) - w0) / ws);
        blks.push_back(make_int4((int)s, (int)e0, (int)e1, 0));
      }
      b += nb;
      pre[s + 1] = (int)b;
    }
    return;
  }
  for (int64_t s = 0; s < S; ++s) {
    const int64_t o = off[s], m = off[s + 1] - o, nb = blocks_of(m);
    for (int64_t k = 0; k < nb; ++k) blks.push_back(make_int4((int)s, (int)(o + m * k / nb), (int)(o + m * (k + 1) / nb), 0));
    pre[s + 1] = (int)blks.size();
  }
}

int pick_cells(int64_t max_set, int flags) {
  const int g = (flags >> LOMPC_PLAN_CELLS_SHIFT) & 2047;  // the caller's choice (LOMPC_PLAN_CELLS)
  if (g >= 1 && g <= LQ_GMAX) return g;
  // the path of a set has a handful of breakpoints over its gamma window: the cell count trades
  // per-wave tracking latency against more cold starts; one cell for tiny sets
  if (max_set <= 64) return 1;
  if (max_set <= 1024) return 8;
  return 16;  // measured flat over 12..24 at config 3 (42.1-42.4 us/step), 8 and 48+ slower
}

int take_events(std::vector<hipEvent_t>& pool, hipEvent_t* e0, hipEvent_t* e1) {
  for (hipEvent_t* e : {e0, e1}) {
    if (!pool.empty()) {
      *e = pool.back();
      pool.pop_back();
    } else if (hipEventCreateWithFlags(e, hipEventDisableSystemFence) != hipSuccess) {
      return LOMPC_ERR_HIP;
    }
  }
  return LOMPC_OK;
}

// every recorded pair (a pair may span `mult` launches: read as that many launches)
int plan_events_read(std::vector<hipEvent_t>& ev, std::vector<int>& mult, std::vector<hipEvent_t>& pool, double& ms_acc,
                     int64_t& n_acc) {
  for (size_t k = 0; k + 1 < ev.size(); k += 2) {
    if (hipEventSynchronize(ev[k + 1]) != hipSuccess) return LOMPC_ERR_HIP;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) != hipSuccess) return LOMPC_ERR_HIP;
    ms_acc += ms;
    n_acc += k / 2 < mult.size() ? mult[k / 2] : 1;
  }
  pool.insert(pool.end(), ev.begin(), ev.end());
  ev.clear();
  mult.clear();
  return LOMPC_OK;
}

}  // namespace

// ============================================================== host
// k_eval's dynamic LDS: up to cap pieces of one set (NS double2 + 8 + 1 doubles each) + the cells
size_t eval_lds(int N, int G, int cap) {
  const size_t stage = (size_t)cap * (eval_row_stride(N) * sizeof(double2) + 9 * sizeof(double)) +
                       (size_t)2 * eval_row_stride(N) * sizeof(double2) +
                       (size_t)G * sizeof(double) + (size_t)((G + 1) & ~1) * sizeof(int) +
                       (size_t)(cap + 2) * (sizeof(unsigned long long) + sizeof(int));
  return std::max(stage, (size_t)2 * EVAL_WAVES * FIN_W * sizeof(double));  // (close mode: red / rep)
}

// The dynamic LDS the evaluation kernels of horizon N may ask for: a workgroup's LDS on the device less
// the largest static LDS of k_eval (both close modes), k_evals and k_step (any of them may run a plan).
// Queried once per (device, instantiation) in the process.
static int eval_lds_room(lompc_plan* p, int device, int N, size_t* room) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, size_t> known;
  const int inst = (N == 12 || N == 16 || N == 24 || N == 48) ? N : 0;
  std::lock_guard<std::mutex> lock(mu);
  const auto it = known.find({device, inst});
  if (it != known.end()) {
    *room = it->second;
    return LOMPC_OK;
  }
  int limit = 0;
  HIPCHK(p, hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  const void* const kern[4] = {(const void*)eval_kernel<false>(N), (const void*)eval_kernel<true>(N),
                               (const void*)evals_kernel(N), (const void*)step_kernel(N)};
  size_t fixed = 0;
  for (const void* f : kern) {
    hipFuncAttributes at;
    HIPCHK(p, hipFuncGetAttributes(&at, f));
    fixed = std::max(fixed, (size_t)at.sharedSizeBytes);
  }
  *room = (size_t)limit > fixed ? (size_t)limit - fixed : 0;
  // the runtime's own account must agree that a workgroup asking for all of it is resident (a request
  // past the limit is not refused at the launch: it aborts the queue)
  for (const void* f : kern) {
    int occ = 0;
    while (*room >= 1024) {
      HIPCHK(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, f, EVAL_EVS, *room));
      if (occ >= 1) break;
      *room -= 1024;
    }
  }
  known[{device, inst}] = *room;
  return LOMPC_OK;
}

// The piece slots of one set that the evaluation stages in LDS (EvalArgs::cap): LQ_PIECE_CAP, or all of
// the set's G LQ_PPL when that is fewer, lowered by whole cells until eval_lds fits beside the kernels'
// static LDS (long horizons with many cells: 16 (N + 1) + 92 bytes per slot and 12 per cell).  The EVs
// of the cells left unstaged take the certified individual re-solve, as those past LQ_PIECE_CAP do.
static int eval_cap(lompc_plan* p, int device, int N, int G, int* cap) {
  size_t room = 0;
  const int rc = eval_lds_room(p, device, N, &room);
  if (rc) return rc;
  int c = std::min(LQ_PIECE_CAP, G * LQ_PPL);
  while (c > LQ_PPL && eval_lds(N, G, c) > room) c -= LQ_PPL;
  if (eval_lds(N, G, c) > room) {
    p->err = "plan: horizon " + std::to_string(N) + " with " + std::to_string(G) +
             " cells per set does not fit a workgroup's LDS (" + std::to_string(room) + " bytes for the evaluation)";
    return LOMPC_ERR_UNSUPPORTED;
  }
  *cap = c;
  return LOMPC_OK;
}

// The cells of one set that k_scalar / k_scalars stage in LDS (LOMPC_PLAN_SCALAR_PASS): all G, lowered by whole cells
// until scalar_lds fits beside the kernels' static LDS on the device (576 bytes per cell and 12 per cell
// of the set: every G <= 256 fits whole at any horizon).  As for k_eval the request is checked here, on
// the host: one past the limit is not refused at the launch, it aborts the queue.  The EVs of the cells
// left unstaged take the certified individual re-solve.
static int scalar_cells_fit(lompc_plan* p, int device, int G, int* cells) {
  static std::mutex mu;
  static std::map<int, size_t> known;
  size_t room = 0;
  {
    std::lock_guard<std::mutex> lock(mu);
    const auto it = known.find(device);
    if (it != known.end()) {
      room = it->second;
    } else {
      int limit = 0;
      HIPCHK(p, hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
      // (k_scalar and k_scalars: either may run the plan, so the larger static LDS counts)
      const void* const kern[2] = {(const void*)k_scalar, (const void*)k_scalars};
      size_t fixed = 0;
      for (const void* f : kern) {
        hipFuncAttributes at;
        HIPCHK(p, hipFuncGetAttributes(&at, f));
        fixed = std::max(fixed, (size_t)at.sharedSizeBytes);
      }
      room = (size_t)limit > fixed ? (size_t)limit - fixed : 0;
      for (const void* f : kern) {  // (the runtime's own account must agree, as in eval_lds_room)
        int occ = 0;
        while (room >= 1024) {
          HIPCHK(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, f, EVAL_EVS, room));
          if (occ >= 1) break;
          room -= 1024;
        }
      }
      known[device] = room;
    }
  }
  int c = G;
  while (c > 1 && scalar_lds(G, c) > room) --c;
  if (scalar_lds(G, c) > room) {
    p->err = "plan: the scalar pass with " + std::to_string(G) + " cells per set does not fit a workgroup's LDS (" +
             std::to_string(room) + " bytes)";
    return LOMPC_ERR_UNSUPPORTED;
  }
  *cells = c;
  return LOMPC_OK;
}

// events of one profiled dispatch (null events when kernel k is not profiled)
int plan_prof_begin(lompc_plan* p, int k, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  return (p->prof >> k) & 1 ? take_events(p->prof_pool, e0, e1) : LOMPC_OK;
}
void plan_prof_end(lompc_plan* p, int k, hipEvent_t e0, hipEvent_t e1, int launches = 1) {
  if (!e0) return;
  p->prof_ev[k].push_back(e0);
  p->prof_ev[k].push_back(e1);
  p->prof_mult[k].push_back(launches);
}
// One launch with its profile events: the event pair of kernel k (null when k is not profiled, or when
// `carry` is false — a launch that carries no events at all, LOMPC_STEPS_SPAN_EVENTS past the first
// group), launch(e0, e1) (a hipExtLaunchKernelGGL), the launch check, and the pair recorded as `launches`.
template <typename Launch>
int timed_launch(lompc_plan* p, int k, int launches, bool carry, Launch&& launch) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (carry && plan_prof_begin(p, k, &e0, &e1)) return fail_arg(p, "profiling events");
  launch(e0, e1);
  HIPCHK(p, hipGetLastError());
  if (carry) plan_prof_end(p, k, e0, e1, launches);
  return LOMPC_OK;
}

#ifdef LQ_PREP_PROF  // diagnostic builds: lq_plan_prepare's phases on stderr (host microseconds)
#define LQ_PREP_MARK(k) prep_t[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count()
#else
#define LQ_PREP_MARK(k)
#endif
int lq_plan_prepare(lompc_plan* p, int nctx, lompc_ctx* const* ctxs, const int64_t* sets_per_ctx, int64_t B,
                    const double* gamma, const int64_t* set_offsets, const double* w_ref, int flags,
                    hipStream_t st) {
#ifdef LQ_PREP_PROF
  double prep_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  struct PrepPrint {
    double* t;
    ~PrepPrint() {
      fprintf(stderr, "prep us: checks %.1f occ %.1f grow %.1f evsync %.1f host %.1f copy %.1f kernels %.1f\n", t[1] - t[0],
              t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5], t[7] - t[6]);
    }
  } prep_print{prep_t};
#endif
  LQ_PREP_MARK(0);
  if (nctx < 1 || nctx > LQ_PLAN_MAX_CTX || !ctxs || !sets_per_ctx || !set_offsets)
    return fail_arg(p, "plan: 1 <= n_ctx <= LOMPC_PLAN_MAX_CTX contexts and their set counts required");
  int64_t S = 0;
  for (int k = 0; k < nctx; ++k) {
    if (!ctxs[k]) return fail_arg(p, "plan: null context");
    if (ctxs[k]->N != ctxs[0]->N || ctxs[k]->device != ctxs[0]->device)
      return fail_arg(p, "plan: every context must have the same horizon N and device");
    if (sets_per_ctx[k] < 0) return fail_arg(p, "plan: negative set count");
    S += sets_per_ctx[k];
  }
  if (S < 1) return fail_arg(p, "plan: at least one parameter set required");
  if (S > (1 << 20)) return fail_arg(p, "plan: too many parameter sets");
  if (B < 0 || B >= (1ll << 31) - EVAL_MAXB) return fail_arg(p, "plan: 0 <= B < 2^31 required");
  if (set_offsets[0] != 0 || set_offsets[S] != B) return fail_arg(p, "plan: set_offsets must run from 0 to B");
  int64_t max_set = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t m = set_offsets[s + 1] - set_offsets[s];
    if (m < 0) return fail_arg(p, "plan: set_offsets must be non-decreasing");
    max_set = std::max(max_set, m);
  }
  if (B > 0 && !gamma) return fail_arg(p, "plan: gamma required");
  const int N = ctxs[0]->N;
  HIPCHK(p, hipSetDevice(ctxs[0]->device));
  if (((flags >> LOMPC_PLAN_CELLS_SHIFT) & 2047) > LQ_GMAX) return fail_arg(p, "plan: at most 1024 cells per set");
  const int G = pick_cells(max_set, flags);
  const int64_t ncell = S * G;
  // k_eval work split: every set in nb near-equal blocks of <= EVAL_MAXB EVs, the block count
  // chosen so the workgroups fill the CUs a whole number of times (r rounds of n_cu, at most 90%
  // of EVAL_MAXB per block) rather than spilling a few blocks into an extra round
  if (!p->n_cu) {
    HIPCHK(p, hipDeviceGetAttribute(&p->n_cu, hipDeviceAttributeMultiprocessorCount, ctxs[0]->device));
    if (p->n_cu < 1) p->n_cu = 1;
  }
  LQ_PREP_MARK(1);
  int cap = 0;
  if (const int rc_cap = eval_cap(p, ctxs[0]->device, N, G, &cap)) return rc_cap;
  int scalar_cells = 0;
  if (flags & LOMPC_PLAN_SCALAR_PASS)
    if (const int rc_sc = scalar_cells_fit(p, ctxs[0]->device, G, &scalar_cells)) return rc_sc;
  const int64_t occ_key = (int64_t)N * 4096 + cap;
  if (p->eval_occ_key != occ_key) {  // k_eval workgroups resident per CU (either variant may run)
    int occ0 = 0, occ1 = 0;
    HIPCHK(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ0, eval_kernel<false>(N), EVAL_EVS, eval_lds(N, G, cap)));
    HIPCHK(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ1, eval_kernel<true>(N), EVAL_EVS, eval_lds(N, G, cap)));
    p->eval_occ = std::max(std::min(occ0, occ1), 1);
    p->eval_occ_key = occ_key;
  }
  LQ_PREP_MARK(2);
  const int64_t slots = (int64_t)p->n_cu * p->eval_occ;
  const int64_t rounds = std::max<int64_t>(1, (10 * B + 9ll * slots * EVAL_MAXB - 1) / (9ll * slots * EVAL_MAXB));
  const int64_t target = rounds * slots;
  // the k_eval block map (weighted by dispatch round when the blocks take one round: block_map)
  std::vector<int4> bmap;
  std::vector<int> bpre;
  block_map(set_offsets, S, B, EVAL_MAXB, target, p->n_cu, rounds == 1, bmap, bpre);
  const int64_t nblk = (int64_t)bmap.size();
  int64_t n_empty = 0;
  // lompc_plan_reserve: a buffer that must grow is sized at once for the reserved batch size (upper
  // bounds: blocks_of(m) <= ceil(m / 256), sorted blocks ceil(m / LQ_AGG_SB) per set)
  const int64_t RB = std::max(B, p->reserve_B);
  const int64_t nblk_r = p->reserve_B ? RB / 256 + S + 1 : 0, nsblk_r = p->reserve_B ? RB / LQ_AGG_SB + S + 1 : 0;
  for (int64_t s = 0; s < S; ++s) n_empty += bpre[s + 1] == bpre[s] ? 1 : 0;
  p->device = ctxs[0]->device;
  p->N = N;
  p->nctx = nctx;
  for (int k = 0; k < nctx; ++k) p->ctx[k] = ctxs[k];
  p->flags = flags;
  p->w_ref = w_ref;
  p->gamma = gamma;
  int rc;
  if (!p->d_errflag) {
    if ((rc = grow(p, &p->d_errflag, 1))) return rc;
    HIPCHK(p, hipMemset(p->d_errflag, 0, sizeof(int)));
  }
  if (!p->ev_stage) HIPCHK(p, hipEventCreateWithFlags(&p->ev_stage, hipEventDisableTiming));
  if (S > p->cap_S) {
    if ((rc = grow(p, &p->d_window, 2 * S)) || (rc = grow(p, &p->d_wacc, 3 * S)) ||
        (rc = grow(p, &p->d_stats_own, S * LOMPC_SET_STATS)) || (rc = grow(p, &p->d_arrive, S)))
      return rc;
    HIPCHK(p, hipMemsetAsync(p->d_wacc, 0, 3 * S * sizeof(unsigned long long), st));
    HIPCHK(p, hipMemsetAsync(p->d_arrive, 0, S * sizeof(int), st));
    p->cap_S = S;
  }
  if (nblk > p->cap_blk) {
    const int64_t c = std::max(with_slack(nblk, p->cap_blk), nblk_r);
    if ((rc = grow(p, &p->d_partial, (size_t)c * (N + NPX))) ||
        (rc = grow(p, &p->d_fail_cnt, (size_t)c * EVAL_WAVES)) || (rc = grow(p, &p->d_fail_idx, (size_t)c * EVAL_MAXB)))
      return rc;
    p->cap_blk = c;
  }
  const bool warm = (flags & LOMPC_PLAN_WARM_START) != 0;
  bool fresh_ws = false;
  if (ncell > p->cap_cells || (warm && !p->d_ws)) {
    // (a reserved plan: sized for the most cells the plan's choice gives a set, LQ_RESERVE_CELLS)
    const int64_t cn = std::max(ncell, p->reserve_B ? S * (int64_t)std::max(G, LQ_RESERVE_CELLS) : 0);
    if ((rc = grow(p, &p->t_cnt, cn)) || (rc = grow(p, &p->t_lo, cn)) ||
        (rc = grow(p, &p->t_ge, cn * LQ_PPL)) || (rc = grow(p, &p->t_cf, cn * LQ_PPL * 8)) ||
        (rc = grow(p, &p->t_ab, cn * LQ_PPL * N)) || (rc = grow(p, &p->t_sl, 2 * cn * 64)))
      return rc;
    if (warm && (rc = grow(p, &p->d_ws, (size_t)cn * 64))) return rc;
    p->cap_cells = cn;
    fresh_ws = true;
  }
  // (0xff: no stored set — a cell's first run starts cold, from "all free", and its later runs warm)
  if (warm && (fresh_ws || p->G != G || p->S != S)) HIPCHK(p, hipMemsetAsync(p->d_ws, 0xff, (size_t)ncell * 64, st));
  if (!p->d_tally) {
    if ((rc = grow(p, &p->d_tally, 3))) return rc;
    HIPCHK(p, hipMemsetAsync(p->d_tally, 0, 3 * sizeof(unsigned long long), st));
  }
  // the sets close inside k_eval when the plan asks for it, and by default in single runs that
  // write no w rows (a price loop's reductions-only runs): nothing then makes the arriving
  // workgroups wait for row stores, and the k_finalize launch and its boundary go
  p->close = (flags & LOMPC_PLAN_CLOSE_IN_EVAL) != 0;
  p->close_no_w = (flags & LOMPC_PLAN_CLOSE_IN_FINALIZE) == 0;
  p->B = B;
  p->S = S;
  p->G = G;
  p->cap = cap;
  p->scalar_cells = scalar_cells;
  p->nblk = (int)nblk;
  p->n_empty = (int)n_empty;
  p->d_stats = p->d_stats_own;
  p->stp.ok = false;
  // host arrays -> pinned staging -> device (the staging may still feed the previous prepare)
  // the plan's host-built metadata, one block in pinned memory and one copy to its device
  // mirror: [QPConst x LQ_PLAN_MAX_CTX | int4 blocks | int64 set offsets | int block prefix]
  auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t o_blk = up16(LQ_PLAN_MAX_CTX * sizeof(QPConst));
  const size_t o_off = o_blk + up16((size_t)nblk * sizeof(int4));
  const size_t o_pre = o_off + up16((size_t)(S + 1) * sizeof(int64_t));
  // gamma-sorted sets: blocks of <= LQ_AGG_SB positions of one set for the prepare kernels
  // (the exact prefix sums hold 2^40-scaled gamma in 64 bits: a set of 2^24 EVs or more would wrap,
  // so such a plan evaluates every EV instead)
  const bool sorted = (flags & LOMPC_PLAN_SORTED_GAMMA) != 0 && max_set < (1ll << 24);
  int64_t nsblk = 0;
  if (sorted)
    for (int64_t s = 0; s < S; ++s) nsblk += (set_offsets[s + 1] - set_offsets[s] + LQ_AGG_SB - 1) / LQ_AGG_SB;
  const size_t o_sblk = o_pre + up16((size_t)(S + 1) * sizeof(int));
  const size_t o_spre = o_sblk + up16((size_t)nsblk * sizeof(int4));
  const size_t need_h = sorted ? o_spre + up16((size_t)(S + 1) * sizeof(int)) : o_sblk;
  const size_t need_h_r = p->reserve_B ? up16(LQ_PLAN_MAX_CTX * sizeof(QPConst)) + up16((size_t)nblk_r * sizeof(int4)) +
                                             2 * up16((size_t)(S + 1) * sizeof(int64_t)) + up16((size_t)nsblk_r * sizeof(int4)) +
                                             up16((size_t)(S + 1) * sizeof(int))
                                       : 0;
  LQ_PREP_MARK(3);
  HIPCHK(p, hipEventSynchronize(p->ev_stage));  // (the staging may still feed the previous copy)
  LQ_PREP_MARK(4);
  if ((int64_t)need_h > p->cap_h) {
    const int64_t c = std::max(with_slack((int64_t)need_h, p->cap_h), (int64_t)need_h_r);
    if (p->h_buf) HIPCHK(p, hipHostFree(p->h_buf));
    p->h_buf = nullptr;
    HIPCHK(p, hipHostMalloc((void**)&p->h_buf, (size_t)c, hipHostMallocDefault));
    if ((rc = grow(p, &p->d_meta, (size_t)c))) return rc;
    p->cap_h = c;
  }
  QPConst* hq = reinterpret_cast<QPConst*>(p->h_buf);
  for (int k = 0; k < nctx; ++k) hq[k] = ctxs[k]->q;
  int4* hblk = reinterpret_cast<int4*>(p->h_buf + o_blk);
  int64_t* hoff = reinterpret_cast<int64_t*>(p->h_buf + o_off);
  p->h_off_at = (int64_t)o_off;
  int* hpre = reinterpret_cast<int*>(p->h_buf + o_pre);
  memcpy(hoff, set_offsets, (S + 1) * sizeof(int64_t));
  if (nblk > 0) memcpy(hblk, bmap.data(), (size_t)nblk * sizeof(int4));
  memcpy(hpre, bpre.data(), (size_t)(S + 1) * sizeof(int));
  for (int k = 0, e = 0; k < LQ_PLAN_MAX_CTX; ++k) {
    e += k < nctx ? (int)sets_per_ctx[k] : 0;
    p->ce.end[k] = k + 1 < nctx ? e : (int)S;  // contexts past the last: never selected
  }
  p->d_q = reinterpret_cast<QPConst*>(p->d_meta);
  p->d_blk = reinterpret_cast<int4*>(p->d_meta + o_blk);
  p->d_set_off = reinterpret_cast<int64_t*>(p->d_meta + o_off);
  p->d_blk_prefix = reinterpret_cast<int*>(p->d_meta + o_pre);
  p->sorted = sorted;
  p->nsblk = (int)nsblk;
  if (sorted) {
    int4* hs = reinterpret_cast<int4*>(p->h_buf + o_sblk);
    int* hsp = reinterpret_cast<int*>(p->h_buf + o_spre);
    int64_t k = 0;
    hsp[0] = 0;
    for (int64_t s = 0; s < S; ++s) {
      for (int64_t i = set_offsets[s]; i < set_offsets[s + 1]; i += LQ_AGG_SB)
        hs[k++] = make_int4((int)s, (int)i, (int)std::min<int64_t>(i + LQ_AGG_SB, set_offsets[s + 1]), 0);
      hsp[s + 1] = (int)k;
    }
    p->d_sblk = reinterpret_cast<int4*>(p->d_meta + o_sblk);
    p->d_sblk_prefix = reinterpret_cast<int*>(p->d_meta + o_spre);
    p->aggF = G * LQ_AGG_KF;
    const int64_t nP = 3 * (B + S), npos = S * (int64_t)(p->aggF + 1);
    if (nsblk > p->cap_sblk) {
      const int64_t c = std::max(with_slack(nsblk, p->cap_sblk), nsblk_r);
      if ((rc = grow(p, &p->d_bsum, (size_t)c * 4))) return rc;
      p->cap_sblk = c;
    }
    if (nP > p->cap_P) {
      const int64_t c = std::max(with_slack(nP, p->cap_P), p->reserve_B ? 3 * (RB + S) : 0);
      if ((rc = grow(p, &p->d_P, c))) return rc;
      p->cap_P = c;
    }
    if (npos > p->cap_pos) {
      const int64_t pr = std::max(npos, p->reserve_B ? S * (int64_t)(std::max(G, LQ_RESERVE_CELLS) * LQ_AGG_KF + 1) : 0);
      if ((rc = grow(p, &p->d_pos, pr))) return rc;
      p->cap_pos = pr;
    }
    if (S > p->cap_sinfo) {
      if ((rc = grow(p, &p->d_sinfo, S))) return rc;
      p->cap_sinfo = S;
    }
  }
  LQ_PREP_MARK(5);
  HIPCHK(p, hipMemcpyAsync(p->d_meta, p->h_buf, need_h, hipMemcpyHostToDevice, st));
  HIPCHK(p, hipEventRecord(p->ev_stage, st));
  LQ_PREP_MARK(6);
  WindowArgs wa{p->d_q, p->ce, p->d_blk, p->d_blk_prefix, gamma, p->d_wacc, p->d_window, (int)S, (int)nblk};
  if (sorted) hipLaunchKernelGGL(k_plan_window_sorted, dim3((unsigned)S), dim3(64), 0, st, wa, p->d_set_off);
  else hipLaunchKernelGGL(k_plan_window, dim3((unsigned)nblk + 1), dim3(256), 0, st, wa);
  HIPCHK(p, hipGetLastError());
  if (sorted) {  // order check, prefix sums and fine index of the sorted sets (lompc_agg.hpp)
    SortArgs sa{p->d_q, p->ce, p->d_sblk, p->d_sblk_prefix, p->d_set_off, gamma, p->d_window, p->d_bsum, p->d_P,
                p->d_pos, p->d_sinfo, (int)S, G, p->aggF, B + S};
    if (nsblk > 0) hipLaunchKernelGGL(k_sorted_sum, dim3((unsigned)nsblk), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_sorted_scan, dim3((unsigned)S), dim3(256), 0, st, sa);
    if (nsblk > 0) hipLaunchKernelGGL(k_sorted_fill, dim3((unsigned)nsblk), dim3(256), 0, st, sa);
    HIPCHK(p, hipGetLastError());
  }
  LQ_PREP_MARK(7);
  return LOMPC_OK;
}

// the plan's path table; `half` selects one of the two halves of the cell-start working sets
// (run_steps alternates them: a run's closing may re-solve from its own while the next run's path
// writes the other)
PathTab own_tab(const lompc_plan* p, int half = 0) {
  PathTab t;
  t.cnt = p->t_cnt;
  t.lo = p->t_lo;
  t.ge = p->t_ge;
  t.cf = p->t_cf;
  t.ab = p->t_ab;
  t.sl = p->t_sl + (size_t)half * p->S * p->G * 64;
  return t;
}

PathArgs path_args(lompc_plan* p, const double* lmbd, const double* lmbd_r, const PathTab& tb) {
  PathArgs pa{};
  const int N = p->N;
  pa.S = (int)p->S;
  pa.G = p->G;
  pa.N = N;
  pa.flags = p->flags;
  pa.qd = p->d_q;
  pa.ce = p->ce;
  pa.window = p->d_window;
  pa.lmbd = lmbd;
  pa.lmbd_r = lmbd_r;
  pa.w_ref = p->w_ref;
  pa.ws = (p->flags & LOMPC_PLAN_WARM_START) ? p->d_ws : nullptr;
  pa.t_cnt = tb.cnt;
  pa.t_lo = tb.lo;
  pa.t_sl = tb.sl;
  pa.t_ge = tb.ge;
  pa.t_cf = tb.cf;
  pa.t_ab = tb.ab;
  pa.errflag = p->d_errflag;
  pa.skip = p->skip;
  return pa;
}

// k_path of one run into the path table `tb`; with `fin` (run_steps) the previous run's closing
// rides in the same launch (k_path_fin)
int lq_launch_path(lompc_plan* p, const double* lmbd, const double* lmbd_r, const PathTab& tb, hipStream_t st,
                   const FinalArgs* fin = nullptr) {
  if (!lmbd || !lmbd_r) return fail_arg(p, "run: lmbd and lmbd_r required");
  const PathArgs pa = path_args(p, lmbd, lmbd_r, tb);
  const unsigned ncell = (unsigned)(p->S * p->G);
  return timed_launch(p, LOMPC_PLAN_K_PATH, 1, true, [&](hipEvent_t e0, hipEvent_t e1) {
    if (fin)
      hipExtLaunchKernelGGL(path_fin_kernel(p->N), dim3(ncell + (unsigned)p->S), dim3(64), 0, st, e0, e1, 0, pa, *fin);
    else
      hipExtLaunchKernelGGL(path_kernel(p->N), dim3(ncell), dim3(64), 0, st, e0, e1, 0, pa);
  });
}

// k_agg's / k_aggs' / the price loops' arguments from path table `tb` into the given set outputs
AggArgs agg_args(const lompc_plan* p, const double* lmbd, const double* lmbd_r, const PathTab& tb, double* set_sum_w,
                 double* set_stats, const int* skip) {
  return AggArgs{(int)p->S, p->G, p->N, p->aggF, p->d_q, p->ce, p->d_set_off, p->d_window, p->gamma, lmbd, lmbd_r,
                 p->w_ref, tb.cnt, tb.lo, tb.sl, tb.ge, tb.cf, tb.ab, p->d_P, p->B + p->S, p->d_pos,
                 p->d_sinfo, set_sum_w, set_stats, p->d_stats, p->d_tally, skip};
}

// the rest of one run from the path table `tb`: k_eval (or k_agg) and k_finalize, then with a
// communicator the all-gather and the combine
// defer (run_steps, no communicator): a k_finalize launch is not issued but its arguments are
// returned in *defer (defer->N = 0 when this run needs none) for the next run's k_path_fin
// the arguments of k_eval and of the set closing for one run from path table `tb`
void eval_args(lompc_plan* p, const double* lmbd, const double* lmbd_r, double* w, double* cost, double* w0,
               int8_t* status, const PathTab& tb, EvalArgs& a, FinalArgs& r) {
  const int N = p->N;
  a = EvalArgs{};
  a.S = (int)p->S;
  a.G = p->G;
  a.N = N;
  a.want_err = 1;
  a.qd = p->d_q;
  a.ce = p->ce;
  a.blk = p->d_blk;
  a.set_off = p->d_set_off;
  a.window = p->d_window;
  a.gamma = p->gamma;
  a.lmbd = lmbd;
  a.lmbd_r = lmbd_r;
  a.w_ref = p->w_ref;
  a.t_cnt = tb.cnt;
  a.t_lo = tb.lo;
  a.t_sl = tb.sl;
  a.t_ge = tb.ge;
  a.t_cf = tb.cf;
  a.t_ab = tb.ab;
  a.w = w;
  a.cost = cost;
  a.w0 = w0;
  a.status = status;
  a.partial = p->d_partial;
  a.fail_cnt = p->d_fail_cnt;
  a.fail_idx = p->d_fail_idx;
  a.w_rsrc_ok = (p->B * (int64_t)N * 8) <= LQ_DROP_OFF ? 1 : 0;
  a.w_bytes = a.w_rsrc_ok ? (int)(p->B * (int64_t)N * 8) : 0;
  a.cap = p->cap;
  a.nblk = p->nblk;
  a.skip = p->skip;
  r = FinalArgs{};
  r.N = N;
  r.G = p->G;
  r.want_err = 1;
  r.qd = p->d_q;
  r.ce = p->ce;
  r.blk_prefix = p->d_blk_prefix;
  r.set_off = p->d_set_off;
  r.window = p->d_window;
  r.gamma = p->gamma;
  r.lmbd = lmbd;
  r.lmbd_r = lmbd_r;
  r.w_ref = p->w_ref;
  r.t_sl = tb.sl;
  r.fail_cnt = p->d_fail_cnt;
  r.fail_idx = p->d_fail_idx;
  r.partial = p->d_partial;
  r.w = w;
  r.cost = cost;
  r.w0 = w0;
  r.status = status;
  r.stats = p->d_stats;
  r.tally = p->d_tally;
  r.skip = p->skip;
  r.arrive = p->d_arrive;
}

// with a communicator: `slots` packed send records [S][N] sums | [S][8] stats and the all-gather's
// receive buffer [nranks][S (N + 8)] (grown when the plan or the communicator outgrows them)
int lq_xbufs(lompc_plan* p, int slots, int recv_runs = 1) {
  const int64_t L = p->S * (p->N + LOMPC_SET_STATS);
  int rc;
  if (L * slots > p->cap_xsend) {
    if ((rc = grow(p, &p->d_xsend, L * slots))) return rc;
    p->cap_xsend = L * slots;
  }
  if (L * p->comm->nranks * recv_runs > p->cap_xrecv) {
    if ((rc = grow(p, &p->d_xrecv, L * p->comm->nranks * recv_runs))) return rc;
    p->cap_xrecv = L * p->comm->nranks * recv_runs;
  }
  return LOMPC_OK;
}

void lq_combine(const double* recv, int nranks, int64_t S, int N, double* set_sum_w, double* set_stats, hipStream_t st) {
  const int64_t L = S * (N + LOMPC_SET_STATS);
  const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>((L + 255) / 256, 1024));
  hipLaunchKernelGGL(k_combine, dim3(nb), dim3(256), 0, st, recv, nranks, (int)S, N, set_sum_w, set_stats);
}

// a run's send record (closed on this rank) -> every rank's record -> the rank-ordered combine into
// the caller's set outputs (all ranks bitwise equal)
int lq_exchange(lompc_plan* p, const double* send, double* set_sum_w, double* set_stats, hipStream_t st) {
  const int64_t L = p->S * (p->N + LOMPC_SET_STATS);
  int rc = lq_comm_allgather(p->comm, send, p->d_xrecv, (size_t)L, st);
  if (rc) {
    p->err = p->comm->err;
    return rc;
  }
  if (set_sum_w || set_stats) {
    lq_combine(p->d_xrecv, p->comm->nranks, p->S, p->N, set_sum_w, set_stats, st);
    HIPCHK(p, hipGetLastError());
  }
  return LOMPC_OK;
}

int lq_launch_eval(lompc_plan* p, const double* lmbd, const double* lmbd_r, double* w, double* cost, double* w0,
                   int8_t* status, double* set_sum_w, double* set_stats, const PathTab& tb, hipStream_t st,
                   lompc_ctx* prof_ctx, FinalArgs* defer = nullptr, bool scalar_ok = false) {
  if (defer) defer->N = 0;
  const int N = p->N;
  EvalArgs a;
  FinalArgs r;
  eval_args(p, lmbd, lmbd_r, w, cost, w0, status, tb, a, r);
  const size_t lds = eval_lds(N, p->G, a.cap);
  // with a communicator the sets close into the packed send record [S][N] | [S][8]
  const bool xr = p->comm != nullptr;
  if (xr) {
    const int rc = lq_xbufs(p, 1);
    if (rc) return rc;
  }
  r.set_sum_w = xr ? p->d_xsend : set_sum_w;
  r.set_stats = xr ? p->d_xsend + p->S * N : set_stats;
  // gamma-sorted sets and no per-EV output: per-piece aggregation (k_agg) instead of k_eval
  const bool agg = p->sorted && !w && !cost && !w0 && !status && p->nblk > 0;
  const bool cprof = prof_ctx && prof_ctx->prof;  // lompc_solve_batch: the context's k_eval timing
  // the scalar pass (lompc_plan_run of a LOMPC_PLAN_SCALAR_PASS plan, the rule of lompc_amd.h): no w row and
  // no per-stage sum asked for, so k_scalar evaluates from the coefficient records alone; k_finalize closes
  const bool scalar = scalar_ok && (p->flags & LOMPC_PLAN_SCALAR_PASS) && !(p->flags & LOMPC_PLAN_DIAG_REPAIR) && !w &&
                      !set_sum_w && (cost || w0 || status || set_stats) && !xr && !agg && !defer && !prof_ctx &&
                      p->nblk > 0 && p->scalar_cells >= 1;
  const bool close = !agg && !scalar && (p->close || (p->close_no_w && !w)) && p->nblk > 0;
  int rc = LOMPC_OK;
  if (agg) {  // timed as k_eval
    const AggArgs ga = agg_args(p, lmbd, lmbd_r, tb, r.set_sum_w, r.set_stats, p->skip);
    const int nw = std::min(p->G, (int)LQ_AGG_W);
    rc = timed_launch(p, LOMPC_PLAN_K_EVAL, 1, true, [&](hipEvent_t e0, hipEvent_t e1) {
      hipExtLaunchKernelGGL(agg_kernel(N), dim3((unsigned)p->S), dim3(64 * nw), 0, st, e0, e1, 0, ga);
    });
  } else if (scalar) {
    rc = timed_launch(p, LOMPC_PLAN_K_SCALAR, 1, true, [&](hipEvent_t e0, hipEvent_t e1) {
      hipExtLaunchKernelGGL(k_scalar, dim3((unsigned)p->nblk), dim3(EVAL_EVS), scalar_lds(p->G, p->scalar_cells), st, e0,
                            e1, 0, a, p->scalar_cells);
    });
  } else if (p->nblk > 0) {  // (hand-written: lompc_solve_batch's runs are timed on their context, not the plan)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (cprof ? take_events(prof_ctx->prof_pool, &e0, &e1) : plan_prof_begin(p, LOMPC_PLAN_K_EVAL, &e0, &e1))
      return fail_arg(p, "profiling events");
    if (close) {  // + one workgroup for the sets without EVs
      hipExtLaunchKernelGGL(eval_kernel<true>(N), dim3((unsigned)(p->nblk + (p->n_empty > 0 ? 1 : 0))), dim3(EVAL_EVS), lds, st,
                            e0, e1, 0, a, r);
    } else {
      hipExtLaunchKernelGGL(eval_kernel<false>(N), dim3((unsigned)p->nblk), dim3(EVAL_EVS), lds, st, e0, e1, 0, a, r);
    }
    HIPCHK(p, hipGetLastError());
    if (cprof) {
      prof_ctx->prof_ev.push_back(e0);
      prof_ctx->prof_ev.push_back(e1);
    } else {
      plan_prof_end(p, LOMPC_PLAN_K_EVAL, e0, e1);
    }
  }
  if (rc) return rc;
  if (!close && !agg && defer && !xr && N + NPX <= 64) {  // (one-wave closing: a record fits the wave)
    *defer = r;
    return LOMPC_OK;
  }
  if (!close && !agg &&  // (else the sets were closed inside k_eval / k_agg)
      (rc = timed_launch(p, LOMPC_PLAN_K_FINAL, 1, true, [&](hipEvent_t e0, hipEvent_t e1) {
         hipExtLaunchKernelGGL(k_finalize, dim3((unsigned)p->S), dim3(256), 0, st, e0, e1, 0, r);
       })))
    return rc;
  if (!xr) return LOMPC_OK;
  return lq_exchange(p, p->d_xsend, set_sum_w, set_stats, st);
}

int lq_plan_launch(lompc_plan* p, const double* lmbd, const double* lmbd_r, double* w, double* cost, double* w0,
                   int8_t* status, double* set_sum_w, double* set_stats, hipStream_t st, lompc_ctx* prof_ctx,
                   bool scalar_ok) {
  const PathTab tb = own_tab(p);
  int rc = lq_launch_path(p, lmbd, lmbd_r, tb, st);
  if (rc) return rc;
  return lq_launch_eval(p, lmbd, lmbd_r, w, cost, w0, status, set_sum_w, set_stats, tb, st, prof_ctx, nullptr, scalar_ok);
}

bool lq_loop_fusable(const lompc_plan* p, bool persistent) {  // (S = 2: the loop's sets; ctl holds 2 set counters)
  const int gmax = (persistent && LQ_LOOP_REDUNDANT) ? LQ_LOOP_G2 : LQ_LOOP_G;  // (k_loop_run2: chunked closing)
  return p->sorted && !p->comm && p->nblk > 0 && p->S == 2 && p->G >= 1 && p->G <= gmax;
}

int lq_launch_loop_iter(lompc_plan* p, const double* lmbd, const double* lmbd_r, double* set_sum_w, double* set_stats,
                        const StepArgs& sa, int m, hipStream_t st) {
  return lq_launch_loop(p, lmbd, lmbd_r, set_sum_w, set_stats, sa, m, st, false);
}

// the whole loop as one persistent launch (k_loop_run)
int lq_launch_loop_run(lompc_plan* p, const double* lmbd, const double* lmbd_r, double* set_sum_w, double* set_stats,
                       const StepArgs& sa, hipStream_t st) {
  return lq_launch_loop(p, lmbd, lmbd_r, set_sum_w, set_stats, sa, 0, st, true);
}

int loop_records(lompc_plan* p, hipStream_t st);

int lq_launch_loop(lompc_plan* p, const double* lmbd, const double* lmbd_r, double* set_sum_w, double* set_stats,
                   const StepArgs& sa, int m, hipStream_t st, bool persistent) {
  if (!lq_loop_fusable(p, persistent)) return fail_arg(p, "k_loop_iter: plan not fusable");
  const int N = p->N;
  const int rr = loop_records(p, st);
  if (rr) return rr;
  const PathTab tb = own_tab(p);
  const PathArgs pa = path_args(p, lmbd, lmbd_r, tb);
  const AggArgs ga = agg_args(p, lmbd, lmbd_r, tb, set_sum_w, set_stats, p->skip);
  return timed_launch(p, LOMPC_PLAN_K_PATH, 1, true, [&](hipEvent_t e0, hipEvent_t e1) {  // (timed as k_path)
    if (persistent)  // (S * G one-wave workgroups: all resident at once, whatever else runs)
      hipExtLaunchKernelGGL(loop_run_kernel(N), dim3((unsigned)(p->S * p->G)), dim3(64), 0, st, e0, e1, 0, pa, ga, sa,
                            p->d_aggrec);
    else
      hipExtLaunchKernelGGL(loop_iter_kernel(N), dim3((unsigned)(p->S * p->G)), dim3(64), 0, st, e0, e1, 0, pa, ga, sa,
                            p->d_aggrec, m);
  });
}

// the plan's cell records, grown to its cell count, their zero record zeroed (on the stream)
int loop_records(lompc_plan* p, hipStream_t st) {
  // [cell records | the zero record (k_loop_iter's padding) | (k_loop_run2) the second record buffer]
  const int64_t zoff = p->S * p->G * (int64_t)LQ_AGG_REC;
  const int64_t nrec = (2 * p->S * p->G + 1) * (int64_t)LQ_AGG_REC;
  if (nrec > p->cap_aggrec) {
    const int64_t c = std::max(nrec, p->reserve_B ? (2 * p->S * LQ_RESERVE_CELLS + 1) * (int64_t)LQ_AGG_REC : 0);
    const int rc = grow(p, &p->d_aggrec, c);
    if (rc) return rc;
    p->cap_aggrec = c;
    p->aggrec_zero = -1;
  }
  if (p->aggrec_zero != zoff) {  // (the cell records never reach it: zeroed once per layout)
    HIPCHK(p, hipMemsetAsync(p->d_aggrec + zoff, 0, LQ_AGG_REC * sizeof(double), st));
    p->aggrec_zero = zoff;
  }
  return LOMPC_OK;
}

// ---- the batched persistent loops (lompc_price_loops, lompc_loop.hip; kernel k_loop_runs)
bool lq_loop_runs_ok(const lompc_plan* p) { return LQ_LOOP_REDUNDANT && lq_loop_fusable(p, true); }

size_t lq_loop_job_bytes() { return sizeof(LoopJob); }

// loop j's record at ``slot`` (host): k_loop_run2's arguments for the plan with its price buffer dev_in
// [2*3N | 2 | 2N] — the reference w of both sets read from THAT buffer, not from the pointer the plan
// was created with (concurrent loops of one solver's partitions have different targets)
int lq_loop_job_fill(lompc_plan* p, const double* dev_in, double* set_sum_w, double* set_stats, const StepArgs& sa,
                     void* slot, hipStream_t st) {
  if (!lq_loop_runs_ok(p)) return fail_arg(p, "k_loop_runs: plan not fusable");
  const int rr = loop_records(p, st);
  if (rr) return rr;
  const int N = p->N;
  const double *lmbd = dev_in, *lmbd_r = dev_in + 6 * N, *w_ref = dev_in + 6 * N + 2;
  const PathTab tb = own_tab(p);
  LoopJob job{path_args(p, lmbd, lmbd_r, tb), agg_args(p, lmbd, lmbd_r, tb, set_sum_w, set_stats, p->skip), sa,
              p->d_aggrec};
  job.pa.w_ref = job.ga.w_ref = w_ref;
  memcpy(slot, &job, sizeof(job));
  return LOMPC_OK;
}

typedef void (*LoopRunsKernel)(const LoopJob*, int);
LoopRunsKernel loop_runs_kernel(int N) {
  switch (N) {
    case 12: return k_loop_runs<12>;
    case 16: return k_loop_runs<16>;
    case 24: return k_loop_runs<24>;
    case 48: return k_loop_runs<48>;
    default: return k_loop_runs<0>;
  }
}

// the one-wave workgroups of k_loop_runs<N> resident at once on the plan's device
int lq_loop_runs_places(lompc_plan* p, int* places) {
  int per_cu = 0, dev_cus = 0;
  HIPCHK(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)loop_runs_kernel(p->N), 64, 0));
  HIPCHK(p, hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, p->device));
  *places = per_cu * dev_cus;
  return LOMPC_OK;
}

// n_jobs loops of plans like p (same N and cell count), their records at d_jobs, as one launch
int lq_launch_loop_runs(lompc_plan* p, int n_jobs, const void* d_jobs, hipStream_t st) {
  const int nsg = (int)p->S * p->G;
  hipLaunchKernelGGL(loop_runs_kernel(p->N), dim3((unsigned)(n_jobs * nsg)), dim3(64), 0, st,
                     static_cast<const LoopJob*>(d_jobs), nsg);
  HIPCHK(p, hipGetLastError());
  return LOMPC_OK;
}

void lq_plan_free(lompc_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  (void)hipDeviceSynchronize();
  void* ptrs[] = {p->d_meta,  p->d_stats_own, p->d_window, p->d_partial, p->t_cnt,     p->t_lo,      p->t_ge,         p->t_cf,
                  p->t_ab,    p->t_sl,        p->d_ws,      p->d_errflag,
                  p->d_fail_cnt, p->d_fail_idx, p->d_tally, p->d_wacc, p->d_arrive, p->d_xsend, p->d_xrecv, p->d_loop, p->d_aggrec,
                  p->d_bsum, p->d_P, p->d_pos, p->d_sinfo};
  for (void* x : ptrs)
    if (x) (void)hipFree(x);
  {
    auto& z = p->stp;
    for (int k = 0; k < 2; ++k) {
      void* zs[] = {z.tab[k].cnt, z.tab[k].lo, z.tab[k].ge, z.tab[k].cf, z.tab[k].ab, z.part[k], z.fcnt[k], z.fidx[k]};
      for (void* x : zs)
        if (x) (void)hipFree(x);
    }
    for (void* x : {(void*)z.d_map, (void*)z.sl3, (void*)z.wt.cnt, (void*)z.wt.lo, (void*)z.wt.ge, (void*)z.wt.cf,
                    (void*)z.wt.ab, (void*)z.wt.sl, (void*)z.rpart, (void*)z.rfcnt, (void*)z.rfidx})
      if (x) (void)hipFree(x);
    if (z.h_map) (void)hipHostFree(z.h_map);
  }
  if (p->h_buf) (void)hipHostFree(p->h_buf);

  if (p->h_loop) (void)hipHostFree(p->h_loop);
  if (p->h_dec) (void)hipHostFree(p->h_dec);
  if (p->h_jobs) (void)hipHostFree(p->h_jobs);
  if (p->ev_stage) (void)hipEventDestroy(p->ev_stage);
  for (auto& v : p->prof_ev)
    for (hipEvent_t e : v) (void)hipEventDestroy(e);
  for (hipEvent_t e : p->prof_pool) (void)hipEventDestroy(e);
  delete p;
}

extern "C" {

#ifdef LOMPC_STAMPS
int lompc_debug_wstart(long long* host, int n) {
  if (n > 32768 * 8) n = 32768 * 8;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wstart), sizeof(long long) * n, 0, hipMemcpyDeviceToHost) == hipSuccess
             ? LOMPC_OK
             : LOMPC_ERR_HIP;
}
int lompc_debug_loopstamps(unsigned long long* host, int reset) {  // [64][16] (g_lstamps)
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_lstamps), sizeof(g_lstamps), 0, hipMemcpyDeviceToHost) != hipSuccess)
    return LOMPC_ERR_HIP;
  if (reset) {
    static const unsigned long long z[64 * 16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_lstamps), z, sizeof(z), 0, hipMemcpyHostToDevice) != hipSuccess)
      return LOMPC_ERR_HIP;
  }
  return LOMPC_OK;
}
int lompc_debug_stamps(long long* host, int n) {
  if (n > 65536 * 8) n = 65536 * 8;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), sizeof(long long) * n, 0, hipMemcpyDeviceToHost) == hipSuccess
             ? LOMPC_OK
             : LOMPC_ERR_HIP;
}
#endif

int lompc_plan_create(int n_ctx, lompc_ctx* const* ctxs, const int64_t* sets_per_ctx, int64_t B,
                      const double* gamma, const int64_t* set_offsets, const double* w_ref, int flags, void* stream,
                      lompc_plan** out) {
  if (!out) return LOMPC_ERR_INVALID_ARG;
  *out = nullptr;
  lompc_plan* p = new lompc_plan();
  const int rc = lq_plan_prepare(p, n_ctx, ctxs, sets_per_ctx, B, gamma, set_offsets, w_ref, flags,
                                 (hipStream_t)stream);
  if (rc) {
    if (n_ctx >= 1 && ctxs && ctxs[0]) ctxs[0]->err = p->err;
    lq_plan_free(p);
    return rc;
  }
  *out = p;
  return LOMPC_OK;
}

int lompc_plan_update(lompc_plan* p, int64_t B, const double* gamma, const int64_t* set_offsets,
                      const double* w_ref, void* stream) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  HIPCHK(p, hipSetDevice(p->device));
  int64_t spc[LQ_PLAN_MAX_CTX];
  for (int k = 0, prev = 0; k < p->nctx; ++k) {  // the plan's set counts per context
    const int e = k + 1 < p->nctx ? p->ce.end[k] : (int)p->S;
    spc[k] = e - prev;
    prev = e;
  }
  return lq_plan_prepare(p, p->nctx, p->ctx, spc, B, gamma, set_offsets, w_ref, p->flags, (hipStream_t)stream);
}

int lompc_plan_reserve(lompc_plan* p, int64_t max_B) {
  if (!p || max_B < 0 || max_B >= (1ll << 31) - EVAL_MAXB) return LOMPC_ERR_INVALID_ARG;
  p->reserve_B = max_B;
  return LOMPC_OK;
}

}  // extern "C"

// the message for QPs reported failed by a gamma-sorted plan: a set whose gamma is not ascending
// (k_agg reports all its EVs failed) says so instead of "no certified optimum" (synchronises `st`)
const char* lq_failed_text(lompc_plan* p, hipStream_t st) {
  const char* none = "LoMPC QPs without a certified optimum";
  if (!p->sorted || !p->d_sinfo || p->S < 1) return none;
  std::vector<int4> si((size_t)p->S);
  if (hipMemcpyAsync(si.data(), p->d_sinfo, si.size() * sizeof(int4), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return none;
  for (const int4& x : si)
    if (x.y == 0) return "LOMPC_PLAN_SORTED_GAMMA: a set's valid gamma is not ascending (all its EVs reported failed)";
  return none;
}

// The host form of lompc_price_loop (device_loop = 0): per iteration one plan run, one D2H copy and a
// stream sync, the convergence test and lompc_price_step on the host.  Arguments checked by the caller.
int lq_price_loop_host(lompc_plan* p, const lompc_price_loop_args* a, double* lmbd, double* w_k, double* dual_cost,
                       double* dec_actual, double* dec_pred, int* iterations, double* errs, hipStream_t st) {
  const int N = a->N, r = a->r, N3 = 3 * N;
  const size_t n_in = (size_t)6 * N + 2 + 2 * N;
  // per-part timing (args->prof): host clock for issue / wait / price step, HIP events for the
  // GPU span of every engine call (H2D copy .. D2H copy)
  double* prof = a->prof;
  hipEvent_t pe[2] = {nullptr, nullptr};
  if (prof) {
    for (hipEvent_t& x : pe) HIPCHK(p, hipEventCreateWithFlags(&x, hipEventDefault));
  }
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int k = 0; k < 2; ++k)
        if (e[k]) (void)hipEventDestroy(e[k]);
    }
  } ev_guard{pe};
  auto now_us = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_start = prof ? now_us() : 0.0;
  // one engine call at prices x: the batch errors and the central solve (price_solver.py:106/:132)
  double e[3] = {0.0, 0.0, 0.0};
  double cost_c = 0.0;
  auto iterate = [&](const double* x) -> int {
    const double t0 = prof ? now_us() : 0.0;
    if (prof) HIPCHK(p, hipEventRecord(pe[0], st));
    double* h = a->host_in;
    memcpy(h, x, N3 * sizeof(double));
    memcpy(h + N3, x, N3 * sizeof(double));
    h[2 * N3] = h[2 * N3 + 1] = a->lmbd_r;
    memcpy(h + 2 * N3 + 2, a->w_ref, N * sizeof(double));
    memcpy(h + 2 * N3 + 2 + N, a->w_ref, N * sizeof(double));
    HIPCHK(p, hipMemcpyAsync(a->dev_in, h, n_in * sizeof(double), hipMemcpyHostToDevice, st));
    const int rc = lq_plan_launch(p, a->dev_in, a->dev_in + 2 * N3, nullptr, nullptr, nullptr, nullptr,
                                  const_cast<double*>(a->dev_sw), const_cast<double*>(a->dev_st), st, nullptr);
    if (rc) return rc;
    if (a->dev_sw != a->host_sw)  // (pinned outputs written by the kernel itself need no copy)
      HIPCHK(p, hipMemcpyAsync(a->host_sw, a->dev_sw, 2 * N * sizeof(double), hipMemcpyDeviceToHost, st));
    if (a->dev_st != a->host_st)
      HIPCHK(p, hipMemcpyAsync(a->host_st, a->dev_st, 2 * LOMPC_SET_STATS * sizeof(double), hipMemcpyDeviceToHost,
                               st));
    double t1 = 0.0;
    if (prof) {
      HIPCHK(p, hipEventRecord(pe[1], st));
      t1 = now_us();
    }
    HIPCHK(p, hipStreamSynchronize(st));
    if (prof) {
      const double t2 = now_us();
      float ms = 0.f;
      HIPCHK(p, hipEventElapsedTime(&ms, pe[0], pe[1]));
      prof[LOMPC_LOOP_PROF_ITERS] += 1.0;
      prof[LOMPC_LOOP_PROF_ISSUE] += t1 - t0;
      prof[LOMPC_LOOP_PROF_WAIT] += t2 - t1;
      prof[LOMPC_LOOP_PROF_GPU] += 1e3 * ms;
    }
    const double* sw = a->host_sw;
    const double* sst = a->host_st;
    for (int s = 0; s < 2; ++s) {
      if (sst[s * LOMPC_SET_STATS + LOMPC_STAT_N_INVALID] > 0) return fail_arg(p, "gamma outside [0, y_max]");
      if (sst[s * LOMPC_SET_STATS + LOMPC_STAT_N_FAILED] > 0) {
        p->err = lq_failed_text(p, st);
        return LOMPC_ERR_NOT_CONVERGED;
      }
    }
    double qf = 0.0;  // (w_avg - w_ref)' A_bar (w_avg - w_ref)  (price_solver.py:210-214)
    for (int i = 0; i < N; ++i) {
      const double di = sw[i] / a->n_evs - a->w_ref[i];
      double acc = 0.0;
      for (int j = 0; j < N; ++j) acc += a->A_bar[(size_t)i * N + j] * (sw[j] / a->n_evs - a->w_ref[j]);
      qf += di * acc;
    }
    e[0] = sst[LOMPC_STAT_MAX_ERR];
    e[1] = std::fabs(sw[0] / a->n_evs - a->w_ref[0]);
    e[2] = std::sqrt(qf);
    memcpy(w_k, sw + N, N * sizeof(double));
    cost_c = sst[LOMPC_SET_STATS + LOMPC_STAT_SUM_COST];
    return LOMPC_OK;
  };
  // phi(w_ref) (lompc.py:172-177)
  std::vector<double> phi_ref(N3), lm(lmbd, lmbd + N3), lm_new(N3, 0.0);
  const double q_s = 3.0 * a->theta / (4.0 * a->w_max);
  for (int t = 0; t < N; ++t) {
    phi_ref[t] = a->theta * a->w_ref[t];
    phi_ref[N + t] = a->theta * (a->w_max - a->w_ref[t]);
    phi_ref[2 * N + t] = q_s * a->w_ref[t] * a->w_ref[t];
  }
  int rc = iterate(lm.data());
  if (rc) return rc;
  double dc = cost_c;
  int it = 0;
  for (it = 0; it < a->max_iter; ++it) {
    if ((a->tol_avg ? e[2] : e[0]) <= a->tol) break;
    double dec = 0.0;
    int qit = 0;
    const double ts = prof ? now_us() : 0.0;
    rc = lompc_price_step(N, r, a->theta, a->w_max, a->m, a->kappa, a->eps_reg, a->w_ref, w_k, lm.data(),
                          lm_new.data(), &dec, &qit);
    if (prof) prof[LOMPC_LOOP_PROF_STEP] += now_us() - ts;
    if (rc) {
      p->err = "price-gradient QP: no certified optimum";
      return rc;
    }
    rc = iterate(lm_new.data());
    if (rc) return rc;
    double dterm = 0.0;  // (lmbd_k - lmbd_k_new) @ phi(w_ref): the reference's two arrays alias
    if (it == 0)         // after the first iteration (lmbd_k = lmbd_k_new), so the term is 0 then
      for (int i = 0; i < N3; ++i) dterm += (lm[i] - lm_new[i]) * phi_ref[i];
    if (dec_actual) dec_actual[it] = cost_c - dc + dterm;
    if (dec_pred) dec_pred[it] = dec;
    dc = cost_c;
    lm = lm_new;
  }
  *iterations = it;  // steps taken (= the reference's `iter` unless the cap was hit: then max_iter)
  if (prof) {
    const double wall = now_us() - t_start;
    prof[LOMPC_LOOP_PROF_WALL] += wall;
    // the rest of the loop's host time: convergence test, A_bar metric, copies into the staging
    prof[LOMPC_LOOP_PROF_HOST] = prof[LOMPC_LOOP_PROF_WALL] - prof[LOMPC_LOOP_PROF_ISSUE] -
                                 prof[LOMPC_LOOP_PROF_WAIT] - prof[LOMPC_LOOP_PROF_STEP];
  }
  memcpy(lmbd, lm.data(), N3 * sizeof(double));
  if (dual_cost) *dual_cost = dc;
  if (errs) memcpy(errs, e, sizeof(e));
  return LOMPC_OK;
}

// The stepped form's block map, tables and records (once per prepare).  The path takes np_wg of the
// k_step workgroup slots for the whole launch, so the evaluation blocks are sized to fill the rest once
// (or a whole number of times for big batches).
int stepped_setup(lompc_plan* p, hipStream_t st, bool wide) {
  auto& z = p->stp;
  const int N = p->N;
  const int64_t S = p->S, G = p->G, ncell = S * G, B = p->B;
  const int cap = p->cap;
  const int64_t okey = (int64_t)N * 4096 + G;
  if (z.occ_key != okey) {
    HIPCHK(p, hipOccupancyMaxActiveBlocksPerMultiprocessor(&z.occ, step_kernel(N), EVAL_EVS, eval_lds(N, p->G, cap)));
    z.occ = std::max(z.occ, 1);
    z.occ_key = okey;
  }
  const int64_t maxb = EVAL_MAXB;  // EVs per block at most
  z.np_wg = wide ? 0 : (int)((ncell + LQ_STEP_CELLS - 1) / LQ_STEP_CELLS);  // (wide: the paths have their own launch)
  const int64_t slots = (int64_t)p->n_cu * z.occ;
  const int64_t free1 = std::max<int64_t>(slots - z.np_wg, slots / 2);  // the first round, beside the path
  const int64_t rounds = std::max<int64_t>(1, (10 * B + 9ll * slots * maxb - 1) / (9ll * slots * maxb));
  const int64_t target = free1 + (rounds - 1) * slots;
  std::vector<int64_t> off(S + 1);
  {  // the set offsets from the prepared map (host copy kept in the pinned metadata)
    const int64_t* hoff = reinterpret_cast<const int64_t*>(p->h_buf + p->h_off_at);
    for (int64_t s = 0; s <= S; ++s) off[s] = hoff[s];
  }
  // the block map: (set, first EV, end EV) per k_evals / k_step workgroup, and each set's first block
  // (the wide form's: one dispatch round, weighted as lq_plan_prepare's — the same map, so the same bits)
  std::vector<int4> blks;
  std::vector<int> pre;
  block_map(off.data(), S, B, maxb, target, p->n_cu, wide && rounds == 1, blks, pre);
  int64_t nblk = (int64_t)blks.size();
  const size_t o_pre = ((size_t)nblk * sizeof(int4) + 15) & ~(size_t)15;
  const size_t bytes = o_pre + (size_t)(S + 1) * sizeof(int);
  int rc;
  if ((int64_t)bytes > z.cap_map) {
    if (z.h_map) HIPCHK(p, hipHostFree(z.h_map));
    z.h_map = nullptr;
    HIPCHK(p, hipHostMalloc((void**)&z.h_map, bytes, hipHostMallocDefault));
    if ((rc = grow(p, &z.d_map, bytes))) return rc;
    z.cap_map = (int64_t)bytes;
  }
  HIPCHK(p, hipStreamSynchronize(st));  // (the pinned map may still feed an earlier copy)
  memcpy(z.h_map, blks.data(), (size_t)nblk * sizeof(int4));
  memcpy(z.h_map + o_pre, pre.data(), (size_t)(S + 1) * sizeof(int));
  HIPCHK(p, hipMemcpyAsync(z.d_map, z.h_map, bytes, hipMemcpyHostToDevice, st));
  z.nblk = (int)nblk;
  if (ncell > z.cap_cells) {
    for (int k = 0; k < 2; ++k) {
      auto& t = z.tab[k];
      if ((rc = grow(p, &t.cnt, ncell)) || (rc = grow(p, &t.lo, ncell)) || (rc = grow(p, &t.ge, ncell * LQ_PPL)) ||
          (rc = grow(p, &t.cf, ncell * LQ_PPL * 8)) || (rc = grow(p, &t.ab, ncell * LQ_PPL * N)))
        return rc;
    }
    if ((rc = grow(p, &z.sl3, 3 * (size_t)ncell * 64))) return rc;
    z.cap_cells = ncell;
  }
  if (nblk > z.cap_blk) {
    for (int k = 0; k < 2; ++k)
      if ((rc = grow(p, &z.part[k], (size_t)nblk * (N + NPX))) || (rc = grow(p, &z.fcnt[k], (size_t)nblk * EVAL_WAVES)) ||
          (rc = grow(p, &z.fidx[k], (size_t)nblk * EVAL_MAXB)))
        return rc;
    z.cap_blk = nblk;
  }
  z.ok = true;
  z.wide = wide;
  return LOMPC_OK;
}

#ifndef LQ_WIDE_RUNS
#define LQ_WIDE_RUNS 64                 // wide form: runs per path launch (its table ring: wide_slots; 64: 13.96
                                        // vs 14.32 us per step over 64 steps with 32 — the paths' launch tail amortised)
#endif
#define LQ_WIDE_BYTES (1ll << 30)        // wide form: the table ring's memory at most
#ifndef LQ_WIDE_TAIL_PATHS
#define LQ_WIDE_TAIL_PATHS 1            // wide form: group g + 1's paths behind group g's evaluations in ONE launch
                                        // (k_evals_tail; 0: a k_paths launch before every group's k_evals)
#endif

// The wide form's runs per path launch for K runs: bounded by the table ring's memory
// (LQ_WIDE_BYTES) and the grid (fit: the most the plan allows; < 1: the plan is too big for two slots)
int64_t wide_fit(const lompc_plan* p) {
  const int64_t ncell = p->S * p->G;
  const int64_t cell_bytes = LQ_PPL * (16 * (int64_t)p->N + 8 * 8 + 8) + 4 + 8 + 64;
  return std::min<int64_t>(LQ_WIDE_BYTES / (ncell * cell_bytes), INT32_MAX / 64 / ncell) - 1;
}

// The ring's slots for groups of grp runs: 2 grp where the plan allows them (wide_fit + 1 slots at most) — TWO
// groups at once, so that group g + 1's paths can be written while group g is evaluated (k_evals_tail): runs
// g grp .. (g + 2) grp - 1 are 2 grp consecutive j, so their slots j % (2 grp) never collide, and group g + 2's
// paths rewrite group g's slots only after group g has closed.  Else grp + 1 (one group and the next run).
int64_t wide_slots(const lompc_plan* p, int64_t grp) {
  return LQ_WIDE_TAIL_PATHS && 2 * grp <= wide_fit(p) + 1 ? 2 * grp : grp + 1;
}

// the wide form's table ring, sized for the largest group the plan allows whatever this call's K (a
// later call with more runs must not reallocate — hipMalloc / hipFree synchronise the device)
int wide_ring(lompc_plan* p, hipStream_t st) {
  auto& z = p->stp;
  int rc;
  const int N = p->N;
  const int64_t ncell = p->S * p->G;
  const int64_t ring = wide_slots(p, std::min<int64_t>(LQ_WIDE_RUNS, wide_fit(p))) * ncell;
  if (ring > z.cap_wt) {
    auto& t = z.wt;
    const int64_t c = ring;
    if ((rc = grow(p, &t.cnt, c)) || (rc = grow(p, &t.lo, c)) || (rc = grow(p, &t.ge, c * LQ_PPL)) ||
        (rc = grow(p, &t.cf, c * LQ_PPL * 8)) || (rc = grow(p, &t.ab, c * LQ_PPL * N)) || (rc = grow(p, &t.sl, c * 64)))
      return rc;
    // every slot written once now, in the call that sizes the ring (a plan's first wide call: the
    // warmup), so a later call's first use of a slot meets no cold page translations
    HIPCHK(p, hipMemsetAsync(t.ge, 0, (size_t)c * LQ_PPL * sizeof(*t.ge), st));
    HIPCHK(p, hipMemsetAsync(t.cf, 0, (size_t)c * LQ_PPL * 8 * sizeof(*t.cf), st));
    HIPCHK(p, hipMemsetAsync(t.ab, 0, (size_t)c * LQ_PPL * N * sizeof(*t.ab), st));
    HIPCHK(p, hipMemsetAsync(t.sl, 0, (size_t)c * 64 * sizeof(*t.sl), st));
    z.cap_wt = c;
  }
  return LOMPC_OK;
}

// ---------------------------------------------------------------- lompc_plan_run_steps: K independent runs
// Outputs, in every schedule below: run j reads the prices lm(j), lr(j) and writes its set outputs at the
// per-run strides; its per-EV outputs at w + j ev_stride N (cost, w0, status + j ev_stride).  With
// ev_stride = 0 every run writes the same rows and only the LAST run's closing writes per-EV outputs (an
// earlier closing may share its launch with a later run's evaluation, whose rows must win).
namespace {

// One lompc_plan_run_steps call as every schedule takes it: the caller's arguments, the steps flags
// decoded (span: LOMPC_STEPS_SPAN_EVENTS, split: LOMPC_STEPS_PER_KERNEL) and the entry point's decisions
// (wide: the plan takes the wide forms; scalar: the call takes the wide scalar form).
struct StepsCall {
  const double* lmbd;
  int64_t lmbd_stride;
  const double* lmbd_r;
  int64_t lmbd_r_stride;
  int K, profile_every;
  bool span, split, wide, scalar;
  double *w, *cost, *w0;
  int8_t* status;
  int64_t ev_stride;
  double* set_sum_w;
  int64_t sw_stride;
  double* set_stats;
  int64_t st_stride;
  hipStream_t st;
  const double* lm(int j) const { return lmbd + (size_t)j * lmbd_stride; }
  const double* lr(int j) const { return lmbd_r + (size_t)j * lmbd_r_stride; }
  double* sw_of(int j) const { return set_sum_w ? set_sum_w + (size_t)j * sw_stride : nullptr; }
  double* st_of(int j) const { return set_stats ? set_stats + (size_t)j * st_stride : nullptr; }
  // run j's part of the per-EV output x of `width` values per EV (a null output stays null)
  template <typename T>
  T* ev_of(T* x, int j, int width = 1) const {
    return x ? x + (size_t)j * ev_stride * width : nullptr;
  }
};

// the wide forms' runs per path launch for a call of K runs (< 1: the plan is too big for two ring slots)
int wide_group(const lompc_plan* p, int K) { return (int)std::min<int64_t>({(int64_t)K, LQ_WIDE_RUNS, wide_fit(p)}); }

// What the k_evals and k_step schedules need before their first launch, in this order: the stepped state
// (block map, tables, records) of the plan's kind, a communicator's two send slots, the wide table ring.
int steps_setup(lompc_plan* p, bool wide, hipStream_t st) {
  auto& z = p->stp;
  int rc;
  if ((!z.ok || z.wide != wide) && (rc = stepped_setup(p, st, wide))) return rc;
  if (p->comm && (rc = lq_xbufs(p, 2))) return rc;
  return wide ? wide_ring(p, st) : LOMPC_OK;
}

// the stepped state's block map and one slot of its records in place of the plan's own (eval_args')
void bind_stepped(const lompc_plan::Stepped& z, double* part, int* fcnt, int* fidx, EvalArgs& a, FinalArgs& r) {
  a.blk = reinterpret_cast<const int4*>(z.d_map);
  a.nblk = z.nblk;
  a.partial = part;
  r.partial = part;
  a.fail_cnt = fcnt;
  r.fail_cnt = fcnt;
  a.fail_idx = fidx;
  r.fail_idx = fidx;
  r.blk_prefix = reinterpret_cast<const int*>(z.d_map + (((size_t)z.nblk * sizeof(int4) + 15) & ~(size_t)15));
}

// k_paths: the paths of runs g0 .. g0 + n - 1 into the table ring, run j in slot j % slots; one K_PATH
// pair read as `launches`
int launch_paths(lompc_plan* p, const StepsCall& c, int g0, int n, int slots, int launches = 1) {
  const PathArgs pw = path_args(p, c.lmbd, c.lmbd_r, p->stp.wt);
  const int64_t ncell = p->S * p->G;
  return timed_launch(p, LOMPC_PLAN_K_PATH, launches, true, [&](hipEvent_t e0, hipEvent_t e1) {
    hipExtLaunchKernelGGL(paths_kernel(p->N), dim3((unsigned)(n * ncell)), dim3(64), 0, c.st, e0, e1, 0, pw, c.lmbd_stride,
                          c.lmbd_r_stride, g0, slots);
  });
}

// With a communicator, behind the closings of runs g0 .. g0 + n - 1 into their contiguous send records: ONE
// all-gather of the n records and one rank-ordered combine into the caller's set outputs.
int exchange_runs(lompc_plan* p, const StepsCall& c, int g0, int n) {
  const int64_t tot = (int64_t)n * p->S * (p->N + LOMPC_SET_STATS);
  if (const int rc = lq_comm_allgather(p->comm, p->d_xsend, p->d_xrecv, (size_t)tot, c.st)) {
    p->err = p->comm->err;
    return rc;
  }
  if (c.set_sum_w || c.set_stats) {
    const CombineRunsArgs ca{p->d_xrecv, p->comm->nranks, n, (int)p->S, p->N, g0, c.K - 1, c.set_sum_w, c.set_stats,
                             c.sw_stride, c.st_stride};
    hipLaunchKernelGGL(k_combine_runs, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((tot + 255) / 256, 1024))),
                       dim3(256), 0, c.st, ca);
    HIPCHK(p, hipGetLastError());
  }
  return LOMPC_OK;
}

// The batched wide form (plans without warm starts: every run's path depends on its own prices only).  Per
// group of n <= grp runs THREE launches: k_paths (the n paths into the table ring, run j in slot j % slots),
// k_evals (the n evaluations, each workgroup through its block of every run, into the group's record slots
// j - g0) and k_closes (the n x S closings); with a communicator the group's closings fill contiguous send
// records and ONE all-gather and combine follow.  The runs are independent, so the group size changes no bits.
// * tail (LQ_WIDE_TAIL_PATHS): with a second group and a ring that holds two, only group 0 takes a k_paths
//   launch; group g + 1's paths ride behind group g's evaluations in ONE k_evals_tail launch, counted as a
//   K_PATH launch with its time inside the K_EVAL pair, and in z.tail_launches.
// * scalar (LOMPC_STEPS_SCALAR_PASS, the rule of lompc_amd.h): k_scalars instead of k_evals, one workgroup
//   per (run, block) on the same block map and record slots, timed as K_SCALAR; every launch of the form
//   is read as its runs, and no launch is fused.
// * split (LOMPC_STEPS_PER_KERNEL; the entry point sends it here only without w, and for the scalar form):
//   one run per group, so one part per launch.  Runs without w sum the certified pieces instead of rows, so
//   only these kernels give them the wide form's bits.
// Events: k_paths one K_PATH pair; the evaluation one K_EVAL (K_SCALAR) pair read as n launches — with span
// only the first group's —; k_closes one K_FINAL pair read as n.
int lq_steps_wide(lompc_plan* p, const StepsCall& c) {
  auto& z = p->stp;
  int rc;
  const int N = p->N, K = c.K, Kc = wide_group(p, K);
  const int64_t ncell = p->S * p->G, L = p->S * (N + LOMPC_SET_STATS);
  const bool xr = p->comm != nullptr;
  if ((rc = steps_setup(p, true, c.st))) return rc;
  // record slots x blocks, bounded like the table ring: a run's slot holds every block's record, its
  // re-solve counts and its re-solve list (EVAL_MAXB indices per block), so a batch of many blocks
  // takes smaller groups instead of gigabytes of mostly empty lists
  const int64_t rec_run = (int64_t)z.nblk * ((N + NPX) * 8 + EVAL_WAVES * 4 + EVAL_MAXB * 4);
  const int64_t kr =
      std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(LQ_WIDE_RUNS, wide_fit(p)), LQ_WIDE_BYTES / rec_run));
  const int64_t need = kr * z.nblk;
  if (need > z.cap_rrec) {
    if ((rc = grow(p, &z.rpart, need * (N + NPX))) || (rc = grow(p, &z.rfcnt, need * EVAL_WAVES)) ||
        (rc = grow(p, &z.rfidx, need * EVAL_MAXB)))
      return rc;
    // (touched once here, as the table ring)
    HIPCHK(p, hipMemsetAsync(z.rpart, 0, (size_t)need * (N + NPX) * sizeof(*z.rpart), c.st));
    HIPCHK(p, hipMemsetAsync(z.rfcnt, 0, (size_t)need * EVAL_WAVES * sizeof(*z.rfcnt), c.st));
    HIPCHK(p, hipMemsetAsync(z.rfidx, 0, (size_t)need * EVAL_MAXB * sizeof(*z.rfidx), c.st));
    z.cap_rrec = need;
  }
  if (xr && (rc = lq_xbufs(p, Kc, Kc))) return rc;
  // run 0's arguments on ring slot 0 and record slot 0: the kernels offset them per run
  EvalArgs ea;
  FinalArgs ff;
  eval_args(p, c.lmbd, c.lmbd_r, c.w, c.cost, c.w0, c.status, z.wt, ea, ff);
  ea.piece_sums = c.w ? 0 : 1;  // (no rows to store: the per-stage sums from the piece aggregates)
  bind_stepped(z, z.rpart, z.rfcnt, z.rfidx, ea, ff);
  ff.set_sum_w = xr ? p->d_xsend : c.set_sum_w;
  ff.set_stats = xr ? p->d_xsend + p->S * N : c.set_stats;
  const int grp = c.split ? 1 : (int)std::min<int64_t>(Kc, kr);
  // (the ring is sized for the plan's largest group, which a smaller group's two may still exceed)
  const bool tail = LQ_WIDE_TAIL_PATHS && !c.split && !c.scalar && K > grp && p->G % LQ_STEP_CELLS == 0 &&
                    wide_slots(p, grp) == 2 * (int64_t)grp && 2 * (int64_t)grp * ncell <= z.cap_wt;
  const int slots = tail ? 2 * grp : Kc + 1;
  const size_t lds = eval_lds(N, p->G, p->cap);
  const int kk = c.scalar ? LOMPC_PLAN_K_SCALAR : LOMPC_PLAN_K_EVAL;
  for (int g0 = 0; g0 < K; g0 += grp) {
    const int n = std::min(grp, K - g0);
    const int np = tail ? std::max(0, std::min(grp, K - g0 - grp)) : 0;  // the next group's runs, behind this one's
    if ((!tail || g0 == 0) && (rc = launch_paths(p, c, g0, n, slots, c.scalar ? n : 1))) return rc;
    const EvalsArgs x{g0, n, slots, z.nblk, c.lmbd_stride, c.lmbd_r_stride, c.ev_stride, ncell};
    rc = timed_launch(p, kk, n, !c.span || g0 == 0, [&](hipEvent_t e0, hipEvent_t e1) {
      if (c.scalar) {
        hipExtLaunchKernelGGL(k_scalars, dim3((unsigned)(n * z.nblk)), dim3(EVAL_EVS), scalar_lds(p->G, p->scalar_cells),
                              c.st, e0, e1, 0, ea, x, p->scalar_cells, K - 1);
      } else if (np > 0) {
        const PathArgs pw = path_args(p, c.lmbd, c.lmbd_r, z.wt);
        const int64_t npw = (int64_t)((np + LQ_TAIL_RUNS - 1) / LQ_TAIL_RUNS) * (ncell / LQ_STEP_CELLS);
        hipExtLaunchKernelGGL(evals_tail_kernel(N), dim3((unsigned)(z.nblk + npw)), dim3(EVAL_EVS), lds, c.st, e0, e1, 0,
                              ea, x, pw, g0 + grp, np);
        if ((p->prof >> LOMPC_PLAN_K_PATH) & 1) p->prof_n[LOMPC_PLAN_K_PATH] += 1;
        z.tail_launches += 1;
      } else {
        hipExtLaunchKernelGGL(evals_kernel(N), dim3((unsigned)z.nblk), dim3(EVAL_EVS), lds, c.st, e0, e1, 0, ea, x);
      }
    });
    if (rc) return rc;
    const ClosesArgs cl{g0, n, slots, z.nblk, (int)p->S, K - 1, xr ? 1 : 0, c.lmbd_stride, c.lmbd_r_stride, c.ev_stride,
                        xr ? L : c.sw_stride, xr ? L : c.st_stride, ncell};
    rc = timed_launch(p, LOMPC_PLAN_K_FINAL, n, true, [&](hipEvent_t e0, hipEvent_t e1) {
      hipExtLaunchKernelGGL(k_closes, dim3((unsigned)(n * p->S)), dim3(256), 0, c.st, e0, e1, 0, ff, cl);
    });
    if (rc || (xr && (rc = exchange_runs(p, c, g0, n)))) return rc;
  }
  return LOMPC_OK;
}

// The k_step loop: one launch per run that carries parts of consecutive runs.  Two plan kinds share it:
// * stepped (warm-started plans: run j + 1's path starts from run j's working sets): launch 0 = run 0's
//   path; launch k (1 <= k <= K) = k_step(run k's path (k < K), run k - 1's evaluation, run k - 2's closing
//   (k >= 2)); launch K + 1 = run K - 1's closing.  Run j uses path table j % 2, records j % 2 and
//   cell-start working sets j % 3 (a closing re-solves from run j's while run j + 2's path writes).
// * wide with split and w (LOMPC_STEPS_PER_KERNEL's reference for the batched form with rows): the paths of
//   up to Kc runs in ONE k_paths launch before the first launch that needs them, run j in ring slot
//   j % (Kc + 1); launch k (0 <= k <= K) = k_step(run k's evaluation (k < K), run k - 1's closing (k >= 1)),
//   records j % 2.
// split: every launch issued as one launch per part (path / evaluation / closing), in that order — the same
// kernel on the same arguments without the overlap, so the same bits.  With a communicator, run j's closing
// fills send slot j % 2 and its all-gather + combine follow the launch that carried it (one per run).
// Events (K_EVAL): the steady launches 1 .. K - 1 (split: their evaluation part), every profile_every-th of
// them when sampled; span: ONE pair from the first steady launch to the last steady one of the first path
// group (stepped: of the call), read as that many launches.  k_paths launches carry a K_PATH pair each.
int lq_steps_kstep(lompc_plan* p, const StepsCall& c) {
  auto& z = p->stp;
  int rc;
  const int N = p->N, K = c.K, Kc = wide_group(p, K);
  const bool wide = c.wide, xr = p->comm != nullptr;
  const int64_t ncell = p->S * p->G, L = p->S * (N + LOMPC_SET_STATS);
  const int slots = Kc + 1;  // (wide) a path group and the run before it
  if ((rc = steps_setup(p, wide, c.st))) return rc;
  auto tab = [&](int j) {
    PathTab t;
    if (wide) {  // ring slot j % slots
      const int64_t o = (int64_t)(j % slots) * ncell;
      t.cnt = z.wt.cnt + o;
      t.lo = z.wt.lo + o;
      t.ge = z.wt.ge + o * LQ_PPL;
      t.cf = z.wt.cf + o * LQ_PPL * 8;
      t.ab = z.wt.ab + o * LQ_PPL * N;
      t.sl = z.wt.sl + o * 64;
    } else {
      t = z.tab[j & 1];
      t.sl = z.sl3 + (size_t)(j % 3) * ncell * 64;
    }
    return t;
  };
  auto xsend = [&](int j) { return p->d_xsend + (size_t)(j & 1) * L; };
  auto args = [&](int j, EvalArgs& a, FinalArgs& r) {
    eval_args(p, c.lm(j), c.lr(j), c.ev_of(c.w, j, N), c.ev_of(c.cost, j), c.ev_of(c.w0, j), c.ev_of(c.status, j), tab(j),
              a, r);
    bind_stepped(z, z.part[j & 1], z.fcnt[j & 1], z.fidx[j & 1], a, r);
    r.set_sum_w = xr ? xsend(j) : c.sw_of(j);
    r.set_stats = xr ? xsend(j) + p->S * N : c.st_of(j);
    if (c.ev_stride == 0 && j != K - 1) {  // (its re-solved rows would race a later evaluation's)
      r.w = r.cost = r.w0 = nullptr;
      r.status = nullptr;
    }
  };
  const size_t lds = eval_lds(N, p->G, p->cap);
  const StepKernel kern = step_kernel(N);
  const int s_first = 1, s_last = wide ? Kc - 1 : K - 1;  // the steady launches the span events cover
  hipEvent_t span0 = nullptr, span1 = nullptr;
  if (c.span && s_last >= s_first && plan_prof_begin(p, LOMPC_PLAN_K_EVAL, &span0, &span1))
    return fail_arg(p, "profiling events");
  // one k_step launch of (npw path, ne evaluation, nf closing workgroups); prof: its own event pair (else it
  // starts or ends the span, or carries no event)
  auto launch = [&](const PathArgs& pa, const EvalArgs& ea, const FinalArgs& ff, int npw, int ne, int nf, bool prof,
                    hipEvent_t s0, hipEvent_t s1) -> int {
    if (npw + ne + nf == 0) return LOMPC_OK;
    hipEvent_t e0 = s0, e1 = s1;
    if (prof && plan_prof_begin(p, LOMPC_PLAN_K_EVAL, &e0, &e1)) return fail_arg(p, "profiling events");
    hipExtLaunchKernelGGL(kern, dim3((unsigned)(npw + ne + nf)), dim3(EVAL_EVS), lds, c.st, e0, e1, 0, pa, ea, ff, npw, ne,
                          nf);
    HIPCHK(p, hipGetLastError());
    if (prof) plan_prof_end(p, LOMPC_PLAN_K_EVAL, e0, e1);
    return LOMPC_OK;
  };
  int paths_to = 0;  // wide: runs whose paths are launched
  const int last = wide ? K : K + 1;
  for (int k = 0; k <= last; ++k) {
    PathArgs pa{};
    EvalArgs ea{}, unused_e;
    FinalArgs ff{}, unused_f;
    int npw = 0, ne = 0, nf = 0;
    const int ev_run = wide ? k : k - 1, fin_run = ev_run - 1;  // the runs this launch evaluates and closes
    if (wide && k < K && k >= paths_to) {  // the next group's paths, one launch
      const int n = std::min(Kc, K - k);
      if ((rc = launch_paths(p, c, k, n, slots))) return rc;
      paths_to = k + n;
    }
    if (!wide && k < K) {
      pa = path_args(p, c.lm(k), c.lr(k), tab(k));
      npw = z.np_wg;
    }
    if (ev_run >= 0 && ev_run < K) {
      args(ev_run, ea, unused_f);
      ne = z.nblk;
    }
    if (fin_run >= 0) {
      args(fin_run, unused_e, ff);
      nf = (int)p->S;
    }
    int npw_l = npw;
#ifdef LQ_STEP_DIAG
    // diagnostic builds only (-DLQ_STEP_DIAG=1 / 2, timing of the launch's parts): from launch 3 on,
    // 1 drops the path workgroups, 2 the evaluation and closing workgroups; outputs are not the runs'
    if (k >= 3 && k < K) {
      if (LQ_STEP_DIAG == 1) npw_l = 0;
      if (LQ_STEP_DIAG == 2) ne = nf = 0;
    }
#endif
    // the steady launches carry the events: sampled, or one pair around all of them
    const bool steady = k >= 1 && k <= K - 1;
    const bool prof = !c.span && steady && (c.profile_every <= 0 || (k - 1) % c.profile_every == 0);
    const hipEvent_t s0 = (span0 && k == s_first) ? span0 : nullptr, s1 = (span0 && k == s_last) ? span1 : nullptr;
    if (c.split) {  // the same parts, one launch each (no overlap)
      if ((rc = launch(pa, ea, ff, npw_l, 0, 0, false, nullptr, nullptr)) ||
          (rc = launch(pa, ea, ff, 0, ne, 0, prof, s0, s1)) || (rc = launch(pa, ea, ff, 0, 0, nf, false, nullptr, nullptr)))
        return rc;
    } else if ((rc = launch(pa, ea, ff, npw_l, ne, nf, prof, s0, s1))) {
      return rc;
    }
    if (s1) plan_prof_end(p, LOMPC_PLAN_K_EVAL, span0, span1, s_last - s_first + 1);
    if (xr && nf && (rc = lq_exchange(p, xsend(fin_run), c.sw_of(fin_run), c.st_of(fin_run), c.st))) return rc;
  }
  return LOMPC_OK;
}

// Reductions-only runs over gamma-sorted sets (k_agg plans), wide: per group of up to Kc runs TWO
// launches — k_paths (the group's paths into the table ring, run j in slot j % (Kc + 1)) and k_aggs (one
// workgroup per (run, set): k_agg's per-piece aggregation on run j's tables).  The same kernels'
// arithmetic as one k_path + k_agg per run (lq_steps_single, LOMPC_STEPS_PER_KERNEL), so the same bits.
// With a communicator the group's closings fill its contiguous send records: ONE all-gather and one
// combine per group.  Events: k_paths one K_PATH pair; the k_aggs launch one K_EVAL pair read as n
// launches, with span only the first group's.
int lq_steps_aggs(lompc_plan* p, const StepsCall& c) {
  int rc;
  const int N = p->N, K = c.K, Kc = wide_group(p, K);
  const int64_t L = p->S * (N + LOMPC_SET_STATS);
  const int slots = Kc + 1;
  if ((rc = wide_ring(p, c.st))) return rc;
  const bool xr = p->comm != nullptr;
  if (xr && (rc = lq_xbufs(p, Kc, Kc))) return rc;
  const AggArgs ga = agg_args(p, c.lmbd, c.lmbd_r, p->stp.wt, xr ? p->d_xsend : c.set_sum_w,
                              xr ? p->d_xsend + p->S * N : c.set_stats, nullptr);
  const int nw = std::min(p->G, (int)LQ_AGG_W);
  for (int g0 = 0; g0 < K; g0 += Kc) {
    const int n = std::min(Kc, K - g0);
    if ((rc = launch_paths(p, c, g0, n, slots))) return rc;
    const AggsArgs x{g0, slots, K - 1, xr ? 1 : 0, c.lmbd_stride, c.lmbd_r_stride, xr ? L : c.sw_stride, xr ? L : c.st_stride};
    rc = timed_launch(p, LOMPC_PLAN_K_EVAL, n, !c.span || g0 == 0, [&](hipEvent_t e0, hipEvent_t e1) {
      hipExtLaunchKernelGGL(aggs_kernel(N), dim3((unsigned)(n * p->S)), dim3(64 * nw), 0, c.st, e0, e1, 0, ga, x);
    });
    if (rc || (xr && (rc = exchange_runs(p, c, g0, n)))) return rc;
  }
  return LOMPC_OK;
}

// One k_path_fin + k_eval (k_agg) per run, for the plans no other schedule takes: run k's closing
// (k_finalize) rides in run k + 1's path launch (k_path_fin) where a record fits one wave — else, and with a
// communicator or the sets closed inside k_eval, it follows its run —, and the last run's closes on its
// own, untimed.  The cell-start working sets alternate halves between runs.  Events: every run's k_path
// and k_eval carry their own pairs; sampled (profile_every), only every profile_every-th run's do.
int lq_steps_single(lompc_plan* p, const StepsCall& c) {
  const int mask = p->prof;  // (restored on every exit)
  int rc = LOMPC_OK;
  FinalArgs fin{};
  fin.N = 0;
  for (int k = 0; k < c.K && rc == LOMPC_OK; ++k) {
    if (c.profile_every > 0) p->prof = (k % c.profile_every == 0) ? mask : 0;  // sampled runs carry the events
    const PathTab tb = own_tab(p, k & 1);
    if ((rc = lq_launch_path(p, c.lm(k), c.lr(k), tb, c.st, fin.N ? &fin : nullptr))) break;
    rc = lq_launch_eval(p, c.lm(k), c.lr(k), c.ev_of(c.w, k, p->N), c.ev_of(c.cost, k), c.ev_of(c.w0, k),
                        c.ev_of(c.status, k), c.sw_of(k), c.st_of(k), tb, c.st, nullptr, &fin);
  }
  p->prof = mask;
  if (rc == LOMPC_OK && fin.N) {  // the last run's closing
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)p->S), dim3(256), 0, c.st, fin);
    HIPCHK(p, hipGetLastError());
  }
  return rc;
}

}  // namespace

extern "C" {

int lompc_plan_run(lompc_plan* p, const double* lmbd, const double* lmbd_r, double* w, double* cost, double* w0,
                   int8_t* status, double* set_sum_w, double* set_stats, void* stream) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  HIPCHK(p, hipSetDevice(p->device));
  // (takes the scalar pass of a LOMPC_PLAN_SCALAR_PASS plan; lompc_plan_run_steps only on request: LOMPC_STEPS_SCALAR_PASS)
  return lq_plan_launch(p, lmbd, lmbd_r, w, cost, w0, status, set_sum_w, set_stats, (hipStream_t)stream, nullptr, true);
}

int lompc_plan_run_steps(lompc_plan* p, const double* lmbd, int64_t lmbd_stride, const double* lmbd_r,
                         int64_t lmbd_r_stride, int n_runs, int profile_every, double* w, double* cost, double* w0,
                         int8_t* status, double* set_sum_w, double* set_stats, int64_t set_sum_w_stride,
                         int64_t set_stats_stride, int64_t ev_stride, int steps_flags, void* stream) {
  constexpr int known = LOMPC_STEPS_PER_KERNEL | LOMPC_STEPS_SPAN_EVENTS | LOMPC_STEPS_SCALAR_PASS;
  if (!p || n_runs < 0 || profile_every < 0 || set_sum_w_stride < 0 || set_stats_stride < 0 || ev_stride < 0 ||
      (steps_flags & ~known))
    return LOMPC_ERR_INVALID_ARG;
  if (ev_stride > 0 && ev_stride < p->B) return fail_arg(p, "run_steps: 0 or ev_stride >= B required");
  if ((steps_flags & LOMPC_STEPS_SCALAR_PASS) && !(p->flags & LOMPC_PLAN_SCALAR_PASS))
    return fail_arg(p, "run_steps: LOMPC_STEPS_SCALAR_PASS requires a plan created with LOMPC_PLAN_SCALAR_PASS");
  HIPCHK(p, hipSetDevice(p->device));
  StepsCall c{lmbd, lmbd_stride, lmbd_r, lmbd_r_stride, n_runs, profile_every,
              (steps_flags & LOMPC_STEPS_SPAN_EVENTS) != 0, (steps_flags & LOMPC_STEPS_PER_KERNEL) != 0, false, false,
              w, cost, w0, status, ev_stride, set_sum_w, set_sum_w_stride, set_stats, set_stats_stride,
              (hipStream_t)stream};
  // The schedule of the call, first match first.  Every batched schedule needs runs, a batch with EVs and no
  // device price loop around the plan (its kernels poll the loop's flag); the wide ones a plan without warm
  // starts (every run's path depends on its own prices only) whose table ring holds two runs or more.
  const bool some = n_runs >= 1 && !p->skip && p->nblk > 0;
  c.wide = (p->flags & LOMPC_PLAN_WARM_START) == 0 && wide_fit(p) >= 1;
  const bool per_ev = w || cost || w0 || status;
  const bool agg = p->sorted && !per_ev;  // gamma-sorted sets and no per-EV output: the per-piece aggregation
  // 1. The wide scalar form (LOMPC_STEPS_SCALAR_PASS on a LOMPC_PLAN_SCALAR_PASS plan, the rule of lompc_amd.h):
  //    no w row and no per-stage sum asked for, some other output, no communicator.  A per-call condition that
  //    fails leaves the call exactly as without the flag.
  c.scalar = (steps_flags & LOMPC_STEPS_SCALAR_PASS) && some && c.wide && !(p->flags & LOMPC_PLAN_DIAG_REPAIR) && !w &&
             !set_sum_w && (per_ev || set_stats) && !p->comm && !agg && p->scalar_cells >= 1;
  if (c.scalar) return lq_steps_wide(p, c);
  // 2. Gamma-sorted sets without per-EV output: k_paths + k_aggs per group of runs (per kernel: rule 4, the
  //    same bits).
  if (some && c.wide && agg && !c.split) return lq_steps_aggs(p, c);
  // 3. The k_eval / k_finalize plans (not k_agg, not closed inside k_eval on request) whose cells fill whole
  //    k_step workgroups; runs without w output too (their evaluation then sums what it does not store).
  //    Wide plans take the batched launches — per kernel only without w, where no other kernel gives the
  //    batched form's bits —, warm-started plans and the per-kernel runs with w the k_step loop.
  if (some && !agg && !p->close && p->G % LQ_STEP_CELLS == 0)
    return c.wide && (!c.split || !w) ? lq_steps_wide(p, c) : lq_steps_kstep(p, c);
  // 4. Everything else, n_runs = 0 included: one k_path_fin + k_eval per run.
  return lq_steps_single(p, c);
}

int lompc_plan_run_chain(lompc_plan* p, const double* lmbd0, const double* lmbd_r, const double* w_target, double step,
                         int n_runs, double* lmbd_out, double* w, double* cost, double* w0, int8_t* status,
                         double* set_sum_w, double* set_stats, void* stream) {
  if (!p || n_runs < 0 || !lmbd0 || !lmbd_r || !w_target || !lmbd_out || !set_sum_w || !set_stats ||
      !(step >= 0.0) || !std::isfinite(step))
    return LOMPC_ERR_INVALID_ARG;
  HIPCHK(p, hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  const int N = p->N;
  const size_t L = (size_t)p->S * 3 * N, SN = (size_t)p->S * N, SS = (size_t)p->S * LOMPC_SET_STATS;
  for (int k = 0; k < n_runs; ++k) {
    double* lm = lmbd_out + (size_t)k * L;
    if (k == 0) {
      if (lm != lmbd0) HIPCHK(p, hipMemcpyAsync(lm, lmbd0, L * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else {  // run k's prices from run k - 1's (combined) reductions
      hipLaunchKernelGGL(k_chain_price, dim3((unsigned)p->S), dim3(64 * ((3 * N + 63) / 64)), 0, st, p->d_q, p->ce,
                         p->nctx, N, lm - L, set_sum_w + (k - 1) * SN, set_stats + (k - 1) * SS, w_target, step, lm);
      HIPCHK(p, hipGetLastError());
    }
    const int rc = lq_plan_launch(p, lm, lmbd_r, w, cost, w0, status, set_sum_w + k * SN, set_stats + k * SS, st, nullptr);
    if (rc) return rc;
  }
  return LOMPC_OK;
}

int lompc_plan_status(lompc_plan* p, void* stream, int64_t* n_repaired, int64_t* n_failed, int64_t* n_invalid) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  HIPCHK(p, hipSetDevice(p->device));
  // the sticky tallies of every run since the last call (finalize_set adds each set's counts)
  unsigned long long h[3] = {0, 0, 0};
  int ef = 0;
  HIPCHK(p, hipMemcpyAsync(h, p->d_tally, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(p, hipMemcpyAsync(&ef, p->d_errflag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(p, hipMemsetAsync(p->d_tally, 0, sizeof(h), (hipStream_t)stream));
  HIPCHK(p, hipStreamSynchronize((hipStream_t)stream));
  if (n_repaired) *n_repaired = (int64_t)h[0];
  if (n_failed) *n_failed = (int64_t)h[1];
  if (n_invalid) *n_invalid = (int64_t)h[2];
  if (h[1]) p->err = lq_failed_text(p, (hipStream_t)stream);  // (the caller's exception text)
  if (ef) {
    HIPCHK(p, hipMemsetAsync(p->d_errflag, 0, sizeof(int), (hipStream_t)stream));
    return fail_arg(p, "negative or NaN price parameter (lmbd >= 0, lmbd_r >= 0 required)");
  }
  return LOMPC_OK;
}

int lompc_plan_get_info(const lompc_plan* p, int64_t* B, int64_t* S, int* cells, int* eval_workgroups,
                        int* steps_group) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  if (steps_group) *steps_group = p->stp.ok ? 1 : 0;
  if (B) *B = p->B;
  if (S) *S = p->S;
  if (cells) *cells = p->G;
  if (eval_workgroups) *eval_workgroups = p->nblk;
  return LOMPC_OK;
}

int lompc_plan_get_wide_info(const lompc_plan* p, int64_t* ring_runs, int64_t* tail_launches) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  if (ring_runs) *ring_runs = std::max<int64_t>(0, wide_fit(p) + 1);
  if (tail_launches) *tail_launches = p->stp.tail_launches;
  return LOMPC_OK;
}

int lompc_plan_profile_enable(lompc_plan* p, int kernel_mask) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  HIPCHK(p, hipSetDevice(p->device));
  p->prof = kernel_mask & ((1 << LOMPC_PLAN_KERNELS) - 1);
  while (p->prof && p->prof_pool.size() < 512) {
    hipEvent_t e;
    HIPCHK(p, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    p->prof_pool.push_back(e);
  }
  return LOMPC_OK;
}

int lompc_plan_profile_read(lompc_plan* p, int kernel, double* total_ms, int64_t* launches, int reset) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  if (kernel < 0 || kernel >= LOMPC_PLAN_KERNELS) return fail_arg(p, "profile_read: kernel out of range");
  HIPCHK(p, hipSetDevice(p->device));
  for (int k = 0; k < LOMPC_PLAN_KERNELS; ++k)
    if (plan_events_read(p->prof_ev[k], p->prof_mult[k], p->prof_pool, p->prof_ms[k], p->prof_n[k])) return LOMPC_ERR_HIP;
  if (total_ms) *total_ms = p->prof_ms[kernel];
  if (launches) *launches = p->prof_n[kernel];
  if (reset) {
    p->prof_ms[kernel] = 0.0;
    p->prof_n[kernel] = 0;
  }
  return LOMPC_OK;
}

const char* lompc_plan_last_error(const lompc_plan* p) { return p ? p->err.c_str() : ""; }

int lompc_plan_set_comm(lompc_plan* p, lompc_comm* comm) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  if (comm && comm->device != p->device) return fail_arg(p, "set_comm: the communicator's device differs from the plan's");
  p->comm = comm;
  return LOMPC_OK;
}

int lompc_combine_records(const double* recv, int nranks, int64_t S, int N, double* set_sum_w, double* set_stats,
                          int device, void* stream) {
  if (!recv || nranks < 1 || S < 1 || N < 1 || N > LOMPC_MAX_N || S * (N + LOMPC_SET_STATS) >= (1ll << 31))
    return LOMPC_ERR_INVALID_ARG;
  if (hipSetDevice(device) != hipSuccess) return LOMPC_ERR_HIP;
  lq_combine(recv, nranks, S, N, set_sum_w, set_stats, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? LOMPC_OK : LOMPC_ERR_HIP;
}

int lompc_plan_destroy(lompc_plan* p) {
  lq_plan_free(p);
  return LOMPC_OK;
}

}  // extern "C"

// diagnostics (scripts/, not in the header): synchronous copies of a plan's path table and sorted index
extern "C" int lompc_debug_plan_tables(lompc_plan* p, int* cnt, double* lo, double* ge, int* pos, int* sinfo,
                                       unsigned long long* P) {
  if (!p) return LOMPC_ERR_INVALID_ARG;
  HIPCHK(p, hipDeviceSynchronize());
  const size_t nc = (size_t)p->S * p->G;
  if (cnt) HIPCHK(p, hipMemcpy(cnt, p->t_cnt, nc * sizeof(int), hipMemcpyDeviceToHost));
  if (lo) HIPCHK(p, hipMemcpy(lo, p->t_lo, nc * sizeof(double), hipMemcpyDeviceToHost));
  if (ge) HIPCHK(p, hipMemcpy(ge, p->t_ge, nc * LQ_PPL * sizeof(double), hipMemcpyDeviceToHost));
  if (pos && p->d_pos) HIPCHK(p, hipMemcpy(pos, p->d_pos, (size_t)p->S * (p->aggF + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (sinfo && p->d_sinfo) HIPCHK(p, hipMemcpy(sinfo, p->d_sinfo, (size_t)p->S * sizeof(int4), hipMemcpyDeviceToHost));
  if (P && p->d_P) HIPCHK(p, hipMemcpy(P, p->d_P, (size_t)3 * (p->B + p->S) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return LOMPC_OK;
}
