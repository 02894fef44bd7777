// lompc_plan_eval.hpp — the plan's evaluation side: EvalArgs, the table loads (ld_t), finalize_set and the
// closing / combine / chain kernels, eval_block and the kernels built on it (k_eval, k_step, k_evals,
// k_evals_tail), k_paths, k_closes, with their *_kernel(int N) dispatchers and the tuning macros only they use
// (those the host code shares — EVAL_*, LQ_STEP_CELLS, LQ_PIECE_CAP, LQ_DROP_OFF — are in lompc_plan.hip).
// Plain text of lompc_plan.hip, included by it alone, inside its kernel namespace after lompc_plan_path.hpp.

// ---------------------------------------------------------------- k_eval
struct EvalArgs {
  int S, G, N, want_err;
  const QPConst* qd;
  CtxEnds ce;
  const int4* blk;        // [nblk] (set, first EV, end EV, -): <= EVAL_MAXB EVs of one set
  const int64_t* set_off; // [S+1]
  const double* window;
  const double* gamma;    // caller's [B]
  const double* lmbd;
  const double* lmbd_r;
  const double* w_ref;
  const int* t_cnt;
  const double* t_lo;
  const uint8_t* t_sl;
  const double* t_ge;
  const double* t_cf;
  const double2* t_ab;
  double* w;
  double* cost;
  double* w0;
  int8_t* status;
  double* partial;        // [nblk][N + NPX]
  int* fail_cnt;          // [nblk][EVAL_WAVES]  EVs left for the individual re-solve (k_finalize)
  int* fail_idx;          // [nblk][EVAL_MAXB]   their indices, per wave in row order
  int w_rsrc_ok;          // B*N*8 <= LQ_DROP_OFF: w through a buffer descriptor (offsets from 0)
  int w_bytes;            // B*N*8 when w_rsrc_ok (the descriptor's range)
  int cap;                // pieces staged in LDS (a set with more re-solves the rest individually)
  int nblk;               // workgroups of EVs (close mode: workgroup nblk closes the empty sets)
  const int* skip;        // device-resident price loop: nonzero = the loop has finished, run nothing
  int piece_sums;         // (k_evals, no w output) per-stage sums from per-piece aggregates, no rows
};

// cost / A_bar error / price0 of a QP solved by the whole wave (lane t = w_t), valid on every lane
__device__ __forceinline__ void wave_ev_outputs(const QPConst& q, const lqw::WaveSet& ws, double c0, double kappa,
                                                const double* l0, double lr, double wr, double gamma, double w,
                                                double& cost, double& err, double& price0) {
  const int N = ws.N, lane = ws.lane;
  const bool act = lane < N;
  lqw::Aff<2> h = lqw::Aff<2>::identity();
  if (act) {
    h.B[0] = w;
    h.B[1] = w - wr;
  }
  const lqw::Aff<2> Y = lqw::wave_scan(h, N);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (act) {
    const double y = Y.B[0], ey = Y.B[1];
    v[0] = 0.5 * q.c * y * y - q.c * gamma * y + w * fma(0.5 * ws.d_nat, w, ws.e_nat);
    v[1] = ey * ey;
    v[2] = (w - wr) * (w - wr);
    v[3] = q.ev_small ? 0.0 : lq_pwl(w * q.inv_wmax);
  }
  lqw::wave_totals(v, N);
  const double tw = q.theta * q.w_max;
  cost = v[0] + c0 + tw * tw * v[3];
  err = sqrt(fmax(v[1] + kappa * v[2], 0.0));
  const double w0 = lqw::readlane_d(w, 0);
  price0 = q.theta * (w0 * l0[0] + (q.w_max - w0) * l0[1]) + q.q_scale * w0 * w0 * l0[2] +
           q.theta * q.theta * w0 * w0 * lr;
}

// loads of k_eval's records: plain after a kernel boundary (k_finalize), device-coherent (sc1, past
// any stale L2 line of this XCD) when other workgroups of the same launch wrote them (close mode)
template <bool COH>
__device__ __forceinline__ double ld_t(const double* p) {
  if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool COH>
__device__ __forceinline__ int ld_t(const int* p) {
  if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool COH>
__device__ __forceinline__ double2 ld_t(const double2* p) {
  if constexpr (COH) {
    const double* d = reinterpret_cast<const double*>(p);
    return make_double2(ld_t<true>(d), ld_t<true>(d + 1));
  } else {
    return *p;
  }
}

struct FinalArgs {
  int N, G, want_err;
  unsigned long long* tally;  // [3] plan-wide repaired / failed / invalid since the last status read (or null)
  const int* skip;            // device-resident price loop: nonzero = the loop has finished
  int* arrive;             // [S] k_eval (close mode): arrived workgroups per set, zero between runs
  const QPConst* qd;
  CtxEnds ce;
  const int* blk_prefix;   // [S+1] k_eval workgroups of each set
  const int64_t* set_off;
  const double* window;
  const double* gamma;
  const double* lmbd;
  const double* lmbd_r;
  const double* w_ref;
  const uint8_t* t_sl;
  const int* fail_cnt;
  const int* fail_idx;
  const double* partial;
  double* w;
  double* cost;
  double* w0;
  int8_t* status;
  double* set_sum_w;
  double* set_stats;
  double* stats;
};

constexpr int FIN_W = LOMPC_MAX_N + NPX + 1;

// Closing of set s by one workgroup of NW waves (k_finalize: one 4-wave workgroup per set; k_eval
// in close mode and k_step: 8 waves; k_path_fin: one wave; COH = records read with sc1 loads when
// other workgroups of the same launch wrote them).  The summation order does not depend on NW, so
// every form of a run gives the same bits: records (and re-solve lists) fall into LQ_FIN_CLASSES
// classes by their index mod 4, each class summed in increasing index by one wave, the classes
// combined as ((c0 + c1) + c2) + c3.
// (1) reduction of the set's k_eval records (lane = column);
// (2) if k_eval listed EVs no certified piece covers: the lists of waves (workgroup, wave) are
//     re-solved individually (wave_solve from the working set at their cell's start: fp32 search,
//     fp64 PDAS, primal active set; KKT-certified), their outputs written and added by class.
#define LQ_FIN_CLASSES 4
template <int NW, bool COH>
__device__ __forceinline__ void finalize_set(const FinalArgs& r, const int s, double (*red)[FIN_W], double (*rep)[FIN_W]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int N = r.N, W = N + NPX;
  const int b0 = r.blk_prefix[s], b1 = r.blk_prefix[s + 1];
  constexpr int NC = LQ_FIN_CLASSES;
  for (int cl = wv; cl < NC; cl += NW) {
    for (int c = lane; c < W; c += 64) {
      const bool is_max = c == N + PX_MAX_ERR;
      double acc = 0.0;
      constexpr int U = 8;
      for (int b = b0 + cl; b < b1; b += NC * U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int bb = b + NC * u;
          v[u] = bb < b1 ? ld_t<COH>(r.partial + (size_t)bb * W + c) : 0.0;  // 0: neutral for sums and max of errors >= 0
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = is_max ? fmax(acc, v[u]) : acc + v[u];
      }
      red[cl][c] = acc;
    }
  }
  __syncthreads();
  for (int c = tid; c < W; c += 64 * NW) {
    const bool is_max = c == N + PX_MAX_ERR;
    double v = red[0][c];
#pragma unroll
    for (int k = 1; k < NC; ++k) v = is_max ? fmax(v, red[k][c]) : v + red[k][c];
    red[0][c] = v;
  }
  __syncthreads();
  if (red[0][N + PX_N_FAILED] > 0.0) {  // block-uniform: individual re-solves pending
    const QPConst& q = set_consts(r.qd, r.ce, s);
    lq_tab_init(q);
    const double* __restrict__ L = r.lmbd + (size_t)s * 3 * N;
    const double lr = r.lmbd_r[s];
    lqw::WaveSet ws;
    double l2;
    bool bad;  // (checked by k_path)
    load_set(q, L, lr, N, lane, ws, l2, bad);
    const double c0 = q.theta * q.w_max * lqw::wave_sum(l2, N);
    const double kappa = lr / q.delta;
    const double l0[3] = {L[0], L[N], L[2 * N]};
    const double wr = (r.w_ref && lane < N) ? r.w_ref[(size_t)s * N + lane] : 0.0;
    const double wlo = r.window[2 * s], whi = r.window[2 * s + 1];
    const int G = r.G;
    for (int cl = wv; cl < NC; cl += NW) {
      double acc_w = 0.0, acc_cost = 0.0, acc_p0 = 0.0, acc_err = 0.0;
      int nrep = 0, nfail = 0;
      for (int j = b0 * EVAL_WAVES + cl; j < b1 * EVAL_WAVES; j += NC) {  // (workgroup, wave) lists of class cl
        const int nf = ld_t<COH>(r.fail_cnt + j);
        for (int k = 0; k < nf; ++k) {
          const int i = ld_t<COH>(r.fail_idx + (size_t)(j / EVAL_WAVES) * EVAL_MAXB + 64 * EVAL_PASSES * (j % EVAL_WAVES) + k);
          const double g = r.gamma[i];
          const int c = cell_of(g, wlo, (double)G / (whi - wlo), G);
          int sl = lane < N ? (int)r.t_sl[((size_t)s * G + c) * 64 + lane] : 0;
          double wl = 0.0, rl = 0.0;
          const bool okk = lqw::wave_solve(q, ws, g, sl, wl, rl);
          double co, eo, po;
          wave_ev_outputs(q, ws, c0, kappa, l0, lr, wr, g, wl, co, eo, po);
          if (!r.want_err) eo = 0.0;
          if (r.w && lane < N) r.w[(size_t)i * N + lane] = wl;
          if (lane == 0) {
            if (r.cost) r.cost[i] = co;
            if (r.w0) r.w0[i] = wl;
            if (r.status) r.status[i] = okk ? LOMPC_QP_REPAIRED : LOMPC_QP_FAILED;
          }
          acc_w += lane < N ? wl : 0.0;
          acc_cost += co;
          acc_p0 += po;
          acc_err = fmax(acc_err, eo);
          nrep += okk ? 1 : 0;
          nfail += okk ? 0 : 1;
        }
      }
      if (lane < N) rep[cl][lane] = acc_w;
      if (lane == 0) {
        rep[cl][N + PX_COST] = acc_cost;
        rep[cl][N + PX_PRICE0] = acc_p0;
        rep[cl][N + PX_MAX_ERR] = acc_err;
        rep[cl][N + PX_N_OK] = (double)nrep;
        rep[cl][N + PX_N_REPAIRED] = (double)nrep;
        rep[cl][N + PX_N_FAILED] = (double)nfail;
        rep[cl][N + PX_N_INVALID] = 0.0;
      }
    }
    __syncthreads();
    for (int c = tid; c < W; c += 64 * NW) {
      const bool is_max = c == N + PX_MAX_ERR;
      double v = (c == N + PX_N_FAILED) ? 0.0 : red[0][c];  // pending -> the outcome
#pragma unroll
      for (int k = 0; k < NC; ++k) v = is_max ? fmax(v, rep[k][c]) : v + rep[k][c];
      red[0][c] = v;
    }
    __syncthreads();
  }
  if (tid == 0 && r.tally) {  // sticky plan-wide counters (lompc_plan_status): one atomic per nonzero count
    const double nr = red[0][N + PX_N_REPAIRED], nf = red[0][N + PX_N_FAILED], ni = red[0][N + PX_N_INVALID];
    if (nr > 0.0) __hip_atomic_fetch_add(r.tally + 0, (unsigned long long)nr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nf > 0.0) __hip_atomic_fetch_add(r.tally + 1, (unsigned long long)nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ni > 0.0) __hip_atomic_fetch_add(r.tally + 2, (unsigned long long)ni, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid < N && r.set_sum_w) r.set_sum_w[(size_t)s * N + tid] = red[0][tid];
  if (tid < LOMPC_SET_STATS) {
    double v = 0.0;
    switch (tid) {
      case LOMPC_STAT_COUNT: v = (double)(r.set_off[s + 1] - r.set_off[s]); break;
      case LOMPC_STAT_SUM_W0: v = red[0][0]; break;
      case LOMPC_STAT_SUM_PRICE0: v = red[0][N + PX_PRICE0]; break;
      case LOMPC_STAT_MAX_ERR: v = red[0][N + PX_MAX_ERR]; break;
      case LOMPC_STAT_SUM_COST: v = red[0][N + PX_COST]; break;
      case LOMPC_STAT_N_REPAIRED: v = red[0][N + PX_N_REPAIRED]; break;
      case LOMPC_STAT_N_FAILED: v = red[0][N + PX_N_FAILED]; break;
      default: v = red[0][N + PX_N_INVALID]; break;
    }
    if (r.set_stats) r.set_stats[(size_t)s * LOMPC_SET_STATS + tid] = v;
    if (r.stats) r.stats[(size_t)s * LOMPC_SET_STATS + tid] = v;
  }
}


__global__ __launch_bounds__(256) void k_finalize(FinalArgs r) {
  __shared__ double red[LQ_FIN_CLASSES][FIN_W];
  __shared__ double rep[LQ_FIN_CLASSES][FIN_W];
  if (r.skip && *r.skip) return;
  finalize_set<4, false>(r, (int)blockIdx.x, red, rep);
}

// lompc_plan_run_steps: run k's path (workgroups [0, S G)) and run k - 1's closing (one one-wave
// workgroup per set after them) in ONE launch — the two are independent (run k - 1's records
// are complete at the kernel boundary behind its k_eval; run k's path writes the other half of
// the cell-start working sets the closing's individual re-solves read), so every run after the
// first costs two launches instead of three.
template <int NT>
__global__ __launch_bounds__(64) void k_path_fin(PathArgs a, FinalArgs r) {
  const int b = (int)blockIdx.x, nc = a.S * a.G;
  if (b < nc) {
    path_cell<NT, true>(a, b);
  } else {
    __shared__ double red[LQ_FIN_CLASSES][FIN_W];
    __shared__ double rep[LQ_FIN_CLASSES][FIN_W];
    finalize_set<1, false>(r, b - nc, red, rep);
  }
}

PathKernel2 path_fin_kernel(int N) {
  switch (N) {
    case 12: return k_path_fin<12>;
    case 16: return k_path_fin<16>;
    case 24: return k_path_fin<24>;
    case 48: return k_path_fin<48>;
    default: return k_path_fin<0>;
  }
}

// Plans with a communicator: the all-gathered records recv[rank][S (N + 8)] of every rank combined
// in rank order — sums, max for LOMPC_STAT_MAX_ERR — into the caller's set outputs (either may be
// null).  Every rank runs the same arithmetic on the same bytes: the results are bitwise equal.
__global__ __launch_bounds__(256) void k_combine(const double* __restrict__ recv, int nranks, int S, int N,
                                                 double* set_sum_w, double* set_stats) {
  const int SN = S * N, L = S * (N + LOMPC_SET_STATS);
  for (int c = (int)(blockIdx.x * 256 + threadIdx.x); c < L; c += (int)(gridDim.x * 256)) {
    const bool is_max = c >= SN && (c - SN) % LOMPC_SET_STATS == LOMPC_STAT_MAX_ERR;
    double v = recv[c];
    for (int k = 1; k < nranks; ++k) {
      const double x = recv[(size_t)k * L + c];
      v = is_max ? fmax(v, x) : v + x;
    }
    if (c < SN) {
      if (set_sum_w) set_sum_w[c] = v;
    } else if (set_stats) {
      set_stats[c - SN] = v;
    }
  }
}

// The wide form's exchange for a group of n runs (one all-gather of the n runs' packed records):
// recv[rank][n][S (N + 8)]; run r's records combined in rank order as k_combine does, into the run's
// set outputs at (run0 + r) * stride (stride 0: shared outputs, only run `last` writes them)
struct CombineRunsArgs {
  const double* recv;
  int nranks, n, S, N, run0, last;
  double* set_sum_w;
  double* set_stats;
  int64_t sw_stride, st_stride;
};
__global__ __launch_bounds__(256) void k_combine_runs(CombineRunsArgs a) {
  const int SN = a.S * a.N, L = a.S * (a.N + LOMPC_SET_STATS);
  const int64_t tot = (int64_t)a.n * L;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
    const int r = (int)(e / L), c = (int)(e - (int64_t)r * L), j = a.run0 + r;
    const bool is_max = c >= SN && (c - SN) % LOMPC_SET_STATS == LOMPC_STAT_MAX_ERR;
    double v = a.recv[(size_t)r * L + c];
    for (int k = 1; k < a.nranks; ++k) {
      const double x = a.recv[((size_t)k * a.n + r) * L + c];
      v = is_max ? fmax(v, x) : v + x;
    }
    if (c < SN) {
      if (a.set_sum_w && (a.sw_stride || j == a.last)) a.set_sum_w[(size_t)j * a.sw_stride + c] = v;
    } else if (a.set_stats && (a.st_stride || j == a.last)) {
      a.set_stats[(size_t)j * a.st_stride + c - SN] = v;
    }
  }
}

// lompc_plan_run_chain: run k's prices from run k - 1's closed set reductions (the dependence of the
// reference's price iterations, price_solver.py:111-140): one workgroup per set, lane = price
// coordinate i = seg N + t,
//   lmbd_k[i] = max(0, lmbd_{k-1}[i] + step (phi(wbar)[i] - phi(w_target)[i])),  wbar = sum_w / count
// with phi = (theta w, theta (w_max - w), q_s w^2) (lompc.py:172-177) of the set's EV type.  A set
// without EVs keeps its prices.
__global__ __launch_bounds__(256) void k_chain_price(const QPConst* __restrict__ q, CtxEnds ce, int nctx, int N,
                                                     const double* __restrict__ prev, const double* __restrict__ sum_w,
                                                     const double* __restrict__ stats,
                                                     const double* __restrict__ target, double step,
                                                     double* __restrict__ next) {
  const int s = blockIdx.x;
  int k = 0;
  while (k + 1 < nctx && s >= ce.end[k]) ++k;
  const double th = q[k].theta, wm = q[k].w_max, qs = q[k].q_scale;
  const double n = stats[(size_t)s * LOMPC_SET_STATS + LOMPC_STAT_COUNT];
  for (int i = threadIdx.x; i < 3 * N; i += blockDim.x) {
    const int seg = i / N, t = i - seg * N;
    const double x = prev[(size_t)s * 3 * N + i];
    double v = x;
    if (n > 0) {
      const double wb = sum_w[(size_t)s * N + t] / n, wr = target[(size_t)s * N + t];
      const double g = seg == 0 ? th * (wb - wr) : (seg == 1 ? th * ((wm - wb) - (wm - wr)) : qs * (wb * wb - wr * wr));
      v = fmax(0.0, x + step * g);
    }
    next[(size_t)s * 3 * N + i] = v;
  }
}

// One k_eval block (EVs [start, end) of one set, <= EVAL_MAXB) by the whole workgroup.
// NT: the horizon as a compile-time constant (0: a.N at run time) — the row loop's lane map
// (stages per lane, rows per store instruction) and its address arithmetic become constants.
// CLOSE: the set is closed inside the launch (no k_finalize).  The workgroup record is built
// BEFORE the rows: the per-stage sums come from per-piece aggregates (EV count and gamma sum of
// each piece, fixed-point integer LDS atomics: exact and order-free), so wave 0 publishes the
// record and arrives on the set's counter while no row store is in flight, and the other waves
// write all the rows; the set's last arriver closes it (finalize_set) after its rows.  Rows of
// EVs left to the individual re-solve are not written here (key ZD), the closing workgroup writes
// them, so no two writes of a row race.
// k_evals: where one run's tables, records, per-EV outputs and prices sit (offsets from the
// EvalArgs pointers, so a loop over runs keeps one base per array instead of one pointer per run)
struct RunOff {
  int64_t tab = 0;  // cells: the run's path-table ring slot
  int rec = 0;      // blocks: the run's record slot
  int64_t ev = 0;   // EVs: per-run per-EV outputs
  const double* lmbd = nullptr;    // (null: a.lmbd / a.lmbd_r)
  const double* lmbd_r = nullptr;
  bool launder = false;
  bool gamma_lds = false;  // the block's gamma from the previous run's s_g (k_evals: the same EVs every run)
  bool nostage = false;  // (diagnostic builds, LQ_EVALS_NOSTAGE: keep the previous run's staged table)
  bool pipelined = false;  // (k_evals) staging loads before a barrier, the record by the block's last wave
  bool first = false;      // (k_evals) the launch's first run
};

template <int NT = 0, bool CLOSE = false>
__device__ __forceinline__ void eval_block(const EvalArgs& a, const int blk, const FinalArgs* fr = nullptr,
                                           const RunOff ro = RunOff{}) {
  // dynamic LDS: [cap + 2][NS] piece rows (rows cap, cap + 1: zero pieces) | [cap][8]
  // coefficients (cfx) | [LQ_PPL][Gs] piece ends | cells: coverage start | piece count | (CLOSE) per
  // piece: gamma sum, EV count.  Laid out for the banks (64 dwords for ds_read_b64 / b128): a
  // piece row holds its even stages, then its odd ones (even N: the row phase's two 16-B reads
  // per lane are contiguous across a row's lanes, not 32 B apart), and rows, coefficient records
  // and piece ends are padded / swizzled / transposed so that lanes reading different pieces or cells
  // spread over the banks instead of landing on the same few
  extern __shared__ __attribute__((aligned(16))) double2 s_dyn[];
  __shared__ double s_g[EVAL_MAXB];  // block row r = EV start + r: gamma
  __shared__ int s_k[EVAL_MAXB];     //   its piece (ZK / ZD: zero pieces)
  __shared__ double s_accw[EVAL_WAVES][LOMPC_MAX_N];  // per-wave row sums per stage
  __shared__ double s_red[EVAL_WAVES][8];
  __shared__ int s_fc[EVAL_WAVES];  // (CLOSE) re-solve list lengths
  __shared__ int s_last;            // (CLOSE) this workgroup closes the set
  __shared__ int s_mx;              // the set's largest piece count of a cell
  __shared__ int s_done;            // (pipelined) waves past their rows, this run
  int tid_ = (int)threadIdx.x;
  if (ro.launder) asm volatile("" : "+v"(tid_));  // (k_evals: lane-derived indices recomputed every run, not
                                                  // hoisted out of its loop and spilled)
  // (the wave index through readfirstlane: what follows from it — the wave's rows, its pass counts, its record
  // slots — is then scalar: branches on it are scalar branches, not exec masks)
  const int tid = tid_, lane = tid & 63, wv = LQ_EVAL_WV_SCALAR ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int4 info = a.blk[blk];
  const int rb = ro.rec + blk;  // this block's record (k_evals: in its run's record slot)
  // per-EV outputs (k_evals with per-run outputs: at the run's offset)
  double* const aw = a.w ? a.w + ro.ev * (NT ? NT : a.N) : nullptr;
  double* const acost = a.cost ? a.cost + ro.ev : nullptr;
  double* const aw0 = a.w0 ? a.w0 + ro.ev : nullptr;
  int8_t* const astatus = a.status ? a.status + ro.ev : nullptr;
  const int s = info.x, start = info.y, end = info.z;  // thread: EVs start + tid + EVAL_EVS h
  auto brow = [&](const int h) { return tid + EVAL_EVS * h; };  // block row of pass h
  auto bact = [&](const int h) { return start + tid + EVAL_EVS * h < end; };
  LQ_STAMPW(6);  // (diagnostic build: the block map's load round)
  int G_ = a.G, cap_ = a.cap;
  if (ro.launder) asm volatile("" : "+s"(G_), "+s"(cap_));  // (k_evals: the LDS layout per run, as tid)
  const int N = NT ? NT : a.N, G = G_;
  const int cap = cap_;
  const int ZK = cap;      // the zero piece (a = b = 0): rows of invalid (and, without CLOSE,
                           // re-solved) EVs, which then add exactly 0 to the row sums and need no
                           // branch in the row loop
  const int ZD = cap + 1;  // (CLOSE) zero piece whose row is not written: re-solved EVs
  // (k_evals of a run with no w output: the set's per-stage sums from per-piece EV counts and
  // fixed-point gamma sums — sum_p n_p a_p + Gamma_p b_p, unclamped, as the close mode and k_agg —
  // instead of evaluating and summing every EV's N rows that are never stored)
  const bool psum = !CLOSE && ro.pipelined && a.piece_sums && !aw;
  LQ_STAMPE(0);
  LQ_WSTART();
  const int NS = eval_row_stride(N);
  // LDS index of stage t of piece row k
  auto abx = [&](const int k, const int t) { return k * NS + ((N & 1) ? t : (t & 1) * (N >> 1) + (t >> 1)); };
  double2* s_ab = s_dyn;
  double* s_cf = reinterpret_cast<double*>(s_ab + (size_t)(cap + 2) * NS);
  double* s_ge = s_cf + (size_t)cap * 8;
  double* s_lo = s_ge + cap;
  int* s_cnt = reinterpret_cast<int*>(s_lo + G);
  unsigned long long* s_pf = reinterpret_cast<unsigned long long*>(s_cnt + ((G + 1) & ~1));
  int* s_pn = reinterpret_cast<int*>(s_pf + cap + 2);
  const int np = min(G * LQ_PPL, cap);
  const int Gs = np / LQ_PPL;  // cells with staged pieces (the rest are re-solved)
  // staged cells per wave (wv, wv + W, ...) and piece-row loads per lane and cell
  constexpr int CPW = (LQ_PIECE_CAP / LQ_PPL + EVAL_WAVES - 1) / EVAL_WAVES;
  constexpr int UA = ((NT ? NT : LOMPC_MAX_N) * LQ_PPL + 63) / 64;
  int wc = 0;  // lane j < CPW: piece count of cell wv + W j
  if (lane < CPW && wv + EVAL_WAVES * lane < Gs)
    wc = ld_t<false>(a.t_cnt + ro.tab + (size_t)s * G + wv + EVAL_WAVES * lane);
  // this thread's EVs (caller order)
  double gh[EVAL_PASSES];
#pragma unroll
  for (int h = 0; h < EVAL_PASSES; ++h) {  // (k_evals after its first run: from LDS, no memory round
    const int i = start + brow(h);            //  queued behind the previous run's row stores)
    gh[h] = ro.gamma_lds ? s_g[brow(h)] : bact(h) ? a.gamma[i] : 0.0;
  }
  const QPConst& q = set_consts(a.qd, a.ce, s);
  double wlo = a.window[2 * s], whi = a.window[2 * s + 1];
  const double* __restrict__ L = (ro.lmbd ? ro.lmbd : a.lmbd) + (size_t)s * 3 * N;
  double l0[3] = {L[0], L[N], L[2 * N]};  // price0 (lompc.py:164-170)
  double lr = (ro.lmbd_r ? ro.lmbd_r : a.lmbd_r)[s];
  const int64_t cb = ro.tab + (int64_t)s * G;  // the set's first cell in the table
  // the set's USED piece slots (a cell's first t_cnt of its LQ_PPL; cells past the first `cap`
  // slots are re-solved individually) and the cells' counts / coverage starts.  Two memory rounds,
  // both wave-local (no barrier): each wave reads the counts of the cells whose pieces it stages
  // (issued before the gamma loads, above), then only those cells' used rows, coefficient records
  // and piece ends — cells hold 1-2 pieces on average, so this moves a fraction of the 8 slots
  const size_t sb = (size_t)cb * LQ_PPL;
  if (ro.pipelined && ro.first && tid == 0) s_done = 0;  // (published by the staging barriers)
  if (!ro.nostage) {
    int vn = 0;
    double vl = 0.0;
    if (tid < G) {
      vn = ld_t<false>(a.t_cnt + cb + tid);
      vl = ld_t<false>(a.t_lo + cb + tid);
    }
    // the set's constants and this workgroup's scalars land with this round, not after the
    // staging (scalar loads are otherwise issued at first use, each a memory round of its own)
    lq_tab_fill(q);  // (published by the barrier below)
    lq_pin(wlo);
    lq_pin(whi);
    lq_pin(l0[0]);
    lq_pin(l0[1]);
    lq_pin(l0[2]);
    lq_pin(lr);
    LQ_STAMPW(2);  // (diagnostic build: counts, gamma and the cells' loads)
    double2 v[CPW][UA];
    double vc[CPW], vg[CPW];
    int nc[CPW];
#pragma unroll
    for (int j = 0; j < CPW; ++j)  // (every count read before any piece load is issued; a lane of
      nc[j] = min(max(lqw::readlane_i(wc, j), 0), LQ_PPL);  //  a cell past Gs loaded 0)
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int c = wv + EVAL_WAVES * j;
      const size_t so = sb + (size_t)c * LQ_PPL;  // the cell's first slot
#pragma unroll
      for (int u = 0; u < UA; ++u) {
        const int it = lane + 64 * u;
        v[j][u] = it < nc[j] * N ? ld_t<false>(a.t_ab + so * N + it) : make_double2(0.0, 0.0);
      }
      vc[j] = lane < nc[j] * 8 ? ld_t<false>(a.t_cf + so * 8 + lane) : 0.0;
      vg[j] = lane < nc[j] ? ld_t<false>(a.t_ge + so + lane) : 0.0;
    }
    LQ_STAMPW(3);  // (diagnostic build: the pieces' load round)
    // (k_evals: the loads above were issued while other waves may still write the previous run's rows
    // from the table; the LDS writes below wait until every wave is past them)
    if (ro.pipelined) __syncthreads();
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const int c = wv + EVAL_WAVES * j;
#pragma unroll
      for (int u = 0; u < UA; ++u) {
        const int it = lane + 64 * u;
        if (it < nc[j] * N) {
          const int k = it / N;
          s_ab[abx(c * LQ_PPL + k, it - k * N)] = v[j][u];
        }
      }
      if (lane < nc[j] * 8) s_cf[cfx(c * LQ_PPL + (lane >> 3), lane & 7)] = vc[j];
      if (lane < nc[j]) s_ge[lane * Gs + c] = vg[j];
    }
    if (tid < G) {
      s_cnt[tid] = vn;
      s_lo[tid] = vl;
    }
    if (wv == 0) {  // the set's largest cell piece count: the lookup reads no piece end past it
      const double m = lqw::wave_max(tid < G ? (double)vn : 0.0, 64);
      if (lane == 0) s_mx = G <= 64 ? (int)m : LQ_PPL;
    }
    if (tid < 2 * NS) s_ab[ZK * NS + tid] = make_double2(0.0, 0.0);  // both zero pieces
    if ((CLOSE || psum) && tid < cap + 2) {
      s_pf[tid] = 0ull;
      s_pn[tid] = 0;
    }
    for (int c = tid + EVAL_EVS; c < G; c += EVAL_EVS) {
      s_cnt[c] = ld_t<false>(a.t_cnt + cb + c);
      s_lo[c] = ld_t<false>(a.t_lo + cb + c);
    }
  }
  __syncthreads();  // the staged table and the box table (lq_tab_fill) published
  LQ_STAMPE(1);
  // ---- lane = EV: piece, scalar outputs; EVs no certified piece covers listed for the
  //      individual re-solve (counted as pending failures until then)
  // (w_max canonical here, once: fmin quiets its operands, and the compiler otherwise does so per row batch)
  const double ym = q.y_max, wm = __builtin_canonicalize(q.w_max);
  const double tt = q.theta * q.theta;
  const double cscale = (double)G / (whi - wlo);
  const double fxs = 0x1p40 / (whi - wlo);  // (CLOSE) gamma - wlo in units of the window / 2^40
  double acc_cost = 0.0, acc_p0 = 0.0, acc_err = 0.0;
  // (wave-uniform counts: ballot + popcount per pass, no per-lane counters to reduce; the wave's re-solved
  // EVs are its list's length)
  int n_ok = 0, n_inv = 0, nlist = 0;
  bool inv_rows = false;  // (wave-uniform) some row of this wave has an invalid gamma
  const int mxc = s_mx;  // (block-uniform) the set's largest cell piece count: no piece end past it is read
  // one pass of the lookup: this thread's EV h
  // the lookup in two halves: lookup_key (the piece: the rows need only it) and lookup_out (the piece's
  // coefficients -> the scalar outputs), which the row passes run after their rows (its LDS round and
  // stores then follow the row stores instead of holding them back); per pass the piece and flags
  int pk[EVAL_PASSES];
  unsigned pf[EVAL_PASSES];  // bit 0: cov, bit 1: act && !valid
  // MX > 0: the set's largest cell piece count (mxc) as a constant, so the compare and select chains below run
  // over MX ends and not the table's LQ_PPL (a cell's count is at most mxc: the dropped terms are all false);
  // MX = 0: any mxc
  auto lookup_key_mx = [&](auto mx_t, const int h) {
    constexpr int MX = decltype(mx_t)::value, KE = MX ? MX : LQ_PPL;
    const int i = start + brow(h);
    const bool act = bact(h);
    const double g = gh[h];
    const bool valid = act && g >= 0.0 && g <= ym;
    const int c = valid ? cell_of(g, wlo, cscale, G) : 0;
    const int nc = s_cnt[c];
    const int kb = c * LQ_PPL, ke = kb + nc;  // the cell's pieces [kb, ke), ascending gamma
    double ge[LQ_PPL];
#pragma unroll
    for (int k = 0; k < KE; ++k)
      ge[k] = ((MX || k < mxc) && !LQ_DIAG_NOLOOKUP) ? s_ge[k * Gs + min(c, Gs - 1)] : 0.0;
    const double glo_c = s_lo[c];
    int key = kb;  // piece = number of piece ends below g (every end read at once, no loop)
    double gend = ge[0];
#pragma unroll
    for (int k = 0; k + 1 < KE; ++k) key += (k + 1 < nc && g > ge[k]) ? 1 : 0;
#pragma unroll
    for (int k = 1; k < KE; ++k) gend = nc == k + 1 ? ge[k] : gend;  // the last piece's end
    const bool cov = LQ_DIAG_NOLOOKUP ? valid && ke > kb  // (diagnostic timing builds: the cell's first piece)
                                      : valid && ke > kb && ke <= np && g >= glo_c && g <= gend;
    pk[h] = key;
    pf[h] = (cov ? 1u : 0u) | ((act && !valid) ? 2u : 0u);
    s_g[brow(h)] = g;
    s_k[brow(h)] = cov ? key : ((CLOSE && valid) ? ZD : ZK);
    inv_rows |= __ballot(act && !valid) != 0ull;
    const unsigned long long need = __ballot(valid && !cov);
    if (valid && !cov) {
      st_wt4(a.fail_idx + (size_t)rb * EVAL_MAXB + 64 * EVAL_PASSES * wv + nlist +
                 __popcll(need & ((1ull << lane) - 1ull)), i);
    }
    nlist += __popcll(need);
  };
  const int mxu = __builtin_amdgcn_readfirstlane(mxc);
  auto lookup_key = [&](const int h) {  // (a wave-uniform switch)
    switch (mxu) {
      case 1: lookup_key_mx(std::integral_constant<int, 1>{}, h); break;
      case 2: lookup_key_mx(std::integral_constant<int, 2>{}, h); break;
      case 3: lookup_key_mx(std::integral_constant<int, 3>{}, h); break;
      case 4: lookup_key_mx(std::integral_constant<int, 4>{}, h); break;
      default: lookup_key_mx(std::integral_constant<int, 0>{}, h); break;
    }
  };
  auto lookup_out = [&](const int h) {
    const int i = start + brow(h);
    const double g = gh[h];
    const int key = pk[h];
    const bool cov = (pf[h] & 1u) != 0u;
    n_inv += __popcll(__ballot((pf[h] & 2u) != 0u));
    n_ok += __popcll(__ballot(pf[h] == 1u));
    if ((pf[h] & 2u) != 0u) {
      if (acost) st_ev8(acost + i, NAN);
      if (aw0) st_ev8(aw0 + i, NAN);
      if (astatus) astatus[i] = LOMPC_QP_INVALID;
    } else if (cov) {
      const double2 q0 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 0));
      const double2 q1 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 2));
      const double2 q2 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 4));
      const double2 q3 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 6));
      const double4 c0 = make_double4(q0.x, q0.y, q1.x, q1.y), c1 = make_double4(q2.x, q2.y, q3.x, q3.y);
      const double cst = fma(fma(c0.z, g, c0.y), g, c0.x);
      const double e2 = fma(fma(c1.y, g, c1.x), g, c0.w);
      const double er = a.want_err ? fmax(e2, 0.0) : 0.0;  // squared: sqrt of the max at the record
      const double w0v = clampw(fma(c1.w, g, c1.z), wm);
      const double p0 = q.theta * (w0v * l0[0] + (wm - w0v) * l0[1]) + q.q_scale * w0v * w0v * l0[2] +
                        tt * w0v * w0v * lr;  // lompc.py:164-170
      acc_cost += cst;
      acc_p0 += p0;
      acc_err = fmax(acc_err, er);
      if (acost) st_ev8(acost + i, cst);
      if (aw0) st_ev8(aw0 + i, w0v);
      if (astatus) astatus[i] = LOMPC_QP_OK;
      if (CLOSE || psum) {
        atomicAdd(s_pn + key, 1);
        atomicAdd(s_pf + key, (unsigned long long)rint(fmax(g - wlo, 0.0) * fxs));
      }
    }
  };
  auto lookup = [&](const int h) {
    lookup_key(h);
    lookup_out(h);
  };
  // a wave without EVs in a pass skips it (wave-uniform; its rows are never read)
  auto pass_live = [&](const int h) { return h == 0 || start + EVAL_EVS * h + 64 * wv < end; };
  if constexpr (CLOSE) {  // (the record is built before the rows: every lookup first)
#pragma unroll
    for (int h = 0; h < EVAL_PASSES; ++h)
      if (pass_live(h)) lookup(h);
  }
  LQ_STAMPE(7);
  // this wave's record and row sums (plain variables on purpose: as constants, k_eval, k_step and the run-time-N
  // k_evals came out with other registers and another schedule)
  double* accw_all = &s_accw[0][0];  // [EVAL_WAVES][astr] row sums
  double* red_all = &s_red[0][0];    // [EVAL_WAVES][8] wave records
  int astr = LOMPC_MAX_N;
  double* const red_w = red_all + wv * 8;
  double* const accw_w = accw_all + wv * astr;
  // per-wave totals of the scalar outputs
  auto wave_record = [&]() {
    double tot[2] = {acc_cost, acc_p0};
    lqw::wave_totals(tot, 64);
    // (without want_err every lane's error is 0: no scan; sqrt is monotone: max of the roots)
    const double mx = a.want_err ? sqrt(lqw::wave_max(acc_err, 64)) : 0.0;
    if (lane == 0) {
      red_w[PX_COST] = tot[0];
      red_w[PX_PRICE0] = tot[1];
      red_w[PX_MAX_ERR] = mx;
      red_w[PX_N_OK] = (double)n_ok;
      red_w[PX_N_REPAIRED] = 0.0;
      red_w[PX_N_FAILED] = (double)nlist;
      red_w[PX_N_INVALID] = (double)n_inv;
    }
  };
  // the workgroup record (fixed-order combination of the waves'), by the threads of `lanes`
  auto store_record = [&](int t, int nthreads) {
    double* part = a.partial + (size_t)rb * (N + NPX);
    for (int c = t; c < N + NPX; c += nthreads) {
      double v = 0.0;
      if (c < N) {
        for (int k = 0; k < EVAL_WAVES; ++k) v += accw_all[k * astr + c];
      } else {
        const int x = c - N;
        for (int k = 0; k < EVAL_WAVES; ++k) v = x == PX_MAX_ERR ? fmax(v, red_all[k * 8 + x]) : v + red_all[k * 8 + x];
      }
      st_wt8(part + c, v);
    }
  };
  bool any_inv = inv_rows;  // (CLOSE: the block's; else this wave's own rows)
  if constexpr (CLOSE) {
    if (lane == 0) s_fc[wv] = nlist;
    if (nlist > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's re-solve list has landed
    __syncthreads();  // every row's key, the piece aggregates and the list lengths complete
    // per-stage sums of the block's rows: sum over pieces p of n_p a_t + Gamma_p b_t, pieces
    // p = wv, wv + W, ... by wave wv (lane = stage), the waves combined in a fixed order
    const double fxi = (whi - wlo) * 0x1p-40;
    double accs = 0.0;
    constexpr int PU = (LQ_PIECE_CAP + EVAL_WAVES - 1) / EVAL_WAVES;
    for (int p0 = wv; p0 < np; p0 += EVAL_WAVES * PU) {  // (one iteration for np <= LQ_PIECE_CAP)
      int n[PU];
      unsigned long long f[PU];
      double2 ab[PU];
#pragma unroll
      for (int k = 0; k < PU; ++k) {  // every read of the batch in flight together
        const int p = p0 + EVAL_WAVES * k;
        const int pc = min(p, np - 1);
        n[k] = p < np ? s_pn[pc] : 0;
        f[k] = s_pf[pc];
        ab[k] = s_ab[abx(pc, min(lane, N - 1))];
      }
#pragma unroll
      for (int k = 0; k < PU; ++k) {
        // (n = 0: an unused slot, whose row is not read into the sum)
        const double gsum = fma((double)f[k], fxi, (double)n[k] * wlo);
        accs = fma((double)n[k], n[k] ? ab[k].x : 0.0, accs);
        accs = fma(n[k] ? gsum : 0.0, n[k] ? ab[k].y : 0.0, accs);
      }
    }
    if (lane < N) s_accw[wv][lane] = accs;
    wave_record();
    __syncthreads();
    any_inv = false;
    for (int k = 0; k < EVAL_WAVES; ++k) any_inv |= s_red[k][PX_N_INVALID] > 0.0;
    if (wv == 0) {  // publish the record, then arrive (nothing but the lookup's stores in flight)
      store_record(lane, 64);
      if (lane < EVAL_WAVES) st_wt4(a.fail_cnt + (size_t)rb * EVAL_WAVES + lane, s_fc[lane]);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) {
        const int nb = fr->blk_prefix[s + 1] - fr->blk_prefix[s];
        const int old = __hip_atomic_fetch_add(fr->arrive + s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == nb - 1;
        if (old == nb - 1) __hip_atomic_store(fr->arrive + s, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  // ---- rows (lane = stage pair): w_t = a_t + b_t gamma of the EV's piece -> contiguous rows
  const int V = (N & 1) ? 1 : 2;  // stages per lane (16-B stores for even N)
  const int Lr = N / V;           // lanes per row
  const int R = 64 / Lr;          // rows per store instruction
  const int rr = lane / Lr, col = lane - rr * Lr;
  const bool rlane = rr < R;
  const int t0 = V * col;
  constexpr int RU = EVAL_RU;  // row instructions per batch: their LDS reads in flight together
  double acc0 = 0.0, acc1 = 0.0;
  // a segment of the block's rows r0b .. r0b + nrows - 1 (EVs start + r, contiguous in w): every
  // row is a plain piece lookup (re-solved and invalid EVs read a zero piece), so the loop has
  // no per-row branch: the stores of a full batch use one address register and immediate
  // offsets; lanes past the row width (rlane false) store out of the descriptor's range, which
  // drops them (a w too large for a descriptor, B N 8 > LQ_DROP_OFF, takes plain stores: there those
  // lanes' row is clamped to the segment, see the store)
  const bool fast = aw && a.w_rsrc_ok;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(aw, (short)0, aw ? a.w_bytes : 0, 0x00020000);
  // (LDS through 32-bit address-space pointers: the piece rows' and the keys' addresses are 32-bit
  // multiply-adds and shifts, not 64-bit ones)
  typedef double lds_d2v __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) const lds_d2v lds_cd2;
  typedef __attribute__((address_space(3))) const double lds_cd;
  typedef __attribute__((address_space(3))) const int lds_ci;
  auto row_segment = [&](const int r0b, const int nrows) {
    lds_ci* sk = (lds_ci*)(s_k + r0b);
    lds_cd* sg = (lds_cd*)(s_g + r0b);
    lds_cd2* sab = (lds_cd2*)s_ab;
    const int rbase = start + r0b;
    const int vb = rlane ? ((rbase + rr) * N + t0) * 8 : LQ_DROP_OFF;  // row rr of the segment
    int kk[RU];
    double gg[RU];
#pragma unroll
    for (int j = 0; j < RU; ++j) {
      const int rc = min(j * R + rr, nrows - 1);
      kk[j] = sk[rc];
      gg[j] = sg[rc];
    }
    // the batches r0 = rb, rb + RU R, ... < re.  FULL (every row of the batch exists and is written: no
    // per-row masks) and FAST (w through the descriptor: one address register, immediate offsets) are
    // wave-uniform and chosen per run of batches, so a run's loop carries neither test
    auto batches = [&](auto full_t, auto fast_t, const int rb, const int re) {
      constexpr bool FULL = decltype(full_t)::value, FAST = decltype(fast_t)::value;
      for (int r0 = rb; r0 < re; r0 += RU * R) {
        double2 u0[RU], u1[RU];
#pragma unroll
        for (int j = 0; j < RU; ++j) {
          if (LQ_DIAG_NOROWLDS) {  // (diagnostic timing builds: no LDS reads in the rows)
            u0[j] = make_double2(1e-3 * kk[j], 1e-3);
            u1[j] = make_double2(2e-3 * kk[j], 1e-3);
          } else {
            const lds_d2v p0 = sab[kk[j] * NS + col];  // stages t0, t0 + 1 (abx)
            u0[j] = make_double2(p0.x, p0.y);
            u1[j] = make_double2(0.0, 0.0);
            if (V == 2) {
              const lds_d2v p1 = sab[kk[j] * NS + (N >> 1) + col];
              u1[j] = make_double2(p1.x, p1.y);
            }
          }
        }
        int kn[RU];  // the next batch's keys and gammas (software pipeline: one LDS round per batch)
        double gn[RU];
#pragma unroll
        for (int j = 0; j < RU; ++j) {
          const int rc = min(r0 + (RU + j) * R + rr, nrows - 1);
          kn[j] = sk[rc];
          gn[j] = sg[rc];
        }
#pragma unroll
        for (int j = 0; j < RU; ++j) {
          const double x0 = clampw(fma(u0[j].y, gg[j], u0[j].x), wm);
          const double x1 = V == 2 ? clampw(fma(u1[j].y, gg[j], u1[j].x), wm) : 0.0;
          if (FULL || (rlane && r0 + j * R + rr < nrows && (!CLOSE || kk[j] != ZD))) {
            if (!CLOSE) {  // (FULL: lanes past the row width add 0 below)
              acc0 += x0;
              acc1 += x1;
            }
            if (FAST) {
              const int off = vb + (r0 + j * R) * N * 8;
              if (V == 2) st_wt16(rs, off, x0, x1);
              else st_wt8b(rs, off, x0);
            } else if (aw) {
              // (the row the lane's key and gamma were read from: for the rows' lanes r0 + j R + rr itself;
              // the lanes past the row width, which no descriptor drops here, hold row R of the instruction —
              // the next row, a duplicate of its own store — clamped at the segment's end to its last row.
              // Unclamped they wrote the last row's values into the next wave's first row or past the end
              // of w)
              double* dst = aw + (size_t)(rbase + min(r0 + j * R + rr, nrows - 1)) * N + t0;
              st_wt8(dst, x0);
              if (V == 2) st_wt8(dst + 1, x1);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < RU; ++j) {
          kk[j] = kn[j];
          gg[j] = gn[j];
        }
      }
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    if constexpr (CLOSE) {  // a batch with a row left to the re-solve takes the masked path: chosen per batch
      for (int r0 = 0; r0 < nrows; r0 += RU * R) {
        bool drop = false;
#pragma unroll
        for (int j = 0; j < RU; ++j) drop |= kk[j] == ZD;
        const bool full = r0 + RU * R <= nrows && !__any(drop);  // wave-uniform
        if (full) {
          if (fast) batches(T_{}, T_{}, r0, r0 + 1);
          else batches(T_{}, F_{}, r0, r0 + 1);
        } else {
          if (fast) batches(F_{}, T_{}, r0, r0 + 1);
          else batches(F_{}, F_{}, r0, r0 + 1);
        }
      }
    } else {  // the full batches, then the one partial batch (each lane: the same rows in the same order)
      const int nfull = nrows - nrows % (RU * R);
      if (fast) {
        batches(T_{}, T_{}, 0, nfull);
        if (nfull < nrows) batches(F_{}, T_{}, nfull, nrows);
      } else {
        batches(T_{}, F_{}, 0, nfull);
        if (nfull < nrows) batches(F_{}, F_{}, nfull, nrows);
      }
    }
    // rows of invalid EVs (gamma outside [0, y_max] or NaN): NaN, written after the loop's
    // zeros of the same rows (rare; ordered by the wait)
    if (any_inv && aw) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      for (int r = 0; r < nrows; ++r) {
        const double g = sg[r];
        if (!(g >= 0.0 && g <= ym) && lane < N) st_wt8(aw + (size_t)(rbase + r) * N + lane, NAN);
      }
    }
  };
  if constexpr (CLOSE) {  // waves 1.. split the block's rows evenly (wave 0 published the record)
    if (wv > 0 && aw) {  // (no w output: nothing to write, the sums are in the record)
      const int tot = end - start;
      const int lo = (wv - 1) * tot / (EVAL_WAVES - 1), hi = wv * tot / (EVAL_WAVES - 1);
      if (hi > lo) row_segment(lo, hi - lo);
    }
  } else {  // each wave: the lookup of a pass, then that pass's rows (the first row stores leave
            // half a lookup earlier and the second lookup overlaps their drain)
#pragma unroll
    for (int h = 0; h < EVAL_PASSES; ++h) {
      if (!pass_live(h)) break;
      if (LQ_EVAL_OUT_AFTER_ROWS) lookup_key(h);
      else lookup(h);
      __builtin_amdgcn_wave_barrier();  // this wave's own rows in LDS: in order
      any_inv = inv_rows;
      const int r0b = EVAL_EVS * h + 64 * wv;
      const int nh = __builtin_amdgcn_readfirstlane(max(0, min(64, end - start - r0b)));  // wave-uniform
      if (nh > 0 && !psum) row_segment(r0b, nh);
      if (LQ_EVAL_OUT_AFTER_ROWS) lookup_out(h);
    }
    if (lane == 0) st_wt4(a.fail_cnt + (size_t)rb * EVAL_WAVES + wv, nlist);
    wave_record();
  }
  LQ_STAMPE(4);
  if constexpr (CLOSE) {
    __syncthreads();  // every row written; the staged table is free (finalize_set's scratch)
    if (s_last) {
      double (*red)[FIN_W] = reinterpret_cast<double (*)[FIN_W]>(s_dyn);
      finalize_set<EVAL_WAVES, true>(*fr, s, red, red + EVAL_WAVES);
    }
  } else {
    if (!rlane) acc0 = acc1 = 0.0;  // (lanes past the row width read real rows in full batches)
    // this wave's row sums per stage: lanes col, col + Lr, ... (fixed order)
    {
      double s0 = acc0, s1 = acc1;
      for (int k = 1; k < R; ++k) {
        s0 += __shfl(acc0, lane + k * Lr, 64);
        s1 += __shfl(acc1, lane + k * Lr, 64);
      }
      if (lane < Lr) {
        accw_w[V * lane] = s0;
        if (V == 2) accw_w[V * lane + 1] = s1;
      }
    }
    if (ro.pipelined) {
      // the block's last wave to finish its rows writes the record (the others go on to the next run's
      // staging loads); the acquire-release LDS counter orders every wave's row sums before its read
      // Every lane of the wave takes part in the ordering: a workgroup-scope release fence (LDS only:
      // the row stores to HBM stay in flight) before lane 0's increment orders all lanes' row-sum
      // writes, and the acquire fence after the broadcast orders the last wave's reads of every
      // wave's sums, per the HIP memory model rather than per-wave LDS issue order
      int old = 0;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if (lane == 0) old = __hip_atomic_fetch_add(&s_done, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
      old = __shfl(old, 0, 64);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      if (old == EVAL_WAVES - 1) {
        if (psum) {
          // every wave's lookups (and their LDS piece aggregates) are complete: the per-stage sums
          // over the set's piece slots in slot order (lane = stage) into this wave's row sums (the
          // other waves' are zero: they evaluated no rows)
          const double fxi = (whi - wlo) * 0x1p-40;
          double accs = 0.0;
          for (int p = 0; p < np; ++p) {
            const int n = s_pn[p];
            if (n == 0) continue;  // (block-uniform)
            const double2 ab = s_ab[abx(p, min(lane, N - 1))];
            const double gsum = fma((double)s_pf[p], fxi, (double)n * wlo);
            accs = fma((double)n, ab.x, accs);
            accs = fma(gsum, ab.y, accs);
          }
          if (lane < N) accw_w[lane] = accs;  // (its own row: zero, no rows were evaluated)
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
        store_record(lane, 64);
        if (lane == 0) __hip_atomic_store(&s_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    } else {
      __syncthreads();
      if (tid < 64) store_record(tid, 64);
    }
  }
  LQ_STAMPE(5);
}

// k_eval.  CLOSE: the set's closing (finalize_set) runs inside the launch, by the workgroup of the
// set that arrives last (eval_block<..., CLOSE>), so no k_finalize launch and no kernel boundary
// follow; workgroup nblk closes the sets that have no EVs.
template <bool CLOSE, int NT>
__global__ __launch_bounds__(EVAL_EVS, EVAL_MIN_WAVES) void k_eval(EvalArgs a, FinalArgs r) {  // (4 waves per SIMD: two workgroups per CU)
  extern __shared__ __attribute__((aligned(16))) double2 s_dyn[];
  const int b = (int)blockIdx.x;
  if (a.skip && *a.skip) return;  // (every workgroup: the arrival counters stay at zero)
  if constexpr (CLOSE) {
    if (b == a.nblk) {
      double (*red)[FIN_W] = reinterpret_cast<double (*)[FIN_W]>(s_dyn);
      for (int s = 0; s < a.S; ++s)
        if (r.blk_prefix[s + 1] == r.blk_prefix[s]) {
          finalize_set<EVAL_WAVES, true>(r, s, red, red + EVAL_WAVES);
          __syncthreads();  // (red / rep are rewritten for the next set)
        }
      return;
    }
  }
  eval_block<NT, CLOSE>(a, b, &r);
}

// k_eval for horizon N: exact-N instantiations for the shipped horizons, run-time N otherwise
typedef void (*EvalKernel)(EvalArgs, FinalArgs);
template <bool CLOSE>
EvalKernel eval_kernel(int N) {
  switch (N) {
    case 12: return k_eval<CLOSE, 12>;
    case 16: return k_eval<CLOSE, 16>;
    case 24: return k_eval<CLOSE, 24>;
    case 48: return k_eval<CLOSE, 48>;
    default: return k_eval<CLOSE, 0>;
  }
}

// lompc_plan_run_steps, stepped form: ONE launch carries run k + 1's path (workgroups [0, np_wg):
// LQ_STEP_CELLS cells of one set each, one per wave), run k's evaluation (the next ne workgroups,
// k_eval's block; the block map sized for the slots the path leaves) and run k - 1's closing (nf
// workgroups, one per set).  The three are independent (separate path tables, records and cell-start
// working sets per run in flight), so the latency-bound path chain runs beside the bandwidth-bound
// evaluation instead of before it.  (The arguments stay kernel arguments: preloaded, where a record in
// memory would add a dependent load round at the start of every workgroup.)
template <int NT>
__global__ __launch_bounds__(EVAL_EVS, EVAL_MIN_WAVES) void k_step(PathArgs pa, EvalArgs ea, FinalArgs ff, int np_wg,
                                                                    int ne, int nf) {
  extern __shared__ __attribute__((aligned(16))) double2 s_dyn[];
  int b = (int)blockIdx.x;
  if (b < np_wg) {
    // (G % LQ_STEP_CELLS == 0: every cell of the workgroup in one set).  The waves without a cell exit
    // here; the path waves initialise the set's box table inside path_cell, after their price loads
    // are issued (the barrier overlaps them, as in k_path)
    const int wv = (int)(threadIdx.x >> 6), cell = b * LQ_STEP_CELLS + wv;
    if (wv >= LQ_STEP_CELLS || cell >= pa.S * pa.G) return;
    // the path chain is the launch's critical path: its waves issue first on a SIMD they share
    // with evaluation waves (which mostly wait on memory)
    if (LQ_STEP_PRIO) __builtin_amdgcn_s_setprio(3);
    path_cell<NT, true>(pa, cell);
    return;
  }
  b -= np_wg;
  if (b < ne) {
    eval_block<NT, false>(ea, b);
    return;
  }
  b -= ne;
  if (b < nf) {
    double (*red)[FIN_W] = reinterpret_cast<double (*)[FIN_W]>(s_dyn);
    finalize_set<EVAL_WAVES, false>(ff, b, red, red + EVAL_WAVES);
  }
}

typedef void (*StepKernel)(PathArgs, EvalArgs, FinalArgs, int, int, int);
StepKernel step_kernel(int N) {
  switch (N) {
    case 12: return k_step<12>;
    case 16: return k_step<16>;
    case 24: return k_step<24>;
    case 48: return k_step<48>;
    default: return k_step<0>;
  }
}

// The wide form's path launch (lompc_plan_run_steps without warm starts): the paths of runs run0 ..
// run0 + nruns - 1 in ONE launch, one wave per (run, set, cell) — thousands of independent
// latency-bound chains at once instead of one run's 384 beside an evaluation; run j's prices at
// lmbd + j lm_stride, its tables in ring slot j % slots
#ifndef LQ_PATHS_WAVES
#define LQ_PATHS_WAVES 1  // k_paths: min waves per SIMD the compiler must fit (registers)
#endif
template <int NT>
__global__ __launch_bounds__(64, LQ_PATHS_WAVES) void k_paths(PathArgs a, int64_t lm_stride, int64_t lr_stride, int run0,
                                                               int slots) {
  const int SG = a.S * a.G;
  const int r = (int)blockIdx.x / SG, cell = (int)blockIdx.x - r * SG;
  const int j = run0 + r;
  const int64_t o = (int64_t)(j % slots) * SG;
  PathArgs b = a;
  b.lmbd = a.lmbd + (size_t)j * lm_stride;
  b.lmbd_r = a.lmbd_r + (size_t)j * lr_stride;
  b.t_cnt = a.t_cnt + o;
  b.t_lo = a.t_lo + o;
  b.t_sl = a.t_sl + o * 64;
  b.t_ge = a.t_ge + o * LQ_PPL;
  b.t_cf = a.t_cf + o * LQ_PPL * 8;
  b.t_ab = a.t_ab + o * LQ_PPL * a.N;
  path_cell<NT, true>(b, cell);
}

typedef void (*PathsKernel)(PathArgs, int64_t, int64_t, int, int);
PathsKernel paths_kernel(int N) {
  switch (N) {
    case 12: return k_paths<12>;
    case 16: return k_paths<16>;
    case 24: return k_paths<24>;
    case 48: return k_paths<48>;
    default: return k_paths<0>;
  }
}

// The wide form's evaluations (lompc_plan_run_steps without warm starts, one part per kind): the
// evaluations of runs run0 .. run0 + nruns - 1 in ONE launch.  Workgroup b evaluates its block of
// every run in turn (k_eval's block map and arithmetic: eval_block), run j from ring slot j % slots
// of the path tables and into record slot j - run0, so the launch holds no kernel boundary between
// runs: while one workgroup stages run j + 1's pieces (its own loads wait for its row stores to be
// acknowledged: vmcnt counts both in order), the other workgroups of the CU keep their rows streaming,
// and no workgroup tail idles the chip between two runs.  Per-EV outputs at j ev_stride (0: every
// run rewrites the same rows, each row by the same wave and lane in every run, so in run order).
struct EvalsArgs {
  int run0, nruns, slots, nblk;
  int64_t lm_stride, lr_stride, ev_stride, SG;
};

#ifndef LQ_EVALS_PIPELINED
#define LQ_EVALS_PIPELINED 1  // k_evals: staging loads issued before the table's barrier, records by the last wave
#endif
#ifndef LQ_EVALS_RUN_BARRIER
#define LQ_EVALS_RUN_BARRIER 0  // 1: k_evals' former barrier at the end of every run (diagnostic builds)
#endif
#ifndef LQ_EVALS_SKEW
#define LQ_EVALS_SKEW 0  // k_evals: start delay (100 MHz ticks) of the grid's second half (diagnostic builds)
#endif

// (k_evals' second argument in the kernel argument segment: after the first, at its own alignment)
constexpr size_t KARG_X = (sizeof(EvalArgs) + alignof(EvalsArgs) - 1) / alignof(EvalsArgs) * alignof(EvalsArgs);
static_assert(alignof(EvalArgs) <= 8 && alignof(EvalsArgs) <= 8, "k_evals reads its arguments at offsets 0 and KARG_X");

template <int NT>
__global__ __launch_bounds__(EVAL_EVS, EVAL_MIN_WAVES) void k_evals(EvalArgs a, EvalsArgs x_) {
  const int b = (int)blockIdx.x;
  if (LQ_EVALS_SKEW > 0 && 2 * b >= x_.nblk) {  // (the two workgroups of a CU out of phase)
    const long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < LQ_EVALS_SKEW) __builtin_amdgcn_s_sleep(8);
  }
  for (int r = 0; r < x_.nruns; ++r) {
#if LQ_EVALS_KARGS
    // (the kernel's two argument structs read where they are used, from the argument segment through a
    // pointer laundered per run: scalar loads that hit the scalar cache, instead of some 70 scalar registers
    // held across the loop and spilled to vector lanes, each spill and reload a VALU instruction)
    typedef __attribute__((address_space(4))) const EvalArgs karg_t;
    typedef __attribute__((address_space(4))) const EvalsArgs kargx_t;
    typedef __attribute__((address_space(4))) const char kargc_t;
    karg_t* ka = (karg_t*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const EvalArgs& ar = *(const EvalArgs*)ka;
    const EvalsArgs& x = *(const EvalsArgs*)(kargx_t*)((kargc_t*)ka + KARG_X);
#else
    const EvalArgs& ar = a;
    const EvalsArgs& x = x_;
#endif
    const int j = x.run0 + r;
    RunOff ro;
    ro.tab = (int64_t)(j % x.slots) * x.SG;
    ro.rec = r * x.nblk;
    ro.ev = (int64_t)j * x.ev_stride;
    ro.lmbd = ar.lmbd + (size_t)j * x.lm_stride;
    ro.lmbd_r = ar.lmbd_r + (size_t)j * x.lr_stride;
    ro.launder = true;
    ro.gamma_lds = r > 0;
    ro.pipelined = LQ_EVALS_PIPELINED;
    ro.first = r == 0;
#ifdef LQ_EVALS_NOSTAGE
    ro.nostage = r > 0;  // (timing only: every run after the first evaluates run 0's table)
#endif
    // (the block index laundered per run: nothing derived from it — the block's EVs and gamma, the set's
    // constants — is hoisted out of the loop and kept live across runs, which made the loop spill)
    int bl = b;
    asm volatile("" : "+s"(bl));
#ifdef LOMPC_STAMPS
    // diagnostic build (scripts/evals_stamps.py): per (workgroup, run < 32) the run's start, the end
    // of its staging phases, the end of its rows and its end, at g_stamps[((b * 32 + r) * 8 + k]
    const long long t0__ = __builtin_amdgcn_s_memtime();
#endif
    eval_block<NT, false>(ar, bl, nullptr, ro);
    // (no barrier here: every wave has passed the block's record barrier, so every row of the run is
    // written and its table no longer read; wave 0 reads only the row sums while the others stage the
    // next run, and no wave writes row sums again before the next run's staging barrier, which wave 0
    // reaches after its record)
#if LQ_EVALS_RUN_BARRIER
    __syncthreads();
#endif
#ifdef LOMPC_STAMPS
    if (threadIdx.x == 0 && r < 32 && b < 512) {  // start, block map, scalars, counts, pieces, staged, rows, end
      long long* q = g_stamps + ((size_t)b * 32 + r) * 8;
      const long long* e = g_stamps + (32768 + b) * 8;
      q[0] = t0__;
      q[1] = e[6];
      q[2] = e[0];
      q[3] = e[2];
      q[4] = e[3];
      q[5] = e[1];
      q[6] = e[4];
      q[7] = __builtin_amdgcn_s_memtime();
    }
#endif
  }
}

// k_evals' runs for k_evals_tail's evaluation workgroups (b: the block): the same eval_block calls on the same RunOff,
// with k_evals' idioms (the argument structs re-read from the argument segment per run, where they sit at offsets
// 0 and KARG_X as in k_evals; the block index laundered per run), without its diagnostic builds' branches.  A
// copy, not a shared body: k_evals calling a common function kept its instruction counts but came out in another
// order, and k_evals stays the measured kernel, instruction for instruction
template <int NT>
__device__ __forceinline__ void evals_runs(const EvalArgs& a, const EvalsArgs& x_, const int b) {
  for (int r = 0; r < x_.nruns; ++r) {
#if LQ_EVALS_KARGS
    typedef __attribute__((address_space(4))) const EvalArgs karg_t;
    typedef __attribute__((address_space(4))) const EvalsArgs kargx_t;
    typedef __attribute__((address_space(4))) const char kargc_t;
    karg_t* ka = (karg_t*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const EvalArgs& ar = *(const EvalArgs*)ka;
    const EvalsArgs& x = *(const EvalsArgs*)(kargx_t*)((kargc_t*)ka + KARG_X);
#else
    const EvalArgs& ar = a;
    const EvalsArgs& x = x_;
#endif
    const int j = x.run0 + r;
    RunOff ro;
    ro.tab = (int64_t)(j % x.slots) * x.SG;
    ro.rec = r * x.nblk;
    ro.ev = (int64_t)j * x.ev_stride;
    ro.lmbd = ar.lmbd + (size_t)j * x.lm_stride;
    ro.lmbd_r = ar.lmbd_r + (size_t)j * x.lr_stride;
    ro.launder = true;
    ro.gamma_lds = r > 0;
    ro.pipelined = LQ_EVALS_PIPELINED;
    ro.first = r == 0;
    int bl = b;
    asm volatile("" : "+s"(bl));
    eval_block<NT, false>(ar, bl, nullptr, ro);
#if LQ_EVALS_RUN_BARRIER
    __syncthreads();
#endif
  }
}

// The wide form's fused launch (LQ_WIDE_TAIL_PATHS): group g's evaluations and, BEHIND them in grid order, group
// g + 1's paths.  Workgroups [0, x_.nblk) are k_evals' (evals_runs: the same eval_block calls on the same RunOff).
// Workgroups [nblk, nblk + npw) are path workgroups laid out as k_step's: LQ_STEP_CELLS cells of one set, one per
// wave (G % LQ_STEP_CELLS == 0), of LQ_TAIL_RUNS runs each (runs r < np of the next group; the waves left over return
// at once), the box table's barrier stays inside the set; run run0p + r's tables go to ring slot (run0p + r) %
// slots as k_paths writes them.  The
// evaluation workgroups fill the chip in one dispatch round, so the path workgroups are dispatched as evaluation
// workgroups retire and run in the launch's tail, which otherwise idles; no workgroup waits for another and the
// two kinds share no memory (the ring holds both groups: no run of group g uses a slot of group g + 1), so any
// dispatch order gives the same results.  The path waves keep the default issue priority: beside them the
// evaluation's last waves are the launch's critical path.
#ifndef LQ_TAIL_RUNS
// k_evals_tail: runs per path workgroup, the same LQ_STEP_CELLS cells of each (1: k_step's layout, the upper waves
// return at once; EVAL_WAVES / LQ_STEP_CELLS = 2: every wave a path — one set's box table serves both runs).  A
// workgroup is dispatched with all its waves' registers, so of the layout with 1 run a CU holds three workgroups
// (12 path waves), of the layout with 2 runs two (16 path waves, k_paths' own occupancy): 36 runs of 96 cells are
// 864 workgroups over 768 places (two rounds) against 432 over 512 (one).  Measured at 100 steps: 9.85 (9.80-9.91)
// against 9.93 (9.82-9.96) us per step, the fused launch 9.11 against 9.19 us per run (profiles/r08)
#define LQ_TAIL_RUNS (EVAL_WAVES / LQ_STEP_CELLS)
#endif
static_assert(LQ_TAIL_RUNS >= 1 && LQ_TAIL_RUNS * LQ_STEP_CELLS <= EVAL_WAVES, "k_evals_tail: one path per wave");
template <int NT>
__global__ __launch_bounds__(EVAL_EVS, EVAL_MIN_WAVES) void k_evals_tail(EvalArgs a, EvalsArgs x_, PathArgs pa, int run0p,
                                                                          int np) {
  const int q = (int)blockIdx.x - x_.nblk;
  if (q < 0) {
    evals_runs<NT>(a, x_, (int)blockIdx.x);
    return;
  }
  const int wv = (int)(threadIdx.x >> 6), wr = wv / LQ_STEP_CELLS;  // the wave's run of the workgroup's
  const int SG = (int)x_.SG, wpr = SG / LQ_STEP_CELLS;              // path workgroups per LQ_TAIL_RUNS runs
  const int r = q / wpr * LQ_TAIL_RUNS + wr, cell = (q % wpr) * LQ_STEP_CELLS + (wv - wr * LQ_STEP_CELLS);
  if (wr >= LQ_TAIL_RUNS || r >= np) return;
  const int j = run0p + r;
  const int64_t o = (int64_t)(j % x_.slots) * SG;
  PathArgs b = pa;
  b.lmbd = pa.lmbd + (size_t)j * x_.lm_stride;
  b.lmbd_r = pa.lmbd_r + (size_t)j * x_.lr_stride;
  b.t_cnt = pa.t_cnt + o;
  b.t_lo = pa.t_lo + o;
  b.t_sl = pa.t_sl + o * 64;
  b.t_ge = pa.t_ge + o * LQ_PPL;
  b.t_cf = pa.t_cf + o * LQ_PPL * 8;
  b.t_ab = pa.t_ab + o * LQ_PPL * pa.N;
  path_cell<NT, true>(b, cell);
}

typedef void (*EvalsKernel)(EvalArgs, EvalsArgs);
typedef void (*EvalsTailKernel)(EvalArgs, EvalsArgs, PathArgs, int, int);
EvalsTailKernel evals_tail_kernel(int N) {
  switch (N) {
    case 12: return k_evals_tail<12>;
    case 16: return k_evals_tail<16>;
    case 24: return k_evals_tail<24>;
    case 48: return k_evals_tail<48>;
    default: return k_evals_tail<0>;
  }
}
EvalsKernel evals_kernel(int N) {
  switch (N) {
    case 12: return k_evals<12>;
    case 16: return k_evals<16>;
    case 24: return k_evals<24>;
    case 48: return k_evals<48>;
    default: return k_evals<0>;
  }
}

// ... and their closings in ONE launch: workgroup (r, s) closes set s of run run0 + r (finalize_set: the
// same summation order as every other closing form).  Set outputs at j sw_stride / st_stride; with
// shared set outputs (stride 0) or shared per-EV outputs (ev_stride 0) only the call's last run writes
// them (the closings of one launch are unordered); the plan's status rows likewise.
struct ClosesArgs {
  int run0, nruns, slots, nblk, S, last;
  int rel;  // set outputs indexed by the run's place in the launch (a communicator's send slots), not j
  int64_t lm_stride, lr_stride, ev_stride, sw_stride, st_stride, SG;
};

__global__ __launch_bounds__(256) void k_closes(FinalArgs f, ClosesArgs x) {
  __shared__ double red[LQ_FIN_CLASSES][FIN_W];
  __shared__ double rep[LQ_FIN_CLASSES][FIN_W];
  const int r = (int)blockIdx.x / x.S, s = (int)blockIdx.x - r * x.S, j = x.run0 + r, N = f.N;
  FinalArgs c = f;
  c.lmbd = f.lmbd + (size_t)j * x.lm_stride;
  c.lmbd_r = f.lmbd_r + (size_t)j * x.lr_stride;
  c.t_sl = f.t_sl + (int64_t)(j % x.slots) * x.SG * 64;
  c.partial = f.partial + (size_t)r * x.nblk * (N + NPX);
  c.fail_cnt = f.fail_cnt + (size_t)r * x.nblk * EVAL_WAVES;
  c.fail_idx = f.fail_idx + (size_t)r * x.nblk * EVAL_MAXB;
  const bool last = j == x.last;
  if (x.ev_stride) {
    const size_t eo = (size_t)j * x.ev_stride;
    if (f.w) c.w = f.w + eo * N;
    if (f.cost) c.cost = f.cost + eo;
    if (f.w0) c.w0 = f.w0 + eo;
    if (f.status) c.status = f.status + eo;
  } else if (!last) {
    c.w = c.cost = c.w0 = nullptr;
    c.status = nullptr;
  }
  const int js = x.rel ? r : j;
  if (f.set_sum_w) c.set_sum_w = (x.sw_stride || last) ? f.set_sum_w + (size_t)js * x.sw_stride : nullptr;
  if (f.set_stats) c.set_stats = (x.st_stride || last) ? f.set_stats + (size_t)js * x.st_stride : nullptr;
  if (!last) c.stats = nullptr;
  finalize_set<4, false>(c, s, red, rep);
}
