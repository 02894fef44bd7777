// k_scalar: the scalar pass of a plan run (LOMPC_PLAN_SCALAR_PASS) — per-EV w0 / cost / status and the
// per-set sums of a run that asks for no w row and no per-stage sum.  Everything such a run needs of an
// EV's piece is in the path table's 64-byte coefficient record (cost quadratic, A_bar error^2
// quadratic, affine w0), so a workgroup stages per piece slot 72 bytes (record + piece end) where
// k_eval stages 16 N + 72: no piece rows, no box table, no row keys, no zero piece, and no per-stage
// sums are built.
//
// Included by lompc_plan.hip after k_eval (it reads EvalArgs and writes the records k_finalize
// closes).  The lookup is k_eval's (eval_block: lookup_key_mx / lookup_out) in its own copy: the same
// cell_of, the same count of piece ends below gamma, the same coverage test, the same explicit fma
// forms, so an EV's cost, w0 and status carry the same bits as the default evaluation's.  It keeps
// the plan's block map and k_eval's record layout — partial[nblk][N + NPX] with column 0 = sum of w0,
// columns 1 .. N - 1 zero; fail_cnt[nblk][EVAL_WAVES]; fail_idx[nblk][EVAL_MAXB], 64 EVAL_PASSES per
// wave — so the unchanged k_finalize closes the run: records summed in its fixed order, the listed
// EVs re-solved individually, the sticky tallies kept.
//
// k_scalars (below) is the same pass for the runs of a wide-form group (lompc_plan_run_steps with
// LOMPC_STEPS_SCALAR_PASS): both kernels call scalar_block, so the arithmetic exists once.
#pragma once

// waves per SIMD the compiler must fit (<= 64 VGPRs): four 8-wave workgroups per CU, which the
// pass's LDS (9.4 KB at 16 cells) allows
#ifndef LQ_SCALAR_MIN_WAVES
#define LQ_SCALAR_MIN_WAVES 8
#endif

// dynamic LDS of k_scalar with gs of a set's G cells staged: per staged slot the coefficient record
// and the piece end, per cell (all G) the coverage start and the piece count
__host__ __device__ inline size_t scalar_lds(int G, int gs) {
  return (size_t)gs * LQ_PPL * 9 * sizeof(double) + (size_t)G * sizeof(double) + (size_t)((G + 1) & ~1) * sizeof(int);
}

// One block of one run: k_scalar's whole body, shared with k_scalars.  ro: where the run's tables
// (ro.tab, cells), its records (ro.rec, blocks), its per-EV outputs (ro.ev, EVs) and its prices sit, as
// k_evals hands them to eval_block (k_scalar: all zero / the arguments' own).  store: the per-EV outputs
// are written (k_scalars with one shared per-EV buffer: by the call's last run only).
__device__ __forceinline__ void scalar_block(const EvalArgs& a, const int gs, const int blk, const RunOff ro,
                                             const bool store) {
  // dynamic LDS: [np][8] coefficient records (cfx) | [LQ_PPL][Gs] piece ends (transposed, as k_eval) |
  // [G] coverage starts | [G] piece counts
  extern __shared__ __attribute__((aligned(16))) double2 s_dyn[];
  __shared__ double s_red[EVAL_WAVES][8];  // wave records: the NPX scalars, [7] = the wave's sum of w0
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int4 info = a.blk[blk];
  const size_t rb = (size_t)ro.rec + blk;  // this block's record (k_scalars: in its run's record slot)
  double* const acost = store && a.cost ? a.cost + ro.ev : nullptr;
  double* const aw0 = store && a.w0 ? a.w0 + ro.ev : nullptr;
  int8_t* const astatus = store && a.status ? a.status + ro.ev : nullptr;
  const int s = info.x, start = info.y, end = info.z;  // thread: EVs start + tid + EVAL_EVS h
  const int N = a.N, G = a.G, Gs = gs;
  const int np = Gs * LQ_PPL;  // staged piece slots: the set's first Gs cells (the rest are re-solved)
  double* s_cf = reinterpret_cast<double*>(s_dyn);
  double* s_ge = s_cf + (size_t)np * 8;
  double* s_lo = s_ge + np;
  int* s_cnt = reinterpret_cast<int*>(s_lo + G);
  // this thread's EVs (caller order)
  double gh[EVAL_PASSES];
#pragma unroll
  for (int h = 0; h < EVAL_PASSES; ++h) {
    const int i = start + tid + EVAL_EVS * h;
    gh[h] = i < end ? a.gamma[i] : 0.0;
  }
  // the set's scalars (wave-uniform: scalar loads)
  const QPConst& q = set_consts(a.qd, a.ce, s);
  const double wlo = a.window[2 * s], whi = a.window[2 * s + 1];
  const double* __restrict__ L = (ro.lmbd ? ro.lmbd : a.lmbd) + (size_t)s * 3 * N;
  const double l0[3] = {L[0], L[N], L[2 * N]};  // price0 (lompc.py:164-170)
  const double lr = (ro.lmbd_r ? ro.lmbd_r : a.lmbd_r)[s];
  const int64_t cb = ro.tab + (int64_t)s * G;  // the set's first cell in the table
  const size_t sb = (size_t)cb * LQ_PPL;
  // ---- staging: every cell's count and coverage start; of the staged cells' USED slots the records
  //      and the piece ends (a cell's first t_cnt of its LQ_PPL)
  for (int c = tid; c < G; c += EVAL_EVS) {
    s_cnt[c] = a.t_cnt[cb + c];
    s_lo[c] = a.t_lo[cb + c];
  }
  for (int x = tid; x < np * 8; x += EVAL_EVS) {  // (x: double j = x & 7 of slot x >> 3)
    const int slot = x >> 3;
    const int nc = min(max(a.t_cnt[cb + slot / LQ_PPL], 0), LQ_PPL);
    if ((slot & (LQ_PPL - 1)) < nc) s_cf[cfx(slot, x & 7)] = a.t_cf[sb * 8 + x];
  }
  for (int x = tid; x < np; x += EVAL_EVS) {
    const int c = x / LQ_PPL, k = x & (LQ_PPL - 1);
    const int nc = min(max(a.t_cnt[cb + c], 0), LQ_PPL);
    if (k < nc) s_ge[k * Gs + c] = a.t_ge[sb + x];
  }
  __syncthreads();
  // ---- lane = EV: piece, scalar outputs; EVs no certified piece covers listed for the individual
  //      re-solve (counted as pending failures until then)
  const double ym = q.y_max, wm = __builtin_canonicalize(q.w_max);
  const double tt = q.theta * q.theta;
  const double cscale = (double)G / (whi - wlo);
  // the set's largest cell piece count: the lookup reads no piece end past it (wave-uniform)
  const int mxc = G <= 64 ? __builtin_amdgcn_readfirstlane((int)lqw::wave_max(lane < G ? (double)s_cnt[lane] : 0.0, 64)) : LQ_PPL;
  double acc_cost = 0.0, acc_p0 = 0.0, acc_w0 = 0.0, acc_err = 0.0;
  int n_ok = 0, n_inv = 0, nlist = 0;  // (wave-uniform counts: ballot + popcount per pass)
#pragma unroll
  for (int h = 0; h < EVAL_PASSES; ++h) {
    if (h > 0 && start + EVAL_EVS * h + 64 * wv >= end) break;  // a wave without EVs in a pass skips it
    const int i = start + tid + EVAL_EVS * h;
    const bool act = i < end;
    const double g = gh[h];
    const bool valid = act && g >= 0.0 && g <= ym;
    const int c = valid ? cell_of(g, wlo, cscale, G) : 0;
    const int nc = s_cnt[c];
    const int kb = c * LQ_PPL, ke = kb + nc;  // the cell's pieces [kb, ke), ascending gamma
    double ge[LQ_PPL];
#pragma unroll
    for (int k = 0; k < LQ_PPL; ++k) ge[k] = k < mxc ? s_ge[k * Gs + min(c, Gs - 1)] : 0.0;
    const double glo_c = s_lo[c];
    int key = kb;  // piece = number of piece ends below g
    double gend = ge[0];
#pragma unroll
    for (int k = 0; k + 1 < LQ_PPL; ++k) key += (k + 1 < nc && g > ge[k]) ? 1 : 0;
#pragma unroll
    for (int k = 1; k < LQ_PPL; ++k) gend = nc == k + 1 ? ge[k] : gend;  // the last piece's end
    const bool cov = valid && ke > kb && ke <= np && g >= glo_c && g <= gend;
    const bool inv = act && !valid;
    const unsigned long long need = __ballot(valid && !cov);
    if (valid && !cov) {
      st_wt4(a.fail_idx + rb * EVAL_MAXB + 64 * EVAL_PASSES * wv + nlist +
                 __popcll(need & ((1ull << lane) - 1ull)), i);
    }
    nlist += __popcll(need);
    n_inv += __popcll(__ballot(inv));
    n_ok += __popcll(__ballot(cov));
    if (inv) {
      if (acost) st_ev8(acost + i, NAN);
      if (aw0) st_ev8(aw0 + i, NAN);
      if (astatus) astatus[i] = LOMPC_QP_INVALID;
    } else if (cov) {
      const double2 q0 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 0));
      const double2 q1 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 2));
      const double2 q2 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 4));
      const double2 q3 = *reinterpret_cast<const double2*>(s_cf + cfx(key, 6));
      const double cst = fma(fma(q1.x, g, q0.y), g, q0.x);
      const double e2 = fma(fma(q2.y, g, q2.x), g, q1.y);
      const double er = a.want_err ? fmax(e2, 0.0) : 0.0;  // squared: sqrt of the max at the record
      const double w0v = clampw(fma(q3.y, g, q3.x), wm);
      const double p0 = q.theta * (w0v * l0[0] + (wm - w0v) * l0[1]) + q.q_scale * w0v * w0v * l0[2] +
                        tt * w0v * w0v * lr;  // lompc.py:164-170
      acc_cost += cst;
      acc_p0 += p0;
      acc_w0 += w0v;
      acc_err = fmax(acc_err, er);
      if (acost) st_ev8(acost + i, cst);
      if (aw0) st_ev8(aw0 + i, w0v);
      if (astatus) astatus[i] = LOMPC_QP_OK;
    }
  }
  // ---- records: per-wave totals (fixed lane order), the workgroup's in wave order
  {
    double tot[3] = {acc_cost, acc_p0, acc_w0};
    lqw::wave_totals(tot, 64);
    const double mx = a.want_err ? sqrt(lqw::wave_max(acc_err, 64)) : 0.0;
    if (lane == 0) {
      s_red[wv][PX_COST] = tot[0];
      s_red[wv][PX_PRICE0] = tot[1];
      s_red[wv][PX_MAX_ERR] = mx;
      s_red[wv][PX_N_OK] = (double)n_ok;
      s_red[wv][PX_N_REPAIRED] = 0.0;
      s_red[wv][PX_N_FAILED] = (double)nlist;
      s_red[wv][PX_N_INVALID] = (double)n_inv;
      s_red[wv][7] = tot[2];
      st_wt4(a.fail_cnt + rb * EVAL_WAVES + wv, nlist);
    }
  }
  __syncthreads();
  if (tid < N + NPX) {
    double v = 0.0;
    if (tid == 0) {
      for (int k = 0; k < EVAL_WAVES; ++k) v += s_red[k][7];
    } else if (tid >= N) {
      const int x = tid - N;
      for (int k = 0; k < EVAL_WAVES; ++k) v = x == PX_MAX_ERR ? fmax(v, s_red[k][x]) : v + s_red[k][x];
    }
    st_wt8(a.partial + rb * (N + NPX) + tid, v);
  }
}

__global__ __launch_bounds__(EVAL_EVS, LQ_SCALAR_MIN_WAVES) void k_scalar(EvalArgs a, int gs) {
  if (a.skip && *a.skip) return;
  scalar_block(a, gs, (int)blockIdx.x, RunOff{}, true);
}

// k_scalars: the scalar pass of the wide form (lompc_plan_run_steps with LOMPC_STEPS_SCALAR_PASS) — k_scalar's
// work for the x.nruns runs of a path group in ONE launch, one workgroup per (run, block): workgroup
// r x.nblk + b evaluates block b of run j = x.run0 + r from ring slot j % x.slots of the path tables, at run
// j's prices, into record slot r (k_eval's layout, so k_closes closes the group).  Not persistent over the
// runs: the pass is latency-bound (staging -> lookup -> stores) at a few KB of LDS, so the runs' workgroups
// share the CUs four at a time instead of queueing behind each other in a loop.  The runs of a launch are
// unordered: with one shared per-EV buffer (ev_stride 0) only run `last` (the call's last) stores per-EV
// outputs, the NaN / INVALID of invalid EVs included; the earlier runs write records and re-solve lists
// only (k_closes withholds their re-solved rows likewise).
__global__ __launch_bounds__(EVAL_EVS, LQ_SCALAR_MIN_WAVES) void k_scalars(EvalArgs a, EvalsArgs x, int gs, int last) {
  if (a.skip && *a.skip) return;
  const int r = (int)blockIdx.x / x.nblk, b = (int)blockIdx.x - r * x.nblk, j = x.run0 + r;
  RunOff ro;
  ro.tab = (int64_t)(j % x.slots) * x.SG;
  ro.rec = r * x.nblk;
  ro.ev = (int64_t)j * x.ev_stride;
  ro.lmbd = a.lmbd + (size_t)j * x.lm_stride;
  ro.lmbd_r = a.lmbd_r + (size_t)j * x.lr_stride;
  scalar_block(a, gs, b, ro, x.ev_stride != 0 || j == last);
}
