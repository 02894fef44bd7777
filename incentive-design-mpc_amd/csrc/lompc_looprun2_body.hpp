// lompc_looprun2_body.hpp — the body of the persistent price loop's wave, a FRAGMENT included inside
// k_loop_run2 and k_loop_runs (lompc_plan.hip) and nowhere else, so the loop's arithmetic exists once.
// It is shared as text, not as a __device__ function: called through a function, even a force-inlined
// one, the optimiser first sees the body on its own and k_loop_run2 comes out as an equivalent kernel
// with other operand orders, another schedule and other registers; included, k_loop_run2's
// instructions are exactly those of the kernel written in one piece.
// In scope at the include: NT (the horizon, 0: run time), S (= 2), pa (PathArgs), ga (AggArgs), sa
// (StepArgs), rec (the loop's cell records), blk (the wave's index among its loop's S * G), lane, G.
  const int s = blk / G, c = blk - s * G;
  const bool writer = blk == 0;
  int cl_n[S], cl_v[S], cl_ok[S];
#pragma unroll
  for (int t = 0; t < S; ++t) {
    const int4 si = ga.sinfo[t];
    cl_n[t] = (int)(ga.set_off[t + 1] - ga.set_off[t]);
    cl_v[t] = si.x;
    cl_ok[t] = si.y;
    asm volatile("" : "+v"(cl_n[t]), "+v"(cl_v[t]), "+v"(cl_ok[t]));
  }
  AggArgs gw = ga;  // (the closing's outputs: wave 0's only)
  if (!writer) {
    gw.set_sum_w = nullptr;
    gw.set_stats = nullptr;
    gw.stats = nullptr;
    gw.tally = nullptr;
  }
  const int nsg = S * G;
  StepIn in;
  step_prices<false>(sa, lane, in);  // (the first call's prices, w_ref, the zeroed loop state)
  double pv[3] = {in.lm[0], in.lm[1], in.lm[2]};
  // the cell's stored working set, kept in a register from call to call (as each call stores it);
  // w_ref from the price buffer (the plan's w_ref of both sets, constant over the loop)
  const int N_ = NT ? NT : pa.N;
  const double wr_c = (pa.w_ref && lane < N_) ? pa.w_ref[(size_t)s * N_ + lane] : 0.0;
  int wsr = pa.ws ? (int)pa.ws[(size_t)blk * 64 + lane] : 0;
  for (int m = 0; m <= sa.max_iter; ++m) {
    // (the box table in LDS: written by the first call; the one-wave workgroup keeps its LDS)
    if (m == 0) path_cell<NT, true, true, true>(pa, blk, pv[0], pv[1], pv[2], wr_c, &wsr);
    else path_cell<NT, false, true, true>(pa, blk, pv[0], pv[1], pv[2], wr_c, &wsr);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the cell's tables have reached L2
    double* rb = rec + (size_t)(m & 1) * (nsg + 1) * LQ_AGG_REC;  // this call's record buffer
    {
      AggSet z = agg_set_init<NT, true>(ga, s);
      if (m > 0) {  // (the prices of this call: registers)
        z.preg = true;
        z.p1 = pv[0];
        z.p2 = pv[1];
        z.p3 = pv[2];
        z.l1 = lqw::readlane_d(pv[0], 0);
        z.l2 = lqw::readlane_d(pv[1], 0);
        z.l3 = lqw::readlane_d(pv[2], 0);
      }
      AggPart ap;
      if (z.order_ok) agg_cell<NT, true, true>(ga, z, s, c, agg_cell_range(z, c), lane, ap);
      const AggRec x = agg_wave_record(ap);
      double* rc = rb + (size_t)blk * LQ_AGG_REC;
      if (lane < z.N) st_wt8(rc + lane, ap.accw);
      if (lane < 5) st_wt8(rc + LOMPC_MAX_N + lane, x.pick(lane));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int ok = 1;
    if (lane == 0) {
      __hip_atomic_fetch_add(sa.ctl + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int target = (m + 1) * nsg;
      int spins = 0;
      while (__hip_atomic_load(sa.ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
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
    AggSet zs[S];
#pragma unroll
    for (int t = 0; t < S; ++t) {
      zs[t].N = NT ? NT : ga.N;
      zs[t].n_s = cl_n[t];
      zs[t].si = make_int4(cl_v[t], cl_ok[t], 0, 0);
      zs[t].order_ok = cl_ok[t] != 0;
    }
    const int N = zs[0].N;
    const int tl = min(lane, N - 1), xl = min(lane, 4);
    // the records in cell order, 16 of each set per memory round (records k >= G: the zero record
    // after buffer 0; with G <= 16 one round, the sums of k_loop_run's padded 16)
    double v[S] = {0.0, 0.0}, xs[S] = {0.0, 0.0}, xm[S] = {0.0, 0.0};
    for (int k0 = 0; k0 < G; k0 += LQ_LOOP_G) {  // (wave-uniform)
      double rw[S][LQ_LOOP_G], rx[S][LQ_LOOP_G];
#pragma unroll
      for (int t = 0; t < S; ++t)
#pragma unroll
        for (int k = 0; k < LQ_LOOP_G; ++k) {
          const double* rk =
              k0 + k < G ? rb + (size_t)(t * G + k0 + k) * LQ_AGG_REC : rec + (size_t)nsg * LQ_AGG_REC;
          rw[t][k] = ld_t<true>(rk + tl);
          rx[t][k] = ld_t<true>(rk + LOMPC_MAX_N + xl);
        }
#pragma unroll
      for (int t = 0; t < S; ++t)
#pragma unroll
        for (int k = 0; k < LQ_LOOP_G; ++k) {
          v[t] += rw[t][k];
          xs[t] += rx[t][k];
          xm[t] = fmax(xm[t], rx[t][k]);
        }
    }
    AggSetOut o[S];
#pragma unroll
    for (int t = 0; t < S; ++t) o[t] = agg_finish_tail<false>(gw, zs[t], t, lane, v[t], xs[t], xm[t]);
    in.s0 = o[0].sumw;
    in.wk = o[1].sumw;
    in.emax = lqw::readlane_d(o[0].stat, LOMPC_STAT_MAX_ERR);
    in.cost_c = lqw::readlane_d(o[1].stat, LOMPC_STAT_SUM_COST);
    in.n_inv = lqw::readlane_d(o[0].stat, LOMPC_STAT_N_INVALID) + lqw::readlane_d(o[1].stat, LOMPC_STAT_N_INVALID);
    in.n_fail = lqw::readlane_d(o[0].stat, LOMPC_STAT_N_FAILED) + lqw::readlane_d(o[1].stat, LOMPC_STAT_N_FAILED);
    StepOut so;
    if (writer) loop_step_core<NoStamp, NoRelease, true>(sa, m, lane, in, NoStamp{}, NoRelease{}, &so);
    else loop_step_core<NoStamp, NoRelease, false>(sa, m, lane, in, NoStamp{}, NoRelease{}, &so);
    if (so.fin) return;
    // the next call's inputs: what the step stored, kept in registers
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      pv[k] = so.v[k];
      in.lm[k] = so.v[k];
    }
    in.dc = so.cost_c;
    in.dterm = so.dterm;
    in.ab = so.ab;
  }
