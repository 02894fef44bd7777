"""Diagnostic: L independent price loops in one lompc_price_loops call against L single loops in sequence.

Every loop is of config 5's partition size (175 000 small EVs on levels 0.05 y_max wide, N = 48, 6 cells,
"linear-convex"), has a tolerance no error reaches (eps_tol = -1: the convergence test never passes) and
the cap at 200, so every loop takes exactly 200 steps (201 engine calls) around its fixed point.  Per L: the wall time of one
compute_optimal_prices_parallel call over L staged partitions of one solver (from zero prices), median
/ min / max of R repetitions, divided by 200 as us per iteration, set against L times the single loop
(compute_optimal_prices_chain over one partition: lompc_price_loop, one k_loop_run2 launch) measured
in the same process.

    python scripts/loops_timing.py [reps] [--single-only] [--ls 1,2,6,12,24] [--max-parts K]

--single-only measures the single loop alone and uses nothing a library without lompc_price_loops
lacks (LOMPC_LIB: a variant build).
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "incentive-design-mpc_amd"), os.path.join(ROOT, "oracle")]
import lompc_oracle as O  # noqa: E402
from lompc_amd import LoMPCConstants, settings  # noqa: E402
from lompc_amd.price_solver import PriceSolver  # noqa: E402

argv = sys.argv[1:]
single_only = "--single-only" in argv
LS = [int(x) for x in argv[argv.index("--ls") + 1].split(",")] if "--ls" in argv else [1, 2, 6, 12, 24]
MAX_PARTS = int(argv[argv.index("--max-parts") + 1]) if "--max-parts" in argv else 0
R = int(argv[0]) if argv and argv[0].isdigit() else 7
N, NEV, STEPS = 48, 175_000, 200

settings.PRINT_LEVEL = 0
settings.MAX_PRICE_SOLVER_ITERATIONS = STEPS
c = O.small_consts()
ps = PriceSolver(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), "linear-convex", device=0)
ps.eps_tol = -1.0  # (tol = sqrt(N) y0_rng + eps_tol < 0: unreachable)
rng = np.random.default_rng(5)
w_ref = c.w_max * (0.2 + 0.6 * rng.random(N))
n_parts = 1 if single_only else max(LS)
for p in range(n_parts):
    y0 = np.sort((0.45 + 0.05 * rng.random(NEV)) * c.y_max)[::-1].copy()
    ps.stage_partition(p, torch.as_tensor(y0, device="cuda:0"), NEV, float(y0.max()), float(y0.min()), float(y0.sum()),
                       descending=True)
torch.cuda.synchronize()


def timed(fn):
    ts = []
    for r in range(R + 1):  # (the first repetition warms up: allocations, the plans' first loop)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = fn()
        torch.cuda.synchronize()
        if r:
            ts.append(time.perf_counter() - t0)
        assert all(s == STEPS for s in steps), steps  # (every loop ran to the cap)
    ts = np.array(ts) * 1e6 / STEPS
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def single():
    ps.prev_prices = np.zeros(ps.r)
    (lm, st), = ps.compute_optimal_prices_chain([0], w_ref[None, :], 0.0)
    return [len(st["dual_cost_decrease_actual"])]


s_med, s_min, s_max = timed(single)
print(f"single loop (lompc_price_loop): {s_med:.2f} us per iteration (min {s_min:.2f}, max {s_max:.2f}; {R} reps)",
      flush=True)
if not single_only:
    from lompc_amd.price_solver import compute_optimal_prices_parallel  # noqa: E402

    for L in LS:
        jobs = [(ps, p, w_ref, np.zeros(ps.r)) for p in range(L)]

        def batched():
            res = compute_optimal_prices_parallel(jobs, 0.0, max_parts_per_launch=MAX_PARTS)
            return [len(st["dual_cost_decrease_actual"]) for _, st in res]

        med, lo, hi = timed(batched)
        print(f"L {L:3d}: {med:8.2f} us per iteration (min {lo:.2f}, max {hi:.2f}); sequential {L * s_med:8.2f}; "
              f"ratio batched / sequential {med / (L * s_med):.3f}; per loop {med / L:.2f}", flush=True)
