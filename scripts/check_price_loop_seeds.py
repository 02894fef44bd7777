"""CPU check of the seeds of tests/test_gpu_price_loop_shapes.py: for every (case, call) the oracle
loop's iteration count must not sit on a knife-edge of its convergence test.

The oracle's iterates before the exit do not depend on the tolerance, so its count is unchanged
under tol -> tol (1 +- 1e-6) exactly when every error before the exit is above tol (1 + 1e-6) and the
exit's error is at most tol (1 - 1e-6) (a loop that ends at the iteration cap has no exit error).
Prints one line per call — iterations, the closest error / tol ratio, oracle seconds — and exits
non-zero if any call is on the edge.  ``--literal`` also reruns every loop with the tolerance scaled
both ways and compares the counts (three times the time).

    python scripts/check_price_loop_seeds.py [--literal] [cells|horizon|shapes ...]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("incentive-design-mpc_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import lompc_oracle as O  # noqa: E402
import price_oracle as PO  # noqa: E402
import test_gpu_price_loop_shapes as T  # noqa: E402

EDGE = 1e-6


def loops(N, ev, pt, calls, scale=1.0):
    """The oracle's loops over ``calls`` with its tolerance scaled: [(iter, errors / tol, seconds)]."""
    c, _ = T.consts(ev)
    po = PO.OraclePriceSolver(N, c, pt)
    po.warm = True
    errs = []
    inner = po._get_w_err

    def recording(*a, **k):
        r = inner(*a, **k)
        errs.append(r[2])
        return r

    po._get_w_err = recording
    bounds = O.get_robustness_bounds
    PO.O.get_robustness_bounds = lambda *a, **k: tuple(scale * x for x in bounds(*a, **k))
    out = []
    try:
        for y0, w_ref, lr in calls:
            errs.clear()
            po.set_charge_levels(y0)
            t0 = time.perf_counter()
            _, st = po.compute_optimal_prices(w_ref, lr)
            dt = time.perf_counter() - t0
            tol = scale * bounds(N, c.delta, po.y0_rng, lr)[0]
            out.append((st["iter"], np.array(errs) / tol, dt))
    finally:
        PO.O.get_robustness_bounds = bounds
    return out


def cases(which):
    if "cells" in which:
        for cfg, (ev, pt, N) in T.CELL_CONFIGS.items():
            yield f"cells {cfg}", N, ev, pt, [(y0[:T.N_ORACLE], w, lr) for y0, w, lr in T.cells_calls(cfg)]
    if "horizon" in which:
        for N in sorted({n for n, _ in T.HORIZON_CASES}):
            for ev in T.EVS:
                for pt in T.PTS:
                    yield f"horizon N{N} {ev} {pt}", N, ev, pt, T.horizon_calls(N, ev, pt)
    if "shapes" in which:
        for shape in T.SHAPES:
            for ev in T.EVS:
                for robust in (False, True):
                    yield f"shapes {shape} {ev} robust={robust}", 24, ev, "linear-convex", T.shape_calls(shape, ev, robust)


def main(argv):
    literal = "--literal" in argv
    which = [a for a in argv if not a.startswith("--")] or ["cells", "horizon", "shapes"]
    bad = 0
    for name, N, ev, pt, calls in cases(which):
        res = loops(N, ev, pt, calls)
        alt = [loops(N, ev, pt, calls, 1.0 + s * EDGE) for s in (-1, 1)] if literal else []
        for k, (it, ratio, dt) in enumerate(res):
            capped = it == PO.MAX_ITERS - 1 and ratio[-1] > 1.0
            before = ratio if capped else ratio[:-1]
            ok = (before.size == 0 or before.min() > 1.0 + EDGE) and (capped or ratio[-1] <= 1.0 - EDGE)
            for a in alt:
                ok = ok and a[k][0] == it
            near = np.min(np.abs(ratio - 1.0))
            print(f"{name:44s} call {k}: iter {it:4d}  closest |e/tol - 1| {near:9.3e}  {dt:6.2f} s  "
                  f"{'ok' if ok else 'KNIFE-EDGE'}", flush=True)
            bad += not ok
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
