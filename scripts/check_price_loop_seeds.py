"""CPU check of the seeds of tests/test_gpu_price_loop_shapes.py and tests/test_gpu_price_loop_exits.py:
for every (case, call) the oracle loop's iteration count must not sit on a knife-edge of its convergence
test.

The oracle's iterates before the exit do not depend on the tolerance, so its count is unchanged
under tol -> tol (1 +- 1e-6) exactly when every error before the exit is above tol (1 + 1e-6) and the
exit's error is at most tol (1 - 1e-6) (a loop that ends at the iteration cap has no exit error).
Prints one line per call — iterations, the closest error / tol ratio, oracle seconds — and exits
non-zero if any call is on the edge.  ``--literal`` also reruns every loop with the tolerance scaled
both ways and compares the counts (three times the time).

Section ``exits`` (tests/test_gpu_price_loop_exits.py): the three calls of every cap configuration at the
default cap (a loop stopped by a cap K takes the first K of the same steps, so it needs nothing more; the
line of the third call prints the n of the K in {n - 1, n, n + 1} cases), with the counts the test asserts
(first call above 20, third call 3..5); the "max" configurations under "max", where the error tested is
the oracle's w_err_max, and under "avg" on the same inputs (the first calls' counts must differ).  A
"max" configuration must also have a call whose count would change if the maximum were taken over the
lower half of the set's gamma window alone (the first closing round's cells of a 32-cell plan): an
iteration before the exit at which that partial maximum is already below the tolerance.  And the
chain's partitions under its cap (the middle one stopped by it, the outer ones at least two below it).

    python scripts/check_price_loop_seeds.py [--literal] [cells|horizon|shapes|exits ...]
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
import test_gpu_price_loop_exits as X  # noqa: E402
import test_gpu_price_loop_shapes as T  # noqa: E402

EDGE = 1e-6


def loops(N, ev, pt, calls, scale=1.0, tol_type="avg", max_iters=None):
    """The oracle's loops over ``calls`` with its tolerance scaled: [(iter, errors / tol, seconds, lower)].
    tol_type "max": the loop tests, and this records, w_err_max, and ``lower`` is the same maximum over
    the EVs in the lower half of the set's gamma window alone, / tol (else None); max_iters: the
    oracle's cap."""
    c, _ = T.consts(ev)
    po = PO.OraclePriceSolver(N, c, pt)
    po.warm = True
    po.tol_type = tol_type
    errs, lower, last = [], [], {}
    inner, batch = po._get_w_err, po._batch

    def keeping(*a, **k):
        last["W"] = batch(*a, **k)
        return last["W"]

    def recording(lmbd, lmbd_r, w_ref, A_bar, **k):
        r = inner(lmbd, lmbd_r, w_ref, A_bar, **k)
        errs.append(r[0] if tol_type == "max" else r[2])
        if tol_type == "max":
            g = c.y_max - po.y0
            dv = last["W"][g <= 0.5 * (g.min() + g.max())] - w_ref
            lower.append(float(np.max(np.sqrt(np.einsum("bi,bi->b", dv @ A_bar, dv)))))
        return r

    po._get_w_err, po._batch = recording, keeping
    bounds = O.get_robustness_bounds
    PO.O.get_robustness_bounds = lambda *a, **k: tuple(scale * x for x in bounds(*a, **k))
    out = []
    cap = PO.MAX_ITERS
    if max_iters is not None:
        PO.MAX_ITERS = max_iters
    try:
        for y0, w_ref, lr in calls:
            errs.clear()
            lower.clear()
            po.set_charge_levels(y0)
            t0 = time.perf_counter()
            _, st = po.compute_optimal_prices(w_ref, lr)
            dt = time.perf_counter() - t0
            tol = scale * bounds(N, c.delta, po.y0_rng, lr)[0]
            out.append((st["iter"], np.array(errs) / tol, dt, np.array(lower) / tol if tol_type == "max" else None))
    finally:
        PO.O.get_robustness_bounds = bounds
        PO.MAX_ITERS = cap
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


def exits_cases():
    """(name, N, ev, pt, calls, loops' keywords, check of the loops' results or None)."""
    for cfg, (ev, pt, N) in X.CONFIGS.items():
        yield (f"exits cap {cfg}", N, ev, pt, X.cap_calls(cfg), {},
               lambda res: res[0][0] > 20 and 3 <= res[2][0] <= 5)
    first = {}
    for cfg in X.MAX_CONFIGS:
        ev, pt, N = X.CONFIGS[cfg]
        for tt in ("max", "avg"):
            def differ(res, cfg=cfg, tt=tt):
                first[cfg, tt] = res[0][0]
                if tt == "avg":
                    return first[cfg, "max"] != res[0][0]
                halves = [bool(np.any(lo[:it] <= 1.0 - EDGE)) for it, _, _, lo in res]
                print(f"exits max {cfg}: calls whose count needs the upper half of the window: {halves}")
                return any(halves)
            yield f"exits {tt} {cfg}", N, ev, pt, X.max_calls(cfg), {"tol_type": tt}, differ
    K = X.K_CHAIN
    for cfg in X.TWO_CONFIGS:
        ev, pt, N = X.CONFIGS[cfg]
        yield (f"exits chain K={K} {cfg}", N, ev, pt, X.chain_calls(cfg), {"max_iters": K},
               lambda res, K=K: res[0][0] < K - 1 and res[1][0] == K - 1 and res[2][0] < K - 1)


def main(argv):
    literal = "--literal" in argv
    which = [a for a in argv if not a.startswith("--")] or ["cells", "horizon", "shapes", "exits"]
    bad = 0
    todo = [(*x, {}, None) for x in cases(which)] + (list(exits_cases()) if "exits" in which else [])
    for name, N, ev, pt, calls, kw, counts_ok in todo:
        res = loops(N, ev, pt, calls, **kw)
        alt = [loops(N, ev, pt, calls, 1.0 + s * EDGE, **kw) for s in (-1, 1)] if literal else []
        if counts_ok is not None and not counts_ok(res):
            print(f"{name:44s} COUNTS {[r[0] for r in res]} are not what the test needs", flush=True)
            bad += 1
        for k, (it, ratio, dt, _) in enumerate(res):
            capped = it == kw.get("max_iters", PO.MAX_ITERS) - 1 and ratio.size == it + 1 and ratio[-1] > 1.0
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
