"""CPU record for tests/test_gpu_constants.py: the reference side alone meets every condition the tests state.

For exactly the batches the tests use (test_gpu_constants.ConstBatch, built without a device), at every
(plan, N) and every run's prices:

* the C oracle (oracle/lompc_oracle.c) solves every EV of every set (nf == 0, asserted);
* the host path engine (oracle/path_cpu.cpp, oracle_c.path_run) at the plan's cell count fails none (asserted)
  and its w is compared with the oracle's.

Prints one line per (plan, N, context): per non-empty set at run 0 the pieces and the individually solved EVs
(at the plan's 16 cells, and for the 1100-EV set at 8 cells as well), and over all runs the largest
|dw| host-vs-oracle and the individually solved EVs in total.

Then the device price loop's seeds (LOOP_SEEDS): for each of the three constant sets the seeds 1..16 in turn
until one passes scripts/check_price_loop_seeds.py's criterion on BOTH calls (every average error before the
exit > tol (1 + 1e-6), the exit's <= tol (1 - 1e-6)), with the first call's oracle loop between 3 iterations
and the cap and the second below the cap.  Prints iterations and the closest |err - tol| / tol per call.

    python scripts/select_constants_cases.py [batches] [loops [A3 B0 ...]]

(constant sets named after ``loops``: probe those rows of the table instead of LOOP_SEEDS' own.)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("incentive-design-mpc_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import lompc_oracle as O  # noqa: E402
import oracle_c  # noqa: E402
import price_oracle as PO  # noqa: E402
import test_gpu_constants as T  # noqa: E402

EDGE = 1e-6
SEEDS = range(1, 17)


def host_set(bt, k, s, cells):
    """The host path engine on set s at run k: (w, pieces, individually solved)."""
    a, b = bt.off[s], bt.off[s + 1]
    o = oracle_c.path_run(bt.N, [bt.consts_of(s)], [1], bt.lm[k, s][None, :], bt.lr[k, s:s + 1], bt.gn[a:b],
                          np.array([0, b - a], dtype=np.int64), cells=cells, want_cost=False)
    assert int(o["info"][3]) == 0, (bt.label(s), k, o["info"])
    return o["w"], int(o["info"][0]), int(o["info"][2])


def batches():
    cells = T.plan_cells(max(T.SIZES))
    for plan, N in T.CASES:
        for layout in ("ragged", "sorted"):
            bt = T.ConstBatch(plan, N, layout, device=False)
            for k in range(T.K):
                bt.oracle(k)  # (asserts nf == 0 per set)
            if layout == "sorted":
                continue  # (the same gammas, each set sorted: the oracle solves them all, nothing more to print)
            for t in range(len(bt.cs)):
                run0, dw, solo_all = [], 0.0, 0
                for p, m in enumerate(T.SIZES):
                    if m == 0:
                        continue
                    s = t * bt.P + p
                    a, b = bt.off[s], bt.off[s + 1]
                    for k in range(T.K):
                        w, pieces, solo = host_set(bt, k, s, cells)
                        dw = max(dw, float(np.max(np.abs(w - bt.oracle(k)[0][a:b]))))
                        solo_all += solo
                        if k == 0:
                            run0.append(f"{m}: {pieces}/{solo}")
                _, p8, s8 = host_set(bt, 0, t * bt.P + T.BIG, 8)
                print(f"{plan}{t} N={N:2d}  run 0 pieces/individual per set  {', '.join(run0)}  (1100 at 8 cells: {p8}/{s8})  "
                      f"all runs: individual {solo_all}, max |dw| host-oracle {dw:.2e}", flush=True)


def loop_errors(c, calls):
    """The oracle's loops over ``calls``: [(iter, errors / tol)] (check_price_loop_seeds.loops)."""
    po = PO.OraclePriceSolver(T.LOOP_N, c, T.LOOP_PT)
    po.warm = True
    errs = []
    inner = po._get_w_err

    def recording(*a, **k):
        r = inner(*a, **k)
        errs.append(r[2])
        return r

    po._get_w_err = recording
    out = []
    for y0, w_ref, lr in calls:
        errs.clear()
        po.set_charge_levels(y0)
        _, st = po.compute_optimal_prices(w_ref, lr)
        tol = O.get_robustness_bounds(T.LOOP_N, c.delta, po.y0_rng, lr)[0]
        out.append((st["iter"], np.array(errs) / tol))
    return out


def loops(sets):
    bad = 0
    for plan, ctx in sets:
        c = T.PLANS[plan][ctx]
        chosen = None
        for seed in SEEDS:
            res = loop_errors(c, T.loop_calls(plan, ctx, seed))
            ok, text = True, []
            for call, (it, ratio) in enumerate(res):
                capped = it == PO.MAX_ITERS - 1 and ratio[-1] > 1.0
                before = ratio if capped else ratio[:-1]
                edge = (before.size == 0 or before.min() > 1.0 + EDGE) and (capped or ratio[-1] <= 1.0 - EDGE)
                ok = ok and edge and not capped and (call > 0 or it >= 3)
                text.append(f"call {call}: iter {it:4d} closest |err - tol| / tol {np.min(np.abs(ratio - 1.0)):9.3e}")
            print(f"loop {plan}{ctx} seed {seed:2d}  {'  '.join(text)}  {'SELECTED' if ok else 'no'}", flush=True)
            if ok:
                chosen = seed
                break
        if chosen != T.LOOP_SEEDS.get((plan, ctx)):
            print(f"loop {plan}{ctx}: LOOP_SEEDS has {T.LOOP_SEEDS.get((plan, ctx))}, selected {chosen}")
            bad += 1
    return bad


def main(argv):
    sets = [(a[0], int(a[1])) for a in argv if len(a) == 2 and a[0] in T.PLANS]  # (other rows of the table)
    which = [a for a in argv if len(a) != 2] or ["batches", "loops"]
    if "batches" in which:
        batches()
    return loops(sets or list(T.LOOP_SEEDS)) if "loops" in which else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
