"""CPU selection of the committed cases of tests/price_step_cases.py and of the natural-loop seeds of
tests/test_gpu_price_step_cases.py.  Needs no GPU.

Section ``cases``: per cell of the grid (constants, N, r, lmbd_r flag) and family, the first seed in 1..200 at
which the host step (``lompc_price_step``) returns LOMPC_OK in the half the family is for — ``iterations > 64``
(the primal fallback ran) for the near families, ``<= 64`` for control.  Prints one line per cell — the seeds and
the host's iterations at them — then the cells of the coverage condition without a fallback case (there must be
none), the other cells without one, and whether the table equals price_step_cases.SEEDS; ``--table`` prints
the table as the module holds it.

Section ``loops``: whole price loops on a one-EV partition (shipped large constants, linear-convex prices, the
default tolerance), emulated on the CPU: the oracle LoMPC with the HOST price step, counting the steps whose
``iterations > 64``.  Per horizon the seeds 1..40 in turn until one passes scripts/check_price_loop_seeds.py's
knife-edge rule on the ORACLE's loop (dense step; every error before the exit above tol (1 + 1e-6), the exit's at
most tol (1 - 1e-6), below the cap), the emulated loop has the oracle's count and at least 3 of its steps fell
back.

    python scripts/select_price_step_cases.py [--table] [cases|loops ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("incentive-design-mpc_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import lompc_oracle as O  # noqa: E402
import price_oracle as PO  # noqa: E402
import price_step_cases as C  # noqa: E402

EDGE = 1e-6
LOOP_SEEDS = range(1, 41)


def cases(table):
    chosen, bad = {}, 0
    for cell in C.cells():
        picks = [C.select(cell, fam) for fam in C.FAMILIES]
        chosen[cell] = tuple(s for s, _ in picks)
        text = "  ".join(f"{fam} " + (f"seed {s:3d} it {it:4d}" if s is not None else "none in 1..200")
                         for fam, (s, it) in zip(C.FAMILIES, picks))
        cn, N, k, lf = cell
        print(f"{cn:5s} N={N:2d} r={k}N lr{lf}  {text}", flush=True)
    empty = [cell for cell in C.cells() if all(s is None for s in chosen[cell][:-1])]
    for cell in empty:
        need = C.required(cell)
        bad += need
        print(f"no fallback case: {cell}" + ("  REQUIRED by the coverage condition" if need else "  (control only)"))
    for cell in C.cells():
        if chosen[cell][-1] is None:
            print(f"no control case: {cell}")
            bad += 1
    n = sum(s is not None for v in chosen.values() for s in v)
    print(f"{n} cases; {sum(C.required(c) for c in C.cells())} required cells, "
          f"{sum(C.required(c) and c not in empty for c in C.cells())} with a fallback case")
    if table:
        for cell in C.cells():
            print(f"    {cell!r}: {chosen[cell]!r},")
    if chosen != C.SEEDS:
        print("price_step_cases.SEEDS differs from this selection")
        bad += 1
    else:
        print("price_step_cases.SEEDS equals this selection")
    return bad


def emulate(N, calls, host):
    """The oracle's loop over ``calls`` with the dense step, or (host) with lompc_price_step:
    [(iter, errors / tol, steps that fell back)]."""
    import test_gpu_price_step_cases as T

    c = O.large_consts()
    po = PO.OraclePriceSolver(N, c, T.NATURAL_PT)
    po.warm = True
    errs, fell = [], []
    inner = po._get_w_err

    def recording(*a, **k):
        res = inner(*a, **k)
        errs.append(res[2])
        return res

    def step(N_, r, th, wm, m, A_bar_inv, w_ref, w, lmbd):
        from lompc_amd import _lib
        import ctypes

        out = np.empty(r)
        dec, it = ctypes.c_double(), ctypes.c_int()
        kappa = max(np.linalg.inv(A_bar_inv)[-1, -1] - 1.0, 0.0)
        w_ref, w, lmbd = (np.ascontiguousarray(a, dtype=np.float64) for a in (w_ref, w, lmbd))
        rc = _lib.load().lompc_price_step(N_, r, th, wm, m, kappa, PO.EPS_REG, w_ref.ctypes.data, w.ctypes.data,
                                          lmbd.ctypes.data, out.ctypes.data, ctypes.byref(dec), ctypes.byref(it))
        assert rc == 0, rc
        fell.append(it.value > C.PDAS_ROUNDS)
        return out, dec.value

    po._get_w_err = recording
    dense = PO.price_step
    if host:
        PO.price_step = step
    out = []
    try:
        for y0, w_ref, lr in calls:
            errs.clear()
            fell.clear()
            po.set_charge_levels(y0)
            _, st = po.compute_optimal_prices(w_ref, lr)
            tol = O.get_robustness_bounds(N, c.delta, po.y0_rng, lr)[0]
            out.append((st["iter"], np.array(errs) / tol, int(sum(fell))))
    finally:
        PO.price_step = dense
    return out


def loops():
    import test_gpu_price_step_cases as T

    bad = 0
    for N in T.NATURAL_N:
        chosen = None
        for seed in LOOP_SEEDS:
            calls = T.natural_calls(N, seed)
            (it, ratio, _), = emulate(N, calls, host=False)
            (ith, _, fell), = emulate(N, calls, host=True)
            capped = it == PO.MAX_ITERS - 1 and ratio[-1] > 1.0
            edge = (ratio[:-1].size == 0 or ratio[:-1].min() > 1.0 + EDGE) and ratio[-1] <= 1.0 - EDGE
            ok = edge and not capped and ith == it and fell >= 3
            print(f"loop N={N} seed {seed:2d}: oracle iter {it:4d}, closest |err - tol| / tol {np.min(np.abs(ratio - 1.0)):9.3e}; "
                  f"host-step loop iter {ith:4d}, steps with iterations > 64: {fell:3d}  {'SELECTED' if ok else 'no'}",
                  flush=True)
            if ok:
                chosen = seed
                break
        if chosen != T.NATURAL_SEEDS.get(N):
            print(f"loop N={N}: NATURAL_SEEDS has {T.NATURAL_SEEDS.get(N)}, selected {chosen}")
            bad += 1
    return bad


def main(argv):
    which = [a for a in argv if not a.startswith("--")] or ["cases", "loops"]
    bad = 0
    if "cases" in which:
        bad += cases("--table" in argv)
    if "loops" in which:
        bad += loops()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
