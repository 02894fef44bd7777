"""lompc_price_loops: L independent price loops in one call, those the persistent form takes as shared
``k_loop_runs`` launches (csrc/lompc_plan.hip, csrc/lompc_loop.hip), and
``price_solver.compute_optimal_prices_parallel`` on top of it.

The contract under test: every part's outputs carry the BITS of ``lompc_price_loop`` on the same inputs,
whatever the other parts are and however the call is split into launches.  So the reference of every
part is the single loop on a FRESH identical plan (a new PriceSolver on the same levels), and every
comparison is bitwise: iterations, prices, w_k, dual cost, the ``iterations`` decreases, errs.  One call
is also checked against the CPU oracle loop with the bars of test_gpu_price_solver.py's
test_compute_optimal_prices_matches_oracle (``compare_oracle`` of test_gpu_price_loop_shapes.py) on
inputs whose seeds that file committed (``horizon_calls`` at N = 13: not on a knife-edge of the count).

Every part is one PriceSolver: its plan, and its own price block (the solver's ``_in`` / ``_h_in``, on
whose w_ref view the plan was created, so the reference w of the single loop and of the batched form
coincide).  Populations are at most 700 EVs and loops at most a few hundred iterations: every case runs
in well under a second on the GPU.  Nothing here provokes a fault or a time-out.
"""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Guarded
from lompc_amd import _lib, settings
from lompc_amd.price_solver import compute_optimal_prices_parallel
from test_gpu_price_loop_exits import counted
from test_gpu_price_loop_shapes import compare_oracle, consts, horizon_calls, oracle_horizon, solver, stage

pytestmark = pytest.mark.gpu

SEED = 3100
CAP = 1000  # settings.MAX_PRICE_SOLVER_ITERATIONS' default
OUT_KEYS = ("it", "calls", "lm", "w_k", "dual", "dec", "errs")


class Spec:
    """One loop's inputs; build() makes a fresh solver (plan + price block) on them."""

    def __init__(self, N, ev, pt, cells, y0, w_ref, lr=0.0, start=None, max_iter=CAP, device_loop=True, bad=None,
                 tol=None, lc=None):
        self.N, self.ev, self.pt, self.cells = N, ev, pt, cells
        self.y0, self.w_ref, self.lr, self.max_iter, self.device_loop, self.bad = y0, w_ref, lr, max_iter, device_loop, bad
        self.tol = tol  # the loop's tolerance instead of get_robustness_bounds' (loop_args)
        self.lc = lc    # LoMPCConstants other than the shipped set ``ev`` names
        self.r = (2 if pt == "linear" else 3) * N
        self.start = np.zeros(self.r) if start is None else np.asarray(start, dtype=np.float64)[: self.r].copy()

    def but(self, **kw):
        s = Spec(self.N, self.ev, self.pt, self.cells, self.y0, self.w_ref, self.lr, self.start, self.max_iter,
                 self.device_loop, self.bad, self.tol, self.lc)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def build(self):
        lc = consts(self.ev)[1] if self.lc is None else self.lc
        ps = solver(self.N, lc, self.pt, self.cells, device_loop=self.device_loop)
        set_levels(ps, self)
        return ps


def set_levels(ps, spec):
    if spec.bad is None:
        ps.set_charge_levels(spec.y0)
    else:  # (statistics that pass the host check over device levels that do not: test_invalid_level's form)
        y0 = spec.y0
        ps.set_charge_levels_stats(torch.as_tensor(spec.bad, device="cuda:0"), len(y0), float(y0.max()),
                                   float(y0.min()), float(y0.sum()), descending=False)


def make(N, ev, pt, cells, nev, seed, lo=0.35, width=0.04, robust=False, **kw):
    c, _ = consts(ev)
    rng = np.random.default_rng(SEED + seed)
    y0 = (lo + width * rng.random(nev)) * c.y_max
    w_ref = c.w_max * (0.2 + 0.6 * rng.random(N))
    return Spec(N, ev, pt, cells, y0, w_ref, lr=1.5 * N * c.delta if robust else 0.0, **kw)


def loop_args(ps, spec, dev_in=None, host_in=None, dev_sw=None, dev_st=None, tol=None):
    """lompc_price_loop_args as PriceSolver._native_loop fills them: (args, what they point to).  ``tol`` (or
    the spec's) replaces the tolerance of get_robustness_bounds."""
    tol = spec.tol if tol is None else tol
    if tol is None:
        tol, _ = ps.get_robustness_bounds(spec.lr)
    A_bar, A_bar_inv = ps._get_w_inner_product_metric(spec.lr)
    A_bar = np.ascontiguousarray(A_bar, dtype=np.float64)
    w_ref = np.ascontiguousarray(spec.w_ref, dtype=np.float64)
    args = _lib.PriceLoopArgs(
        ps.N, ps.r, spec.max_iter, 1, float(ps.consts.theta), float(ps.consts.w_max), float(ps.m),
        float(ps._kappa_of(A_bar_inv)), float(ps.eps_reg), float(tol), float(ps.nEVs), float(spec.lr),
        A_bar.ctypes.data, w_ref.ctypes.data, ps._in.data_ptr() if dev_in is None else dev_in,
        ps._h_in.data_ptr() if host_in is None else host_in,
        ps._plan.out["set_sum_w"].data_ptr() if dev_sw is None else dev_sw,
        ps._plan.out["set_stats"].data_ptr() if dev_st is None else dev_st, ps._h_sw.data_ptr(), ps._h_st.data_ptr(),
        None, 1 if ps.device_loop else 0)
    return args, (A_bar, w_ref)


class Out:
    """A part's host outputs, pre-filled: prices with the start, everything else with NaN."""

    def __init__(self, spec):
        self.lm = np.zeros(3 * spec.N)
        self.lm[: spec.r] = spec.start
        self.w_k = np.full(spec.N, np.nan)
        self.dec = np.full((2, spec.max_iter), np.nan)

    def untouched(self, spec):
        return (np.array_equal(self.lm[: spec.r], spec.start) and not self.lm[spec.r:].any()
                and np.isnan(self.w_k).all() and np.isnan(self.dec).all())


def result(rc, it, calls, out, dual, errs, pre=None, post=None):
    n = max(calls - 1, 0) if rc == 0 else 0
    return {"rc": rc, "it": it, "calls": calls, "lm": out.lm, "w_k": out.w_k, "dual": dual, "dec": out.dec[:, :n].copy(),
            "errs": np.array(errs), "pre": pre, "post": post, "out": out}


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_single(spec, ps=None):
    """lompc_price_loop on a fresh identical plan (or on ``ps``)."""
    ps = spec.build() if ps is None else ps
    args, keep = loop_args(ps, spec)
    out = Out(spec)
    dual, it = ctypes.c_double(np.nan), ctypes.c_int(-1)
    errs = np.full(3, np.nan)
    rc = ps._lib.lompc_price_loop(ps._plan._plan, ctypes.byref(args), out.lm.ctypes.data, out.w_k.ctypes.data,
                                  ctypes.byref(dual), out.dec[0].ctypes.data, out.dec[1].ctypes.data, ctypes.byref(it),
                                  errs.ctypes.data, stream())
    torch.cuda.synchronize()
    return result(rc, it.value, it.value + 1, out, dual.value, errs)


def fill_parts(specs, solvers, regularize=0, blocks=None):
    n = len(specs)
    arr = (_lib.PriceLoopsPart * n)()
    keep, outs = [], []
    for k, (spec, ps) in enumerate(zip(specs, solvers)):
        args, kp = loop_args(ps, spec, **(blocks[k] if blocks else {}))
        out = Out(spec)
        keep.append((args, kp))
        outs.append(out)
        q = arr[k]
        q.plan, q.args = ps._plan._plan.value, ctypes.addressof(args)
        q.lmbd, q.w_k = out.lm.ctypes.data, out.w_k.ctypes.data
        q.dec_actual, q.dec_pred = out.dec[0].ctypes.data, out.dec[1].ctypes.data
        q.regularize = regularize
        q.rc = q.iterations = q.calls = -7
    return arr, keep, outs


def run_batched(specs, solvers=None, regularize=0, mppl=0, blocks=None):
    """One lompc_price_loops call: (rc, launches, [result per part], solvers)."""
    solvers = [s.build() for s in specs] if solvers is None else solvers
    arr, keep, outs = fill_parts(specs, solvers, regularize, blocks)
    launches = ctypes.c_int(-1)
    rc = solvers[0]._lib.lompc_price_loops(len(specs), ctypes.cast(arr, ctypes.c_void_p), mppl, ctypes.byref(launches),
                                           stream())
    torch.cuda.synchronize()
    res = [result(q.rc, q.iterations, q.calls, out, q.dual_cost, list(q.errs), q.price_before_reg, q.price_after_reg)
           for q, out in zip(arr, outs)]
    return rc, launches.value, res, solvers


def assert_bits(got, want, what=""):
    assert got["rc"] == want["rc"] == 0, (what, got["rc"], want["rc"])
    for k in OUT_KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, got[k], want[k])


def persistent_launches(specs):
    """The launches of a call: one per (N, r, cells) among the parts the persistent form takes."""
    return len({(s.N, s.r, s.cells) for s in specs if s.device_loop and s.cells <= 32})


# ------------------------------------------------------------------ bits against single loops
def mixed_specs():
    """Seven loops of three shapes — (N 12, r 2N, 6 cells), (N 13: the runtime-N instantiation, r 3N, 1
    cell), (N 48, r 3N, 20 cells: the two-round closing) — both EV types inside each shape, 1 / 65 / 700
    EVs, and lengths from no step at all (start = a previous run's converged prices) over the one or two
    steps of levels spread over the whole range to the long loop of a single EV."""
    a = [make(12, "small", "linear", 6, 700, 1), make(12, "large", "linear", 6, 65, 2),
         make(12, "small", "linear", 6, 1, 3)]
    b = [make(13, "large", "linear-convex", 1, 700, 4, lo=0.0, width=1.0), make(13, "small", "linear-convex", 1, 65, 5)]
    c = [make(48, "small", "linear-convex", 20, 700, 6, robust=True), make(48, "large", "linear-convex", 20, 65, 7)]
    b[1] = b[1].but(start=run_single(b[1])["lm"])
    return a + b + c


@pytest.mark.parametrize("L", [1, 2, 7])
def test_bits_against_single_loops(gpu, monkeypatch, L):
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = mixed_specs()[:L] if L < 7 else mixed_specs()
    want = [run_single(s) for s in specs]
    rc, launches, got, _ = run_batched(specs)
    assert rc == 0 and launches == persistent_launches(specs) == {1: 1, 2: 1, 7: 3}[L], (rc, launches)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_bits(g, w, f"part {k}")
    its = [w["it"] for w in want]
    if L >= 2:
        assert len(set(its)) > 1, its  # (loops of different lengths in one call)
    if L == 7:
        assert its[4] == 0, its  # (no step at all)
        pos = [i for i in its if i > 0]
        assert max(pos) >= 3 * min(pos), its


# ------------------------------------------------------------------ the oracle
def test_oracle(gpu, monkeypatch):
    """L = 3 in one launch (N 13, r 2N, 6 cells), both EV types, regularised as the solver does: the first
    calls of test_gpu_price_loop_shapes.py's horizon_calls from zero prices and the small type's second call
    from the oracle's first prices, each against the oracle started from the same prices."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    N, pt = 13, "linear"
    cases = [("small", 0), ("large", 0), ("small", 1)]
    specs, orc = [], []
    for ev, call in cases:
        y0, w_ref, lr = horizon_calls(N, ev, pt)[call]
        o = oracle_horizon(N, ev, pt)
        start = None if call == 0 else o[call - 1][0]
        specs.append(Spec(N, ev, pt, 6, y0, w_ref, lr, start=start))
        orc.append(o[call])
    rc, launches, got, solvers = run_batched(specs, regularize=1)
    assert rc == 0 and launches == 1
    for spec, ps, g, o in zip(specs, solvers, got, orc):
        c, _ = consts(spec.ev)
        st = {"iter": g["it"], "price_before_reg": g["pre"], "price_after_reg": g["post"],
              "dual_cost_decrease_actual": g["dec"][0], "dual_cost_decrease_predicted": g["dec"][1]}
        compare_oracle(ps, (g["lm"], st), o, spec.lr, c)
    assert max(g["it"] for g in got) >= 3


# ------------------------------------------------------------------ per-part cap, split, mixed forms
def same_shape(n, **kw):
    return [make(12, ("small", "large")[k % 2], "linear", 6, (700, 65, 300)[k % 3], 20 + k, **kw) for k in range(n)]


def test_per_part_cap(gpu, monkeypatch):
    """max_iter is per part: one part stopped at 5 steps (below its natural count) beside uncapped ones."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = same_shape(3)
    natural = run_single(specs[1])["it"]
    assert natural > 5
    specs[1] = specs[1].but(max_iter=5)
    want = [run_single(s) for s in specs]
    assert want[1]["it"] == 5 and want[0]["it"] > 5 and want[2]["it"] > 5
    rc, launches, got, _ = run_batched(specs)
    assert rc == 0 and launches == 1
    for k, (g, w) in enumerate(zip(got, want)):
        assert_bits(g, w, f"part {k}")
    # regularised, the capped part reports the reference's loop variable (max_iter - 1), as the chain does
    rc, _, reg, _ = run_batched(specs, regularize=1)
    assert rc == 0 and reg[1]["it"] == 4 and reg[1]["calls"] == 6 and reg[0]["it"] == want[0]["it"]


def test_split(gpu, monkeypatch):
    """L = 5 of one shape: one launch, or three with at most 2 parts per launch — the same bits."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = same_shape(5)
    rc1, l1, one, _ = run_batched(specs)
    rc3, l3, three, _ = run_batched(specs, mppl=2)
    assert (rc1, l1, rc3, l3) == (0, 1, 0, 3)
    for k, (a, b) in enumerate(zip(one, three)):
        assert_bits(a, b, f"part {k}")
    assert_bits(one[3], run_single(specs[3]), "part 3 against the single loop")


def test_mixed_forms(gpu, monkeypatch):
    """A part of 40 cells (the unfused device loop) and one with device_loop = 0 (the host loop) run
    beside two the persistent form takes: all right, and *launches counts the persistent launch only."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = same_shape(4)
    specs[1] = specs[1].but(cells=40)
    specs[2] = specs[2].but(device_loop=False)
    want = [run_single(s) for s in specs]
    solvers = [s.build() for s in specs]
    (rc, launches, got, _), n = counted(solvers[1]._plan, lambda: run_batched(specs, solvers))
    assert rc == 0 and launches == 1
    assert solvers[1]._plan.info()["cells"] == 40 and n["k_eval"] >= got[1]["calls"], n  # (the unfused form ran)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_bits(g, w, f"part {k}")


# ------------------------------------------------------------------ a failing part
def test_failing_part(gpu, monkeypatch):
    """The middle part holds a level above y_max behind statistics that pass the host check: its rc is
    LOMPC_ERR_INVALID_ARG (the call's too), its plan's error text names gamma and it writes no output; the
    other parts are bitwise right; the same plans, the level repaired, then give fresh-plan bits."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = same_shape(3)
    c, _ = consts(specs[1].ev)
    bad = specs[1].y0.copy()
    bad[17] = c.y_max + 1e-3
    broken = [specs[0], specs[1].but(bad=bad), specs[2]]
    want = [run_single(s) for s in specs]
    arr_rc, launches, got, solvers = run_batched(broken)
    assert arr_rc == _lib.LOMPC_ERR_INVALID_ARG and launches == 1
    assert [g["rc"] for g in got] == [0, _lib.LOMPC_ERR_INVALID_ARG, 0]
    assert "gamma" in solvers[1]._lib.lompc_plan_last_error(solvers[1]._plan._plan).decode()
    assert got[1]["out"].untouched(specs[1])
    for k in (0, 2):
        assert_bits(got[k], want[k], f"part {k} beside the failing one")
    set_levels(solvers[1], specs[1])  # the level repaired: the same plan re-targeted
    rc, launches, again, _ = run_batched(specs, solvers)
    assert rc == 0 and launches == 1
    for k, (g, w) in enumerate(zip(again, want)):
        assert_bits(g, w, f"part {k} after the failure")


# ------------------------------------------------------------------ refusals and extents
def test_refusals(gpu, monkeypatch):
    """Each refusal gives LOMPC_ERR_INVALID_ARG with every output untouched: the parts' host arrays, their
    out fields and *launches."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = same_shape(2)
    solvers = [s.build() for s in specs]
    lib = solvers[0]._lib
    word = 8 * (8 * specs[0].N + 2)

    def refused(n, edit):
        arr, keep, outs = fill_parts(specs, solvers)
        edit(arr, keep)
        launches = ctypes.c_int(-1)
        rc = lib.lompc_price_loops(n, ctypes.cast(arr, ctypes.c_void_p), 0, ctypes.byref(launches), stream())
        torch.cuda.synchronize()
        assert rc == _lib.LOMPC_ERR_INVALID_ARG and launches.value == -1, (rc, launches.value)
        for q, out, spec in zip(arr, outs, specs):
            assert out.untouched(spec) and (q.rc, q.iterations, q.calls) == (-7, -7, -7)

    def field(k, name, value):
        return lambda arr, keep: setattr(arr[k], name, value)

    def arg(k, name, value):
        return lambda arr, keep: setattr(keep[k][0], name, value(keep) if callable(value) else value)

    refused(-1, lambda arr, keep: None)
    for name in ("plan", "args", "lmbd", "w_k"):
        refused(2, field(1, name, None))
    for name in ("A_bar", "w_ref", "dev_in", "host_in", "dev_sw", "dev_st", "host_sw", "host_st"):
        refused(2, arg(1, name, None))
    refused(2, field(1, "plan", solvers[0]._plan._plan.value))  # the same plan twice
    refused(2, arg(1, "dev_in", lambda keep: keep[0][0].dev_in + word - 8))  # dev_in ranges overlap by one element
    refused(2, arg(1, "host_in", lambda keep: keep[0][0].host_in + 8 * specs[0].N))  # host_in ranges overlap
    # (the plans are untouched: the call they were built for still gives the single loops' bits)
    rc, launches, got, _ = run_batched(specs, solvers)
    assert rc == 0 and launches == 1
    for k, g in enumerate(got):
        assert_bits(g, run_single(specs[k]), f"part {k}")


def test_extents(gpu, monkeypatch):
    """A passing L = 3 call on guard-banded price blocks and set outputs: every band around every part's
    dev_in [8N + 2], dev_sw [2, N] and dev_st [2, 8] is intact, the outputs are written, and the bits are
    the single loops'."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = same_shape(3)
    N = specs[0].N
    gb = Guarded()
    for k in range(3):
        gb.inp(f"in{k}", np.zeros(8 * N + 2))
        gb.out(f"sw{k}", (2, N))
        gb.out(f"st{k}", (2, _lib.LOMPC_SET_STATS))
    gb.build()
    solvers = []
    for k, spec in enumerate(specs):
        _, lc = consts(spec.ev)
        ps = solver(spec.N, lc, spec.pt, spec.cells)
        ps._in = gb.view(f"in{k}")  # (the plan is created on this block's w_ref view)
        ps._lm2, ps._lr2, ps._wr2 = ps._in[: 6 * N].view(2, 3 * N), ps._in[6 * N: 6 * N + 2], ps._in[6 * N + 2:].view(2, N)
        set_levels(ps, spec)
        solvers.append(ps)
    blocks = [{"dev_in": gb.ptr(f"in{k}"), "dev_sw": gb.ptr(f"sw{k}"), "dev_st": gb.ptr(f"st{k}")} for k in range(3)]
    rc, launches, got, _ = run_batched(specs, solvers, blocks=blocks)
    assert rc == 0 and launches == 1
    gb.check_bands()
    for k in range(3):
        gb.check_written(f"sw{k}")
        gb.check_written(f"st{k}")
        assert_bits(got[k], run_single(specs[k]), f"part {k}")


# ------------------------------------------------------------------ Python
def test_compute_optimal_prices_parallel(gpu, monkeypatch):
    """Partitions of a small-EV and a large-EV solver in one call, from the caller's start prices, against
    each partition run alone through compute_optimal_prices with prev_prices set to the same start: equal
    prices and stats, the solvers' prev_prices unchanged, one native call."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    N, pt = 12, "linear-convex"
    rng = np.random.default_rng(SEED + 90)
    sizes = {0: 700, 1: 65, 3: 1}
    sol, levels = {}, {}
    for ev in ("small", "large"):
        c, lc = consts(ev)
        levels[ev] = {p: np.sort((0.3 + 0.1 * p + 0.04 * rng.random(n)) * c.y_max)[::-1].copy() for p, n in sizes.items()}
        sol[ev] = solver(N, lc, pt, 6)
        for p, y0 in levels[ev].items():
            stage(sol[ev], p, y0)
        sol[ev].prev_prices = np.full(sol[ev].r, 0.125)
    jobs = []
    for ev in ("small", "large"):
        c, _ = consts(ev)
        for p in sizes:
            start = np.zeros(3 * N) if p != 1 else 0.05 * c.theta * rng.random(3 * N)
            jobs.append((sol[ev], p, c.w_max * (0.2 + 0.6 * rng.random(N)), start))
    with pytest.raises(ValueError, match="not staged"):
        compute_optimal_prices_parallel([(sol["small"], 2, jobs[0][2], jobs[0][3])], 0.0)
    calls = []
    lib = sol["small"]._lib
    inner = lib.lompc_price_loops
    monkeypatch.setattr(lib, "lompc_price_loops", lambda *a: (calls.append(1), inner(*a))[1])
    n0 = {ev: sol[ev].n_batched_calls for ev in sol}
    res = compute_optimal_prices_parallel(jobs, 0.0)
    assert len(calls) == 1 and len(res) == len(jobs)
    made = {ev: 0 for ev in sol}
    for (ps, p, w_ref, start), (lm, st) in zip(jobs, res):
        ev = "small" if ps is sol["small"] else "large"
        _, lc = consts(ev)
        alone = solver(N, lc, pt, 6)
        stage(alone, p, levels[ev][p])
        alone.use_partition(p)
        alone.prev_prices = start.copy()
        lm1, st1 = alone.compute_optimal_prices(w_ref, 0.0)
        assert lm.shape == lm1.shape == (3 * N,) and lm.tobytes() == lm1.tobytes(), (ev, p)
        assert st.keys() == st1.keys()
        for k in st:
            assert np.ascontiguousarray(st[k]).tobytes() == np.ascontiguousarray(st1[k]).tobytes(), (ev, p, k)
        made[ev] += alone.n_batched_calls
    for ev in sol:
        assert np.array_equal(sol[ev].prev_prices, np.full(sol[ev].r, 0.125))
        assert sol[ev].n_batched_calls - n0[ev] == made[ev]
