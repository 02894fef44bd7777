"""The price loop's other ends.  Every other loop test ends because the average error falls below the
tolerance; here the loop ends at the iteration cap, under the "max" tolerance type, or with an error,
and the same plan then runs an ordinary loop.

What runs (csrc/lompc_loop.hip, csrc/lompc_loopstep.hpp, csrc/lompc_plan.hip, lompc_amd/price_solver.py):
the device loop in its three forms — PERSISTENT at 6 cells (``k_loop_run2``, one closing round) and at 32
(two rounds), UNFUSED at 33 (k_path + k_agg + ``k_loop_step`` per call, enqueued LOMPC_LOOP_AHEAD = 2
calls past the device's progress) — at N in {12, 24} (``k_loop_run2<N>``) and N = 20 (``k_loop_run2<0>``),
both EV types with their price types; the host C++ loop (``device_loop = False``) and the Python loop
(``native_loop = False``).  Every device case asserts its form (``assert_form``, ``assert_launches``:
persistent = one k_path-timed launch and no k_eval-timed one; unfused = exactly
min(cap, finishing call + LOMPC_LOOP_AHEAD) + 1 launch pairs, a number that depends on the finishing call
alone).  All populations are 600 EVs, so every run is checked against the oracle too.

1. The cap (``settings.MAX_PRICE_SOLVER_ITERATIONS = K``, the oracle's ``MAX_ITERS = K``).  With
   ``steps`` the price steps taken, min(natural count, K): ``iter == min(steps, K - 1)`` (the reference's
   loop variable after ``for iter in range(K)``, so a loop stopped by the cap reports K - 1 after K steps),
   engine calls = steps + 1, both decrease arrays of length ``steps``.  K in {1, 2, 3, 5} on a first call
   (1 and 2 are at or below LOMPC_LOOP_AHEAD, 3 the first above it), and K in {n - 1, n, n + 1} on a warm
   third call of natural count n.  Then: one chain (``lompc_price_chain``) whose middle partition is
   stopped by the cap; the cap changing 3 -> 1000 -> 3 on one solver (the pinned decrease buffer
   ``[2][max_iter]`` growing, then read with a shorter row than it was allocated for); and K = 3 on the
   world-1 RCCL group of test_gpu_comm.py (unfused with the collective).
2. ``settings.PRICE_SOLVER_TOL_TYPE = "max"``: three consecutive calls; the loop's length then depends on
   LOMPC_STAT_MAX_ERR, which a loop plan takes from each certified piece's error quadratic at the piece's
   extreme EVs and the persistent kernel closes from the cell records; the three errors of the exit's
   test (``lompc_price_loop``'s errs) are also compared with the oracle's.
4. The error ends: a level above y_max and a NaN behind statistics that pass the host check
   (AssertionError, the plan's tally counts both), an unsorted set handed over as sorted (SolverError), and
   the C entry's refusals (nothing launched).
5. After every cap and error case the same solver runs a converging loop on valid levels: bit for bit a
   fresh solver's prices, count, decreases and get_w0_price0, and ``lompc_plan_status`` (read once after
   the earlier loop, as its contract asks: the tallies are sticky until read) counts that loop alone.

Bars (the suite's existing ones; nothing new): device against host loop — equal ``iter`` and engine
calls, prices within 1e-9 theta, decreases at rtol 1e-8 (atol 1e-8 of the largest), prices before / after
regularisation within 1e-9 relative (test_gpu_price_solver.py's test_device_loop_matches_host_loop), and
``lompc_price_loop``'s errs[3] within 1e-9; engine against oracle — ``compare_oracle`` of
test_gpu_price_loop_shapes.py (equal ``iter``, prices within 1e-6 theta, or per component within
1e-6 max(theta, |lambda_i|) where the oracle's loop is longer than 100, stats within 1e-6, decrease arrays
of equal shape, get_w0_price0 within 1e-6).  "Equal to a fresh solver" is bit for bit: the device loop is
deterministic.

Seeds (scripts/check_price_loop_seeds.py, section ``exits``; the rule of test_gpu_price_loop_shapes.py:
every error before the exit above tol (1 + 1e-6), the exit's at most tol (1 - 1e-6), a capped loop needs
only the first; the "max" cases test the oracle's w_err_max).  The oracle's counts at the committed seeds:
cap configurations, calls 1..3 at the default cap (the third is the n of K = n - 1, n, n + 1) — small
linear N 12: 50, 14, 4; large linear-convex N 12: 36, 1, 4; small N 24: 58, 17, 4; large N 24: 30, 15, 3;
small N 20: 34, 23, 4; large N 20: 38, 4, 3 (closest error / tolerance ratio 1.8e-4 from 1).  "max", and
"avg" on the same inputs — small N 12: 48, 22, 4 against 41, 13, 4; large N 12: 91, 53, 5 against 57, 1, 5;
small N 24: 55, 24, 5 against 31, 13, 4; large N 24: 33, 51, 6 against 26, 14, 4 (closest 6.4e-4); in each
the second call's count under "max" would be lower if the maximum were taken over the lower half of the
gamma window alone (the first closing round's cells at 32), which the script checks.  The
chain under K_CHAIN = 8 — small N 24: 4, 7 (stopped; 62 uncapped), 3; large N 20: 5, 7 (stopped; 33), 1
(closest 3.1e-4).

Left out: err = 3 (a price QP without a certificate) — no input is known that reaches it, and none is
searched for on the GPU (the price QP's primal fallback, the half of it that runs when the primal-dual active
set does not end, is steered and checked in test_gpu_price_step_cases.py: it certifies on every case there);
world sizes above 1 (one GPU: the RCCL path runs at world size 1).
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import price_oracle as PO
from lompc_amd import BatchPlan, _lib, settings
from lompc_amd.lompc import SolverError
from test_gpu_comm import nccl1  # noqa: F401  (the world-1 RCCL group; skips where it skips)
from test_gpu_price_loop_shapes import (assert_form, assert_same_results, compare_host, compare_oracle, consts,
                                        run_loop, solver, spread_calls, stage)

pytestmark = pytest.mark.gpu

SEED_CAP = 2100
# (per configuration: seeds at which one call's count under "max" needs the cells of the second closing round)
SEED_MAX = {"small-linear-N12": 2207, "large-linear-convex-N12": 2200, "small-linear-N24": 2257,
            "large-linear-convex-N24": 2203}
SEED_CHAIN = 2300
NEV = 600
AHEAD = 2  # LOMPC_LOOP_AHEAD (include/lompc_amd.h)
DEFAULT_CAP = 1000  # settings.py:14

CONFIGS = {f"{ev}-{pt}-N{N}": (ev, pt, N)
           for N in (12, 24, 20) for ev, pt in (("small", "linear"), ("large", "linear-convex"))}
MAX_CONFIGS = [k for k, v in CONFIGS.items() if v[2] in (12, 24)]
TWO_CONFIGS = ["small-linear-N24", "large-linear-convex-N20"]  # (k_loop_run2<24>, k_loop_run2<0>)
FORMS = (6, 32, 33)
FORM_IDS = {6: "G6-persistent-1round", 32: "G32-persistent-2rounds", 33: "G33-unfused"}
K_CHAIN = 8


# ------------------------------------------------------------------ inputs (pure functions of the case)
def _seed(base, cfg):
    ev, pt, N = CONFIGS[cfg]
    return base + 4 * N + 2 * (ev == "large")


def cap_calls(cfg):
    """Three calls: the first is section 1's capped first call, the third its warm short call, the
    second section 5's converging loop."""
    ev, pt, N = CONFIGS[cfg]
    return spread_calls(_seed(SEED_CAP, cfg), ev, N, NEV, 3)


def max_calls(cfg):
    ev, pt, N = CONFIGS[cfg]
    return spread_calls(SEED_MAX[cfg], ev, N, NEV, 3)


def chain_calls(cfg):
    """Three partitions in descending charge level, [(levels descending, w_ref, 0.0)]: a narrow middle
    one (a long loop) between two wide ones (short loops)."""
    ev, pt, N = CONFIGS[cfg]
    c, _ = consts(ev)
    rng = np.random.default_rng(_seed(SEED_CHAIN, cfg))
    out = []
    for base, width in ((0.60, 0.12), (0.50, 0.015), (0.32, 0.12)):
        y0 = np.sort((base + width * rng.random(NEV)) * c.y_max)[::-1].copy()
        out.append((y0, c.w_max * (0.2 + 0.6 * rng.random(N)), 0.0))
    return out


# ------------------------------------------------------------------ the oracle, once per input set
def oracle_seq(cfg, calls, tol_type="avg", cap=None, start=None):
    """The oracle's loops over ``calls`` on one solver: [((prices, stats, w0, price0), prices before,
    (w_err_max, w0_err, w_avg_err) of the loop's last convergence test)]."""
    ev, pt, N = CONFIGS[cfg]
    c, _ = consts(ev)
    po = PO.OraclePriceSolver(N, c, pt)
    po.warm = True
    po.tol_type = tol_type
    if start is not None:
        po.prev_prices = start.copy()
    tested, inner = [], po._get_w_err
    po._get_w_err = lambda *a, **k: (tested.append(inner(*a, **{**k, "want_max": True})), tested[-1])[1]
    out = []
    old = PO.MAX_ITERS
    PO.MAX_ITERS = old if cap is None else cap
    try:
        for y0, w_ref, lr in calls:
            before = po.prev_prices.copy()
            po.set_charge_levels(y0)
            lmo, sto = po.compute_optimal_prices(w_ref, lr)
            lmo = lmo.copy()
            w0o, p0o = po.get_w0_price0_batch(lmo[: po.r], lr)
            out.append(((lmo, sto, w0o, p0o), before, np.array(tested[-1])))
    finally:
        PO.MAX_ITERS = old
    return out


@functools.lru_cache(maxsize=None)
def oracle_natural(cfg):
    return oracle_seq(cfg, cap_calls(cfg))


@functools.lru_cache(maxsize=None)
def oracle_capped(cfg, call, K):
    """Call ``call`` of cap_calls stopped at K, after the earlier calls at the default cap."""
    return oracle_seq(cfg, [cap_calls(cfg)[call]], cap=K, start=oracle_natural(cfg)[call][1])[0][0]


@functools.lru_cache(maxsize=None)
def oracle_max(cfg, tol_type):
    return [(r, e) for r, _, e in oracle_seq(cfg, max_calls(cfg), tol_type=tol_type)]


@functools.lru_cache(maxsize=None)
def oracle_chain(cfg):
    return [r for r, _, _ in oracle_seq(cfg, chain_calls(cfg), cap=K_CHAIN)]


# ------------------------------------------------------------------ running and comparing
@contextlib.contextmanager
def cap(K):
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(settings, "MAX_PRICE_SOLVER_ITERATIONS", K)
        yield


def quiet(monkeypatch):
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)


def plan_status(ps):
    """lompc_plan_status of the solver's loop plan: (repaired, failed, invalid) since the last read."""
    rep, fail, inv = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    plan = ps._plan
    rc = ps._lib.lompc_plan_status(plan._plan, plan._stream, ctypes.byref(rep), ctypes.byref(fail), ctypes.byref(inv))
    assert rc == _lib.LOMPC_OK
    return rep.value, fail.value, inv.value


def counted(plan, fn):
    """fn() with the plan's launches counted: (fn's result or the exception it raised, {k_path, k_eval})."""
    kern = ("k_path", "k_eval")
    plan.profile(enable=kern)
    for k in kern:
        plan.profile(read=True, reset=True, kernel=k)
    try:
        res = fn()
    except (AssertionError, SolverError, ValueError) as e:
        res = e
    n = {k: plan.profile(read=True, kernel=k)[1] for k in kern}
    plan.profile(enable=False)
    return res, n


def assert_launches(n, cells, calls, max_iter):
    """The launches of one device loop that made ``calls`` engine calls: one for the persistent form;
    the unfused form enqueues call j for every j <= min(max_iter, finishing call + AHEAD), whatever the
    host saw of the device's progress in between (lompc_loop.hip)."""
    if cells <= 32:
        assert n == {"k_path": 1, "k_eval": 0}, n
    else:
        want = min(max_iter, calls - 1 + AHEAD) + 1
        assert n == {"k_path": want, "k_eval": want}, (n, want)


def raw_loop(ps, start, w_ref, lr, max_iter, tol_type="avg", plan=None, r=None, n_evs=None):
    """lompc_price_loop called as PriceSolver._native_loop calls it, on the solver's current plan and
    levels from the prices ``start``: (rc, steps, prices, decreases, errs)."""
    plan = ps._plan if plan is None else plan
    tol, _ = ps.get_robustness_bounds(lr)
    A_bar, A_bar_inv = ps._get_w_inner_product_metric(lr)
    A_bar = np.ascontiguousarray(A_bar, dtype=np.float64)
    w_ref = np.ascontiguousarray(w_ref, dtype=np.float64)
    args = _lib.PriceLoopArgs(
        ps.N, ps.r if r is None else r, max_iter, 1 if tol_type != "max" else 0, float(ps.consts.theta),
        float(ps.consts.w_max), float(ps.m), float(ps._kappa_of(A_bar_inv)), float(ps.eps_reg), float(tol),
        float(ps.nEVs if n_evs is None else n_evs), float(lr), A_bar.ctypes.data, w_ref.ctypes.data,
        ps._in.data_ptr(), ps._h_in.data_ptr(), ps._plan.out["set_sum_w"].data_ptr(),
        ps._plan.out["set_stats"].data_ptr(), ps._h_sw.data_ptr(), ps._h_st.data_ptr(), None,
        1 if ps.device_loop else 0)
    lm = np.zeros(3 * ps.N)
    lm[: ps.r] = start
    w_k = np.empty(ps.N)
    n_dec = max(max_iter, 1)
    dec = np.full((2, n_dec), np.nan)
    dual, it = ctypes.c_double(0.0), ctypes.c_int(-1)
    errs = np.full(3, np.nan)
    with torch.cuda.stream(ps._stream):
        rc = ps._lib.lompc_price_loop(plan._plan, ctypes.byref(args), lm.ctypes.data, w_k.ctypes.data, ctypes.byref(dual),
                                      dec[0].ctypes.data, dec[1].ctypes.data, ctypes.byref(it), errs.ctypes.data,
                                      ps._stream.cuda_stream)
        ps._stream.synchronize()
    return rc, it.value, lm, dec[:, : max(it.value, 0)], errs


def compare_capped(dev, host, theta, K, steps):
    """compare_host for a loop under the cap K that took ``steps`` price steps.  compare_host's
    ``calls == iter + 1`` does not hold at the cap: a loop the cap stops reports iter = K - 1 (the
    reference's loop variable) after K steps and K + 1 engine calls, so calls = iter + 2 there."""
    (ld, sd, nd, _), (lh, sh, nh, kh) = dev, host
    assert nd == nh == steps + 1, (nd, nh, steps)
    assert sd["iter"] == sh["iter"] == min(steps, K - 1), (sd["iter"], sh["iter"], steps, K)
    assert kh["k_eval"] == kh["k_path"] == steps + 1, kh  # (the host loop: one engine call per launch pair)
    np.testing.assert_allclose(ld, lh, rtol=0, atol=1e-9 * theta)
    for k in ("dual_cost_decrease_actual", "dual_cost_decrease_predicted"):
        assert sd[k].shape == sh[k].shape == (steps,), (k, sd[k].shape, sh[k].shape, steps)
        np.testing.assert_allclose(sd[k], sh[k], rtol=1e-8, atol=1e-8 * np.max(np.abs(sh[k]), initial=1.0), err_msg=k)
    for k in ("price_before_reg", "price_after_reg"):
        assert abs(sd[k] - sh[k]) <= 1e-9 * max(1.0, abs(sh[k])), (k, sd[k], sh[k])


def warm(ps, calls):
    for y0, w_ref, lr in calls:
        ps.set_charge_levels(y0)
        ps.compute_optimal_prices(w_ref, lr)


def same_bits(a, b):
    """Two run_loop results, bit for bit."""
    assert a[2] == b[2], (a[2], b[2])
    assert_same_results([(a[0], a[1])], [(b[0], b[1])])
    for k in ("dual_cost_decrease_actual", "dual_cost_decrease_predicted"):
        assert a[1][k].shape == b[1][k].shape, k


def loop_after(ps, cfg, cells):
    """Section 5: after a loop that ended at the cap or with an error, the same solver (same plan) runs
    cap_calls' second call, a converging loop on valid levels, at the default cap.  It equals a fresh
    solver started from the same prices bit for bit, and the plan's tallies, read once after the earlier
    loop, then count this loop alone."""
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    y0, w_ref, lr = cap_calls(cfg)[1]
    plan_status(ps)  # (the earlier loop's tallies: sticky until read)
    fresh = solver(N, lc, pt, cells, device_loop=ps.device_loop)
    fresh.prev_prices = ps.prev_prices.copy()
    res = []
    for s in (ps, fresh):
        r = run_loop(s, y0, w_ref, lr)
        tally = plan_status(s)
        w0, p0 = s.get_w0_price0(r[0][: s.r], lr)
        res.append((r, tally, w0, p0))
    (ra, ta, w0a, p0a), (rf, tf, w0f, p0f) = res
    assert ra[2] == ra[1]["iter"] + 1 < DEFAULT_CAP  # (converged: not the cap, no error)
    if ps.device_loop:
        assert_form(ps, ra[1], ra[3], cells)
        assert_launches(ra[3], cells, ra[2], DEFAULT_CAP)
    same_bits(ra, rf)
    assert ra[3] == rf[3], (ra[3], rf[3])
    assert ta == tf and ta[1:] == (0, 0), (ta, tf)
    np.testing.assert_array_equal(w0a, w0f)
    assert p0a == p0f


def capped_case(cfg, before, call, K, orc, steps):
    """One call under the cap K after the calls ``before`` at the default cap: the three device forms
    against the host loop and the oracle, the Python loop against the oracle, errs[3] device against
    host, then section 5 on every device solver and on the host solver."""
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    y0, w_ref, lr = call
    assert orc[1]["iter"] == min(steps, K - 1)
    for cells in FORMS:
        dev, host = solver(N, lc, pt, cells), solver(N, lc, pt, cells, device_loop=False)
        res, start = {}, {}
        for name, ps in (("dev", dev), ("host", host)):
            warm(ps, before)
            start[name] = ps.prev_prices.copy()
            with cap(K):
                res[name] = run_loop(ps, y0, w_ref, lr)
        rd, rh = res["dev"], res["host"]
        assert_form(dev, rd[1], rd[3], cells)
        assert_launches(rd[3], cells, rd[2], K)
        compare_capped(rd, rh, c.theta, K, steps)
        compare_oracle(dev, rd, orc, lr, c)
        compare_oracle(host, rh, orc, lr, c)
        # the C entry itself, from the same prices: steps, decreases and the three errors
        raw = {name: raw_loop(ps, start[name], w_ref, lr, K) for name, ps in (("dev", dev), ("host", host))}
        for name in raw:
            assert raw[name][:2] == (_lib.LOMPC_OK, steps), (name, raw[name][:2])
        np.testing.assert_array_equal(raw["dev"][3], np.stack([rd[1]["dual_cost_decrease_actual"],
                                                               rd[1]["dual_cost_decrease_predicted"]]))
        ed, eh = raw["dev"][4], raw["host"][4]
        assert np.all(np.abs(ed - eh) <= 1e-9 * np.maximum(1.0, np.abs(eh))), (ed, eh)
        loop_after(dev, cfg, cells)
        if cells == FORMS[0]:
            loop_after(host, cfg, cells)
    py = solver(N, lc, pt, FORMS[0])
    py.native_loop = False
    warm(py, before)
    with cap(K):
        rp = run_loop(py, y0, w_ref, lr)
    assert rp[2] == steps + 1 and rp[1]["iter"] == min(steps, K - 1), (rp[2], rp[1]["iter"])
    assert rp[3]["k_path"] == rp[3]["k_eval"] == steps + 1, rp[3]  # (one plan run per engine call)
    for k in ("dual_cost_decrease_actual", "dual_cost_decrease_predicted"):
        assert rp[1][k].shape == (steps,), k
    compare_oracle(py, rp, orc, lr, c)


# ------------------------------------------------------------------ 1. the cap
@pytest.mark.parametrize("K", [1, 2, 3, 5], ids=lambda k: f"K{k}")
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_cap_below_convergence(gpu, monkeypatch, cfg, K):
    """A first call whose natural count is above 20, stopped after K steps: K = 1 and 2 are at or below
    LOMPC_LOOP_AHEAD (the unfused form enqueues every call of the loop before the first has run), 3 is
    the first above it."""
    quiet(monkeypatch)
    assert oracle_natural(cfg)[0][0][1]["iter"] > 20
    orc = oracle_capped(cfg, 0, K)
    assert orc[1]["iter"] == K - 1 and orc[1]["dual_cost_decrease_predicted"].shape == (K,)
    capped_case(cfg, [], cap_calls(cfg)[0], K, orc, K)


@pytest.mark.parametrize("dK", [-1, 0, 1], ids=["K=n-1", "K=n", "K=n+1"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_cap_around_the_natural_count(gpu, monkeypatch, cfg, dK):
    """The warm third call, of natural count n in 3..5 (asserted from the oracle), under K = n - 1 (the
    cap stops it one step early), K = n (n steps, and the reference's loop ends without its convergence
    test: iter = n - 1) and K = n + 1 (the first cap it does not feel: iter = n)."""
    quiet(monkeypatch)
    calls = cap_calls(cfg)
    n = oracle_natural(cfg)[2][0][1]["iter"]
    assert 3 <= n <= 5, n
    K = n + dK
    capped_case(cfg, calls[:2], calls[2], K, oracle_capped(cfg, 2, K), min(n, K))


@pytest.mark.parametrize("cells", [6, 33], ids=[FORM_IDS[6], FORM_IDS[33]])
@pytest.mark.parametrize("cfg", TWO_CONFIGS)
def test_chain_with_a_capped_partition(gpu, monkeypatch, cfg, cells):
    """lompc_price_chain over three staged partitions under K_CHAIN, which stops the middle one: its
    iter = K - 1, calls = K + 1 and decrease slices of length K, the outer ones converge below the cap;
    bit for bit the per-partition loops (so the third starts from the capped one's regularised prices —
    also run on its own from them), counts equal to the oracle's."""
    quiet(monkeypatch)
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    parts, K = [0, 1, 2], K_CHAIN
    calls = chain_calls(cfg)
    w_refs = np.stack([w for _, w, _ in calls])
    orc = oracle_chain(cfg)
    want_iter = [o[1]["iter"] for o in orc]
    want_steps = [o[1]["dual_cost_decrease_predicted"].shape[0] for o in orc]
    assert want_steps[1] == K and want_iter[1] == K - 1 and want_steps[0] == want_iter[0] < K - 1 \
        and want_steps[2] == want_iter[2] < K - 1, (want_iter, want_steps)
    sol = {}
    for mode in ("loops", "chain", "third"):
        ps = solver(N, lc, pt, cells)
        for p in parts:
            stage(ps, p, calls[p][0])
        ps.prev_prices = np.zeros(ps.r)
        sol[mode] = ps
    with cap(K):
        loops = []
        for p in parts:
            sol["loops"].use_partition(p)
            (lm, st), n = counted(sol["loops"]._plan, lambda: sol["loops"].compute_optimal_prices(w_refs[p], 0.0))
            assert sol["loops"]._plan.info()["cells"] == cells
            assert_launches(n, cells, st["dual_cost_decrease_predicted"].shape[0] + 1, K)
            loops.append((lm.copy(), st))
        ps = sol["chain"]
        assert ps.chain_ok(parts)
        n0 = ps.n_batched_calls
        plans = [ps._staged[p]["_plan"] for p in parts]
        chain, n = counted(plans[1], lambda: [(lm.copy(), st) for lm, st in
                                              ps.compute_optimal_prices_chain(parts, w_refs, 0.0)])
        assert plans[1].info()["cells"] == cells
        assert_launches(n, cells, K + 1, K)  # (the capped partition's loop, in the chain)
        assert ps.n_batched_calls - n0 == sum(want_steps) + len(parts)
        # the third partition alone, from the capped partition's regularised prices
        sol["third"].prev_prices = chain[1][0][: ps.r].copy()
        sol["third"].use_partition(2)
        lm3, st3 = sol["third"].compute_optimal_prices(w_refs[2], 0.0)
    assert_same_results(loops, chain)
    assert_same_results([(lm3, st3)], [chain[2]])
    np.testing.assert_array_equal(ps.prev_prices, chain[2][0][: ps.r])
    for p in parts:
        st = chain[p][1]
        assert st["iter"] == want_iter[p], (p, st["iter"], want_iter)
        for k in ("dual_cost_decrease_actual", "dual_cost_decrease_predicted"):
            assert st[k].shape == (want_steps[p],) == loops[p][1][k].shape, (p, k, st[k].shape, want_steps)
        np.testing.assert_allclose(chain[p][0], orc[p][0], rtol=0, atol=1e-6 * c.theta)
    for p in parts:  # section 5 on the chain's plans: each runs an ordinary loop afterwards
        ps.use_partition(p)
        loop_after(ps, cfg, cells)


@pytest.mark.parametrize("cells", FORMS, ids=[FORM_IDS[g] for g in FORMS])
@pytest.mark.parametrize("cfg", TWO_CONFIGS)
def test_cap_changing_on_one_solver(gpu, monkeypatch, cfg, cells):
    """One solver under K = 3, then the default 1000, then 3 again (the pinned decrease buffer grows at
    the second loop, and the third reads its [2][max_iter] rows at a max_iter below the one it was
    allocated for): each loop equals, bit for bit, a fresh solver's from the same prices."""
    quiet(monkeypatch)
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    calls = cap_calls(cfg)
    one = solver(N, lc, pt, cells)
    for K, (y0, w_ref, lr) in ((3, calls[0]), (DEFAULT_CAP, calls[1]), (3, calls[0])):
        fresh = solver(N, lc, pt, cells)
        fresh.prev_prices = one.prev_prices.copy()
        with cap(K):
            ro, rf = run_loop(one, y0, w_ref, lr), run_loop(fresh, y0, w_ref, lr)
        steps = ro[2] - 1
        assert_form(one, ro[1], ro[3], cells)
        assert_launches(ro[3], cells, ro[2], K)
        assert ro[1]["iter"] == min(steps, K - 1) and ro[1]["dual_cost_decrease_actual"].shape == (steps,)
        assert steps == 3 if K == 3 else steps < K, (steps, K)
        same_bits(ro, rf)


def test_cap_on_the_sharded_form(nccl1, monkeypatch):  # noqa: F811
    """K = 3 on a world-1 RCCL group: the unfused form with the collective inside every engine call, so
    the calls enqueued must depend on the finishing call alone (every rank issues the same collectives):
    exactly K + 1 launch pairs, and bit for bit the plain solver's result."""
    quiet(monkeypatch)
    from lompc_amd.price_solver import PriceSolver

    cfg, K = "large-linear-convex-N24", 3
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    y0, w_ref, lr = cap_calls(cfg)[0]
    plain = solver(N, lc, pt, 6)
    shard = PriceSolver(N, lc, pt, device=0, group=nccl1)
    with cap(K):
        rp = run_loop(plain, y0, w_ref, lr)
        rs = run_loop(shard, y0, w_ref, lr)
    assert shard._plan.comm is not None and shard._native_ok() and shard.device_loop
    assert_launches(rp[3], 6, K + 1, K)
    assert_launches(rs[3], 33, K + 1, K)  # (unfused whatever the cell count: a communicator is attached)
    assert rs[1]["iter"] == K - 1 and rs[2] == K + 1 and rs[1]["dual_cost_decrease_actual"].shape == (K,)
    same_bits(rs, rp)
    compare_oracle(shard, rs, oracle_capped(cfg, 0, K), lr, c)


# ------------------------------------------------------------------ 2. the "max" tolerance
@pytest.mark.parametrize("cfg", MAX_CONFIGS)
def test_max_tolerance(gpu, monkeypatch, cfg):
    """PRICE_SOLVER_TOL_TYPE = "max" (tol_avg = 0): three consecutive calls in the three device forms
    against the host loop and the oracle; the Python loop against the oracle at one configuration.  The
    first call's count differs from its count under "avg" (from the same zero prices), in the oracle and
    on the device, so the case shows which test ran."""
    quiet(monkeypatch)
    monkeypatch.setattr(settings, "PRICE_SOLVER_TOL_TYPE", "max")
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    calls = max_calls(cfg)
    (orc, exit_errs), (avg, _) = (list(zip(*oracle_max(cfg, tt))) for tt in ("max", "avg"))
    assert orc[0][1]["iter"] != avg[0][1]["iter"]
    with_python = cfg == MAX_CONFIGS[-1]
    for cells in FORMS:
        dev, host = solver(N, lc, pt, cells), solver(N, lc, pt, cells, device_loop=False)
        for call, (y0, w_ref, lr) in enumerate(calls):
            start = dev.prev_prices.copy()
            rd = run_loop(dev, y0, w_ref, lr)
            assert_form(dev, rd[1], rd[3], cells)
            assert_launches(rd[3], cells, rd[2], DEFAULT_CAP)
            compare_host(rd, run_loop(host, y0, w_ref, lr), c.theta)
            compare_oracle(dev, rd, orc[call], lr, c)
            # the errors of the exit's test, LOMPC_STAT_MAX_ERR first, against the oracle's (the stats' bar)
            rc, steps, _, _, errs = raw_loop(dev, start, w_ref, lr, DEFAULT_CAP, tol_type="max")
            assert (rc, steps) == (_lib.LOMPC_OK, rd[1]["iter"])
            assert np.all(np.abs(errs - exit_errs[call]) <= 1e-6 * np.maximum(1.0, np.abs(exit_errs[call]))), \
                (errs, exit_errs[call])
        with pytest.MonkeyPatch.context() as mp:  # the same first call under "avg"
            mp.setattr(settings, "PRICE_SOLVER_TOL_TYPE", "avg")
            other = solver(N, lc, pt, cells)
            ra = run_loop(other, *calls[0])
            assert_form(other, ra[1], ra[3], cells)
            assert ra[1]["iter"] == avg[0][1]["iter"] != orc[0][1]["iter"]
    if with_python:
        py = solver(N, lc, pt, FORMS[0])
        py.native_loop = False
        for call, (y0, w_ref, lr) in enumerate(calls):
            rp = run_loop(py, y0, w_ref, lr)
            assert rp[3]["k_path"] == rp[3]["k_eval"] == rp[1]["iter"] + 1, rp[3]
            compare_oracle(py, rp, orc[call], lr, c)


# ------------------------------------------------------------------ 4. the error ends, 5. the loop after
ERROR_FORMS = [(6, True), (33, True), (6, False)]
ERROR_IDS = [FORM_IDS[6], FORM_IDS[33], "host-loop"]


def failing_loop(ps, cells, w_ref, lr, exc, match):
    """compute_optimal_prices must raise ``exc``; the launches of the form that ran are asserted (the
    error shows at the first engine call)."""
    res, n = counted(ps._plan, lambda: ps.compute_optimal_prices(w_ref, lr))
    assert isinstance(res, exc) and match in str(res), repr(res)
    assert ps._plan.info()["cells"] == cells
    if ps.device_loop:
        assert_launches(n, cells, 1, DEFAULT_CAP)
    else:
        assert n == {"k_path": 1, "k_eval": 1}, n


@pytest.mark.parametrize("cells,device_loop", ERROR_FORMS, ids=ERROR_IDS)
@pytest.mark.parametrize("cfg", TWO_CONFIGS)
def test_invalid_level(gpu, monkeypatch, cfg, cells, device_loop):
    """set_charge_levels_stats with statistics that pass the host check while the device levels hold one
    level at y_max + 1e-3 (gamma < 0) and one NaN: err = 1, LOMPC_ERR_INVALID_ARG, AssertionError naming
    gamma; lompc_plan_status reports the two; then section 5."""
    quiet(monkeypatch)
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    y0, w_ref, lr = cap_calls(cfg)[0]
    bad = y0.copy()
    bad[17], bad[311] = c.y_max + 1e-3, np.nan
    ps = solver(N, lc, pt, cells, device_loop=device_loop)
    ps.set_charge_levels_stats(torch.as_tensor(bad, device="cuda:0"), len(y0), float(y0.max()), float(y0.min()),
                               float(y0.sum()), descending=False)
    failing_loop(ps, cells, w_ref, lr, AssertionError, "gamma")
    assert plan_status(ps)[1:] == (0, 2)
    loop_after(ps, cfg, cells)


@pytest.mark.parametrize("cells,device_loop", ERROR_FORMS, ids=ERROR_IDS)
@pytest.mark.parametrize("cfg", TWO_CONFIGS)
def test_unsorted_set_handed_over_as_sorted(gpu, monkeypatch, cfg, cells, device_loop):
    """descending = True with two levels swapped: the sorted plan reports every EV of the set failed,
    err = 2, LOMPC_ERR_NOT_CONVERGED, SolverError, the plan's last error saying the set is unsorted;
    then section 5."""
    quiet(monkeypatch)
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    y0, w_ref, lr = cap_calls(cfg)[0]
    lv = np.sort(y0)[::-1].copy()
    lv[100], lv[400] = lv[400], lv[100]
    ps = solver(N, lc, pt, cells, device_loop=device_loop)
    ps.set_charge_levels_stats(torch.as_tensor(lv, device="cuda:0"), len(lv), float(lv.max()), float(lv.min()),
                               float(lv.sum()), descending=True)
    failing_loop(ps, cells, w_ref, lr, SolverError, "not ascending")
    assert "not ascending" in ps._lib.lompc_plan_last_error(ps._plan._plan).decode()
    assert plan_status(ps)[1:] == (len(lv), 0)
    loop_after(ps, cfg, cells)


@pytest.mark.parametrize("cells,device_loop", ERROR_FORMS, ids=ERROR_IDS)
def test_abi_refusals(gpu, monkeypatch, cells, device_loop):
    """lompc_price_loop refuses, with LOMPC_ERR_INVALID_ARG and nothing launched: max_iter = 0, r not in
    {2N, 3N}, n_evs = 0, and a plan whose S is not 2; then section 5 on the same plan."""
    quiet(monkeypatch)
    cfg = TWO_CONFIGS[0]
    ev, pt, N = CONFIGS[cfg]
    c, lc = consts(ev)
    y0, w_ref, lr = cap_calls(cfg)[0]
    ps = solver(N, lc, pt, cells, device_loop=device_loop)
    ps.set_charge_levels(y0)
    zero = np.zeros(ps.r)
    one_set = BatchPlan(ps.lompc, ps._gam_w0, np.array([0, len(y0)], dtype=np.int64), w_ref=ps._wr2[:1], want_w=False,
                        want_cost=False, want_set=True, validate=False, sorted_gamma=False)

    def refusals():
        return [raw_loop(ps, zero, w_ref, lr, 0)[0], raw_loop(ps, zero, w_ref, lr, 5, r=N)[0],
                raw_loop(ps, zero, w_ref, lr, 5, r=3 * N + 1)[0], raw_loop(ps, zero, w_ref, lr, 5, n_evs=0.0)[0]]

    rcs, n = counted(ps._plan, refusals)
    assert rcs == [_lib.LOMPC_ERR_INVALID_ARG] * 4, rcs
    assert n == {"k_path": 0, "k_eval": 0}, n
    rc, n = counted(one_set, lambda: raw_loop(ps, zero, w_ref, lr, 5, plan=one_set)[0])
    assert rc == _lib.LOMPC_ERR_INVALID_ARG and n == {"k_path": 0, "k_eval": 0}, (rc, n)
    assert plan_status(ps) == (0, 0, 0)
    loop_after(ps, cfg, cells)
