"""The device price loop away from the product's default shapes: more than 6 cells per set, horizons
outside the specialised {12, 16, 24, 48}, degenerate partitions, and reserved plans at 32 cells.

What runs (csrc/lompc_plan.hip, csrc/lompc_loop.hip):

* cells <= 32, one rank: the PERSISTENT form, the whole loop in one ``k_loop_run2`` launch (timed as
  k_path).  Its closing reads the cell records 16 at a time: one round for G <= 16, two for 17..32
  (the second padded with the zero record behind buffer 0), two record buffers by call parity.
* cells > 32: the UNFUSED form, per price iteration k_path + k_agg (timed as k_eval) + ``k_loop_step``.
* N in {12, 16, 24, 48}: ``k_loop_run2<N>``; every other horizon ``k_loop_run2<0>`` (the GENERIC form).

Every case asserts which form ran (``assert_form``), so no case can pass through the host loop that
``lompc_price_loop`` falls back to: persistent = exactly one k_path-timed launch per loop and no
k_eval-timed launch, the plan reporting the requested cell count; unfused = at least iter + 1
evaluation launches.

Checkers and bars (the suite's existing ones):

* the host C++ loop (``device_loop = False``), as test_gpu_price_solver.py's
  test_device_loop_matches_host_loop: equal iterations, engine calls = iter + 1, prices within
  1e-9 theta, decreases at rtol 1e-8 (atol 1e-8 of the largest), prices before / after
  regularisation within 1e-9 relative;
* the CPU oracle loop (oracle/price_oracle.py, ``warm = True``), as test_gpu_price_solver.py's
  compare(): equal iterations, prices within 1e-6 theta, the stats within 1e-6, get_w0_price0 within
  1e-6 w_max / 1e-6 relative.  Where the ORACLE's loop is longer than 100 iterations the prices are
  compared per component within 1e-6 max(theta, |lambda_i|) (test_gpu_price_loop_long.py documents
  why the absolute form cannot hold for long loops).

Seeds.  The iteration count must match the oracle's exactly, so every (case, call) here was checked on
the CPU (scripts/check_price_loop_seeds.py) not to sit on a knife-edge: with e_k the oracle's average
error before step k and tol its tolerance, e_k > tol (1 + 1e-6) for every k before the last and
e_last <= tol (1 - 1e-6) — which is exactly the statement that the oracle's count is unchanged when
its tolerance is scaled by 1 +- 1e-6 (the iterates before the exit do not depend on the tolerance).
The seeds are the ``SEED_*`` constants below.  The oracle's counts at these seeds (the script prints
them per call; the closest any error comes to its tolerance is 8e-4 relative): section 1 — 46, 14, 4
(small, linear, N 24) and 36, 3, 4 (large, linear-convex, N 48); section 2 — first calls 26..82, later
calls 0..24; section 3 — one EV 202 / 235 and one level 168 / 164 (small / large) at lmbd_r = 0, the
other shapes 25..35 and 5..21 at lmbd_r = 1.5 N delta, the full range 1..2 at either.

The oracle's results are computed once per input set and shared (``functools.lru_cache``) by the cell
counts that run the same inputs; nothing mutates them.
"""
import functools

import numpy as np
import pytest

import lompc_oracle as O
import price_oracle as PO
from lompc_amd import LoMPCConstants, settings
from lompc_amd.price_solver import PriceSolver

pytestmark = pytest.mark.gpu

SEED_CELLS = 1100
SEED_HORIZON = 1200
SEED_SHAPES = 1300
SEED_CHAIN = 1400
N_ORACLE = 600  # section 1: the oracle runs on the first 600 EVs

EVS = ("small", "large")
PTS = ("linear", "linear-convex")


def consts(ev):
    c = O.small_consts() if ev == "small" else O.large_consts()
    return c, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type)


# ------------------------------------------------------------------ inputs (pure functions of the case)
def spread_calls(seed, ev, N, nev, calls):
    """[(y0, w_ref, lmbd_r)] per call: test_device_loop_matches_host_loop's pattern, the last call
    with lmbd_r > 0."""
    c, _ = consts(ev)
    rng = np.random.default_rng(seed)
    out = []
    for call in range(calls):
        y0 = 0.3 + (0.02 + 0.02 * call) * c.y_max * rng.random(nev)
        w_ref = c.w_max * (0.2 + 0.6 * rng.random(N))
        lr = 0.0 if call < calls - 1 else 3.0 * N * c.delta * (0.25 + 0.5 * rng.random())
        out.append((y0, w_ref, lr))
    return out


CELL_CONFIGS = {"small-linear-N24": ("small", "linear", 24), "large-convex-N48": ("large", "linear-convex", 48)}


def cells_calls(cfg):
    ev, pt, N = CELL_CONFIGS[cfg]
    return spread_calls(SEED_CELLS + N + (ev == "large"), ev, N, 3000, 3)


def horizon_calls(N, ev, pt):
    seed = SEED_HORIZON + 4 * N + 2 * (ev == "large") + (pt == "linear-convex")
    return spread_calls(seed, ev, N, 600, 3 if N <= 32 else 2)


SHAPES = ("one", "same500", "clusters", "at-empty", "at-full", "full-range")


def shape_calls(shape, ev, robust):
    c, _ = consts(ev)
    N = 24
    rng = np.random.default_rng(SEED_SHAPES + 10 * SHAPES.index(shape) + 2 * (ev == "large") + int(robust))
    ym = c.y_max
    if shape == "one":
        y0 = np.array([0.4 * ym])
    elif shape == "same500":
        y0 = np.full(500, 0.37 * ym)
    elif shape == "clusters":
        y0 = np.concatenate([np.full(300, 0.35 * ym), np.full(300, 0.35 * ym + 0.03 * ym)])
    elif shape == "at-empty":
        y0 = np.concatenate([np.zeros(50), 0.03 * ym * rng.random(400)])
    elif shape == "at-full":
        y0 = np.concatenate([np.full(50, ym), ym - 0.03 * ym * rng.random(400)])
    else:
        y0 = ym * rng.random(800)
    y0 = rng.permutation(y0)
    w_ref = c.w_max * (0.2 + 0.6 * rng.random(N))
    return [(y0, w_ref, 1.5 * N * c.delta if robust else 0.0)]


# ------------------------------------------------------------------ the oracle, once per input set
def oracle_loops(N, ev, pt, calls):
    c, _ = consts(ev)
    po = PO.OraclePriceSolver(N, c, pt)
    po.warm = True
    out = []
    for y0, w_ref, lr in calls:
        po.set_charge_levels(y0)
        lmo, sto = po.compute_optimal_prices(w_ref, lr)
        lmo = lmo.copy()
        w0o, p0o = po.get_w0_price0_batch(lmo[: po.r], lr)
        out.append((lmo, sto, w0o, p0o))
    return out


@functools.lru_cache(maxsize=None)
def oracle_cells(cfg):
    ev, pt, N = CELL_CONFIGS[cfg]
    return oracle_loops(N, ev, pt, [(y0[:N_ORACLE], w, lr) for y0, w, lr in cells_calls(cfg)])


@functools.lru_cache(maxsize=None)
def oracle_horizon(N, ev, pt):
    return oracle_loops(N, ev, pt, horizon_calls(N, ev, pt))


@functools.lru_cache(maxsize=None)
def oracle_shape(shape, ev, robust):
    return oracle_loops(24, ev, "linear-convex", shape_calls(shape, ev, robust))


# ------------------------------------------------------------------ running and comparing
def solver(N, lc, pt, cells, device_loop=True):
    ps = PriceSolver(N, lc, pt, device=0)
    ps.loop_cells = cells
    ps.device_loop = device_loop
    assert ps.native_loop
    return ps


def run_loop(ps, y0, w_ref, lr):
    """set_charge_levels + compute_optimal_prices with the loop's launches counted:
    (prices, stats, engine calls, {k_path, k_eval: launches})."""
    ps.set_charge_levels(y0)
    plan = ps._plan
    kern = ("k_path", "k_eval")
    plan.profile(enable=kern)
    for k in kern:
        plan.profile(read=True, reset=True, kernel=k)
    n0 = ps.n_batched_calls
    lm, st = ps.compute_optimal_prices(w_ref, lr)
    n = {k: plan.profile(read=True, kernel=k)[1] for k in kern}
    plan.profile(enable=False)
    return lm.copy(), st, ps.n_batched_calls - n0, n


def assert_form(ps, st, n, cells):
    """Which device loop ran: persistent (k_loop_run2, one launch) up to 32 cells, unfused beyond."""
    assert ps.device_loop and ps._plan.info()["cells"] == cells
    if cells <= 32:
        assert n["k_path"] == 1 and n["k_eval"] == 0, n
    else:
        assert n["k_eval"] >= st["iter"] + 1 and n["k_path"] >= st["iter"] + 1, (n, st["iter"])


def compare_host(dev, host, theta):
    (ld, sd, nd, _), (lh, sh, nh, kh) = dev, host
    assert sd["iter"] == sh["iter"] and nd == nh == sd["iter"] + 1, (sd["iter"], sh["iter"], nd, nh)
    assert kh["k_eval"] == kh["k_path"] == sh["iter"] + 1, kh  # (the host loop: one engine call per launch pair)
    np.testing.assert_allclose(ld, lh, rtol=0, atol=1e-9 * theta)
    for k in ("dual_cost_decrease_actual", "dual_cost_decrease_predicted"):
        np.testing.assert_allclose(sd[k], sh[k], rtol=1e-8, atol=1e-8 * np.max(np.abs(sh[k]), initial=1.0), err_msg=k)
    for k in ("price_before_reg", "price_after_reg"):
        assert abs(sd[k] - sh[k]) <= 1e-9 * max(1.0, abs(sh[k])), (k, sd[k], sh[k])


def compare_oracle(ps, dev, orc, lr, c):
    lm, st = dev[0], dev[1]
    lmo, sto, w0o, p0o = orc
    assert st["iter"] == sto["iter"], (st["iter"], sto["iter"])
    if sto["iter"] > 100:  # (the long-loop price form, test_gpu_price_loop_long.py)
        err = np.abs(lm - lmo) / np.maximum(c.theta, np.abs(lmo))
        assert err.max() <= 1e-6, (float(err.max()), int(np.argmax(err)))
    else:
        np.testing.assert_allclose(lm, lmo, rtol=0, atol=1e-6 * c.theta)
    for k in ("price_before_reg", "price_after_reg"):
        assert abs(st[k] - sto[k]) <= 1e-6 * max(1.0, abs(sto[k])), (k, st[k], sto[k])
    for k in ("dual_cost_decrease_actual", "dual_cost_decrease_predicted"):
        assert st[k].shape == sto[k].shape, k
        np.testing.assert_allclose(st[k], sto[k], rtol=1e-6, atol=1e-6 * np.max(np.abs(sto[k]), initial=1.0), err_msg=k)
    w0, p0 = ps.get_w0_price0(lm[: ps.r], lr)
    np.testing.assert_allclose(w0, w0o, rtol=0, atol=1e-6 * c.w_max)
    assert abs(p0 - p0o) <= 1e-6 * max(1.0, abs(p0o)), (p0, p0o)


# ------------------------------------------------------------------ 1. cell counts
@pytest.mark.parametrize("cfg", list(CELL_CONFIGS))
@pytest.mark.parametrize("cells", [1, 16, 17, 20, 31, 32, 33],
                         ids=lambda g: f"G{g}-" + ("persistent-1round" if g <= 16 else
                                                   "persistent-2rounds" if g <= 32 else "unfused"))
def test_cell_counts(gpu, monkeypatch, cfg, cells):
    """k_loop_run2's chunked closing on both sides of its one-round / two-round boundary (16 | 17),
    up to its limit (32), and the unfused form past it (33): three consecutive calls on one solver
    (warm prices, both record buffers' parities, the last with lmbd_r > 0) against the host loop on
    3 000 EVs; at 20 and 32 cells also against the oracle on the first 600 EVs."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    ev, pt, N = CELL_CONFIGS[cfg]
    c, lc = consts(ev)
    dev, host = solver(N, lc, pt, cells), solver(N, lc, pt, cells, device_loop=False)
    with_oracle = cells in (20, 32)
    small = solver(N, lc, pt, cells) if with_oracle else None
    for call, (y0, w_ref, lr) in enumerate(cells_calls(cfg)):
        rd = run_loop(dev, y0, w_ref, lr)
        assert_form(dev, rd[1], rd[3], cells)
        compare_host(rd, run_loop(host, y0, w_ref, lr), c.theta)
        if with_oracle:
            rs = run_loop(small, y0[:N_ORACLE], w_ref, lr)
            assert_form(small, rs[1], rs[3], cells)
            compare_oracle(small, rs, oracle_cells(cfg)[call], lr, c)
            if call == 0:
                assert rs[1]["iter"] >= 3


# ------------------------------------------------------------------ 2. horizons outside {12, 16, 24, 48}
HORIZON_CASES = [(N, 6) for N in (1, 2, 13, 20, 32, 64)] + [(13, 32), (64, 32)]


@pytest.mark.parametrize("pt", PTS)
@pytest.mark.parametrize("ev", EVS)
@pytest.mark.parametrize("N,cells", HORIZON_CASES, ids=[f"N{n}-G{g}-persistent-generic" for n, g in HORIZON_CASES])
def test_generic_horizons(gpu, monkeypatch, N, cells, ev, pt):
    """k_loop_run2<0>, the generic-N instantiation of the persistent kernel, as a LOOP (N = 64: every
    lane of the wave holds a stage; N = 1, 2: the shortest horizons; 13, 20, 32: between the
    specialised ones), at the default 6 cells and, for 13 and 64, at 32 (two closing rounds): against
    the oracle and the host loop over consecutive calls."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c, lc = consts(ev)
    dev, host = solver(N, lc, pt, cells), solver(N, lc, pt, cells, device_loop=False)
    orc = oracle_horizon(N, ev, pt)
    for call, (y0, w_ref, lr) in enumerate(horizon_calls(N, ev, pt)):
        rd = run_loop(dev, y0, w_ref, lr)
        assert_form(dev, rd[1], rd[3], cells)
        if call == 0:
            assert rd[1]["iter"] >= 3  # (a loop of several calls in the one launch)
        compare_host(rd, run_loop(host, y0, w_ref, lr), c.theta)
        compare_oracle(dev, rd, orc[call], lr, c)


# ------------------------------------------------------------------ 3. degenerate partitions
@pytest.mark.parametrize("cells", [6, 32], ids=["G6-persistent-1round", "G32-persistent-2rounds"])
@pytest.mark.parametrize("robust", [False, True], ids=["lr0", "lr1.5Ndelta"])
@pytest.mark.parametrize("ev", EVS)
@pytest.mark.parametrize("shape", SHAPES)
def test_degenerate_partitions(gpu, monkeypatch, shape, ev, robust, cells):
    """k_loop_run2<24> on the partitions the station produces but no loop test draws: one EV (every
    cell but one empty; prewarm_partitions' placeholder), 500 EVs on one charge level (the gamma
    window collapses), two clusters of identical levels, EVs exactly at y0 = 0 and at y0 = y_max, and
    levels over the whole [0, y_max] (a 1-2 iteration loop: the closing and w0)."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    N, pt = 24, "linear-convex"
    c, lc = consts(ev)
    dev, host = solver(N, lc, pt, cells), solver(N, lc, pt, cells, device_loop=False)
    (y0, w_ref, lr), = shape_calls(shape, ev, robust)
    rd = run_loop(dev, y0, w_ref, lr)
    assert_form(dev, rd[1], rd[3], cells)
    compare_host(rd, run_loop(host, y0, w_ref, lr), c.theta)
    compare_oracle(dev, rd, oracle_shape(shape, ev, robust)[0], lr, c)


# ------------------------------------------------------------------ 4. reserved plans and the chain at 32 cells
@pytest.mark.parametrize("ev,pt,N", [("large", "linear-convex", 24), ("small", "linear", 20)],
                         ids=["large-convex-N24-k_loop_run2<24>", "small-linear-N20-k_loop_run2<0>"])
@pytest.mark.parametrize("reserve", [0, 8192], ids=["grown", "reserved"])
def test_zero_record_follows_the_cell_count(gpu, monkeypatch, ev, pt, N, reserve):
    """A plan created with an explicit cell count keeps it for life, so the record layout of one plan
    (2 S G + 1 records, the zero record at S G) moves only where the ENGINE picks the count from the
    set size (``loop_cells = None``: 16 cells above 1 024 EVs, 8 above 64, else 1).  One solver
    re-targeted 40 -> 500 -> 5 000 -> 500 -> 40 -> 5 000 EVs: the record buffer grows twice on the way
    up ("grown") or is sized once for 16 cells ("reserved": ``reserve_evs``), and after each move the
    closing's padding must read the zero record of the new layout, not a stale cell record of the old
    one — persistent form every time, equal to the host loop (which reads no records)."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c, lc = consts(ev)
    rng = np.random.default_rng(SEED_CHAIN + 50 + N)
    dev, host = solver(N, lc, pt, None), solver(N, lc, pt, None, device_loop=False)
    dev.reserve_evs = host.reserve_evs = reserve
    for nev, cells in ((40, 1), (500, 8), (5000, 16), (500, 8), (40, 1), (5000, 16)):
        y0 = 0.3 + 0.04 * c.y_max * rng.random(nev)
        w_ref = c.w_max * (0.2 + 0.6 * rng.random(N))
        rd = run_loop(dev, y0, w_ref, 0.0)
        assert_form(dev, rd[1], rd[3], cells)
        compare_host(rd, run_loop(host, y0, w_ref, 0.0), c.theta)


def stage(ps, p, y0):
    import torch

    yd = torch.as_tensor(y0, device="cuda:0")
    ps.stage_partition(p, yd, len(y0), float(y0.max()), float(y0.min()), float(y0.sum()), descending=True)


def assert_same_results(a, b):
    for (la, sa), (lb, sb) in zip(a, b):
        assert sa["iter"] == sb["iter"]
        np.testing.assert_array_equal(lb, la)
        for k in ("price_before_reg", "price_after_reg"):
            assert sa[k] == sb[k], k
        for k in ("dual_cost_decrease_actual", "dual_cost_decrease_predicted"):
            np.testing.assert_array_equal(sb[k], sa[k])


@pytest.mark.parametrize("N", [48, 20], ids=["N48-k_loop_run2<48>", "N20-k_loop_run2<0>"])
@pytest.mark.parametrize("ev", EVS)
def test_reserved_chain_at_32_cells(gpu, monkeypatch, ev, N):
    """test_price_chain_equals_partition_loops at 32 cells on RESERVED plans created by
    prewarm_partitions (one-EV placeholder batches; the reserve sizes every cell-indexed buffer and
    the record buffer for 16 cells per set, which 32 exceeds: they must take the plan's own count,
    the record buffer at its first loop): lompc_price_chain equals the
    per-partition loops bit for bit, a one-EV partition between two of 6 000 and an empty partition
    skipped.  Then the same plans are re-targeted at batches of other sizes (the one-EV and 6 000-EV
    partitions swapped, the third cut to 777 EVs), run, and re-targeted back: the second run of the
    first batches equals the first bit for bit.  (A plan's explicit cell count cannot change, so the
    move of the zero record between layouts is test_zero_record_follows_the_cell_count's.)"""
    from lompc_amd.settings import MIN_INITIAL_SOC

    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c, lc = consts(ev)
    rng = np.random.default_rng(SEED_CHAIN + N + (ev == "large"))
    edges = np.linspace(MIN_INITIAL_SOC, c.y_max, 13)
    parts = [0, 1, 3]  # (partition 2 has no EVs)
    sizes = {0: 6000, 1: 1, 3: 6000}
    w_refs = 0.8 * c.w_max * rng.random((4, N))
    levels = {p: np.sort(edges[p] + (edges[p + 1] - edges[p]) * rng.random(sizes[p]))[::-1].copy() for p in parts}
    other = {0: levels[1], 1: levels[0], 3: levels[3][:777].copy()}
    sol = {}
    for mode in ("loops", "chain"):
        ps = solver(N, lc, "linear-convex", 32)
        ps.reserve_evs = 8192
        ps.prewarm_partitions(parts)
        for p in parts:
            assert ps._staged[p]["_plan"].info()["cells"] == 32
        sol[mode] = ps

    def run_loops(ps, lv):
        for p in parts:
            stage(ps, p, lv[p])
        ps.prev_prices = np.zeros(ps.r)
        res, n0 = [], ps.n_batched_calls
        for p in parts:
            ps.use_partition(p)
            plan = ps._plan
            plan.profile(enable=("k_path", "k_eval"))
            for k in ("k_path", "k_eval"):
                plan.profile(read=True, reset=True, kernel=k)
            lm, st = ps.compute_optimal_prices(w_refs[p], 0.0)
            n = {k: plan.profile(read=True, kernel=k)[1] for k in ("k_path", "k_eval")}
            plan.profile(enable=False)
            assert_form(ps, st, n, 32)
            res.append((lm.copy(), st))
        return res, ps.n_batched_calls - n0

    def run_chain(ps, lv):
        for p in parts:
            stage(ps, p, lv[p])
        ps.prev_prices = np.zeros(ps.r)
        assert ps.chain_ok(parts)
        n0 = ps.n_batched_calls
        res = ps.compute_optimal_prices_chain(parts, w_refs[parts], 0.0)
        return [(lm.copy(), st) for lm, st in res], ps.n_batched_calls - n0

    first_loops, nl = run_loops(sol["loops"], levels)
    first_chain, nc = run_chain(sol["chain"], levels)
    assert nl == nc
    assert_same_results(first_loops, first_chain)
    np.testing.assert_array_equal(sol["chain"].prev_prices, sol["loops"].prev_prices)
    assert sum(st["iter"] for _, st in first_loops) >= 3
    # other batches through the same plans, then back
    mid_loops, _ = run_loops(sol["loops"], other)
    mid_chain, _ = run_chain(sol["chain"], other)
    assert_same_results(mid_loops, mid_chain)
    again_loops, _ = run_loops(sol["loops"], levels)
    again_chain, _ = run_chain(sol["chain"], levels)
    assert_same_results(first_loops, again_loops)
    assert_same_results(first_chain, again_chain)
