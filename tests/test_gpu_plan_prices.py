"""Every plan form of the PATH engine, and DIRECT mode, on structured and extreme price vectors.

The other GPU tests that drive a plan draw their prices as theta * rand (dense, tie-free, of magnitude
theta).  The product's own prices are max(0, ...) steps: exact zeros, ties, flat stretches, and in the
capped loop of tests/golden/price_loop_long.npz one convex-price component at 3.9e5 theta.  Here the
families of tests/price_families.py (flat / tied / zero / two-level / ramped / spiked / square-wave
prices, one component at the fixture's largest price in each block, lambda_3 * 1e6, everything * 1e-12,
per-entry scales 1e-8 .. 1e3, dense theta * rand times 1, 1e3, the fixture's largest price, 1e7, 1e9) are
the parameter sets of one plan per horizon: both EV types in one plan, every family at lmbd_r = 0 and
1.5 N delta, about 130 EVs per set (gamma = 0 and y_max exactly, 13 values five times, the rest
uniform), and 1100-EV sets (more than one evaluation block) of all_1e-12, ramp_l1_down and, from N = 24,
the dense fixture-max rung.  N in {2, 13, 64} takes the generic <0> kernels, N in {12, 16, 24, 48} the
compiled ones.

The dense rung at the fixture's largest price is a set of the per-horizon plan, through every form, at the
horizons where the engine certifies it (N >= 24).  Below (RUNG_DEFECT) it has a plan of its own, which goes
through every form too, under the contract of the range beyond the product's — never silently wrong: every
OK or REPAIRED EV at the bars, every other EV FAILED and counted, and the FAILED EVs' w at the 1e-9 bar as
well, since the defect is a certificate that refuses right answers — and only the assertion that nothing
FAILED is a strict xfail (test_fixture_max_rung_nothing_failed_*).

Reference: the C oracle (oracle/lompc_oracle.c, certified on these families by tests/test_oracle.py)
over EVERY EV of every set.  Bars: test_gpu_plan_horizons.py's, through its helpers — per-EV |dw| <=
1e-9; cost, SUM_PRICE0, SUM_COST 1e-9 relative; set sums rtol 1e-10, atol 1e-9; a rows form against its
own sums 1e-11; COUNT exact.  Every case prints its largest deviation as a share of the bar first.

Status contract.  Product range (every family but dense 1e7 and 1e9): N_FAILED = N_INVALID = 0 and
every status OK or REPAIRED.  Beyond it the engine may fail but not be silently wrong: every EV whose
status is OK or REPAIRED meets the bars, every other EV is counted in N_FAILED
(test_beyond_product_range_is_never_silently_wrong prints which of the two happened).

Forms and what identifies them (launch counts of k_path, k_eval, k_finalize; see the table in
test_gpu_plan_horizons.py): single run with rows (1, 1, 1); wide run_steps with rows (1, K, K); the same
without w, piece sums (1, K, K); sort_sets plans, k_agg (1, 1, 0) and k_aggs wide (1, K, 0); the
station's w0 pass after plan.update (1, 1, 0); solve_batch in mode "direct" (k_direct, one launch, after
k_central from gamma_ref).
"""
import functools

import numpy as np
import pytest
import torch

import oracle_c
import price_families as PF
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, SolverError
from test_gpu_plan_horizons import (ST, Batch, Dev, clone, contexts, counted, groups, np_, rows_vs_oracle,
                                    sets_vs_oracle, sets_vs_own_rows)

pytestmark = pytest.mark.gpu

NS = [2, 12, 13, 16, 24, 48, 64]
NS_DIRECT = [5, 13, 24, 64]
K = 3
BIG = 1100                      # EVs of a set that spans more than one evaluation block
RUNG = "dense_fixture_max"     # the dense rung at the fixture's largest price
BIG_PRODUCT = (("all_1e-12", 1), ("ramp_l1_down", 1))  # (the host path engine re-solves most there)
RUNG_FROM = 24                 # the rung is a set of the per-horizon plan from this horizon, below: rung_batch
BIG_BEYOND = ("dense_1e7", 0)
# The engine's certificate tolerance is 1e-11 (1 + c N^2 w_max + slope + theta^2): it ignores the prices'
# magnitude.  With EVERY price at 3.9e5 theta the rounding of the gradient itself exceeds it at short
# horizons (N^2 small), and correct optima (the FAILED EVs' w is asserted at the 1e-9 bar) are reported FAILED.
RUNG_FAILS_PATH = (2, 12, 13, 16)
RUNG_FAILS_DIRECT = (5, 13)
RUNG_DEFECT = ("certificate tolerance ignores price magnitude: dense prices at the fixture's largest price "
               "(3.9e5 theta) are reported FAILED at N <= 16 although w is right (q.scale, lompc_kernels.hip)")
EVAL_BLOCK = 1024               # k_eval: EVs per workgroup at most (EVAL_MAXB, lompc_plan.hip)
TYPES = ("small", "large")


class FamilyBatch(Batch):
    """test_gpu_plan_horizons.Batch with the price families as its sets: per type, every family at both
    lmbd_r (N_GAMMA EVs each), then the ``big`` (family, lmbd_r index) sets with BIG EVs.  Run k's prices
    are the families at seed k."""

    def __init__(self, N, families, big=(), runs=K):
        self.N, self.K = N, runs
        self.cs, lompcs = contexts(N)
        self.lompcs = list(lompcs)
        self.names = [(f, i) for f in families for i in (0, 1)] + list(big)
        self.n_own = 2 * len(families)
        self.P = P = len(self.names)
        sizes = [PF.N_GAMMA] * (2 * len(families)) + [BIG] * len(big)
        self.rng = np.random.default_rng(7000 + N)
        parts, lm, lr = [], np.zeros((runs, 2 * P, 3 * N)), np.zeros((runs, 2 * P))
        for t, ev in enumerate(TYPES):
            for p, ((f, i), m) in enumerate(zip(self.names, sizes)):
                parts.append(PF.gammas(N, ev, seed=p, n=m))
                for k in range(runs):
                    lm[k, t * P + p] = PF.prices(f, N, ev, seed=k)
                lr[:, t * P + p] = PF.lmbd_rs(N, ev)[i]
        self.take(parts, lm, lr)
        self._host = None

    def label(self, s):
        f, i = self.names[s % self.P]
        return f"{TYPES[s // self.P]}/{f}/lr{i}" + ("/big" if s % self.P >= self.n_own else "")


@functools.lru_cache(maxsize=None)
def product_batch(N):
    if N >= RUNG_FROM:
        return FamilyBatch(N, PF.PRODUCT, big=BIG_PRODUCT + ((RUNG, 0),))
    return FamilyBatch(N, [f for f in PF.PRODUCT if f != RUNG], big=BIG_PRODUCT)


@functools.lru_cache(maxsize=None)
def rung_batch(N):
    return FamilyBatch(N, (RUNG,), big=((RUNG, 0),))


@functools.lru_cache(maxsize=None)
def beyond_batch(N):
    return FamilyBatch(N, PF.BEYOND, big=(BIG_BEYOND,), runs=1)


def ok_or_repaired(status):
    return (status == ST.LOMPC_QP_OK) | (status == ST.LOMPC_QP_REPAIRED)


def repaired_by_set(bt, status):
    return {bt.label(s): int(np.sum(status[bt.off[s]:bt.off[s + 1]] == ST.LOMPC_QP_REPAIRED)) for s in range(bt.S)}


def repaired_span(bt, status, big):
    """Largest distance between two REPAIRED EVs of the BIG set ``big`` = (family, lmbd_r index), per
    type: two EVs at least EVAL_BLOCK apart lie in different evaluation blocks (a block holds at most
    EVAL_BLOCK EVs)."""
    p = bt.n_own + bt.names[bt.n_own:].index(big)
    spans = []
    for t in range(2):
        a, b = bt.off[t * bt.P + p], bt.off[t * bt.P + p + 1]
        assert b - a == BIG
        r = np.flatnonzero(status[a:b] == ST.LOMPC_QP_REPAIRED)
        spans.append(int(r[-1] - r[0]) if r.size else -1)
    return spans


def host_individual(bt, cells=0):
    """EVs the host path engine (oracle/path_cpu.cpp) solves individually at run 0's prices, per set label.
    cells: gamma cells per set (0: the host engine's choice from each set's own size)."""
    if bt._host is None:
        bt._host = {}
    if cells in bt._host:
        return bt._host[cells]
    out = bt._host[cells] = {}
    for s in range(bt.S):
        a, b = bt.off[s], bt.off[s + 1]
        o = oracle_c.path_run(bt.N, [bt.consts_of(s)], [1], bt.lm[0, s][None, :], bt.lr[0, s:s + 1], bt.gn[a:b],
                              np.array([0, b - a], dtype=np.int64), cells=cells, want_cost=False)
        out[bt.label(s)] = int(o["info"][2])
    return out


def print_repaired(name, bt, nrep, cells=0):
    """Run 0's REPAIRED count per set (nrep: (S,)) beside the host path engine's individually solved EVs."""
    host = host_individual(bt, cells)
    print(f"{name}: REPAIRED (device) / solved individually (host) per set: "
          + ", ".join(f"{bt.label(s)} {int(nrep[s])}/{host[bt.label(s)]}" for s in range(bt.S)
                      if nrep[s] or host[bt.label(s)]))


def counted_loud(plan, call):
    """counted() for a plan that may report FAILED EVs: the tallies' SolverError is not an error here."""
    try:
        return counted(plan, call)
    except SolverError:
        n = tuple(plan.profile(read=True, reset=True, kernel=k)[1] for k in BatchPlan.KERNELS)
        plan.profile(enable=False)
        return None, n


def loud_sets(dev, bt, k, sw, st, name, cost=True):
    """Set reductions of a plan that may fail loudly: COUNT exact, nothing INVALID, and every set without
    a FAILED EV at the set bars of sets_vs_oracle.  Returns N_FAILED per set."""
    osw, ow0, op0, oc = bt.oracle_sets(k)
    np.testing.assert_array_equal(st[:, ST.LOMPC_STAT_COUNT], np.diff(bt.off))
    assert np.all(st[:, ST.LOMPC_STAT_N_INVALID] == 0)
    nf = st[:, ST.LOMPC_STAT_N_FAILED].astype(np.int64)
    assert np.all(nf >= 0) and np.all(nf + st[:, ST.LOMPC_STAT_N_REPAIRED] <= np.diff(bt.off))
    z = nf == 0
    dev.add(f"set sums ({name})", np.abs(sw - osw)[z], (1e-9 + 1e-10 * np.abs(osw))[z])
    dev.add(f"sum w0 ({name})", np.abs(st[:, ST.LOMPC_STAT_SUM_W0] - ow0)[z], (1e-9 + 1e-10 * np.abs(ow0))[z])
    dev.add(f"sum price0 ({name})", np.abs(st[:, ST.LOMPC_STAT_SUM_PRICE0] - op0)[z], (1e-9 * np.maximum(1.0, np.abs(op0)))[z])
    if cost:
        dev.add(f"sum cost ({name})", np.abs(st[:, ST.LOMPC_STAT_SUM_COST] - oc)[z], (1e-9 * np.maximum(1.0, np.abs(oc)))[z])
    return nf


def loud_rows(dev, bt, k, w, cost, status, sw, st, name, failed_w=False):
    """Per-EV rows of a plan that may fail loudly: every status OK, REPAIRED or FAILED; every OK or REPAIRED
    EV at the bars; every other EV counted in its set's N_FAILED; failed_w: the FAILED EVs' w at the 1e-9
    bar too.  Returns N_FAILED per set."""
    good = ok_or_repaired(status)
    assert np.all(good | (status == ST.LOMPC_QP_FAILED))
    W, C = bt.oracle(k)
    dev.add(f"|dw| of OK / REPAIRED ({name})", np.abs(w - W)[good], 1e-9)
    dev.add(f"cost of OK / REPAIRED ({name})", np.abs(cost - C)[good], (1e-9 + 1e-9 * np.abs(C))[good])
    if failed_w:
        dev.add(f"|dw| of FAILED ({name})", np.abs(w - W)[~good], 1e-9)
    nf = loud_sets(dev, bt, k, sw, st, name)
    np.testing.assert_array_equal(nf, [int(np.sum(~good[bt.off[s]:bt.off[s + 1]])) for s in range(2 * bt.P)])
    np.testing.assert_array_equal(st[:, ST.LOMPC_STAT_N_REPAIRED],
                                  [int(np.sum(status[bt.off[s]:bt.off[s + 1]] == ST.LOMPC_QP_REPAIRED)) for s in range(2 * bt.P)])
    return nf


@functools.lru_cache(maxsize=None)
def single_run(N):
    """One run with rows of the product-range plan at run 0's prices: numpy outputs and launch counts."""
    bt = product_batch(N)
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_w=True, want_cost=True,
                     want_status=True)
    assert plan.launches_per_run() == 3
    o, n = counted(plan, lambda: clone(plan.run(bt.lm_d[0], bt.lr_d[0])))
    return {k: np_(v) for k, v in o.items()}, n, plan.last_check


@pytest.mark.parametrize("N", NS)
def test_single_run_rows_vs_oracle(gpu, N):
    """k_path, k_eval, k_finalize, one launch each, with rows: every EV against the oracle; REPAIRED
    counts per family beside the host path engine's individually solved EVs."""
    bt = product_batch(N)
    o, n, chk = single_run(N)
    assert n == (1, 1, 1), n
    dev = Dev(f"prices single N={N}")
    rep = repaired_by_set(bt, o["status"])
    print_repaired(f"prices single N={N}", bt, o["set_stats"][:, ST.LOMPC_STAT_N_REPAIRED])
    print(f"prices single N={N}: REPAIRED span of the {BIG}-EV sets: "
          f"{[repaired_span(bt, o['status'], b) for b in BIG_PRODUCT]}")
    assert np.all(ok_or_repaired(o["status"])) and chk[1:] == (0, 0)
    assert chk[0] == sum(rep.values())
    rows_vs_oracle(dev, bt, 0, o["w"], o["cost"])
    sets_vs_oracle(dev, bt, 0, o["set_sum_w"], o["set_stats"])
    sets_vs_own_rows(dev, bt, o["w"], o["cost"], o["set_sum_w"], o["set_stats"])
    np.testing.assert_array_equal(o["set_stats"][:, ST.LOMPC_STAT_N_REPAIRED], [rep[bt.label(s)] for s in range(2 * bt.P)])
    dev.check()


@pytest.mark.parametrize("N", NS)
def test_wide_run_steps_rows_vs_oracle(gpu, N):
    """Wide run_steps (k_paths, k_evals, k_closes), K = 3 runs with rows kept per run: every run's w,
    cost, status and set reductions against the oracle, run 0 bitwise equal to the single run."""
    bt = product_batch(N)
    dev = Dev(f"prices wide rows N={N}")
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_w=True, want_cost=True,
                     want_status=True)
    o, n = counted(plan, lambda: plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True))
    info = plan.info()
    assert plan.cells % 4 == 0 and info["steps_group"] == 1 and n == (groups(K), K, K), n
    assert plan.last_check[1:] == (0, 0)
    w, cost, status = np_(o["w"]), np_(o["cost"]), np_(o["status"])
    sw, st = np_(o["set_sum_w"]), np_(o["set_stats"])
    assert np.all(ok_or_repaired(status))
    one, _, _ = single_run(N)
    print_repaired(f"prices wide rows N={N}", bt, st[0, :, ST.LOMPC_STAT_N_REPAIRED])
    for key, got in (("w", w), ("cost", cost), ("status", status)):
        np.testing.assert_array_equal(got[0], one[key], err_msg=key)
    if not info["evals_staged"]:
        np.testing.assert_array_equal(sw[0], one["set_sum_w"])
        np.testing.assert_array_equal(st[0], one["set_stats"])
    for k in range(K):
        rows_vs_oracle(dev, bt, k, w[k], cost[k])
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
        sets_vs_own_rows(dev, bt, w[k], cost[k], sw[k], st[k])
    dev.check()


@pytest.mark.parametrize("N", NS)
def test_wide_run_steps_piece_sums_vs_oracle(gpu, N):
    """The wide form without w: each certified piece summed from its EV count and fixed-point gamma sum.
    Every run's sums against the oracle and against the rows form (1e-11); COUNT and N_REPAIRED equal the
    rows form's."""
    bt = product_batch(N)
    dev = Dev(f"prices piece sums N={N}")
    kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_cost=False)
    red = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=False, **kw)
    rows = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=True, **kw)
    o, n = counted(red, lambda: red.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True))
    assert red.cells % 4 == 0 and red.info()["steps_group"] == 1 and n == (groups(K), K, K), n
    assert red.last_check[1:] == (0, 0)
    orow = rows.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)
    assert rows.check()[1:] == (0, 0)
    sw, st, swr, stw = np_(o["set_sum_w"]), np_(o["set_stats"]), np_(orow["set_sum_w"]), np_(orow["set_stats"])
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k], cost=False)
    dev.add("vs rows form", np.abs(sw - swr), 1e-11 + 1e-11 * np.abs(swr))
    print_repaired(f"prices piece sums N={N}", bt, st[0, :, ST.LOMPC_STAT_N_REPAIRED])
    dev.check()
    for j in (ST.LOMPC_STAT_COUNT, ST.LOMPC_STAT_N_REPAIRED, ST.LOMPC_STAT_MAX_ERR):
        np.testing.assert_array_equal(st[:, :, j], stw[:, :, j])


@pytest.mark.parametrize("N", NS)
def test_sort_sets_aggregation_vs_oracle(gpu, N):
    """sort_sets plans over the (unsorted) batch: a single run through k_agg, the wide run_steps through
    k_paths + k_aggs and its per-kernel form (bitwise the same), each run's sums against the oracle."""
    bt = product_batch(N)
    dev = Dev(f"prices sorted N={N}")
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_w=False, want_cost=False,
                     sort_sets=True)
    assert plan.launches_per_run() == 2
    o1, n = counted(plan, lambda: clone(plan.run(bt.lm_d[0], bt.lr_d[0])))
    assert n == (1, 1, 0) and plan.last_check[1:] == (0, 0), n
    ow, n = counted(plan, lambda: clone(plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)))
    assert plan.info()["steps_group"] == 0 and n == (groups(K), K, 0) and plan.last_check[1:] == (0, 0), n
    ok, n = counted(plan, lambda: plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True, per_kernel=True))
    assert n == (K, K, 0), n
    for key in ("set_sum_w", "set_stats"):
        assert torch.equal(ow[key], ok[key]) and torch.equal(ow[key][0], o1[key]), key
    sw, st = np_(ow["set_sum_w"]), np_(ow["set_stats"])
    print_repaired(f"prices sorted N={N}", bt, st[0, :, ST.LOMPC_STAT_N_REPAIRED])
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
    dev.check()


@pytest.mark.parametrize("N", NS)
def test_w0_pass_after_update_vs_oracle(gpu, N):
    """The station's w0 pass: a plan with w0 and set outputs only, created on another batch (other sizes
    and gamma) and re-targeted at the family batch by plan.update: w0 against the oracle's w[:, 0] at
    1e-9, SUM_W0 / SUM_PRICE0 / COUNT against the oracle; two launches, no k_finalize."""
    bt = product_batch(N)
    dev = Dev(f"prices w0 N={N}")
    S = 2 * bt.P
    sizes = 40 + (np.arange(S) * 37) % 90
    off0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g0 = np.concatenate([bt.consts_of(s).y_max * bt.rng.random(m) for s, m in enumerate(sizes)])
    plan = BatchPlan(bt.lompcs, torch.as_tensor(g0, device="cuda:0"), off0, sets_per_ctx=[bt.P, bt.P], want_w=False,
                     want_cost=False, want_w0=True, want_set=True, validate=False)
    plan.run(bt.lm_d[0], bt.lr_d[0])
    assert plan.check()[1:] == (0, 0)
    plan.update(bt.g, bt.off, validate=False)
    assert plan.launches_per_run() == 2
    o, n = counted(plan, lambda: clone(plan.run(bt.lm_d[0], bt.lr_d[0])))
    assert n == (1, 1, 0) and plan.last_check[1:] == (0, 0), n
    assert "w" not in o and "cost" not in o
    print_repaired(f"prices w0 N={N}", bt, np_(o["set_stats"])[:, ST.LOMPC_STAT_N_REPAIRED])
    W, _ = bt.oracle(0)
    w0 = np_(o["w0"])
    assert w0.shape == (bt.B,)
    dev.add("|dw0|", np.abs(w0 - W[:, 0]), 1e-9)
    sets_vs_oracle(dev, bt, 0, np_(o["set_sum_w"]), np_(o["set_stats"]), cost=False)
    dev.check()


@pytest.mark.parametrize("N", NS_DIRECT)
def test_direct_mode_vs_oracle(gpu, N):
    """solve_batch in mode "direct" (k_central from gamma_ref, then k_direct: every EV its own wave
    solve), per type over the product-range families: rows, cost, status and set sums against the oracle."""
    direct_vs_oracle(product_batch(N), Dev(f"prices direct N={N}"))


def direct_vs_oracle(bt, dev, loud=False):
    """loud: the never-silently-wrong contract instead of the product range's (loud_rows, FAILED EVs' w
    included).  Returns N_FAILED per set.  The C ABI counts k_direct's launches only; k_central, the
    preparation kernel of lompc_set_params in this mode, runs because gamma_ref is given."""
    N, P = bt.N, bt.P
    W, C = bt.oracle(0)
    w, cost, status = np.zeros((bt.B, N)), np.zeros(bt.B), np.zeros(bt.B, dtype=np.int8)
    sw, st = np.zeros((bt.S, N)), np.zeros((bt.S, ST.LOMPC_SET_STATS))
    for t, c in enumerate(bt.cs):
        lo = LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0, mode="direct")
        a, b = int(bt.off[t * P]), int(bt.off[(t + 1) * P])
        sl = slice(t * P, (t + 1) * P)
        lo.set_params(bt.lm[0, sl], bt.lr[0, sl], w_ref=bt.wr[sl], gamma_ref=np.full(P, 0.5 * c.y_max))
        lo.profile(enable=True)
        lo.profile(read=True, reset=True)
        r = lo.solve_batch(bt.gn[a:b], bt.off[t * P:(t + 1) * P + 1] - a, want_w=True, want_cost=True, want_status=True,
                           check=False)
        torch.cuda.synchronize()
        if not loud:
            assert lo.check_last()[1:] == (0, 0)
        assert lo.profile(read=True, reset=True)[1] == 1  # one k_direct launch
        lo.profile(enable=False)
        w[a:b], cost[a:b], status[a:b] = np_(r["w"]), np_(r["cost"]), np_(r["status"])
        sw[sl], st[sl] = np_(r["set_sum_w"]), np_(r["set_stats"])
    print_repaired(dev.name, bt, st[:, ST.LOMPC_STAT_N_REPAIRED])
    if loud:
        nf = loud_rows(dev, bt, 0, w, cost, status, sw, st, "direct", failed_w=True)
    else:
        assert np.all(ok_or_repaired(status))
        rows_vs_oracle(dev, bt, 0, w, cost)
        sets_vs_oracle(dev, bt, 0, sw, st)
        nf = st[:, ST.LOMPC_STAT_N_FAILED].astype(np.int64)
    dev.check()
    return nf


@pytest.mark.parametrize("N", NS)
def test_beyond_product_range_is_never_silently_wrong(gpu, N):
    """Dense theta * rand times 1e7 and 1e9 (the host path engine certifies no piece there and solves
    every EV individually), with a 1100-EV set at 1e7: a single run with rows and a sort_sets run.  Every
    EV whose status is OK or REPAIRED meets the bars, every other EV is FAILED and counted in its set's
    N_FAILED; a set without failures meets the set bars.  Prints which of the two happened."""
    bt = beyond_batch(N)
    dev = Dev(f"prices beyond N={N}")
    kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d)
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=True, want_cost=True, want_status=True, **kw)
    o = {k: np_(v) for k, v in clone(plan.run(bt.lm_d[0], bt.lr_d[0])).items()}
    torch.cuda.synchronize()
    agg = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=False, want_cost=False, sort_sets=True, **kw)
    oa = {k: np_(v) for k, v in clone(agg.run(bt.lm_d[0], bt.lr_d[0])).items()}
    torch.cuda.synchronize()
    status, st = o["status"], o["set_stats"]
    good = ok_or_repaired(status)
    assert np.all(good | (status == ST.LOMPC_QP_FAILED))
    W, C = bt.oracle(0)
    dev.add("|dw| of OK / REPAIRED", np.abs(o["w"] - W)[good], 1e-9)
    dev.add("cost of OK / REPAIRED", np.abs(o["cost"] - C)[good], (1e-9 + 1e-9 * np.abs(C))[good])
    osw, ow0, op0, oc = bt.oracle_sets(0)
    tally = {}
    for s in range(2 * bt.P):
        a, b = bt.off[s], bt.off[s + 1]
        nfail = int(np.sum(~good[a:b]))
        tally[bt.label(s)] = (int(np.sum(status[a:b] == ST.LOMPC_QP_REPAIRED)), nfail)
        assert st[s, ST.LOMPC_STAT_COUNT] == b - a and st[s, ST.LOMPC_STAT_N_INVALID] == 0
        assert st[s, ST.LOMPC_STAT_N_FAILED] == nfail, (bt.label(s), st[s, ST.LOMPC_STAT_N_FAILED], nfail)
        for name, sw_, st_ in (("rows", o["set_sum_w"], st), ("k_agg", oa["set_sum_w"], oa["set_stats"])):
            assert st_[s, ST.LOMPC_STAT_COUNT] == b - a
            if st_[s, ST.LOMPC_STAT_N_FAILED] == 0:
                dev.add(f"set sums ({name})", np.abs(sw_[s] - osw[s]), 1e-9 + 1e-10 * np.abs(osw[s]))
                dev.add(f"sum price0 ({name})", abs(st_[s, ST.LOMPC_STAT_SUM_PRICE0] - op0[s]), 1e-9 * max(1.0, abs(op0[s])))
                dev.add(f"sum cost ({name})", abs(st_[s, ST.LOMPC_STAT_SUM_COST] - oc[s]), 1e-9 * max(1.0, abs(oc[s])))
    print(f"prices beyond N={N}: (REPAIRED, FAILED) per set: {tally}; k_agg N_FAILED "
          f"{oa['set_stats'][:, ST.LOMPC_STAT_N_FAILED].astype(int).tolist()}; REPAIRED span of the {BIG}-EV set "
          f"{repaired_span(bt, status, BIG_BEYOND)}")
    dev.check()


def test_resolve_lists_span_more_than_one_evaluation_block(gpu):
    """The closing's re-solve must actually run across workgroup records: over the horizons, at least one
    product-range family's 1100-EV set (all_1e-12 and ramp_l1_down at lmbd_r > 0, where the host engine
    re-solves most) has REPAIRED EVs at least EVAL_BLOCK apart, that is in more than one evaluation block.
    Every such set is compared with the oracle over every EV in test_single_run_rows_vs_oracle."""
    spans = {(N, b[0]): repaired_span(product_batch(N), single_run(N)[0]["status"], b) for N in NS for b in BIG_PRODUCT}
    print(f"REPAIRED span of the product-range {BIG}-EV sets per (N, family): (small, large) {spans}")
    assert any(s >= EVAL_BLOCK for v in spans.values() for s in v), spans


def rung_forms(N):
    """Every plan form over the rung's own plan at a short horizon, under the never-silently-wrong
    contract; the kernels that ran are asserted as in the product-range cases.  Returns N_FAILED of the
    wide rows form, (K, S)."""
    bt = rung_batch(N)
    dev = Dev(f"prices rung N={N}")
    kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d)
    full = dict(want_w=True, want_cost=True, want_status=True)
    # single run with rows
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, **full, **kw)
    _, n = counted_loud(plan, lambda: plan.run(bt.lm_d[0], bt.lr_d[0]))
    assert n == (1, 1, 1), n
    one = {k: np_(v) for k, v in clone(plan.out).items()}
    print_repaired(f"prices rung single N={N}", bt, one["set_stats"][:, ST.LOMPC_STAT_N_REPAIRED])
    loud_rows(dev, bt, 0, one["w"], one["cost"], one["status"], one["set_sum_w"], one["set_stats"], "single", failed_w=True)
    # wide run_steps with rows, every run
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, **full, **kw)
    call, o = plan.steps_call(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True)
    _, n = counted_loud(plan, call)
    assert plan.info()["steps_group"] == 1 and n == (groups(K), K, K), n
    w, cost, status, sw, st = (np_(o[k]) for k in ("w", "cost", "status", "set_sum_w", "set_stats"))
    np.testing.assert_array_equal(w[0], one["w"])
    np.testing.assert_array_equal(status[0], one["status"])
    failed = np.stack([loud_rows(dev, bt, k, w[k], cost[k], status[k], sw[k], st[k], "wide rows", failed_w=True)
                       for k in range(K)])
    print(f"prices rung N={N}: N_FAILED per run and set {failed.tolist()}")
    # the same without w: piece sums
    red = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=False, want_cost=False, **kw)
    call, o = red.steps_call(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)
    _, n = counted_loud(red, call)
    assert red.info()["steps_group"] == 1 and n == (groups(K), K, K), n
    for k in range(K):
        nf = loud_sets(dev, bt, k, np_(o["set_sum_w"])[k], np_(o["set_stats"])[k], "piece sums", cost=False)
        np.testing.assert_array_equal(nf, failed[k])
    # sort_sets: k_agg, k_aggs
    agg = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=False, want_cost=False, sort_sets=True, **kw)
    _, n = counted_loud(agg, lambda: agg.run(bt.lm_d[0], bt.lr_d[0]))
    assert n == (1, 1, 0), n
    o1 = {k: np_(v) for k, v in clone(agg.out).items()}
    call, o = agg.steps_call(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)
    _, n = counted_loud(agg, call)
    assert n == (groups(K), K, 0), n
    np.testing.assert_array_equal(np_(o["set_stats"])[0], o1["set_stats"])
    for k in range(K):
        loud_sets(dev, bt, k, np_(o["set_sum_w"])[k], np_(o["set_stats"])[k], "k_aggs")
    # the w0 pass after plan.update
    sizes = 40 + (np.arange(2 * bt.P) * 37) % 90
    off0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g0 = np.concatenate([bt.consts_of(s).y_max * np.linspace(0.0, 1.0, m) for s, m in enumerate(sizes)])
    pw = BatchPlan(bt.lompcs, torch.as_tensor(g0, device="cuda:0"), off0, sets_per_ctx=[bt.P, bt.P], want_w=False,
                   want_cost=False, want_w0=True, want_set=True, validate=False)
    pw.update(bt.g, bt.off, validate=False)
    _, n = counted_loud(pw, lambda: pw.run(bt.lm_d[0], bt.lr_d[0]))
    assert n == (1, 1, 0), n
    W, _ = bt.oracle(0)
    nf = loud_sets(dev, bt, 0, np_(pw.out["set_sum_w"]), np_(pw.out["set_stats"]), "w0 pass", cost=False)
    ok = np.repeat(nf == 0, np.diff(bt.off))  # (this plan has no status output: the sets without a failure)
    dev.add("|dw0| (sets without FAILED)", np.abs(np_(pw.out["w0"]) - W[:, 0])[ok], 1e-9)
    dev.add("|dw0| (sets with FAILED)", np.abs(np_(pw.out["w0"]) - W[:, 0])[~ok], 1e-9)
    dev.check()
    return failed


@functools.lru_cache(maxsize=None)
def rung_failed(N):
    return rung_forms(N)


@functools.lru_cache(maxsize=None)
def rung_failed_direct(N):
    return direct_vs_oracle(rung_batch(N), Dev(f"prices rung direct N={N}"), loud=True)


@pytest.mark.parametrize("N", RUNG_FAILS_PATH)
def test_fixture_max_rung_short_horizons_never_silently_wrong(gpu, N):
    """The dense rung at the fixture's largest price (every price 3.885e5 theta * rand; both lmbd_r and a
    1100-EV set) below N = 24, a plan of its own through every form: single run with rows, wide run_steps
    with rows over K = 3 price draws, piece sums, k_agg / k_aggs, the w0 pass.  Every OK or REPAIRED EV at
    the bars, every other EV FAILED and counted in N_FAILED (the same counts with and without rows), the
    FAILED EVs' w at the 1e-9 bar as well, every set without a failure at the set bars."""
    rung_failed(N)


@pytest.mark.parametrize("N", RUNG_FAILS_DIRECT)
def test_fixture_max_rung_short_horizons_direct_never_silently_wrong(gpu, N):
    """The same through solve_batch in mode "direct" (k_direct's own wave solve and certificate)."""
    rung_failed_direct(N)


@pytest.mark.xfail(strict=True, reason=RUNG_DEFECT)
@pytest.mark.parametrize("N", RUNG_FAILS_PATH)
def test_fixture_max_rung_nothing_failed_plan(gpu, N):
    """What the product range promises and the engine misses here (RUNG_DEFECT): nothing FAILED.  The only
    assertion under the mark; everything else about these runs is asserted, unmarked, above."""
    failed = rung_failed(N)
    assert failed.sum() == 0, failed.tolist()


@pytest.mark.xfail(strict=True, reason=RUNG_DEFECT)
@pytest.mark.parametrize("N", RUNG_FAILS_DIRECT)
def test_fixture_max_rung_nothing_failed_direct(gpu, N):
    failed = rung_failed_direct(N)
    assert failed.sum() == 0, failed.tolist()
