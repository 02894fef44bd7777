"""The engine at EV constants other than the two shipped sets, against the per-EV C oracle.

Every other GPU test builds its contexts from (delta, theta, y_max, w_max) = (0.05, 10, 0.9, 0.25) small and
(0.025, 50, 0.9, 0.15) large.  What lompc_create derives from the constants (q.scale and the tolerances built
from it, the fp32 working-set search's 1e-6 w_max and 1e-6 q.scale, the large type's knots and slopes,
q_scale = 3 theta / (4 w_max), dsmall = 2 theta^2 / 0.9^2 with the reference's LITERAL 0.9, the per-context
lookups of k_chain_price and of the plan kernels' set_consts, the price loop's m and kappa) runs here at eight
other sets, as two plans of FOUR contexts each (LOMPC_PLAN_MAX_CTX; sets_per_ctx = [P, P, P, P]):

  plan ctx type   delta  theta  y_max  w_max
  A    0   small  1e-4   0.1    0.75   0.01   gradients of order 1e-2 against the "1 +" of q.scale; y_max != 0.9
  A    1   small  50     1000   0.8    0.1    q.scale of order 1e9
  A    2   large  1e-4   1000   0.75   0.01   weak charging term, strong PWL slopes
  A    3   large  50     0.1    0.9    0.25   the opposite; w_max at the admissible maximum
  B    0   small  1      10     0.75   0.01   cap-heavy: cells fill their 8 pieces, EVs of every larger set re-solved
  B    1   small  0.025  10     0.8    0.1    next to the shipped small set: pins the literal 0.9 and w_max
  B    2   large  0.025  10     0.75   0.01   cap-heavy: 204 of 1100 re-solved at N = 48 (633 at 8 cells)
  B    3   large  1      0.1    0.8    0.1    cap-heavy

Horizons N in {13, 24, 48}: the generic <0> kernels at an odd N and two compiled instantiations.

Batch (ConstBatch, a test_gpu_plan_horizons.Batch): per context the ragged sets [0, 1, 63, 65, 1100], gamma
uniform on [0, y_max] of THAT context, five EVs each at exactly 0 and y_max in the 1100-EV set, the 65-EV set
clustered (13 values five times); prices theta_ctx * rand for K = 3 runs; one set per context with
lmbd[:N] = 0 (the 63-EV set of contexts 0 and 2, the 1100-EV set of contexts 1 and 3); lmbd_r =
3 N delta_ctx * rand on the sets of 1, 65 and 1100 EVs, 0 on the others; w_ref given.  One batch per
(plan, N) and its oracle results are built once and shared by the forms (functools.lru_cache; the sorted
forms' batch is the same draw with every set's gamma sorted); what a form draws itself (the chain's target,
the shuffle, the single-QP gammas) comes from a generator seeded per (plan, N, form).

Forms, each for both plans at each N, each identified by its launch counts (k_path, k_eval, k_finalize; the
table in test_gpu_plan_horizons.py): single run with rows (1, 1, 1); wide run_steps with rows (1, K, K); the
same without w, piece sums (1, K, K); sorted_gamma plans over the host-sorted batch, k_agg (1, 1, 0) and
k_aggs wide (1, K, 0), sort_sets over the shuffled batch (bitwise the sorted plan's) and a plan over an
unsorted set, which only k_agg reports failed; run_chain, 3 runs, step 0.5 (K, K, K): every lmbd_out[k]
against lompc_plan_run_chain's documented rule restated in numpy with EACH SET'S OWN context constants, every
run's reductions against the oracle at the recorded prices; DIRECT mode, solve_batch per context (one
k_direct launch); lompc_solve_host (LoMPC.solve_lompc) at gamma = 0, y_max and one value between, per context.

Reference: oracle_c.solve_batch over EVERY EV.  Bars (the suite's, through test_gpu_plan_horizons.py's
helpers, none new): per-EV |dw| <= 1e-9; cost, SUM_PRICE0, SUM_COST 1e-9 relative; set sums rtol 1e-10, atol
1e-9; a rows form against its own sums 1e-11; COUNT exact.  Every case prints its largest deviations as a
share of the bar first; the plan forms with rows and the single-QP call also print max |dw| / w_max per
context (w_max = 0.01 makes the absolute bar 25 times looser relative to the box; printed, not asserted).

Status contract: inside this grid nothing is FAILED or INVALID, every EV is OK or REPAIRED.  REPAIRED per set
is printed beside the host path engine's individually solved EVs at the plan's own cell count.  For plan B
at N = 48 the device must really take the re-solve route: REPAIRED > 0 in the 1100-EV sets of B0 and B2
(test_single_run_rows_vs_oracle; REPAIRED_CELLS below).

The device price loop runs at A2, B1 and B2 (N = 24, 600 EVs, two calls, the second with lmbd_r > 0, 8 cells,
linear-convex prices) through test_gpu_price_loop_shapes.py's checkers unchanged: the host C++ loop (equal
iterations, prices within 1e-9 theta, decreases at rtol 1e-8) and oracle/price_oracle.py (equal iterations,
prices within 1e-6 theta; per component 1e-6 max(theta, |lambda_i|) beyond 100 iterations), assert_form: the
persistent k_loop_run2 ran.  LOOP_SEEDS are picked on the CPU by scripts/select_constants_cases.py with
scripts/check_price_loop_seeds.py's criterion.  A2 stands for A1: at delta = 50 (A1, and A3) the oracle's first
call ends at the iteration cap for every seed 1..16 (record below), so A1 has no admissible seed; A2 keeps its
theta = 1000.  A2 is also where this module found a defect: at delta = 1e-4 the price-gradient QP's reduced
solves lost 1e-8 against a certificate of 1e-11 (1 + max |q|) and every step of the loop, host and device, ended
in "price-gradient QP: no certified optimum"; the solves now take a step of iterative refinement there
(lompc_price.cpp PriceQP::solve, lompc_pricewave.hpp; tests/test_price_host.py has the host cases).

Record of scripts/select_constants_cases.py (its lines abbreviated; the oracle solves every EV, the host path
engine fails none; "pieces/individual" of the host engine at the plan's 16 cells per set, run 0; the loop
lines of A1 and A3 from ``select_constants_cases.py loops A1 A3``).  The device's REPAIRED counts printed by
the cases equal the host engine's individual counts set by set (B, N = 48, run 0: B0 5 / 10 / 61, B2 11 / 20 /
204, B3 67):

  A0 N=13 1: 16/0, 63: 16/0, 65: 16/0, 1100: 16/0; (at 8 cells: 8/0) all runs individual 0, max |dw| 6.94e-18
  A1 N=13 1: 16/0, 63: 31/0, 65: 28/0, 1100: 22/0; (at 8 cells: 14/0) all runs individual 0, max |dw| 8.19e-16
  A2 N=13 1: 16/0, 63: 16/0, 65: 17/0, 1100: 16/0; (at 8 cells: 8/0) all runs individual 0, max |dw| 5.20e-18
  A3 N=13 1: 16/0, 63: 45/0, 65: 37/0, 1100: 42/0; (at 8 cells: 34/0) all runs individual 0, max |dw| 1.95e-15
  A0 N=24 1: 16/0, 63: 16/0, 65: 16/0, 1100: 16/0; (at 8 cells: 8/0) all runs individual 0, max |dw| 1.21e-17
  A1 N=24 1: 16/0, 63: 30/0, 65: 24/0, 1100: 24/54; (at 8 cells: 16/113) all runs individual 182, max |dw| 3.03e-15
  A2 N=24 1: 16/0, 63: 16/0, 65: 17/0, 1100: 16/0; (at 8 cells: 8/0) all runs individual 0, max |dw| 1.04e-17
  A3 N=24 1: 16/0, 63: 45/0, 65: 34/0, 1100: 43/55; (at 8 cells: 35/119) all runs individual 111, max |dw| 5.48e-15
  A0 N=48 1: 16/0, 63: 16/0, 65: 16/0, 1100: 18/0; (at 8 cells: 10/0) all runs individual 0, max |dw| 1.56e-17
  A1 N=48 1: 16/0, 63: 31/0, 65: 29/0, 1100: 23/68; (at 8 cells: 15/133) all runs individual 202, max |dw| 8.14e-15
  A2 N=48 1: 16/0, 63: 16/0, 65: 16/0, 1100: 18/0; (at 8 cells: 10/0) all runs individual 0, max |dw| 1.21e-17
  A3 N=48 1: 16/0, 63: 44/0, 65: 37/0, 1100: 45/62; (at 8 cells: 35/130) all runs individual 186, max |dw| 1.47e-14
  B0 N=13 1: 16/0, 63: 29/0, 65: 34/0, 1100: 37/0; (at 8 cells: 25/59) all runs individual 0, max |dw| 1.04e-17
  B1 N=13 1: 16/0, 63: 21/0, 65: 21/0, 1100: 18/0; (at 8 cells: 10/0) all runs individual 0, max |dw| 8.33e-17
  B2 N=13 1: 16/0, 63: 29/0, 65: 38/0, 1100: 32/0; (at 8 cells: 24/0) all runs individual 0, max |dw| 8.67e-18
  B3 N=13 1: 16/0, 63: 74/0, 65: 62/0, 1100: 70/7; (at 8 cells: 52/118) all runs individual 35, max |dw| 4.86e-16
  B0 N=24 1: 16/0, 63: 48/0, 65: 48/0, 1100: 52/38; (at 8 cells: 36/154) all runs individual 68, max |dw| 2.43e-17
  B1 N=24 1: 16/0, 63: 21/0, 65: 23/0, 1100: 24/0; (at 8 cells: 16/0) all runs individual 0, max |dw| 1.39e-16
  B2 N=24 1: 16/0, 63: 43/0, 65: 74/0, 1100: 73/12; (at 8 cells: 52/107) all runs individual 12, max |dw| 4.34e-17
  B3 N=24 1: 16/0, 63: 74/0, 65: 74/0, 1100: 71/16; (at 8 cells: 56/217) all runs individual 53, max |dw| 1.08e-15
  B0 N=48 1: 16/0, 63: 83/5, 65: 82/10, 1100: 80/61; (at 8 cells: 55/210) all runs individual 233, max |dw| 1.41e-16
  B1 N=48 1: 16/0, 63: 29/0, 65: 33/0, 1100: 31/0; (at 8 cells: 23/0) all runs individual 0, max |dw| 1.94e-16
  B2 N=48 1: 16/0, 63: 120/11, 65: 118/20, 1100: 123/204; (at 8 cells: 64/633) all runs individual 862, max |dw| 4.23e-17
  B3 N=48 1: 16/0, 63: 76/0, 65: 77/0, 1100: 84/67; (at 8 cells: 60/306) all runs individual 170, max |dw| 4.19e-15

  loop A1 seeds 1..16  call 0: iter 999 (the cap) for every seed                                         no
  loop A3 seed 1       call 0: iter 999, call 1: iter 999                                                no
  loop A2 seed 1  call 0: iter 146 closest |err - tol| / tol 1.684e-02  call 1: iter 5 closest 1.094e-03  SELECTED
  loop B1 seed 1  call 0: iter  22 closest |err - tol| / tol 1.384e-02  call 1: iter 3 closest 6.908e-02  SELECTED
  loop B2 seed 1  call 0: iter  13 closest |err - tol| / tol 1.303e-02  call 1: iter 7 closest 2.433e-02  SELECTED
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lompc_oracle as O
import oracle_c
import price_oracle as PO
import test_gpu_price_loop_shapes as PL
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, _lib, settings
from test_gpu_plan_horizons import (ST, Batch, Dev, clone, counted, groups, np_, phi, rows_vs_oracle, sets_vs_oracle,
                                    sets_vs_own_rows)
from test_gpu_plan_prices import direct_vs_oracle, ok_or_repaired, print_repaired

pytestmark = pytest.mark.gpu

C = O.OracleConstants
PLANS = {
    "A": (C(1e-4, 0.1, 0.75, 0.01, "small"), C(50.0, 1000.0, 0.8, 0.1, "small"),
          C(1e-4, 1000.0, 0.75, 0.01, "large"), C(50.0, 0.1, 0.9, 0.25, "large")),
    "B": (C(1.0, 10.0, 0.75, 0.01, "small"), C(0.025, 10.0, 0.8, 0.1, "small"),
          C(0.025, 10.0, 0.75, 0.01, "large"), C(1.0, 0.1, 0.8, 0.1, "large")),
}
NS = [13, 24, 48]
CASES = [(p, n) for p in PLANS for n in NS]
SIZES = [0, 1, 63, 65, 1100]
BIG = SIZES.index(1100)
K = 3
FORMS = {"batch": 0, "sorted": 4, "chain": 5, "host": 7}
REPAIRED_CELLS = None  # cells of the (B, 48) run whose REPAIRED counts are asserted (None: the plan's choice)
LOOP_N, LOOP_EVS, LOOP_CELLS, LOOP_PT = 24, 600, 8, "linear-convex"
LOOP_SEEDS = {("A", 2): 1, ("B", 1): 1, ("B", 2): 1}


def seed_of(plan, N, form):
    return 9000000 + 100000 * "AB".index(plan) + 1000 * FORMS[form] + N


def lc_of(c):
    return LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type)


@functools.lru_cache(maxsize=None)
def contexts(plan, N):
    return tuple(LoMPC(N, lc_of(c), device=0) for c in PLANS[plan])


class ConstBatch(Batch):
    """test_gpu_plan_horizons.Batch over the four contexts of a plan of PLANS (see the module docstring)."""

    def __init__(self, plan, N, layout="ragged", device=True):
        self.plan, self.N, self.K = plan, N, K
        self.rng = rng = np.random.default_rng(seed_of(plan, N, "batch"))
        self.cs = PLANS[plan]
        self.lompcs = list(contexts(plan, N)) if device else None
        self.P = P = len(SIZES)
        parts = []
        for c in self.cs:
            for m in SIZES:
                g = c.y_max * rng.random(m)
                if m == 65:  # clustered, duplicated gamma
                    g = rng.permutation(np.repeat(c.y_max * rng.random(13), 5))
                if m >= 1000:
                    g[:5] = 0.0
                    g[5:10] = c.y_max
                if layout == "sorted":
                    g = np.sort(g)
                parts.append(g)
        lm = np.stack([np.concatenate([c.theta * rng.random((P, 3 * N)) for c in self.cs]) for _ in range(K)])
        for t in range(len(self.cs)):  # no charging price (upper bound active): the 63-EV or the 1100-EV set
            lm[:, t * P + (2 if t % 2 == 0 else BIG), :N] = 0.0
        mask = np.resize([0.0, 1.0, 0.0, 1.0, 1.0], P)
        lr = np.concatenate([3 * N * c.delta * rng.random((K, P)) * mask for c in self.cs], axis=1)
        self.take(parts, lm, lr, device=device)
        self._host = None

    def label(self, s):
        return f"{self.plan}{s // self.P}/{SIZES[s % self.P]}"

    def at_prices(self, lm):
        """The same batch at one run of other prices lm (S, 3N) (the oracle recomputed)."""
        at = Batch.__new__(ConstBatch)
        at.__dict__.update(self.__dict__)
        at.lm, at.lr, at._oracle = lm[None], self.lr[:1], {}
        return at


@functools.lru_cache(maxsize=None)
def batch(plan, N, layout="ragged"):
    return ConstBatch(plan, N, layout)


def plan_cells(max_set):
    """The engine's gamma cells per set from the plan's largest set (pick_cells, lompc_plan.hip)."""
    return 1 if max_set <= 64 else (8 if max_set <= 1024 else 16)


def tally(name, bt, status):
    """Printed before anything is asserted: (REPAIRED, FAILED, INVALID or other) of the sets that have any."""
    rows = []
    for s in range(bt.S):
        st = status[..., bt.off[s]:bt.off[s + 1]]
        t = (int(np.sum(st == ST.LOMPC_QP_REPAIRED)), int(np.sum(st == ST.LOMPC_QP_FAILED)),
             int(np.sum(~ok_or_repaired(st) & (st != ST.LOMPC_QP_FAILED))))
        if any(t):
            rows.append(f"{bt.label(s)} {t}")
    print(f"{name}: (REPAIRED, FAILED, other) per set: " + ", ".join(rows))


def dw_rel(name, bt, k, w):
    """max |dw| / w_max per context (printed, not asserted)."""
    W, _ = bt.oracle(k)
    out = []
    for t, c in enumerate(bt.cs):
        a, b = bt.off[t * bt.P], bt.off[(t + 1) * bt.P]
        out.append(f"{bt.plan}{t} {np.max(np.abs(w[a:b] - W[a:b])) / c.w_max:.3e}")
    print(f"{name}: max |dw| / w_max per context: " + ", ".join(out))


def nothing_failed(bt, st):
    assert np.all(st[..., ST.LOMPC_STAT_N_FAILED] == 0) and np.all(st[..., ST.LOMPC_STAT_N_INVALID] == 0), \
        (st[..., ST.LOMPC_STAT_N_FAILED].tolist(), st[..., ST.LOMPC_STAT_N_INVALID].tolist())


def spc(bt):
    return [bt.P] * len(bt.cs)


# ------------------------------------------------------------------ 1. single run with rows
@functools.lru_cache(maxsize=None)
def single_run(plan, N, cells=None):
    bt = batch(plan, N)
    pl = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=spc(bt), w_ref=bt.wr_d, want_w=True, want_cost=True,
                   want_status=True, cells=cells)
    assert pl.launches_per_run() == 3
    o, n = counted(pl, lambda: clone(pl.run(bt.lm_d[0], bt.lr_d[0])))
    return {k: np_(v) for k, v in o.items()}, n, pl.last_check, pl.cells


def check_single(bt, name, o, n, chk, cells):
    dev = Dev(name)
    print(f"{name}: launches (k_path, k_eval, k_finalize) {n}, cells {cells}")
    tally(name, bt, o["status"])
    print_repaired(name, bt, o["set_stats"][:, ST.LOMPC_STAT_N_REPAIRED], cells=cells)
    dw_rel(name, bt, 0, o["w"])
    assert n == (1, 1, 1), n
    rows_vs_oracle(dev, bt, 0, o["w"], o["cost"])
    nothing_failed(bt, o["set_stats"])
    sets_vs_oracle(dev, bt, 0, o["set_sum_w"], o["set_stats"])
    sets_vs_own_rows(dev, bt, o["w"], o["cost"], o["set_sum_w"], o["set_stats"])
    dev.check()
    assert np.all(ok_or_repaired(o["status"])) and chk[1:] == (0, 0)
    nrep = [int(np.sum(o["status"][bt.off[s]:bt.off[s + 1]] == ST.LOMPC_QP_REPAIRED)) for s in range(bt.S)]
    np.testing.assert_array_equal(o["set_stats"][:, ST.LOMPC_STAT_N_REPAIRED], nrep)
    assert chk[0] == sum(nrep)
    return nrep


@pytest.mark.parametrize("plan,N", CASES)
def test_single_run_rows_vs_oracle(gpu, plan, N):
    """k_path, k_eval, k_finalize, one launch each, with rows: every EV of the four contexts against the
    oracle, the set reductions against the oracle and the run's own rows.  Plan B at N = 48: REPAIRED > 0 in
    the 1100-EV sets of B0 and B2 (the individual re-solve really runs), at REPAIRED_CELLS."""
    bt = batch(plan, N)
    o, n, chk, cells = single_run(plan, N)
    assert cells == plan_cells(max(SIZES))
    nrep = check_single(bt, f"constants single {plan} N={N}", o, n, chk, cells)
    if (plan, N) == ("B", 48):
        if REPAIRED_CELLS is not None:
            o, n, chk, cells = single_run(plan, N, REPAIRED_CELLS)
            assert cells == REPAIRED_CELLS
            nrep = check_single(bt, f"constants single {plan} N={N} cells={cells}", o, n, chk, cells)
        assert nrep[0 * bt.P + BIG] > 0 and nrep[2 * bt.P + BIG] > 0, nrep


# ------------------------------------------------------------------ 2. wide run_steps with rows
@pytest.mark.parametrize("plan,N", CASES)
def test_wide_run_steps_rows_vs_oracle(gpu, plan, N):
    """Wide run_steps (k_paths, k_evals, k_closes), K = 3 runs with rows kept per run: every run's w, cost,
    status and set reductions against the oracle; run 0 bitwise the single run's."""
    bt = batch(plan, N)
    name = f"constants wide rows {plan} N={N}"
    dev = Dev(name)
    pl = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=spc(bt), w_ref=bt.wr_d, want_w=True, want_cost=True,
                   want_status=True)
    o, n = counted(pl, lambda: pl.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True))
    info = pl.info()
    w, cost, status, sw, st = (np_(o[k]) for k in ("w", "cost", "status", "set_sum_w", "set_stats"))
    print(f"{name}: launches {n}, steps_group {info['steps_group']}, cells {pl.cells}")
    tally(name, bt, status)
    print_repaired(name, bt, st[0, :, ST.LOMPC_STAT_N_REPAIRED], cells=pl.cells)
    for k in range(K):
        dw_rel(f"{name} run {k}", bt, k, w[k])
    assert pl.cells % 4 == 0 and info["steps_group"] == 1 and n == (groups(K), K, K), n
    for k in range(K):
        rows_vs_oracle(dev, bt, k, w[k], cost[k])
    nothing_failed(bt, st)
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
        sets_vs_own_rows(dev, bt, w[k], cost[k], sw[k], st[k])
    dev.check()
    assert np.all(ok_or_repaired(status)) and pl.last_check[1:] == (0, 0)
    one = single_run(plan, N)[0]
    for key, got in (("w", w), ("cost", cost), ("status", status)):
        np.testing.assert_array_equal(got[0], one[key], err_msg=key)


# ------------------------------------------------------------------ 3. wide run_steps without rows
@pytest.mark.parametrize("plan,N", CASES)
def test_wide_run_steps_piece_sums_vs_oracle(gpu, plan, N):
    """The wide form without w: each certified piece summed from its EV count and fixed-point gamma sum,
    the other EVs re-solved in the closing.  Every run's reductions against the oracle."""
    bt = batch(plan, N)
    name = f"constants piece sums {plan} N={N}"
    dev = Dev(name)
    pl = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=spc(bt), w_ref=bt.wr_d, want_w=False, want_cost=False)
    o, n = counted(pl, lambda: pl.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True))
    sw, st = np_(o["set_sum_w"]), np_(o["set_stats"])
    print(f"{name}: launches {n}, steps_group {pl.info()['steps_group']}, cells {pl.cells}")
    print_repaired(name, bt, st[0, :, ST.LOMPC_STAT_N_REPAIRED], cells=pl.cells)
    assert pl.cells % 4 == 0 and pl.info()["steps_group"] == 1 and n == (groups(K), K, K), n
    nothing_failed(bt, st)
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k], cost=False)
    dev.check()
    assert pl.last_check[1:] == (0, 0)
    for s in np.flatnonzero(np.diff(bt.off) == 0):
        assert np.all(sw[:, s] == 0.0)


# ------------------------------------------------------------------ 4. gamma-sorted plans
@pytest.mark.parametrize("plan,N", CASES)
def test_sorted_gamma_aggregation_vs_oracle(gpu, plan, N):
    """sorted_gamma plans over the host-sorted batch: a single run (k_agg), the wide run_steps (k_paths +
    k_aggs; run 0 bitwise the single run's), sort_sets over the shuffled batch (bitwise the sorted plan's);
    every run's reductions against the oracle.  A sorted plan over an unsorted set reports the set's EVs
    failed: only k_agg reads the order."""
    bt = batch(plan, N, "sorted")
    name = f"constants sorted {plan} N={N}"
    dev = Dev(name)
    rng = np.random.default_rng(seed_of(plan, N, "sorted"))
    kw = dict(sets_per_ctx=spc(bt), w_ref=bt.wr_d, want_w=False, want_cost=False)
    agg = BatchPlan(bt.lompcs, bt.g, bt.off, sorted_gamma=True, **kw)
    assert agg.launches_per_run() == 2
    o1, n1 = counted(agg, lambda: clone(agg.run(bt.lm_d[0], bt.lr_d[0])))
    ow, nw = counted(agg, lambda: clone(agg.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)))
    shuf = np.concatenate([rng.permutation(bt.gn[a:b]) for a, b in zip(bt.off[:-1], bt.off[1:])])
    srt = BatchPlan(bt.lompcs, torch.as_tensor(shuf, device="cuda:0"), bt.off, sort_sets=True, **kw)
    os_, ns = counted(srt, lambda: srt.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True))
    sw, st = np_(ow["set_sum_w"]), np_(ow["set_stats"])
    print(f"{name}: launches k_agg {n1}, k_aggs {nw}, sort_sets {ns}; steps_group {agg.info()['steps_group']}, cells {agg.cells}")
    print_repaired(name, bt, st[0, :, ST.LOMPC_STAT_N_REPAIRED], cells=agg.cells)
    assert n1 == (1, 1, 0) and agg.info()["steps_group"] == 0 and nw == ns == (groups(K), K, 0), (n1, nw, ns)
    nothing_failed(bt, st)
    nothing_failed(bt, np_(o1["set_stats"]))
    sets_vs_oracle(dev, bt, 0, np_(o1["set_sum_w"]), np_(o1["set_stats"]))
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
    dev.check()
    for key in ("set_sum_w", "set_stats"):
        assert torch.equal(ow[key][0], o1[key]), key
        assert torch.equal(os_[key], ow[key]), key
    assert agg.last_check[1:] == (0, 0) and srt.last_check[1:] == (0, 0)
    # an unsorted set (two EVs of context 3's 63-EV set swapped): k_agg reports its EVs failed
    s = 3 * bt.P + 2
    g3 = bt.gn.copy()
    a = bt.off[s]
    g3[a + 10], g3[a + 40] = g3[a + 40], g3[a + 10]
    uns = BatchPlan(bt.lompcs, torch.as_tensor(g3, device="cuda:0"), bt.off, sorted_gamma=True, **kw)
    ou = uns.run(bt.lm_d[0], bt.lr_d[0])
    with pytest.raises(Exception):
        uns.check()
    assert np_(ou["set_stats"])[s, ST.LOMPC_STAT_N_FAILED] == 63


# ------------------------------------------------------------------ 5. run_chain
@pytest.mark.parametrize("plan,N", CASES)
def test_run_chain_rule_and_oracle(gpu, plan, N):
    """run_chain, 3 dependent runs at step 0.5 (k_chain_price between them, the only reader of theta, w_max
    and q_scale per context outside the solves): every lmbd_out[k] equals
    max(0, lmbd + step (phi(sum_w / count) - phi(w_target))) with phi of the SET'S OWN context (rtol 1e-14,
    atol 1e-14 theta: every term of the rule is at most theta in magnitude, a few roundings each), an empty
    set keeps its prices, and every run's reductions and the last run's rows equal the oracle's at the
    recorded prices."""
    step = 0.5
    bt = batch(plan, N)
    name = f"constants chain {plan} N={N}"
    dev = Dev(name)
    rng = np.random.default_rng(seed_of(plan, N, "chain"))
    wt = np.concatenate([c.w_max * (0.2 + 0.6 * rng.random((bt.P, N))) for c in bt.cs])
    pl = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=spc(bt), w_ref=torch.as_tensor(wt, device="cuda:0"),
                   want_w=True, want_cost=True, want_status=True, close_in_finalize=True)
    assert pl.launches_per_run() == 3
    out, n = counted(pl, lambda: pl.run_chain(bt.lm[0], bt.lr_d[0], wt, step, K))
    lm, sw, st = np_(out["lmbd"]), np_(out["set_sum_w"]), np_(out["set_stats"])
    w, cost, status = np_(out["w"]), np_(out["cost"]), np_(out["status"])
    print(f"{name}: launches {n}, cells {pl.cells}")
    tally(name, bt, status)
    assert n == (K, K, K), n
    nothing_failed(bt, st)
    np.testing.assert_array_equal(lm[0], bt.lm[0])
    count = np.diff(bt.off)
    for k in range(1, K):
        for s in range(bt.S):
            if count[s] == 0:
                np.testing.assert_array_equal(lm[k, s], lm[k - 1, s])
                continue
            c = bt.consts_of(s)
            wb = sw[k - 1, s] / st[k - 1, s, ST.LOMPC_STAT_COUNT]
            exp = np.maximum(0.0, lm[k - 1, s] + step * (phi(c, wb) - phi(c, wt[s])))
            dev.add("chain rule", np.abs(lm[k, s] - exp), 1e-14 * c.theta + 1e-14 * np.abs(exp))
            assert not np.array_equal(lm[k, s], lm[k - 1, s]), (k, s)  # the prices move
    for k in range(K):
        at = bt.at_prices(lm[k])
        sets_vs_oracle(dev, at, 0, sw[k], st[k])
        if k == K - 1:
            dw_rel(name, at, 0, w)
            rows_vs_oracle(dev, at, 0, w, cost)
            sets_vs_own_rows(dev, at, w, cost, sw[k], st[k])
    dev.check()
    assert np.all(ok_or_repaired(status)) and pl.last_check[1:] == (0, 0)


# ------------------------------------------------------------------ 6. DIRECT mode, 7. the single-QP call
@pytest.mark.parametrize("plan,N", CASES)
def test_direct_mode_vs_oracle(gpu, plan, N):
    """solve_batch in mode "direct" (k_central from gamma_ref, then k_direct: every EV its own wave solve),
    per context: rows, cost, status and set sums against the oracle (test_gpu_plan_prices.direct_vs_oracle)."""
    nf = direct_vs_oracle(batch(plan, N), Dev(f"constants direct {plan} N={N}"))
    assert nf.sum() == 0


@pytest.mark.parametrize("plan,N", CASES)
def test_solve_host_vs_oracle(gpu, plan, N):
    """lompc_solve_host (LoMPC.solve_lompc's route) per context at the 1100-EV set's prices of each run:
    gamma = 0, y_max and one value between, against the oracle."""
    bt = batch(plan, N)
    name = f"constants solve_host {plan} N={N}"
    dev = Dev(name)
    rng = np.random.default_rng(seed_of(plan, N, "host"))
    rel = []
    for t, c in enumerate(bt.cs):
        lo = LoMPC(N, lc_of(c), device=0)
        g = np.array([0.0, c.y_max, c.y_max * rng.random()])
        worst = 0.0
        for k in range(K):
            lm, lr = bt.lm[k, t * bt.P + BIG], float(bt.lr[k, t * bt.P + BIG])
            W, Cc, nf = oracle_c.solve_batch(N, c, lm, lr, g)
            assert nf == 0
            for i, gi in enumerate(g):
                wi, ci = lo.solve_lompc(lm, lr, float(gi))
                assert wi.shape == (N,)
                dev.add("|dw|", np.abs(wi - W[i]), 1e-9)
                dev.add("cost", abs(ci - Cc[i]), 1e-9 + 1e-9 * abs(Cc[i]))
                worst = max(worst, float(np.max(np.abs(wi - W[i]))) / c.w_max)
        rel.append(f"{plan}{t} {worst:.3e}")
    print(f"{name}: max |dw| / w_max per context: " + ", ".join(rel))
    dev.check()


# ------------------------------------------------------------------ the admissible range and the context limit
def test_five_contexts_are_refused(gpu):
    """A plan holds at most LOMPC_PLAN_MAX_CTX = 4 contexts: the binding raises ValueError, and
    lompc_plan_create itself returns LOMPC_ERR_INVALID_ARG and no plan."""
    assert ST.LOMPC_PLAN_MAX_CTX == 4
    N = 13
    los = list(contexts("A", N)) + [LoMPC(N, lc_of(PLANS["B"][0]), device=0)]
    g = torch.as_tensor(0.5 * np.ones(5), device="cuda:0")
    off = np.arange(6, dtype=np.int64)
    with pytest.raises(ValueError):
        BatchPlan(los, g, off, sets_per_ctx=[1] * 5)
    four = BatchPlan(los[:4], g[:4], off[:5], sets_per_ctx=[1] * 4)  # (the same call with four is accepted)
    assert four.info()["sets"] == 4
    lib = _lib.load()
    ctxs = (ctypes.c_void_p * 5)(*[x._ctx.value for x in los])
    spc5 = np.ones(5, dtype=np.int64)
    handle = ctypes.c_void_p()
    rc = lib.lompc_plan_create(5, ctypes.cast(ctxs, ctypes.c_void_p), spc5.ctypes.data, 5, g.data_ptr(), off.ctypes.data,
                               None, 0, torch.cuda.current_stream(0).cuda_stream, ctypes.byref(handle))
    assert rc == ST.LOMPC_ERR_INVALID_ARG and not handle.value, (rc, handle.value)


def test_admissible_range_ends_are_accepted(gpu):
    """LoMPC accepts y_max = 0.75 and 0.9 and w_max = 0.25 exactly, as the reference does (lompc.py:36-38),
    solves there like the oracle, and refuses the next value outside."""
    N = 5
    rng = np.random.default_rng(31)
    dev = Dev("constants range ends")
    for c in (C(0.05, 10.0, 0.75, 0.25, "small"), C(0.05, 10.0, 0.9, 0.25, "large"),
              C(0.025, 50.0, 0.75, 0.25, "large"), C(0.025, 50.0, 0.9, 0.25, "small")):
        lo = LoMPC(N, lc_of(c), device=0)
        lm, lr = c.theta * rng.random(3 * N), 3 * N * c.delta * rng.random()
        g = np.array([0.0, c.y_max, c.y_max * rng.random()])
        lo.set_params(lm, lr)
        r = lo.solve_batch(g, want_w=True, want_cost=True)
        W, Cc, nf = oracle_c.solve_batch(N, c, lm, lr, g)
        assert nf == 0
        dev.add("|dw|", np.abs(np_(r["w"]) - W), 1e-9)
        dev.add("cost", np.abs(np_(r["cost"]) - Cc), 1e-9 + 1e-9 * np.abs(Cc))
    dev.check()
    for bad in (C(0.05, 10.0, np.nextafter(0.75, 0.0), 0.25, "small"), C(0.05, 10.0, np.nextafter(0.9, 1.0), 0.25, "small"),
                C(0.05, 10.0, 0.9, np.nextafter(0.25, 1.0), "small")):
        with pytest.raises(AssertionError):
            LoMPC(N, lc_of(bad), device=0)


# ------------------------------------------------------------------ the device price loop
def loop_calls(plan, ctx, seed):
    """[(y0, w_ref, lmbd_r)] of the two calls (test_gpu_price_loop_shapes.spread_calls' pattern at the
    context's constants): the second with lmbd_r > 0."""
    c = PLANS[plan][ctx]
    rng = np.random.default_rng(9900000 + 1000 * "AB".index(plan) + 100 * ctx + seed)
    out = []
    for call in range(2):
        y0 = 0.3 + (0.02 + 0.02 * call) * c.y_max * rng.random(LOOP_EVS)
        w_ref = c.w_max * (0.2 + 0.6 * rng.random(LOOP_N))
        lr = 0.0 if call == 0 else 3.0 * LOOP_N * c.delta * (0.25 + 0.5 * rng.random())
        out.append((y0, w_ref, lr))
    return out


@functools.lru_cache(maxsize=None)
def oracle_loop(plan, ctx, seed):
    c = PLANS[plan][ctx]
    po = PO.OraclePriceSolver(LOOP_N, c, LOOP_PT)
    po.warm = True
    out = []
    for y0, w_ref, lr in loop_calls(plan, ctx, seed):
        po.set_charge_levels(y0)
        lmo, sto = po.compute_optimal_prices(w_ref, lr)
        lmo = lmo.copy()
        w0o, p0o = po.get_w0_price0_batch(lmo[: po.r], lr)
        out.append((lmo, sto, w0o, p0o))
    return out


@pytest.mark.parametrize("plan,ctx", list(LOOP_SEEDS), ids=[f"{p}{t}" for p, t in LOOP_SEEDS])
def test_device_price_loop(gpu, monkeypatch, plan, ctx):
    """k_loop_run2<24> (theta, w_max, m = 2 delta theta^2, kappa = lmbd_r / delta from the context) over two
    consecutive calls on 600 EVs, against the host loop and the oracle loop."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c = PLANS[plan][ctx]
    seed = LOOP_SEEDS[plan, ctx]
    dev_ = PL.solver(LOOP_N, lc_of(c), LOOP_PT, LOOP_CELLS)
    host = PL.solver(LOOP_N, lc_of(c), LOOP_PT, LOOP_CELLS, device_loop=False)
    orc = oracle_loop(plan, ctx, seed)
    for call, (y0, w_ref, lr) in enumerate(loop_calls(plan, ctx, seed)):
        rd = PL.run_loop(dev_, y0, w_ref, lr)
        print(f"constants loop {plan}{ctx} call {call}: iterations device {rd[1]['iter']}, oracle {orc[call][1]['iter']}; "
              f"launches {rd[3]}; max |dlmbd| / theta vs oracle {np.max(np.abs(rd[0] - orc[call][0])) / c.theta:.3e}")
        PL.assert_form(dev_, rd[1], rd[3], LOOP_CELLS)
        PL.compare_host(rd, PL.run_loop(host, y0, w_ref, lr), c.theta)
        PL.compare_oracle(dev_, rd, orc[call], lr, c)
        assert 3 <= orc[call][1]["iter"] < PO.MAX_ITERS - 1 or call > 0
