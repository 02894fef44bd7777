"""The plan kernels at every gamma-cell count at which they change path, against the per-EV C oracle.

include/lompc_amd.h: LOMPC_PLAN_CELLS(g) takes 1 .. 1024 cells per set and "the answer does not depend on
it".  The cell count G is the one plan parameter that selects kernel code paths; the other plan tests run
at pick_cells' 1, 8 and 16, at 4 and 6, and one single run at 512.  What G switches in lompc_plan.hip:

  G % 4 (LQ_STEP_CELLS)   run_steps takes the wide / stepped forms only for whole path workgroups of one set;
                          otherwise one launch per kernel, the closings inside k_path_fin
  G > 16                  k_eval stages min(128, 8 G) piece slots: the EVs of cell 16 and later are re-solved
                          individually (2 cells per wave, 8 waves); fewer at long horizons (eval_cap)
  G > 64                  s_mx (the largest staged piece count) is LQ_PPL instead of a wave maximum
  G > 512 (EVAL_EVS)      the cells' counts and starts are loaded by the strided tail loop
  G vs LQ_AGG_W           k_agg / k_aggs run min(G, LQ_AGG_W) waves, each over cells wv, wv + nw, ...
  S G cell_bytes          the wide form's table ring holds min(64, wide_fit) + 1 slots, wide_fit =
                          2^30 / (S G cell_bytes) - 1, cell_bytes = 8 (16 N + 72) + 76; wide_fit < 1: a cold
                          plan takes the stepped form (else the warm plans' only), a sorted plan one k_agg per run
  G > 16, reserved        lompc_plan_reserve sizes cell-indexed buffers for max(G, 16) cells per set
  G > 1024                refused at create

CELLS: 1 .. 5 around the path workgroup, 15 / 16 / 17 around the staging limit (and LQ_AGG_W, read from
lompc_agg.hpp: one below, at, one above), 63 / 64 / 65, 511 / 512 / 513, 1024.  Horizons: N = 24 (a compiled
instantiation) and 13 (the generic <0> kernels, the odd-N row permutation).

Batch (cell_batch, a test_gpu_plan_horizons.Batch filled through Batch.take): both EV types in one plan, per
type the ragged sets [0, 1, 65, 1100] — 65 clustered (13 values five times), 1100 with five EVs each at
gamma = 0 and y_max —, one set per type with lmbd[:N] = 0, lmbd_r > 0 on some sets, w_ref given; seeds fixed
per (N, G, form).  With more cells than EVs most cells are empty and a one-EV set's cells are 2e-7 y_max / G
wide.

Reference: oracle_c.solve_batch over EVERY EV of every non-empty set.  Bars (test_gpu_plan_horizons.py's
helpers, none new): per-EV |dw| <= 1e-9; cost 1e-9 relative; set sums rtol 1e-10, atol 1e-9; a rows form
against its own per-EV sums 1e-11; close modes against each other 1e-12 with per-EV outputs bitwise; a
warm-started plan against the cold one 1e-12; COUNT exact; N_FAILED = N_INVALID = 0; every status OK or
REPAIRED.  Every case prints its largest deviations as a share of the bar and the REPAIRED count per set
before asserting (above 16 cells large counts are legitimate: unstaged cells are re-solved; printed, not
bounded — every EV is compared all the same).

Which form ran is asserted from plan.info() and the launch counts (k_path, k_eval, k_finalize) of
test_gpu_plan_horizons.counted; its docstring has the table.
"""
import os
import re

import numpy as np
import pytest
import torch

import lompc_oracle as O
import oracle_c
import test_gpu_plan_horizons as H
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, _lib
from test_gpu_plan_horizons import (Batch, Dev, clone, counted, np_, rows_vs_oracle, same_sets, sets_vs_oracle,
                                    sets_vs_own_rows)

pytestmark = pytest.mark.gpu

ST = _lib
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "incentive-design-mpc_amd", "csrc")
with open(os.path.join(CSRC, "lompc_agg.hpp")) as _f:
    LQ_AGG_W = int(re.search(r"constexpr int LQ_AGG_W = (\d+);", _f.read()).group(1))
CELLS = sorted({1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1024, LQ_AGG_W - 1, LQ_AGG_W, LQ_AGG_W + 1})
NS = [24, 13]
NG = [(n, g) for n in NS for g in CELLS]
SIZES = [0, 1, 65, 1100]
K = 3
FORMS = {"single": 1, "steps": 2, "warm": 3, "sorted": 4, "ring": 5, "big": 6, "lds": 7}
ROWS = dict(want_w=True, want_cost=True, want_status=True)
RED = dict(want_w=False, want_cost=False)


def cell_batch(N, G, form, K, sizes=SIZES, layout="ragged", drift=False):
    """The module's batch, seeded per (N, G, form).  drift: run k's prices are run 0's moved by up to 3 k
    per cent (a price loop's slowly varying prices); else every run draws its own."""
    bt = Batch.__new__(Batch)
    bt.N, bt.K = N, K
    bt.rng = rng = np.random.default_rng([FORMS[form], N, G])
    bt.cs, lompcs = H.contexts(N)
    bt.lompcs = list(lompcs)
    sizes = list(sizes)
    bt.P = P = len(sizes)
    parts = []
    for c in bt.cs:
        for m in sizes:
            g = c.y_max * rng.random(m)
            if m == 65:  # clustered, duplicated gamma
                g = rng.permutation(np.repeat(c.y_max * rng.random(13), 5))
            if m >= 600:
                g[:5] = 0.0
                g[5:10] = c.y_max
            parts.append(np.sort(g) if layout == "sorted" else g)
    draw = lambda: np.concatenate([c.theta * rng.random((P, 3 * N)) for c in bt.cs])
    if drift:
        base = draw()
        lm = np.stack([base * (1.0 + 0.03 * k * rng.random(base.shape)) for k in range(K)])
    else:
        lm = np.stack([draw() for _ in range(K)])
    lm[:, min(2, P - 1), :N] = 0.0                 # small type: no charging price (upper bound active)
    lm[:, P + int(np.argmax(sizes)), :N] = 0.0     # large type: its largest set
    mask = np.tile(np.resize([0.0, 1.0, 0.0, 1.0, 1.0], P), 2)
    lr = 0.2 * rng.random((1 if drift else K, 2 * P)) * mask
    if drift:
        lr = np.stack([lr[0] * (1.0 + 0.03 * k) for k in range(K)])
    bt.take(parts, lm, lr)
    return bt


def plan_of(bt, G, **kw):
    p = BatchPlan(bt.lompcs, bt.g, bt.off, sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, cells=G, **kw)
    assert p.cells == G
    return p


def repaired(name, st):
    print(f"{name}: REPAIRED per set {st[..., ST.LOMPC_STAT_N_REPAIRED].astype(int).tolist()}")


def status_ok(status):
    assert np.all((status == ST.LOMPC_QP_OK) | (status == ST.LOMPC_QP_REPAIRED))


def close_modes(dev, a, b):
    """test_close_in_eval_matches_k_finalize's bar: per-EV outputs bitwise, the set reductions to 1e-12."""
    for key in ("w", "cost", "status"):
        assert torch.equal(a[key], b[key]), key
    for key in ("set_sum_w", "set_stats"):
        x, y = np_(a[key]), np_(b[key])
        dev.add("close modes", np.abs(x - y), 1e-12 + 1e-12 * np.abs(y))


def single_forms(dev, bt, G, k=0):
    """(a) a single run with rows, cost and status (k_path, k_eval, k_finalize), the same with
    close_in_eval (two launches); (b) a reductions-only run (closed inside k_eval from the piece
    aggregates) — against the oracle, (b) also against (a)'s rows."""
    lm, lr = bt.lm_d[k], bt.lr_d[k]
    full = plan_of(bt, G, **ROWS)
    assert full.launches_per_run() == 3
    of, n = counted(full, lambda: clone(full.run(lm, lr)))
    assert n == (1, 1, 1), n
    cl = plan_of(bt, G, close_in_eval=True, **ROWS)
    assert cl.launches_per_run() == 2
    oc, n = counted(cl, lambda: clone(cl.run(lm, lr)))
    assert n == (1, 1, 0), n
    red = plan_of(bt, G, **RED)
    assert red.launches_per_run() == 2
    orr, n = counted(red, lambda: clone(red.run(lm, lr)))
    assert n == (1, 1, 0), n
    w, cost, sw, st = np_(of["w"]), np_(of["cost"]), np_(of["set_sum_w"]), np_(of["set_stats"])
    repaired(dev.name, st)
    status_ok(np_(of["status"]))
    rows_vs_oracle(dev, bt, k, w, cost)
    sets_vs_oracle(dev, bt, k, sw, st)
    sets_vs_own_rows(dev, bt, w, cost, sw, st)
    close_modes(dev, oc, of)
    sets_vs_oracle(dev, bt, k, np_(oc["set_sum_w"]), np_(oc["set_stats"]))
    swr, sr = np_(orr["set_sum_w"]), np_(orr["set_stats"])
    sets_vs_oracle(dev, bt, k, swr, sr, cost=False)
    sets_vs_own_rows(dev, bt, w, None, swr, sr)
    dev.add("vs rows form", np.abs(swr - sw), 1e-11 + 1e-11 * np.abs(sw))
    for s in np.flatnonzero(np.diff(bt.off) == 0):
        assert np.all(swr[s] == 0.0) and np.all(sw[s] == 0.0)


def steps_forms(dev, bt, G, K):
    """(c) run_steps over K runs, with rows (per_run) and reductions-only (per_run_sets): every run against
    the oracle and single runs, the per-kernel form bitwise; the form that ran from info() and the launch
    counts.  G % 4 == 0: the wide form (k_paths per group, k_evals, k_closes); else one launch per kernel."""
    N, wide = bt.N, G % 4 == 0
    kw = dict(ROWS)
    ref = plan_of(bt, G, **kw)
    runs = [clone(ref.run(bt.lm_d[k], bt.lr_d[k])) for k in range(K)]
    assert ref.check()[1:] == (0, 0)
    outs = []
    for split in (False, True):
        pr = plan_of(bt, G, **kw)
        o, n = counted(pr, lambda: pr.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True, per_kernel=split))
        info = pr.info()
        if wide:
            assert info["steps_group"] == 1
            if not split:
                assert n == (H.groups(K), K, K), n
            elif info["evals_staged"]:  # (diagnostic builds)
                assert n == (K, K, K), n
            else:
                assert n == (H.groups(K), K - 1, 0), n  # k_paths, then k_step's parts
        else:
            assert info["steps_group"] == 0 and n == (K, K, 0 if N + 7 <= 64 else K), n
        for k in range(K):
            for key in ("w", "cost", "status"):
                assert torch.equal(o[key][k], runs[k][key]), (split, k, key)
            for key in ("set_sum_w", "set_stats"):
                same_sets(o[key][k], runs[k][key], info["evals_staged"], (split, k, key))
        outs.append(o)
    o = outs[0]
    for key in ("w", "cost", "status"):
        assert torch.equal(o[key], outs[1][key]), key
    w, cost, sw, st = np_(o["w"]), np_(o["cost"]), np_(o["set_sum_w"]), np_(o["set_stats"])
    repaired(dev.name, st)
    status_ok(np_(o["status"]))
    for k in range(K):
        rows_vs_oracle(dev, bt, k, w[k], cost[k])
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
        sets_vs_own_rows(dev, bt, w[k], cost[k], sw[k], st[k])
    # reductions only: single runs close inside k_eval from the piece aggregates; the wide form's k_evals
    # sums the same aggregates in its own order (1e-12, test_run_steps_matches_single_runs); the
    # launch-per-kernel form runs the single runs' kernels (bitwise)
    ref = plan_of(bt, G, **RED)
    runs = [clone(ref.run(bt.lm_d[k], bt.lr_d[k])) for k in range(K)]
    assert ref.check()[1:] == (0, 0)
    outs = []
    for split in (False, True):
        pl = plan_of(bt, G, **RED)
        o, n = counted(pl, lambda: pl.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True, per_kernel=split))
        info = pl.info()
        if wide:
            assert info["steps_group"] == 1 and n == ((K, K, K) if split else (H.groups(K), K, K)), n
        else:
            assert info["steps_group"] == 0 and n == (K, K, 0), n
        for k in range(K):
            for key in ("set_sum_w", "set_stats"):
                same_sets(o[key][k], runs[k][key], wide, ("reductions", split, k, key))
        outs.append(o)
    for key in ("set_sum_w", "set_stats"):
        assert torch.equal(outs[0][key], outs[1][key]), key
    swr, sr = np_(outs[0]["set_sum_w"]), np_(outs[0]["set_stats"])
    for k in range(K):
        sets_vs_oracle(dev, bt, k, swr[k], sr[k], cost=False)
        sets_vs_own_rows(dev, bt, w[k], None, swr[k], sr[k])
    dev.add("vs rows form", np.abs(swr - sw), 1e-11 + 1e-11 * np.abs(sw))
    np.testing.assert_array_equal(sr[:, :, ST.LOMPC_STAT_COUNT], st[:, :, ST.LOMPC_STAT_COUNT])


@pytest.mark.parametrize("N,G", NG)
def test_single_runs_vs_oracle(gpu, N, G):
    """(a), (b): single_forms at every cell count."""
    bt = cell_batch(N, G, "single", 1)
    dev = Dev(f"single N={N} G={G}")
    single_forms(dev, bt, G)
    dev.check()


@pytest.mark.parametrize("N,G", NG)
def test_run_steps_vs_oracle(gpu, N, G):
    """(c): steps_forms at every cell count, K = 3."""
    bt = cell_batch(N, G, "steps", K)
    dev = Dev(f"steps N={N} G={G}")
    steps_forms(dev, bt, G, K)
    dev.check()


@pytest.mark.parametrize("N,G", NG)
def test_warm_run_steps_vs_oracle(gpu, N, G):
    """(d) a warm-started plan through run_steps, three runs at slowly varying prices (every cell's solve
    starts from the previous run's working set; twice, so the second call's first run is warm too).
    G % 4 == 0: the stepped form, one fused k_step launch per step (k_step's path part: cell = 4 b + wv,
    ceil(S G / 4) path workgroups); else one launch per kernel.  Every run against the oracle and the cold
    plan's single runs at 1e-12 (test_warm_start_and_cell_counts)."""
    bt = cell_batch(N, G, "warm", K, drift=True)
    dev = Dev(f"warm N={N} G={G}")
    cold = plan_of(bt, G, **ROWS)
    runs = [clone(cold.run(bt.lm_d[k], bt.lr_d[k])) for k in range(K)]
    assert cold.check()[1:] == (0, 0)
    warm = plan_of(bt, G, warm_start=True, **ROWS)
    for call in range(2):
        o, n = counted(warm, lambda: clone(warm.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True)))
        info = warm.info()
        if G % 4 == 0:
            assert info["steps_group"] == 1 and not info["evals_staged"] and n == (0, K - 1, 0), n
        else:
            assert info["steps_group"] == 0 and n == (K, K, 0), n
        w, cost, sw, st = np_(o["w"]), np_(o["cost"]), np_(o["set_sum_w"]), np_(o["set_stats"])
        if call == 0:
            repaired(dev.name, st)
        status_ok(np_(o["status"]))
        for k in range(K):
            wc, cc = np_(runs[k]["w"]), np_(runs[k]["cost"])
            dev.add("vs cold plan", np.abs(w[k] - wc), 1e-12)
            dev.add("vs cold plan", np.abs(cost[k] - cc), 1e-12 + 1e-12 * np.abs(cc))
            rows_vs_oracle(dev, bt, k, w[k], cost[k])
            sets_vs_oracle(dev, bt, k, sw[k], st[k])
            sets_vs_own_rows(dev, bt, w[k], cost[k], sw[k], st[k])
    dev.check()


@pytest.mark.parametrize("N,G", NG)
def test_sorted_aggregation_vs_oracle(gpu, N, G):
    """(e) gamma-sorted sets without per-EV output: a single run (k_agg: min(G, LQ_AGG_W) waves, each over
    the cells wv, wv + nw, ...), wide run_steps (k_paths + k_aggs) bitwise equal to its per-kernel form and
    to single runs; against the oracle and the full per-EV plan (1e-11, atol 1e-9, as
    test_sorted_gamma_aggregation).  A sorted plan over a set with two EVs swapped reports the set's EVs
    failed."""
    bt = cell_batch(N, G, "sorted", K, layout="sorted")
    dev = Dev(f"sorted N={N} G={G}")
    agg = plan_of(bt, G, sorted_gamma=True, **RED)
    full = plan_of(bt, G, **ROWS)
    assert agg.launches_per_run() == 2
    oa, n = counted(agg, lambda: clone(agg.run(bt.lm_d[0], bt.lr_d[0])))
    assert n == (1, 1, 0), n
    of = full.run(bt.lm_d[0], bt.lr_d[0])
    assert full.check()[1:] == (0, 0)
    sa, sf = np_(oa["set_stats"]), np_(of["set_stats"])
    repaired(dev.name, sa)
    keep = [ST.LOMPC_STAT_COUNT, ST.LOMPC_STAT_SUM_W0, ST.LOMPC_STAT_SUM_PRICE0, ST.LOMPC_STAT_SUM_COST,
            ST.LOMPC_STAT_MAX_ERR, ST.LOMPC_STAT_N_FAILED, ST.LOMPC_STAT_N_INVALID]  # (REPAIRED: the forms re-solve other EVs)
    dev.add("vs per-EV plan", np.abs(np_(oa["set_sum_w"]) - np_(of["set_sum_w"])), 1e-9 + 1e-11 * np.abs(np_(of["set_sum_w"])))
    dev.add("vs per-EV plan", np.abs(sa[:, keep] - sf[:, keep]), 1e-9 + 1e-11 * np.abs(sf[:, keep]))
    sets_vs_oracle(dev, bt, 0, np_(oa["set_sum_w"]), sa)
    rows_vs_oracle(dev, bt, 0, np_(of["w"]), np_(of["cost"]))
    ow, n = counted(agg, lambda: clone(agg.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)))
    assert agg.info()["steps_group"] == 0 and n == (H.groups(K), K, 0), n
    osq, n = counted(agg, lambda: agg.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True, per_kernel=True))
    assert n == (K, K, 0), n
    for key in ("set_sum_w", "set_stats"):
        assert torch.equal(ow[key], osq[key]), key
    for k in range(K):
        o1 = agg.run(bt.lm_d[k], bt.lr_d[k])
        assert torch.equal(o1["set_sum_w"], ow["set_sum_w"][k]) and torch.equal(o1["set_stats"], ow["set_stats"][k]), k
    assert agg.check()[1:] == (0, 0)
    sw, st = np_(ow["set_sum_w"]), np_(ow["set_stats"])
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
    # two EVs of the small type's 1100-EV set swapped: only k_agg reads the order
    g3 = bt.gn.copy()
    a = bt.off[3]
    assert g3[a + 10] != g3[a + 40]
    g3[a + 10], g3[a + 40] = g3[a + 40], g3[a + 10]
    uns = BatchPlan(bt.lompcs, torch.as_tensor(g3, device="cuda:0"), bt.off, sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d,
                    cells=G, sorted_gamma=True, **RED)
    ou = uns.run(bt.lm_d[0], bt.lr_d[0])
    with pytest.raises(Exception):
        uns.check()
    su = np_(ou["set_stats"])
    assert su[3, ST.LOMPC_STAT_N_FAILED] == 1100
    assert np.all(np.delete(su[:, ST.LOMPC_STAT_N_FAILED], 3) == 0)
    dev.check()


def test_short_table_ring(gpu):
    """N = 24, sets [0, 1, 63, 65] per type (S = 8), G = 1024: cell_bytes = 8 (16 24 + 72) + 76 = 3724,
    wide_fit = 2^30 / (8192 3724) - 1 = 34, so the wide form's ring has 35 slots and K = 40 runs take a
    group of 34 and one of 6 (two k_paths launches; run 35 reuses slot 0).  Reductions-only (k_evals,
    k_closes) and sorted (k_aggs): every run against the oracle; runs 1, 34, 35, 36 and 40 against single
    runs — the sorted form bitwise against lompc_plan_run; the reductions-only form bitwise against a
    run_steps call of that one run (the same kernels on a ring of two slots: the wide evaluation's piece
    sums equal lompc_plan_run's only to 1e-12, test_run_steps_matches_single_runs' bar, checked too)."""
    N, G, K = 24, 1024, 40
    dev = Dev("short ring")
    picks = [0, 33, 34, 35, K - 1]
    for form in ("reductions", "sorted"):
        srt = form == "sorted"
        bt = cell_batch(N, G, "ring", K, sizes=[0, 1, 63, 65], layout="sorted" if srt else "ragged")
        assert bt.S == 8
        kw = dict(sorted_gamma=True, **RED) if srt else dict(RED)
        plan = plan_of(bt, G, **kw)
        o, n = counted(plan, lambda: clone(plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)))
        assert n == ((2, K, 0) if srt else (2, K, K)), n
        assert plan.info()["steps_group"] == (0 if srt else 1)
        sw, st = np_(o["set_sum_w"]), np_(o["set_stats"])
        repaired(f"short ring {form}", st[0])
        for k in range(K):
            sets_vs_oracle(dev, bt, k, sw[k], st[k], cost=srt)
        one = plan_of(bt, G, **kw)
        for k in picks:
            o1 = clone(one.run(bt.lm_d[k], bt.lr_d[k]))
            for key in ("set_sum_w", "set_stats"):
                same_sets(o[key][k], o1[key], not srt, (form, k, key))
            if not srt:
                o2 = one.run_steps(bt.lm_d[k], bt.lr_d[k], 1, *bt.strides, per_run_sets=True)
                for key in ("set_sum_w", "set_stats"):
                    assert torch.equal(o2[key][0], o[key][k]), (form, k, key)
        assert one.check()[1:] == (0, 0)
    dev.check()


def test_plan_too_big_for_two_ring_slots(gpu):
    """N = 48, 39 sets of 1 .. 9 EVs per type (S = 78), G = 1024: 79,872 cells of 8 (16 48 + 72) + 76 =
    6796 bytes, 543 MB per table, wide_fit = 2^30 / 542,810,112 - 1 = 0.  lq_run_steps_stepped: Kc = 0, so
    a cold plan takes the warm plans' stepped form — launches 0 .. K + 1 of k_step (path, evaluation and
    closing fused), of which the K - 1 steady ones carry K_EVAL events: (0, K - 1, 0), steps_group 1.
    lompc_plan_run_steps sends a sorted reductions plan with wide_fit < 1 to its launch-per-kernel loop:
    k_path + k_agg per run, (K, K, 0), steps_group 0.  Every EV of both against the oracle.  (The rows
    plan holds its own path table and the stepped form's two: about 1.7 GB of device memory.)"""
    N, G, K = 48, 1024, 3
    sizes = [1 + p % 9 for p in range(39)]
    dev = Dev("too big")
    bt = cell_batch(N, G, "big", K, sizes=sizes)
    assert bt.S * G == 79872
    plan = plan_of(bt, G, **ROWS)
    o, n = counted(plan, lambda: clone(plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True)))
    assert plan.info()["steps_group"] == 1 and n == (0, K - 1, 0), n
    w, cost, sw, st = np_(o["w"]), np_(o["cost"]), np_(o["set_sum_w"]), np_(o["set_stats"])
    print(f"too big: REPAIRED in all {int(st[0, :, ST.LOMPC_STAT_N_REPAIRED].sum())} of {bt.B}")
    status_ok(np_(o["status"]))
    for k in range(K):
        rows_vs_oracle(dev, bt, k, w[k], cost[k])
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
        sets_vs_own_rows(dev, bt, w[k], cost[k], sw[k], st[k])
    one = plan_of(bt, G, **ROWS)
    o1 = one.run(bt.lm_d[K - 1], bt.lr_d[K - 1])
    assert one.check()[1:] == (0, 0)
    for key in ("w", "cost", "status", "set_sum_w", "set_stats"):
        assert torch.equal(o1[key], o[key][K - 1]), key
    del plan, one, o, o1
    bs = cell_batch(N, G, "big", K, sizes=sizes, layout="sorted")
    agg = plan_of(bs, G, sorted_gamma=True, **RED)
    oa, n = counted(agg, lambda: clone(agg.run_steps(bs.lm_d, bs.lr_d, K, *bs.strides, per_run_sets=True)))
    assert agg.info()["steps_group"] == 0 and n == (K, K, 0), n
    sw, st = np_(oa["set_sum_w"]), np_(oa["set_stats"])
    for k in range(K):
        sets_vs_oracle(dev, bs, k, sw[k], st[k])
    dev.check()


def test_reserved_sorted_plan_above_16_cells(gpu):
    """lompc_plan_reserve sizes the cell-indexed buffers for max(G, LQ_RESERVE_CELLS = 16) cells per set: a
    sorted plan with 32 cells and reserve = 8192, re-targeted by update at batches of 40, 5000 and 500 EVs —
    every run bitwise a fresh plan's (test_plan_update_matches_fresh_plan) and its sums the oracle's."""
    rng = np.random.default_rng(3216)
    N, G = 24, 32
    c = O.large_consts()
    lompc = LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0)
    kw = dict(sorted_gamma=True, cells=G, **RED)
    plan = None
    for m in (40, 5000, 500):
        gn = np.sort(c.y_max * rng.random(m))
        off = np.array([0, m // 3, m], dtype=np.int64)
        g = torch.as_tensor(gn, device="cuda:0")
        lmn, lrn = c.theta * rng.random((2, 3 * N)), np.array([0.1, 0.0])
        lm, lr = torch.as_tensor(lmn, device="cuda:0"), torch.as_tensor(lrn, device="cuda:0")
        if plan is None:
            plan = BatchPlan(lompc, g, off, **kw)
            plan.reserve(8192)
        else:
            plan.update(g, off)
        assert plan.cells == G
        o1 = clone(plan.run(lm, lr))
        assert plan.check()[1:] == (0, 0)
        fresh = BatchPlan(lompc, g, off, **kw)
        o2 = fresh.run(lm, lr)
        assert fresh.check()[1:] == (0, 0)
        for key in ("set_sum_w", "set_stats"):
            assert torch.equal(o1[key], o2[key]), (m, key)
        sw, st = np_(o1["set_sum_w"]), np_(o1["set_stats"])
        dev = Dev(f"reserve m={m}")
        for s in range(2):
            wo, co, nf = oracle_c.solve_batch(N, c, lmn[s], float(lrn[s]), gn[off[s]:off[s + 1]])
            assert nf == 0 and st[s, ST.LOMPC_STAT_COUNT] == off[s + 1] - off[s]
            assert st[s, ST.LOMPC_STAT_N_FAILED] == 0 and st[s, ST.LOMPC_STAT_N_INVALID] == 0
            dev.add("set sums", np.abs(sw[s] - wo.sum(0)), 1e-9 + 1e-10 * np.abs(wo.sum(0)))
            dev.add("sum cost", abs(st[s, ST.LOMPC_STAT_SUM_COST] - co.sum()), 1e-9 * max(1.0, abs(co.sum())))
        dev.check()


def test_cell_count_limits(gpu):
    """More than 1024 cells are refused at create with a message naming the limit (the plan does not exist
    yet: the text is the first context's lompc_last_error, which the exception carries); without
    LOMPC_PLAN_CELLS the plan picks 1, 8 or 16 cells by its largest set (<= 64, <= 1024, more)."""
    N = 24
    c = O.small_consts()
    lompc = LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0)
    g = torch.as_tensor(np.linspace(0.0, c.y_max, 1100), device="cuda:0")
    for cells in (1025, 2047):
        with pytest.raises(ValueError, match="at most 1024 cells"):
            BatchPlan(lompc, g[:100], np.array([0, 100], dtype=np.int64), cells=cells)
        assert b"at most 1024 cells" in lompc._lib.lompc_last_error(lompc._ctx)
    for m, want in ((1, 1), (64, 1), (65, 8), (1024, 8), (1025, 16)):
        p = BatchPlan(lompc, g[:m + 3], np.array([0, 3, m + 3], dtype=np.int64), cells=None)
        assert p.cells == want, (m, p.cells)
    assert BatchPlan(lompc, g[:100], np.array([0, 100], dtype=np.int64), cells=1024).cells == 1024


LDS_EDGE = [(64, 16), (64, 40), (64, 41), (64, 43), (64, 44), (64, 64), (64, 1024), (63, 216), (63, 217), (63, 1024),
            (59, 910), (59, 911), (58, 1024)]


@pytest.mark.parametrize("N,G", LDS_EDGE)
def test_lds_edge_of_the_staged_table(gpu, N, G):
    """Long horizons with many cells, where the evaluation's LDS request meets the workgroup limit.

    eval_lds(N, G, cap), the dynamic LDS of k_eval / k_evals / k_step for cap staged piece slots:

        cap (16 (N + 1) + 72) + 32 (N + 1) + 8 G + 4 ((G + 1) & ~1) + 12 (cap + 2)   bytes

    The kernels' static LDS (a gfx950 build, -Rpass-analysis=kernel-resource-usage): 17,344 bytes for
    k_eval<false>, k_evals and k_step, 17,376 for k_eval<true> (the form that closes in the evaluation); a
    workgroup has 163,840, which leaves 146,496 / 146,464 bytes.  With cap = min(128, 8 G) = 128 at N = 64
    the request is 145,976 + 12 G: 146,168 at G = 16 (fits), past 146,464 from G = 41 (k_eval<true>) and
    past 146,496 from G = 44 (the others); at N = 63 from G = 217, N = 62 from 391, 61 from 564, 60 from
    737, 59 from 911; at N <= 58 1024 cells fit.  Before eval_cap those plans were created, and the
    HIP runtime does not refuse such a launch: at N = 64, G = 41 the rows run (k_eval<false>, 163,816
    bytes) solved and the close_in_eval run (163,848 bytes) aborted the queue with
    HSA_STATUS_ERROR_INVALID_ALLOCATION, after which every HIP call of the process failed — so the header's
    "1 .. 1024" was false for N >= 59.
    eval_cap (lompc_plan.hip) now lowers cap by whole cells (8 slots, 16 (N + 1) + 92 bytes each) until the
    request fits beside the largest static size hipFuncGetAttributes reports: at N = 64, G >= 41 to 120
    slots (15 staged cells), as at N = 63, G >= 217 and N = 59, G >= 911; cap is unchanged wherever it
    fitted.  The cells left unstaged take the certified individual re-solve, so every pair here must SOLVE
    within the bars — single runs (a) with close_in_eval, (b), and run_steps (c) — and neither be refused
    nor fail at a run.  Sets [1, 65, 600] per type."""
    dev = Dev(f"lds edge N={N} G={G}")
    bt = cell_batch(N, G, "lds", K, sizes=[1, 65, 600])
    single_forms(dev, bt, G)
    steps_forms(dev, bt, G, K)
    dev.check()
