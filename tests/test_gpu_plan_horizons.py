"""Every plan form of the PATH engine at every horizon class, against the per-EV C oracle.

The engine compiles each plan kernel for N = 12, 16, 24, 48 and a generic <0> form that serves every
other horizon from 1 to 64 (LOMPC_MAX_N-strided records, the odd-N row permutation of the evaluation's
LDS table).  test_gpu_pipeline.py / test_gpu_chain.py run the forms below at 24 and 48 only; here they
run at N in {1, 2, 5, 12, 13, 16, 32, 63, 64}: 12 and 16 are the other two compiled instantiations,
the rest take <0> (5, 13, 63 odd; 63 and 64 at the table's edge).

Batch: both EV types in one plan (sets_per_ctx = [P, P]), per type the ragged sets [0, 1, 63, 65, 1100]
(empty, one EV, a wave minus one, a wave plus one — clustered, duplicated gamma —, more than one
evaluation block: gamma uniform over [0, y_max] with five EVs each at exactly 0 and y_max).  Prices
theta * rand; one set per type with lmbd[:N] = 0 (upper bound active); lmbd_r > 0 on some sets; w_ref
given.  Seeds fixed per (N, form).  The ring-wrap cases (K = 66 > 64: two path groups) run at N = 13 and
16 without the 1100-EV set.

Reference: oracle_c.solve_batch over EVERY EV of every non-empty set.  Bars (test_gpu_pipeline.py's, none
new): per-EV |dw| <= 1e-9; cost 1e-9 relative; set sums vs the oracle's per-EV sums rtol 1e-10, atol
1e-9; a rows form vs its own per-EV sums 1e-11; COUNT exact; N_FAILED = N_INVALID = 0; SUM_PRICE0 within
1e-9 relative of the oracle's price0 formula (price_oracle.OraclePriceSolver.get_w0_price0_batch).  Every
case prints its largest deviations and their ratio to the bar before asserting.

Every case asserts which kernel form ran, from what the API exposes: plan.launches_per_run(),
plan.info() (steps_group: the stepped / wide run_steps has run; evals_staged: its evaluation is
k_evals_st) and the launch counts of plan.profile() for BatchPlan.KERNELS.  What those identify:

  run_steps form                               steps_group  k_path launches  k_eval     k_finalize
  wide batched (k_paths, k_evals, k_closes)         1        ceil(K / 64)     K          K
  the same per kernel, without rows or staged       1        K                K          K
  wide per kernel, rows (k_paths, k_step's parts)   1        ceil(K / 64)     K - 1      0
  stepped, warm-started plans (k_step fused)        1        0                K - 1      0
  launch per kernel (k_path_fin: cells = 6)         0        K                K          0  (N + 7 <= 64)
  gamma-sorted wide (k_paths, k_aggs)               0        ceil(K / 64)     K          0
  gamma-sorted per kernel (k_path, k_agg)           0        K                K          0

What the API cannot tell apart, and how the cases still pin it: a k_agg run and a k_eval run that closes
its sets both count (1, 1, 0) launches — the sorted cases add a plan over an UNSORTED set, which only
k_agg reports as failed.  The template instantiation is chosen from N alone by the dispatchers' switch.
At N = 63 and 64 the host never defers a closing into k_path_fin (a record of N + 7 doubles does not fit
its one wave): the launch-per-kernel form then issues K k_finalize launches, asserted as such.
The stepped k_step launch (path + evaluation + closing fused) is the warm-started plans' form only:
plans without warm start take the wide form whatever their outputs, so k_step<N> as one launch is
reached in the repairs case (default cells), and as separate parts in the rows case's per-kernel form
(k_evals_st, the staged evaluation, is compiled into diagnostic builds only: evals_staged is False).
"""
import functools

import numpy as np
import pytest
import torch

import lompc_oracle as O
import oracle_c
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, _lib

pytestmark = pytest.mark.gpu

NS = [1, 2, 5, 12, 13, 16, 32, 63, 64]
SIZES = [0, 1, 63, 65, 1100]
SIZES_WRAP = [0, 1, 63, 65]  # K = 66: without the 1100-EV set
WRAP = [(13, 66), (16, 66)]
NK = [(n, 3) for n in NS] + WRAP
FORMS = {"rows": 1, "reductions": 2, "sorted": 3, "chain": 4, "repairs": 5, "w0": 6}
ST = _lib


def seed_of(N, form, K=0):
    return 100000 * FORMS[form] + 100 * N + (K > 64)


@functools.lru_cache(maxsize=None)
def contexts(N):
    cs = (O.small_consts(), O.large_consts())
    return cs, tuple(LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0) for c in cs)


class Batch:
    """Both EV types' ragged sets, prices for K runs and w_ref, on the host and on the device."""

    def __init__(self, N, form, K, sizes=None, layout="ragged"):
        self.N, self.K = N, K
        self.rng = rng = np.random.default_rng(seed_of(N, form, K))
        self.cs, lompcs = contexts(N)
        self.lompcs = list(lompcs)
        sizes = list(sizes if sizes is not None else (SIZES if K <= 64 else SIZES_WRAP))
        self.P = P = len(sizes)
        parts = []
        for c in self.cs:
            for m in sizes:
                if layout == "narrow":  # (a window inside [0, y_max]: EVs can move outside it)
                    g = c.y_max - (0.3 + 0.2 * rng.random(m))
                else:
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
        big = int(np.argmax(sizes))
        lm[:, 2, :N] = 0.0        # small type: the 63-EV set, no charging price (upper bound active)
        lm[:, P + big, :N] = 0.0  # large type: its largest set
        mask = np.tile(np.resize([0.0, 1.0, 0.0, 1.0, 1.0], P), 2)
        lr = 0.2 * rng.random((K, 2 * P)) * mask
        self.take(parts, lm, lr)

    def take(self, parts, lm, lr, device=True):
        """The batch from prepared data: parts, each set's gamma (P sets per context of self.cs, in their
        order: the small type's first); lm (K, S, 3N) and lr (K, S), the runs' prices, S = len(cs) P.
        w_ref is drawn from self.rng.  device = False: the host arrays only (CPU scripts)."""
        N, P = self.N, self.P
        self.gn = np.concatenate(parts)
        self.off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
        self.B = int(self.off[-1])
        self.lm, self.lr = lm, lr
        self.wr = np.concatenate([c.w_max * self.rng.random((P, N)) for c in self.cs])
        self.strides = (self.S * 3 * N, self.S)
        self._oracle = {}
        if not device:
            return
        dev = "cuda:0"
        self.g = torch.as_tensor(self.gn, device=dev)
        self.lm_d, self.lr_d = torch.as_tensor(self.lm, device=dev), torch.as_tensor(self.lr, device=dev)
        self.wr_d = torch.as_tensor(self.wr, device=dev)

    @property
    def S(self):
        """Parameter sets of the batch: P per context."""
        return len(self.cs) * self.P

    def consts_of(self, s):
        return self.cs[s // self.P]

    def oracle(self, k, gn=None):
        """(w (B, N), cost (B,)) of every EV at run k's prices (cached for the batch's own gamma)."""
        if gn is None and k in self._oracle:
            return self._oracle[k]
        g = self.gn if gn is None else gn
        W, C = np.zeros((self.B, self.N)), np.zeros(self.B)
        for s in range(self.S):
            a, b = self.off[s], self.off[s + 1]
            if b > a:
                W[a:b], C[a:b], nf = oracle_c.solve_batch(self.N, self.consts_of(s), self.lm[k, s], float(self.lr[k, s]), g[a:b])
                assert nf == 0
        if gn is None:
            self._oracle[k] = (W, C)
        return W, C

    def oracle_sets(self, k, gn=None):
        """The oracle's per-set sums at run k: (sum w (S, N), sum w0, sum price0, sum cost)."""
        W, C = self.oracle(k, gn)
        N, S = self.N, self.S
        sw, p0, sc = np.zeros((S, N)), np.zeros(S), np.zeros(S)
        for s in range(S):
            a, b = self.off[s], self.off[s + 1]
            c, lm, lr = self.consts_of(s), self.lm[k, s], self.lr[k, s]
            w0 = W[a:b, 0]
            q_scale = 3 * c.theta / (4 * c.w_max)
            p0[s] = np.sum(c.theta * (w0 * lm[0] + (c.w_max - w0) * lm[N]) + q_scale * w0 ** 2 * lm[2 * N]
                           + c.theta ** 2 * w0 ** 2 * lr)
            sw[s], sc[s] = W[a:b].sum(0), C[a:b].sum()
        return sw, sw[:, 0].copy(), p0, sc


class Dev:
    """Largest deviations of one case, each with its bar; printed before anything is asserted."""

    def __init__(self, name):
        self.name, self.rows = name, {}

    def add(self, what, err, bar):
        """err, bar: arrays (or scalars) of |deviation| and of the bar it must meet."""
        err, bar = np.broadcast_arrays(np.asarray(err, dtype=float), np.asarray(bar, dtype=float))
        if err.size == 0:
            return
        k = int(np.argmax(err / bar))
        e, r = float(err.flat[k]), float(err.flat[k] / bar.flat[k])
        if what not in self.rows or r > self.rows[what][1]:
            self.rows[what] = (e, r)

    def check(self):
        print(f"{self.name}: " + "; ".join(f"{k} {e:.3e} ({r:.3e} of its bar)" for k, (e, r) in self.rows.items()))
        for k, (e, r) in self.rows.items():
            assert r <= 1.0, (self.name, k, e, r)


def np_(t):
    return t.cpu().numpy()


def rows_vs_oracle(dev, bt, k, w, cost, gn=None):
    """Per-EV rows against the oracle: |dw| <= 1e-9, cost rtol 1e-9 + atol 1e-9."""
    W, C = bt.oracle(k, gn)
    dev.add("|dw|", np.abs(w - W), 1e-9)
    dev.add("cost", np.abs(cost - C), 1e-9 + 1e-9 * np.abs(C))


def sets_vs_oracle(dev, bt, k, sw, st, cost=True, gn=None):
    """Set reductions against the oracle's per-EV sums (rtol 1e-10, atol 1e-9; SUM_COST and SUM_PRICE0
    1e-9 relative); counts exact, nothing failed or invalid."""
    osw, ow0, op0, oc = bt.oracle_sets(k, gn)
    np.testing.assert_array_equal(st[:, ST.LOMPC_STAT_COUNT], np.diff(bt.off))
    assert np.all(st[:, ST.LOMPC_STAT_N_FAILED] == 0) and np.all(st[:, ST.LOMPC_STAT_N_INVALID] == 0)
    dev.add("set sums", np.abs(sw - osw), 1e-9 + 1e-10 * np.abs(osw))
    dev.add("sum w0", np.abs(st[:, ST.LOMPC_STAT_SUM_W0] - ow0), 1e-9 + 1e-10 * np.abs(ow0))
    dev.add("sum price0", np.abs(st[:, ST.LOMPC_STAT_SUM_PRICE0] - op0), 1e-9 * np.maximum(1.0, np.abs(op0)))
    if cost:
        dev.add("sum cost", np.abs(st[:, ST.LOMPC_STAT_SUM_COST] - oc), 1e-9 * np.maximum(1.0, np.abs(oc)))


def sets_vs_own_rows(dev, bt, w, cost, sw, st):
    """A rows form's set reductions against the sums of its own per-EV outputs (check_reductions of
    test_gpu_pipeline.py: rtol 1e-11, atol 1e-9)."""
    for s in range(bt.S):
        a, b = bt.off[s], bt.off[s + 1]
        ref = w[a:b].sum(0)
        dev.add("sums vs own rows", np.abs(sw[s] - ref), 1e-9 + 1e-11 * np.abs(ref))
        dev.add("sums vs own rows", abs(st[s, ST.LOMPC_STAT_SUM_W0] - ref[0]), 1e-9 + 1e-11 * abs(ref[0]))
        if cost is not None:
            cs_ = cost[a:b].sum()
            dev.add("sums vs own rows", abs(st[s, ST.LOMPC_STAT_SUM_COST] - cs_), 1e-9 + 1e-11 * abs(cs_))


def same_sets(a, b, staged, what):
    """test_gpu_pipeline.py's same_sets: bitwise, or through k_evals_st (seven row waves) to 1e-12."""
    if not staged:
        assert torch.equal(a, b), what
        return
    an, bn = np_(a), np_(b)
    np.testing.assert_allclose(an, bn, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(bn).max())), err_msg=str(what))


def counted(plan, call):
    """Launch counts (k_path, k_eval, k_finalize) of the plan's kernels over ``call()``."""
    plan.profile(enable=BatchPlan.KERNELS)
    for k in BatchPlan.KERNELS:
        plan.profile(read=True, reset=True, kernel=k)
    res = call()
    plan.last_check = plan.check()
    n = tuple(plan.profile(read=True, reset=True, kernel=k)[1] for k in BatchPlan.KERNELS)
    plan.profile(enable=False)
    return res, n


def groups(K):
    return (K + 63) // 64


def clone(out):
    return {n: v.clone() for n, v in out.items() if v is not None and n[0] != "_"}


@pytest.mark.parametrize("N,K", NK)
def test_run_steps_rows_every_run_vs_oracle(gpu, N, K):
    """(a) run_steps with rows (want_w): per_run = True keeps every run's w, cost, status and set
    reductions — each compared with the oracle over every EV and, bitwise, with an independent single
    run (sets through k_evals_st to 1e-12, as test_run_steps_matches_single_runs); the per-kernel form
    and the shared-output form give the same bits.  Default cells: the wide form (k_paths / k_evals /
    k_closes; its per-kernel form runs k_step's evaluation and closing parts, one launch each); cells = 6:
    launch per kernel, the closings inside the next run's k_path_fin."""
    bt = Batch(N, "rows", K)
    dev = Dev(f"rows N={N} K={K}")
    for cells in (None, 6):
        kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_w=True, want_cost=True, want_status=True, cells=cells)
        ref = BatchPlan(bt.lompcs, bt.g, bt.off, **kw)
        assert ref.launches_per_run() == 3
        runs = [clone(ref.run(bt.lm_d[k], bt.lr_d[k])) for k in range(K)]
        assert ref.check()[1:] == (0, 0)
        for split in (False, True):
            pr = BatchPlan(bt.lompcs, bt.g, bt.off, **kw)
            o, n = counted(pr, lambda: pr.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True, per_kernel=split))
            info = pr.info()
            if cells is None:
                assert pr.cells % 4 == 0 and info["steps_group"] == 1
                if not split:
                    assert n == (groups(K), K, K), n  # k_paths per group, k_evals and k_closes as K runs
                elif info["evals_staged"]:            # (diagnostic builds: k_evals_st, groups of one run)
                    assert n == (K, K, K), n
                else:
                    assert n == (groups(K), K - 1, 0), n  # k_paths, then k_step's parts (steady launches timed)
            else:
                assert pr.cells == 6 and info["steps_group"] == 0
                assert n == (K, K, 0 if N + 7 <= 64 else K), n  # the closings inside k_path_fin (the last: untimed)
            for k in range(K):
                for key in ("w", "cost", "status"):
                    assert torch.equal(o[key][k], runs[k][key]), (cells, split, k, key)
                for key in ("set_sum_w", "set_stats"):
                    same_sets(o[key][k], runs[k][key], info["evals_staged"], (cells, split, k, key))
            if split:
                continue
            w, cost, sw, st = np_(o["w"]), np_(o["cost"]), np_(o["set_sum_w"]), np_(o["set_stats"])
            status = np_(o["status"])
            assert np.all((status == ST.LOMPC_QP_OK) | (status == ST.LOMPC_QP_REPAIRED))
            for k in range(K):
                rows_vs_oracle(dev, bt, k, w[k], cost[k])
                sets_vs_oracle(dev, bt, k, sw[k], st[k])
                sets_vs_own_rows(dev, bt, w[k], cost[k], sw[k], st[k])
        # shared outputs: every run writes the plan's rows, the last run's remain
        sh = BatchPlan(bt.lompcs, bt.g, bt.off, **kw)
        osh = sh.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)
        assert sh.check()[1:] == (0, 0)
        for key in ("w", "cost", "status"):
            assert torch.equal(osh[key], runs[-1][key]), (cells, key)
        for k in range(K):
            for key in ("set_sum_w", "set_stats"):
                same_sets(osh[key][k], runs[k][key], sh.info()["evals_staged"], (cells, "shared", k, key))
    dev.check()


@pytest.mark.parametrize("N,K", NK)
def test_run_steps_reductions_piece_sums_vs_oracle(gpu, N, K):
    """(b) reductions-only run_steps (want_w = False, per_run_sets): the wide form's evaluation sums each
    certified piece from its count and fixed-point gamma sum.  Every run's sums against the oracle's
    per-EV sums and the rows form (1e-11, as test_run_steps_piece_sums_match_oracle); MAX_ERR and COUNT
    equal the rows form's."""
    bt = Batch(N, "reductions", K)
    dev = Dev(f"reductions N={N} K={K}")
    kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_cost=False)
    red = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=False, **kw)
    rows = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=True, **kw)
    o, n = counted(red, lambda: red.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True))
    assert red.cells % 4 == 0 and red.info()["steps_group"] == 1 and n == (groups(K), K, K), n  # the wide batched form
    orow = rows.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)
    assert rows.check()[1:] == (0, 0)
    sw, st = np_(o["set_sum_w"]), np_(o["set_stats"])
    swr, stw = np_(orow["set_sum_w"]), np_(orow["set_stats"])
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k], cost=False)
        sets_vs_oracle(dev, bt, k, swr[k], stw[k], cost=False)
    dev.add("vs rows form", np.abs(sw - swr), 1e-11 + 1e-11 * np.abs(swr))
    dev.check()
    for s in np.flatnonzero(np.diff(bt.off) == 0):
        assert np.all(sw[:, s] == 0.0)
    np.testing.assert_array_equal(st[:, :, ST.LOMPC_STAT_MAX_ERR], stw[:, :, ST.LOMPC_STAT_MAX_ERR])
    np.testing.assert_array_equal(st[:, :, ST.LOMPC_STAT_COUNT], stw[:, :, ST.LOMPC_STAT_COUNT])


@pytest.mark.parametrize("N,K", NK)
def test_sorted_gamma_aggregation_vs_oracle(gpu, N, K):
    """(c) gamma-sorted sets without per-EV output: a single run (k_agg), wide run_steps (k_paths +
    k_aggs) against its per-kernel form and single runs (bitwise, as test_run_steps_sorted_wide), a
    sort_sets plan over the unsorted batch (bitwise the sorted plan's), and diag_repair (every EV through
    k_agg's individual re-solve) on the sets of at most 65 EVs — each against the full per-EV plan
    (1e-11, atol 1e-9, as test_sorted_gamma_aggregation) and the oracle.  A sorted plan over an unsorted
    set reports the set's EVs failed: only k_agg reads the order."""
    bt = Batch(N, "sorted", K, layout="sorted")
    dev = Dev(f"sorted N={N} K={K}")
    P = bt.P
    kw = dict(sets_per_ctx=[P, P], w_ref=bt.wr_d)
    red = dict(want_w=False, want_cost=False)
    agg = BatchPlan(bt.lompcs, bt.g, bt.off, sorted_gamma=True, **red, **kw)
    full = BatchPlan(bt.lompcs, bt.g, bt.off, want_w=True, want_cost=True, **kw)
    assert agg.launches_per_run() == 2
    oa, n = counted(agg, lambda: clone(agg.run(bt.lm_d[0], bt.lr_d[0])))
    assert n == (1, 1, 0), n
    of = full.run(bt.lm_d[0], bt.lr_d[0])
    assert full.check()[1:] == (0, 0)
    sa, sf = np_(oa["set_stats"]), np_(of["set_stats"])
    dev.add("vs per-EV plan", np.abs(np_(oa["set_sum_w"]) - np_(of["set_sum_w"])), 1e-9 + 1e-11 * np.abs(np_(of["set_sum_w"])))
    dev.add("vs per-EV plan", np.abs(sa - sf), 1e-9 + 1e-11 * np.abs(sf))
    sets_vs_oracle(dev, bt, 0, np_(oa["set_sum_w"]), sa)
    rows_vs_oracle(dev, bt, 0, np_(of["w"]), np_(of["cost"]))
    # wide run_steps: k_paths + k_aggs per group of runs; per kernel: k_path + k_agg per run
    ow, n = counted(agg, lambda: clone(agg.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True)))
    assert agg.info()["steps_group"] == 0 and n == (groups(K), K, 0), n
    osq, n = counted(agg, lambda: agg.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True, per_kernel=True))
    assert n == (K, K, 0), n
    for key in ("set_sum_w", "set_stats"):
        assert torch.equal(ow[key], osq[key]), key
    for k in sorted({0, 1, K - 3, K - 2, K - 1}):
        o1 = agg.run(bt.lm_d[k], bt.lr_d[k])
        assert torch.equal(o1["set_sum_w"], ow["set_sum_w"][k]) and torch.equal(o1["set_stats"], ow["set_stats"][k]), k
    assert agg.check()[1:] == (0, 0)
    sw, st = np_(ow["set_sum_w"]), np_(ow["set_stats"])
    for k in range(K):
        sets_vs_oracle(dev, bt, k, sw[k], st[k])
    # sort_sets over the unsorted batch: the sorted plan's bits
    shuf = np.concatenate([bt.rng.permutation(bt.gn[a:b]) for a, b in zip(bt.off[:-1], bt.off[1:])])
    srt = BatchPlan(bt.lompcs, torch.as_tensor(shuf, device="cuda:0"), bt.off, sort_sets=True, **red, **kw)
    os_, n = counted(srt, lambda: srt.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run_sets=True))
    assert n == (groups(K), K, 0), n
    for key in ("set_sum_w", "set_stats"):
        assert torch.equal(os_[key], ow[key]), key
    # an unsorted set (two EVs of the 63-EV set swapped): k_agg reports its EVs failed
    g3 = bt.gn.copy()
    a = bt.off[2]
    g3[a + 10], g3[a + 40] = g3[a + 40], g3[a + 10]
    uns = BatchPlan(bt.lompcs, torch.as_tensor(g3, device="cuda:0"), bt.off, sorted_gamma=True, **red, **kw)
    ou = uns.run(bt.lm_d[0], bt.lr_d[0])
    with pytest.raises(Exception):
        uns.check()
    assert np_(ou["set_stats"])[2, ST.LOMPC_STAT_N_FAILED] == 63
    # diag_repair: no certified pieces, every EV re-solved inside k_agg (sets of at most 65 EVs)
    if K <= 64:
        small = Batch(N, "sorted", K, sizes=SIZES_WRAP, layout="sorted")
        kws = dict(sets_per_ctx=[small.P, small.P], w_ref=small.wr_d, diag_repair=True)
        da = BatchPlan(small.lompcs, small.g, small.off, sorted_gamma=True, **red, **kws)
        df = BatchPlan(small.lompcs, small.g, small.off, want_w=True, want_cost=True, **kws)
        oda, n = counted(da, lambda: clone(da.run(small.lm_d[0], small.lr_d[0])))
        assert n == (1, 1, 0), n
        odf = df.run(small.lm_d[0], small.lr_d[0])
        assert da.last_check == (small.B, 0, 0) and df.check() == (small.B, 0, 0)
        sda, sdf = np_(oda["set_stats"]), np_(odf["set_stats"])
        np.testing.assert_array_equal(sda[:, ST.LOMPC_STAT_N_REPAIRED], np.diff(small.off))
        dev.add("diag vs per-EV plan", np.abs(sda - sdf), 1e-9 + 1e-11 * np.abs(sdf))
        dev.add("diag vs per-EV plan", np.abs(np_(oda["set_sum_w"]) - np_(odf["set_sum_w"])),
                1e-9 + 1e-11 * np.abs(np_(odf["set_sum_w"])))
        sets_vs_oracle(dev, small, 0, np_(oda["set_sum_w"]), sda)
        rows_vs_oracle(dev, small, 0, np_(odf["w"]), np_(odf["cost"]))
    dev.check()


def phi(c, w):
    q_s = 3 * c.theta / (4 * c.w_max)
    return np.concatenate([c.theta * w, c.theta * (c.w_max - w), q_s * w * w], axis=-1)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("want_w", [True, False])
def test_run_chain_rule_and_oracle(gpu, want_w, N):
    """(d) run_chain, K = 4 dependent runs (k_chain_price between them): the prices follow the rule
    restated on the host from the previous run's reductions (non-empty sets; an empty set's count is 0),
    every run equals an independent wide run_steps at the recorded prices as in test_gpu_chain.py, and
    the first and last run's sums match the oracle."""
    K, step = 4, 0.5
    bt = Batch(N, "chain", 1)
    dev = Dev(f"chain N={N} want_w={want_w}")
    P = bt.P
    wt = np.concatenate([c.w_max * (0.2 + 0.6 * bt.rng.random((P, N))) for c in bt.cs])
    lr = bt.lr_d[0]
    kw = dict(sets_per_ctx=[P, P], want_w=want_w, want_cost=True, close_in_finalize=True)
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, w_ref=torch.as_tensor(wt, device="cuda:0"), **kw)
    assert plan.launches_per_run() == 3
    out, n = counted(plan, lambda: plan.run_chain(bt.lm[0], lr, wt, step, K))
    assert n == (K, K, K), n  # k_path, k_eval, k_finalize per run
    lm = np_(out["lmbd"])
    sw, st = np_(out["set_sum_w"]), np_(out["set_stats"])
    np.testing.assert_array_equal(lm[0], bt.lm[0])
    nonempty = np.flatnonzero(np.diff(bt.off) > 0)
    for k in range(1, K):
        for s in nonempty:
            c = bt.consts_of(s)
            wb = sw[k - 1, s] / st[k - 1, s, ST.LOMPC_STAT_COUNT]
            exp = np.maximum(0.0, lm[k - 1, s] + step * (phi(c, wb) - phi(c, wt[s])))
            np.testing.assert_allclose(lm[k, s], exp, rtol=1e-14, atol=1e-14 * c.theta)
        for s in np.flatnonzero(np.diff(bt.off) == 0):
            np.testing.assert_array_equal(lm[k, s], lm[k - 1, s])  # (an empty set keeps its prices)
        assert not np.array_equal(lm[k][nonempty], lm[k - 1][nonempty])  # the prices move
    ref = BatchPlan(bt.lompcs, bt.g, bt.off, w_ref=torch.as_tensor(wt, device="cuda:0"), **kw)
    o = ref.run_steps(out["lmbd"], lr, K, 2 * P * 3 * N, 0, per_run_sets=True)
    assert ref.check()[1:] == (0, 0)
    staged = ref.info()["evals_staged"]
    for k in range(K):
        for key in ("set_sum_w", "set_stats"):
            a_, b_ = np_(o[key][k]), np_(out[key][k])
            if not want_w:  # (piece aggregates, unclamped, vs the single runs' row sums: their documented bar)
                np.testing.assert_allclose(a_, b_, rtol=1e-10, atol=1e-9)
            elif staged:
                np.testing.assert_allclose(a_, b_, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(b_).max())))
            else:
                assert torch.equal(o[key][k], out[key][k]), (k, key)
    for key in ("w", "cost"):
        if o.get(key) is not None:
            assert torch.equal(o[key], out[key]), key
    for k in (0, K - 1):  # the oracle at the recorded prices
        at = Batch.__new__(Batch)
        at.__dict__.update(bt.__dict__)
        at.lm, at.lr, at._oracle = lm[k][None], bt.lr[:1], {}
        sets_vs_oracle(dev, at, 0, sw[k], st[k])
        if k == K - 1:
            if want_w:
                rows_vs_oracle(dev, at, 0, np_(out["w"]), np_(out["cost"]))
            else:
                _, C = at.oracle(0)
                dev.add("cost", np.abs(np_(out["cost"]) - C), 1e-9 + 1e-9 * np.abs(C))
    dev.check()


@pytest.mark.parametrize("N", NS)
def test_run_steps_repairs_vs_oracle(gpu, N):
    """(e) a warm-started plan whose EVs moved outside their set's gamma window after its creation (a
    tenth of them, to the box bounds' neighbourhood): run_steps over K = 3 runs equals three single runs
    bit for bit and the oracle over every EV, as test_run_steps_repairs_match_single_runs.  Default
    cells: the stepped form, one fused k_step launch per step (path + evaluation + closing, the
    re-solves from the edge cells' working sets); cells = 6: launch per kernel, run k's closing and
    re-solves inside run k + 1's k_path_fin (N + 7 <= 64; else K k_finalize launches)."""
    K = 3
    bt = Batch(N, "repairs", K, layout="narrow")
    dev = Dev(f"repairs N={N}")
    rng = bt.rng
    moved = rng.choice(bt.B, bt.B // 10, replace=False)
    ymax = np.repeat([c.y_max for c in bt.cs], [bt.off[bt.P], bt.B - bt.off[bt.P]])
    gm = bt.gn.copy()
    gm[moved] = np.where(rng.random(moved.size) < 0.5, 0.02 * rng.random(moved.size), 1.0 - 0.02 * rng.random(moved.size)) * ymax[moved]
    gm[moved[:2]] = [0.0, ymax[moved[1]]]  # and the bounds themselves
    for cells in (None, 6):
        g = bt.g.clone()
        kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_w=True, want_cost=True, want_status=True, warm_start=True,
                  cells=cells)
        ref = BatchPlan(bt.lompcs, g, bt.off, **kw)
        plan = BatchPlan(bt.lompcs, g, bt.off, **kw)
        g.copy_(torch.as_tensor(gm))
        outs = [clone(ref.run(bt.lm_d[k], bt.lr_d[k])) for k in range(K)]
        rep, fail, inv = ref.check()
        assert rep >= K * (moved.size - 2) and fail == 0 and inv == 0
        out, n = counted(plan, lambda: plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides))
        info = plan.info()
        if cells is None:
            assert plan.cells % 4 == 0 and info["steps_group"] == 1 and not info["evals_staged"]
            assert n == (0, K - 1, 0), n  # no k_path / k_finalize launch: k_step carries all three parts
        else:
            assert plan.cells == 6 and info["steps_group"] == 0
            assert n == (K, K, 0 if N + 7 <= 64 else K), n
        assert plan.last_check == (rep, 0, 0)
        for key in ("w", "cost", "status", "set_sum_w", "set_stats"):
            assert torch.equal(out[key], outs[-1][key]), (cells, key)
        status = np_(out["status"])
        assert np.all(status[moved] == ST.LOMPC_QP_REPAIRED) and np.all(status != ST.LOMPC_QP_FAILED)
        w, cost, sw, st = np_(out["w"]), np_(out["cost"]), np_(out["set_sum_w"]), np_(out["set_stats"])
        rows_vs_oracle(dev, bt, K - 1, w, cost, gn=gm)
        sets_vs_oracle(dev, bt, K - 1, sw, st, gn=gm)
        sets_vs_own_rows(dev, bt, w, cost, sw, st)
    dev.check()


def station_batch(rng, cs, sizes):
    """Both types' partitions as the station lays them out: each set a band of charge levels, sorted
    descending in level (ascending gamma)."""
    parts, P = [], len(sizes)
    for c in cs:
        edges = np.linspace(0.3, c.y_max, P + 1)
        for p, m in enumerate(sizes):
            y = np.sort(edges[p] + (edges[p + 1] - edges[p]) * rng.random(m))[::-1]
            parts.append(c.y_max - y)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)


@pytest.mark.parametrize("N", NS)
def test_w0_contract_vs_oracle(gpu, N):
    """(f) the station's w0 pass (charging_station.py, _w0_both): a plan with want_w = False, want_cost =
    False, want_w0 = True, want_set = True over both types' partitions (each sorted descending in level),
    no w_ref, re-targeted by plan.update at a batch of another size.  Before and after the update: w0
    against the oracle's w[:, 0] at 1e-9, SUM_W0 / SUM_PRICE0 / COUNT against the oracle; each type's
    sets through LoMPC.solve_batch(want_w0 = True) (the context's transient plan) bit for bit.  Close
    modes: the default and close_in_eval (sets closed inside k_eval: 2 launches, no k_finalize) and
    close_in_finalize (3 launches); per-EV w0 bitwise equal between them, the set reductions to 1e-12 (the
    summation order, as test_close_in_eval_matches_k_finalize)."""
    bt = Batch(N, "w0", 1)
    dev = Dev(f"w0 N={N}")
    P, rng = bt.P, bt.rng
    batches = [station_batch(rng, bt.cs, [0, 1, 63, 65, 1100]), station_batch(rng, bt.cs, [70, 2, 0, 1200, 130])]
    lm, lr = bt.lm_d[0], bt.lr_d[0]
    res = {}
    for mode, kw, launches in (("default", {}, 2), ("close_in_eval", dict(close_in_eval=True), 2),
                               ("close_in_finalize", dict(close_in_finalize=True), 3)):
        plan = None
        for i, (gn, off) in enumerate(batches):
            g = torch.as_tensor(gn, device="cuda:0")
            if plan is None:
                plan = BatchPlan(bt.lompcs, g, off, sets_per_ctx=[P, P], want_w=False, want_cost=False, want_w0=True,
                                 want_set=True, validate=False, **kw)
            else:
                plan.update(g, off, validate=False)
            assert plan.launches_per_run() == launches
            out, n = counted(plan, lambda: clone(plan.run(lm, lr)))
            assert n == (1, 1, launches - 2), (mode, n)
            assert "w" not in out and "cost" not in out
            res[mode, i] = out
            at = Batch.__new__(Batch)
            at.__dict__.update(bt.__dict__)
            at.gn, at.off, at.B, at._oracle = gn, off, int(off[-1]), {}
            W, _ = at.oracle(0)
            w0 = np_(out["w0"])
            assert w0.shape == (at.B,)
            dev.add("|dw0|", np.abs(w0 - W[:, 0]), 1e-9)
            sets_vs_oracle(dev, at, 0, np_(out["set_sum_w"]), np_(out["set_stats"]), cost=False)
            if mode != "default":
                assert torch.equal(out["w0"], res["default", i]["w0"]), (mode, i)
                for key in ("set_sum_w", "set_stats"):
                    np.testing.assert_allclose(np_(out[key]), np_(res["default", i][key]), rtol=1e-12, atol=1e-12, err_msg=key)
    # each type's sets through the context's own solve_batch, as charging_station.py's _w0_batched
    for i, (gn, off) in enumerate(batches):
        for t, lo in enumerate(bt.lompcs):
            a, b = int(off[t * P]), int(off[(t + 1) * P])
            lo.set_params(lm[t * P:(t + 1) * P], lr[t * P:(t + 1) * P])
            r = lo.solve_batch(torch.as_tensor(gn[a:b], device="cuda:0"), off[t * P:(t + 1) * P + 1] - a, want_w=False,
                               want_cost=False, want_w0=True, want_set=True, check=False)
            assert lo.check_last()[1:] == (0, 0)
            assert "w" not in r and "cost" not in r
            ref = res["default", i]
            assert torch.equal(r["w0"], ref["w0"][a:b]), (i, t)
            assert torch.equal(r["set_sum_w"], ref["set_sum_w"][t * P:(t + 1) * P]), (i, t)
            assert torch.equal(r["set_stats"], ref["set_stats"][t * P:(t + 1) * P]), (i, t)
    dev.check()
