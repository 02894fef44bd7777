"""The wide form's fused launch (k_evals_tail): group g + 1's paths behind group g's evaluations.

run_steps with more than one group of runs (K > 64) issues k_paths for group 0 only; every later group's paths
ride in the launch that evaluates the group before it, into the other half of a table ring that holds two
groups.  The runs are independent, so every output must be the split form's (run_steps(per_kernel=True): one
part per launch, no overlap) bit for bit, whatever order the path and evaluation workgroups were dispatched in.

Populations (small on purpose: the schedule, not the evaluation, is under test): five sets in one plan, both EV
types, of 0, 65 and 300 EVs (small type) and 1 and 301 EVs (large type); gamma uniform over [0, y_max] with 0
and y_max exactly in every set of two or more EVs; 4 and 8 cells per set; horizons 24, 48 and 13 (the generic
instantiation).  K crosses every group boundary: 1, 2, 64 (one group: no fused launch), 65, 100, 128 (two
groups), 129, 130 (three).

Per (horizon, cells) ONE split-form reference of K_MAX = 130 runs with every output per run, and one oracle
solve of the runs checked (0, 1, 63, 64, 65, 99, 127, 128, 129) over every EV, shared by all K (run k's
prices do not depend on K).  Tolerances against the oracle: tests/test_gpu_pipeline.py's for the wide form
(|dw| <= 1e-9, cost 1e-9 relative and absolute; set sums rtol 1e-10, atol 1e-9).

Which schedule ran is read from plan.info(): tail_launches (fused launches so far) and ring_runs (the runs the
table ring may hold: the fused launch needs twice the group's 64).  The profile's launch counts are those of
the schedule without the fused launch (a fused launch counts as its group's path launch), so they cannot tell.
"""
import functools

import numpy as np
import pytest
import torch

import lompc_oracle as O
import oracle_c
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, _lib

from test_gpu_comm import nccl1  # noqa: F401  (the world-1 communicator: a module-scoped fixture)

pytestmark = pytest.mark.gpu

HORIZONS = [24, 48, 13]
CELLS = [4, 8]
KS = [1, 2, 64, 65, 100, 128, 129, 130]
K_MAX = max(KS)
GROUP = 64
SIZES = ([0, 65, 300], [1, 301])  # small type's sets, large type's
ORACLE_RUNS = sorted({0, 63, 64, 65} | {K - 1 for K in KS})
PER_EV = ("w", "cost", "status")
SETS = ("set_sum_w", "set_stats")


def fused_launches(K, group=GROUP):
    """Groups after the first: each one's paths ride in the launch before it."""
    return (K + group - 1) // group - 1


def same_bits(a, b):
    """Tensors equal bit for bit (NaN patterns included)."""
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


class Pop:
    """One (horizon, cells) population on the device: contexts, gamma, K_MAX runs' prices."""

    def __init__(self, N, cells, sizes=SIZES):
        self.N, self.cells = N, cells
        rng = np.random.default_rng([11, N, cells])
        self.cs = (O.small_consts(), O.large_consts())
        self.lompcs = [LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0) for c in self.cs]
        gs, lms, lrs = [], [], []
        for c, ms in zip(self.cs, sizes):
            for m in ms:
                g = c.y_max * rng.random(m)
                if m >= 2:
                    g[m // 3], g[m - 1] = 0.0, c.y_max
                gs.append(g)
            lms.append(c.theta * rng.random((K_MAX, len(ms), 3 * N)))
            lrs.append(0.2 * rng.random((K_MAX, len(ms))) * (np.arange(len(ms)) % 2))
        self.P = [len(ms) for ms in sizes]
        self.S = sum(self.P)
        self.gn = np.concatenate(gs)
        self.off = np.concatenate([[0], np.cumsum([len(g) for g in gs])]).astype(np.int64)
        self.B = int(self.off[-1])
        self.lmn, self.lrn = np.concatenate(lms, axis=1), np.concatenate(lrs, axis=1)
        self.g = torch.as_tensor(self.gn, device="cuda:0")
        self.lm = torch.as_tensor(self.lmn, device="cuda:0")
        self.lr = torch.as_tensor(self.lrn, device="cuda:0")
        self.strides = (self.S * 3 * N, self.S)

    def plan(self, rows=True, **kw):
        want = dict(want_w=True, want_cost=True, want_status=True) if rows else dict(want_w=False, want_cost=False)
        p = BatchPlan(self.lompcs, self.g, self.off, sets_per_ctx=self.P, cells=self.cells, **want, **kw)
        assert p.cells == self.cells
        return p

    def steps(self, plan, K, **kw):
        """run_steps of the first K runs; the plan's tallies must show no failed and no invalid QP."""
        out = plan.run_steps(self.lm, self.lr, K, *self.strides, **kw)
        assert plan.check()[1:] == (0, 0)
        return out


@functools.lru_cache(maxsize=None)
def pop(N, cells):
    return Pop(N, cells)


@functools.lru_cache(maxsize=None)
def split_rows(N, cells):
    """The split form's K_MAX runs, every output per run (the shared reference; left unchanged)."""
    pp = pop(N, cells)
    p = pp.plan()
    o = pp.steps(p, K_MAX, per_run=True, per_kernel=True)
    assert p.info()["tail_launches"] == 0
    return {k: o[k] for k in PER_EV + SETS}


@functools.lru_cache(maxsize=None)
def split_sums(N, cells):
    """The split form without w output (piece sums), K_MAX runs' set reductions."""
    pp = pop(N, cells)
    p = pp.plan(rows=False)
    o = pp.steps(p, K_MAX, per_run_sets=True, per_kernel=True)
    assert p.info()["tail_launches"] == 0
    return {k: o[k] for k in SETS}


@functools.lru_cache(maxsize=None)
def oracle_runs(N, cells):
    """{run: (w (B, N), cost (B,))} of the C oracle over every EV, for the runs in ORACLE_RUNS."""
    pp = pop(N, cells)
    res = {}
    for k in ORACLE_RUNS:
        w, cost = np.zeros((pp.B, N)), np.zeros(pp.B)
        for s in range(pp.S):
            a, b = pp.off[s], pp.off[s + 1]
            if b > a:
                wo, co, nf = oracle_c.solve_batch(N, pp.cs[0 if s < pp.P[0] else 1], pp.lmn[k, s], float(pp.lrn[k, s]),
                                                  pp.gn[a:b])
                assert nf == 0
                w[a:b], cost[a:b] = wo, co
        res[k] = (w, cost)
    return res


def check_schedule(plan, K):
    info = plan.info()
    assert info["ring_runs"] >= 2 * GROUP, info  # (these plans are small: the ring holds two groups)
    assert info["tail_launches"] == fused_launches(K), (K, info)
    assert not info["evals_staged"]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_equals_split_and_oracle(gpu, N, cells, K):
    pp, ref = pop(N, cells), split_rows(N, cells)
    # every output per run (out=: w [K][B][N], cost [K][B], ...): every run's bits are the split form's
    p = pp.plan()
    out = {"w": torch.empty((K, pp.B, N), dtype=torch.float64, device="cuda:0"),
           "cost": torch.empty((K, pp.B), dtype=torch.float64, device="cuda:0")}
    o = pp.steps(p, K, per_run=True, out=out)
    assert o["w"] is out["w"] and o["cost"] is out["cost"]
    check_schedule(p, K)
    for key in PER_EV + SETS:
        assert same_bits(o[key], ref[key][:K]), (key, "per run")
    # the shared buffers: the last run's rows remain; every run's set reductions kept
    q = pp.plan()
    os_ = pp.steps(q, K, per_run_sets=True)
    check_schedule(q, K)
    for key in PER_EV:
        assert same_bits(os_[key], ref[key][K - 1]), (key, "shared")
    for key in SETS:
        assert same_bits(os_[key], ref[key][:K]), (key, "shared")
    # a second call on the same plan (its ring and records in place) fuses again and gives the same bits
    o2 = pp.steps(p, K, per_run=True, out=out)
    assert p.info()["tail_launches"] == 2 * fused_launches(K)
    for key in PER_EV + SETS:
        assert same_bits(o2[key], ref[key][:K]), (key, "second call")
    # the oracle, over every EV of the runs at the group boundaries and the last run
    orc = oracle_runs(N, cells)
    wn, cn, sw = o["w"].cpu().numpy(), o["cost"].cpu().numpy(), o["set_sum_w"].cpu().numpy()
    st = o["set_stats"].cpu().numpy()
    for k in sorted({0, 63, 64, 65, K - 1}):
        if k >= K:
            continue
        wo, co = orc[k]
        print(f"N {N} cells {cells} K {K} run {k}: max |dw| {np.abs(wn[k] - wo).max():.3e}, "
              f"max |dcost| / max(1, |cost|) {(np.abs(cn[k] - co) / np.maximum(1.0, np.abs(co))).max():.3e}")
        np.testing.assert_allclose(wn[k], wo, rtol=0, atol=1e-9)
        np.testing.assert_allclose(cn[k], co, rtol=1e-9, atol=1e-9)
        for s in range(pp.S):
            a, b = pp.off[s], pp.off[s + 1]
            np.testing.assert_allclose(sw[k, s], wo[a:b].sum(0), rtol=1e-10, atol=1e-9)
            assert abs(st[k, s, _lib.LOMPC_STAT_SUM_COST] - co[a:b].sum()) <= 1e-9 * max(1.0, abs(co[a:b].sum()))
            assert st[k, s, _lib.LOMPC_STAT_COUNT] == b - a
            assert st[k, s, _lib.LOMPC_STAT_N_FAILED] == 0 and st[k, s, _lib.LOMPC_STAT_N_INVALID] == 0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_piece_sums_equal_split(gpu, N, cells, K):
    """Runs without w output (their evaluation sums the certified pieces): the split form's bits, and the
    oracle's per-EV sums at test_run_steps_piece_sums_match_oracle's bar (rtol 1e-10, atol 1e-9)."""
    pp, ref = pop(N, cells), split_sums(N, cells)
    p = pp.plan(rows=False)
    o = pp.steps(p, K, per_run_sets=True)
    check_schedule(p, K)
    for key in SETS:
        assert same_bits(o[key], ref[key][:K]), key
    orc = oracle_runs(N, cells)
    sw = o["set_sum_w"].cpu().numpy()
    for k in sorted({0, 63, 64, 65, K - 1}):
        if k >= K:
            continue
        wo, _ = orc[k]
        for s in range(pp.S):
            a, b = pp.off[s], pp.off[s + 1]
            np.testing.assert_allclose(sw[k, s], wo[a:b].sum(0), rtol=1e-10, atol=1e-9, err_msg=f"run {k} set {s}")


@pytest.mark.parametrize("K", [65, 130])
def test_fused_with_world1_communicator(nccl1, K):  # noqa: F811
    """With a communicator each group's closings are followed by its all-gather and combine; the fused
    launches stay.  World 1: the combine of one record is a copy, so the outputs are the plain plan's bits."""
    from lompc_amd.dist import device_comm

    N, cells = 24, 4
    pp, ref = pop(N, cells), split_rows(N, cells)
    shard = pp.plan()
    shard.set_comm(device_comm(nccl1, 0))
    o = pp.steps(shard, K, per_run=True)
    check_schedule(shard, K)
    for key in PER_EV + SETS:
        assert same_bits(o[key], ref[key][:K]), key
    shard.set_comm(None)


def test_fallback_when_the_ring_cannot_hold_two_groups(gpu):
    """A plan of many cells: the ring's memory bound (1 GiB over S x G cells of 8 pieces each, some 16 N + 72
    bytes per piece) leaves fewer than 2 x 64 runs, so run_steps keeps a k_paths launch before every group's
    k_evals — no fused launch — and gives the split form's bits.  N = 48, five sets of 256 cells: 1280 cells of
    6796 bytes, 123 runs.  Few EVs: the cells, not the batch, make the plan big."""
    N, cells, K = 48, 256, 65
    pp = Pop(N, cells, sizes=([0, 65], [1, 300, 7]))
    p = pp.plan()
    assert GROUP + 1 <= p.info()["ring_runs"] < 2 * GROUP, p.info()
    o = pp.steps(p, K, per_run=True)
    info = p.info()
    assert info["tail_launches"] == 0 and info["steps_group"] == 1, info
    q = pp.plan()
    ref = pp.steps(q, K, per_run=True, per_kernel=True)
    for key in PER_EV + SETS:
        assert same_bits(o[key], ref[key]), key
    # ... and the launch counts are the three-launches-per-group schedule's
    r = pp.plan()
    r.profile(enable=BatchPlan.KERNELS)
    for k in BatchPlan.KERNELS:
        r.profile(read=True, reset=True, kernel=k)
    pp.steps(r, K, per_run_sets=True)
    n = tuple(r.profile(read=True, reset=True, kernel=k)[1] for k in BatchPlan.KERNELS)
    r.profile(enable=False)
    assert n == (2, K, K), n
    assert r.info()["tail_launches"] == 0
