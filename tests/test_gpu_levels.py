"""GPU tests of the station's partition layout (lompc_levels_layout, ChargingStation._sorted_layouts):
one descending sort per EV type gives the statistics the reference's index masks define
(charging_station.py:111-116 with price_solver.py:66-77) and each partition's EVs as one run in
descending charge level; levels exactly on boundaries, ties and an out-of-range level included."""
import ctypes
import math

import numpy as np
import pytest
import torch

from guarded import Guarded
from lompc_amd import _lib
from lompc_amd.charging_station import ChargingStation, partition_stats

pytestmark = pytest.mark.gpu


def _ref_indices(y, rng, idx0):
    idx = idx0.copy()
    for p in range(len(rng) - 1):
        idx[(y >= rng[p]) & (y <= rng[p + 1])] = p
    return idx


@pytest.mark.parametrize("case", range(5))
def test_sorted_layouts_match_index_partitions(gpu, case):
    rs = np.random.default_rng(80 + case)
    P = 12 if case != 4 else 1
    rng_s, rng_l = np.linspace(0.3, 0.9, P + 1), np.linspace(0.3, 0.85, P + 1)
    n_s, n_l = (5000, 4000) if case != 2 else (300000, 1)
    y_s = 0.3 + 0.2 * rs.random(n_s)
    y_l = 0.3 + 0.55 * rs.random(n_l)
    y_s[:20] = rng_s[rs.integers(0, P + 1, 20)]  # levels exactly on the boundaries
    if n_l > 4:
        y_l[:3] = y_l[3]  # ties
    if case == 3:
        y_l[min(7, n_l - 1)] = 0.2  # below rng[0]: the large type takes the index path
    cs = object.__new__(ChargingStation)
    cs.P, cs.group, cs.device = P, None, 0
    cs.replicated, cs._exchange = False, False
    cs.y_s, cs.y_l = torch.as_tensor(y_s, device="cuda:0"), torch.as_tensor(y_l, device="cuda:0")
    cs.y0_s_rng, cs.y0_l_rng = rng_s, rng_l
    cs.idx_s = torch.zeros(n_s, dtype=torch.int64, device="cuda:0")
    cs.idx_l = torch.zeros(n_l, dtype=torch.int64, device="cuda:0")
    cs._bounds, cs._lv = {}, {}
    ChargingStation._update_indices(cs)  # (resets cs._layout)
    out = ChargingStation._sorted_layouts(cs)
    assert set(out) == ({"Small"} if case == 3 else {"Small", "Large"})
    for kind, y, idx, rng in (("Small", y_s, cs.idx_s, rng_s), ("Large", y_l, cs.idx_l, rng_l)):
        if kind not in out:
            continue
        ix = idx.cpu().numpy()
        np.testing.assert_array_equal(ix, _ref_indices(y, rng, np.zeros(len(y), dtype=np.int64)))
        ref = partition_stats(torch.as_tensor(y), torch.as_tensor(ix), P)
        st = out[kind]
        np.testing.assert_array_equal(st[:, 0], ref[:, 0])
        np.testing.assert_array_equal(st[:, 1:3], ref[:, 1:3])
        np.testing.assert_allclose(st[:, 3], ref[:, 3], rtol=1e-13)
        yt = cs.y_s if kind == "Small" else cs.y_l
        perm, ys, seg = ChargingStation._partition_layout(cs, kind, yt, idx)  # (the deferred sort, if any)
        if P <= 16:  # (the statistics came without the sort: the sort's own equal them, sums to rounding)
            srt = cs._lv[kind]["stats_sort"].cpu().numpy()[: 4 * P].reshape(P, 4)
            np.testing.assert_array_equal(srt[:, :3], st[:, :3])
            np.testing.assert_allclose(srt[:, 3], st[:, 3], rtol=1e-13)
        perm, ys = perm.cpu().numpy(), ys.cpu().numpy()
        assert np.array_equal(np.sort(perm), np.arange(len(y)))
        np.testing.assert_array_equal(ys, y[perm])
        for p in range(P):
            a, b = seg[p]
            assert np.array_equal(np.sort(perm[a:b]), np.nonzero(ix == p)[0])
            assert np.all(np.diff(ys[a:b]) <= 0)
            # stable: equal levels keep index order
            eq = np.diff(ys[a:b]) == 0
            assert np.all(np.diff(perm[a:b])[eq] > 0)


class _Solver:  # (what ChargingStation._gamma_layout reads of a PriceSolver)
    def __init__(self, y_max, rank):
        self.consts = type("C", (), {"y_max": y_max})()
        self._r = rank

    def _rank(self):
        return self._r


@pytest.mark.parametrize("rank", [0, 1])
def test_gamma_layout_matches_per_partition_batches(gpu, rank):
    """ChargingStation._gamma_layout (lompc_levels_gamma: every partition's loop-plan batch of a type in
    one launch) equals the per-partition construction of PriceSolver._build_plans bit for bit: each
    partition's y_max - y (ascending), then on rank 0 its central QP's gamma_sc = y_max - (y_hi + y_lo) / 2;
    empty partitions included."""
    rs = np.random.default_rng(90 + rank)
    P = 12
    rng_s = np.linspace(0.3, 0.9, P + 1)
    y = 0.3 + 0.35 * rs.random(40000)  # (partitions 7 .. 11 empty)
    y[:10] = rng_s[rs.integers(0, 7, 10)]
    cs = object.__new__(ChargingStation)
    cs.P, cs.group, cs.device = P, None, 0
    cs.replicated, cs._exchange = False, False
    cs.y_s, cs.y_l = torch.as_tensor(y, device="cuda:0"), torch.as_tensor(y[:5000].copy(), device="cuda:0")
    cs.y0_s_rng, cs.y0_l_rng = rng_s, rng_s
    cs.idx_s = torch.zeros(len(y), dtype=torch.int64, device="cuda:0")
    cs.idx_l = torch.zeros(5000, dtype=torch.int64, device="cuda:0")
    cs._bounds, cs._lv, cs._gl_host, cs._gl_keep = {}, {}, {}, {}
    ChargingStation._update_indices(cs)
    out = ChargingStation._sorted_layouts(cs)
    st = out["Small"]
    _, ys, seg = ChargingStation._partition_layout(cs, "Small", cs.y_s, cs.idx_s)
    sol = _Solver(0.9, rank)
    gam, at = ChargingStation._gamma_layout(cs, sol, ys, seg, st)
    g = gam.cpu().numpy()
    for p in range(P):
        a, b = seg[p]
        ref = (0.9 - ys[a:b]).cpu().numpy()
        v = g[at[p][0]:at[p][1]]
        assert len(v) == b - a + (1 if rank == 0 else 0)
        np.testing.assert_array_equal(v[: b - a], ref)
        assert np.all(np.diff(v[: b - a]) >= 0)
        if rank == 0 and st[p, 0] > 0:
            assert v[-1] == 0.9 - (float(st[p, 1]) + float(st[p, 2])) / 2


@pytest.mark.parametrize("where", [0, 777, 39999])
def test_levels_stats_nan_fails_the_range_check(gpu, where):
    """A NaN charge level reaches the caller: lompc_levels_stats' whole-type max y / min y propagate it
    (fmax / fmin would drop it), so _sorted_layouts' range check fails and the type takes the index
    path — instead of a NaN counted in partition 0 while the deferred sort puts it elsewhere."""
    rs = np.random.default_rng(95)
    P = 12
    rng_s = np.linspace(0.3, 0.9, P + 1)
    y = 0.3 + 0.55 * rs.random(40000)
    y[where] = np.nan
    cs = object.__new__(ChargingStation)
    cs.P, cs.group, cs.device = P, None, 0
    cs.replicated, cs._exchange = False, False
    cs.y_s, cs.y_l = torch.as_tensor(y, device="cuda:0"), torch.as_tensor(y[:5000].copy(), device="cuda:0")
    cs.y_l[:] = 0.5  # (the large type: no NaN)
    cs.y0_s_rng, cs.y0_l_rng = rng_s, rng_s
    cs.idx_s = torch.zeros(len(y), dtype=torch.int64, device="cuda:0")
    cs.idx_l = torch.zeros(5000, dtype=torch.int64, device="cuda:0")
    cs._bounds, cs._lv = {}, {}
    ChargingStation._update_indices(cs)
    out = ChargingStation._sorted_layouts(cs)
    assert set(out) == {"Large"}
    rec = cs._lv["Small"]["stats"].cpu().numpy()
    assert np.isnan(rec[4 * P]) and np.isnan(rec[4 * P + 1])


# ---------------------------------------------------------------------------------------------------
# the three entry points called directly, on guarded buffers (tests/guarded.py), at the partition counts
# and sizes where their code changes path: P = 13 .. 16 the top of k_lvh_partial's register arrays, 17 the
# first count lompc_levels_stats refuses, 256 = LV_MAXP (the end of k_lv_gamma's LDS array); n below one
# wave, around one wave and around the 4096-EV chunks of lompc_levels_stats' workgroups
LV_P = [1, 2, 13, 16, 17, 256]
LV_N = [1, 63, 64, 65, 4095, 4096, 4097, 40000]


def _levels(kind, n, P, bounds, rs):
    """spread: the lower 60 % of the range (the upper partitions empty), levels exactly on boundaries (the
    outermost two included) and ties; one: every level in one middle partition, half of them tied."""
    if kind == "one":
        p = P // 2
        y = bounds[p] + (bounds[p + 1] - bounds[p]) * (0.25 + 0.5 * rs.random(n))
        y[::2] = y[0]
        return y
    y = bounds[0] + 0.6 * (bounds[P] - bounds[0]) * rs.random(n)
    k = min(n, 24)
    y[:k] = bounds[rs.integers(0, P + 1, k)]
    if n >= 4:
        y[n - 4:n - 2] = bounds[[0, P]]
        y[n - 2:] = y[n // 2]
    return y


def _ref_stats(y, bounds):
    P = len(bounds) - 1
    idx = _ref_indices(y, bounds, np.zeros(len(y), dtype=np.int64))
    ref = np.zeros((P, 4))
    for p in range(P):
        v = y[idx == p]
        ref[p] = (len(v), v.max(), v.min(), math.fsum(v)) if len(v) else (0.0, -np.inf, np.inf, 0.0)
    return idx, ref


def _check_stats(st, y, bounds, ref):
    P = len(bounds) - 1
    np.testing.assert_array_equal(st[:4 * P].reshape(P, 4)[:, :3], ref[:, :3])
    np.testing.assert_allclose(st[:4 * P].reshape(P, 4)[:, 3], ref[:, 3], rtol=1e-13)
    np.testing.assert_array_equal(st[4 * P:], [y.max(), y.min(), bounds[0], bounds[P]])


@pytest.mark.parametrize("n", LV_N)
@pytest.mark.parametrize("P", LV_P)
def test_levels_entry_points_extents(gpu, P, n):
    """lompc_levels_layout, lompc_levels_stats and lompc_levels_gamma on guarded buffers: ys / perm bitwise
    np.argsort(-y, kind="stable"), each partition's run the reference's index mask (later partitions
    winning on shared edges), count / max / min exact, sums against math.fsum at 1e-13, the trailing four
    statistics exact; work exactly *work_bytes long, gam exactly n + P central; lompc_levels_stats refuses
    P > 16 with LOMPC_ERR_UNSUPPORTED and writes nothing; every band intact, every input unchanged."""
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    y_max = 0.9
    bounds = np.linspace(0.3, y_max, P + 1)
    for kind in ("spread", "one"):
        rs = np.random.default_rng(1000 * P + n + (kind == "one"))
        y = _levels(kind, n, P, bounds, rs)
        idx, ref = _ref_stats(y, bounds)
        order = np.argsort(-y, kind="stable")
        counts = ref[::-1, 0].astype(np.int64)  # storage order: partition P - 1 first
        runs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        gsc = y_max * rs.random(P)
        wb_l, wb_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert lib.lompc_levels_layout(None, n, None, P, None, None, None, None, ctypes.byref(wb_l), stream) == 0
        rc_s = lib.lompc_levels_stats(None, n, None, P, None, None, ctypes.byref(wb_s), stream)
        assert rc_s == (0 if P <= 16 else _lib.LOMPC_ERR_UNSUPPORTED) and wb_l.value > 0
        gb = Guarded().inp("y", y).inp("bounds", bounds).inp("runs", runs).inp("gsc", gsc).inp("ys_in", y[order])
        gb.out("ys", (n,)).out("perm", (n,), torch.int64).out("stats", (4 * P + 4,)).out("stats_h", (4 * P + 4,))
        gb.out("gam0", (n,)).out("gam1", (n + P,))
        gb.out("work_l", (wb_l.value,), torch.int8).out("work_s", (max(wb_s.value, 16),), torch.int8).build()
        assert lib.lompc_levels_layout(gb.ptr("y"), n, gb.ptr("bounds"), P, gb.ptr("ys"), gb.ptr("perm"), gb.ptr("stats"),
                                       gb.ptr("work_l"), ctypes.byref(wb_l), stream) == 0
        rc = lib.lompc_levels_stats(gb.ptr("y"), n, gb.ptr("bounds"), P, gb.ptr("stats_h"), gb.ptr("work_s"), ctypes.byref(wb_s),
                                    stream)
        assert rc == rc_s
        for central in (0, 1):
            assert lib.lompc_levels_gamma(gb.ptr("ys_in"), n, gb.ptr("runs"), P, y_max, central, gb.ptr("gsc"),
                                          gb.ptr(f"gam{central}"), stream) == 0
        torch.cuda.synchronize()
        gb.check_bands()
        gb.check_inputs()
        for name in ("ys", "perm", "stats", "gam0", "gam1"):
            gb.check_written(name)
        ys, perm = gb.np("ys"), gb.np("perm")
        np.testing.assert_array_equal(perm, order)
        assert np.array_equal(ys.view(np.int64), y[order].view(np.int64))
        _check_stats(gb.np("stats"), y, bounds, ref)
        for p in range(P):  # partition p: the run [c[p + 1], c[p]) of the descending levels
            a, b = runs[P - 1 - p], runs[P - p]
            assert np.array_equal(np.sort(perm[a:b]), np.nonzero(idx == p)[0]), p
        if P <= 16:
            gb.check_written("stats_h")
            _check_stats(gb.np("stats_h"), y, bounds, ref)
        else:
            gb.check_untouched("stats_h")
            gb.check_untouched("work_s")
        g0, g1 = gb.np("gam0"), gb.np("gam1")
        exp = y_max - y[order]
        assert np.array_equal(g0.view(np.int64), exp.view(np.int64))
        for k in range(P):
            a, b = runs[k], runs[k + 1]
            assert np.array_equal(g1[a + k:b + k].view(np.int64), exp[a:b].view(np.int64)), k
            assert g1[b + k] == gsc[k], k
