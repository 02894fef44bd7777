"""ChargingStation(price_start="own"): every (type, partition) price loop starts from that partition's own
previous prices (zeros at first), so a step's loops of both types are independent and go out as ONE
compute_optimal_prices_parallel call (lompc_price_loops; the persistent loops share k_loop_runs launches).

* batched against ``price_loops_batched = False`` (the same start rule, one lompc_price_loop at a time):
  every log ``array_equal`` — at the oracle comparison's size of test_gpu_station.py (M_2 = 60, horizons
  12 / 16, 3 steps) and at M_2 = 4 096, horizons 12 / 12, 2 steps;
* both against oracle/station_oracle.py's OracleStation with the bars of test_gpu_station.py
  (``compare_logs``: discrete logs exact, continuous 1e-6), its two price solvers wrapped HERE so that
  each partition's loop starts from that partition's own previous prices (``OwnStart``);
* a default-constructed station takes exactly today's path: lompc_price_loops is never called.

The seed of the oracle case (1, test_gpu_station.py's) was checked on the oracle alone under this start
rule, by the criterion of test_gpu_station.py's cases: every tested average error of the trajectory is at
least 1e-6 tol away from tol (467 tests over the 3 steps, the closest |err - tol| / tol = 5.4e-4), so the
iteration counts do not sit on a knife-edge.
"""
import numpy as np
import pytest

import lompc_oracle as O
from lompc_amd import _lib, settings
from lompc_amd.bimpc import BiMPCChargingCostType
from lompc_amd.charging_station import ChargingStation
from test_gpu_station import N_BI, N_LO, P, TF, compare_logs, consts

pytestmark = pytest.mark.gpu

SEED = 1


def simulate(c, seed, **kw):
    np.random.seed(seed)
    batched = kw.pop("batched", True)
    cs = ChargingStation(c, device=0, **kw)
    cs.price_loops_batched = batched
    return cs, cs.simulate()


def assert_logs_equal(a, b, at=""):
    assert type(a) is type(b), at
    if isinstance(a, dict):
        assert a.keys() == b.keys(), at
        for k in a:
            assert_logs_equal(a[k], b[k], f"{at}/{k}")
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=at)


def count_calls(monkeypatch):
    lib = _lib.load()
    calls = []
    inner = lib.lompc_price_loops
    monkeypatch.setattr(lib, "lompc_price_loops", lambda *a: (calls.append(a[0]), inner(*a))[1])
    return calls


class OwnStart:
    """An oracle price solver whose loop for partition p starts from p's own previous prices.  The station
    oracle runs a type's loops in ascending partition order over the populated partitions, which
    ``begin_step`` is given (the indices at the start of the step)."""

    def __init__(self, ps):
        self.ps, self.own, self.parts = ps, {}, iter(())
        self.inner = ps.compute_optimal_prices
        ps.compute_optimal_prices = self.compute

    def begin_step(self, idx):
        self.parts = iter(sorted(set(int(p) for p in idx)))

    def compute(self, w_ref, lmbd_r):
        p = next(self.parts)
        self.ps.prev_prices = self.own.get(p, np.zeros(self.ps.r)).copy()
        lm, st = self.inner(w_ref, lmbd_r)
        self.own[p] = np.array(lm[: self.ps.r], dtype=np.float64)
        return lm, st


def oracle_own(c, seed, Tf):
    import station_oracle as SO

    np.random.seed(seed)
    bi = dict(delta=1e3, c_g=1, u_g_max=1, u_b_max=0.3, x_max=0.3, cost_type=BiMPCChargingCostType.UNWEIGHTED.value,
              exp_rate=5)
    so = SO.OracleStation(N_BI, N_LO, c.nEVs_per_EV_type, P, c.demand, bi, O.small_consts(), O.large_consts(),
                          c.price_type, Tf)
    ws, wl = OwnStart(so.ps_s), OwnStart(so.ps_l)
    for _ in range(Tf):
        ws.begin_step(so.idx_s)
        wl.begin_step(so.idx_l)
        so.step()
    return so


def test_own_start_matches_oracle(gpu, monkeypatch):
    """M_2 = 60, horizons 12 / 16, 3 steps: batched == unbatched on every log, both within
    test_gpu_station.py's bars of the oracle station under the same start rule, and the batched run
    makes one lompc_price_loops call per step."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c = consts(60)
    calls = count_calls(monkeypatch)
    cs, logs = simulate(c, SEED, price_start="own")
    assert len(calls) == TF and all(n >= 2 for n in calls), calls
    cu, logs_u = simulate(c, SEED, price_start="own", batched=False)
    assert len(calls) == TF  # (the unbatched form: lompc_price_loop only)
    assert_logs_equal(logs, logs_u)
    np.testing.assert_array_equal(cs.y_s.cpu().numpy(), cu.y_s.cpu().numpy())
    np.testing.assert_array_equal(cs.y_l.cpu().numpy(), cu.y_l.cpu().numpy())
    so = oracle_own(c, SEED, TF)
    compare_logs(logs, so.logs)
    assert cs.ncharged_s == so.ncharged_s and cs.ncharged_l == so.ncharged_l
    np.testing.assert_allclose(cs.y_s.cpu().numpy(), so.y_s, rtol=0, atol=1e-6)
    np.testing.assert_allclose(cs.y_l.cpu().numpy(), so.y_l, rtol=0, atol=1e-6)
    # another warm start than the chained one: another trajectory (the loops' lengths differ)
    _, chained = simulate(c, SEED)
    assert not np.array_equal(chained["statistics"]["niter_s"], logs["statistics"]["niter_s"])


def test_own_start_batched_equals_unbatched_at_4096(gpu, monkeypatch):
    """M_2 = 4 096, horizons 12 / 12, 2 steps: the batched run against one lompc_price_loop at a time."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c = consts(4096, Tf=2, n_lo=12, n_bi=12)
    cs, logs = simulate(c, 3, price_start="own")
    cu, logs_u = simulate(c, 3, price_start="own", batched=False)
    assert_logs_equal(logs, logs_u)
    np.testing.assert_array_equal(cs.y_s.cpu().numpy(), cu.y_s.cpu().numpy())
    np.testing.assert_array_equal(cs.y_l.cpu().numpy(), cu.y_l.cpu().numpy())
    assert (np.asarray(logs["statistics"]["niter_s"]) > 0).any()


def test_default_station_takes_the_chained_path(gpu, monkeypatch):
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    calls = count_calls(monkeypatch)
    cs, _ = simulate(consts(60, Tf=1), SEED)
    assert cs.price_start == "chained" and calls == []


def test_own_start_refusals(gpu, monkeypatch):
    with pytest.raises(ValueError, match="price_start"):
        ChargingStation(consts(60, Tf=1), device=0, price_start="mine")
    with pytest.raises(ValueError, match="single process"):
        ChargingStation(consts(60, Tf=1), device=0, price_start="own", group=object())
    monkeypatch.setattr(settings, "PRINT_LEVEL", 1)
    with pytest.raises(ValueError, match="PRINT_LEVEL"):
        np.random.seed(SEED)
        ChargingStation(consts(60, Tf=1), device=0, price_start="own").simulate()
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    cs = ChargingStation(consts(60, Tf=1), device=0, price_start="own")
    cs.stage_partitions = False
    with pytest.raises(ValueError, match="staged"):
        cs.simulate()
