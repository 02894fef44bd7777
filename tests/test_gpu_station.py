"""GPU tests of the CVXPY-free closed loop (charging_station.py:42-433): the batched
engine + host price / BiMPC solvers against the CPU oracle station
(oracle/station_oracle.py), on the example's constants (real_time_price_control.py:
11-52) with a small EV population, and the EV-sharded loop (2 ranks sharing the
device over gloo) against the single-process loop.

Tolerance: discrete quantities (partition sizes Mp, price iterations, EVs charged)
must match exactly; continuous logs within 1e-6 (relative to the largest entry of
each log, the north star's trajectory tolerance).
"""
import os
import socket

import numpy as np
import pytest
import torch

import lompc_oracle as O
from lompc_amd import settings
from lompc_amd.bimpc import BiMPCChargingCostType, BiMPCConstants
from lompc_amd.charging_station import ChargingStation, ChargingStationConstants
from lompc_amd.demand_data import medium_term_demand_forecast
from lompc_amd.lompc import LoMPCConstants

pytestmark = pytest.mark.gpu

TF, N_LO, N_BI, P = 3, 12, 16, 12


def consts(M_2, Tf=TF, cost=BiMPCChargingCostType.UNWEIGHTED, n_lo=N_LO, n_bi=N_BI, storage=0.3,
           price_type="linear-convex"):
    """The example's constants (real_time_price_control.py:26-52) with the BiMPC charging
    cost UNWEIGHTED by default: with EXP_UNWEIGHTED (rate 5) the first steps of w_hat carry
    weight 5^(t-N+1) ~ 3e-11, so they are determined only to the solvers' tolerance and two
    correct solvers need not agree on them; the trajectory comparison needs a
    BiMPC whose optimum both solvers resolve to ~1e-10."""
    cs = LoMPCConstants(0.05, 10, 0.9, 0.25, "small")
    cl = LoMPCConstants(0.025, 50, 0.9, 0.15, "large")
    bi = BiMPCConstants(1e3, 1, 1, storage, storage, cost, 5)
    demand = medium_term_demand_forecast(Tf + n_bi + 1, 1 / 4 * M_2 / 500, interpolate=False)  # scaled to M_2
    return ChargingStationConstants(Tf, n_bi, n_lo, M_2, P, demand, bi, cs, cl, price_type)


def compare_logs(logs, ol, populated_w_hat_only=False):
    """populated_w_hat_only (WEIGHTED charging cost): w_hat_s / w_hat_l are compared where the oracle's Mp > 0
    at that step — an empty partition's row of w_hat has weight 0 and no coupling coefficient there, so it is
    free and both sides log whatever their solver left in it.  Every other log in full."""
    L = {**logs["inputs"], **logs["bounds"], **logs["prices"], "x": logs["states"]["x"],
         **{k: v for k, v in logs["statistics"].items() if k not in ("ncharged_s", "ncharged_l")}}
    for k in ("Mp_s", "Mp_l", "niter_s", "niter_l"):
        np.testing.assert_array_equal(L[k], ol[k], err_msg=k)
    for k in ("w_s", "w_l", "w_hat_s", "w_hat_l", "beta_s", "beta_l", "gamma_sm", "gamma_lm", "avg_price_s",
              "avg_price_l", "price_red_s", "price_red_l", "u_g", "x"):
        a, b = np.asarray(L[k]), np.asarray(ol[k])
        if populated_w_hat_only and k in ("w_hat_s", "w_hat_l"):
            m = np.asarray(ol["Mp" + k[-2:]]) > 0
            assert m.any() and not m.all()  # (the case has both kinds of partition)
            a, b = a[m], b[m]
        scale = max(1.0, float(np.nanmax(np.abs(b))))
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6 * scale, err_msg=k)


UNW, LC = BiMPCChargingCostType.UNWEIGHTED, "linear-convex"


@pytest.mark.parametrize("n_lo,n_bi,storage,M_2,seed,Tf,cost,price_type",
                         [(N_LO, N_BI, 0.3, 60, 1, TF, UNW, LC), (48, 48, 0.5, 60, 1, TF, UNW, LC),
                          (12, 16, 0.3, 512, 2, 2, UNW, LC), (16, 16, 0.3, 768, 6, 2, UNW, LC),
                          (12, 16, 0.3, 60, 1, 2, BiMPCChargingCostType.WEIGHTED, LC), (12, 16, 0.3, 60, 1, 2, UNW, "linear")],
                         ids=["example", "config5_N48", "mid_N12", "mid_N16", "weighted", "linear_prices"])
def test_closed_loop_matches_oracle(gpu, monkeypatch, n_lo, n_bi, storage, M_2, seed, Tf, cost, price_type):
    """The example's horizons (12 / 16) and config 5's (48 / 48; storage rate and capacity 0.5,
    as bench.py's station leg: at horizon 48 the example's 0.3 / 0.3 leaves the first BiMPC
    infeasible), at M_2 = 60: five EVs per partition.

    mid_N12 / mid_N16: the same loop at mid size, where a partition holds up to a few hundred EVs — the
    sorted layout's piece boundaries and prefix sums, the perm scatter of w0, plan.update between steps
    and the re-draws are compared with the oracle over the trajectory; (16, 16) is the route by which the
    station's own call sequence reaches the <16> kernels.  M_2, seed and Tf were chosen on the oracle
    alone (scripts/select_station_case.py, CPU): the smallest M_2 from 512 and the first seed of 1..8
    whose oracle trajectory has >= 2 distinct active-set patterns (each stage at 0, at w_max, interior)
    among the per-EV optima at the final prices in at least half of its populated (type, partition, step)
    loops, at least one EV of each type changing partition, a re-draw, and every tested average error at
    least 1e-6 tol away from tol.  With Tf = 3 no candidate reached the piece share (M_2 = 512, seeds 1..8:
    0.26-0.43; 768, seeds 1..3: 0.30-0.46 at (12, 16); (16, 16), 512 and 768: 0.23-0.33 — a partition's gamma window is
    0.05 wide whatever M_2, so most loops hold one piece, and the later steps' partitions fewer EVs); the
    oracle's time is dominated by its dense BiMPC interior point (about 2.5 s per step whatever M_2, the M_2 = 60
    cases included), so Tf was lowered to 2.  The script's output for the selected cases:

      n_lo 12 n_bi 16 Tf 2 M_2 512 seed 2: loops 17  >=2-pattern share 0.529  moved s/l 971/1024
        ncharged 53  closest |err - tol| / tol 2.542e-03  max niter 55  oracle 13.05 s
      n_lo 16 n_bi 16 Tf 2 M_2 768 seed 6: loops 16  >=2-pattern share 0.500  moved s/l 1523/1536
        ncharged 13  closest |err - tol| / tol 8.288e-03  max niter 22  oracle 6.71 s

    (seconds with both selections running side by side on a busy host; alone 5.9 s and 6.1 s there, of
    which the two BiMPC solves take about 5; each case, oracle included, 1.7 s on the MI355X machine).
    The oracle's price solvers run its warm C batch there (ps.warm = "state", get_w0_price0_batch: the
    same optima).  mid_N16 failed on its first run (w_hat_s[7, 0] of step 1 off by 1.7e-6): the host
    BiMPC planner's polish, fixed with it (tests/test_bimpc_host.py).

    weighted / linear_prices: the example's horizons at M_2 = 60 over two steps with the WEIGHTED charging
    cost (the planner's empty partitions then carry no weight: w_hat is compared on the populated ones,
    compare_logs) and with the "linear" price type on both sides (r = 2N in the loop step, the chain's
    regularisation and get_w0_price0).  Seeds chosen on the oracle alone, the first of 1..8 whose every
    tested average error is at least 1e-6 tol away from tol and that has a re-draw or a partition move:

      python scripts/select_station_case.py 12 16 2 --small --cost WEIGHTED
      WEIGHTED linear-convex n_lo 12 n_bi 16 Tf 2 M_2 60 seed 1: loops 17  >=2-pattern share 0.294  moved s/l 112/120
        ncharged 8  closest |err - tol| / tol 1.140e-03  max niter 63  oracle 6.02 s  SELECTED
      python scripts/select_station_case.py 12 16 2 --small --price-type linear
      UNWEIGHTED linear n_lo 12 n_bi 16 Tf 2 M_2 60 seed 1: loops 17  >=2-pattern share 0.294  moved s/l 111/120
        ncharged 9  closest |err - tol| / tol 1.734e-03  max niter 45  oracle 5.60 s  SELECTED"""
    import station_oracle as SO

    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c = consts(M_2, Tf=Tf, cost=cost, n_lo=n_lo, n_bi=n_bi, storage=storage, price_type=price_type)
    np.random.seed(seed)
    cs = ChargingStation(c, device=0)
    logs = cs.simulate()
    np.random.seed(seed)
    bi = dict(delta=1e3, c_g=1, u_g_max=1, u_b_max=storage, x_max=storage, cost_type=cost.value, exp_rate=5)
    so = SO.OracleStation(n_bi, n_lo, M_2, P, c.demand, bi, O.small_consts(), O.large_consts(), price_type, Tf)
    if M_2 > 60:
        for ps in (so.ps_s, so.ps_l):
            ps.warm = "state"
            ps.get_w0_price0 = ps.get_w0_price0_batch
    for _ in range(Tf):
        so.step()
    compare_logs(logs, so.logs, populated_w_hat_only=cost == BiMPCChargingCostType.WEIGHTED)
    # logs hold the count before the last state update (_update_logs precedes _update_state, :181-183)
    assert cs.ncharged_s == so.ncharged_s and cs.ncharged_l == so.ncharged_l
    np.testing.assert_allclose(cs.y_s.cpu().numpy(), so.y_s, rtol=0, atol=1e-6)
    np.testing.assert_allclose(cs.y_l.cpu().numpy(), so.y_l, rtol=0, atol=1e-6)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, M_2, q, mode):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import faulthandler
    import traceback

    faulthandler.dump_traceback_later(100, exit=True)  # a hung rank names where it hangs
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        settings.PRINT_LEVEL = 0
        torch.cuda.set_device(0)
        np.random.seed(5)
        cs = ChargingStation(consts(M_2, Tf=2), device=0, group=dist.group.WORLD, sharded_loops=mode)
        assert cs.replicated == (mode == "replicated")
        assert cs.price_solver_s.device_loop == (mode == "replicated")  # (no collective inside a loop)
        logs = cs.simulate()
        q.put((rank, logs["inputs"], logs["prices"], logs["statistics"], logs["states"]["x"], cs.y_s.cpu().numpy(),
               logs["bounds"]))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))
        raise


@pytest.mark.parametrize("mode", ["replicated", "exchange"])
def test_sharded_loop_matches_single_process(gpu, monkeypatch, mode):
    """Two EV shards (gloo over device tensors, both ranks on cuda:0) give the single-process
    trajectory: partition statistics, price0 sums, aggregate demand and the globally ordered
    full-charge re-draws are combined across ranks.  ``replicated`` (the default): one all-gather of
    the levels per step, every price loop on every rank (the device loop, no collective inside it):
    the first step's statistics, BiMPC plan, iteration counts and price reductions equal the single
    process's bit for bit (later steps: the w0 sums' order, to rounding).  ``exchange``: one
    all-gather of the set reductions per price iteration."""
    import torch.multiprocessing as mp

    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    M_2 = 61  # odd: unequal shards
    np.random.seed(5)
    ref = ChargingStation(consts(M_2, Tf=2), device=0).simulate()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, M_2, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    outs = []
    for _ in range(2):  # (a rank's error is reported at once, not after the other rank's timeout)
        o = q.get(timeout=120)
        assert o[1] != "error", f"rank {o[0]}:\n{o[2]}"
        outs.append(o)
    outs.sort(key=lambda o: o[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for _, inputs, prices, stats, x, _, bounds in outs:
        if mode == "replicated":  # step 0 bit for bit: statistics, BiMPC plan, loops
            for sec, k in (("inputs", "w_hat_s"), ("inputs", "w_hat_l"), ("inputs", "u_g"), ("prices", "price_red_s"),
                           ("prices", "price_red_l"), ("statistics", "gamma_sm"), ("statistics", "gamma_lm"),
                           ("bounds", "beta_s"), ("bounds", "beta_l")):
                got = {"inputs": inputs, "prices": prices, "statistics": stats, "bounds": bounds}[sec][k]
                np.testing.assert_array_equal(np.asarray(got)[..., 0], np.asarray(ref[sec][k])[..., 0], err_msg=k)
        for k in ("w_s", "w_l", "w_hat_s", "w_hat_l", "u_g"):
            np.testing.assert_allclose(inputs[k], ref["inputs"][k], rtol=0, atol=1e-9, err_msg=k)
        for k in ("avg_price_s", "avg_price_l"):
            np.testing.assert_allclose(prices[k], ref["prices"][k], rtol=0, atol=1e-9, err_msg=k)
        for k in ("Mp_s", "Mp_l", "niter_s", "niter_l"):
            np.testing.assert_array_equal(stats[k], ref["statistics"][k], err_msg=k)
        assert stats["ncharged_s"] == ref["statistics"]["ncharged_s"]
        np.testing.assert_allclose(x, ref["states"]["x"], rtol=0, atol=1e-12)
