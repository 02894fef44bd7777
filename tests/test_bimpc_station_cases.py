"""CPU tests of the host BiMPC planner on STATION-SHAPED instances: most partitions empty, the storage
anywhere between empty and full, all three charging costs — what ChargingStation._get_bimpc_solution
hands it, and what tests/test_bimpc_host.py's simplex instances (no empty partition, x0 = 0) never do.

Instances and references: tests/golden/make_bimpc_station_cases.py -> tests/golden/bimpc_station_cases.json
(the generator's ``instance`` is a pure function of the case; the fixture stores each instance with the
dense oracle's optimum, kept only where that optimum is certified to 1e-12 and confirmed to 1e-10 by a
long-double Newton on its active set).  Each test is one planner solve and one certificate; the LIVE cases,
(8, 3) and (12, 1), run the oracle and its confirmation inside the test.

Asserted per case: the solve returns (rc = 0); feasibility 1e-9; the KKT certificate lit.kkt(z, duals) at
CERT; the objective not above the reference's; u_g and the DETERMINED part of w_hat equal to the
reference's at 1e-9 (the bar of test_polish_solves_again_after_releasing_a_row).  Determined
(make_bimpc_station_cases.determined — decided from the instance, never from the planner's output):
UNWEIGHTED all of w_hat; WEIGHTED the rows of populated partitions (an empty partition's rows have weight
0 and no coupling coefficient: free); EXP_UNWEIGHTED the partition sums (A w_hat) at the last stage, with
u_g and the objective, as test_matches_dense_oracle_ipm compares.

CERT = 3e-12: the polished planner's residuals on the drawn instances, measured after the fixes of the
polish, are at worst 2.3e-13 in stationarity (N16_P12_EXP_UNWEIGHTED_seed54_x0.5_station,
2.24e-13 on seed55_x1), 8.8e-16 in complementarity and 0 in dual feasibility (feasibility, held at the
existing 1e-9: 1.4e-13); CERT is one decade above the worst, rounded up.  The unpolished interior-point
iterates sat at 7e-12 .. 1.3e-8 in stationarity or 2e-11 .. 3e-10 in complementarity and fail it.

OBJ = 1e-11 (relative): "not above" up to rounding.  Both points meet their active rows to about 1e-14 and the
multipliers reach delta = 1e3, so two correct points can differ by 1e-11 in objective; the unpolished
iterates were 1e-9 .. 1e-8 above (relative).

Dropped at generation: 2 of the 69 drawn cases (the allowance is 1 in 10), the (48, 12) EXP_UNWEIGHTED ones of
x0 > 0, seeds 72 and 73.  There the ORACLE's polish gives up (weights down to 5^-47) and its interior-point
iterate misses the 1e-12 certificate (stationarity 3.4e-9 and 2.9e-12), so they have no reference point; their
ids and residuals are in the fixture's "dropped" and test_fixture_is_the_generators holds the count.  They stay
in the suite on what needs no reference — rc, feasibility and the certificate (test_dropped_case_certificate) —
and there the PLANNER fails too: its polish ends at the Cholesky of a numerically singular block and it returns
the interior point's iterate, stationarity 1.3e-8 and 1.1e-8.  The N = 48 EXP_UNWEIGHTED class is not fixed, and
these two are strict expected failures with those figures.  (Four more EXP cases, seeds 36, 45, 54 and 82, were
dropped until the oracle's polish took more than six feasibility rounds and, past its tenth pass, released one
row at a time — the planner's own two faults on this class; the planner was polished on them before the oracle.)

The oracle's own changes (oracle/bimpc_oracle.py's polish: a unit diagonal for the variables of a zero-weight
block; the rounds and passes above) are held outside the generation by the LIVE cases, the WEIGHTED ones for the first: G.reference requires lit.kkt of the oracle's point <= 1e-12
and the long-double Newton's agreement to 1e-10 on instances with empty partitions, inside the test.
"""
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import make_bimpc_station_cases as G  # noqa: E402
from lompc_amd.bimpc import BiMPC, BiMPCChargingCostType, BiMPCConstants, BiMPCParameters  # noqa: E402
from lompc_amd.lompc import LoMPCConstants  # noqa: E402

CS = LoMPCConstants(0.05, G.THETA_S, 0.9, G.W_MAX_S, "small")
CL = LoMPCConstants(0.025, G.THETA_L, 0.9, G.W_MAX_L, "large")
CERT, OBJ, ATOL = 3e-12, 1e-11, 1e-9

with open(os.path.join(GOLDEN, "bimpc_station_cases.json")) as _f:
    FIXTURE = json.load(_f)
CASES = {c["id"]: c for c in FIXTURE["cases"]}
NAMED = [G.case_id(c) for c in G.NAMED]


def planner(inst):
    b = inst["bi"]
    bi = BiMPCConstants(b["delta"], b["c_g"], b["u_g_max"], b["u_b_max"], b["x_max"],
                        BiMPCChargingCostType(b["cost_type"]), b["exp_rate"])
    eng = BiMPC(inst["N"], inst["P"], bi, CS, CL)
    ws, wl, ug = eng.solve_bimpc(BiMPCParameters(*[np.asarray(inst[k], dtype=float) for k in G.ARRAYS[:6]],
                                                 inst["x0"], np.asarray(inst["demand"], dtype=float)))  # raises on rc != 0
    return eng, ws, wl, ug


def check(inst, zo):
    N = inst["N"]
    lit = G.literal(inst)
    eng, ws, wl, ug = planner(inst)
    z, zo = lit.pack(ws, wl, ug), np.asarray(zo)
    stat, infeas, comp, dual_inf = lit.kkt(z, eng.last_duals)
    f, fo = lit.objective(z), lit.objective(zo)
    du = float(np.max(np.abs(ug - zo[-N:])))
    dd = float(np.max(np.abs(G.determined(inst, z) - G.determined(inst, zo))))
    print(f"stat {stat:.2e} infeas {infeas:.2e} comp {comp:.2e} dual {dual_inf:.1e}  f - f_ref {f - fo:+.2e} (f {fo:.6g})  "
          f"|u_g - ref| {du:.2e}  |determined - ref| {dd:.2e}")
    assert infeas <= 1e-9
    assert stat <= CERT and comp <= CERT and dual_inf == 0.0
    assert f <= fo + OBJ * max(1.0, abs(fo))
    np.testing.assert_allclose(ug, zo[-N:], rtol=0, atol=ATOL)
    np.testing.assert_allclose(G.determined(inst, z), G.determined(inst, zo), rtol=0, atol=ATOL)


@pytest.mark.parametrize("cid", NAMED)
def test_named_instance(cid):
    """The six instances on which the planner was found returning its unpolished iterate (WEIGHTED cost with
    empty partitions: the zero reduced Hessian of an empty partition's block ended the polish at its
    Cholesky) — before the fix the five WEIGHTED ones had u_g off by 1.2e-5, 6.6e-11, 8.1e-9, 1.6e-9 and
    1.2e-6 (four above the bar), the determined w_hat by 1.4e-8 .. 8.7e-5 and the certificate at 3e-11 .. 4e-9.
    The instances are re-drawn from the report's (N, P, cost, seed, x0) by this generator, not the report's own
    (its generator was not kept).  So the UNWEIGHTED one reproduces nothing: it passed before the fix too, both
    sides agree on it to 3e-15, and the report's 3.5e-6 objective gap remains neither reproduced nor adjudicated;
    it is here as one more (16, 12) case with 8 / 5 empty partitions and a full storage."""
    assert cid in CASES, "a named instance was dropped at generation"
    check(CASES[cid], CASES[cid]["z"])


@pytest.mark.parametrize("cid", [i for i in CASES if i not in NAMED])
def test_station_shaped_case(cid):
    """x0 in {0, 1/2, 1} x_max, the three costs, (N, P) in {(8, 3), (12, 4), (16, 4), (16, 12), (12, 1),
    (48, 12)}; P = 1 with that partition empty for one type and for both; all but one partition empty.
    Two EXP_UNWEIGHTED cases came back unpolished before the polish released one constraint at a time once
    its passes cycle and took more than six feasibility rounds: seed 55 (16, 12) with stationarity 9.4e-9, u_g
    5.3e-8 and the partition sums 1.1e-6 off, seed 64 (12, 1) with complementarity 3.2e-10 and the sums 3.4e-6 off."""
    check(CASES[cid], CASES[cid]["z"])


# the planner's measured miss on the dropped cases it does not polish ("polish: chol"); strict: a
# case that starts to pass has to leave this list
UNPOLISHED = {
    "N48_P12_EXP_UNWEIGHTED_seed72_x0.5_station": "unpolished (polish: chol): stationarity 1.3e-8, complementarity 2.1e-11",
    "N48_P12_EXP_UNWEIGHTED_seed73_x1_station": "unpolished (polish: chol): stationarity 1.1e-8, complementarity 4.7e-13",
}
DROPPED = [pytest.param(d["id"], marks=pytest.mark.xfail(strict=True, reason=UNPOLISHED[d["id"]]))
           if d["id"] in UNPOLISHED else d["id"] for d in FIXTURE["dropped"]]


@pytest.mark.parametrize("cid", DROPPED)
def test_dropped_case_certificate(cid):
    """The cases without a reference (the oracle's certificate failed at generation), on what needs none: the
    solve returns, feasibility 1e-9, the certificate at CERT.  The instance is the generator's."""
    inst = G.instance(next(c for c in G.cases() if G.case_id(c) == cid))
    lit = G.literal(inst)
    eng, ws, wl, ug = planner(inst)
    stat, infeas, comp, dual_inf = lit.kkt(lit.pack(ws, wl, ug), eng.last_duals)
    print(f"stat {stat:.2e} infeas {infeas:.2e} comp {comp:.2e} dual {dual_inf:.1e}")
    assert infeas <= 1e-9
    assert stat <= CERT and comp <= CERT and dual_inf == 0.0


@pytest.mark.parametrize("case", G.LIVE, ids=[G.case_id(c) for c in G.LIVE])
def test_live_oracle_case(case):
    """Small cases with the reference computed here: the dense oracle, certified to 1e-12 and confirmed
    by the long-double Newton to 1e-10 (the generator's own rule), then the same assertions."""
    rec, why = G.reference(case)
    assert rec is not None, why
    check(G.instance(case), rec["z"])


def test_fixture_is_the_generators():
    """The committed instances are the generator's (a pure function of the case); every drawn case is either
    kept or recorded as dropped, and no more than 1 in 10 is dropped."""
    drawn = G.cases()
    ids = [G.case_id(c) for c in drawn]
    dropped = [d["id"] for d in FIXTURE["dropped"]]
    assert FIXTURE["drawn"] == len(drawn) and sorted(list(CASES) + dropped) == sorted(ids)
    assert 10 * len(dropped) <= len(drawn)
    for c in drawn:
        if G.case_id(c) in CASES:
            inst, rec = G.instance(c), CASES[G.case_id(c)]
            assert rec["bi"] == inst["bi"] and rec["x0"] == inst["x0"]
            for k in G.ARRAYS:
                np.testing.assert_array_equal(np.asarray(rec[k]), inst[k], err_msg=f"{rec['id']} {k}")
            assert max(rec["ref_kkt"]) <= 1e-12 and rec["second_dev"] <= 1e-10
    empty = [int((np.asarray(r["Mp_s"]) == 0).sum() + (np.asarray(r["Mp_l"]) == 0).sum()) for r in CASES.values()]
    assert np.mean(np.array(empty) > 0) >= 0.8  # (station-shaped: nearly every instance has an empty partition)
