"""CPU tests: the oracle against the committed 50-digit golden vectors and the
reference's own test invariants (chargingstation/test/test_lompc.py)."""
import numpy as np
import pytest

import lompc_oracle as O
import oracle_c
from conftest import oracle_consts

TOL_W = 1e-12  # fp64 oracle vs 50-digit optimum (absolute, w in [0, 0.25])


def test_golden_manifest(golden):
    assert len(golden) == 36
    kinds = {(c["ev_type"], c["N"], c["price"]) for c in golden}
    assert len(kinds) == 18


def test_python_oracle_matches_golden(golden):
    for case in golden[::3]:
        o = O.OracleLoMPC(case["N"], oracle_consts(case))
        for i, g in enumerate(case["gamma"][:6]):
            w, cost = o.solve_lompc(case["lmbd"], case["lmbd_r"], g)
            np.testing.assert_allclose(w, case["w"][i], rtol=0, atol=TOL_W)
            assert abs(cost - case["cost"][i]) <= 1e-10 * max(1.0, abs(case["cost"][i]))


def test_c_oracle_matches_golden(golden):
    for case in golden:
        w, cost, nfail = oracle_c.solve_batch(case["N"], oracle_consts(case), case["lmbd"], case["lmbd_r"],
                                              case["gamma"], nthreads=2)
        assert nfail == 0
        np.testing.assert_allclose(w, case["w"], rtol=0, atol=TOL_W)
        np.testing.assert_allclose(cost, case["cost"], rtol=1e-10, atol=1e-10)


def test_golden_kkt_certificates(golden):
    """Every stored optimum satisfies the KKT conditions in fp64 too."""
    for case in golden:
        o = O.OracleLoMPC(case["N"], oracle_consts(case))
        for i, g in enumerate(case["gamma"]):
            res, infeas = o.kkt_residual(case["w"][i], case["lmbd"], case["lmbd_r"], g, knot_tol=1e-10)
            assert res <= 1e-13 and infeas == 0.0


def test_mp_refinement_certifies_fresh_solve():
    o = O.OracleLoMPC(24, O.large_consts())
    rng = np.random.default_rng(5)
    lmbd = 50 * rng.random(72)
    w, st = o.solve_state(lmbd, 0.7, 0.45)
    wmp, res, _ = O.refine_mp(o, st, lmbd, 0.7, 0.45)
    assert res < 1e-30
    np.testing.assert_allclose(w, wmp, atol=1e-14)


def test_known_answer_zero_price_zero_gamma():
    """lambda = 0, gamma = 0 => w = 0 and cost = 0 (g = 0, H > 0)."""
    for c in (O.small_consts(), O.large_consts()):
        o = O.OracleLoMPC(12, c)
        w, cost = o.solve_lompc(np.zeros(36), 0.0, 0.0)
        assert np.all(w == 0.0) and cost == 0.0


def test_unpriced_response_charges_towards_gamma():
    """test_lompc.py:43-58: with lambda = 0 and gamma = y_max the cumulative
    charge approaches gamma (up to w_max per step)."""
    c = O.small_consts()
    o = O.OracleLoMPC(12, c)
    w, _ = o.solve_lompc(np.zeros(36), 0.0, c.y_max)
    y = np.cumsum(w)
    assert np.all(np.diff(y) >= -1e-15)
    assert y[-1] <= c.y_max + 1e-12 and y[-1] > 0.5 * c.y_max


def test_robustness_bound_invariant():
    """test_lompc.py:61-98: ||w_avg - w_ref||_{A_bar} <= sqrt(N) Gamma_bar."""
    rng = np.random.default_rng(3)
    N = 12
    c = O.small_consts()
    o = O.OracleLoMPC(N, c)
    lmbd = c.theta * rng.random(3 * N)
    kappa = (3 * N) * rng.random() + 1e-5
    lmbd_r = c.delta * kappa
    A_bar = o.A.T @ o.A + kappa * np.eye(N)
    for gmax in (0.9, 0.5, 0.1):
        gam = gmax * rng.random(10)
        w_avg = np.mean([o.solve_lompc(lmbd, lmbd_r, g)[0] for g in gam], axis=0)
        w_ref, _ = o.solve_lompc(lmbd, lmbd_r, (gam.max() + gam.min()) / 2)
        err = np.sqrt((w_avg - w_ref) @ A_bar @ (w_avg - w_ref))
        assert err <= np.sqrt(N) * gmax / 2 + 1e-12


def test_reductions_restate_price_solver(golden):
    """price_solver.py:196-214 / 272-285 restated: recompute from the golden w."""
    for case in golden[:12]:
        o = O.OracleLoMPC(case["N"], oracle_consts(case))
        A_bar, _ = O.w_inner_product_metric(o.A, case["delta"], case["lmbd_r"])
        W = case["w"]
        dv = W - case["w_ref"]
        errs = np.sqrt(np.einsum("bi,ij,bj->b", dv, A_bar, dv))
        assert abs(errs.max() - case["w_err_max"]) <= 1e-10
        w_avg = W.mean(axis=0)
        assert abs(np.sqrt((w_avg - case["w_ref"]) @ A_bar @ (w_avg - case["w_ref"])) - case["w_avg_err"]) <= 1e-10
        np.testing.assert_allclose(W[:, 0], case["w0"], atol=1e-12)


def test_oracle_input_checks():
    o = O.OracleLoMPC(12, O.small_consts())
    with pytest.raises(AssertionError):
        o.solve_lompc(np.zeros(36), 0.0, 0.95)
    with pytest.raises(ValueError):
        o.solve_lompc(-np.ones(36), 0.0, 0.5)
    with pytest.raises(AssertionError):
        O.OracleLoMPC(12, O.OracleConstants(0.05, 10, 0.95, 0.25, "small"))


def test_c_oracle_warm_batch_equals_cold_batch():
    """oracle_c.solve_batch(warm=True) (each solve started from the previous solve's working set)
    returns the same optima as the cold batch (the same final equality-constrained solve)."""
    import oracle_c

    rng = np.random.default_rng(4)
    for c, N in ((O.small_consts(), 48), (O.large_consts(), 48), (O.large_consts(), 12)):
        lm = c.theta * rng.random(3 * N)
        g = np.sort(c.y_max - (0.3 + 0.2 * rng.random(3000)))
        for gg in (g, rng.permutation(g)):
            w, cost, nf = oracle_c.solve_batch(N, c, lm, 0.0, gg)
            w2, cost2, nf2 = oracle_c.solve_batch(N, c, lm, 0.0, gg, warm=True)
            assert nf == nf2 == 0
            np.testing.assert_allclose(w2, w, rtol=0, atol=1e-12)
            np.testing.assert_allclose(cost2, cost, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# The oracle on structured and extreme prices (tests/price_families.py)
# ------------------------------------------------------------------------------------------------
import price_families as PF  # noqa: E402

CERT_NS = [2, 12, 13, 24, 48, 64]
TOL_REF = 1e-10  # oracle vs the 50-digit optimum: a tenth of the GPU tests' 1e-9 bar


def _certify(o, lm, lr, gamma, w_c):
    """One EV: refine_mp on the numpy oracle's final working set, and the 50-digit optimum itself.
    Returns (literal, moves): literal = the oracle's own state is certified as it stands."""
    w, st = o.solve_state(lm, lr, gamma)
    w_st, res, slack = O.refine_mp(o, st, lm, lr, gamma)
    literal = res <= 1e-30 and slack >= 0
    moves = 0
    w_opt = w_st
    if not literal:
        # The working set is wrong at 50 digits.  That is admissible only below the oracle's own
        # release rule (RELEASE_ULPS (N + 2) eps of the magnitudes entering the coordinate, which
        # refine_mp's scale bounds): a multiplier fp64 cannot sign, as an exact tie that the inputs'
        # rounding broke.  The optimum is then finished at 50 digits and must certify there.
        assert res <= O.RELEASE_ULPS * (o.N + 2) * np.finfo(np.float64).eps, (res, slack)
        w_opt, res, slack, _, moves = O.certify_mp(o, st, lm, lr, gamma)
        assert moves > 0
    assert res <= 1e-30 and slack >= 0, (res, slack)
    assert np.max(np.abs(w - w_opt)) <= TOL_REF, np.max(np.abs(w - w_opt))
    assert np.max(np.abs(w_c - w_opt)) <= TOL_REF, np.max(np.abs(w_c - w_opt))
    return literal, moves


@pytest.mark.parametrize("ev_type", ["small", "large"])
@pytest.mark.parametrize("N", CERT_NS)
def test_oracle_certified_on_price_families(N, ev_type):
    """Every price family at both lmbd_r: no failed solve over the whole gamma set, and on a fixed
    sample per (family, lmbd_r) — gamma = 0, gamma = y_max, two more, and the EV where the C oracle and
    the host path engine differ most: at least 8 per family — the numpy oracle's final working set
    certifies at 50 digits (res <= 1e-30, slack >= 0) and both oracles' w are within 1e-10 of the
    50-digit point.

    Where the working set does not certify as it stands, the violation must be below the oracle's own
    release rule and the comparison is with the optimum finished at 50 digits (_certify).  That happens
    for large EVs at lmbd_r = 0 only, on tie_l1_l2, ramp_l1_down, ramp_l2_up (exact ties in real arithmetic,
    broken at 1e-18 relative by the rounding of the inputs) and all_1e-12 (multipliers of 1e-15 relative: the
    prices themselves are below one ulp of the gradient); the distance to the optimum there is at most
    6.6e-12.  Which (family, type, lmbd_r) may do so is an explicit list, asserted below."""
    c = PF.CONSTS[ev_type]()
    o = O.OracleLoMPC(N, c)
    g = PF.gammas(N, ev_type)
    fixed = [int(np.flatnonzero(g == 0.0)[0]), int(np.flatnonzero(g == c.y_max)[0]), 43, 86]
    n_moved = {}
    for fam, lm, lr in PF.cases(N, ev_type):
        w_c, _, nf = oracle_c.solve_batch(N, c, lm, lr, g)
        assert nf == 0, (fam, lr)
        p = oracle_c.path_run(N, [c], [1], lm[None, :], np.array([lr]), g, np.array([0, g.size], dtype=np.int64))
        d = np.max(np.abs(w_c - p["w"]), axis=1)
        worst = int(np.argmax(np.where(np.isnan(d), np.inf, d)))
        for i in sorted(set(fixed + [worst])):
            literal, moves = _certify(o, lm, lr, g[i], w_c[i])
            if not literal:
                n_moved[fam, lr] = n_moved.get((fam, lr), 0) + 1
    print(f"N={N} {ev_type}: sampled EVs finished at 50 digits: {n_moved}")
    # only these may take the non-literal branch: large EVs at lmbd_r = 0 on the exact-tie families (equal
    # lambda_1 and lambda_2, whose price gradient is exactly zero, and the two ramps) and on prices below one
    # ulp of the gradient (every other family, type and lmbd_r certifies as it stands)
    allowed = {(f, 0.0) for f in ("tie_l1_l2", "ramp_l1_down", "ramp_l2_up", "all_1e-12")} if ev_type == "large" else set()
    assert set(n_moved) <= allowed, n_moved


@pytest.mark.parametrize("ev_type,N,ev", [("small", 24, 250), ("large", 48, 508)])
def test_oracle_pinned_huge_component_instances(ev_type, N, ev):
    """theta * rand prices with one lambda_3 component at 3.9e5 theta (PF.pinned_instance).  With the
    release tolerance 1e-12 (1 + max|g| + max|H| w_max N) the oracle kept a working set with a
    wrong-signed multiplier at these EVs (slack -2.3e-7 and -7.7e-7; |dw| 4.7e-7 and 6.5e-6 from the
    host path engine).  Now: the working set certifies as it stands, strictly, both oracles are within
    1e-10 of the 50-digit point, and the whole batch agrees with the path engine at the GPU bar."""
    c, lm, g = PF.pinned_instance(N, ev_type)
    o = O.OracleLoMPC(N, c)
    w_c, _, nf = oracle_c.solve_batch(N, c, lm, 0.0, g)
    assert nf == 0
    w, st = o.solve_state(lm, 0.0, g[ev])
    w_mp, res, slack = O.refine_mp(o, st, lm, 0.0, g[ev])
    assert res <= 1e-30 and slack > 0, (res, slack)
    assert np.max(np.abs(w - w_mp)) <= TOL_REF and np.max(np.abs(w_c[ev] - w_mp)) <= TOL_REF
    p = oracle_c.path_run(N, [c], [1], lm[None, :], np.array([0.0]), g, np.array([0, g.size], dtype=np.int64))
    assert p["info"][3] == 0
    np.testing.assert_allclose(p["w"], w_c, rtol=0, atol=1e-9)
