"""Station-shaped BiMPC planner cases with their reference optima: tests/golden/bimpc_station_cases.json.

    python tests/golden/make_bimpc_station_cases.py [jobs]      (CPU; the dense oracle, minutes)

``instance(case)`` is a pure function of the case (N, P, cost type, seed, x0 / x_max, shape) and is
what tests/test_bimpc_station_cases.py imports for its live cases; the committed fixture stores each
instance next to its reference so that a test is one planner solve plus one certificate.

The instances have the shape the closed loop hands the planner (ChargingStation._get_bimpc_solution):
* counts: Mp_s, Mp_l multinomial over a Dirichlet(1) draw of M = 500 EVs, then each partition zeroed
  with probability 0.4; divided by B = (theta_s + theta_l) M.  Shapes "s_empty" / "both_empty" (P = 1:
  that partition empty for one type / for both) and "one_left" (all but one partition empty, both types)
  set the zeros themselves;
* gamma = 0.6 U, beta = 0.02 U on the populated partitions, 0 on the empty ones;
* demand: N steps of medium_term_demand_forecast / B from a random hour;
* constants: the example's (delta 1e3, c_g 1, u_g_max 1, exp_rate 5), storage rate and capacity 0.3
  (0.5 at N = 48, as config 5), x0 in {0, 1/2, 1} x_max.

Reference: oracle/bimpc_oracle.py's dense interior point and polish.  A case is kept only if
* lit.kkt(z_ref, lam_ref) <= 1e-12 in stationarity, infeasibility and complementarity, and
* a second reference — Newton in long double on the identified active set, with the objective restated
  from the problem's data (``second_reference``) — agrees within 1e-10 on the compared entries (u_g and
  the determined part of w_hat, ``determined`` below).
Dropped cases are printed and recorded in the fixture ("dropped"); more than 1 in 10 is an error.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in ("oracle", "incentive-design-mpc_amd"):
    if os.path.join(ROOT, p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, p))

OUT = os.path.join(HERE, "bimpc_station_cases.json")
THETA_S, THETA_L, W_MAX_S, W_MAX_L = 10, 50, 0.25, 0.15  # the example's EV constants
M = 500
SHAPES = ("station", "s_empty", "both_empty", "one_left")
COST = {0: "WEIGHTED", 1: "UNWEIGHTED", 2: "EXP_UNWEIGHTED"}

GRID_NP = [(8, 3), (12, 4), (16, 4), (16, 12), (12, 1), (48, 12)]
# the six instances of the planner's failure report: (N, P, cost type, seed, x0 / x_max, shape)
NAMED = [(8, 3, 0, 3, 0.0, "station"), (16, 4, 0, 4, 1.0, "station"), (16, 4, 0, 2, 0.0, "station"),
         (12, 4, 0, 0, 0.0, "station"), (12, 1, 0, 5, 0.0, "both_empty"), (16, 12, 1, 3, 1.0, "station")]
# cases small enough for the dense oracle to run inside a test
LIVE = [(8, 3, 0, 11, 0.5, "station"), (8, 3, 1, 12, 1.0, "station"), (8, 3, 2, 13, 0.0, "station"),
        (12, 1, 0, 14, 1.0, "s_empty"), (12, 1, 1, 15, 0.5, "both_empty")]


def cases():
    out = list(NAMED)
    for i, (N, P) in enumerate(GRID_NP):
        for ct in (0, 1, 2):
            for j, x0f in enumerate((0.0, 0.5, 1.0)):
                out.append((N, P, ct, 20 + 9 * i + 3 * ct + j, x0f, "station"))
    for ct in (0, 1, 2):
        out.append((12, 1, ct, 80 + ct, (0.0, 0.5, 1.0)[ct], "s_empty"))
        out.append((12, 1, ct, 83 + ct, (1.0, 0.0, 0.5)[ct], "both_empty"))
        out.append((16, 12, ct, 86 + ct, (0.5, 1.0, 0.0)[ct], "one_left"))
    return out


def case_id(case):
    N, P, ct, seed, x0f, shape = case
    return f"N{N}_P{P}_{COST[ct]}_seed{seed}_x{x0f:g}_{shape}"


def instance(case):
    """The case's planner inputs: dict(N, P, bi, x0, Mp_s, Mp_l, beta_s, beta_l, gamma_sm, gamma_lm, demand)."""
    from lompc_amd.demand_data import medium_term_demand_forecast

    N, P, ct, seed, x0f, shape = case
    rng = np.random.default_rng([N, P, ct, seed, int(round(2 * x0f)), SHAPES.index(shape)])
    B = (THETA_S + THETA_L) * M
    Mp = []
    for _ in range(2):
        c = rng.multinomial(M, rng.dirichlet(np.ones(P)))
        c[rng.random(P) < 0.4] = 0
        Mp.append(c)
    keep = int(rng.integers(P))
    if shape == "s_empty":
        Mp[0][:] = 0
        Mp[1][:] = np.maximum(Mp[1], 1)
    elif shape == "both_empty":
        Mp[0][:] = 0
        Mp[1][:] = 0
    elif shape == "one_left":
        for c in Mp:
            k = max(int(c[keep]), 1)
            c[:] = 0
            c[keep] = k
    stats = []
    for c in Mp:
        stats.append(np.where(c > 0, 0.02 * rng.random(P), 0.0))  # beta
        stats.append(np.where(c > 0, 0.6 * rng.random(P), 0.0))   # gamma
    hour = int(rng.integers(24))
    demand = medium_term_demand_forecast(48 + N, 1 / 4, interpolate=False)[hour: hour + N] / B
    storage = 0.5 if N == 48 else 0.3
    bi = dict(delta=1e3, c_g=1, u_g_max=1, u_b_max=storage, x_max=storage, cost_type=ct, exp_rate=5)
    return dict(N=N, P=P, bi=bi, x0=x0f * storage, Mp_s=Mp[0] / B, Mp_l=Mp[1] / B, beta_s=stats[0], beta_l=stats[2],
                gamma_sm=stats[1], gamma_lm=stats[3], demand=demand)


ARRAYS = ("Mp_s", "Mp_l", "beta_s", "beta_l", "gamma_sm", "gamma_lm", "demand")


def literal(inst):
    import bimpc_oracle as BO

    return BO.BiMPCLiteral(inst["N"], inst["P"], dict(inst["bi"]), THETA_S, THETA_L, W_MAX_S, W_MAX_L,
                           dict(x0=inst["x0"], **{k: np.asarray(inst[k], dtype=float) for k in ARRAYS}))


def determined(inst, z):
    """The entries of a point z = [W_s | W_l | u_g] that the problem determines, as one vector — a property
    of the instance alone.  UNWEIGHTED: all of z.  WEIGHTED: u_g and the rows of W of the populated
    partitions (an empty partition's rows have weight 0 and no coupling coefficient: free).
    EXP_UNWEIGHTED: u_g and the partition sums (A W)[:, N - 1] (the early stages carry weights down to
    5^(1-N): determined only to the solver's tolerance)."""
    N, P, ct = inst["N"], inst["P"], inst["bi"]["cost_type"]
    z = np.asarray(z)
    Ws, Wl, ug = z[: P * N].reshape(P, N), z[P * N: 2 * P * N].reshape(P, N), z[2 * P * N:]
    if ct == 1:
        return z
    if ct == 0:
        return np.concatenate([Ws[np.asarray(inst["Mp_s"]) > 0].ravel(), Wl[np.asarray(inst["Mp_l"]) > 0].ravel(), ug])
    return np.concatenate([Ws.sum(1), Wl.sum(1), ug])


def _solve_ld(K, r):
    """K x = r in long double: Gaussian elimination with partial pivoting; a column whose pivot is below
    1e-13 of the matrix scale is skipped and its unknown left at 0 (an active coupling row that the
    other active rows and the fixed variables already imply: its multiplier is not unique, the point is)."""
    K, r = K.copy(), r.copy()
    m = len(r)
    tol = np.longdouble(1e-13) * np.max(np.abs(K))
    piv, row = [], 0
    for col in range(m):
        if row == m:
            break
        i = row + int(np.argmax(np.abs(K[row:, col])))
        if abs(K[i, col]) <= tol:
            continue
        if i != row:
            K[[row, i]] = K[[i, row]]
            r[[row, i]] = r[[i, row]]
        f = K[row + 1:, col] / K[row, col]
        K[row + 1:, col:] -= f[:, None] * K[row, col:][None, :]
        r[row + 1:] -= f * r[row]
        piv.append((row, col))
        row += 1
    x = np.zeros(m, dtype=np.longdouble)
    for ro, col in reversed(piv):
        x[col] = (r[ro] - K[ro, col + 1:] @ x[col + 1:]) / K[ro, col]
    return x


def second_reference(inst, z, lam, G, h):
    """The optimum again, by another route: Newton in long double on the active set that (z, lam)
    identifies (rows with lam > slack), with the objective restated from the problem's data in long
    double (block k: 2 delta A' diag(omega_k) A, target g_k; c_g u^1.7) instead of the oracle's autograd.
    The variables of an empty partition under the WEIGHTED cost (no weight, no coupling) are not unknowns."""
    ld = np.longdouble
    N, P, bi = inst["N"], inst["P"], inst["bi"]
    n, nb = (2 * P + 1) * N, 2 * P
    act = np.where(lam > h - G @ z)[0]
    fixed = np.zeros(n, dtype=bool)
    x = np.array(z, dtype=ld)
    ub = h[n: 2 * n]
    for j in act[act < 2 * n]:
        fixed[j % n] = True
        x[j % n] = 0.0 if j < n else ub[j - n]
    rows = act[act >= 2 * n]
    A = np.tril(np.ones((N, N), dtype=ld))
    Hb, qb = [], []
    for k in range(nb):
        Mp = ld((inst["Mp_s"] if k < P else inst["Mp_l"])[k % P])
        th = ld(THETA_S if k < P else THETA_L)
        gk = ld((inst["gamma_sm"] if k < P else inst["gamma_lm"])[k % P])
        ct = bi["cost_type"]
        om = np.full(N, (th * Mp) ** 2 if ct == 0 else 1.0, dtype=ld) if ct < 2 else \
            ld(bi["exp_rate"]) ** np.arange(-N + 1, 1).astype(ld)
        if ct == 0 and Mp == 0:
            fixed[k * N: (k + 1) * N] = True
        Hb.append(2 * ld(bi["delta"]) * A.T @ (om[:, None] * A))
        qb.append(-2 * ld(bi["delta"]) * A.T @ (om * gk))
    F = np.where(~fixed)[0]
    Gc = G[rows][:, F].astype(ld)
    for _ in range(12):
        g = np.zeros(n, dtype=ld)
        H = np.zeros((n, n), dtype=ld)
        for k in range(nb):
            sl = slice(k * N, (k + 1) * N)
            g[sl] = Hb[k] @ x[sl] + qb[k]
            H[sl, sl] = Hb[k]
        u = x[nb * N:]
        g[nb * N:] = ld(1.7) * bi["c_g"] * u ** ld(0.7)
        H[nb * N:, nb * N:] = np.diag(ld(1.19) * bi["c_g"] * u ** ld(-0.3))
        K = np.block([[H[np.ix_(F, F)], Gc.T], [Gc, np.zeros((len(rows), len(rows)), dtype=ld)]])
        r = np.concatenate([-g[F], h[rows].astype(ld) - G[rows].astype(ld) @ x])
        d = _solve_ld(K, r)[: len(F)]
        x[F] += d
        if np.max(np.abs(d), initial=0.0) <= 1e-17:
            break
    return x.astype(float)


def reference(case):
    """(record, the oracle's seconds) or (None, reason): the oracle's optimum of the case, certified and
    confirmed."""
    inst = instance(case)
    lit = literal(inst)
    t0 = time.perf_counter()
    z, lam, _ = lit.solve_ipm()
    stat, infeas, comp, dual_inf = lit.kkt(z, lam)
    if not (max(stat, infeas, comp) <= 1e-12 and dual_inf == 0.0):
        return None, f"certificate stat {stat:.1e} infeas {infeas:.1e} comp {comp:.1e} dual {dual_inf:.1e}"
    G, h, _ = lit.dense_data()
    dev = float(np.max(np.abs(determined(inst, second_reference(inst, z, lam, G, h)) - determined(inst, z))))
    if not dev <= 1e-10:
        return None, f"second reference off by {dev:.1e}"
    rec = dict(id=case_id(case), case=list(case), bi=inst["bi"], x0=inst["x0"], N=inst["N"], P=inst["P"],
               **{k: np.asarray(inst[k]).tolist() for k in ARRAYS}, z=z.tolist(),
               ref_kkt=[stat, infeas, comp], second_dev=dev, f=lit.objective(z))
    return rec, f"{time.perf_counter() - t0:.2f} s"


def _one(case):
    try:
        rec, why = reference(case)
    except Exception as e:  # (the oracle itself failing on a case is a dropped case, counted below)
        rec, why = None, f"{type(e).__name__}: {e}"
    print(f"{case_id(case)}: " + (f"kept, kkt {max(rec['ref_kkt']):.1e}, second {rec['second_dev']:.1e}, "
                                  f"{why}" if rec else f"DROPPED ({why})"), flush=True)
    return case, rec, why


def main(argv):
    import multiprocessing as mp

    jobs = int(argv[0]) if argv else 4
    todo = cases()
    with mp.get_context("spawn").Pool(jobs) as pool:
        res = pool.map(_one, todo, chunksize=1)
    kept = [r for _, r, _ in res if r]
    dropped = [dict(id=case_id(c), why=w) for c, r, w in res if not r]
    print(f"{len(kept)} kept, {len(dropped)} dropped of {len(todo)}")
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/make_bimpc_station_cases.py", drawn=len(todo), dropped=dropped,
                       cases=kept), f, separators=(",", ":"))
        f.write("\n")
    assert 10 * len(dropped) <= len(todo), "more than 1 in 10 cases dropped"
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
