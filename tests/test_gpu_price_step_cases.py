"""The device price QP (``nnqp_wave``, csrc/lompc_pricewave.hpp) where its primal active-set fallback runs.

``nnqp_wave`` is run from ``loop_step_core`` by every device form of the price loop.  Its first half, a primal-dual
active set of at most 64 rounds, ends on every input the other loop tests draw; its second half — a primal
active set from x = 0 with a wave-wide ratio test, ``row_argmin`` ties in the host's row order and one row freed
or blocked per round on a single lane — runs near the loop's fixed point, which a station's one-EV and narrow
partitions reach routinely.  tests/price_step_cases.py commits inputs that take it there (the host twin reports
it: ``lompc_price_step``'s ``iterations > 64``; tests/test_price_host.py runs the same cases on the CPU).

ONE device step is what ``lompc_price_loop`` does with ``max_iter = 1`` at a tolerance no error meets (``TOL``):
call 0 steps, call 1 ends at the cap and publishes the stepped prices, w_k, the dual cost, dec_pred[0] and
dec_actual[0] with ``iterations = 1``.  No kernel, entry point or build flag is added for it.

1. ``test_one_step``: every committed case in the loop's four forms — persistent ``k_loop_run2`` at 8 cells and
   at 32 (two closing rounds), unfused at 33 (k_path + k_agg + ``k_loop_step``), the host loop — each device form
   asserted (``assert_form``).  N = 5, 13 take ``k_loop_run2<0>``, 24 and 48 the specialised kernels, 64 =
   LOMPC_MAX_N fills the wave (no lane holds the identity behind the last stage in tri_factor / tri_solve).
   Per case: rc 0, iterations 1, calls 2, prices >= 0 and zero in rows >= r; then, with the dense QP
   (``price_qp_data``) built at the DEVICE's own central optimum (set_sum_w[1] of a run of the same plan at the
   start prices before the loop; within 1e-9 of the oracle's) and x_o the dense oracle's solution of it:
   KKT residual rho_dev <= 1e-9 (1 + max |q|); |x_dev - x_o|_inf <= sqrt(r) (rho_dev + rho_o) / (2 eps_reg) (two
   KKT points of one strictly convex QP whose Hessian's smallest eigenvalue is 2 eps_reg; test_price_host.py's
   bars); dec_pred[0] within 1e-13 mags + rho_dev |x_dev|_1 of the oracle's decrease (the device takes Q x = mu - q
   from its certificate, so the certificate's slack enters); w_k within 1e-9 of ``oracle_c.solve_batch`` at the
   device's stepped prices (in the persistent form the non-writer waves step on their own: different prices
   would show here); the dual cost within 1e-9 relative of the oracle's central cost; dec_actual[0] against its
   definition (price_solver.py:133-138) restated at the oracle's optima, evaluated exactly (below), at rtol 1e-8
   (atol 1e-8 max(1, |.|), test_gpu_price_loop_shapes.py's form).  Every case prints its share of every bar.
2. ``test_batched``: per (constants, N, r) every case as a part of ONE ``lompc_price_loops`` call (``k_loop_runs``),
   and again with max_parts_per_launch = 2: the bits of ``lompc_price_loop`` on a fresh identical plan, ``*launches``
   asserted.
3. ``test_loop_after_a_fallback_step``: per (constants, N), the persistent solver then runs an ordinary loop on
   600 EVs bit for bit as a fresh solver does (test_gpu_price_loop_exits.py section 5's pattern).
4. ``test_natural_one_ev_loops``: whole loops of a one-EV partition (shipped large, linear-convex, default
   tolerance, N 13 and 24) whose CPU emulation takes the fallback, persistent and unfused, under
   ``compare_host`` and ``compare_oracle`` of test_gpu_price_loop_shapes.py, unchanged.

Populations are 8 EVs (1 for the natural loops, 600 for the loop after) plus the central QP; a fallback is a few
hundred reduced solves on one wave (the code bounds it at 64 r + 64 rounds).  The module runs in about 15 s.
Nothing here provokes a fault or a time-out: every case certifies on the host first.

Selection record (scripts/select_price_step_cases.py cases; seed / the host step's iterations per family, - = no
seed in 1..200 — that family of that cell has no case).  All 60 cells have at least one fallback case and their
control, the 29 cells of the coverage condition (every a2 cell, the large lr0 cells other than N64 r2N) among
them; no cell is control-only; 246 cases.

    cell                near-1e-9 near-1e-8 near-1e-6 near-big  control
    small N 5 r2N lr0     1/70    31/71        -     1/70      1/2
    small N 5 r2N lr1    29/72    65/71        -     4/73      1/2
    small N 5 r3N lr0     2/78    21/76   108/76     1/77      1/2
    small N 5 r3N lr1     8/73   127/76        -    17/74      1/4
    small N13 r2N lr0     5/84    12/82        -     1/87      1/3
    small N13 r2N lr1    97/80        -        -    22/83      1/3
    small N13 r3N lr0     2/98    1/102        -     1/96      1/3
    small N13 r3N lr1  122/102   144/93        -     4/87      1/3
    small N24 r2N lr0    1/100   76/111        -    1/106      1/3
    small N24 r2N lr1   194/97        -        -    32/97      1/2
    small N24 r3N lr0    7/112   10/116        -    1/108      1/4
    small N24 r3N lr1        -        -        -   41/109      1/3
    small N48 r2N lr0    2/134        -        -    1/127      1/4
    small N48 r2N lr1        -        -        -  141/125      1/3
    small N48 r3N lr0    8/170   81/165        -    1/188      1/3
    small N48 r3N lr1        -        -        -  111/154      1/3
    small N64 r2N lr0    3/171        -        -    1/183      1/3
    small N64 r2N lr1        -        -        -   11/168      1/3
    small N64 r3N lr0   16/211        -        -    1/209      1/3
    small N64 r3N lr1        -        -        -   63/218      1/4
    large N 5 r2N lr0     1/72    11/73    39/71     1/72      1/2
    large N 5 r2N lr1    12/71     1/73    44/72     5/71      1/2
    large N 5 r3N lr0     1/72     1/76     9/76     1/75      1/3
    large N 5 r3N lr1     3/72    36/75        -     1/71      1/2
    large N13 r2N lr0     1/84     4/85    37/89     1/81      1/2
    large N13 r2N lr1    11/82    19/80        -     1/85      1/2
    large N13 r3N lr0     1/94     5/98     3/94     1/92      1/3
    large N13 r3N lr1     6/99    32/91        -     1/90      1/3
    large N24 r2N lr0     1/94     1/99        -    1/101      1/3
    large N24 r2N lr1   22/106   66/101        -    11/91      1/3
    large N24 r3N lr0    2/124    8/136        -    1/106      1/3
    large N24 r3N lr1   34/123   88/122        -    4/119      1/3
    large N48 r2N lr0    1/143   33/143        -    1/136      1/4
    large N48 r2N lr1        -        -        -    3/129      1/3
    large N48 r3N lr0    1/179    4/181   14/198    1/173      1/3
    large N48 r3N lr1   30/168        -        -    5/161      1/4
    large N64 r2N lr0    2/169   62/159        -    1/149      1/4
    large N64 r2N lr1        -        -        -    3/141      1/4
    large N64 r3N lr0    3/200    3/208        -    1/185      1/4
    large N64 r3N lr1   75/213        -        -   14/214      1/3
    a2    N 5 r2N lr0     3/67     2/69     5/69     1/73      1/2
    a2    N 5 r2N lr1     1/72     1/71    26/69     3/70      1/2
    a2    N 5 r3N lr0     1/76     2/74     2/74     1/76      1/3
    a2    N 5 r3N lr1     5/76     1/76     1/76     1/75      1/2
    a2    N13 r2N lr0     1/80     1/84     1/85     1/84      1/3
    a2    N13 r2N lr1     1/80     1/76    21/84     1/80      1/3
    a2    N13 r3N lr0     1/99     1/93     1/95     1/93      1/2
    a2    N13 r3N lr1     1/84     1/88     7/99     1/96      1/2
    a2    N24 r2N lr0     1/96     1/95    1/108    1/109      1/3
    a2    N24 r2N lr1     1/93     1/94    13/97     1/87      1/3
    a2    N24 r3N lr0    1/116    1/115    4/119    1/132      1/3
    a2    N24 r3N lr1    1/114    2/113   26/117    1/105      1/3
    a2    N48 r2N lr0    1/132    1/141    1/123    1/137      1/3
    a2    N48 r2N lr1    1/122    1/119   35/125    1/122      1/3
    a2    N48 r3N lr0    1/204    1/158    1/184    1/172      1/3
    a2    N48 r3N lr1    1/163    1/169   10/168    1/151      1/3
    a2    N64 r2N lr0    1/172    1/183    1/153    1/202      1/3
    a2    N64 r2N lr1    1/148    3/142    8/146    1/139      1/3
    a2    N64 r3N lr0    1/211    1/221    7/226    1/236      1/3
    a2    N64 r3N lr1    1/207    1/205   73/200    1/186      1/2

Natural loops (scripts/select_price_step_cases.py loops; the knife-edge rule of scripts/check_price_loop_seeds.py
on the oracle's loop, the emulated loop — oracle LoMPC + the host step — of the same count with at least 3 steps of
host ``iterations > 64``).  N 13: seed 1 refused (110 iterations, 2 fallback steps), seed 2 taken: 132
iterations, 13 of them fallback steps, closest error / tolerance ratio 0.24 from 1.  N 24: seed 1 taken: 116
iterations, 13 fallback steps, closest ratio 3.3e-2 from 1.  The loops after (section 3) take 9..24 (small, large)
and 45..149 (a2) steps in the oracle, 0 at a2 N 5 (its tolerance accepts the zero start prices).

Measured on the MI355X (the worst share of each bar over all cases and forms): KKT 0.010, x 0.253, dec_pred
0.010, w_k 1e-6, dual cost 6e-6, dec_actual 0.397 (a2-N64-r3N-lr1-near-big-s1, 3.97e-9).

dec_actual's reference is evaluated EXACTLY (``price_step_cases.dec_actual_exact``: rational arithmetic at the
oracle's optima, rounded once).  Near the fixed point its three terms are 1.45e7 each at prices of 100 theta
(A2-like, N 64) and cancel to 1e-16; summed in fp64 from the oracle's costs, the restatement itself came out at
7.4e-9 for a2-N64-r3N-lr0-near-big-s1 — 4 ulps of the terms, 0.74 of the bar spent by the reference alone — and
the device's -3.8e-9 then read as a miss of 1.118e-8.  Against the exact value the device is at 0.38 of the bar
there.  The bar itself (rtol 1e-8, atol 1e-8 max(1, |.|)) is unchanged.
"""
import functools

import numpy as np
import pytest
import torch

import price_oracle as PO
import price_step_cases as PSC
from lompc_amd import LoMPCConstants, settings
from test_gpu_price_loop_exits import counted, same_bits
from test_gpu_price_loop_shapes import assert_form, compare_host, compare_oracle, consts, oracle_loops, run_loop, solver
from test_gpu_price_loops import Spec, assert_bits, run_batched, run_single, set_levels

pytestmark = pytest.mark.gpu

# The loop's tolerance.  The entry takes any double; 0 would do wherever the error is positive, but clipping makes
# w_ref EQUAL to the central optimum in some committed cases (small-N5-r2N-lr1-near-big-s4: all three errors are
# exactly 0 and the loop converges at call 0 under tolerance 0).  Below zero no error converges, so call 0 steps.
TOL = -1.0
FORMS = {"G8-persistent-1round": (8, True), "G32-persistent-2rounds": (32, True), "G33-unfused": (33, True),
         "host-loop": (8, False)}
GROUPS = PSC.groups()
GROUP_IDS = [f"{cn}-N{N}-r{k}N" for cn, N, k in GROUPS]
SEED_AFTER = 4100
SEED_NATURAL = 4200
NATURAL_N = (13, 24)
NATURAL_PT = "linear-convex"
NATURAL_SEEDS = {13: 2, 24: 1}  # scripts/select_price_step_cases.py loops
WORST = {}  # the largest share of each bar over the module's run (printed by every test)


def lompc_consts(cname):
    c = PSC.CONSTS[cname]
    return consts(cname)[1] if cname in ("small", "large") else LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type)


def spec_of(case, cells, device_loop=True):
    """The case as ONE step of a price loop: max_iter = 1 at a tolerance no error meets."""
    return Spec(case.N, case.consts.ev_type, case.price_type, cells, np.array(case.y0), np.array(case.w_ref),
                lr=case.lmbd_r, start=case.start, max_iter=1, device_loop=device_loop, tol=TOL, lc=lompc_consts(case.cname))


def share(name, value, bar):
    s = value / bar if bar > 0 else (0.0 if value == 0 else np.inf)
    WORST[name] = max(WORST.get(name, 0.0), s)
    return s


def report():
    print("worst share of each bar so far: " + ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))


def central_dev(ps, case):
    """The device's central optimum at the case's start prices: set_sum_w[1] of a run of the loop's own plan,
    taken before the loop.  Within the suite's 1e-9 of the oracle's."""
    A_bar, _ = ps._get_w_inner_product_metric(case.lmbd_r)
    with torch.cuda.stream(ps._stream):
        _, (w, _) = ps._iterate(np.array(case.start), case.lmbd_r, np.array(case.w_ref), A_bar)
    torch.cuda.synchronize()
    assert np.max(np.abs(w - case.w_c)) <= 1e-9, (case.id, float(np.max(np.abs(w - case.w_c))))
    return w


def check_step(case, res, w_dev, what):
    """One device step's outputs against the dense oracle at the device's own central optimum ``w_dev`` and
    against the CPU oracle's LoMPC at the stepped prices.  Returns the bars missed (every case of a test is
    checked before the test asserts that there are none)."""
    c, N, r = case.consts, case.N, case.r
    assert (res["rc"], res["it"], res["calls"]) == (0, 1, 2), (what, res["rc"], res["it"], res["calls"])
    lm = res["lm"]
    assert not lm[r:].any() and np.all(lm >= 0), what
    x, start = lm[:r], case.start[:r]
    P, q, _ = PSC.dense(case, w_dev)
    xo, deco = PSC.dense_oracle(case, w_dev)
    rho_dev, rho_o = PO.price_qp_kkt(P, q, x), PO.price_qp_kkt(P, q, xo)
    bar_kkt = 1e-9 * (1.0 + np.max(np.abs(q)))
    bar_x = np.sqrt(r) * (rho_dev + rho_o) / (2 * PO.EPS_REG)
    mags = abs(start @ P @ start) + abs(q @ start) + abs(x @ P @ x) + abs(q @ x)
    bar_dec = 1e-13 * mags + rho_dev * np.sum(np.abs(x))
    dx = float(np.max(np.abs(x - xo)))
    dec_act, dec_pred = res["dec"][0][0], res["dec"][1][0]
    # the other outputs, at the stepped prices
    w_o, cost_o = PSC.central(N, c, lm, case.lmbd_r, case.gamma_sc)
    dw = float(np.max(np.abs(res["w_k"] - w_o)))
    # price_solver.py:133-138 at the oracle's optima, evaluated exactly: cost_o - case.cost_c + (start - lm)' phi(w_ref)
    # in fp64 carries the rounding of its own three terms, several ulps of them where they cancel
    dec_act_o = PSC.dec_actual_exact(case, lm, w_o)
    bar_act = 1e-8 * abs(dec_act_o) + 1e-8 * max(abs(dec_act_o), 1.0)
    print(f"{what}: KKT {rho_dev:.2e} = {share('kkt', rho_dev, bar_kkt):.3f} of its bar (oracle {rho_o:.2e}); "
          f"|dx| {dx:.2e} = {share('x', dx, bar_x):.3f}; |dec_pred - oracle| {abs(dec_pred - deco):.2e} = "
          f"{share('dec_pred', abs(dec_pred - deco), bar_dec):.4f}; |dw_k| {dw:.2e} = {share('w_k', dw, 1e-9):.3f}; "
          f"dual cost {share('dual_cost', abs(res['dual'] - cost_o), 1e-9 * max(1.0, abs(cost_o))):.3f}; "
          f"|dec_actual - oracle| {abs(dec_act - dec_act_o):.2e} = {share('dec_actual', abs(dec_act - dec_act_o), bar_act):.3f}")
    checks = (("KKT", rho_dev, bar_kkt), ("x", dx, bar_x), ("dec_pred", abs(dec_pred - deco), bar_dec), ("w_k", dw, 1e-9),
              ("dual_cost", abs(res["dual"] - cost_o), 1e-9 * max(1.0, abs(cost_o))),
              ("dec_actual", abs(dec_act - dec_act_o), bar_act))
    return [f"{what}: {name} {value:.3e} above its bar {bar:.3e}" for name, value, bar in checks if not value <= bar]


def one_step(ps, case, cells):
    """The case through ``lompc_price_loop`` with max_iter = 1 on ``ps`` (re-targeted at the case's levels),
    its form asserted, its outputs checked: the bars missed."""
    spec = spec_of(case, cells, ps.device_loop)
    set_levels(ps, spec)
    w_dev = central_dev(ps, case)
    res, n = counted(ps._plan, lambda: run_single(spec, ps))
    assert isinstance(res, dict), res
    if ps.device_loop:
        assert_form(ps, {"iter": res["it"]}, n, cells)
    else:
        assert n == {"k_path": 2, "k_eval": 2}, n  # (the host loop: one engine call per launch pair)
    return check_step(case, res, w_dev, f"{case.id} G{cells}{'' if ps.device_loop else ' host loop'}")


# ------------------------------------------------------------------ 1. one step in the loop's four forms
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_one_step(gpu, monkeypatch, group, form):
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    cells, device_loop = FORMS[form]
    cname, N, k = group
    ps = solver(N, lompc_consts(cname), "linear" if k == 2 else "linear-convex", cells, device_loop=device_loop)
    missed = []
    for case in GROUPS[group]:
        missed += one_step(ps, case, cells)
    report()
    assert not missed, missed


# ------------------------------------------------------------------ 2. the batched form
@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_batched(gpu, monkeypatch, group):
    """Every case of the group as a part of ONE lompc_price_loops call (k_loop_runs; both lmbd_r, fallback and
    control parts side by side), then split into launches of at most 2 parts: each part carries the bits of
    lompc_price_loop on a fresh identical plan."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    specs = [spec_of(case, 8) for case in GROUPS[group]]
    want = [run_single(s) for s in specs]
    for case, w in zip(GROUPS[group], want):
        assert (w["rc"], w["it"], w["calls"]) == (0, 1, 2), (case.id, w["rc"], w["it"], w["calls"])
    for mppl, launches_want in ((0, 1), (2, (len(specs) + 1) // 2)):
        rc, launches, got, _ = run_batched(specs, mppl=mppl)
        assert rc == 0 and launches == launches_want, (rc, launches, launches_want)
        for case, g, w in zip(GROUPS[group], got, want):
            assert_bits(g, w, f"{case.id} max_parts_per_launch {mppl}")


# ------------------------------------------------------------------ 3. the loop after a fallback step
AFTER = [next(c for c in GROUPS[cn, N, 3] if c.family != "control") for cn in PSC.CONSTS for N in PSC.HORIZONS]


def after_call(case):
    c = case.consts
    rng = np.random.default_rng(SEED_AFTER + case.N + 100 * list(PSC.CONSTS).index(case.cname))
    return 0.3 + 0.04 * c.y_max * rng.random(600), c.w_max * (0.2 + 0.6 * rng.random(case.N)), 0.0


@pytest.mark.parametrize("case", AFTER, ids=lambda c: c.id)
def test_loop_after_a_fallback_step(gpu, monkeypatch, case):
    """The persistent form's solver, after a step whose QP fell back, runs an ordinary converging loop on 600
    EVs: bit for bit a fresh solver's (test_gpu_price_loop_exits.py section 5's pattern) — the loop's kept
    A_bar factor and state do not leak."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    lc = lompc_consts(case.cname)
    ps, fresh = solver(case.N, lc, case.price_type, 8), solver(case.N, lc, case.price_type, 8)
    missed = one_step(ps, case, 8)
    assert not missed, missed
    y0, w_ref, lr = after_call(case)
    ra, rf = run_loop(ps, y0, w_ref, lr), run_loop(fresh, y0, w_ref, lr)
    assert ra[2] == ra[1]["iter"] + 1 < 1000  # (converged: not the cap, no error)
    print(f"{case.id}: the loop after took {ra[1]['iter']} steps")
    # (the oracle's counts are 9..149; at A2-like N = 5 its tolerance accepts the zero prices: the loop ends at its
    # first test, which still has to find the earlier loop's finished flag and records gone)
    assert ra[1]["iter"] >= 2 or (case.cname, case.N) == ("a2", 5), ra[1]["iter"]
    assert_form(ps, ra[1], ra[3], 8)
    same_bits(ra, rf)
    assert ra[3] == rf[3], (ra[3], rf[3])


# ------------------------------------------------------------------ 4. the natural route: one-EV loops
def natural_calls(N, seed):
    c = PSC.CONSTS["large"]
    rng = np.random.default_rng(SEED_NATURAL + 100 * N + seed)
    y0 = np.array([(0.3 + 0.2 * rng.random()) * c.y_max])
    return [(y0, c.w_max * (0.2 + 0.6 * rng.random(N)), 0.0)]


@functools.lru_cache(maxsize=None)
def oracle_natural(N):
    return oracle_loops(N, "large", NATURAL_PT, natural_calls(N, NATURAL_SEEDS[N]))


@pytest.mark.parametrize("cells", [8, 33], ids=["G8-persistent", "G33-unfused"])
@pytest.mark.parametrize("N", NATURAL_N)
def test_natural_one_ev_loops(gpu, monkeypatch, N, cells):
    """Whole loops of a one-EV partition at the default tolerance, on seeds whose CPU emulation (oracle LoMPC +
    the host step) takes the fallback at 3 steps or more: against the host loop and the oracle loop with
    test_gpu_price_loop_shapes.py's bars, unchanged."""
    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    c, lc = consts("large")
    dev, host = solver(N, lc, NATURAL_PT, cells), solver(N, lc, NATURAL_PT, cells, device_loop=False)
    (y0, w_ref, lr), = natural_calls(N, NATURAL_SEEDS[N])
    rd = run_loop(dev, y0, w_ref, lr)
    assert_form(dev, rd[1], rd[3], cells)
    compare_host(rd, run_loop(host, y0, w_ref, lr), c.theta)
    compare_oracle(dev, rd, oracle_natural(N)[0], lr, c)
