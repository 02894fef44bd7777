"""lompc_price_step_many / LoMPC.price_step_many (k_price_steps, csrc/lompc_pricemany.hip) and the per-EV price
loops on top of it and lompc_solve_many (price_solver.personal_prices).

The step of QP k is the price-gradient step of price_solver.py:216-246 at (w_k, w_ref_k, lmbd_k, lmbd_r_k); its
reference is the dense oracle (oracle/price_oracle.py: ``price_qp_data``, ``price_step`` — Lawson-Hanson on the
Cholesky factor — and ``price_qp_kkt``) with the bars of test_gpu_price_step_cases.py::test_one_step:

    KKT   rho_dev <= 1e-9 (1 + max |q|)
    x     |x_dev - x_o|_inf <= sqrt(r) (rho_dev + rho_o) / (2 eps_reg)     (two KKT points of one strictly convex QP
                                                                           whose Hessian's least eigenvalue is 2 eps_reg)
    dec   |dec_dev - dec_o| <= 1e-13 magnitudes + rho_dev |x_dev|_1        (the device takes Q x = mu - q from its
                                                                           certificate, so the certificate's slack enters)

and the x bar again against the host ``lompc_price_step`` on the same inputs (with the host's own residual).

1. ``test_committed_cases``: per (constants, N, r) of tests/price_step_cases.py every case of the cell in ONE call
   (w = the case's w_c, its w_ref, start prices and lmbd_r): N in {5, 13, 24, 48, 64} (64 fills the wave), the
   families whose QP takes nnqp_wave's primal fallback and their controls.  Rows >= r zero, x >= 0, state RUNNING,
   iters 1.
2. ``test_random_batch``: K = 257 (a last workgroup with one wave of four), N in {2, 13, 64}, both EV types, r in
   {2N, 3N}, lmbd_r NULL and per QP.  Same bars.
3. ``test_bits_do_not_depend_on_placement``: a QP's row and dec are the same bits alone (K = 1), at position 0, 3, 4
   and 256 of K = 257, with lmbd_stride = r + 5 / next_stride = 3N + 3 and NaN padding (the output's padding keeps
   its pattern), and in place.
4. ``test_state_rules``: frozen QPs, err == tol against nextafter(tol), every kind of invalid input (and the
   neighbours' bits), counts, iters over two calls.
5. ``test_extents``: through tests/guarded.py at N in {2, 13, 63, 64}, K in {1, 5}: bands intact, inputs unchanged,
   every requested output written to its last element, every optional pointer NULL in turn.
6. ``test_refusals_write_nothing``.
7. ``test_personal_prices``: against a restatement of ``price_oracle.OraclePriceSolver.compute_optimal_prices``'
   loop for ONE EV (no LP, from zero prices): OracleLoMPC.solve_lompc, price_oracle.price_step,
   w_inner_product_metric, get_robustness_bounds(y0_rng = 0).  Shipped small and large constants, N in {5, 13}, r in
   {2N, 3N}, K = 9, cap 60; per cell drawn with default_rng(1), for j = 0..8 in order: gamma = y_max (0.3 + 0.6 u),
   w_ref = w_max (0.2 + 0.6 U^N), lmbd_r = 0 for even j, else 1.5 N delta u.  On the CPU with the oracle alone every
   cell has both converged loops (7 to 54 steps) and loops that reach the cap, and no error / tolerance ratio before
   or at an exit lies closer to 1 than 1.3e-2; the project's knife-edge margin is 1e-6
   (scripts/check_price_loop_seeds.py) and the test re-asserts it on the restatement, as a condition.  Asserted:
   iters and state identical for all 9 EVs; prices per component within 1e-6 max(theta, |lmbd_i|) (the long-loop
   test's bar); w within 1e-6 of the oracle's optimum at the oracle's final prices and within 1e-9 of
   oracle_c.solve_batch at the device's own final prices; solves = max(iters) + 1.  One more case starts from given
   prices with max_iter = 3.

Every test prints the worst share of each bar so far.  Measured on the MI355X (the worst share of each bar over the
module's 75 tests): KKT 0.010, x against the dense oracle 0.252, x against the host step 0.169, dec 0.020; the loops'
prices 2.7e-5, w against the oracle's optimum 1.4e-6, w at the device's own prices 2.1e-6.  Every loop took the
oracle's number of steps.  The module runs in about 27 s; the N = 64 random batches take 1.4 to 3.6 s each, nearly all
of it the dense oracle's 257 Lawson-Hanson solves on the CPU (computed once per family).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import lompc_oracle as O
import oracle_c
import price_oracle as PO
import price_step_cases as PSC
from guarded import Guarded
from lompc_amd import LoMPC, LoMPCConstants, _lib
from lompc_amd.price_solver import personal_prices

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

guarded.SENTINEL.setdefault(torch.int32, 0x5A5A5A5B)  # (iters is the one int32 buffer of the C ABI)
RUN, CONV, FAIL, INV = (_lib.LOMPC_STEP_RUNNING, _lib.LOMPC_STEP_CONVERGED, _lib.LOMPC_STEP_FAILED,
                        _lib.LOMPC_STEP_INVALID)
EPS = PO.EPS_REG
K0 = 257
PAT = guarded.SENTINEL[torch.float64]
GROUPS = PSC.groups()
GROUP_IDS = [f"{cn}-N{N}-r{k}N" for cn, N, k in GROUPS]
WORST = {}


def share(name, value, bar):
    s = value / bar if bar > 0 else (0.0 if value == 0 else np.inf)
    WORST[name] = max(WORST.get(name, 0.0), s)
    return s


def report():
    print("worst share of each bar so far: " + ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))


@functools.lru_cache(maxsize=None)
def ctx(cname, N):
    c = PSC.CONSTS[cname]
    return LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0)


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def nbits(a):
    return np.ascontiguousarray(a).view(np.int64)


def step(lo, r, w, wr, lm, lr=None, err=None, tol=0.0, state="zeros", iters="zeros", in_place=False, ls=None, ns=None,
         eps=EPS):
    """One lompc_price_step_many through the C ABI on fresh buffers.  lm: (K, cols) host prices, laid out with
    stride ls (NaN padding); the output with stride ns, filled with a pattern first."""
    K, N = w.shape
    ls = ls or lm.shape[1]
    ns = ns or 3 * N
    lin = np.full((K, ls), np.nan)
    lin[:, :min(ls, lm.shape[1])] = lm[:, :min(ls, lm.shape[1])]
    t_lm = dev(lin)
    if in_place:
        nxt = t_lm
    else:
        nxt = torch.empty((K, ns), dtype=torch.float64, device="cuda:0")
        bits(nxt).fill_(PAT)
    t = {"w": dev(w), "wr": dev(wr), "lr": dev(lr), "err": dev(err)}
    dec = torch.empty(K, dtype=torch.float64, device="cuda:0")
    st = torch.zeros(K, dtype=torch.int8, device="cuda:0") if isinstance(state, str) else dev(state, torch.int8)
    it = torch.zeros(K, dtype=torch.int32, device="cuda:0") if isinstance(iters, str) else dev(iters, torch.int32)
    counts = torch.full((4,), -7, dtype=torch.int64, device="cuda:0")
    rc = lo._lib.lompc_price_step_many(lo._ctx, K, r, eps, ptr(t["w"]), ptr(t["wr"]), ptr(t_lm), ls, ptr(t["lr"]),
                                       ptr(t["err"]), tol, ptr(nxt), ns, ptr(dec), ptr(st), ptr(it), ptr(counts),
                                       lo._stream())
    assert rc == _lib.LOMPC_OK, _lib.status_text(lo._lib, lo._ctx, rc)
    torch.cuda.synchronize()
    full = nxt.cpu().numpy()
    return {"full": full, "x": full[:, :3 * N].copy(), "dec": dec.cpu().numpy(), "state": st.cpu().numpy(),
            "iters": it.cpu().numpy(), "counts": counts.cpu().numpy()}


def host_step(c, N, r, m, lr, w, wr, start):
    """lompc_price_step on the same inputs: (rc, x (r,))."""
    lib = _lib.load()
    w, wr, lm = (np.ascontiguousarray(a, dtype=np.float64) for a in (w, wr, start[:r]))
    out = np.empty(r)
    dec = ctypes.c_double(np.nan)
    rc = lib.lompc_price_step(N, r, c.theta, c.w_max, m, lr / c.delta, EPS, wr.ctypes.data, w.ctypes.data, lm.ctypes.data,
                              out.ctypes.data, ctypes.byref(dec), None)
    return rc, out


def bars(what, P, q, start, xo, deco, xh, x3, dec, r):
    """The bars missed by one QP's device step x3 (3N,), dec."""
    assert not x3[r:].any() and np.all(x3 >= 0), what
    x = x3[:r]
    rho_dev, rho_o, rho_h = PO.price_qp_kkt(P, q, x), PO.price_qp_kkt(P, q, xo), PO.price_qp_kkt(P, q, xh)
    bar_kkt = 1e-9 * (1.0 + np.max(np.abs(q)))
    bar_x = np.sqrt(r) * (rho_dev + rho_o) / (2 * EPS)
    bar_h = np.sqrt(r) * (rho_dev + rho_h) / (2 * EPS)
    mags = abs(start @ P @ start) + abs(q @ start) + abs(x @ P @ x) + abs(q @ x)
    bar_dec = 1e-13 * mags + rho_dev * np.sum(np.abs(x))
    dx, dh, dd = float(np.max(np.abs(x - xo))), float(np.max(np.abs(x - xh))), abs(dec - deco)
    checks = (("kkt", rho_dev, bar_kkt), ("x", dx, bar_x), ("x_host", dh, bar_h), ("dec", dd, bar_dec))
    for name, value, bar in checks:
        share(name, value, bar)
    return [f"{what}: {name} {value:.3e} above its bar {bar:.3e}" for name, value, bar in checks if not value <= bar]


# ------------------------------------------------------------------ 1. the committed cases
@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_committed_cases(gpu, group):
    cname, N, k = group
    r, cases = k * N, GROUPS[group]
    lo = ctx(cname, N)
    w, wr, lm = (np.stack([getattr(c, n) for c in cases]) for n in ("w_c", "w_ref", "start"))
    lr = np.array([c.lmbd_r for c in cases])
    out = step(lo, r, w, wr, lm, lr)
    assert np.all(out["state"] == RUN) and np.all(out["iters"] == 1), (out["state"], out["iters"])
    assert out["counts"].tolist() == [len(cases), 0, 0, 0]
    missed = []
    for j, case in enumerate(cases):
        P, q, _ = PSC.dense(case)
        xo, deco = PSC.dense_oracle(case)
        rc, xh, _, _ = PSC.host_step(case)
        assert rc == 0, case.id
        missed += bars(case.id, P, q, case.start[:r], xo, deco, xh, out["x"][j], out["dec"][j], r)
    report()
    assert not missed, missed


# ------------------------------------------------------------------ 2. a random batch
RANDOM = [(ev, N, k, per) for ev in ("small", "large") for N in (2, 13, 64) for k in (2, 3) for per in (False, True)]


@functools.lru_cache(maxsize=None)
def random_inputs(ev, N, k):
    """(w, w_ref, lmbd (K0, 3N) with rows >= r zero and about 40 % exact zeros below, lmbd_r) of the family."""
    c = PSC.CONSTS[ev]
    rng = np.random.default_rng(7000 + 10 * N + 2 * k + (ev == "large"))
    r = k * N
    w, wr = c.w_max * rng.random((K0, N)), c.w_max * rng.random((K0, N))
    lm = np.zeros((K0, 3 * N))
    lm[:, :r] = c.theta * rng.random((K0, r)) * (rng.random((K0, r)) < 0.6)
    lr = 1.5 * N * c.delta * rng.random(K0)
    for a in (w, wr, lm, lr):
        a.setflags(write=False)
    return w, wr, lm, lr


def dense_of(ev, N, r, lr, w, wr, start):
    c = PSC.CONSTS[ev]
    m = 2 * c.delta * c.theta ** 2
    _, A_bar_inv = O.w_inner_product_metric(np.tril(np.ones((N, N))), c.delta, lr)
    return c, m, A_bar_inv


@functools.lru_cache(maxsize=None)
def random_oracle(ev, N, k, per):
    """Per QP of the family: (x_o, dec_o, x_host), computed once."""
    w, wr, lm, lr = random_inputs(ev, N, k)
    r, out = k * N, []
    for j in range(K0):
        lrj = lr[j] if per else 0.0
        c, m, Ainv = dense_of(ev, N, r, lrj, w[j], wr[j], lm[j])
        xo, deco = PO.price_step(N, r, c.theta, c.w_max, m, Ainv, wr[j], w[j], lm[j, :r])
        rc, xh = host_step(c, N, r, m, lrj, w[j], wr[j], lm[j])
        assert rc == 0
        out.append((xo, deco, xh))
    return out


@pytest.mark.parametrize("ev,N,k,per", RANDOM, ids=[f"{ev}-N{N}-r{k}N-{'lr' if per else 'null'}" for ev, N, k, per in RANDOM])
def test_random_batch(gpu, ev, N, k, per):
    w, wr, lm, lr = random_inputs(ev, N, k)
    r = k * N
    out = step(ctx(ev, N), r, w, wr, lm, lr if per else None)
    assert np.all(out["state"] == RUN) and np.all(out["iters"] == 1) and out["counts"].tolist() == [K0, 0, 0, 0]
    missed = []
    for j, (xo, deco, xh) in enumerate(random_oracle(ev, N, k, per)):
        c, m, Ainv = dense_of(ev, N, r, lr[j] if per else 0.0, w[j], wr[j], lm[j])
        P, q, _ = PO.price_qp_data(N, r, c.theta, c.w_max, m, Ainv, wr[j], w[j], lm[j, :r])
        missed += bars(f"{ev} N{N} r{k}N QP {j}", P, q, lm[j, :r], xo, deco, xh, out["x"][j], out["dec"][j], r)
    report()
    assert not missed, missed


# ------------------------------------------------------------------ 3. placement
@pytest.mark.parametrize("ev,N,k", [("large", 13, 3), ("small", 64, 2)])
def test_bits_do_not_depend_on_placement(gpu, ev, N, k):
    lo = ctx(ev, N)
    w, wr, lm, lr = random_inputs(ev, N, k)
    r = k * N
    base = step(lo, r, w, wr, lm, lr)
    again = step(lo, r, w, wr, lm, lr)
    assert np.array_equal(nbits(again["x"]), nbits(base["x"])) and np.array_equal(nbits(again["dec"]), nbits(base["dec"]))
    for j in (0, 3, 4, 256):  # alone: K = 1
        one = step(lo, r, w[j:j + 1], wr[j:j + 1], lm[j:j + 1], lr[j:j + 1])
        assert np.array_equal(nbits(one["x"][0]), nbits(base["x"][j])), j
        assert nbits(one["dec"])[0] == nbits(base["dec"])[j], j
    moved = [256, 4, 3, 0] + list(range(5, 256)) + [1, 2]  # (every QP somewhere else)
    perm = step(lo, r, w[moved], wr[moved], lm[moved], lr[moved])
    assert np.array_equal(nbits(perm["x"]), nbits(base["x"][moved])) and np.array_equal(nbits(perm["dec"]), nbits(base["dec"][moved]))
    pad = step(lo, r, w, wr, lm[:, :r], lr, ls=r + 5, ns=3 * N + 3)  # NaN between the vectors read, a pattern between those written
    assert np.array_equal(nbits(pad["x"]), nbits(base["x"])) and np.array_equal(nbits(pad["dec"]), nbits(base["dec"]))
    assert np.all(nbits(pad["full"][:, 3 * N:]) == np.int64(PAT))
    inp = step(lo, r, w, wr, lm, lr, in_place=True)
    assert np.array_equal(nbits(inp["x"]), nbits(base["x"])) and np.array_equal(nbits(inp["dec"]), nbits(base["dec"]))


# ------------------------------------------------------------------ 4. the state rules
def test_state_rules(gpu):
    ev, N, k = "large", 13, 2
    lo, c = ctx(ev, N), PSC.CONSTS[ev]
    r, K = k * N, 24
    w, wr, lm, lr = (a[:K].copy() for a in random_inputs(ev, N, k))
    lm[:, r:] = np.nan  # rows >= r are never read
    err, tol = np.full(K, 1.0), 0.5
    base = step(lo, r, w, wr, lm, lr, err, tol)
    assert np.all(base["state"] == RUN) and np.all(base["iters"] == 1) and not np.isnan(base["x"]).any()
    assert not base["x"][:, r:].any()

    # frozen QPs keep their prices, state and iters; err == tol converges, the next double steps
    state, iters = np.zeros(K, dtype=np.int8), np.arange(K, dtype=np.int32) + 10
    state[[2, 7, 11]] = [CONV, FAIL, INV]
    e = err.copy()
    e[4], e[5] = tol, np.nextafter(tol, np.inf)
    w2 = w.copy()
    w2[7] = np.nan  # (a frozen QP is not validated)
    out = step(lo, r, w2, wr, lm, lr, e, tol, state=state, iters=iters)
    want = state.copy()
    want[4] = CONV
    assert out["state"].tolist() == want.tolist()
    kept = [2, 7, 11, 4]
    assert np.array_equal(nbits(out["x"][kept, :r]), nbits(lm[kept, :r])) and not out["x"][kept, r:].any()
    assert np.all(out["dec"][kept] == 0.0)
    stepped = np.setdiff1d(np.arange(K), kept)
    assert np.array_equal(nbits(out["x"][stepped]), nbits(base["x"][stepped]))
    assert np.array_equal(nbits(out["dec"][stepped]), nbits(base["dec"][stepped]))
    assert out["iters"].tolist() == (iters + np.isin(np.arange(K), stepped)).tolist()
    assert out["counts"].tolist() == np.bincount(out["state"], minlength=4).tolist() and out["counts"].sum() == K

    # every kind of invalid input is that QP's own
    def edit(name, j, i, v):
        a = {"w": w, "wr": wr, "lm": lm, "lr": lr, "err": err}
        a = {n: x.copy() for n, x in a.items()}
        if i is None:
            a[name][j] = v
        else:
            a[name][j, i] = v
        return a

    kinds = [("w", 1, 0, np.nan), ("w", 6, N - 1, np.nan), ("wr", 3, N - 1, np.nan), ("lm", 4, 0, np.nan),
             ("lm", 8, r - 1, np.nan), ("lm", 23, N, -1e-9), ("lm", 9, r - 1, -np.inf), ("lr", 12, None, np.nan),
             ("lr", 0, None, -1e-12), ("err", 20, None, np.nan)]
    for name, j, i, v in kinds:
        a = edit(name, j, i, v)
        out = step(lo, r, a["w"], a["wr"], a["lm"], a["lr"], a["err"], tol)
        good = np.setdiff1d(np.arange(K), [j])
        assert out["state"][j] == INV and np.all(out["state"][good] == RUN), (name, j, i)
        assert np.all(np.isnan(out["x"][j, :r])) and not out["x"][j, r:].any() and np.isnan(out["dec"][j]), (name, j, i)
        assert out["iters"][j] == 0 and np.all(out["iters"][good] == 1)
        assert out["counts"].tolist() == [K - 1, 0, 0, 1]
        without = step(lo, r, w[good], wr[good], lm[good], lr[good], err[good], tol)
        assert np.array_equal(nbits(out["x"][good]), nbits(base["x"][good])), (name, j, i)
        assert np.array_equal(nbits(out["dec"][good]), nbits(base["dec"][good])), (name, j, i)
        assert np.array_equal(nbits(out["x"][good]), nbits(without["x"])), (name, j, i)
        assert np.array_equal(nbits(out["dec"][good]), nbits(without["dec"])), (name, j, i)
    # without err there is no test (and nothing of err to be NaN); lmbd_r NULL = zeros
    assert np.array_equal(nbits(step(lo, r, w, wr, lm, lr)["x"]), nbits(base["x"]))
    a, b = step(lo, r, w, wr, lm, None), step(lo, r, w, wr, lm, np.zeros(K))
    assert np.array_equal(nbits(a["x"]), nbits(b["x"])) and np.array_equal(nbits(a["dec"]), nbits(b["dec"]))

    # iters accumulates over two calls (the second from the first's prices, through the Python form, in place)
    t_lm = dev(np.where(np.isnan(lm), 0.0, lm))
    st = torch.zeros(K, dtype=torch.int8, device="cuda:0")
    it = torch.zeros(K, dtype=torch.int32, device="cuda:0")
    e2 = err.copy()
    e2[3] = 0.0  # converges at the first call: one QP fewer steps at both
    for n in (1, 2):
        res = lo.price_step_many(w, wr, t_lm, lr, price_type="linear", err=e2, tol=tol, state=st, iters=it, in_place=True)
        assert res["lmbd"] is t_lm and res["state"] is st and res["iters"] is it
        want = np.full(K, n)
        want[3] = 0
        assert it.cpu().numpy().tolist() == want.tolist()
        assert res["counts"].cpu().numpy().tolist() == [K - 1, 1, 0, 0]
    first = step(lo, r, w, wr, np.where(np.isnan(lm), 0.0, lm), lr, e2, tol)
    second = step(lo, r, w, wr, first["x"], lr, e2, tol, state=first["state"], iters=first["iters"])
    assert np.array_equal(nbits(t_lm.cpu().numpy()), nbits(second["x"]))
    out_of_place = lo.price_step_many(w, wr, first["x"], lr, price_type="linear", err=e2, tol=tol, state=dev(first["state"], torch.int8))
    assert np.array_equal(nbits(out_of_place["lmbd"].cpu().numpy()), nbits(second["x"]))
    assert np.array_equal(nbits(out_of_place["dec"].cpu().numpy()), nbits(second["dec"]))


# ------------------------------------------------------------------ 5. extents
OPTIONAL = ("lmbd_r", "err", "dec", "state", "iters", "counts")


def arena(ev, N, k, K, converge):
    w, wr, lm, lr = (a[:K] for a in random_inputs(ev, N if N in (2, 13, 64) else 64, k))
    w, wr, lm = w[:, :N], wr[:, :N], np.concatenate([lm[:, :N], lm[:, 64:64 + N], lm[:, 128:128 + N]], 1) if N == 63 else lm
    gb = Guarded()
    gb.inp("w", w).inp("w_ref", wr).inp("lmbd", lm[:, :k * N]).inp("lmbd_r", lr)
    gb.inp("err", np.full(K, 0.25 if converge else 1.0))
    gb.out("lmbd_next", (K, 3 * N)).out("dec", (K,)).out("state", (K,), torch.int8).out("iters", (K,), torch.int32)
    gb.out("counts", (4,), torch.int64)
    return gb.build()


def guarded_call(lo, gb, K, r, null=(), tol=0.5, eps=EPS, ls=None, ns=None, **over):
    p = {n: (None if n in null else gb.ptr(n)) for n in ("w", "w_ref", "lmbd", "lmbd_r", "err", "lmbd_next", "dec", "state",
                                                         "iters", "counts")}
    p["ctx"] = lo._ctx
    p.update(over)
    rc = lo._lib.lompc_price_step_many(p["ctx"], K, r, eps, p["w"], p["w_ref"], p["lmbd"], r if ls is None else ls,
                                       p["lmbd_r"], p["err"], tol, p["lmbd_next"], 3 * lo.N if ns is None else ns, p["dec"],
                                       p["state"], p["iters"], p["counts"], lo._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("N", [2, 13, 63, 64])
def test_extents(gpu, N, K):
    ev, k = "large", 3
    if N == 63:
        c = PSC.CONSTS[ev]
        lo = LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0)
    else:
        lo = ctx(ev, N)
    r = k * N
    for converge in (False, True):  # every QP steps (iters written) / every QP converges (state written)
        results = {}
        for null in [()] + [(n,) for n in OPTIONAL]:
            gb = arena(ev, N, k, K, converge)
            gb.view("state").zero_()  # (read and written: both start as the caller's zeros)
            gb.view("iters").zero_()
            assert guarded_call(lo, gb, K, r, null) == _lib.LOMPC_OK, null
            gb.check_bands()
            gb.check_inputs()
            gb.check_written("lmbd_next")
            stepped = not converge or "err" in null
            for n in ("dec", "counts"):
                (gb.check_untouched if n in null else gb.check_written)(n)
            if "state" not in null:
                assert gb.np("state").tolist() == [RUN if stepped else CONV] * K
            if "iters" not in null:
                assert gb.np("iters").tolist() == [1 if stepped else 0] * K
            if "counts" not in null:
                assert gb.np("counts").tolist() == ([K, 0, 0, 0] if stepped else [0, K, 0, 0])
            x = gb.np("lmbd_next")
            assert not np.isnan(x).any() and np.all(x >= 0)
            if not stepped:
                assert np.array_equal(nbits(x[:, :r]), nbits(gb.np("lmbd")))
            results[null] = (x, None if "dec" in null else gb.np("dec"))
        full = results[()]
        for null, (x, dec) in results.items():  # the other outputs do not depend on which are asked for
            if null not in (("lmbd_r",), ("err",)):
                assert np.array_equal(nbits(x), nbits(full[0])), null
                assert dec is None or np.array_equal(nbits(dec), nbits(full[1])), null


# ------------------------------------------------------------------ 6. refusals
def test_refusals_write_nothing(gpu):
    ev, N, k, K = "small", 13, 2, 5
    lo, r = ctx(ev, N), 2 * 13
    gb = arena(ev, N, k, K, False)
    outs = ("lmbd_next", "dec", "state", "iters", "counts")
    refused = [dict(K=-1), dict(ctx=None), dict(w=None), dict(w_ref=None), dict(lmbd=None), dict(lmbd_next=None),
               dict(r=N), dict(r=0), dict(r=3 * N + 1), dict(r=-2 * N), dict(eps=0.0), dict(eps=-1e-2), dict(eps=np.nan),
               dict(ls=r - 1), dict(ls=0), dict(ls=-r), dict(ns=3 * N - 1), dict(ns=r), dict(ns=-3 * N),
               # overlaps that are not exactly in place: another start, the same start with other strides
               dict(lmbd_next=gb.ptr("lmbd", 1)), dict(lmbd_next=gb.ptr("lmbd", K * r - 1)), dict(lmbd_next=gb.ptr("lmbd")),
               dict(lmbd_next=gb.ptr("lmbd"), ls=3 * N + 1, ns=3 * N),
               dict(lmbd=gb.ptr("lmbd_next", 3 * N * K - 1)), dict(lmbd=gb.ptr("lmbd_next", 5), ls=3 * N, ns=3 * N)]
    for kw in refused:
        rc = guarded_call(lo, gb, kw.pop("K", K), kw.pop("r", r), **kw)
        assert rc == _lib.LOMPC_ERR_INVALID_ARG, kw
        gb.check_bands()
        gb.check_inputs()
        for n in outs:
            gb.check_untouched(n)
    assert guarded_call(lo, gb, 0, r) == _lib.LOMPC_OK  # K = 0: nothing but the zeroed counts
    gb.check_bands()
    for n in outs[:-1]:
        gb.check_untouched(n)
    assert gb.np("counts").tolist() == [0, 0, 0, 0]
    assert guarded_call(lo, gb, 0, r, null=("counts",)) == _lib.LOMPC_OK
    res = lo.price_step_many(np.zeros((0, N)), np.zeros((0, N)), np.zeros((0, 3 * N)), None, price_type="linear")
    assert res["lmbd"].shape == (0, 3 * N) and res["counts"].cpu().numpy().tolist() == [0, 0, 0, 0]
    z = np.zeros((4, N))
    with pytest.raises(ValueError):
        lo.price_step_many(z, z, np.zeros((4, 3 * N)), None, price_type="convex")
    with pytest.raises(ValueError):
        lo.price_step_many(z, z, np.zeros((4, 3 * N + 1)), None, price_type="linear")
    with pytest.raises(ValueError):
        lo.price_step_many(z, z, np.zeros((4, 3 * N)), None, price_type="linear", in_place=True)  # not a device tensor
    with pytest.raises(ValueError):
        lo.price_step_many(z, z, dev(np.zeros((4, 2 * N))), None, price_type="linear", in_place=True)  # (K, 3N) needed
    with pytest.raises(ValueError):
        lo.price_step_many(z, z, np.zeros((4, 3 * N)), np.zeros(3), price_type="linear")
    # in place through the C ABI, exactly: allowed
    gb = arena(ev, N, 3, K, False)
    assert guarded_call(lo, gb, K, 3 * N, null=("state", "iters"), lmbd_next=gb.ptr("lmbd")) == _lib.LOMPC_OK
    gb.check_bands()
    gb.check_untouched("lmbd_next")


# ------------------------------------------------------------------ 7. the loops
EDGE = 1e-6  # scripts/check_price_loop_seeds.py
CAP = 60
LOOPS = [(cn, N, k) for cn in ("small", "large") for N in (5, 13) for k in (2, 3)]


@functools.lru_cache(maxsize=None)
def loop_inputs(cname, N, k):
    c = PSC.CONSTS[cname]
    rng = np.random.default_rng(1)
    g, wr, lr = [], [], []
    for j in range(9):
        g.append(c.y_max * (0.3 + 0.6 * rng.random()))
        wr.append(c.w_max * (0.2 + 0.6 * rng.random(N)))
        lr.append(0.0 if j % 2 == 0 else 1.5 * N * c.delta * rng.random())
    return np.array(g), np.array(wr), np.array(lr)


def oracle_loop(c, N, r, gamma, w_ref, lr, start, cap):
    """price_oracle.OraclePriceSolver.compute_optimal_prices:166-185 for a population of ONE EV (y0_rng = 0, gamma_sc =
    gamma: the batch is the central QP), without the LP: (prices (3N,), w_k, steps, converged, error / tol ratios)."""
    lompc = O.OracleLoMPC(N, c)
    m = lompc.get_sc_modulus()
    tol, _ = O.get_robustness_bounds(N, c.delta, 0.0, lr)
    A_bar, A_bar_inv = O.w_inner_product_metric(lompc.get_input_mat(), c.delta, lr)
    lmbd_k = np.zeros(3 * N)
    lmbd_k[:r] = start
    w_k, _ = lompc.solve_lompc(lmbd_k, lr, gamma)
    ratios, steps, conv = [], 0, False
    for _ in range(cap):
        w_err = np.sqrt((w_k - w_ref) @ A_bar @ (w_k - w_ref))
        ratios.append(w_err / tol)
        if w_err <= tol:
            conv = True
            break
        lmbd_new = np.zeros(3 * N)
        lmbd_new[:r], _ = PO.price_step(N, r, c.theta, c.w_max, m, A_bar_inv, w_ref, w_k, lmbd_k[:r])
        w_k, _ = lompc.solve_lompc(lmbd_new, lr, gamma)
        lmbd_k = lmbd_new
        steps += 1
    return lmbd_k, w_k, steps, conv, np.array(ratios)


@functools.lru_cache(maxsize=None)
def oracle_loops(cname, N, k, cap, started):
    c, r = PSC.CONSTS[cname], k * N
    g, wr, lr = loop_inputs(cname, N, k)
    start = loop_start(cname, N, k) if started else np.zeros((9, r))
    return [oracle_loop(c, N, r, g[j], wr[j], lr[j], start[j], cap) for j in range(9)]


def loop_start(cname, N, k):
    c = PSC.CONSTS[cname]
    return c.theta * np.random.default_rng(2).random((9, k * N))


def check_loops(cname, N, k, cap, started):
    c, r = PSC.CONSTS[cname], k * N
    g, wr, lr = loop_inputs(cname, N, k)
    ref = oracle_loops(cname, N, k, cap, started)
    near = 1.0
    for lm_o, w_o, steps, conv, ratio in ref:  # the condition: no loop on a knife-edge of its test
        before = ratio[:-1] if conv else ratio
        assert (before.size == 0 or before.min() > 1.0 + EDGE) and (not conv or ratio[-1] <= 1.0 - EDGE)
        near = min(near, float(np.min(np.abs(ratio - 1.0))))
    res = personal_prices(ctx(cname, N), "linear" if k == 2 else "linear-convex", g, wr, lr,
                          lmbd0=loop_start(cname, N, k) if started else None, max_iter=cap)
    torch.cuda.synchronize()
    lm, w, state, iters = (res[n].cpu().numpy() for n in ("lmbd", "w", "state", "iters"))
    steps_o = [x[2] for x in ref]
    print(f"{cname} N{N} r{k}N cap {cap}: oracle steps {steps_o}, device {iters.tolist()}, states {state.tolist()}, "
          f"closest |e/tol - 1| {near:.2e}")
    assert iters.tolist() == steps_o
    assert state.tolist() == [CONV if x[3] else RUN for x in ref]
    assert res["solves"] == max(steps_o) + 1
    assert lm.shape == (9, 3 * N) and not lm[:, r:].any() and np.all(lm >= 0)
    for j, (lm_o, w_o, _, _, _) in enumerate(ref):
        dl = np.abs(lm[j] - lm_o) / np.maximum(c.theta, np.abs(lm_o))
        assert share("loop prices", float(dl.max()), 1e-6) <= 1.0, (j, float(dl.max()))
        assert share("loop w vs oracle", float(np.abs(w[j] - w_o).max()), 1e-6) <= 1.0, j
        w_c, _, nf = oracle_c.solve_batch(N, c, lm[j], lr[j], g[j:j + 1])
        assert nf == 0
        assert share("loop w at own prices", float(np.abs(w[j] - w_c[0]).max()), 1e-9) <= 1.0, j
    report()
    return ref


@pytest.mark.parametrize("cname,N,k", LOOPS, ids=[f"{cn}-N{N}-r{k}N" for cn, N, k in LOOPS])
def test_personal_prices(gpu, cname, N, k):
    ref = check_loops(cname, N, k, CAP, False)
    conv = [x[2] for x in ref if x[3]]
    assert conv and len(conv) < 9 and 7 <= min(conv) and max(conv) <= 54, [(x[2], x[3]) for x in ref]


def test_personal_prices_from_given_prices(gpu):
    ref = check_loops("large", 13, 3, 3, True)
    assert all(x[2] == 3 and not x[3] for x in ref)  # every loop stopped by the cap
