"""lompc_solve_many / LoMPC.solve_many: K unrelated QPs, each with its own (lmbd, lmbd_r, gamma), in one launch.

Reference: oracle_c.solve_batch per QP (one price vector, one gamma each) and the 50-digit goldens.  Bars, the
project's own (test_gpu_parity.py): |dw| <= 1e-9, cost within 1e-9 relative, w0 = w[:, 0] bit for bit, price0
within 1e-9 max(1, |p|) of OracleLoMPC.get_price0, every status OK or REPAIRED, counts = the tally of status.

Input family (seeded): lmbd ~ theta U[0,1]^{3N}; lmbd_r = 0 for about half of the QPs and 3 N delta U otherwise;
gamma ~ y_max U with gamma_0 = 0 and gamma_1 = y_max; QP 2 with lmbd = 0; QP 3 with lmbd2 = 0.  K = 257 (64 full
workgroups of four waves plus one wave), N in {1, 2, 12, 13, 24, 48, 63, 64}: one stage, odd horizons, the
common ones, one idle lane and none.  The oracle of a family is computed once and shared.
"""
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

import lompc_oracle as O
import oracle_c
from conftest import oracle_consts
from guarded import Guarded
from lompc_amd import LoMPC, LoMPCConstants, SolverError, _lib

# (the shared inputs are read-only arrays; torch says so once when it copies one to the device)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

TOL = 1e-9
K0 = 257
NS = [1, 2, 12, 13, 24, 48, 63, 64]
EVS = ("small", "large")
F64 = ("w", "cost", "w0", "price0", "err")
OUTS = F64 + ("status",)
OKS = (_lib.LOMPC_QP_OK, _lib.LOMPC_QP_REPAIRED)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "incentive-design-mpc_amd", "csrc")
with open(os.path.join(CSRC, "lompc_many.hip")) as _f:
    MANY_CHUNK = 1 << int(re.search(r"#define MANY_CHUNK \(1ll << (\d+)\)", _f.read()).group(1))


def consts(ev):
    return O.small_consts() if ev == "small" else O.large_consts()


@functools.lru_cache(maxsize=None)
def ctx(ev, N, mode="path"):
    c = consts(ev)
    return LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0, mode=mode)


@functools.lru_cache(maxsize=None)
def problem(ev, N, moved=False):
    """(lmbd (K0, 3N), lmbd_r, gamma, w_ref) of the family; moved: every price scaled by 1 + 0.01 U."""
    c = consts(ev)
    rng = np.random.default_rng(4000 + 2 * N + (ev == "large"))
    lm = c.theta * rng.random((K0, 3 * N))
    lr = np.where(rng.random(K0) < 0.5, 0.0, 3 * N * c.delta * rng.random(K0))
    g = c.y_max * rng.random(K0)
    g[0], g[1] = 0.0, c.y_max
    lm[2] = 0.0
    lm[3, N:2 * N] = 0.0
    wr = c.w_max * rng.random((K0, N))
    if moved:
        lm = lm * (1.0 + 0.01 * rng.random(lm.shape))
    for a in (lm, lr, g, wr):
        a.setflags(write=False)
    return lm, lr, g, wr


@functools.lru_cache(maxsize=None)
def oracle(ev, N, moved=False):
    """(w, cost, price0) of every QP of the family, each from its own oracle solve."""
    c = consts(ev)
    lm, lr, g, _ = problem(ev, N, moved)
    o = O.OracleLoMPC(N, c)
    w, cost, p0 = np.empty((K0, N)), np.empty(K0), np.empty(K0)
    for k in range(K0):
        wk, ck, nf = oracle_c.solve_batch(N, c, lm[k], lr[k], g[k:k + 1])
        assert nf == 0, f"the oracle failed on QP {k} ({ev}, N = {N})"
        w[k], cost[k] = wk[0], ck[0]
        p0[k] = o.get_price0(w[k], lm[k], lr[k])
    for a in (w, cost, p0):
        a.setflags(write=False)
    return w, cost, p0


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def raw(lo, lm, lr, g, wr=None, ws=None, flags=0, stride=None, want=OUTS, counts=True):
    """One lompc_solve_many through the C ABI on fresh buffers; ws: a uint8 device tensor, used in place."""
    K, N = len(g), lo.N
    if stride is None:
        stride = 0 if np.ndim(lm) == 1 else np.shape(lm)[1]
    t = {"lm": dev(lm), "lr": dev(lr), "g": dev(g), "wr": dev(wr)}
    want = [n for n in want if n != "err" or wr is not None]
    out = {n: torch.empty((K, N) if n == "w" else (K,), dtype=torch.int8 if n == "status" else torch.float64,
                          device="cuda:0") for n in want}
    if counts:
        out["counts"] = torch.full((4,), -7, dtype=torch.int64, device="cuda:0")
    rc = lo._lib.lompc_solve_many(lo._ctx, K, ptr(t["lm"]), stride, ptr(t["lr"]), ptr(t["g"]), ptr(t["wr"]), ptr(ws),
                                  flags, *[ptr(out.get(n)) for n in OUTS], ptr(out.get("counts")), lo._stream())
    assert rc == _lib.LOMPC_OK, _lib.status_text(lo._lib, lo._ctx, rc)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(got, base, idx=None, names=OUTS):
    for n in names:
        if n in got:
            ref = base[n] if idx is None else base[n][torch.as_tensor(idx, device=base[n].device)]
            assert torch.equal(bits(got[n]), bits(ref)), n


def in_bars(out, ref):
    w_o, c_o, p_o = ref
    w = out["w"].cpu().numpy()
    dw = np.abs(w - w_o).max()
    print(f"max |dw| = {dw:.3e}")
    assert dw <= TOL
    if "cost" in out:
        cost = out["cost"].cpu().numpy()
        dc = np.max(np.abs(cost - c_o) / np.maximum(1.0, np.abs(c_o)))
        print(f"max cost error (relative) = {dc:.3e}")
        assert np.all(np.abs(cost - c_o) <= TOL * np.maximum(1.0, np.abs(c_o)))
    if "w0" in out:
        assert torch.equal(bits(out["w0"]), bits(out["w"][:, 0].contiguous()))
    if "price0" in out:
        p = out["price0"].cpu().numpy()
        assert np.all(np.abs(p - p_o) <= TOL * np.maximum(1.0, np.abs(p_o))), np.max(np.abs(p - p_o))
    if "status" in out:
        st = out["status"].cpu().numpy()
        assert np.all(np.isin(st, OKS)), np.bincount(st, minlength=4)
        if "counts" in out:
            assert out["counts"].cpu().numpy().tolist() == np.bincount(st, minlength=4).tolist()


# ------------------------------------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("ev", EVS)
def test_oracle_parity_every_qp(gpu, ev, N):
    lm, lr, g, _ = problem(ev, N)
    res = ctx(ev, N).solve_many(lm, lr, g, want_w0=True, want_price0=True, want_status=True)
    assert res["w"].shape == (K0, N) and res["counts"].shape == (4,)
    in_bars(res, oracle(ev, N))


# ------------------------------------------------------------------------------------------------ 2. goldens
def test_goldens_one_call_per_group(gpu, golden):
    groups = {}
    for c in golden:
        groups.setdefault((c["ev_type"], c["N"]), []).append(c)
    for (ev, N), cases in groups.items():
        c0 = oracle_consts(cases[0])
        assert all(oracle_consts(c) == c0 for c in cases)
        lo = LoMPC(N, LoMPCConstants(c0.delta, c0.theta, c0.y_max, c0.w_max, c0.ev_type), device=0)
        n = [len(c["gamma"]) for c in cases]
        lm = np.concatenate([np.repeat(c["lmbd"][None], k, 0) for c, k in zip(cases, n)])
        lr = np.concatenate([np.full(k, c["lmbd_r"]) for c, k in zip(cases, n)])
        wr = np.concatenate([np.repeat(c["w_ref"][None], k, 0) for c, k in zip(cases, n)])
        g = np.concatenate([c["gamma"] for c in cases])
        res = lo.solve_many(lm, lr, g, w_ref=wr, want_status=True)
        w, cost, err = (res[k].cpu().numpy() for k in ("w", "cost", "err"))
        ref_w, ref_c = np.concatenate([c["w"] for c in cases]), np.concatenate([c["cost"] for c in cases])
        assert np.abs(w - ref_w).max() <= TOL, (ev, N)
        assert np.all(np.abs(cost - ref_c) <= TOL * np.maximum(1.0, np.abs(ref_c))), (ev, N)
        assert np.all(np.isin(res["status"].cpu().numpy(), OKS))
        at = np.concatenate([[0], np.cumsum(n)])
        for c, a, b in zip(cases, at[:-1], at[1:]):
            assert abs(err[a:b].max() - c["w_err_max"]) <= TOL, c["id"]


# -------------------------------------------------------------- 3. placement and batch-size independence
@pytest.mark.parametrize("N", [13, 48])
@pytest.mark.parametrize("ev", EVS)
def test_bits_do_not_depend_on_placement(gpu, ev, N):
    lo = ctx(ev, N)
    lm, lr, g, wr = problem(ev, N)
    base = raw(lo, lm, lr, g, wr)
    in_bars(base, oracle(ev, N))
    same_bits(raw(lo, lm, lr, g, wr), base)  # the same call twice
    subsets = [[0], [3], [4], [255], [256], [0, 1, 2], [0, 1, 2, 3], [0, 1, 2, 3, 4], [252, 253, 254, 255, 256],
               list(range(K0 - 1, -1, -1))]
    for idx in subsets:
        same_bits(raw(lo, lm[idx], lr[idx], g[idx], wr[idx]), base, idx)
    pad = np.full((K0, 3 * N + 5), np.nan)  # padded rows: the padding is never read
    pad[:, :3 * N] = lm
    same_bits(raw(lo, pad, lr, g, wr), base)
    shared = raw(lo, lm[7], lr, g, wr)  # one shared vector through stride 0
    assert shared["w"].shape == (K0, N)
    same_bits(shared, raw(lo, np.repeat(lm[7][None], K0, 0), lr, g, wr))
    same_bits(raw(lo, lm, None, g, wr), raw(lo, lm, np.zeros(K0), g, wr))  # lmbd_r NULL = 0


# --------------------------------------------------------------------------------------------- 4. warm start
@pytest.mark.parametrize("N", [13, 48])
@pytest.mark.parametrize("ev", EVS)
def test_warm_start(gpu, ev, N):
    lo = ctx(ev, N)
    m2 = 2 * (1 if ev == "small" else 4)
    lm, lr, g, _ = problem(ev, N)
    ws = torch.full((K0, 64), 0x5A, dtype=torch.uint8, device="cuda:0")
    cold0 = raw(lo, lm, lr, g, ws=ws)
    in_bars(cold0, oracle(ev, N))
    same_bits(cold0, raw(lo, lm, lr, g))  # writing ws changes nothing else
    s = ws.cpu().numpy()
    assert s[:, :N].max() <= m2 and np.all(s[:, N:] == 0)
    lm2 = problem(ev, N, moved=True)[0]
    ws_warm = ws.clone()
    warm = raw(lo, lm2, lr, g, ws=ws_warm, flags=_lib.LOMPC_MANY_WARM)
    cold = raw(lo, lm2, lr, g, ws=ws)
    for r in (warm, cold):
        in_bars(r, oracle(ev, N, True))
    assert (warm["w"] - cold["w"]).abs().max().item() <= TOL
    s = ws_warm.cpu().numpy()
    assert s[:, :N].max() <= m2 and np.all(s[:, N:] == 0)
    junk = torch.full((K0, 64), 0xFF, dtype=torch.uint8, device="cuda:0")  # clamped to 2m
    in_bars(raw(lo, lm2, lr, g, ws=junk, flags=_lib.LOMPC_MANY_WARM), oracle(ev, N, True))
    s = junk.cpu().numpy()
    assert s[:, :N].max() <= m2 and np.all(s[:, N:] == 0)
    res = lo.solve_many(lm2, lr, g, ws=ws_warm, warm=True, want_status=True)  # the Python form
    assert res["ws"] is ws_warm and torch.equal(bits(res["w"]), bits(warm["w"]))


# -------------------------------------------------------------------------------------- 5. per-QP invalidity
def bad_batch(ev, N):
    c = consts(ev)
    lm, lr, g, wr = (a.copy() for a in problem(ev, N))
    g[5] = -1e-3
    g[6] = c.y_max * (1 + 1e-12)
    g[64] = np.nan
    lm[65, 4 % (3 * N)] = -1e-6
    lm[130, 3 * N - 1] = np.nan
    lr[256] = -1.0
    return lm, lr, g, wr, [5, 6, 64, 65, 130, 256]


@pytest.mark.parametrize("ev", EVS)
def test_invalid_qps_are_their_own(gpu, ev):
    N = 13
    lo = ctx(ev, N)
    lm, lr, g, wr, bad = bad_batch(ev, N)
    out = raw(lo, lm, lr, g, wr)
    good = np.setdiff1d(np.arange(K0), bad)
    st = out["status"].cpu().numpy()
    assert np.all(st[bad] == _lib.LOMPC_QP_INVALID) and np.all(np.isin(st[good], OKS))
    for n in F64:
        a = out[n].cpu().numpy()
        assert np.all(np.isnan(a[bad])) and not np.any(np.isnan(a[good])), n
    assert out["counts"].cpu().numpy().tolist() == np.bincount(st, minlength=4).tolist()
    assert out["counts"][_lib.LOMPC_QP_INVALID].item() == len(bad)
    same_bits(raw(lo, lm[good], lr[good], g[good], wr[good]), out, good)  # the neighbours: as without them
    same_bits(raw(lo, *(a[good] for a in problem(ev, N))), out, good)


@pytest.mark.parametrize("tensors", [False, True])
def test_check_raises_the_references_types(gpu, tensors):
    ev, N = "large", 13
    lo, c = ctx(ev, N), consts(ev)
    base = problem(ev, N)
    cv = (lambda a: dev(a)) if tensors else (lambda a: a)

    def run(check=True, **edit):
        lm, lr, g = (a.copy() for a in base[:3])
        for name, (i, v) in edit.items():
            {"lm": lm, "lr": lr, "g": g}[name][i] = v
        return lo.solve_many(cv(lm), cv(lr), cv(g), want_status=True, check=check)

    with pytest.raises(AssertionError):
        run(g=(6, c.y_max * (1 + 1e-12)))
    with pytest.raises(AssertionError):  # the reference asserts gamma <= y_max before cvxpy sees a parameter
        run(g=(6, c.y_max + 0.1), lr=(9, -1.0))
    for edit in ({"g": (5, -1e-3)}, {"g": (64, np.nan)}, {"lm": ((65, 4), -1e-6)}, {"lm": ((130, 3 * N - 1), np.nan)},
                 {"lr": (256, -1.0)}):
        with pytest.raises(ValueError):
            run(**edit)
    res = run(check=False, g=(6, c.y_max + 0.1), lr=(9, -1.0))
    assert res["counts"].cpu().numpy()[_lib.LOMPC_QP_INVALID] == 2
    assert res["status"].cpu().numpy()[[6, 9]].tolist() == [_lib.LOMPC_QP_INVALID] * 2
    assert issubclass(SolverError, Exception)


# ------------------------------------------------------------------------------------------------ 6. extents
def arena(ev, N, K, misalign=False):
    lm, lr, g, wr = (a[:K] for a in problem(ev, N))
    gb = Guarded(misalign=misalign)
    gb.inp("lmbd", lm).inp("lmbd_r", lr).inp("gamma", g).inp("w_ref", wr)
    for n in F64:
        gb.out(n, (K, N) if n == "w" else (K,))
    gb.out("status", (K,), torch.int8).out("ws", (K, 64), torch.int8).out("counts", (4,), torch.int64)
    return gb.build()


def guarded_call(lo, gb, K, want, ws=True, counts=True, flags=0, stride=None, **over):
    a = {"ctx": lo._ctx, "K": K, "lmbd": gb.ptr("lmbd"), "stride": 3 * lo.N if stride is None else stride,
         "lmbd_r": gb.ptr("lmbd_r"), "gamma": gb.ptr("gamma"), "w_ref": gb.ptr("w_ref")}
    a.update(over)
    rc = lo._lib.lompc_solve_many(a["ctx"], a["K"], a["lmbd"], a["stride"], a["lmbd_r"], a["gamma"], a["w_ref"],
                                  gb.ptr("ws") if ws else None, flags, *[gb.ptr(n) if n in want else None for n in OUTS],
                                  gb.ptr("counts") if counts else None, lo._stream())
    torch.cuda.synchronize()
    return rc


def check_extents(gb, want, ws=True, counts=True):
    gb.check_bands()
    gb.check_inputs()
    for n in OUTS + ("ws", "counts"):
        given = {"ws": ws, "counts": counts}.get(n, n in want)
        (gb.check_written if given else gb.check_untouched)(n)


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("N", [1, 13, 64])
def test_extents_full_set(gpu, N, K, misalign):
    for ev in EVS:
        lo = ctx(ev, N)
        gb = arena(ev, N, K, misalign)
        assert guarded_call(lo, gb, K, OUTS) == _lib.LOMPC_OK
        check_extents(gb, OUTS)
        out = {n: gb.view(n) for n in OUTS + ("counts",)}
        in_bars(out, tuple(a[:K] for a in oracle(ev, N)))
        s = gb.np("ws")
        assert s[:, :N].min() >= 0 and s[:, :N].max() <= 8 and np.all(s[:, N:] == 0)


def test_extents_every_subset_of_null_outputs(gpu):
    ev, N, K = "large", 13, 5
    lo = ctx(ev, N)
    full = arena(ev, N, K)
    assert guarded_call(lo, full, K, OUTS) == _lib.LOMPC_OK
    base = {n: full.view(n) for n in OUTS + ("ws", "counts")}
    for r in range(len(OUTS) + 1):
        for want in itertools.combinations(OUTS, r):
            for aux in ((True, True), (False, False)) if r in (0, len(OUTS)) else ((True, True),):
                gb = arena(ev, N, K)
                assert guarded_call(lo, gb, K, want, ws=aux[0], counts=aux[1]) == _lib.LOMPC_OK, want
                check_extents(gb, want, *aux)
                same_bits({n: gb.view(n) for n in want + (("ws", "counts") if aux[0] else ())}, base,
                          names=OUTS + ("ws", "counts"))


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing(gpu):
    ev, N, K = "small", 13, 5
    lo = ctx(ev, N)
    gb = arena(ev, N, K)
    W = _lib.LOMPC_MANY_WARM
    refused = [dict(K=-1), dict(ctx=None), dict(lmbd=None), dict(gamma=None), dict(stride=1), dict(stride=3 * N - 1),
               dict(stride=-3 * N), dict(flags=2), dict(flags=W | 2), dict(flags=-1), dict(flags=W, ws=False),
               dict(w_ref=None)]
    for kw in refused:
        assert guarded_call(lo, gb, kw.pop("K", K), OUTS, **kw) == _lib.LOMPC_ERR_INVALID_ARG, kw
        gb.check_bands()
        gb.check_inputs()
        for n in OUTS + ("ws", "counts"):
            gb.check_untouched(n)
    assert guarded_call(lo, gb, K, [n for n in OUTS if n != "err"], w_ref=None) == _lib.LOMPC_OK  # err is what needs w_ref
    gb = arena(ev, N, K)
    assert guarded_call(lo, gb, 0, OUTS) == _lib.LOMPC_OK  # K = 0: nothing but the zeroed counts
    gb.check_bands()
    for n in OUTS + ("ws",):
        gb.check_untouched(n)
    assert gb.np("counts").tolist() == [0, 0, 0, 0]
    assert guarded_call(lo, gb, 0, OUTS, counts=False) == _lib.LOMPC_OK
    res = lo.solve_many(np.zeros((0, 3 * N)), np.zeros(0), np.zeros(0), want_status=True)
    assert res["w"].shape == (0, N) and res["counts"].cpu().numpy().tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        lo.solve_many(np.zeros((4, 3 * N)), 0.0, np.zeros(4), warm=True)
    with pytest.raises(ValueError):
        lo.solve_many(np.zeros((4, 3 * N + 1)), 0.0, np.zeros(4))
    with pytest.raises(ValueError):
        lo.solve_many(np.zeros((4, 3 * N)), np.zeros(3), np.zeros(4))


# ------------------------------------------------------------------------------------- 8. context untouched
@pytest.mark.parametrize("mode", ["path", "direct"])
def test_context_state_is_untouched(gpu, mode):
    ev, N = "large", 24
    c = consts(ev)
    lo = LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0, mode=mode)
    rng = np.random.default_rng(81)
    S, per = 2, 200
    off = np.arange(S + 1, dtype=np.int64) * per
    gb = c.y_max * rng.random(S * per)
    lo.set_params(c.theta * rng.random((S, 3 * N)), np.array([0.0, 0.3]), w_ref=c.w_max * rng.random((S, N)),
                  gamma_ref=np.full(S, 0.5 * c.y_max))
    r1 = {k: v.clone() for k, v in lo.solve_batch(gb, off, want_w0=True, want_status=True).items()}
    lm, lr, g, wr, bad = bad_batch(ev, N)
    many = lo.solve_many(lm, lr, g, w_ref=wr, want_status=True, check=False)  # invalid QPs: a tally of its own
    assert many["counts"][_lib.LOMPC_QP_INVALID].item() == len(bad) and lo.S == S and lo.mode == mode
    r2 = lo.solve_batch(gb, off, want_w0=True, want_status=True, check=False)
    for k in ("w", "cost", "w0", "status", "set_sum_w", "set_stats"):
        assert torch.equal(bits(r1[k]), bits(r2[k])), k
    rep, fail, inv = lo.check_last()  # the second batch's: nothing of solve_many's invalid QPs
    assert (rep, fail, inv) == (int((r2["status"] == _lib.LOMPC_QP_REPAIRED).sum()), 0, 0)
    good = np.setdiff1d(np.arange(K0), bad)
    same_bits({"w": many["w"][torch.as_tensor(good, device="cuda:0")]}, raw(ctx(ev, N), lm, lr, g, wr), good)


# ---------------------------------------------------------------------------- more than one launch per call
def test_batch_past_one_launch(gpu):
    """K just past the QPs of one launch (MANY_CHUNK): the second launch's offset and the 64-bit indices.  N = 1,
    one shared price vector, no lmbd_r: the large arrays are gamma, w0 and status."""
    ev, N = "small", 1
    lo, c = ctx(ev, N), consts(ev)
    K = MANY_CHUNK + 5
    lm = problem(ev, N)[0][7]
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    g = c.y_max * torch.rand(K, dtype=torch.float64, device="cuda:0", generator=gen)
    res = lo.solve_many(lm, 0.0, g, want_w=False, want_cost=False, want_w0=True, want_status=True)
    assert res["counts"].cpu().numpy().tolist() == [K, 0, 0, 0] and int(res["status"].max()) == _lib.LOMPC_QP_OK
    idx = torch.cat([torch.arange(6), torch.arange(MANY_CHUNK - 3, K)]).to("cuda:0")
    few = lo.solve_many(lm, 0.0, g[idx], want_w=False, want_cost=False, want_w0=True)
    assert torch.equal(bits(res["w0"][idx]), bits(few["w0"]))
    w_o, _, nf = oracle_c.solve_batch(N, c, lm, 0.0, g[idx].cpu().numpy())
    assert nf == 0 and np.abs(few["w0"].cpu().numpy() - w_o[:, 0]).max() <= TOL
