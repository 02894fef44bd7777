"""The scalar pass (LOMPC_PLAN_SCALAR_PASS, k_scalar): per-EV w0 / cost / status and set_stats of a
lompc_plan_run that asks for no w row and no per-stage sum, evaluated from the path table's coefficient
records alone.

Every buffer the C ABI sees comes from tests/guarded.py (outputs pre-filled with a pattern between bands of
it); the calls are raw lompc_plan_run calls, so NULL outputs are NULL.  What every scalar run is checked for
(`check`):

  * the bands untouched, the inputs unchanged, every requested output written to its last element;
  * per EV, against oracle_c.solve_batch over EVERY EV: |dw0| <= 1e-9, cost 1e-9 relative (the project's
    bars); status OK or REPAIRED (INVALID, with NaN outputs, exactly where gamma is invalid);
  * per EV, against an UNFLAGGED plan over the same gamma / w_ref buffers called with the same NULLs:
    cost, w0 and status bit for bit;
  * set_stats: COUNT, N_REPAIRED, N_FAILED, N_INVALID exact (N_REPAIRED / N_INVALID from the per-EV
    status); SUM_W0, SUM_PRICE0, SUM_COST against the sums of the pass's own per-EV outputs at 1e-9 + 1e-11
    |ref| and against the oracle's at 1e-9 + 1e-10 |ref| (test_gpu_extents.py's bars); MAX_ERR within 1e-9
    of the unflagged plan's;
  * a second run of the same plan gives the same bits;
  * which kernel ran: one K_SCALAR and no K_EVAL launch.

Shapes: test_gpu_plan_horizons.Batch (both EV types, the ragged sets [0, 1, 63, 65, 1100]) in
test_gpu_extents.py's rotations (shared, cached batches: one oracle each), and one-type batches where the
issue asks for them.  Launch counts come from the plan's HIP-event profile (BatchPlan.ALL_KERNELS).
"""
import functools

import numpy as np
import pytest
import torch

import price_families as PF
from guarded import Guarded
from lompc_amd import BatchPlan, _lib
from test_gpu_extents import ROT, batch
from test_gpu_plan_horizons import Batch, Dev, contexts

pytestmark = pytest.mark.gpu

ST = _lib
NS = [1, 2, 13, 24, 48, 63, 64]
PER_EV = ("cost", "w0", "status")
ALLK = BatchPlan.ALL_KERNELS


def one_type(N, sizes, seed, t=0, gamma=None, K=1):
    """A batch of one EV type (t: 0 small, 1 large) with Batch's interface: sets `sizes`, gamma uniform over
    [0, y_max] (gamma(c, m, rng): the set's own), prices theta * rand, lmbd_r > 0 on every other set."""
    cs, lompcs = contexts(N)
    bt = Batch.__new__(Batch)
    bt.N, bt.K, bt.cs, bt.lompcs, bt.P = N, K, (cs[t],), [lompcs[t]], len(sizes)
    bt.rng = rng = np.random.default_rng(seed)
    c = cs[t]
    parts = [gamma(c, m, rng) if gamma else c.y_max * rng.random(m) for m in sizes]
    lm = c.theta * rng.random((K, len(sizes), 3 * N))
    lr = 0.2 * rng.random((K, len(sizes))) * (np.arange(len(sizes)) % 2)
    bt.take(parts, lm, lr, device=False)
    return bt


def arena(bt, want=PER_EV, stats=True, misalign=False, extra_out=()):
    """Guarded inputs (gamma, every run's prices, w_ref) and the requested outputs of one scalar run."""
    gb = Guarded(misalign=misalign)
    gb.inp("gamma", bt.gn).inp("lmbd", bt.lm).inp("lmbd_r", bt.lr).inp("w_ref", bt.wr)
    outputs(gb, bt, want, stats, extra_out)
    return gb.build()


def outputs(gb, bt, want, stats, extra_out=()):
    for n in want:
        gb.out(n, (bt.B,), torch.int8 if n == "status" else torch.float64)
    if stats:
        gb.out("set_stats", (bt.S * ST.LOMPC_SET_STATS,))
    for n, shape in extra_out:
        gb.out(n, shape)
    return gb


def make_plan(bt, gb, **kw):
    """A plan over the guarded gamma and w_ref with no outputs of its own."""
    kw.setdefault("validate", False)
    plan = BatchPlan(bt.lompcs, gb.view("gamma"), bt.off, sets_per_ctx=[bt.P] * len(bt.lompcs), w_ref=gb.view("w_ref"),
                     want_w=False, want_cost=False, want_set=False, **kw)
    assert plan.gamma.data_ptr() == gb.ptr("gamma") and plan.w_ref.data_ptr() == gb.ptr("w_ref")
    return plan


def run(plan, gin, gout, k=0, w=None, set_sum_w=None):
    """lompc_plan_run at run k's prices (inputs of arena gin) into arena gout's outputs; the others NULL."""
    S, N = plan.S, plan.N
    rc = plan._lib.lompc_plan_run(plan._plan, gin.ptr("lmbd", k * S * 3 * N), gin.ptr("lmbd_r", k * S), w, gout.ptr("cost"),
                                  gout.ptr("w0"), gout.ptr("status"), set_sum_w, gout.ptr("set_stats"), plan._stream)
    assert rc == 0, plan._lib.lompc_plan_last_error(plan._plan)


def counted(plan, call):
    """Launches per kernel name (ALL_KERNELS) that the plan's profile records over call()."""
    plan.profile(enable=ALLK)
    for k in ALLK:
        plan.profile(read=True, reset=True, kernel=k)
    call()
    n = {k: plan.profile(read=True, reset=True, kernel=k)[1] for k in ALLK}
    plan.profile(enable=False)
    return n


def status_counts(plan):
    """(repaired, failed, invalid) of lompc_plan_status, without BatchPlan.check's exceptions."""
    import ctypes

    r = [ctypes.c_int64(0) for _ in range(3)]
    assert plan._lib.lompc_plan_status(plan._plan, plan._stream, *[ctypes.byref(x) for x in r]) == 0
    return tuple(x.value for x in r)


def price0_of(bt, k, s, w0):
    c, lm, lr, N = bt.consts_of(s), bt.lm[k, s], bt.lr[k, s], bt.N
    q_scale = 3 * c.theta / (4 * c.w_max)
    return c.theta * (w0 * lm[0] + (c.w_max - w0) * lm[N]) + q_scale * w0 ** 2 * lm[2 * N] + c.theta ** 2 * w0 ** 2 * lr


def bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def check(name, bt, k, gb, gu, plan, gn=None, invalid=None, allow_failed=False, oracle_sums=True):
    """The module docstring's checks of one scalar run (outputs in gb) against the oracle at gamma gn (the
    batch's own by default) and the unflagged plan's outputs gu.  invalid: indices of the EVs whose gamma is
    invalid.  allow_failed: EVs may be FAILED where the unflagged plan's are (the oracle bars hold for the
    others).  Returns the per-EV status (or None)."""
    torch.cuda.synchronize()
    gb.check_bands()
    gb.check_inputs()
    gu.check_bands()
    B, S = bt.B, bt.S
    g = bt.gn if gn is None else gn
    inv = np.zeros(B, dtype=bool)
    if invalid is not None:
        inv[invalid] = True
    W, C = bt.oracle(k, np.where(inv, 0.0, g) if (gn is not None or invalid is not None) else None)
    dev = Dev(name)
    has = lambda n: n in gb._at
    out = {}
    for n in PER_EV + ("set_stats",):
        if has(n):
            gb.check_written(n)
            out[n] = gb.np(n)
            assert n in gu._at
            if n != "set_stats":  # bit for bit the default evaluation's
                np.testing.assert_array_equal(bits(out[n]), bits(gu.np(n)), err_msg=f"{name}: {n} vs the unflagged plan")
    status = out.get("status")
    ok = ~inv
    if status is not None:
        assert np.all(status[inv] == ST.LOMPC_QP_INVALID), name
        good = (status == ST.LOMPC_QP_OK) | (status == ST.LOMPC_QP_REPAIRED)
        if not allow_failed:
            assert np.all(good[~inv]), (name, np.unique(status))
        ok = good & ~inv
    for n in ("cost", "w0"):
        if n in out:
            assert np.all(np.isnan(out[n][inv])), name
    if "w0" in out:
        dev.add("|dw0|", np.abs(out["w0"][ok] - W[ok, 0]), 1e-9)
    if "cost" in out:
        dev.add("cost", np.abs(out["cost"][ok] - C[ok]), 1e-9 + 1e-9 * np.abs(C[ok]))
    if "set_stats" in out:
        st, su = out["set_stats"].reshape(S, 8), gu.np("set_stats").reshape(S, 8)
        np.testing.assert_array_equal(st[:, ST.LOMPC_STAT_COUNT], np.diff(bt.off))
        for col in (ST.LOMPC_STAT_N_REPAIRED, ST.LOMPC_STAT_N_FAILED, ST.LOMPC_STAT_N_INVALID):
            np.testing.assert_array_equal(st[:, col], su[:, col], err_msg=f"{name}: counter {col} vs the unflagged plan")
        if not allow_failed:
            assert np.all(st[:, ST.LOMPC_STAT_N_FAILED] == 0), name
        dev.add("MAX_ERR vs unflagged", np.abs(st[:, ST.LOMPC_STAT_MAX_ERR] - su[:, ST.LOMPC_STAT_MAX_ERR]), 1e-9)
        for s in range(S):
            a, b = bt.off[s], bt.off[s + 1]
            m = ok[a:b]
            if status is not None:
                assert st[s, ST.LOMPC_STAT_N_INVALID] == np.sum(status[a:b] == ST.LOMPC_QP_INVALID), (name, s)
                assert st[s, ST.LOMPC_STAT_N_REPAIRED] == np.sum(status[a:b] == ST.LOMPC_QP_REPAIRED), (name, s)
                assert st[s, ST.LOMPC_STAT_N_FAILED] == np.sum(status[a:b] == ST.LOMPC_QP_FAILED), (name, s)
            else:
                assert st[s, ST.LOMPC_STAT_N_INVALID] == np.sum(inv[a:b]), (name, s)
            if allow_failed and st[s, ST.LOMPC_STAT_N_FAILED] > 0:
                continue  # (a failed EV's outputs are in the sums but certified by nothing)
            refs = {"sum w0": (ST.LOMPC_STAT_SUM_W0, W[a:b, 0][m].sum()),
                    "sum price0": (ST.LOMPC_STAT_SUM_PRICE0, price0_of(bt, k, s, W[a:b, 0][m]).sum()),
                    "sum cost": (ST.LOMPC_STAT_SUM_COST, C[a:b][m].sum())}
            for what, (col, ref) in refs.items():
                if oracle_sums:
                    dev.add(what + " vs oracle", abs(st[s, col] - ref), 1e-9 + 1e-10 * abs(ref))
            if "w0" in out:
                own = out["w0"][a:b][m]
                dev.add("sum w0 vs own", abs(st[s, ST.LOMPC_STAT_SUM_W0] - own.sum()), 1e-9 + 1e-11 * abs(own.sum()))
                p0 = price0_of(bt, k, s, own).sum()
                dev.add("sum price0 vs own", abs(st[s, ST.LOMPC_STAT_SUM_PRICE0] - p0), 1e-9 + 1e-11 * abs(p0))
            if "cost" in out:
                own = out["cost"][a:b][m].sum()
                dev.add("sum cost vs own", abs(st[s, ST.LOMPC_STAT_SUM_COST] - own), 1e-9 + 1e-11 * abs(own))
    dev.check()
    # the same bits in a second run
    first = {n: gb.view(n).clone() for n in out}
    run(plan, gb, gb, k)
    torch.cuda.synchronize()
    for n, t in first.items():
        v = gb.view(n)
        same = torch.equal(v.view(torch.int64), t.view(torch.int64)) if v.dtype == torch.float64 else torch.equal(v, t)
        assert same, f"{name}: {n} differs between two runs"
    return status


def scalar_case(name, bt, k=0, want=PER_EV, stats=True, misalign=False, gn=None, invalid=None, allow_failed=False,
                move=None, oracle_sums=True, **kw):
    """One flagged plan's scalar run and the unflagged plan's run over the same gamma / w_ref buffers, both
    with w = set_sum_w = NULL, checked (`check`); asserts the flagged run took k_scalar.  move: applied to
    the arena after both plans exist (gamma rewritten in place).  Returns (status, flagged plan, arena)."""
    gb = arena(bt, want, stats, misalign)
    gu = outputs(Guarded(misalign=misalign), bt, want, stats).build()
    plan = make_plan(bt, gb, scalar_pass=True, **kw)
    ref = make_plan(bt, gb, **kw)
    if move is not None:
        move(gb)
    n = counted(plan, lambda: run(plan, gb, gb, k))
    assert n["k_scalar"] == 1 and n["k_eval"] == 0 and n["k_path"] == 1 and n["k_finalize"] == 1, (name, n)
    run(ref, gb, gu, k)
    status = check(name, bt, k, gb, gu, plan, gn=gn, invalid=invalid, allow_failed=allow_failed, oracle_sums=oracle_sums)
    return status, plan, gb


# ------------------------------------------------------------------------------------------------- 1
def test_scalar_kernel_dispatch(gpu):
    """(1) Which runs take k_scalar: lompc_plan_run of a flagged plan with w = set_sum_w = NULL, and no other
    — with w or with set_sum_w it is k_eval; lompc_plan_run_steps (K = 3) and lompc_plan_run_chain never, and
    their outputs are bitwise an unflagged plan's."""
    N, K = 24, 3
    bt = batch(N)
    B, S = bt.B, bt.S
    extra = (("w", (B, N)), ("set_sum_w", (S * N,)))
    gb = arena(bt, extra_out=extra)
    plan = make_plan(bt, gb, scalar_pass=True)
    n = counted(plan, lambda: run(plan, gb, gb, 1))
    assert (n["k_scalar"], n["k_eval"]) == (1, 0), n
    n = counted(plan, lambda: run(plan, gb, gb, 1, w=gb.ptr("w")))
    assert (n["k_scalar"], n["k_eval"]) == (0, 1), n
    n = counted(plan, lambda: run(plan, gb, gb, 1, set_sum_w=gb.ptr("set_sum_w")))
    assert (n["k_scalar"], n["k_eval"]) == (0, 1), n
    assert plan.check()[1:] == (0, 0)
    # run_steps and run_chain: as an unflagged plan
    wt = np.concatenate([c.w_max * (0.2 + 0.6 * np.random.default_rng(N).random((bt.P, N))) for c in bt.cs])
    res = {}
    for flagged in (True, False):
        g2 = Guarded().inp("gamma", bt.gn).inp("lmbd", bt.lm).inp("lmbd_r", bt.lr).inp("w_ref", bt.wr).inp("w_target", wt)
        for n_ in PER_EV:
            g2.out(n_, (K * B,), torch.int8 if n_ == "status" else torch.float64)
        g2.out("set_sum_w", (K * S * N,)).out("set_stats", (K * S * 8,)).out("lmbd_out", (K, S, 3 * N)).build()
        p2 = make_plan(bt, g2, scalar_pass=flagged)
        lib = p2._lib
        per_ev = [None, g2.ptr("cost"), g2.ptr("w0"), g2.ptr("status")]
        rcs = []
        n = counted(p2, lambda: rcs.append(lib.lompc_plan_run_steps(
            p2._plan, g2.ptr("lmbd"), S * 3 * N, g2.ptr("lmbd_r"), S, K, 0, *per_ev, g2.ptr("set_sum_w"), g2.ptr("set_stats"),
            S * N, 8 * S, B, 0, p2._stream)))
        assert rcs == [0] and n["k_scalar"] == 0 and n["k_eval"] >= 1, (rcs, n)
        steps = {k_: g2.view(k_).clone() for k_ in PER_EV + ("set_stats", "set_sum_w")}
        n = counted(p2, lambda: rcs.append(lib.lompc_plan_run_chain(
            p2._plan, g2.ptr("lmbd"), g2.ptr("lmbd_r"), g2.ptr("w_target"), 0.5, K, g2.ptr("lmbd_out"), *per_ev,
            g2.ptr("set_sum_w"), g2.ptr("set_stats"), p2._stream)))
        assert rcs == [0, 0], rcs
        assert n["k_scalar"] == 0 and n["k_eval"] == K, n
        assert p2.check()[1:] == (0, 0)
        g2.check_bands()
        chain = {k_: g2.view(k_).clone() for k_ in PER_EV + ("set_stats", "set_sum_w", "lmbd_out")}
        res[flagged] = (steps, chain)
    for form in (0, 1):
        for k_, t in res[True][form].items():
            u = res[False][form][k_]
            if k_ in PER_EV and form == 1:  # (run_chain: one buffer, the last run's rows)
                t, u = t[:B], u[:B]
            same = torch.equal(t.view(torch.int64), u.view(torch.int64)) if t.dtype == torch.float64 else torch.equal(t, u)
            assert same, (form, k_)


# ------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("N", NS)
def test_parity(gpu, N):
    """(2) Every horizon class: the module docstring's checks on the default batch."""
    scalar_case(f"parity N={N}", batch(N), 1)


# ------------------------------------------------------------------------------------------------- 3
@functools.lru_cache(maxsize=None)
def edge_batch(N):
    return one_type(N, [1023, 1024, 1025, 0, 1, 2049], 3000 + N)


@pytest.mark.parametrize("N", [24, 48])
def test_block_edges(gpu, N):
    """(3) One EV type, sets of 1023, 1024, 1025 (one EV either side of a full block), 0, 1 and 2049 EVs."""
    scalar_case(f"block edges N={N}", edge_batch(N))


# ------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("N", [2, 24, 63])
def test_extents_and_null_subsets(gpu, N):
    """(4) All seven non-empty subsets of {cost, w0, status}, each with and without set_stats, and
    set_stats alone, with the batch ending on the 1100-EV, the 1-EV and the empty set: bands intact, inputs
    unchanged, every requested output written to its last element (no other output exists: NULL); once
    with every device pointer 8 but not 16 bytes aligned."""
    subsets = [tuple(n for i, n in enumerate(PER_EV) if m >> i & 1) for m in range(1, 8)]
    for last in (1100, 1, 0):
        bt = batch(N, last)
        for want, stats in [(w, s) for w in subsets for s in (True, False)] + [((), True)]:
            scalar_case(f"extents N={N} last={last} {'+'.join(want) or 'none'} stats={stats}", bt, 1, want, stats)
    scalar_case(f"misaligned N={N}", batch(N, 1100), 1, misalign=True)


def test_unrequested_outputs_keep_their_pattern(gpu):
    """(4) Outputs that exist but are not passed to the run keep their pattern."""
    N = 24
    bt = batch(N)
    gb = arena(bt)
    plan = make_plan(bt, gb, scalar_pass=True)
    S = bt.S
    rc = plan._lib.lompc_plan_run(plan._plan, gb.ptr("lmbd", S * 3 * N), gb.ptr("lmbd_r", S), None, None, gb.ptr("w0"), None, None,
                                  None, plan._stream)
    assert rc == 0 and plan.check()[1:] == (0, 0)
    gb.check_bands()
    gb.check_written("w0")
    for n in ("cost", "status", "set_stats"):
        gb.check_untouched(n)


# ------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("N", [13, 24])
def test_invalid_gamma(gpu, N):
    """(5) NaN, -1e-3 and y_max + 1e-3 at chosen EVs — a set's first and last EV among them: status INVALID,
    NaN cost and w0, N_INVALID exact, lompc_plan_status agrees; the other EVs pass every check."""
    bt0 = batch(N)
    bt = Batch.__new__(Batch)
    bt.__dict__.update(bt0.__dict__)
    g = bt0.gn.copy()
    off = bt0.off
    big = int(np.argmax(np.diff(off)))  # the small type's 1100-EV set
    a, b = int(off[big]), int(off[big + 1])
    a2, b2 = int(off[-2]), int(off[-1])  # the large type's
    idx = np.array([a, a + 1, a + 64, a + 511, a + 512, b - 1, a2, a2 + 700, b2 - 1, int(off[2])])  # (+ the 63-EV set's first)
    ymax = np.array([bt0.consts_of(np.searchsorted(off, i, side="right") - 1).y_max for i in idx])
    g[idx] = np.where(np.arange(idx.size) % 3 == 0, np.nan, np.where(np.arange(idx.size) % 3 == 1, -1e-3, ymax + 1e-3))
    bt.gn, bt._oracle = g, {}
    status, plan, _ = scalar_case(f"invalid N={N}", bt, 1, invalid=idx)
    assert np.sum(status == ST.LOMPC_QP_INVALID) == idx.size
    rep, fail, inv = status_counts(plan)
    # (the counted run and the repeated run of `check`)
    assert (rep, fail, inv) == (2 * np.sum(status == ST.LOMPC_QP_REPAIRED), 0, 2 * idx.size)


@pytest.mark.parametrize("N", [13, 24])
def test_uncovered_evs_are_repaired(gpu, N):
    """(5) A plan created on gamma in a narrow window (y0 in [0.40, 0.41]); then a third of each set's gamma
    overwritten in place with values across [0, y_max] outside it: the moved EVs report REPAIRED and meet the
    oracle bars, at least one per set of >= 63 EVs, N_REPAIRED and lompc_plan_status agree with the per-EV
    status, outputs bitwise the unflagged plan's."""
    sizes = [0, 1, 63, 65, 1100]
    cs, lompcs = contexts(N)
    bt = Batch.__new__(Batch)
    bt.N, bt.K, bt.cs, bt.lompcs, bt.P = N, 1, cs, list(lompcs), len(sizes)
    bt.rng = rng = np.random.default_rng(5000 + N)
    parts = [c.y_max - (0.40 + 0.01 * rng.random(m)) for c in cs for m in sizes]
    lm = np.concatenate([c.theta * rng.random((len(sizes), 3 * N)) for c in cs])[None]
    lr = (0.2 * rng.random(2 * len(sizes)) * np.tile([0.0, 1.0, 0.0, 1.0, 1.0], 2))[None]
    bt.take(parts, lm, lr, device=False)
    gm = bt.gn.copy()
    moved = []
    for s in range(bt.S):
        a, b = int(bt.off[s]), int(bt.off[s + 1])
        ym = bt.consts_of(s).y_max
        pick = a + rng.choice(b - a, (b - a) // 3, replace=False) if b - a >= 3 else np.zeros(0, dtype=np.int64)
        u = rng.random(pick.size)  # across [0, y_max], outside [y_max - 0.45, y_max - 0.36]
        lo_len, hi_len = ym - 0.45, 0.36
        x = u * (lo_len + hi_len)
        gm[pick] = np.where(x < lo_len, x, ym - 0.36 + (x - lo_len))
        moved.append(pick)
    moved = np.concatenate(moved)
    gm[moved[:2]] = [0.0, bt.consts_of(0).y_max]  # and the bounds themselves

    def move(gb):
        gb.view("gamma").copy_(torch.as_tensor(gm))
        dt, shape, _ = gb._spec["gamma"]
        gb._spec["gamma"] = (dt, shape, gm.copy())  # (the input's reference from here on)

    status, plan, _ = scalar_case(f"uncovered N={N}", bt, 0, gn=gm, move=move)
    assert np.all(status[moved] == ST.LOMPC_QP_REPAIRED)
    for s in range(bt.S):
        a, b = int(bt.off[s]), int(bt.off[s + 1])
        if b - a >= 63:
            assert np.sum(status[a:b] == ST.LOMPC_QP_REPAIRED) >= 1, s
    nrep = int(np.sum(status == ST.LOMPC_QP_REPAIRED))
    assert status_counts(plan) == (2 * nrep, 0, 0)  # (the counted run and the repeated run of `check`)


# ------------------------------------------------------------------------------------------------- 6
@functools.lru_cache(maxsize=None)
def cells_batch(N):
    """One type, sets [65, 700], charge levels in a band 0.05 wide (a station partition's): a cell stores at most
    LQ_PPL = 8 pieces whatever the evaluation stages, and over all of [0, y_max] one cell's path has more
    breakpoints than that — those EVs are re-solved by EITHER evaluation (the piece-slot limit, not the staging
    limit this case is about); over a partition's band the path holds a few pieces."""
    return one_type(N, [65, 700], 6000 + N, t=1, gamma=lambda c, m, rng: c.y_max - (0.40 + 0.05 * rng.random(m)))


@pytest.mark.parametrize("N,g", [(n, g) for n in (24, 64) for g in (1, 6, 16, 17, 40)] + [(64, 1024)])
def test_cell_counts(gpu, N, g):
    """(6) LOMPC_PLAN_CELLS(g): oracle bars for every EV, nothing FAILED; for g <= 16 no EV is lost to the
    staging limit (N_REPAIRED = 0: every used piece staged); g = 1024 at N = 64 is past what a workgroup's
    LDS holds — the host-side check lowers the staged cells, the answer stays exact.  (The unflagged plan
    stages 16 cells at most, so for g > 16 its statuses are REPAIRED where the pass's are OK: the bitwise
    comparison is the other cases'; here both meet the oracle.)"""
    bt = cells_batch(N)
    gb = arena(bt)
    plan = make_plan(bt, gb, scalar_pass=True, cells=g)
    assert plan.cells == g
    n = counted(plan, lambda: run(plan, gb, gb, 0))
    assert (n["k_scalar"], n["k_eval"]) == (1, 0), n
    rep, fail, inv = plan.check()
    assert fail == 0 and inv == 0
    gb.check_bands()
    gb.check_inputs()
    W, C = bt.oracle(0)
    dev = Dev(f"cells N={N} g={g}")
    w0, cost, status = gb.np("w0"), gb.np("cost"), gb.np("status")
    st = gb.np("set_stats").reshape(bt.S, 8)
    assert np.all((status == ST.LOMPC_QP_OK) | (status == ST.LOMPC_QP_REPAIRED))
    dev.add("|dw0|", np.abs(w0 - W[:, 0]), 1e-9)
    dev.add("cost", np.abs(cost - C), 1e-9 + 1e-9 * np.abs(C))
    for s in range(bt.S):
        a, b = bt.off[s], bt.off[s + 1]
        dev.add("sum w0", abs(st[s, ST.LOMPC_STAT_SUM_W0] - W[a:b, 0].sum()), 1e-9 + 1e-10 * abs(W[a:b, 0].sum()))
        dev.add("sum cost", abs(st[s, ST.LOMPC_STAT_SUM_COST] - C[a:b].sum()), 1e-9 + 1e-10 * abs(C[a:b].sum()))
    dev.check()
    assert np.all(st[:, ST.LOMPC_STAT_N_FAILED] == 0)
    assert st[:, ST.LOMPC_STAT_N_REPAIRED].sum() == np.sum(status == ST.LOMPC_QP_REPAIRED) == rep
    if g <= 16:
        # (the batch itself needs no re-solve at this cell count: the default evaluation, which stages every
        # cell up to 16, has none either — so any here would be lost to the pass's staging)
        ref = make_plan(bt, gb, cells=g)
        run(ref, gb, gb, 0)
        assert ref.check() == (0, 0, 0)
        assert rep == 0


# ------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("flag", ["warm_start", "close_in_eval", "close_in_finalize"])
def test_with_other_flags(gpu, flag):
    """(7) WARM_START, CLOSE_IN_EVAL, CLOSE_IN_FINALIZE with the flag: case 2's results (a warm-started plan:
    two runs, the second from the stored working sets)."""
    scalar_case(f"{flag} + scalar", batch(24), 1, **{flag: True})


def test_sorted_gamma_with_scalar_pass(gpu):
    """(7) SORTED_GAMMA | SCALAR_PASS on ascending gamma: with w0 requested the run takes k_scalar and meets
    case 2's bars; with no per-EV output it stays the aggregation — no k_scalar launch, set_sum_w allowed."""
    N = 24
    bt = batch(N, 1100, "sorted")
    scalar_case("sorted + scalar", bt, 1, sorted_gamma=True)
    B, S = bt.B, bt.S
    res = {}
    for flagged in (True, False):
        gb = arena(bt, want=(), extra_out=(("set_sum_w", (S * N,)),))
        plan = make_plan(bt, gb, sorted_gamma=True, scalar_pass=flagged)
        assert plan.launches_per_run() == 2
        n = counted(plan, lambda: run(plan, gb, gb, 1, set_sum_w=gb.ptr("set_sum_w")))
        assert (n["k_path"], n["k_eval"], n["k_finalize"], n["k_scalar"]) == (1, 1, 0, 0), n
        n = counted(plan, lambda: run(plan, gb, gb, 1))  # set_stats alone: still the aggregation
        assert (n["k_eval"], n["k_scalar"]) == (1, 0), n
        assert plan.check()[1:] == (0, 0)
        gb.check_bands()
        res[flagged] = (gb.np("set_sum_w"), gb.np("set_stats"))
    for a_, b_ in zip(res[True], res[False]):
        np.testing.assert_array_equal(bits(a_), bits(b_))


def test_update_keeps_the_flag(gpu):
    """(7) plan.update() to a batch of another size and other set offsets, then a scalar run: case 2's checks
    on the new batch."""
    N = 24
    b0, bt = batch(N, 1100), batch(N, 65)  # (the rotation moves every offset)
    sub = Batch.__new__(Batch)             # ... and the new batch drops the last set's EVs but 7
    sub.__dict__.update(bt.__dict__)
    cut = int(bt.off[-1] - bt.off[-2]) - 7
    sub.off = bt.off.copy()
    sub.off[-1] -= cut
    sub.B = int(sub.off[-1])
    sub.gn, sub._oracle = bt.gn[:sub.B].copy(), {}
    g0 = arena(b0)
    gb = arena(sub)
    gu = outputs(Guarded(), sub, PER_EV, True).build()
    plan = make_plan(b0, g0, scalar_pass=True)
    run(plan, g0, g0, 1)
    assert plan.check()[1:] == (0, 0)
    plan.update(gb.view("gamma"), sub.off, gb.view("w_ref"), validate=False)
    assert plan.B == sub.B != b0.B and plan.scalar_pass
    ref = make_plan(sub, gb)
    n = counted(plan, lambda: run(plan, gb, gb, 1))
    assert (n["k_scalar"], n["k_eval"]) == (1, 0), n
    run(ref, gb, gu, 1)
    check("after update", sub, 1, gb, gu, plan)


# ------------------------------------------------------------------------------------------------- 8
EDGE_FAMILIES = ("flat", "half_zero", "spike", "huge_l1", "huge_l2", "huge_l3")


@functools.lru_cache(maxsize=None)
def family_batch(N):
    """Both types, one set per (family, lmbd_r): price_families' gamma (0 and y_max exactly, ties)."""
    cs, lompcs = contexts(N)
    bt = Batch.__new__(Batch)
    bt.N, bt.K, bt.cs, bt.lompcs = N, 1, cs, list(lompcs)
    bt.rng = np.random.default_rng(8000 + N)
    parts, lm, lr = [], [], []
    for ev in ("small", "large"):
        for i, (f, lmbd, r) in enumerate(PF.cases(N, ev, EDGE_FAMILIES)):
            parts.append(PF.gammas(N, ev, seed=i))
            lm.append(lmbd)
            lr.append(r)
    bt.P = len(parts) // 2
    bt.take(parts, np.array(lm)[None], np.array(lr)[None], device=False)
    return bt


@pytest.mark.parametrize("N", [24, 48])
def test_prices_at_the_edges(gpu, N):
    """(8) flat, half-zero and spiked prices and one component at 3.885e5 theta (each price block's), at
    lmbd_r = 0 and 1.5 N delta: oracle bars for every EV with status OK or REPAIRED, no FAILED where the
    unflagged plan has none (the counters equal the unflagged plan's), per-EV outputs its bits.  The set sums
    are held to the pass's own per-EV outputs here (prices of 3.9e5 theta: the per-EV bar is 1e-9 relative,
    the sums' oracle bar of the other cases 1e-10)."""
    scalar_case(f"price families N={N}", family_batch(N), allow_failed=True, oracle_sums=False)


# ------------------------------------------------------------------------------------------------- 9
def test_binding(gpu):
    """(9) BatchPlan(scalar_pass=True): ValueError with want_w or sort_sets; run() returns set_stats and no
    set_sum_w; profile(kernel="k_scalar") counts its launch; the outputs are an unflagged plan's."""
    N = 24
    bt = batch(N)
    kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d)
    with pytest.raises(ValueError):
        BatchPlan(bt.lompcs, bt.g, bt.off, scalar_pass=True, want_w=True, **kw)
    with pytest.raises(ValueError):
        BatchPlan(bt.lompcs, bt.g, bt.off, scalar_pass=True, want_w=False, want_cost=False, sort_sets=True, **kw)
    want = dict(want_w=False, want_cost=True, want_w0=True, want_status=True, want_set=True)
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, scalar_pass=True, **want, **kw)
    assert plan.launches_per_run() == 3
    plan.profile(enable=("k_scalar", "k_eval"))
    out = plan.run(bt.lm_d[1], bt.lr_d[1])
    assert plan.check()[1:] == (0, 0)
    assert plan.profile(read=True, kernel="k_scalar")[1] == 1 and plan.profile(read=True, kernel="k_eval")[1] == 0
    assert out["set_stats"] is not None and out.get("set_sum_w") is None and out["w"] is None
    ref = BatchPlan(bt.lompcs, bt.g, bt.off, **want, **kw)
    o = ref.run(bt.lm_d[1], bt.lr_d[1])
    assert ref.check()[1:] == (0, 0)
    for k in PER_EV:
        assert torch.equal(out[k], o[k]), k
    a, b = out["set_stats"].cpu().numpy(), o["set_stats"].cpu().numpy()
    for col in (ST.LOMPC_STAT_COUNT, ST.LOMPC_STAT_N_REPAIRED, ST.LOMPC_STAT_N_FAILED, ST.LOMPC_STAT_N_INVALID):
        np.testing.assert_array_equal(a[:, col], b[:, col])
    np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-9)


# ------------------------------------------------------------------------------------------------ 10
def test_station_w0_pass(gpu, monkeypatch):
    """(10) Two identical stations (test_gpu_station.py's small seeded configuration, horizons 12 / 16), one
    with w0_scalar_pass: after one step the per-EV w0 of both types is bitwise equal, the per-partition
    (sum w0, sum price0) agree to 1e-11, the counts exactly, the step's discrete logs are equal, and the
    station with the pass recorded a K_SCALAR launch on its _w0plan (the other none)."""
    from lompc_amd import settings
    from test_gpu_station import consts

    monkeypatch.setattr(settings, "PRINT_LEVEL", 0)
    got = {}
    for flag in (True, False):
        np.random.seed(1)
        from lompc_amd.charging_station import ChargingStation

        cs = ChargingStation(consts(60, Tf=1), device=0)
        cs.w0_scalar_pass = flag
        inner = cs._w0_both
        seen = {}

        def both(*a, _cs=cs, _inner=inner, _seen=seen):
            _inner(*a)  # (creates the plan; the profiled call re-targets it at the same batch)
            n = counted(_cs._w0plan, lambda: _seen.update(res=_inner(*a)))
            _seen["n"] = n
            return _seen["res"]

        cs._w0_both = both
        cs._step()
        w0_s, w0_l, red = seen["res"]
        assert cs._w0plan.scalar_pass == flag
        got[flag] = (w0_s.clone(), w0_l.clone(), red.cpu().numpy(), seen["n"], cs.logs)
    (ws, wl, red, n, logs), (ws0, wl0, red0, n0, logs0) = got[True], got[False]
    assert n["k_scalar"] == 1 and n["k_eval"] == 0 and n0["k_scalar"] == 0 and n0["k_eval"] == 1, (n, n0)
    assert torch.equal(ws, ws0) and torch.equal(wl, wl0)
    np.testing.assert_allclose(red[:, :2], red0[:, :2], rtol=1e-11, atol=0)
    np.testing.assert_array_equal(red[:, 2:], red0[:, 2:])
    for k in ("Mp_s", "Mp_l", "niter_s", "niter_l"):
        np.testing.assert_array_equal(logs["statistics"][k], logs0["statistics"][k], err_msg=k)
    assert logs["statistics"]["ncharged_s"] == logs0["statistics"]["ncharged_s"]
    assert logs["statistics"]["ncharged_l"] == logs0["statistics"]["ncharged_l"]
