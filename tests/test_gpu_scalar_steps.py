"""The wide scalar form (LOMPC_STEPS_SCALAR_PASS, k_scalars): per-EV w0 / cost / status and set_stats of a
lompc_plan_run_steps call over a LOMPC_PLAN_SCALAR_PASS plan that asks for no w row and no per-stage sum —
one EV population at K independent price vectors, evaluated from the path tables' coefficient records alone.

Every buffer the C ABI sees comes from tests/guarded.py (outputs pre-filled with a pattern between bands of
it); the calls are raw lompc_plan_run_steps calls, so NULL outputs are NULL.  Throughout:

  * "flagless": the same plan and the same call without LOMPC_STEPS_SCALAR_PASS (k_evals);
  * "single":   one scalar lompc_plan_run per run at that run's prices (k_scalar).

What a run of a scalar call is checked for (`vs_oracle`, `same_bits`): cost, w0 and status bit for bit the
flagless call's and the single run's; against oracle_c.solve_batch over EVERY EV |dw0| <= 1e-9 and cost
1e-9 + 1e-9 |ref|; status OK or REPAIRED (INVALID with NaN outputs exactly where gamma is invalid); COUNT,
N_REPAIRED, N_FAILED, N_INVALID exact; SUM_W0 / SUM_PRICE0 / SUM_COST against the call's own per-EV outputs at
1e-9 + 1e-11 |ref| and against the oracle's at 1e-9 + 1e-10 |ref|; MAX_ERR within 1e-9 of the flagless
call's; bands intact, inputs unchanged, gaps and unrequested outputs still the pattern.

Shapes: test_gpu_plan_horizons.Batch (both EV types, the ragged sets [0, 1, 63, 65, 1100]) in
test_gpu_extents.py's rotations, and test_gpu_scalar_pass.py's one-type batches.  Launch counts come from
the plan's HIP-event profile.
"""
import functools

import numpy as np
import pytest
import torch

from guarded import Guarded
from lompc_amd import BatchPlan, _lib
from test_gpu_extents import ROT, batch
from test_gpu_plan_horizons import Batch, Dev, contexts
from test_gpu_scalar_pass import bits, counted, make_plan, one_type, outputs, price0_of

pytestmark = pytest.mark.gpu

ST = _lib
NS = [1, 2, 13, 24, 48, 63, 64]
PER_EV = ("cost", "w0", "status")
SC = getattr(_lib, "LOMPC_STEPS_SCALAR_PASS", None)  # (None: a library without the form — every case fails)
PK = _lib.LOMPC_STEPS_PER_KERNEL
OKS = (ST.LOMPC_QP_OK, ST.LOMPC_QP_REPAIRED)


def with_prices(bt, K, seed):
    """bt with K runs of fresh prices (Batch's recipe: theta * rand, lmbd_r > 0 on every other set)."""
    b = Batch.__new__(Batch)
    b.__dict__.update(bt.__dict__)
    rng = np.random.default_rng(seed)
    th = np.array([bt.consts_of(s).theta for s in range(bt.S)])
    b.K = K
    b.lm = th[None, :, None] * rng.random((K, bt.S, 3 * bt.N))
    b.lr = 0.2 * rng.random((K, bt.S)) * (np.arange(bt.S) % 2)
    b._oracle = {}
    return b


def outs_k(gb, bt, K, want=PER_EV, stats=True, evs=None, sts=None):
    """The outputs of a K-run call: per-EV buffers of (K - 1) evs + B elements, set_stats (K - 1) sts + 8 S."""
    evs = bt.B if evs is None else evs
    sts = 8 * bt.S if sts is None else sts
    for n in want:
        gb.out(n, ((K - 1) * evs + bt.B,), torch.int8 if n == "status" else torch.float64)
    if stats:
        gb.out("set_stats", ((K - 1) * sts + 8 * bt.S,))
    return gb


def arena_k(bt, K, want=PER_EV, stats=True, evs=None, sts=None, lm=None, lr=None, misalign=False):
    gb = Guarded(misalign=misalign)
    gb.inp("gamma", bt.gn).inp("lmbd", bt.lm if lm is None else lm).inp("lmbd_r", bt.lr if lr is None else lr)
    gb.inp("w_ref", bt.wr)
    return outs_k(gb, bt, K, want, stats, evs, sts).build()


def steps(plan, gin, gout, K, flags, evs=None, sts=None, lms=None, lrs=None, w=None, ssw=None, run0=0):
    """lompc_plan_run_steps at the prices of arena gin from run run0 on, into arena gout's outputs."""
    S, N, B = plan.S, plan.N, plan.B
    lms = S * 3 * N if lms is None else lms
    lrs = S if lrs is None else lrs
    return plan._lib.lompc_plan_run_steps(
        plan._plan, gin.ptr("lmbd", run0 * lms), lms, gin.ptr("lmbd_r", run0 * lrs), lrs, K, 0, w, gout.ptr("cost"),
        gout.ptr("w0"), gout.ptr("status"), ssw, gout.ptr("set_stats"), S * N, 8 * S if sts is None else sts,
        B if evs is None else evs, flags, plan._stream)


def ok(plan, rc):
    assert rc == 0, plan._lib.lompc_plan_last_error(plan._plan)


def single(plan, gin, gout, k):
    S, N = plan.S, plan.N
    ok(plan, plan._lib.lompc_plan_run(plan._plan, gin.ptr("lmbd", k * S * 3 * N), gin.ptr("lmbd_r", k * S), None,
                                      gout.ptr("cost"), gout.ptr("w0"), gout.ptr("status"), None, gout.ptr("set_stats"),
                                      plan._stream))


def run_of(g, bt, k, evs=None, sts=None):
    """Run k's outputs of a K-run arena: per-EV (B,), set_stats (S, 8)."""
    evs = bt.B if evs is None else evs
    sts = 8 * bt.S if sts is None else sts
    o = {n: g.np(n)[k * evs:k * evs + bt.B] for n in PER_EV if n in g._at}
    if "set_stats" in g._at:
        o["set_stats"] = g.np("set_stats")[k * sts:k * sts + 8 * bt.S].reshape(bt.S, 8)
    return o


def same_bits(a, b, what, names=PER_EV):
    for n in names:
        if n in a:
            assert n in b, (what, n)
            np.testing.assert_array_equal(bits(a[n]), bits(b[n]), err_msg=f"{what}: {n}")


def same_arenas(ga, gb_, what):
    for n in ga._at:
        if ga._spec[n][2] is None:
            a, b = ga.view(n), gb_.view(n)
            same = torch.equal(a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)
            assert same, f"{what}: {n}"


def vs_oracle(dev, name, bt, k, o, flagless=None, invalid=None, gn=None):
    """Run k's outputs o against the oracle (gamma gn, the batch's own by default; invalid: the EVs whose gamma
    is invalid) and its set_stats against its own per-EV outputs and the flagless call's counters."""
    B, S = bt.B, bt.S
    inv = np.zeros(B, dtype=bool)
    if invalid is not None:
        inv[invalid] = True
    g = bt.gn if gn is None else gn
    W, C = bt.oracle(k, np.where(inv, 0.0, g) if (gn is not None or invalid is not None) else None)
    status = o.get("status")
    good = ~inv
    if status is not None:
        assert np.all(status[inv] == ST.LOMPC_QP_INVALID), name
        assert np.all(np.isin(status[~inv], OKS)), (name, np.unique(status))
    for n in ("cost", "w0"):
        if n in o:
            assert np.all(np.isnan(o[n][inv])), name
    if "w0" in o:
        dev.add("|dw0|", np.abs(o["w0"][good] - W[good, 0]), 1e-9)
    if "cost" in o:
        dev.add("cost", np.abs(o["cost"][good] - C[good]), 1e-9 + 1e-9 * np.abs(C[good]))
    if "set_stats" not in o:
        return
    st = o["set_stats"]
    np.testing.assert_array_equal(st[:, ST.LOMPC_STAT_COUNT], np.diff(bt.off))
    assert np.all(st[:, ST.LOMPC_STAT_N_FAILED] == 0), name
    if flagless is not None:
        su = flagless["set_stats"]
        for col in (ST.LOMPC_STAT_N_REPAIRED, ST.LOMPC_STAT_N_FAILED, ST.LOMPC_STAT_N_INVALID):
            np.testing.assert_array_equal(st[:, col], su[:, col], err_msg=f"{name}: counter {col} vs the flagless call")
        dev.add("MAX_ERR vs flagless", np.abs(st[:, ST.LOMPC_STAT_MAX_ERR] - su[:, ST.LOMPC_STAT_MAX_ERR]), 1e-9)
    for s in range(S):
        a, b = bt.off[s], bt.off[s + 1]
        m = good[a:b]
        if status is not None:
            assert st[s, ST.LOMPC_STAT_N_INVALID] == np.sum(status[a:b] == ST.LOMPC_QP_INVALID), (name, s)
            assert st[s, ST.LOMPC_STAT_N_REPAIRED] == np.sum(status[a:b] == ST.LOMPC_QP_REPAIRED), (name, s)
        else:
            assert st[s, ST.LOMPC_STAT_N_INVALID] == np.sum(inv[a:b]), (name, s)
        refs = {"sum w0": (ST.LOMPC_STAT_SUM_W0, W[a:b, 0][m].sum()),
                "sum price0": (ST.LOMPC_STAT_SUM_PRICE0, price0_of(bt, k, s, W[a:b, 0][m]).sum()),
                "sum cost": (ST.LOMPC_STAT_SUM_COST, C[a:b][m].sum())}
        for what, (col, ref) in refs.items():
            dev.add(what + " vs oracle", abs(st[s, col] - ref), 1e-9 + 1e-10 * abs(ref))
        if "w0" in o:
            own = o["w0"][a:b][m]
            dev.add("sum w0 vs own", abs(st[s, ST.LOMPC_STAT_SUM_W0] - own.sum()), 1e-9 + 1e-11 * abs(own.sum()))
            p0 = price0_of(bt, k, s, own).sum()
            dev.add("sum price0 vs own", abs(st[s, ST.LOMPC_STAT_SUM_PRICE0] - p0), 1e-9 + 1e-11 * abs(p0))
        if "cost" in o:
            own = o["cost"][a:b][m].sum()
            dev.add("sum cost vs own", abs(st[s, ST.LOMPC_STAT_SUM_COST] - own), 1e-9 + 1e-11 * abs(own))


def scalar_steps_case(name, bt, K, oracle_runs=None, misalign=False, invalid=None, gn=None, move=None, singles=True,
                      flagless_bits=True, **kw):
    """One flagged plan: the scalar call (asserted to take k_scalars), the flagless call, the single runs —
    ev_stride = B, every run's set_stats — and the module docstring's checks.  Returns (plan, input arena,
    scalar outputs, flagless outputs)."""
    gb = arena_k(bt, K, misalign=misalign)
    gf = outs_k(Guarded(misalign=misalign), bt, K).build()
    plan = make_plan(bt, gb, scalar_pass=True, **kw)
    if move is not None:
        move(gb)
    n = counted(plan, lambda: ok(plan, steps(plan, gb, gb, K, SC)))
    assert (n["k_scalar"], n["k_eval"], n["k_path"], n["k_finalize"]) == (K, 0, K, K), (name, n)
    ok(plan, steps(plan, gb, gf, K, 0))
    torch.cuda.synchronize()
    for g in (gb, gf):
        g.check_bands()
    gb.check_inputs()
    for nm in PER_EV + ("set_stats",):
        gb.check_written(nm)
    dev = Dev(name)
    g1 = outputs(Guarded(misalign=misalign), bt, PER_EV, True).build() if singles else None
    for k in range(K):
        o, f = run_of(gb, bt, k), run_of(gf, bt, k)
        if flagless_bits:
            same_bits(o, f, f"{name}: run {k} vs the flagless call")
        if singles:
            single(plan, gb, g1, k)
            torch.cuda.synchronize()
            same_bits(o, run_of(g1, bt, 0), f"{name}: run {k} vs the single run")
        if oracle_runs is None or k in oracle_runs:
            vs_oracle(dev, f"{name} run {k}", bt, k, o, f if flagless_bits else None, invalid=invalid, gn=gn)
    if g1 is not None:
        g1.check_bands()
    dev.check()
    # a second identical call: the same bits in every output
    g2 = outs_k(Guarded(misalign=misalign), bt, K).build()
    ok(plan, steps(plan, gb, g2, K, SC))
    torch.cuda.synchronize()
    g2.check_bands()
    same_arenas(gb, g2, f"{name}: second call")
    return plan, gb, gb, gf


# ------------------------------------------------------------------------------------------------- 1
def test_dispatch(gpu):
    """(1) Which calls take k_scalars (N = 24, K = 3): a flagged plan with the steps flag and w = set_sum_w =
    NULL.  With w, with set_sum_w, on a warm-started and on a DIAG_REPAIR plan the flag changes nothing: k_eval,
    and every output bitwise the flagless call's.  On an unflagged plan the flag is refused with nothing
    written.  SORTED_GAMMA | SCALAR_PASS: the scalar form with per-EV outputs, the aggregation without."""
    N, K = 24, 3
    bt = batch(N)
    B, S = bt.B, bt.S
    gb = arena_k(bt, K)
    plan = make_plan(bt, gb, scalar_pass=True)
    n = counted(plan, lambda: ok(plan, steps(plan, gb, gb, K, SC)))
    assert (n["k_scalar"], n["k_eval"], n["k_path"]) == (K, 0, K), n
    n = counted(plan, lambda: ok(plan, steps(plan, gb, gb, K, SC | PK)))
    assert (n["k_scalar"], n["k_eval"], n["k_path"]) == (K, 0, K), n
    assert plan.check()[1:] == (0, 0)

    def both(plan, extra=(), **call):
        """The call with and without the flag into two arenas: k_eval both times, the same bits."""
        res = []
        for flags in (SC, 0):
            go = outs_k(Guarded(), bt, K)
            for nm, size in extra:
                go.out(nm, (size,))
            go.build()
            ptrs = {k_: go.ptr(v) for k_, v in call.items()}
            n = counted(plan, lambda: ok(plan, steps(plan, gb, go, K, flags, **ptrs)))
            assert n["k_scalar"] == 0 and n["k_eval"] >= 1, (flags, n)
            torch.cuda.synchronize()
            go.check_bands()
            res.append(go)
        same_arenas(res[0], res[1], f"per-call condition {sorted(call)}")

    both(plan, extra=(("w", K * B * N),), w="w")
    both(plan, extra=(("set_sum_w", K * S * N),), ssw="set_sum_w")
    both(make_plan(bt, gb, scalar_pass=True, warm_start=True))
    both(make_plan(bt, gb, scalar_pass=True, diag_repair=True))
    # the flag on an unflagged plan: a static misuse
    plain = make_plan(bt, gb)
    go = outs_k(Guarded(), bt, K).build()
    assert steps(plain, gb, go, K, SC) == ST.LOMPC_ERR_INVALID_ARG
    assert plain._lib.lompc_plan_last_error(plain._plan)
    torch.cuda.synchronize()
    go.check_bands()
    for nm in PER_EV + ("set_stats",):
        go.check_untouched(nm)
    # gamma-sorted sets
    bs = batch(N, 1100, "sorted")
    gs = arena_k(bs, K)
    ps = make_plan(bs, gs, scalar_pass=True, sorted_gamma=True)
    n = counted(ps, lambda: ok(ps, steps(ps, gs, gs, K, SC)))
    assert (n["k_scalar"], n["k_eval"]) == (K, 0), n
    dev = Dev("sorted + scalar steps")
    for k in range(K):
        vs_oracle(dev, f"sorted run {k}", bs, k, run_of(gs, bs, k))
    dev.check()
    res = []
    for flags in (SC, 0):  # no per-EV output: the aggregation, whatever the flag
        go = outs_k(Guarded(), bs, K, want=()).build()
        n = counted(ps, lambda: ok(ps, steps(ps, gs, go, K, flags)))
        assert n["k_scalar"] == 0 and n["k_eval"] == K, (flags, n)
        res.append(go)
    torch.cuda.synchronize()
    same_arenas(res[0], res[1], "sorted, set_stats alone")
    assert ps.check()[1:] == (0, 0)


# ------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("N", NS)
def test_parity(gpu, N):
    """(2) Every horizon class, K = 3, ev_stride = B: the module docstring's checks over every EV of every run."""
    plan, *_ = scalar_steps_case(f"parity N={N}", batch(N), 3)
    assert plan.check()[1:] == (0, 0)


# ------------------------------------------------------------------------------------------------- 3
@functools.lru_cache(maxsize=None)
def long_batch():
    return with_prices(batch(24), 130, 24130)


@pytest.mark.parametrize("K", [1, 2, 64, 65, 130])
def test_group_boundaries(gpu, K):
    """(3) Groups of 64 runs over a ring of min(K, 64) + 1 table slots: every run bitwise the flagless call's,
    runs 0, 63, 64 and K - 1 against the oracle; run 64 of the K = 65 call equals a K = 1 call at its prices in
    every output bit, set_stats included."""
    bt = long_batch()
    plan, gb, gs, _ = scalar_steps_case(f"groups K={K}", bt, K, oracle_runs={0, 63, 64, K - 1}, singles=K <= 2)
    if K == 65:
        g1 = outs_k(Guarded(), bt, 1).build()
        ok(plan, steps(plan, gb, g1, 1, SC, run0=64))
        torch.cuda.synchronize()
        g1.check_bands()
        same_bits(run_of(gs, bt, 64), run_of(g1, bt, 0), "run 64 of 65 vs K = 1", PER_EV + ("set_stats",))


@pytest.mark.parametrize("K", [3, 65])
def test_per_kernel_is_the_same_bits(gpu, K):
    """(3) PER_KERNEL | SCALAR_PASS (one run per group) is bitwise SCALAR_PASS alone."""
    bt = long_batch()
    gb = arena_k(bt, K)
    go = outs_k(Guarded(), bt, K).build()
    plan = make_plan(bt, gb, scalar_pass=True)
    ok(plan, steps(plan, gb, gb, K, SC))
    n = counted(plan, lambda: ok(plan, steps(plan, gb, go, K, SC | PK)))
    assert (n["k_scalar"], n["k_eval"], n["k_path"]) == (K, 0, K), n
    torch.cuda.synchronize()
    go.check_bands()
    same_arenas(gb, go, f"per kernel K={K}")


# ------------------------------------------------------------------------------------------------- 4
def test_shared_per_ev_buffers(gpu):
    """(4) ev_stride = 0: the per-EV buffers end as the last run of the ev_stride = B call, bit for bit; each
    run's set_stats is its own."""
    N, K = 24, 3
    bt = batch(N)
    gb = arena_k(bt, K)
    g0 = outs_k(Guarded(), bt, K, evs=0).build()
    plan = make_plan(bt, gb, scalar_pass=True)
    ok(plan, steps(plan, gb, gb, K, SC))
    n = counted(plan, lambda: ok(plan, steps(plan, gb, g0, K, SC, evs=0)))
    assert (n["k_scalar"], n["k_eval"]) == (K, 0), n
    torch.cuda.synchronize()
    g0.check_bands()
    same_bits(run_of(g0, bt, 0, evs=0), run_of(gb, bt, K - 1), "ev_stride 0 vs the last run")
    np.testing.assert_array_equal(bits(g0.np("set_stats")), bits(gb.np("set_stats")))


@pytest.mark.parametrize("misalign", [False, True])
def test_strides_and_gaps(gpu, misalign):
    """(4) ev_stride = B + 3, set_stats_stride = 8 S + 3, price stride 3 N S + 7 with NaN padding, one lmbd_r
    for all runs (stride 0): the gaps keep the pattern, every run meets the bars and the flagless call's bits;
    once with every device pointer 8 but not 16 bytes aligned.  ev_stride = B - 1 is refused, nothing written."""
    N, K = 24, 3
    b0 = batch(N)
    bt = Batch.__new__(Batch)
    bt.__dict__.update(b0.__dict__)
    bt.lr, bt._oracle = np.repeat(b0.lr[:1], K, axis=0), {}
    B, S = bt.B, bt.S
    evs, sts, lms = B + 3, 8 * S + 3, 3 * N * S + 7
    lm = np.full((K, lms), np.nan)
    lm[:, :3 * N * S] = bt.lm.reshape(K, -1)
    gb = arena_k(bt, K, evs=evs, sts=sts, lm=lm, lr=b0.lr[:1], misalign=misalign)
    gf = outs_k(Guarded(misalign=misalign), bt, K, evs=evs, sts=sts).build()
    plan = make_plan(bt, gb, scalar_pass=True)
    kw = dict(evs=evs, sts=sts, lms=lms, lrs=0)
    n = counted(plan, lambda: ok(plan, steps(plan, gb, gb, K, SC, **kw)))
    assert (n["k_scalar"], n["k_eval"]) == (K, 0), n
    ok(plan, steps(plan, gb, gf, K, 0, **kw))
    torch.cuda.synchronize()
    gb.check_bands()
    gb.check_inputs()
    gf.check_bands()
    me = np.zeros((K - 1) * evs + B, dtype=bool)
    ms = np.zeros((K - 1) * sts + 8 * S, dtype=bool)
    for k in range(K):
        me[k * evs:k * evs + B] = True
        ms[k * sts:k * sts + 8 * S] = True
    for nm in PER_EV:
        gb.check_written(nm, me)
    gb.check_written("set_stats", ms)
    dev = Dev(f"strides misalign={misalign}")
    for k in range(K):
        o, f = run_of(gb, bt, k, evs, sts), run_of(gf, bt, k, evs, sts)
        same_bits(o, f, f"strides run {k} vs flagless")
        vs_oracle(dev, f"strides run {k}", bt, k, o, f)
    dev.check()
    assert plan.check()[1:] == (0, 0)
    go = outs_k(Guarded(misalign=misalign), bt, K, evs=B, sts=sts).build()
    assert steps(plan, gb, go, K, SC, evs=B - 1, sts=sts, lms=lms, lrs=0) == ST.LOMPC_ERR_INVALID_ARG
    torch.cuda.synchronize()
    go.check_bands()
    for nm in PER_EV + ("set_stats",):
        go.check_untouched(nm)


@pytest.mark.parametrize("N", [24, 63])
def test_rotations(gpu, N):
    """(4) The ragged sets rotated: the batch ending on the 65-EV, the 1-EV and the empty set."""
    for last in (65, 1, 0):
        assert ROT[last][-1] == last
        scalar_steps_case(f"rotation N={N} last={last}", batch(N, last), 3)


# ------------------------------------------------------------------------------------------------- 5
def test_null_subsets(gpu):
    """(5) N = 24, K = 2: every non-empty subset of (cost, w0, status) with and without set_stats, and set_stats
    alone.  The requested outputs are bitwise the all-outputs call's; the others keep their pattern."""
    N, K = 24, 2
    bt = batch(N)
    gb = arena_k(bt, K)
    plan = make_plan(bt, gb, scalar_pass=True)
    ok(plan, steps(plan, gb, gb, K, SC))
    subsets = [tuple(n for i, n in enumerate(PER_EV) if m >> i & 1) for m in range(1, 8)]
    for want, stats in [(w, s) for w in subsets for s in (True, False)] + [((), True)]:
        name = f"{'+'.join(want) or 'none'} stats={stats}"
        go = outs_k(Guarded(), bt, K).build()  # every output exists; only the subset is passed
        S, B = bt.S, bt.B
        p = lambda nm, on: go.ptr(nm) if on else None
        n = counted(plan, lambda: ok(plan, plan._lib.lompc_plan_run_steps(
            plan._plan, gb.ptr("lmbd"), S * 3 * N, gb.ptr("lmbd_r"), S, K, 0, None, p("cost", "cost" in want),
            p("w0", "w0" in want), p("status", "status" in want), None, p("set_stats", stats), S * N, 8 * S, B, SC,
            plan._stream)))
        assert (n["k_scalar"], n["k_eval"]) == (K, 0), (name, n)
        torch.cuda.synchronize()
        go.check_bands()
        for nm in PER_EV + ("set_stats",):
            if nm in want or (nm == "set_stats" and stats):
                a, b = go.view(nm), gb.view(nm)
                same = torch.equal(a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)
                assert same, (name, nm)
            else:
                go.check_untouched(nm)
    gb.check_inputs()
    dev = Dev("null subsets, all outputs")
    for k in range(K):
        vs_oracle(dev, f"run {k}", bt, k, run_of(gb, bt, k))
    dev.check()


# ------------------------------------------------------------------------------------------------- 6
@functools.lru_cache(maxsize=None)
def edge_batch(N):
    return one_type(N, [1023, 1024, 1025, 0, 1, 2049], 3100 + N, K=2)


@pytest.mark.parametrize("N", [24, 48])
def test_block_edges(gpu, N):
    """(6) One EV type, sets of 1023, 1024, 1025 (one EV either side of a full block), 0, 1 and 2049 EVs."""
    scalar_steps_case(f"block edges N={N}", edge_batch(N), 2)


# ------------------------------------------------------------------------------------------------- 7
def test_invalid_gamma(gpu):
    """(7) NaN, -1e-3 and y_max + 1e-3 at chosen EVs (a set's first and last among them): INVALID with NaN cost
    and w0 in every run, N_INVALID exact; with ev_stride = 0 the last run stores them too."""
    N, K = 24, 3
    b0 = batch(N)
    bt = Batch.__new__(Batch)
    bt.__dict__.update(b0.__dict__)
    g, off = b0.gn.copy(), b0.off
    big = int(np.argmax(np.diff(off)))
    a, b = int(off[big]), int(off[big + 1])
    a2, b2 = int(off[-2]), int(off[-1])
    idx = np.array([a, a + 1, a + 64, a + 511, a + 512, b - 1, a2, a2 + 700, b2 - 1, int(off[2])])
    r = np.arange(idx.size) % 3
    g[idx] = np.where(r == 0, np.nan, np.where(r == 1, -1e-3, 0.9 + 1e-3))
    bt.gn, bt._oracle = g, {}
    plan, gb, gs, _ = scalar_steps_case("invalid gamma", bt, K, invalid=idx)
    for k in range(K):
        assert np.sum(run_of(gs, bt, k)["status"] == ST.LOMPC_QP_INVALID) == idx.size
    g0 = outs_k(Guarded(), bt, K, evs=0).build()
    ok(plan, steps(plan, gb, g0, K, SC, evs=0))
    torch.cuda.synchronize()
    g0.check_bands()
    for nm in PER_EV:
        g0.check_written(nm)
    same_bits(run_of(g0, bt, 0, evs=0), run_of(gs, bt, K - 1), "invalid, ev_stride 0 vs the last run")


def status_counts(plan):
    import ctypes

    r = [ctypes.c_int64(0) for _ in range(3)]
    assert plan._lib.lompc_plan_status(plan._plan, plan._stream, *[ctypes.byref(x) for x in r]) == 0
    return tuple(x.value for x in r)


def test_uncovered_evs_are_repaired(gpu):
    """(7) A plan created on gamma in [0.4, 0.6]; then a third of each set's gamma overwritten in place with
    values in [0, 0.3] and [0.7, 0.9]: the moved EVs are REPAIRED by k_closes in every run (ev_stride = B) and
    meet the bars; with ev_stride = 0 the last run's repairs are what remains; lompc_plan_status reports the
    repairs summed over all K runs, then 0."""
    N, K = 24, 3
    bt = batch(N, 1100, "narrow")
    rng = np.random.default_rng(7024)
    gm, moved = bt.gn.copy(), []
    for s in range(bt.S):
        a, b = int(bt.off[s]), int(bt.off[s + 1])
        pick = a + rng.choice(b - a, (b - a) // 3, replace=False) if b - a >= 3 else np.zeros(0, dtype=np.int64)
        x = 0.5 * rng.random(pick.size)
        gm[pick] = np.where(x < 0.3, x, x + 0.4)
        moved.append(pick)
    moved = np.concatenate(moved)

    def move(gb):
        gb.view("gamma").copy_(torch.as_tensor(gm))
        dt, shape, _ = gb._spec["gamma"]
        gb._spec["gamma"] = (dt, shape, gm.copy())

    gb = arena_k(bt, K)
    plan = make_plan(bt, gb, scalar_pass=True)
    move(gb)
    assert status_counts(plan) == (0, 0, 0)
    n = counted(plan, lambda: ok(plan, steps(plan, gb, gb, K, SC)))
    assert (n["k_scalar"], n["k_eval"]) == (K, 0), n
    torch.cuda.synchronize()
    gb.check_bands()
    gb.check_inputs()
    gf = outs_k(Guarded(), bt, K).build()
    dev = Dev("uncovered")
    nrep = 0
    for k in range(K):
        o = run_of(gb, bt, k)
        assert np.all(o["status"][moved] == ST.LOMPC_QP_REPAIRED), k
        nrep += int(np.sum(o["status"] == ST.LOMPC_QP_REPAIRED))
    assert status_counts(plan) == (nrep, 0, 0)
    assert status_counts(plan) == (0, 0, 0)
    ok(plan, steps(plan, gb, gf, K, 0))
    torch.cuda.synchronize()
    for k in range(K):
        o, f = run_of(gb, bt, k), run_of(gf, bt, k)
        same_bits(o, f, f"uncovered run {k} vs flagless")
        vs_oracle(dev, f"uncovered run {k}", bt, k, o, f, gn=gm)
    dev.check()
    g0 = outs_k(Guarded(), bt, K, evs=0).build()
    ok(plan, steps(plan, gb, g0, K, SC, evs=0))
    torch.cuda.synchronize()
    g0.check_bands()
    same_bits(run_of(g0, bt, 0, evs=0), run_of(gb, bt, K - 1), "uncovered, ev_stride 0 vs the last run")
    np.testing.assert_array_equal(bits(g0.np("set_stats")), bits(gb.np("set_stats")))


# ------------------------------------------------------------------------------------------------- 8
@functools.lru_cache(maxsize=None)
def cells_batch(N):
    """One type, sets [65, 300], charge levels in a band 0.05 wide (test_gpu_scalar_pass.cells_batch's reason)."""
    return one_type(N, [65, 300], 6100 + N, t=1, gamma=lambda c, m, rng: c.y_max - (0.40 + 0.05 * rng.random(m)), K=2)


@pytest.mark.parametrize("N,g", [(n, g) for n in (24, 64) for g in (1, 6, 17, 300)])
def test_cell_counts(gpu, N, g):
    """(8) LOMPC_PLAN_CELLS(g), K = 2: the oracle bars for every EV of both runs, nothing FAILED, per-EV bits the
    single runs'; at g = 300 the pass stages 256 cells, the other cells' EVs come back REPAIRED inside the bar.
    (The flagless evaluation stages 16 cells at most, so for g > 16 its statuses are REPAIRED where the pass's
    are OK: the flagless bits are the other cases'.)"""
    bt = cells_batch(N)
    plan, gb, gs, _ = scalar_steps_case(f"cells N={N} g={g}", bt, 2, cells=g, flagless_bits=g <= 16)
    assert plan.cells == g
    rep, fail, inv = plan.check()
    assert fail == 0 and inv == 0
    nrep = sum(int(np.sum(run_of(gs, bt, k)["status"] == ST.LOMPC_QP_REPAIRED)) for k in range(2))
    if g == 300:
        assert nrep > 0  # (gamma spread over the set's window: some EVs sit in cells 256 .. 299)


# ------------------------------------------------------------------------------------------------- 9
def test_binding(gpu):
    """(9) BatchPlan.run_steps(scalar_pass=True): ValueError on a plan built without scalar_pass; on one built
    with it, k_scalars runs and the outputs are the flagless run_steps call's bits."""
    N, K = 24, 3
    bt = batch(N)
    kw = dict(sets_per_ctx=[bt.P, bt.P], w_ref=bt.wr_d, want_w=False, want_cost=True, want_w0=True, want_status=True,
              want_set=True)
    plain = BatchPlan(bt.lompcs, bt.g, bt.off, **kw)
    with pytest.raises(ValueError):
        plain.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True, scalar_pass=True)
    with pytest.raises(ValueError):
        plain.steps_call(bt.lm_d, bt.lr_d, K, *bt.strides, scalar_pass=True)
    plan = BatchPlan(bt.lompcs, bt.g, bt.off, scalar_pass=True, **kw)
    plan.profile(enable=("k_scalar", "k_eval"))
    out = plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True, scalar_pass=True)
    assert plan.check()[1:] == (0, 0)
    assert plan.profile(read=True, reset=True, kernel="k_scalar")[1] == K
    assert plan.profile(read=True, reset=True, kernel="k_eval")[1] == 0
    assert out["w0"].shape == (K, bt.B) and out["set_stats"].shape == (K, bt.S, 8) and out["set_sum_w"] is None
    ref = plan.run_steps(bt.lm_d, bt.lr_d, K, *bt.strides, per_run=True)
    assert plan.profile(read=True, reset=True, kernel="k_scalar")[1] == 0
    for k in PER_EV:
        assert torch.equal(out[k], ref[k]), k
    np.testing.assert_allclose(out["set_stats"].cpu().numpy(), ref["set_stats"].cpu().numpy(), rtol=1e-11, atol=1e-9)


@pytest.mark.parametrize("ev", [0, 1])
def test_price_solver_many(gpu, ev):
    """(9) PriceSolver.get_w0_price0_many at K = 5 on one partition of ~3000 EVs, N = 24: w0 rows bitwise
    get_w0_price0's, price0 within 1e-9 + 1e-11 |ref| of it, w0 within 1e-9 of the oracle."""
    import oracle_c
    from lompc_amd import LoMPCConstants
    from lompc_amd.price_solver import PriceSolver

    N, K, n = 24, 5, 3001
    c = contexts(N)[0][ev]
    rng = np.random.default_rng(9000 + ev)
    ps = PriceSolver(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), "linear-convex", device=0)
    y0 = 0.35 + 0.1 * rng.random(n)  # (one charge-level partition)
    ps.set_charge_levels(y0)
    lmbds = c.theta * rng.random((K, ps.r))
    lmbd_r = 0.1
    w0, p0 = ps.get_w0_price0_many(lmbds, lmbd_r)
    assert w0.shape == (K, n) and p0.shape == (K,)
    assert ps._plan_w0m.scalar_pass  # (the scalar-pass plan exists: the call went through it)
    dev = Dev(f"get_w0_price0_many type {ev}")
    for k in range(K):
        w1, p1 = ps.get_w0_price0(lmbds[k], lmbd_r)
        np.testing.assert_array_equal(bits(w0[k]), bits(w1), err_msg=f"run {k}")
        dev.add("price0 vs get_w0_price0", abs(p0[k] - p1), 1e-9 + 1e-11 * abs(p1))
        lm = np.zeros(3 * N)
        lm[:ps.r] = lmbds[k]
        W, _, nf = oracle_c.solve_batch(N, c, lm, lmbd_r, c.y_max - y0)
        assert nf == 0
        dev.add("|dw0| vs oracle", np.abs(w0[k] - W[:, 0]), 1e-9)
    dev.check()
