"""WHERE the engine's entry points write: output extents, strides, NULL outputs, alignment, and the row
path of batches whose w exceeds a buffer descriptor's range (B N 8 > LQ_DROP_OFF).

Every buffer the C ABI sees is carved from tests/guarded.py's arenas: outputs pre-filled with a pattern
between bands of it, inputs followed by NaN.  Every form asserts (a) the bands bit for bit untouched, (b)
every requested output fully written and inside test_gpu_plan_horizons.py's bars against
oracle_c.solve_batch over EVERY EV (|dw| <= 1e-9, cost 1e-9 relative, set sums rtol 1e-10 atol 1e-9, a
form's set sums against its own per-EV sums rtol 1e-11, COUNT exact, N_FAILED = N_INVALID = 0), (c) the
inputs bitwise unchanged, (d) lompc_plan_status / lompc_last_status report nothing failed or invalid.

Small shapes: test_gpu_plan_horizons.Batch (both EV types, the ragged sets [0, 1, 63, 65, 1100], its
seeded prices) with the set order rotated so that the batch ends on the 1100-EV set (a partial row
batch), the 65-EV set (a full one), the 1-EV set and the empty set.  Horizons by row-store shape (V
stages per lane, Lr = N / V lanes per row, R = 64 / Lr rows per store instruction, 64 - R Lr idle lanes):

    N    1   2   13  24  48  63  64
    Lr   1   1   13  12  24  63  32
    R    64  64  4   5   2   1   2
    idle 0   0   12  4   16  1   0      (13, 63: the generic kernels' 8-B stores; 24, 48: exact-N)

The large cases (test_rows_past_descriptor_range) derive their batch sizes from LQ_DROP_OFF, read from
csrc/lompc_plan.hip: the last batch a descriptor covers and the first it does not at N = 64 (no idle
lanes: the control), the first it does not at N = 48 (16 idle lanes, every full wave segment ends on a
full batch) and N = 63 (odd N, one idle lane).  Reference there: oracle_c.path_run (oracle/path_cpu.cpp,
pinned to the dense oracle by test_path_cpu.py) for every row and cost, the dense oracle on a sample.
"""
import functools
import os
import re
import time

import numpy as np
import pytest
import torch

import oracle_c
from guarded import Guarded
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, _lib
from test_gpu_plan_horizons import Batch, Dev, contexts, sets_vs_oracle, sets_vs_own_rows

pytestmark = pytest.mark.gpu

ST = _lib
NS = [1, 2, 13, 24, 48, 63, 64]
ROT = {1100: [0, 1, 63, 65, 1100], 65: [1100, 0, 1, 63, 65], 1: [63, 65, 1100, 0, 1], 0: [1, 63, 65, 1100, 0]}
EV = ("w", "cost", "w0", "status")
K = 3
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "incentive-design-mpc_amd", "csrc")
with open(os.path.join(CSRC, "lompc_plan.hip")) as _f:
    _src = _f.read()
LQ_DROP_OFF = int(re.search(r"#define LQ_DROP_OFF (0x[0-9a-fA-F]+)", _src).group(1), 16)
EVAL_RU = int(re.search(r"#define EVAL_RU (\d+)", _src).group(1))


@functools.lru_cache(maxsize=None)
def batch(N, last=1100, layout="ragged"):
    """The horizons module's batch with the set order rotated (shared by every form: one oracle)."""
    return Batch(N, "rows", K, sizes=ROT[last], layout=layout)


@functools.lru_cache(maxsize=None)
def direct_contexts(N):
    cs, _ = contexts(N)
    return tuple(LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0, mode="direct") for c in cs)


def arena(bt, want=EV, sets=True, runs=1, ev_stride=0, sw_stride=0, st_stride=0, lm=None, lr=None, misalign=False,
          ev_rows=None, extra=None):
    """Guarded buffers of one call: gamma, lmbd, lmbd_r, w_ref in; per-EV outputs of (runs - 1) ev_stride + B
    rows (ev_rows: that many instead), set outputs of (runs - 1) stride + one record."""
    N, S, B = bt.N, bt.S, bt.B
    gb = Guarded(misalign=misalign)
    gb.inp("gamma", bt.gn).inp("lmbd", bt.lm if lm is None else lm).inp("lmbd_r", bt.lr if lr is None else lr)
    gb.inp("w_ref", bt.wr)
    for name, a in (extra or {}).items():
        gb.inp(name, a)
    E = ev_rows if ev_rows is not None else (runs - 1) * ev_stride + B
    for name in want:
        gb.out(name, (E, N) if name == "w" else (E,), torch.int8 if name == "status" else torch.float64)
    if sets:
        gb.out("set_sum_w", ((runs - 1) * sw_stride + S * N,))
        gb.out("set_stats", ((runs - 1) * st_stride + S * ST.LOMPC_SET_STATS,))
    return gb.build()


def make_plan(bt, gb, **kw):
    """A plan over the guarded gamma and w_ref (no outputs of its own: the calls pass the arena's)."""
    plan = BatchPlan(bt.lompcs, gb.view("gamma"), bt.off, sets_per_ctx=[bt.P, bt.P], w_ref=gb.view("w_ref"), want_w=False,
                     want_cost=False, want_set=False, **kw)
    assert plan.gamma.data_ptr() == gb.ptr("gamma") and plan.w_ref.data_ptr() == gb.ptr("w_ref")
    return plan


def outs(gb):
    return [gb.ptr(n) for n in EV + ("set_sum_w", "set_stats")]


def plan_run(plan, gb, k=0):
    bt_lm = gb._spec["lmbd"][1]
    return plan._lib.lompc_plan_run(plan._plan, gb.ptr("lmbd", k * int(np.prod(bt_lm[1:]))),
                                    gb.ptr("lmbd_r", k * gb._spec["lmbd_r"][1][1]), *outs(gb), plan._stream)


def run_steps(plan, gb, lm_stride, lr_stride, runs, ev_stride=0, sw_stride=0, st_stride=0, flags=0):
    return plan._lib.lompc_plan_run_steps(plan._plan, gb.ptr("lmbd"), lm_stride, gb.ptr("lmbd_r"), lr_stride, runs, 0,
                                          *outs(gb), sw_stride, st_stride, ev_stride, flags, plan._stream)


def verify(name, gb, at, ev_stride=0, sw_stride=0, st_stride=0, status_is=None, ev_at=None):
    """(a) bands, (b) extents written and inside the bars, (c) inputs.  at: per run a (batch, price index)
    whose oracle the run must match; run j's per-EV outputs at rows j ev_stride (0: the last run's remain),
    its set outputs at j sw_stride / j st_stride (0: the last run's).  ev_at: per EV its row in the outputs
    (rows not named must keep the pattern)."""
    torch.cuda.synchronize()
    gb.check_bands()
    gb.check_inputs()
    bt = at[0][0]
    N, S, B, R = bt.N, bt.S, bt.B, len(at)
    dev = Dev(name)
    has = lambda n: n in gb._at
    ev_runs = list(range(R)) if ev_stride else [R - 1]
    where = [(ev_at if ev_at is not None else np.arange(B)) + j * ev_stride for j in ev_runs]
    for n in EV:
        if has(n):
            m = np.zeros(gb._spec[n][1][0], dtype=bool)
            m[np.concatenate(where)] = True
            gb.check_written(n, m[:, None] if n == "w" else m)
    per_ev = {n: gb.np(n) if has(n) else None for n in EV}
    sw = st = None
    if has("set_sum_w"):
        set_runs = list(range(R)) if sw_stride else [R - 1]
        assert bool(sw_stride) == bool(st_stride)
        ms, mt = np.zeros(gb._spec["set_sum_w"][1][0], dtype=bool), np.zeros(gb._spec["set_stats"][1][0], dtype=bool)
        for j in set_runs:
            ms[j * sw_stride:j * sw_stride + S * N] = True
            mt[j * st_stride:j * st_stride + 8 * S] = True
        gb.check_written("set_sum_w", ms)
        gb.check_written("set_stats", mt)
        fs, ft = gb.np("set_sum_w"), gb.np("set_stats")
        sw = {j: fs[j * sw_stride:j * sw_stride + S * N].reshape(S, N) for j in set_runs}
        st = {j: ft[j * st_stride:j * st_stride + 8 * S].reshape(S, 8) for j in set_runs}
        for j in set_runs:
            b_, k_ = at[j]
            sets_vs_oracle(dev, b_, k_, sw[j], st[j])
    for j, rows in zip(ev_runs, where):
        b_, k_ = at[j]
        W, C = b_.oracle(k_)
        w = per_ev["w"][rows] if has("w") else None
        cost = per_ev["cost"][rows] if has("cost") else None
        if w is not None:
            dev.add("|dw|", np.abs(w - W), 1e-9)
        if cost is not None:
            dev.add("cost", np.abs(cost - C), 1e-9 + 1e-9 * np.abs(C))
        if has("w0"):
            dev.add("|dw0|", np.abs(per_ev["w0"][rows] - W[:, 0]), 1e-9)
        if has("status"):
            s_ = per_ev["status"][rows]
            ok = (s_ == status_is) if status_is is not None else ((s_ == ST.LOMPC_QP_OK) | (s_ == ST.LOMPC_QP_REPAIRED))
            assert np.all(ok), (name, np.unique(s_))
        if w is not None and sw is not None and j in sw:
            sets_vs_own_rows(dev, b_, w, cost, sw[j], st[j])
    dev.check()


def plan_ok(plan, repaired=None):
    """(d) nothing failed or invalid (BatchPlan.check raises on either)."""
    rep, fail, inv = plan.check()
    assert fail == 0 and inv == 0
    if repaired is not None:
        assert rep == repaired


def strides(bt):
    return bt.S * 3 * bt.N, bt.S


PLAN_FORMS = {
    "run": {},
    "close_in_eval": dict(close_in_eval=True),
    "close_in_finalize": dict(close_in_finalize=True),
    "diag_repair": dict(diag_repair=True),
}


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("form", list(PLAN_FORMS))
def test_plan_run_extents(gpu, form, N):
    """lompc_plan_run with every output, each closing mode and the all-re-solve form (DIAG_REPAIR: every row
    written by the individual re-solve), at every rotation of the sets."""
    for last in ROT:
        bt = batch(N, last)
        gb = arena(bt)
        plan = make_plan(bt, gb, **PLAN_FORMS[form])
        assert plan_run(plan, gb, 1) == 0
        diag = form == "diag_repair"
        plan_ok(plan, bt.B if diag else None)
        verify(f"{form} N={N} last={last}", gb, [(bt, 1)], status_is=ST.LOMPC_QP_REPAIRED if diag else None)


STEPS_FORMS = {
    "wide": ({}, 0),
    "per_kernel": ({}, ST.LOMPC_STEPS_PER_KERNEL),
    "warm_stepped": (dict(warm_start=True), 0),
    "cells6_path_fin": (dict(cells=6), 0),
}


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("form", list(STEPS_FORMS))
def test_run_steps_extents(gpu, form, N):
    """lompc_plan_run_steps, K = 3 runs with every output per run: the wide form, its per-kernel issue, a
    warm-started plan (the stepped k_step) and a cell count not divisible by 4 (launch per kernel, the
    closings inside k_path_fin)."""
    kw, flags = STEPS_FORMS[form]
    for last in ROT:
        bt = batch(N, last)
        B, S = bt.B, bt.S
        sws, sts = S * N, 8 * S
        gb = arena(bt, runs=K, ev_stride=B, sw_stride=sws, st_stride=sts)
        plan = make_plan(bt, gb, **kw)
        assert run_steps(plan, gb, *strides(bt), K, B, sws, sts, flags) == 0
        plan_ok(plan)
        info = plan.info()
        if form == "cells6_path_fin":
            assert info["cells"] == 6 and info["steps_group"] == 0
        else:
            assert info["cells"] % 4 == 0 and info["steps_group"] == 1
        verify(f"steps {form} N={N} last={last}", gb, [(bt, k) for k in range(K)], B, sws, sts)


def phi(c, w):
    q_s = 3 * c.theta / (4 * c.w_max)
    return np.concatenate([c.theta * w, c.theta * (c.w_max - w), q_s * w * w], axis=-1)


def at_prices(bt, lm):
    """The batch with one run's prices replaced (an oracle of its own)."""
    at = Batch.__new__(Batch)
    at.__dict__.update(bt.__dict__)
    at.lm, at.lr, at._oracle = lm[None], bt.lr[:1], {}
    return at


@pytest.mark.parametrize("N", NS)
def test_run_chain_extents(gpu, N):
    """lompc_plan_run_chain, K = 3 dependent runs: lmbd_out [K][S][3N] and the per-run set outputs fully
    written, run 0 and the last run against the oracle at the recorded prices, the last run's rows too."""
    for last in ROT:
        bt = batch(N, last)
        S, B = bt.S, bt.B
        wt = np.concatenate([c.w_max * (0.2 + 0.6 * np.random.default_rng(N).random((bt.P, N))) for c in bt.cs])
        gb = Guarded().inp("gamma", bt.gn).inp("lmbd", bt.lm[0]).inp("lmbd_r", bt.lr[0]).inp("w_ref", bt.wr).inp("w_target", wt)
        gb.out("lmbd_out", (K, S, 3 * N))
        for n in EV:
            gb.out(n, (B, N) if n == "w" else (B,), torch.int8 if n == "status" else torch.float64)
        gb.out("set_sum_w", (K * S * N,)).out("set_stats", (K * S * 8,)).build()
        plan = make_plan(bt, gb)
        rc = plan._lib.lompc_plan_run_chain(plan._plan, gb.ptr("lmbd"), gb.ptr("lmbd_r"), gb.ptr("w_target"), 0.5, K,
                                            gb.ptr("lmbd_out"), *outs(gb), plan._stream)
        assert rc == 0
        plan_ok(plan)
        gb.check_written("lmbd_out")
        lm = gb.np("lmbd_out")
        np.testing.assert_array_equal(lm[0], bt.lm[0])
        sw, st = gb.np("set_sum_w").reshape(K, S, N), gb.np("set_stats").reshape(K, S, 8)
        for k in range(1, K):  # the price rule, restated on the host (test_run_chain_rule_and_oracle)
            for s in range(S):
                if bt.off[s + 1] == bt.off[s]:
                    np.testing.assert_array_equal(lm[k, s], lm[k - 1, s])
                    continue
                c = bt.consts_of(s)
                wb = sw[k - 1, s] / st[k - 1, s, ST.LOMPC_STAT_COUNT]
                exp = np.maximum(0.0, lm[k - 1, s] + 0.5 * (phi(c, wb) - phi(c, wt[s])))
                np.testing.assert_allclose(lm[k, s], exp, rtol=1e-14, atol=1e-14 * c.theta)
        ats = [(bt, 0)] + [(at_prices(bt, lm[k]), 0) for k in range(1, K)]
        verify(f"chain N={N} last={last}", gb, ats, 0, S * N, 8 * S)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("mode", ["path", "direct"])
@pytest.mark.parametrize("entry", ["solve_batch", "run"])
def test_context_entries_extents(gpu, entry, mode, N):
    """lompc_set_params + lompc_solve_batch and lompc_run, PATH and DIRECT contexts: one call per EV type
    into the same guarded outputs, the second type's rows GAP rows behind the first's (the gap keeps the
    pattern), the large type's call first."""
    GAP = 7
    lompcs = contexts(N)[1] if mode == "path" else direct_contexts(N)
    for last in ROT:
        bt = batch(N, last)
        P, B = bt.P, bt.B
        a = int(bt.off[P])
        gb = arena(bt, ev_rows=B + GAP)
        lib = lompcs[0]._lib
        stream = torch.cuda.current_stream().cuda_stream
        for t in (1, 0):
            lo = lompcs[t]
            off = np.ascontiguousarray(bt.off[t * P:(t + 1) * P + 1] - bt.off[t * P])
            ea, eo = t * a, t * (a + GAP)  # the type's first EV; its first output row
            par = (P, gb.ptr("lmbd", (1 * bt.S + t * P) * 3 * N), gb.ptr("lmbd_r", bt.S + t * P), gb.ptr("w_ref", t * P * N), None)
            bat = (int(off[-1]), gb.ptr("gamma", ea), off.ctypes.data, gb.ptr("w", eo * N), gb.ptr("cost", eo), gb.ptr("w0", eo),
                   gb.ptr("status", eo), gb.ptr("set_sum_w", t * P * N), gb.ptr("set_stats", t * P * 8), stream)
            if entry == "run":
                assert lib.lompc_run(lo._ctx, *par, *bat) == 0
            else:
                assert lib.lompc_set_params(lo._ctx, *par, stream) == 0
                assert lib.lompc_solve_batch(lo._ctx, *bat) == 0
            lo.S = P
            assert lo.check_last()[1:] == (0, 0)
        ev_at = np.concatenate([np.arange(a), np.arange(a, B) + GAP])
        verify(f"{entry} {mode} N={N} last={last}", gb, [(bt, 1)], ev_at=ev_at)


@pytest.mark.parametrize("N", NS)
def test_sorted_sets_only_extents(gpu, N):
    """A SORTED_GAMMA plan with only set outputs (k_agg), single run and wide run_steps (k_aggs)."""
    for last in ROT:
        bt = batch(N, last, "sorted")
        S = bt.S
        gb = arena(bt, want=())
        plan = make_plan(bt, gb, sorted_gamma=True)
        assert plan.launches_per_run() == 2
        assert plan_run(plan, gb, 1) == 0
        plan_ok(plan)
        verify(f"sorted N={N} last={last}", gb, [(bt, 1)])
        gb = arena(bt, want=(), runs=K, sw_stride=S * N, st_stride=8 * S)
        plan = make_plan(bt, gb, sorted_gamma=True)
        assert run_steps(plan, gb, *strides(bt), K, 0, S * N, 8 * S) == 0
        plan_ok(plan)
        verify(f"sorted steps N={N} last={last}", gb, [(bt, k) for k in range(K)], 0, S * N, 8 * S)


def subsets(names):
    return [tuple(n for i, n in enumerate(names) if m >> i & 1) for m in range(1 << len(names))]


@pytest.mark.parametrize("N", [24, 13])
@pytest.mark.parametrize("form", ["run", "wide"])
def test_null_matrix(gpu, form, N):
    """All 16 subsets of {w, cost, w0, status}, each with both set outputs and with neither: the requested
    outputs meet the bars, nothing else is touched; no output at all returns without error."""
    bt = batch(N)
    B, S = bt.B, bt.S
    for want in subsets(EV):
        for sets in (True, False):
            name = f"null {form} N={N} {'+'.join(want) or 'none'} sets={sets}"
            if form == "run":
                gb = arena(bt, want, sets)
                plan = make_plan(bt, gb)
                assert plan_run(plan, gb, 1) == 0, name
                plan_ok(plan)
                verify(name, gb, [(bt, 1)])
            else:
                sws, sts = S * N, 8 * S
                gb = arena(bt, want, sets, runs=K, ev_stride=B, sw_stride=sws, st_stride=sts)
                plan = make_plan(bt, gb)
                assert run_steps(plan, gb, *strides(bt), K, B, sws, sts) == 0, name
                plan_ok(plan)
                verify(name, gb, [(bt, k) for k in range(K)], B, sws, sts)


@pytest.mark.parametrize("N", [24, 13])
@pytest.mark.parametrize("form", ["per_kernel", "warm_stepped", "cells6_path_fin", "close_in_eval", "close_in_finalize",
                                  "diag_repair", "sorted", "chain", "solve_batch path", "run path", "solve_batch direct",
                                  "run direct"])
def test_null_single_outputs(gpu, form, N):
    """The other forms with each single per-EV output and with none (set outputs kept where the form
    requires them: run_chain; dropped for the single outputs elsewhere).  sorted: a SORTED_GAMMA plan, which
    evaluates per EV as soon as one per-EV output is requested."""
    bt = batch(N, layout="sorted") if form == "sorted" else batch(N)
    B, S = bt.B, bt.S
    for want in [(n,) for n in EV] + [()]:
        name = f"null {form} N={N} {'+'.join(want) or 'none'}"
        sets = form == "chain" or not want
        if form in STEPS_FORMS:
            kw, flags = STEPS_FORMS[form]
            sws, sts = S * N, 8 * S
            gb = arena(bt, want, sets, runs=K, ev_stride=B, sw_stride=sws, st_stride=sts)
            plan = make_plan(bt, gb, **kw)
            assert run_steps(plan, gb, *strides(bt), K, B, sws, sts, flags) == 0, name
            plan_ok(plan)
            verify(name, gb, [(bt, k) for k in range(K)], B, sws, sts)
        elif form in PLAN_FORMS or form == "sorted":
            gb = arena(bt, want, sets)
            plan = make_plan(bt, gb, **(dict(sorted_gamma=True) if form == "sorted" else PLAN_FORMS[form]))
            assert plan_run(plan, gb, 1) == 0, name
            plan_ok(plan)
            verify(name, gb, [(bt, 1)], status_is=ST.LOMPC_QP_REPAIRED if form == "diag_repair" else None)
        elif form == "chain":
            wt = np.concatenate([c.w_max * (0.2 + 0.6 * np.random.default_rng(N).random((bt.P, N))) for c in bt.cs])
            gb = Guarded().inp("gamma", bt.gn).inp("lmbd", bt.lm[0]).inp("lmbd_r", bt.lr[0]).inp("w_ref", bt.wr)
            gb.inp("w_target", wt).out("lmbd_out", (K, S, 3 * N))
            for n in want:
                gb.out(n, (B, N) if n == "w" else (B,), torch.int8 if n == "status" else torch.float64)
            gb.out("set_sum_w", (K * S * N,)).out("set_stats", (K * S * 8,)).build()
            plan = make_plan(bt, gb)
            assert plan._lib.lompc_plan_run_chain(plan._plan, gb.ptr("lmbd"), gb.ptr("lmbd_r"), gb.ptr("w_target"), 0.5, K,
                                                  gb.ptr("lmbd_out"), *outs(gb), plan._stream) == 0, name
            plan_ok(plan)
            gb.check_written("lmbd_out")
            lm = gb.np("lmbd_out")
            verify(name, gb, [(bt, 0)] + [(at_prices(bt, lm[k]), 0) for k in range(1, K)], 0, S * N, 8 * S)
        else:  # the small type's sets through its context
            entry, mode = form.split()
            lo = (contexts(N)[1] if mode == "path" else direct_contexts(N))[0]
            P, a = bt.P, int(bt.off[bt.P])
            sub = Batch.__new__(Batch)
            sub.__dict__.update(bt.__dict__)
            sub.cs, sub.gn, sub.off, sub.B = bt.cs[:1], bt.gn[:a], bt.off[:P + 1], a
            sub.lm, sub.lr, sub.wr, sub._oracle = bt.lm[:, :P], bt.lr[:, :P], bt.wr[:P], {}
            gb = arena(sub, want, sets)
            stream = torch.cuda.current_stream().cuda_stream
            par = (P, gb.ptr("lmbd", P * 3 * N), gb.ptr("lmbd_r", P), gb.ptr("w_ref"), None)
            bat = (a, gb.ptr("gamma"), sub.off.ctypes.data, *outs(gb), stream)
            if entry == "run":
                assert lo._lib.lompc_run(lo._ctx, *par, *bat) == 0, name
            else:
                assert lo._lib.lompc_set_params(lo._ctx, *par, stream) == 0
                assert lo._lib.lompc_solve_batch(lo._ctx, *bat) == 0, name
            lo.S = P
            assert lo.check_last()[1:] == (0, 0)
            verify(name, gb, [(sub, 1)])


@pytest.mark.parametrize("N", [24, 13])
def test_run_steps_strides(gpu, N):
    """lompc_plan_run_steps, K = 3, with every stride larger than its record: ev_stride = B + 3 (the gap rows
    and scalars keep the pattern), set strides S N + 5 and 8 S + 3, price strides 3 N S + 7 and S + 1 with
    NaN in the padding; one lmbd_r for all runs (stride 0); ev_stride = B - 1 refused, nothing written."""
    bt = batch(N)
    B, S = bt.B, bt.S
    evs, sws, sts, lms, lrs = B + 3, S * N + 5, 8 * S + 3, 3 * N * S + 7, S + 1
    lm = np.full((K, lms), np.nan)
    lm[:, :3 * N * S] = bt.lm.reshape(K, -1)
    lr = np.full((K, lrs), np.nan)
    lr[:, :S] = bt.lr
    for flags in (0, ST.LOMPC_STEPS_PER_KERNEL):
        gb = arena(bt, runs=K, ev_stride=evs, sw_stride=sws, st_stride=sts, lm=lm, lr=lr)
        plan = make_plan(bt, gb)
        assert run_steps(plan, gb, lms, lrs, K, evs, sws, sts, flags) == 0
        plan_ok(plan)
        verify(f"strides N={N} flags={flags}", gb, [(bt, k) for k in range(K)], evs, sws, sts)
    # one lmbd_r for all runs
    one = Batch.__new__(Batch)
    one.__dict__.update(bt.__dict__)
    one.lr, one._oracle = np.repeat(bt.lr[:1], K, axis=0), {}
    gb = arena(one, runs=K, ev_stride=evs, sw_stride=sws, st_stride=sts, lm=lm, lr=bt.lr[:1])
    plan = make_plan(one, gb)
    assert run_steps(plan, gb, lms, 0, K, evs, sws, sts) == 0
    plan_ok(plan)
    verify(f"strides N={N} lmbd_r_stride=0", gb, [(one, k) for k in range(K)], evs, sws, sts)
    # ev_stride < B: refused before anything is launched
    gb = arena(bt, runs=K, ev_stride=B, sw_stride=sws, st_stride=sts, lm=lm, lr=lr)
    plan = make_plan(bt, gb)
    assert run_steps(plan, gb, lms, lrs, K, B - 1, sws, sts) == ST.LOMPC_ERR_INVALID_ARG
    assert plan._lib.lompc_plan_last_error(plan._plan)
    torch.cuda.synchronize()
    gb.check_bands()
    for n in EV + ("set_sum_w", "set_stats"):
        gb.check_untouched(n)


@pytest.mark.parametrize("N", [24, 48, 13])
def test_pointers_8_not_16_aligned(gpu, N):
    """Every device pointer 8 bytes off a 16-byte boundary (outputs, gamma, prices, w_ref; the row stores
    are 16-B instructions for even N): a single run and wide run_steps.  The calls are accepted and the
    results meet the bars — include/lompc_amd.h states 8-byte alignment as the requirement."""
    bt = batch(N)
    B, S = bt.B, bt.S
    gb = arena(bt, misalign=True)
    plan = make_plan(bt, gb)
    assert plan_run(plan, gb, 1) == 0
    plan_ok(plan)
    verify(f"misaligned run N={N}", gb, [(bt, 1)])
    sws, sts = S * N + 1, 8 * S + 1  # (odd strides: every run's records 8 bytes off the previous run's phase)
    gb = arena(bt, runs=K, ev_stride=B + 1, sw_stride=sws, st_stride=sts, misalign=True)
    plan = make_plan(bt, gb)
    assert run_steps(plan, gb, *strides(bt), K, B + 1, sws, sts) == 0
    plan_ok(plan)
    verify(f"misaligned steps N={N}", gb, [(bt, k) for k in range(K)], B + 1, sws, sts)


# ---------------------------------------------------------------------------------------------------
# the row path above LQ_DROP_OFF
LARGE = [(64, 0), (64, 1), (48, 1), (63, 1)]  # (N, EVs past the last batch a descriptor covers)


def large_sizes(N, B):
    """Both types' three uneven sets: no size a multiple of 1024, residues mod RU R not all alike."""
    V = 1 if N & 1 else 2
    q = EVAL_RU * (64 // (N // V))
    base = [int(B * f) // q * q + r for f, r in zip((0.07, 0.23, 0.2, 0.11, 0.3), (1, 2, 3, 1, 3))]
    sizes = base + [B - sum(base)]
    assert min(sizes) > 0 and all(m % 1024 for m in sizes) and len({m % q for m in sizes}) >= min(3, q)
    return sizes


@pytest.mark.parametrize("N,past", LARGE)
def test_rows_past_descriptor_range(gpu, N, past):
    """The row stores of batches at and past B N 8 = LQ_DROP_OFF (the plain-store path eval_block takes when
    w does not fit a buffer descriptor), every row and cost against oracle_c.path_run, a 2048-EV sample
    against the dense oracle; forms: lompc_plan_run, CLOSE_IN_EVAL, wide run_steps K = 2 with shared rows.
    Measured once on the MI355X, whole test with the host references: 1.12 s (N = 64, last descriptor
    batch; the first case also loads the libraries), 0.52 s (N = 64, first plain batch), 0.38 s (N = 48),
    0.54 s (N = 63); each form's run itself 10 ms or less.  Against the kernel before the plain stores
    clamped the row of the lanes past the row width, the N = 48 case failed with 80 042 rows off the bar,
    largest |dw| 0.15 and the 32 doubles behind w overwritten; the band behind w is
    what made that run safe."""
    B = LQ_DROP_OFF // (8 * N) + past
    assert (B * N * 8 > LQ_DROP_OFF) == bool(past) and ((B - 1) * N * 8 <= LQ_DROP_OFF)
    cs, lompcs = contexts(N)
    rng = np.random.default_rng(7000 + 10 * N + past)
    sizes = large_sizes(N, B)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    S, P = 6, 3
    ymax = np.repeat([c.y_max for c in cs], [off[P], B - off[P]])
    gn = ymax * rng.random(B)
    gn[off[:-1]] = 0.0                    # each set's first EV at gamma = 0 (the batch's first too)
    gn[off[1:] - 1] = ymax[off[1:] - 1]   # each set's last EV at gamma = y_max (the batch's last too)
    gn[off[:-1] + 5], gn[off[1:] - 7] = ymax[off[:-1] + 5], 0.0
    lm = np.stack([np.concatenate([c.theta * rng.random((P, 3 * N)) for c in cs]) for _ in range(2)])
    lm[:, 1, :N] = 0.0
    lr = 0.2 * rng.random((2, S)) * np.array([0.0, 1.0, 0.0, 1.0, 1.0, 0.0])
    wr = np.concatenate([c.w_max * rng.random((P, N)) for c in cs])
    t0 = time.perf_counter()
    # the reference: the host path engine, set by set in chunks, kept on the device
    Wr = torch.empty((B, N), dtype=torch.float64, device="cuda:0")
    Cr = torch.empty(B, dtype=torch.float64, device="cuda:0")
    CH = 1 << 19
    for s in range(S):
        o = None
        for a in range(int(off[s]), int(off[s + 1]), CH):
            b = min(a + CH, int(off[s + 1]))
            o = oracle_c.path_run(N, [cs[s // P]], [1], lm[1, s][None], lr[1, s:s + 1], gn[a:b], np.array([0, b - a], dtype=np.int64),
                                  out=o)
            assert o["info"][3] == 0
            Wr[a:b].copy_(torch.from_numpy(o["w"]))
            Cr[a:b].copy_(torch.from_numpy(o["cost"]))
    o0 = oracle_c.path_run(N, list(cs), [P, P], lm[0], lr[0], gn, off, want_w=False, want_cost=False)  # run 0: the set sums
    ref_sw = torch.stack([Wr[a:b].sum(0) for a, b in zip(off[:-1], off[1:])]).cpu().numpy()
    ref_sc = np.array([float(Cr[a:b].sum()) for a, b in zip(off[:-1], off[1:])])
    # the sample of the dense oracle
    pick = np.unique(np.concatenate([off[:-1], off[1:] - 1, off[:-1] + 5, off[1:] - 7, [0, B - 1], rng.choice(B, 2100, replace=False)]))
    assert pick.size >= 2048
    sid = np.searchsorted(off, pick, side="right") - 1
    Wd, Cd = np.zeros((pick.size, N)), np.zeros(pick.size)
    for s in range(S):
        m = sid == s
        Wd[m], Cd[m], nf = oracle_c.solve_batch(N, cs[s // P], lm[1, s], float(lr[1, s]), gn[pick[m]])
        assert nf == 0
    pick_d = torch.as_tensor(pick, device="cuda:0")
    print(f"\nN={N} B={B} w bytes - LQ_DROP_OFF = {B * N * 8 - LQ_DROP_OFF}: references {time.perf_counter() - t0:.2f} s")

    gb = Guarded().inp("gamma", gn).inp("lmbd", lm).inp("lmbd_r", lr).inp("w_ref", wr)
    gb.out("w", (B, N)).out("cost", (B,)).out("status", (B,), torch.int8)
    gb.out("set_sum_w", (2 * S * N,)).out("set_stats", (2 * S * 8,)).build()
    bits = lambda t: t.view(torch.int64)
    fill = bits(gb._arena[torch.float64])[0].clone()
    counts = np.diff(off)
    for form in ("run", "close_in_eval", "steps"):
        t1 = time.perf_counter()
        for n in ("w", "cost", "set_sum_w", "set_stats"):
            bits(gb.view(n)).fill_(fill)
        gb.view("status").fill_(0x5A)
        plan = BatchPlan(list(lompcs), gb.view("gamma"), off, sets_per_ctx=[P, P], w_ref=gb.view("w_ref"), want_w=False,
                         want_cost=False, want_set=False, validate=False, close_in_eval=form == "close_in_eval")
        assert plan.gamma.data_ptr() == gb.ptr("gamma")
        ptrs = [gb.ptr("w"), gb.ptr("cost"), None, gb.ptr("status"), gb.ptr("set_sum_w"), gb.ptr("set_stats")]
        if form == "steps":
            rc = plan._lib.lompc_plan_run_steps(plan._plan, gb.ptr("lmbd"), S * 3 * N, gb.ptr("lmbd_r"), S, 2, 0, *ptrs, S * N,
                                                8 * S, 0, 0, plan._stream)
        else:
            rc = plan._lib.lompc_plan_run(plan._plan, gb.ptr("lmbd", S * 3 * N), gb.ptr("lmbd_r", S), *ptrs, plan._stream)
        assert rc == 0
        rep, fail, inv = plan.check()
        t_run = time.perf_counter() - t1
        dev = Dev(f"large {form} N={N} B={B}")
        # measured first, asserted after: mismatching rows, the largest |dw|, the band behind w
        w, cost = gb.view("w"), gb.view("cost")
        bad_rows, dmax, unwritten = 0, 0.0, 0
        for a in range(0, B, CH):
            b = min(a + CH, B)
            d = (w[a:b] - Wr[a:b]).abs()
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
            bad_rows += int((d.max(1).values > 1e-9).sum())
            dmax = max(dmax, float(d.max()))
            unwritten += int((bits(w[a:b]) == fill).sum())
        dc = (cost - Cr).abs()
        dc = torch.where(torch.isnan(dc), torch.full_like(dc, float("inf")), dc)
        band_ok = True
        try:
            gb.check_bands()
        except AssertionError as e:
            band_ok = str(e)
        print(f"  {form}: {t_run:.2f} s run + status; rows off the 1e-9 bar: {bad_rows}, largest |dw| {dmax:.3e}, elements never "
              f"written {unwritten}, bands intact: {band_ok}")
        dev.add("|dw| vs path_run", dmax, 1e-9)
        dev.add("cost vs path_run", dc.cpu().numpy(), 1e-9 + 1e-9 * Cr.abs().cpu().numpy())
        ws, cs_ = w[pick_d].cpu().numpy(), cost[pick_d].cpu().numpy()
        dev.add("|dw| vs dense oracle", np.abs(ws - Wd), 1e-9)
        dev.add("cost vs dense oracle", np.abs(cs_ - Cd), 1e-9 + 1e-9 * np.abs(Cd))
        nset = 2 if form == "steps" else 1
        sw = gb.np("set_sum_w")[:nset * S * N].reshape(nset, S, N)
        st = gb.np("set_stats")[:nset * S * 8].reshape(nset, S, 8)
        own_sw = torch.stack([w[a:b].sum(0) for a, b in zip(off[:-1], off[1:])]).cpu().numpy()
        own_sc = np.array([float(cost[a:b].sum()) for a, b in zip(off[:-1], off[1:])])
        dev.add("set sums", np.abs(sw[-1] - ref_sw), 1e-9 + 1e-10 * np.abs(ref_sw))
        dev.add("sum cost", np.abs(st[-1, :, ST.LOMPC_STAT_SUM_COST] - ref_sc), 1e-9 * np.maximum(1.0, np.abs(ref_sc)))
        dev.add("sums vs own rows", np.abs(sw[-1] - own_sw), 1e-9 + 1e-11 * np.abs(own_sw))
        dev.add("sums vs own rows", np.abs(st[-1, :, ST.LOMPC_STAT_SUM_COST] - own_sc), 1e-9 + 1e-11 * np.abs(own_sc))
        if form == "steps":  # run 0 of the shared rows: its set sums against the host engine's
            dev.add("set sums", np.abs(sw[0] - o0["set_sum_w"]), 1e-9 + 1e-10 * np.abs(o0["set_sum_w"]))
        for k in range(nset):
            np.testing.assert_array_equal(st[k, :, ST.LOMPC_STAT_COUNT], counts)
            assert np.all(st[k, :, ST.LOMPC_STAT_N_FAILED] == 0) and np.all(st[k, :, ST.LOMPC_STAT_N_INVALID] == 0)
        assert band_ok is True, band_ok
        assert unwritten == 0 and fail == 0 and inv == 0
        gb.check_written("cost")
        gb.check_written("status")
        gb.check_written("set_sum_w", np.arange(2 * S * N) < nset * S * N)
        gb.check_written("set_stats", np.arange(2 * S * 8) < nset * S * 8)
        gb.check_inputs()
        s_ = gb.view("status")
        assert bool(((s_ == ST.LOMPC_QP_OK) | (s_ == ST.LOMPC_QP_REPAIRED)).all())
        dev.check()
        del plan
