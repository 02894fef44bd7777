"""The evaluation kernels' outputs, bit for bit, against arrays recorded from an earlier build.

tests/golden/evals_bits.npz (written by tests/golden/make_evals_bits.py on an MI355X, from the build of
commit 8707e13) holds the inputs and every output of the cases below.  The evaluation (eval_block: k_eval,
k_step, k_evals) may be re-arranged freely as long as every floating-point operation and its order stay:
this test then keeps passing against the SAME file.  The other suites compare a build with itself or
with the oracle at 1e-9; this one compares it with the recorded build, with np.array_equal (NaN equal to
NaN at the invalid EVs' outputs).

Cases (CASES): N = 24 (exact instantiation, two stages per lane) at 4, 16 and 20 cells per set (20: past
the staged capacity, so unstaged cells whose EVs are re-solved), N = 13 (generic, odd) and N = 48 at 16.
Both EV types in one plan.  Set sizes: at N = 24 / 4 cells 0, 1, 63, 65, 512, 513, 576, 1024, 1100 and a
second 65 (every wave and pass pattern of one block, and two blocks); elsewhere 0, 1, 63, 65, 513, 576.
gamma: uniform over [0, y_max] with 0 and y_max exactly; the large type's 65-EV set holds NaN, a negative
value and one above y_max (INVALID: the n_inv count, the NaN rows); three EVs of the 63-EV set are moved
outside their set's window after the plan's creation (re-solved: the fail list and the n_fail count),
and one set per type runs at a price family that leaves EVs uncovered (price_families: ramp_l1_down,
all_1e-12).  The generator asserts REPAIRED and INVALID statuses in every case.

Forms, all against the same recorded arrays: wide run_steps K = 3 with per-run rows; wide K = 66 with the
shared rows buffer (two groups of runs, the last run's rows remain; N = 24 / 4 cells and N = 13); the
per-kernel form; K single runs; reductions only (want_w = False: piece sums, its own recorded arrays).
Each case asserts the form from plan.info() and the launch counts, as test_gpu_plan_horizons.py.

What is recorded per case: cost, status, set_sum_w, set_stats and the plan's (repaired, failed, invalid)
tallies in full; w as one 64-bit hash per row (a sum of the row's bit patterns times odd constants: any
changed bit changes it) and, for the sets of at most 65 EVs, run 0's rows in full — whole rows of every
run would be some 12 MB.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import lompc_oracle as O
import price_families as PF
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, _lib

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evals_bits.npz")
FULL = ([0, 1, 63, 65, 512, 513], [576, 1024, 1100, 65])
SMALLER = ([1, 63, 513], [0, 65, 576])
# name: horizon, cells per set, (small type's set sizes, large type's), also K = 66
CASES = {
    "n24c4": (24, 4, FULL, True),
    "n24c16": (24, 16, SMALLER, False),
    "n24c20": (24, 20, SMALLER, False),
    "n13c16": (13, 16, SMALLER, True),
    "n48c16": (48, 16, SMALLER, False),
}
K3, KW = 3, 66
WRAP_RUNS = [0, 1, 2, 63, 64, 65]  # the runs of K = 66 whose set reductions are recorded
FAMILY = {"small": ("ramp_l1_down", 513), "large": ("all_1e-12", 576)}  # family prices: at the set of this size
FORMS = ["wide", "wide66", "per_kernel", "single", "reductions"]
ST = _lib


@functools.lru_cache(maxsize=None)
def contexts(N):
    cs = (O.small_consts(), O.large_consts())
    return cs, tuple(LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0) for c in cs)


def make_inputs(name):
    """The case's inputs (host arrays), deterministic from its name."""
    N, cells, sizes, wrap = CASES[name]
    rng = np.random.default_rng([7, N, cells])
    cs = (O.small_consts(), O.large_consts())
    K = KW if wrap else K3
    parts0, parts1, lms, lrs = [], [], [], []
    for c, ms in zip(cs, sizes):
        lm = c.theta * rng.random((K, len(ms), 3 * N))
        for j, m in enumerate(ms):
            g = c.y_max * rng.random(m)
            if m == 63:  # a narrow window; three EVs leave it after the plan's creation
                g = c.y_max - (0.3 + 0.2 * rng.random(m))
            if m >= 2 and m != 63:
                g[m // 3], g[m - 1] = 0.0, c.y_max
            g1 = g.copy()
            if m == 63:
                g1[[5, 31, 62]] = [0.01 * c.y_max, 0.0, 0.02 * c.y_max]
            if m == 65 and c.ev_type == "large":
                g1[[2, 40, 64]] = [np.nan, -0.1, c.y_max + 1e-9]
            parts0.append(g)
            parts1.append(g1)
            fam, at = FAMILY[c.ev_type]
            if m == at:
                for k in range(K):
                    lm[k, j] = PF.prices(fam, N, c.ev_type, seed=k)
        lms.append(lm)
        lrs.append(0.2 * rng.random((K, len(ms))) * (np.arange(len(ms)) % 2))
    P = [len(ms) for ms in sizes]
    S = sum(P)
    wr = np.concatenate([c.w_max * rng.random((p, N)) for c, p in zip(cs, P)])
    return dict(g0=np.concatenate(parts0), g1=np.concatenate(parts1),
                off=np.concatenate([[0], np.cumsum([len(x) for x in parts0])]).astype(np.int64),
                lm=np.concatenate(lms, axis=1), lr=np.concatenate(lrs, axis=1), wr=wr,
                sets_per_ctx=np.asarray(P, dtype=np.int64))


_MULT = np.array([((2 * t + 1) * 0x9E3779B97F4A7C15) % (1 << 64) for t in range(ST.LOMPC_MAX_N)], dtype=np.uint64)


def row_hash(w):
    """(..., N) float64 -> (...) uint64: the rows' bit patterns (NaN: one pattern) times odd constants, summed
    modulo 2^64."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    bits = w.view(np.uint64).copy()
    bits[np.isnan(w)] = np.uint64(0x7FF8000000000000)
    with np.errstate(over="ignore"):
        return (bits * _MULT[: w.shape[-1]]).sum(axis=-1, dtype=np.uint64)


def small_rows(off):
    """Indices of the EVs of the sets of at most 65 EVs."""
    idx = [np.arange(a, b) for a, b in zip(off[:-1], off[1:]) if b - a <= 65]
    return np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)


class Case:
    """A case's inputs on the device, and plans over them."""

    def __init__(self, name, inputs):
        self.name = name
        self.N, self.cells, _, self.wrap = CASES[name]
        self.inp = inputs
        self.cs, lompcs = contexts(self.N)
        self.lompcs = list(lompcs)
        dev = "cuda:0"
        self.off = np.ascontiguousarray(inputs["off"], dtype=np.int64)
        self.B, self.S = int(self.off[-1]), len(self.off) - 1
        self.lm = torch.as_tensor(np.ascontiguousarray(inputs["lm"]), device=dev)
        self.lr = torch.as_tensor(np.ascontiguousarray(inputs["lr"]), device=dev)
        self.wr = torch.as_tensor(np.ascontiguousarray(inputs["wr"]), device=dev)
        self.strides = (self.S * 3 * self.N, self.S)

    def plan(self, **kw):
        """A plan created over the valid gamma, whose gamma is then replaced in place (the run's)."""
        g = torch.as_tensor(np.ascontiguousarray(self.inp["g0"]), device="cuda:0")
        p = BatchPlan(self.lompcs, g, self.off, sets_per_ctx=[int(x) for x in self.inp["sets_per_ctx"]], w_ref=self.wr,
                      cells=self.cells, **kw)
        g.copy_(torch.as_tensor(np.ascontiguousarray(self.inp["g1"])))
        assert p.cells == self.cells
        return p


def tallies(plan):
    """(repaired, failed, invalid) since the previous read: lompc_plan_status (BatchPlan.check raises on them)."""
    rep, fail, inv = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    plan._lib.lompc_plan_status(plan._plan, plan._stream, ctypes.byref(rep), ctypes.byref(fail), ctypes.byref(inv))
    return np.array([rep.value, fail.value, inv.value], dtype=np.int64)


def counted(plan, call):
    """call()'s result, the plan's tallies after it and the launch counts (k_path, k_eval, k_finalize)."""
    plan.profile(enable=BatchPlan.KERNELS)
    for k in BatchPlan.KERNELS:
        plan.profile(read=True, reset=True, kernel=k)
    res = call()
    tl = tallies(plan)
    n = tuple(plan.profile(read=True, reset=True, kernel=k)[1] for k in BatchPlan.KERNELS)
    plan.profile(enable=False)
    return res, tl, n


def np_(t):
    return t.cpu().numpy()


def groups(K):
    return (K + 63) // 64


ROWS = dict(want_w=True, want_cost=True, want_status=True)


def run_form(cs, form):
    """One form's outputs: {name: array}, with its plan's info and launch counts under "_info", "_n"."""
    K = KW if form == "wide66" else K3
    if form == "reductions":
        p = cs.plan(want_w=False, want_cost=False)
        o, tl, n = counted(p, lambda: p.run_steps(cs.lm, cs.lr, K, *cs.strides, per_run_sets=True))
        return dict(red_set_sum_w=np_(o["set_sum_w"]), red_set_stats=np_(o["set_stats"]), red_tallies=tl, _info=p.info(), _n=n)
    p = cs.plan(**ROWS)
    if form == "single":
        assert p.launches_per_run() == 3
        outs = {k: [] for k in ("w", "cost", "status", "set_sum_w", "set_stats")}

        def call():
            for k in range(K):
                o = p.run(cs.lm[k], cs.lr[k])
                for key in outs:
                    outs[key].append(np_(o[key]).copy())

        _, tl, n = counted(p, call)
        r = {key: np.stack(v) for key, v in outs.items()}
    elif form == "wide66":
        o, tl, n = counted(p, lambda: p.run_steps(cs.lm, cs.lr, K, *cs.strides, per_run_sets=True))
        w = np_(o["w"])
        return dict(w66_hash=row_hash(w), cost66=np_(o["cost"]), status66=np_(o["status"]),
                    set_sum_w66=np_(o["set_sum_w"])[WRAP_RUNS], set_stats66=np_(o["set_stats"])[WRAP_RUNS], tallies66=tl,
                    _info=p.info(), _n=n)
    else:
        o, tl, n = counted(p, lambda: p.run_steps(cs.lm, cs.lr, K, *cs.strides, per_run=True,
                                                  per_kernel=form == "per_kernel"))
        r = {key: np_(o[key]) for key in ("w", "cost", "status", "set_sum_w", "set_stats")}
    w = r.pop("w")
    r.update(w_hash=row_hash(w), w_small=w[0][small_rows(cs.off)], tallies=tl, _info=p.info(), _n=n)
    return r


@functools.lru_cache(maxsize=None)
def recorded():
    return np.load(FIXTURE, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def case_of(name):
    rec = recorded()
    # the recorded inputs are make_inputs': the fixture and the code that describes it agree (of the K = 66
    # cases' prices the file keeps the runs WRAP_RUNS only: the rest are 0.4 MB of random numbers)
    inp = make_inputs(name)
    for k, v in inp.items():
        if k == "lm" and CASES[name][3]:
            v = v[WRAP_RUNS]
        assert np.array_equal(v, rec[f"{name}_{k}"], equal_nan=v.dtype.kind == "f"), (name, k)
    return Case(name, inp)


def expected_launches(form, K, staged):
    """(k_path, k_eval, k_finalize) launch counts of a form (test_gpu_plan_horizons.py's table)."""
    if form == "single":
        return (K, K, K)
    if form == "per_kernel":
        return (K, K, K) if staged else (groups(K), K - 1, 0)  # k_paths, then k_step's parts (steady launches timed)
    return (groups(K), K, K)  # k_paths per group, k_evals and k_closes as K runs


# (K = 66 is recorded at N = 24 / 4 cells and N = 13)
NAME_FORM = [(name, form) for name in CASES for form in FORMS if form != "wide66" or CASES[name][3]]


@pytest.mark.parametrize("name,form", NAME_FORM)
def test_outputs_equal_the_recorded_build(gpu, name, form):
    cs = case_of(name)
    rec = recorded()
    out = run_form(cs, form)
    info, n = out.pop("_info"), out.pop("_n")
    K = KW if form == "wide66" else K3
    print(f"{name} {form}: launches {n}, info {info}, tallies {[v.tolist() for k, v in out.items() if 'tallies' in k]}")
    assert not info["evals_staged"]
    if form != "single":
        assert info["steps_group"] == 1, info
    assert n == expected_launches(form, K, info["evals_staged"]), n
    for key, v in out.items():
        ref = rec[f"{name}_{key}"]
        assert v.dtype == ref.dtype and v.shape == ref.shape, (name, form, key, v.dtype, v.shape, ref.shape)
        same = np.array_equal(v, ref, equal_nan=v.dtype.kind == "f")
        if not same:
            bad = np.flatnonzero(~((v == ref) | ((v != v) & (ref != ref))).ravel())
            print(f"{name} {form} {key}: {bad.size} of {v.size} differ, first at {np.unravel_index(bad[0], v.shape)}: "
                  f"{v.ravel()[bad[0]]!r} vs recorded {ref.ravel()[bad[0]]!r}")
        assert same, (name, form, key)
    if form == "wide66":  # its first runs are the K = 3 runs
        assert np.array_equal(out["set_sum_w66"][:3], rec[f"{name}_set_sum_w"])
        assert np.array_equal(out["set_stats66"][:3], rec[f"{name}_set_stats"])
