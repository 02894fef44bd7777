"""Which schedule a lompc_plan_run_steps call takes, pinned by its launch counts.

The schedules' outputs are bitwise equal by design, so the output tests cannot tell which one ran.  This file
pins it: for one call per table row the plan's HIP-event profile (k_path, k_eval, k_scalar, k_finalize launches)
and the change of info()["tail_launches"] must be the literal numbers of the row, and the call's set reductions
must be, bit for bit, those of a LOMPC_STEPS_PER_KERNEL call at the same prices on a fresh plan of the same kind.

Plans: 2 sets of 150 and 151 EVs of the small EV type (one evaluation block each), gamma uniform over
[0, y_max] with 0 and y_max exactly in each set; horizons 13 (the run-time-N instantiation) and 24.  The calls
are raw lompc_plan_run_steps calls with every output at a per-run stride, so a NULL output is NULL whatever the
plan was built with.

The accounting rules behind the numbers (a group is up to 64 runs, groups = ceil(K / 64)):
  (a) batched wide form: one k_paths launch per group counted once under k_path — a fused k_evals_tail launch
      counts as the NEXT group's path launch, so k_path reads `groups` either way and tail_launches grows by
      groups - 1 —, k_evals and k_closes each read as their group's runs (k_eval = k_finalize = K);
  (b) LOMPC_STEPS_SPAN_EVENTS: only the first group's evaluation launch carries k_eval events (min(K, 64));
  (c) LOMPC_STEPS_PER_KERNEL without w: the batched launches, one run per group (k_path = K, no fused launch;
      with (b) k_eval = 1);
  (d) the k_step forms (LOMPC_STEPS_PER_KERNEL with w, and warm-started plans): only the steady launches
      1 .. K - 1 carry k_eval events (K - 1; with the span flag one pair over the first path group's steady
      launches, min(K, 64) - 1); closings have no launch of their own (k_finalize = 0); the wide one takes a
      k_paths launch per group, the warm-started one none;
  (e) the k_path_fin form (cells no multiple of 4, or k_agg plans per kernel): k_path and k_eval once per run,
      every closing rides in the next run's path launch and the last one is not timed (k_finalize = 0);
  (f) k_aggs: one k_paths launch per group, the k_aggs launch read as its runs under k_eval, nothing else;
  (g) the wide scalar form: every launch read as its runs (k_path = k_scalar = k_finalize = K, k_eval = 0), a
      k_paths launch before every group (no fused launch); a per-call condition that fails (w given) leaves
      the call as without the flag.
"""
import functools

import numpy as np
import pytest
import torch

import lompc_oracle as O
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants, _lib

pytestmark = pytest.mark.gpu

SIZES = (150, 151)
K_MAX = 130
PK, SPAN, SC = _lib.LOMPC_STEPS_PER_KERNEL, _lib.LOMPC_STEPS_SPAN_EVENTS, _lib.LOMPC_STEPS_SCALAR_PASS
NAMES = ("k_path", "k_eval", "k_scalar", "k_finalize")

# the plan kinds: BatchPlan's keywords
KINDS = {
    "wide": dict(cells=4),
    "six": dict(cells=6),
    "warm": dict(cells=4, warm_start=True),
    "aggs": dict(cells=4, sort_sets=True),
    "scalar": dict(cells=4, scalar_pass=True),
}

# (plan kind, K, w given, steps flags, per-EV outputs given) -> ((k_path, k_eval, k_scalar, k_finalize), tail launches)
ROWS = [
    # unflagged plan, 4 cells, batched: rule (a)
    ("wide", 1, True, 0, True, (1, 1, 0, 1), 0),
    ("wide", 3, True, 0, True, (1, 3, 0, 3), 0),
    ("wide", 130, True, 0, True, (3, 130, 0, 130), 2),
    ("wide", 1, False, 0, True, (1, 1, 0, 1), 0),
    ("wide", 3, False, 0, True, (1, 3, 0, 3), 0),
    ("wide", 130, False, 0, True, (3, 130, 0, 130), 2),
    # ... with the span flag: rules (a), (b)
    ("wide", 1, True, SPAN, True, (1, 1, 0, 1), 0),
    ("wide", 3, True, SPAN, True, (1, 3, 0, 3), 0),
    ("wide", 130, True, SPAN, True, (3, 64, 0, 130), 2),
    ("wide", 1, False, SPAN, True, (1, 1, 0, 1), 0),
    ("wide", 3, False, SPAN, True, (1, 3, 0, 3), 0),
    ("wide", 130, False, SPAN, True, (3, 64, 0, 130), 2),
    # per kernel with w, one k_step per part and run: rule (d), wide
    ("wide", 1, True, PK, True, (1, 0, 0, 0), 0),
    ("wide", 3, True, PK, True, (1, 2, 0, 0), 0),
    ("wide", 130, True, PK, True, (3, 129, 0, 0), 0),
    ("wide", 1, True, PK | SPAN, True, (1, 0, 0, 0), 0),
    ("wide", 3, True, PK | SPAN, True, (1, 2, 0, 0), 0),
    ("wide", 130, True, PK | SPAN, True, (3, 63, 0, 0), 0),
    # per kernel without w, the batched launches one run per group: rule (c)
    ("wide", 1, False, PK, True, (1, 1, 0, 1), 0),
    ("wide", 3, False, PK, True, (3, 3, 0, 3), 0),
    ("wide", 130, False, PK, True, (130, 130, 0, 130), 0),
    ("wide", 1, False, PK | SPAN, True, (1, 1, 0, 1), 0),
    ("wide", 3, False, PK | SPAN, True, (3, 1, 0, 3), 0),
    ("wide", 130, False, PK | SPAN, True, (130, 1, 0, 130), 0),
    # unflagged plan, 6 cells, the k_path_fin form: rule (e)
    ("six", 1, True, 0, True, (1, 1, 0, 0), 0),
    ("six", 3, True, 0, True, (3, 3, 0, 0), 0),
    # warm-started plan, 4 cells, one k_step per run: rule (d), no k_paths launch
    ("warm", 1, True, 0, True, (0, 0, 0, 0), 0),
    ("warm", 3, True, 0, True, (0, 2, 0, 0), 0),
    # gamma-sorted sets, no per-EV output: k_aggs, rule (f); per kernel one k_path + k_agg per run, rule (e)
    ("aggs", 3, False, 0, False, (1, 3, 0, 0), 0),
    ("aggs", 130, False, 0, False, (3, 130, 0, 0), 0),
    ("aggs", 3, False, PK, False, (3, 3, 0, 0), 0),
    # scalar-pass plan: the wide scalar form, rule (g); with w the flag changes nothing, rule (a)
    ("scalar", 3, False, SC, True, (3, 0, 3, 3), 0),
    ("scalar", 130, False, SC, True, (130, 0, 130, 130), 0),
    ("scalar", 3, True, SC, True, (1, 3, 0, 3), 0),
]


def row_id(r):
    kind, K, w, flags, _, _, _ = r
    tags = [t for t, f in (("pk", PK), ("span", SPAN), ("sc", SC)) if flags & f]
    return "-".join([kind, f"K{K}", "w" if w else "now"] + tags)


class Pop:
    """One horizon's population on the device: the context, gamma, K_MAX runs' prices."""

    def __init__(self, N):
        self.N = N
        rng = np.random.default_rng([29, N])
        c = O.small_consts()
        self.lompc = LoMPC(N, LoMPCConstants(c.delta, c.theta, c.y_max, c.w_max, c.ev_type), device=0)
        gs = []
        for m in SIZES:
            g = c.y_max * rng.random(m)
            g[m // 3], g[m - 1] = 0.0, c.y_max
            gs.append(g)
        self.S = len(SIZES)
        self.off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
        self.B = int(self.off[-1])
        self.g = torch.as_tensor(np.concatenate(gs), device="cuda:0")
        self.lm = torch.as_tensor(c.theta * rng.random((K_MAX, self.S, 3 * N)), device="cuda:0")
        self.lr = torch.as_tensor(0.2 * rng.random((K_MAX, self.S)) * (np.arange(self.S) % 2), device="cuda:0")

    def plan(self, kind):
        p = BatchPlan(self.lompc, self.g, self.off, want_w=False, want_cost=False, want_set=False, **KINDS[kind])
        assert p.cells == KINDS[kind]["cells"]
        return p

    def call(self, plan, kind, K, w, flags, per_ev):
        """One raw lompc_plan_run_steps call of the first K runs, every output per run; a scalar-pass plan has
        no set_sum_w.  Returns the outputs given."""
        N, S, B = self.N, self.S, self.B
        e = lambda shape, dt=torch.float64: torch.full(shape, -1, dtype=dt, device="cuda:0")
        o = {"w": e((K, B, N)) if w else None,
             "cost": e((K, B)) if per_ev else None,
             "status": e((K, B), torch.int8) if per_ev else None,
             "set_sum_w": None if kind == "scalar" else e((K, S, N)),
             "set_stats": e((K, S, _lib.LOMPC_SET_STATS))}
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = plan._lib.lompc_plan_run_steps(
            plan._plan, self.lm.data_ptr(), S * 3 * N, self.lr.data_ptr(), S, K, 0, ptr(o["w"]), ptr(o["cost"]), None,
            ptr(o["status"]), ptr(o["set_sum_w"]), ptr(o["set_stats"]), S * N, S * _lib.LOMPC_SET_STATS,
            B if (w or per_ev) else 0, flags, plan._stream)
        assert rc == 0, plan._lib.lompc_plan_last_error(plan._plan)
        assert plan.check()[1:] == (0, 0)
        return o


@functools.lru_cache(maxsize=None)
def pop(N):
    return Pop(N)


@functools.lru_cache(maxsize=None)
def per_kernel_sets(N, kind, K, w, sc, per_ev):
    """The set reductions of the LOMPC_STEPS_PER_KERNEL call on a fresh plan (shared; left unchanged)."""
    pp = pop(N)
    o = pp.call(pp.plan(kind), kind, K, w, PK | sc, per_ev)
    return o["set_sum_w"], o["set_stats"]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("row", ROWS, ids=row_id)
@pytest.mark.parametrize("N", [13, 24])
def test_schedule_of_a_call(gpu, N, row):
    kind, K, w, flags, per_ev, launches, tail = row
    pp = pop(N)
    plan = pp.plan(kind)
    plan.profile(enable=NAMES)
    for k in NAMES:
        plan.profile(read=True, reset=True, kernel=k)
    tail0 = plan.info()["tail_launches"]
    o = pp.call(plan, kind, K, w, flags, per_ev)
    n = tuple(plan.profile(read=True, reset=True, kernel=k)[1] for k in NAMES)
    plan.profile(enable=False)
    d_tail = plan.info()["tail_launches"] - tail0
    print(f"N {N} {row_id(row)}: launches {dict(zip(NAMES, n))}, tail launches {d_tail}")
    assert n == launches, (dict(zip(NAMES, n)), launches)
    assert d_tail == tail
    ref_sw, ref_st = per_kernel_sets(N, kind, K, w, flags & SC, per_ev)
    assert same_bits(o["set_stats"], ref_st), "set_stats"
    if ref_sw is not None:
        assert same_bits(o["set_sum_w"], ref_sw), "set_sum_w"
    assert float(o["set_stats"][:, :, _lib.LOMPC_STAT_COUNT].min()) == min(SIZES)  # (every run's closing wrote)
