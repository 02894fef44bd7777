"""Structured and extreme price vectors for the plan kernels' oracle tests (CPU and GPU).

test_gpu_plan_horizons.py and its siblings draw every price as theta * rand: dense, tie-free, of
magnitude theta.  The product's price step is max(0, ...), so real prices hold exact zeros, ties and
flat stretches, and the capped loop of tests/golden/price_loop_long.npz drives one convex-price
component to FIXTURE_MAX_REL theta while the rest stay O(theta).  The families below put such vectors
in front of the engines directly.

Everything is deterministic from (N, EV type, seed).  A family is a 3N vector of the lambda_1,
lambda_2, lambda_3 blocks; each is used at lmbd_r = 0 and at 1.5 N delta.  No torch, no device code:
the CPU tests (test_oracle.py, test_path_cpu.py) and the GPU test (test_gpu_plan_prices.py) import it.
"""
import functools
import json
import os

import numpy as np

import lompc_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def fixture_max_rel():
    """The largest price, in units of theta, that the shipped long-loop fixture holds (its capped loop's
    final prices; the fixture's docstring rounds it to 3.9e5)."""
    with open(os.path.join(GOLDEN, "price_loop_long.json")) as f:
        meta = json.load(f)["cases"]
    arr = np.load(os.path.join(GOLDEN, "price_loop_long.npz"), allow_pickle=False)
    rel = 0.0
    for cls, m in meta.items():
        theta = (O.large_consts() if m["kind"] == "Large" else O.small_consts()).theta
        for k in ("prices", "next_prices", "prev_prices"):
            rel = max(rel, float(np.max(arr[f"{cls}_{k}"])) / theta)
    return rel


FIXTURE_MAX_REL = fixture_max_rel()
assert 3.8e5 < FIXTURE_MAX_REL < 4.0e5, FIXTURE_MAX_REL

# dense theta * rand times each of these; the last two are beyond what the product's loops produce
DENSE_RUNGS = (("dense_1", 1.0), ("dense_1e3", 1e3), ("dense_fixture_max", FIXTURE_MAX_REL), ("dense_1e7", 1e7),
               ("dense_1e9", 1e9))
BEYOND = ("dense_1e7", "dense_1e9")  # past the product's range: the engine may fail, never be silently wrong


def _blocks(N, l1=0.0, l2=0.0, l3=0.0):
    return np.concatenate([np.broadcast_to(np.asarray(x, dtype=np.float64), (N,)) for x in (l1, l2, l3)])


def _ramp(N, up):
    r = np.arange(N, dtype=np.float64) / max(N - 1, 1)
    return r if up else r[::-1].copy()


def _huge(block):
    def f(N, th, rng):
        lm = th * rng.random(3 * N)
        lm[block * N + N // 3] = FIXTURE_MAX_REL * th
        return lm
    return f


def _dense(mult):
    return lambda N, th, rng: mult * th * rng.random(3 * N)


def _half_zero(N, th, rng):
    lm = th * rng.random(3 * N)
    lm[rng.permutation(3 * N)[: (3 * N + 1) // 2]] = 0.0
    return lm


def _tie(N, th, rng):
    l = th * rng.random(N)
    return _blocks(N, l, l, 0.0)


def _two_level(N, th, rng):
    return _blocks(N, 0.5 * th * rng.integers(0, 2, N), 0.5 * th * rng.integers(0, 2, N), 0.0)


def _spike(N, th, rng):
    l1 = np.zeros(N)
    l1[N // 2] = th
    return _blocks(N, l1, 0.0, 0.0)


def _square(N, th, rng):
    t = np.arange(N) % 2
    return _blocks(N, th * t, 0.5 * th * (1 - t), 0.3 * th * t)


def _l1_zero(N, th, rng):
    lm = th * rng.random(3 * N)
    lm[:N] = 0.0
    return lm


def _l3_1e6(N, th, rng):
    lm = th * rng.random(3 * N)
    lm[2 * N:] *= 1e6
    return lm


def _per_entry(N, th, rng):
    return th * rng.random(3 * N) * 10.0 ** rng.integers(-8, 4, 3 * N)


# name -> f(N, theta, rng) -> (3N,) prices.  The order is the sets' order in the GPU plans.
FAMILIES = {
    # flat
    "flat": lambda N, th, rng: _blocks(N, 0.5 * th, 0.2 * th, 0.3 * th),
    "flat_l1": lambda N, th, rng: _blocks(N, 0.5 * th, 0.0, 0.0),
    "flat_l2": lambda N, th, rng: _blocks(N, 0.0, 0.5 * th, 0.0),
    # zeros and ties
    "tie_l1_l2": _tie,
    "half_zero": _half_zero,
    "two_level": _two_level,
    "ramp_l1_up": lambda N, th, rng: _blocks(N, th * _ramp(N, True), 0.0, 0.0),
    "ramp_l1_down": lambda N, th, rng: _blocks(N, th * _ramp(N, False), 0.0, 0.0),
    "ramp_l2_up": lambda N, th, rng: _blocks(N, 0.5 * th, th * _ramp(N, True), 0.0),
    "ramp_l2_down": lambda N, th, rng: _blocks(N, 0.5 * th, th * _ramp(N, False), 0.0),
    "ramp_l3_up": lambda N, th, rng: _blocks(N, 0.3 * th, 0.0, th * _ramp(N, True)),
    "ramp_l3_down": lambda N, th, rng: _blocks(N, 0.3 * th, 0.0, th * _ramp(N, False)),
    # one stage or one component
    "spike": _spike,
    "square": _square,
    "l1_zero": _l1_zero,
    "huge_l1": _huge(0),
    "huge_l2": _huge(1),
    "huge_l3": _huge(2),
    # scales
    "l3_1e6": _l3_1e6,
    "all_1e-12": _dense(1e-12),
    "per_entry": _per_entry,
}
FAMILIES.update({name: _dense(mult) for name, mult in DENSE_RUNGS})
PRODUCT = tuple(f for f in FAMILIES if f not in BEYOND)

CONSTS = {"small": O.small_consts, "large": O.large_consts}
N_GAMMA = 130


def _rng(N, ev_type, seed, what):
    return np.random.default_rng([int(seed), int(N), 0 if ev_type == "small" else 1, what])


def prices(family, N, ev_type, seed=0):
    """The family's (3N,) price vector for (N, EV type, seed)."""
    c = CONSTS[ev_type]()
    lm = np.ascontiguousarray(FAMILIES[family](N, c.theta, _rng(N, ev_type, seed, list(FAMILIES).index(family))))
    assert lm.shape == (3 * N,) and np.all(lm >= 0)
    return lm


def lmbd_rs(N, ev_type):
    """The two robustness prices every family is used at."""
    return (0.0, 1.5 * N * CONSTS[ev_type]().delta)


def gammas(N, ev_type, seed=0, n=N_GAMMA):
    """One set's gamma: 0 and y_max exactly, 13 values repeated 5 times, the rest uniform over
    [0, y_max]; shuffled."""
    c = CONSTS[ev_type]()
    rng = _rng(N, ev_type, seed, 1000 + n)
    g = np.concatenate([[0.0, c.y_max], np.repeat(c.y_max * rng.random(13), 5), c.y_max * rng.random(n - 67)])
    return rng.permutation(g)


def cases(N, ev_type, families=None, seed=0):
    """[(family, lmbd (3N,), lmbd_r)] over the families at both lmbd_r."""
    return [(f, prices(f, N, ev_type, seed), lr) for f in (families or FAMILIES) for lr in lmbd_rs(N, ev_type)]


def pinned_instance(N, ev_type):
    """The issue's pinned instances: theta * rand (seed N + 2), the lambda_3 component 2N + N // 3 at
    3.9e5 theta, 512 sorted gamma.  Returns (consts, lmbd, gamma)."""
    c = CONSTS[ev_type]()
    rng = np.random.default_rng(N + 2)
    lm = c.theta * rng.random(3 * N)
    lm[2 * N + N // 3] = 3.9e5 * c.theta
    return c, lm, np.sort(c.y_max * rng.random(512))
