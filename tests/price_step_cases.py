"""Inputs of ONE price-gradient step that steer the price QP's solver into its second half (CPU and GPU).

The step (``lompc_price_step`` on the host, ``nnqp_wave`` in csrc/lompc_pricewave.hpp on the device) solves
min 1/2 x'Qx + q'x, x >= 0 by a primal-dual active set of at most 64 rounds from the start prices' free
set and, when that does not end in a certified point, by a primal active set from x = 0.  With random
``w`` and ``w_ref`` the first half always ends; near the loop's fixed point (``w_ref`` a rounding-sized
distance from the central QP's optimum at the start prices) it cycles and the second half runs.  The host
reports it: ``*iterations`` of ``lompc_price_step`` counts the first half's rounds first, so a value above 64
means the primal method ran (include/lompc_amd.h).

A case is a pure function of (constants, N, r, lmbd_r flag, family, seed):

* ``y0``: 8 charge levels, descending, spread over 0.04 y_max around a drawn centre; ``gamma_sc`` from them as
  ``lompc_oracle.set_charge_levels`` computes it;
* start prices ``theta * scale * U(0, 1)`` on rows < r with about 40 % exact zeros, rows >= r zero;
* ``w_c``: the CPU oracle's central optimum at those prices (``oracle_c.solve_batch`` at gamma_sc);
* ``w_ref`` by family — ``near-1e-9 / -1e-8 / -1e-6``: clip(w_c + s w_max normal, 0, w_max) at price scale 1;
  ``near-big``: s = 1e-8 at price scale 100; ``control``: w_max U(0, 1) (the first half ends: the same shapes
  keep it covered).

The grid: the shipped small and large constants and the A2-like set (delta 1e-4, theta 1000, y_max 0.75,
w_max 0.01: test_price_host.py's SMALL_DELTA, large), N in {5, 13, 24, 48, 64}, r in {2N, 3N}, lmbd_r = 0 and
1.5 N delta U(0, 1).  ``SEEDS`` holds, per cell and family, the first seed in 1..200 at which the host step
returns LOMPC_OK with ``iterations > 64`` (the fallback families) or ``<= 64`` (control), or None where no
seed does; scripts/select_price_step_cases.py finds them on the CPU and prints the record that
tests/test_gpu_price_step_cases.py keeps in its docstring.  No torch, no device code.
"""
import ctypes
import functools
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

import lompc_oracle as O
import oracle_c
import price_oracle as PO

CONSTS = {"small": O.small_consts(), "large": O.large_consts(),
          "a2": O.OracleConstants(1e-4, 1000.0, 0.75, 0.01, "large")}
HORIZONS = (5, 13, 24, 48, 64)
# family -> (s: the distance of w_ref from w_c in units of w_max, or None for control; price scale)
FAMILIES = {"near-1e-9": (1e-9, 1.0), "near-1e-8": (1e-8, 1.0), "near-1e-6": (1e-6, 1.0), "near-big": (1e-8, 100.0),
            "control": (None, 1.0)}
FALLBACK = tuple(f for f in FAMILIES if f != "control")
SEED_RANGE = range(1, 201)
PDAS_ROUNDS = 64  # lompc_price_step's iterations above this: the primal fallback ran
NEV = 8


def cells():
    """The grid's cells (constants, N, r / N, lmbd_r flag), in the order of SEEDS."""
    return [(cn, N, k, lf) for cn in CONSTS for N in HORIZONS for k in (2, 3) for lf in (0, 1)]


def required(cell):
    """The coverage condition: the cells that must carry at least one fallback case — every A2-like cell and
    the shipped-large lmbd_r = 0 cells other than (N 64, r 2N)."""
    cn, N, k, lf = cell
    return cn == "a2" or (cn == "large" and lf == 0 and (N, k) != (64, 2))


@dataclass(frozen=True)
class Case:
    cname: str
    N: int
    r: int
    lr_flag: int
    family: str
    seed: int
    consts: O.OracleConstants
    y0: np.ndarray       # (8,) descending
    gamma_sc: float
    lmbd_r: float
    start: np.ndarray    # (3N,) start prices, rows >= r zero
    w_c: np.ndarray      # (N,) the oracle's central optimum at the start prices
    cost_c: float        # its cost
    w_ref: np.ndarray    # (N,)

    @property
    def id(self):
        return f"{self.cname}-N{self.N}-r{self.r // self.N}N-lr{self.lr_flag}-{self.family}-s{self.seed}"

    @property
    def price_type(self):
        return "linear" if self.r == 2 * self.N else "linear-convex"

    @property
    def m(self):
        return 2 * self.consts.delta * self.consts.theta ** 2  # lompc.py's strong-convexity modulus

    @property
    def kappa(self):
        return self.lmbd_r / self.consts.delta


def central(N, c, lmbd, lmbd_r, gamma_sc):
    """The oracle's central QP at the prices lmbd (3N,): (w, cost)."""
    w, cost, nf = oracle_c.solve_batch(N, c, lmbd, lmbd_r, np.array([gamma_sc]))
    assert nf == 0
    return w[0].copy(), float(cost[0])


@functools.lru_cache(maxsize=None)
def make(cname, N, k, lr_flag, family, seed):
    c = CONSTS[cname]
    s, scale = FAMILIES[family]
    r = k * N
    rng = np.random.default_rng([seed, list(CONSTS).index(cname), N, k, lr_flag, list(FAMILIES).index(family)])
    centre = (0.2 + 0.5 * rng.random()) * c.y_max
    y0 = np.sort(centre + 0.04 * c.y_max * (rng.random(NEV) - 0.5))[::-1].copy()
    _, _, gamma_sc, _ = O.set_charge_levels(y0, c.y_max)
    lmbd_r = 1.5 * N * c.delta * rng.random() if lr_flag else 0.0
    start = np.zeros(3 * N)
    start[:r] = c.theta * scale * rng.random(r) * (rng.random(r) < 0.6)
    w_c, cost_c = central(N, c, start, lmbd_r, gamma_sc)
    if s is None:
        w_ref = c.w_max * rng.random(N)
    else:
        w_ref = np.clip(w_c + s * c.w_max * rng.standard_normal(N), 0.0, c.w_max)
    for a in (y0, start, w_c, w_ref):
        a.setflags(write=False)
    return Case(cname, N, r, lr_flag, family, seed, c, y0, float(gamma_sc), float(lmbd_r), start, w_c, cost_c, w_ref)


def host_step(case, w=None):
    """lompc_price_step at the case's start prices and w (default: the oracle's w_c):
    (rc, x (r,), decrease, iterations)."""
    from lompc_amd import _lib

    lib = _lib.load()
    c, N, r = case.consts, case.N, case.r
    w = np.ascontiguousarray(case.w_c if w is None else w, dtype=np.float64)
    w_ref = np.ascontiguousarray(case.w_ref)
    lm = np.ascontiguousarray(case.start[:r])
    out = np.empty(r)
    dec, it = ctypes.c_double(np.nan), ctypes.c_int(-1)
    rc = lib.lompc_price_step(N, r, c.theta, c.w_max, case.m, case.kappa, PO.EPS_REG, w_ref.ctypes.data, w.ctypes.data,
                              lm.ctypes.data, out.ctypes.data, ctypes.byref(dec), ctypes.byref(it))
    return rc, out, dec.value, it.value


def dense(case, w=None):
    """The reference's dense QP of the step at w (default w_c): (P, q, dual cost at the start prices)."""
    c, N = case.consts, case.N
    _, A_bar_inv = O.w_inner_product_metric(np.tril(np.ones((N, N))), c.delta, case.lmbd_r)
    return PO.price_qp_data(N, case.r, c.theta, c.w_max, case.m, A_bar_inv, case.w_ref,
                            case.w_c if w is None else w, case.start[: case.r])


def dense_oracle(case, w=None):
    """The dense oracle's step (Lawson-Hanson on the Cholesky factor): (x_o, decrease_o)."""
    c, N = case.consts, case.N
    _, A_bar_inv = O.w_inner_product_metric(np.tril(np.ones((N, N))), c.delta, case.lmbd_r)
    return PO.price_step(N, case.r, c.theta, c.w_max, case.m, A_bar_inv, case.w_ref, case.w_c if w is None else w,
                         case.start[: case.r])


def objective_exact(c, N, w, lmbd, lmbd_r, gamma):
    """``OracleLoMPC.objective`` (lompc.py:95-135) at w under the prices lmbd (3N,), term by term in exact
    rational arithmetic on the given doubles (0.9 of the small type's degradation term as the double it is)."""
    w = [Fraction(float(v)) for v in w]
    lm = [Fraction(float(v)) for v in lmbd]
    th, de, wm = Fraction(c.theta), Fraction(c.delta), Fraction(c.w_max)
    if c.ev_type == "small":
        cost = th ** 2 * sum((v / Fraction(0.9)) ** 2 for v in w)
    else:
        cost = (th * wm) ** 2 * sum(max(Fraction(0), v / wm - Fraction(0.125), Fraction(1.5) * v / wm - Fraction(0.375),
                                        2 * v / wm - Fraction(0.75)) for v in w)
    y, s = [], Fraction(0)
    for v in w:
        s += v
        y.append(s)
    cost += de * th ** 2 * (sum(v * v for v in y) - 2 * Fraction(float(gamma)) * sum(y))
    cost += th * (sum(a * b for a, b in zip(lm[:N], w)) + sum(a * (wm - b) for a, b in zip(lm[N:2 * N], w)))
    cost += 3 * th / (4 * wm) * sum(a * b * b for a, b in zip(lm[2 * N:], w))
    return cost + Fraction(float(lmbd_r)) * th ** 2 * sum(v * v for v in w)


def dec_actual_exact(case, lmbd_new, w_new):
    """dual_cost_decrease_actual of the first step (price_solver.py:133-138) from the start prices to lmbd_new
    (3N,): cost(lmbd_new, w_new) - cost(start, w_c) + (start - lmbd_new)' phi(w_ref), with w_new the oracle's
    central optimum at lmbd_new, evaluated exactly and rounded once.  Near the fixed point the three terms are
    of the size of the prices times theta w_max N (1.45e7 at 100 theta, N = 64, A2-like) and cancel to ~1e-16:
    summed in fp64, the restatement itself is off by several ulps of them (7e-9 there)."""
    c, N = case.consts, case.N
    th, wm = Fraction(c.theta), Fraction(c.w_max)
    wr = [Fraction(float(v)) for v in case.w_ref]
    phi_ref = [th * v for v in wr] + [th * (wm - v) for v in wr] + [3 * th / (4 * wm) * v * v for v in wr]
    dlm = [Fraction(float(a)) - Fraction(float(b)) for a, b in zip(case.start, lmbd_new)]
    return float(objective_exact(c, N, w_new, lmbd_new, case.lmbd_r, case.gamma_sc)
                 - objective_exact(c, N, case.w_c, case.start, case.lmbd_r, case.gamma_sc)
                 + sum(a * b for a, b in zip(dlm, phi_ref)))


def select(cell, family):
    """The first seed of SEED_RANGE whose host step certifies in the half the family is for:
    (seed or None, the host's iterations at it)."""
    for seed in SEED_RANGE:
        rc, _, _, it = host_step(make(*cell, family, seed))
        if rc == 0 and ((it > PDAS_ROUNDS) if family != "control" else (it <= PDAS_ROUNDS)):
            return seed, it
    return None, None


# cell -> the seeds of FAMILIES' order (near-1e-9, near-1e-8, near-1e-6, near-big, control); None: no seed in 1..200
SEEDS = {
    ('small', 5, 2, 0): (1, 31, None, 1, 1),
    ('small', 5, 2, 1): (29, 65, None, 4, 1),
    ('small', 5, 3, 0): (2, 21, 108, 1, 1),
    ('small', 5, 3, 1): (8, 127, None, 17, 1),
    ('small', 13, 2, 0): (5, 12, None, 1, 1),
    ('small', 13, 2, 1): (97, None, None, 22, 1),
    ('small', 13, 3, 0): (2, 1, None, 1, 1),
    ('small', 13, 3, 1): (122, 144, None, 4, 1),
    ('small', 24, 2, 0): (1, 76, None, 1, 1),
    ('small', 24, 2, 1): (194, None, None, 32, 1),
    ('small', 24, 3, 0): (7, 10, None, 1, 1),
    ('small', 24, 3, 1): (None, None, None, 41, 1),
    ('small', 48, 2, 0): (2, None, None, 1, 1),
    ('small', 48, 2, 1): (None, None, None, 141, 1),
    ('small', 48, 3, 0): (8, 81, None, 1, 1),
    ('small', 48, 3, 1): (None, None, None, 111, 1),
    ('small', 64, 2, 0): (3, None, None, 1, 1),
    ('small', 64, 2, 1): (None, None, None, 11, 1),
    ('small', 64, 3, 0): (16, None, None, 1, 1),
    ('small', 64, 3, 1): (None, None, None, 63, 1),
    ('large', 5, 2, 0): (1, 11, 39, 1, 1),
    ('large', 5, 2, 1): (12, 1, 44, 5, 1),
    ('large', 5, 3, 0): (1, 1, 9, 1, 1),
    ('large', 5, 3, 1): (3, 36, None, 1, 1),
    ('large', 13, 2, 0): (1, 4, 37, 1, 1),
    ('large', 13, 2, 1): (11, 19, None, 1, 1),
    ('large', 13, 3, 0): (1, 5, 3, 1, 1),
    ('large', 13, 3, 1): (6, 32, None, 1, 1),
    ('large', 24, 2, 0): (1, 1, None, 1, 1),
    ('large', 24, 2, 1): (22, 66, None, 11, 1),
    ('large', 24, 3, 0): (2, 8, None, 1, 1),
    ('large', 24, 3, 1): (34, 88, None, 4, 1),
    ('large', 48, 2, 0): (1, 33, None, 1, 1),
    ('large', 48, 2, 1): (None, None, None, 3, 1),
    ('large', 48, 3, 0): (1, 4, 14, 1, 1),
    ('large', 48, 3, 1): (30, None, None, 5, 1),
    ('large', 64, 2, 0): (2, 62, None, 1, 1),
    ('large', 64, 2, 1): (None, None, None, 3, 1),
    ('large', 64, 3, 0): (3, 3, None, 1, 1),
    ('large', 64, 3, 1): (75, None, None, 14, 1),
    ('a2', 5, 2, 0): (3, 2, 5, 1, 1),
    ('a2', 5, 2, 1): (1, 1, 26, 3, 1),
    ('a2', 5, 3, 0): (1, 2, 2, 1, 1),
    ('a2', 5, 3, 1): (5, 1, 1, 1, 1),
    ('a2', 13, 2, 0): (1, 1, 1, 1, 1),
    ('a2', 13, 2, 1): (1, 1, 21, 1, 1),
    ('a2', 13, 3, 0): (1, 1, 1, 1, 1),
    ('a2', 13, 3, 1): (1, 1, 7, 1, 1),
    ('a2', 24, 2, 0): (1, 1, 1, 1, 1),
    ('a2', 24, 2, 1): (1, 1, 13, 1, 1),
    ('a2', 24, 3, 0): (1, 1, 4, 1, 1),
    ('a2', 24, 3, 1): (1, 2, 26, 1, 1),
    ('a2', 48, 2, 0): (1, 1, 1, 1, 1),
    ('a2', 48, 2, 1): (1, 1, 35, 1, 1),
    ('a2', 48, 3, 0): (1, 1, 1, 1, 1),
    ('a2', 48, 3, 1): (1, 1, 10, 1, 1),
    ('a2', 64, 2, 0): (1, 1, 1, 1, 1),
    ('a2', 64, 2, 1): (1, 3, 8, 1, 1),
    ('a2', 64, 3, 0): (1, 1, 7, 1, 1),
    ('a2', 64, 3, 1): (1, 1, 73, 1, 1),
}


def committed():
    """Every committed case, in the grid's order."""
    return [make(*cell, fam, seed) for cell in cells() for fam, seed in zip(FAMILIES, SEEDS[cell]) if seed is not None]


def groups():
    """(constants, N, r / N) -> its committed cases (both lmbd_r flags): the batched form's calls."""
    out = {}
    for case in committed():
        out.setdefault((case.cname, case.N, case.r // case.N), []).append(case)
    return out
