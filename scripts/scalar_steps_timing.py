"""Timing of lompc_plan_run_steps' wide scalar form (LOMPC_STEPS_SCALAR_PASS, k_scalars) against the flagless
wide form (k_evals) on the SAME plan, the calls alternated in one process.

Workload (seeded, bench.py's recipe): B EVs, half per EV type, P partitions (parameter sets) per type, horizon
N, y0 ~ U[0.3, 0.5], prices theta * rand per run, lmbd_r = 0, a w_ref per set; the plan is created with
LOMPC_PLAN_SCALAR_PASS | LOMPC_PLAN_CELLS(cells).  One call = K runs with the outputs w0 in ONE shared buffer
(ev_stride = 0) and every run's set_stats.  Two shapes by default:

    config 3:  262 144 EVs, N = 24, 12 + 12 sets, 4 cells per set, K = 100
    config 5: 2 097 152 EVs, N = 48, 12 + 12 sets, 4 cells per set, K = 20

Per form and sample two calls: (b) one with profiling off between two HIP events — the whole call's wall time
per step, path and closing launches included; (a) one with LOMPC_STEPS_SPAN_EVENTS and the evaluation kernel's
profile on — the event pair around the first group's evaluation launch, per run (K_EVAL flagless, K_SCALAR
scalar).  The forms alternate: flagless, scalar, scalar, flagless, ...  after one warmup call of each.

    python scripts/scalar_steps_timing.py [--samples 8] [--parent-lib /path/to/parent/liblompc_amd.so]

With --parent-lib (the parent commit built with lompc_amd/build.py, build(out=...)) the single-run scalar pass
(lompc_plan_run, k_scalar) of both libraries is timed too, alternated, at each shape: k_scalar shares its body
with k_scalars.  Raw C ABI through ctypes.  No GPU: the script fails (no fallback).  Prints one JSON line per
(shape, form); --out writes the same lines to a file.  Checks what must not differ: the scalar call's w0 bit for
bit the flagless call's, set_stats counts equal, sums within 2 (1e-9 + 1e-11 |ref|), MAX_ERR within 1e-9.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "incentive-design-mpc_amd"))

TYPES = [(0.05, 10.0, 0.9, 0.25, 0), (0.025, 50.0, 0.9, 0.15, 1)]  # delta, theta, y_max, w_max, ev_type
SHAPES = {"config3": (262144, 24, 100), "config5": (2097152, 48, 20)}  # EVs, N, K


def stat(x):
    x = np.asarray(x, dtype=float)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "n": int(x.size)}


class Plan:
    """A scalar-pass plan of one library over the shape's data, with its outputs."""

    def __init__(self, lib, L, torch, d, cells):
        self.lib, self.L, self.torch, self.d = lib, L, torch, d
        N, P, B = d["N"], d["P"], d["B"]
        self.ctx = []
        for dl, th, ym, wm, ev in TYPES:
            c = ctypes.c_void_p()
            if lib.lompc_create(N, dl, th, ym, wm, ev, 0, ctypes.byref(c)):
                raise RuntimeError("lompc_create failed")
            self.ctx.append(c)
        self.stream = torch.cuda.current_stream().cuda_stream
        ctxs = (ctypes.c_void_p * 2)(*[c.value for c in self.ctx])
        spc = np.array([P, P], dtype=np.int64)
        self.plan = ctypes.c_void_p()
        flags = L.LOMPC_PLAN_SCALAR_PASS | L.LOMPC_PLAN_CELLS(cells)
        if lib.lompc_plan_create(2, ctypes.cast(ctxs, ctypes.c_void_p), spc.ctypes.data, B, d["gamma"].data_ptr(),
                                 d["off"].ctypes.data, d["wr"].data_ptr(), flags, self.stream, ctypes.byref(self.plan)):
            raise RuntimeError("lompc_plan_create failed")
        S, K = 2 * P, d["K"]
        dev = d["gamma"].device
        self.w0 = torch.empty(B, dtype=torch.float64, device=dev)
        self.stats = torch.empty((K, S, 8), dtype=torch.float64, device=dev)
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def err(self):
        return self.lib.lompc_plan_last_error(self.plan)

    def steps(self, flags):
        d = self.d
        S, N = 2 * d["P"], d["N"]
        rc = self.lib.lompc_plan_run_steps(self.plan, d["lm"].data_ptr(), S * 3 * N, d["lr"].data_ptr(), 0, d["K"], 0, None, None,
                                           self.w0.data_ptr(), None, None, self.stats.data_ptr(), 0, 8 * S, 0, flags, self.stream)
        if rc:
            raise RuntimeError(f"lompc_plan_run_steps -> {rc}: {self.err()}")

    def single(self):
        d = self.d
        rc = self.lib.lompc_plan_run(self.plan, d["lm"].data_ptr(), d["lr"].data_ptr(), None, None, self.w0.data_ptr(), None, None,
                                     self.stats.data_ptr(), self.stream)
        if rc:
            raise RuntimeError(f"lompc_plan_run -> {rc}: {self.err()}")

    def profile(self, mask):
        self.lib.lompc_plan_profile_enable(self.plan, mask)
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        for k in range(self.L.LOMPC_PLAN_KERNELS):
            self.lib.lompc_plan_profile_read(self.plan, k, ctypes.byref(ms), ctypes.byref(n), 1)

    def read(self, k):
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        self.lib.lompc_plan_profile_read(self.plan, k, ctypes.byref(ms), ctypes.byref(n), 1)
        return ms.value * 1e3, n.value

    def wall(self, call):
        self.torch.cuda.synchronize()
        self.e0.record()
        call()
        self.e1.record()
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1) * 1e3

    def check(self):
        r = [ctypes.c_int64(0) for _ in range(3)]
        rc = self.lib.lompc_plan_status(self.plan, self.stream, *[ctypes.byref(x) for x in r])
        if rc or r[1].value or r[2].value:
            raise RuntimeError(f"status rc {rc}, failed {r[1].value}, invalid {r[2].value}")

    def close(self):
        self.lib.lompc_plan_destroy(self.plan)
        for c in self.ctx:
            self.lib.lompc_destroy(c)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="config3,config5")
    ap.add_argument("--partitions", type=int, default=12)
    ap.add_argument("--cells", type=int, default=4)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.samples < 6:
        ap.error("--samples >= 6")
    import torch

    from lompc_amd import _lib as L

    if not torch.cuda.is_available():
        raise RuntimeError("scalar_steps_timing: no HIP device (there is no CPU fallback)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    branch = L.load()
    parent = L.load(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    SPAN, SCAL = L.LOMPC_STEPS_SPAN_EVENTS, L.LOMPC_STEPS_SCALAR_PASS
    lines, bad = [], False
    for shape in args.shapes.split(","):
        B, N, K = SHAPES[shape]
        P = args.partitions
        rng = np.random.default_rng(args.seed)
        gam, lm, wr, off, base = [], [], [], [0], 0
        for (dl, th, ym, wm, ev), M in zip(TYPES, [B // 2, B - B // 2]):
            gam.append(ym - (0.3 + 0.2 * rng.random(M)))
            lm.append(th * rng.random((K, P, 3 * N)))
            wr.append(wm * rng.random((P, N)))
            off += [base + (M * p) // P for p in range(1, P + 1)]
            base += M
        d = dict(N=N, P=P, B=B, K=K, gamma=torch.as_tensor(np.concatenate(gam), device=dev),
                 lm=torch.as_tensor(np.concatenate(lm, axis=1), device=dev), wr=torch.as_tensor(np.concatenate(wr), device=dev),
                 lr=torch.zeros(2 * P, dtype=torch.float64, device=dev), off=np.asarray(off, dtype=np.int64))
        pl = Plan(branch, L, torch, d, args.cells)
        forms = {"flagless": (0, L.LOMPC_PLAN_K_EVAL), "scalar": (SCAL, L.LOMPC_PLAN_K_SCALAR)}
        out = {}
        for name, (fl, _) in forms.items():  # warmup, and what must not differ
            pl.profile(0)
            pl.steps(fl)
            pl.check()
            torch.cuda.synchronize()
            out[name] = (pl.w0.clone(), pl.stats.cpu().numpy().copy())
        same_w0 = bool(torch.equal(out["scalar"][0].view(torch.int64), out["flagless"][0].view(torch.int64)))
        a, b = out["scalar"][1], out["flagless"][1]
        counts_same = bool(np.array_equal(a[..., [0, 5, 6, 7]], b[..., [0, 5, 6, 7]]))
        sums = [L.LOMPC_STAT_SUM_W0, L.LOMPC_STAT_SUM_PRICE0, L.LOMPC_STAT_SUM_COST]
        # (each form's sums are held to 1e-9 + 1e-11 |ref| of its per-EV outputs, which are the same bits: twice that)
        sums_bar = float(np.max(np.abs(a[..., sums] - b[..., sums]) / (2e-9 + 2e-11 * np.abs(b[..., sums]))))
        sums_rel = float(np.max(np.abs(a[..., sums] - b[..., sums]) / np.maximum(np.abs(b[..., sums]), 1e-300)))
        max_err_diff = float(np.max(np.abs(a[..., L.LOMPC_STAT_MAX_ERR] - b[..., L.LOMPC_STAT_MAX_ERR])))
        bad |= not (same_w0 and counts_same and sums_bar <= 1.0 and max_err_diff <= 1e-9)
        ev_us = {k: [] for k in forms}
        wall_us = {k: [] for k in forms}
        ev_runs = {}
        for r in range(args.samples):
            for name in (("flagless", "scalar") if r % 2 == 0 else ("scalar", "flagless")):
                fl, kern = forms[name]
                pl.profile(0)
                wall_us[name].append(pl.wall(lambda: pl.steps(fl)) / K)
                pl.profile(1 << kern)
                pl.steps(fl | SPAN)
                torch.cuda.synchronize()
                us, n = pl.read(kern)
                other = pl.read(L.LOMPC_PLAN_K_EVAL if name == "scalar" else L.LOMPC_PLAN_K_SCALAR)[1]
                assert n > 0 and other == 0, (name, n, other)
                ev_us[name].append(us / n)
                ev_runs[name] = n
        pl.profile(0)
        pl.check()
        for name in forms:
            row = {"shape": shape, "evs": B, "N": N, "K": K, "sets": 2 * P, "cells": args.cells, "form": name,
                   "evaluation_us_per_run": stat(ev_us[name]), "span_runs": ev_runs[name], "call_us_per_step": stat(wall_us[name])}
            lines.append(row)
            print(json.dumps(row), flush=True)
        f_ev, f_wall = stat(ev_us["flagless"]), stat(wall_us["flagless"])
        s_ev, s_wall = stat(ev_us["scalar"]), stat(wall_us["scalar"])
        row = {"shape": shape, "summary": True, "w0_bits_equal": same_w0, "counts_equal": counts_same,
               "set_sums_max_rel_diff": sums_rel, "set_sums_max_of_bar": sums_bar, "max_err_max_abs_diff": max_err_diff,
               "evaluation_median_below_flagless_range": s_ev["median"] < f_ev["min"],
               "call_median_below_flagless_range": s_wall["median"] < f_wall["min"]}
        lines.append(row)
        print(json.dumps(row), flush=True)
        if parent is not None:  # the single-run scalar pass, parent against branch
            pp = Plan(parent, L, torch, d, args.cells)
            both = {"parent": pp, "branch": pl}
            t = {k: [] for k in both}
            for p_ in both.values():
                p_.profile(0)
                for _ in range(3):
                    p_.single()
            for r in range(max(args.samples, 10)):
                for name in (("parent", "branch") if r % 2 == 0 else ("branch", "parent")):
                    p_ = both[name]
                    p_.profile(1 << L.LOMPC_PLAN_K_SCALAR)
                    p_.single()
                    torch.cuda.synchronize()
                    us, n = p_.read(L.LOMPC_PLAN_K_SCALAR)
                    assert n == 1
                    t[name].append(us)
            for name in both:
                row = {"shape": shape, "single_run_k_scalar": name, "us": stat(t[name])}
                lines.append(row)
                print(json.dumps(row), flush=True)
            pp.close()
        pl.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    if bad:
        raise SystemExit("scalar_steps_timing: the scalar form's outputs differ from the flagless form's")


if __name__ == "__main__":
    main()
