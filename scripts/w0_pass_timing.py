"""Timing of the station's w0 / price0 pass (ChargingStation._w0_both) at config 5's shape: the scalar
pass (LOMPC_PLAN_SCALAR_PASS, k_scalar) against the default evaluation, and against another build of the
library (the parent commit's), alternated in ONE process.

Workload (seeded): 2 097 152 EVs, N = 48, both EV types x 12 partitions in one plan, y0 ~ U[0.3, 0.5],
prices theta * rand, lmbd_r = 0; outputs w0 [B] + set_stats [S][8] (the default evaluation also gets the
set_sum_w [S][N] buffer the station's plan passes; the scalar pass takes none).  One lompc_plan_run per
sample.  Per variant and round two samples: one with HIP events around the call's launches (profiling
off: the span k_path .. the last launch), one with the plan's per-kernel profile on (each kernel's own
event pair).  Variants alternate inside every round, after `--warmup` untimed runs each.

    python scripts/w0_pass_timing.py --parent-lib /path/to/parent/liblompc_amd.so [--samples 8]

The parent's library: the parent commit checked out elsewhere and built with lompc_amd/build.py
(build(out=...)).  Without --parent-lib only this tree's two variants run.  Raw C ABI through ctypes, so
both libraries live in one process.  No GPU: the script fails (no fallback).  Prints one JSON line per
variant (median and range in microseconds) and a summary; --out writes the same lines to a file.

Also checks what must not change: the scalar pass's w0 bit for bit the default evaluation's (and the
parent's), the set sums to 1e-11 relative.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "incentive-design-mpc_amd"))

HBM_PEAK = 8.0e12   # B/s
COPY_RATE = 6.29e12  # B/s, the measured copy rate (MI355X_MICROARCH.md)
TYPES = [(0.05, 10.0, 0.9, 0.25, 0), (0.025, 50.0, 0.9, 0.15, 1)]  # delta, theta, y_max, w_max, ev_type


class Variant:
    def __init__(self, name, lib, flags, kernels, torch, data, pass_sum_w):
        self.name, self.lib, self.kernels, self.torch = name, lib, kernels, torch
        N, P, dev = data["N"], data["P"], data["dev"]
        self.ctx = []
        for d, th, ym, wm, ev in TYPES:
            c = ctypes.c_void_p()
            rc = lib.lompc_create(N, d, th, ym, wm, ev, dev.index, ctypes.byref(c))
            if rc:
                raise RuntimeError(f"{name}: lompc_create -> {rc}")
            self.ctx.append(c)
        self.stream = torch.cuda.current_stream().cuda_stream
        ctxs = (ctypes.c_void_p * 2)(*[c.value for c in self.ctx])
        spc = np.array([P, P], dtype=np.int64)
        self.plan = ctypes.c_void_p()
        B, S = data["B"], 2 * P
        rc = lib.lompc_plan_create(2, ctypes.cast(ctxs, ctypes.c_void_p), spc.ctypes.data, B, data["gamma"].data_ptr(),
                                   data["off"].ctypes.data, None, flags, self.stream, ctypes.byref(self.plan))
        if rc:
            raise RuntimeError(f"{name}: lompc_plan_create -> {rc}")
        self.w0 = torch.empty(B, dtype=torch.float64, device=dev)
        self.stats = torch.empty((S, 8), dtype=torch.float64, device=dev)
        self.sum_w = torch.empty((S, N), dtype=torch.float64, device=dev) if pass_sum_w else None
        self.data = data
        self.span_us, self.kern_us = [], {k: [] for k in kernels}
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(self):
        d = self.data
        rc = self.lib.lompc_plan_run(self.plan, d["lm"].data_ptr(), d["lr"].data_ptr(), None, None, self.w0.data_ptr(), None,
                                     self.sum_w.data_ptr() if self.sum_w is not None else None, self.stats.data_ptr(),
                                     self.stream)
        if rc:
            raise RuntimeError(f"{self.name}: lompc_plan_run -> {rc}: {self.lib.lompc_plan_last_error(self.plan)}")

    def check(self):
        r = [ctypes.c_int64(0) for _ in range(3)]
        rc = self.lib.lompc_plan_status(self.plan, self.stream, *[ctypes.byref(x) for x in r])
        if rc or r[1].value or r[2].value:
            raise RuntimeError(f"{self.name}: status rc {rc}, failed {r[1].value}, invalid {r[2].value}")
        return r[0].value

    def sample(self):
        torch = self.torch
        self.lib.lompc_plan_profile_enable(self.plan, 0)
        torch.cuda.synchronize()
        self.e0.record()
        self.run()
        self.e1.record()
        self.e1.synchronize()
        self.span_us.append(self.e0.elapsed_time(self.e1) * 1e3)
        self.lib.lompc_plan_profile_enable(self.plan, (1 << len(self.kernels)) - 1)
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        for k in range(len(self.kernels)):
            self.lib.lompc_plan_profile_read(self.plan, k, ctypes.byref(ms), ctypes.byref(n), 1)
        self.run()
        for k, name in enumerate(self.kernels):
            self.lib.lompc_plan_profile_read(self.plan, k, ctypes.byref(ms), ctypes.byref(n), 1)
            self.kern_us[name].append(ms.value * 1e3 if n.value else 0.0)

    def close(self):
        self.lib.lompc_plan_destroy(self.plan)
        for c in self.ctx:
            self.lib.lompc_destroy(c)


def stat(x):
    x = np.asarray(x, dtype=float)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="another build of liblompc_amd.so to alternate with (the parent commit's)")
    ap.add_argument("--evs", type=int, default=2097152)
    ap.add_argument("--horizon", type=int, default=48)
    ap.add_argument("--partitions", type=int, default=12)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.samples < 6:
        ap.error("--samples >= 6")
    import torch

    from lompc_amd import _lib

    if not torch.cuda.is_available():
        raise RuntimeError("w0_pass_timing: no HIP device (there is no CPU fallback)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    N, P, B = args.horizon, args.partitions, args.evs
    rng = np.random.default_rng(args.seed)
    per = [B // 2, B - B // 2]
    gam, lm, off, base = [], [], [0], 0
    for (d, th, ym, wm, ev), M in zip(TYPES, per):
        gam.append(ym - (0.3 + 0.2 * rng.random(M)))
        lm.append(th * rng.random((P, 3 * N)))
        off += [base + (M * p) // P for p in range(1, P + 1)]  # P partitions per type, small type first
        base += M
    data = dict(N=N, P=P, B=B, dev=dev, gamma=torch.as_tensor(np.concatenate(gam), device=dev),
                lm=torch.as_tensor(np.concatenate(lm), device=dev), lr=torch.zeros(2 * P, dtype=torch.float64, device=dev),
                off=np.asarray(off, dtype=np.int64))
    assert data["off"][-1] == B
    branch = _lib.load()
    K3, K4 = ("k_path", "k_eval", "k_finalize"), ("k_path", "k_eval", "k_finalize", "k_scalar")
    variants = []
    if args.parent_lib:
        parent = _lib.load(os.path.abspath(args.parent_lib))
        variants.append(Variant("parent", parent, 0, K3, torch, data, True))
    variants.append(Variant("branch flag off", branch, 0, K4, torch, data, True))
    variants.append(Variant("branch flag on", branch, _lib.LOMPC_PLAN_SCALAR_PASS, K4, torch, data, False))
    for v in variants:
        for _ in range(args.warmup):
            v.run()
        v.repaired = v.check()
    for _ in range(args.samples):
        for v in variants:
            v.sample()
    for v in variants:
        v.check()
    # what must not change
    on, ref = variants[-1], variants[0]
    same_bits = bool(torch.equal(on.w0.view(torch.int64), ref.w0.view(torch.int64)))
    a, b = on.stats.cpu().numpy(), ref.stats.cpu().numpy()
    sums_rel = float(np.max(np.abs(a[:, [1, 2]] - b[:, [1, 2]]) / np.maximum(np.abs(b[:, [1, 2]]), 1e-300)))
    counts_same = bool(np.array_equal(a[:, [0, 5, 6, 7]], b[:, [0, 5, 6, 7]]))
    lines = []
    for v in variants:
        ev = "k_scalar" if v.kern_us.get("k_scalar") and max(v.kern_us["k_scalar"]) > 0 else "k_eval"
        e = stat(v.kern_us[ev])
        row = {"variant": v.name, "evs": B, "N": N, "sets": 2 * P, "samples": args.samples, "repaired_per_run": v.repaired,
               "call_span_us": stat(v.span_us), "evaluation_kernel": ev, "evaluation_us": e,
               "kernels_us": {k: stat(x) for k, x in v.kern_us.items()},
               "algorithmic_bytes": 16 * B, "frac_hbm_peak": 16 * B / (e["median"] * 1e-6) / HBM_PEAK,
               "frac_copy_rate": 16 * B / (e["median"] * 1e-6) / COPY_RATE}
        lines.append(row)
        print(json.dumps(row))
    summary = {"summary": True, "w0_bits_equal_to_" + ref.name.replace(" ", "_"): same_bits, "set_sums_max_rel_diff": sums_rel,
               "counts_equal": counts_same}
    lines.append(summary)
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    for v in variants:
        v.close()
    if not (same_bits and counts_same and sums_rel <= 1e-11):
        raise SystemExit("w0_pass_timing: the scalar pass's outputs differ from the reference variant's")


if __name__ == "__main__":
    main()
