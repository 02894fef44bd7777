"""Timing of lompc_solve_many (K QPs with their own prices in one launch) against the three routes such a
batch had before it, on the same seeded inputs.  Not a test; prints ONE JSON object (and writes it to --out).

Inputs per (EV type, N, K): lmbd ~ theta U[0,1]^{3N}, lmbd_r = 0, gamma ~ y_max U[0,1]; both shipped EV types,
N in {24, 48}, K in {4 096, 262 144}.

Routes
  solve_many cold / warm   lompc_solve_many with w, cost and status: one HIP-event pair around the call, median and
                           range of 10 after one warm-up.  Warm: LOMPC_MANY_WARM from the working sets the cold
                           solve left, after every price moved by 1 % (the sets are restored before each sample).
  solve_lompc loop         a Python loop of LoMPC.solve_lompc over the first 256 QPs: wall time per QP; the figure
                           for K QPs is EXTRAPOLATED from it (K times the per-QP time).
  set_params + solve_batch S = K parameter sets of one EV each (gamma_ref = gamma, set_offsets = arange(K + 1)), in PATH
                           and in DIRECT mode: an event pair around both calls, and the wall time.  At K = 262 144 the
                           route is timed only if one call finishes within 60 s ("skipped: over 60 s" otherwise); 10
                           samples if a call takes under 1 s, 3 under 10 s, else 1.

Every GPU step is a child process of its own under `timeout`; a step that ends abnormally (time limit, abort,
fault) ends the run: nothing more is started on the GPU, the object printed says where it stopped.

    python scripts/many_timing.py [--out many_timing.json]
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "incentive-design-mpc_amd"))

TYPES = {"small": (0.05, 10.0, 0.9, 0.25), "large": (0.025, 50.0, 0.9, 0.15)}  # delta, theta, y_max, w_max
NS = (24, 48)
KS = (4096, 262144)
LOOP_QPS = 256
SAMPLES = 10


def inputs(ev, N, K):
    _, theta, y_max, _ = TYPES[ev]
    rng = np.random.default_rng(9000 + N + (ev == "large"))  # (the K = 4 096 batch is the head of the larger one)
    lm = theta * rng.random((max(KS), 3 * N))[:K]
    g = y_max * rng.random(max(KS))[:K]
    lm2 = lm * (1.0 + 0.01 * rng.random((max(KS), 3 * N))[:K])
    return lm, np.zeros(K), g, lm2


def stat(x):
    x = np.asarray(x, dtype=float)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "samples": int(x.size)}


def make(ev, N, mode="path"):
    from lompc_amd import LoMPC, LoMPCConstants

    d, th, ym, wm = TYPES[ev]
    return LoMPC(N, LoMPCConstants(d, th, ym, wm, ev), device=0, mode=mode)


def step_many(ev, N, K):
    import torch

    from lompc_amd import _lib

    lo = make(ev, N)
    dev = "cuda:0"
    lm, lr, g, lm2 = (torch.as_tensor(a, device=dev) for a in inputs(ev, N, K))
    w = torch.empty((K, N), dtype=torch.float64, device=dev)
    cost = torch.empty(K, dtype=torch.float64, device=dev)
    status = torch.empty(K, dtype=torch.int8, device=dev)
    ws = torch.zeros((K, 64), dtype=torch.uint8, device=dev)
    stream = lo._stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(prices, flags, wsp):
        rc = lo._lib.lompc_solve_many(lo._ctx, K, prices.data_ptr(), 3 * N, lr.data_ptr(), g.data_ptr(), None, wsp, flags,
                                      w.data_ptr(), cost.data_ptr(), None, None, None, status.data_ptr(), None, stream)
        if rc:
            raise RuntimeError(f"lompc_solve_many -> {rc}")

    def timed(prices, flags, wsp, before=None):
        us = []
        for k in range(SAMPLES + 1):  # the first is the warm-up
            if before:
                before()
            torch.cuda.synchronize()
            e0.record()
            call(prices, flags, wsp)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return stat(us[1:])

    def tally():
        return np.bincount(status.cpu().numpy(), minlength=4).tolist()

    cold = timed(lm, 0, None)
    n_cold = tally()
    w_cold = w.clone()
    call(lm, 0, ws.data_ptr())  # the working sets at the first prices
    ws0 = ws.clone()
    warm = timed(lm2, _lib.LOMPC_MANY_WARM, ws.data_ptr(), before=lambda: ws.copy_(ws0))
    n_warm = tally()
    w_warm = w.clone()
    call(lm2, 0, None)  # the cold answer at the moved prices
    torch.cuda.synchronize()
    row = {"solve_many_cold_us": cold, "solve_many_warm_us": warm, "status_cold": n_cold, "status_warm": n_warm,
           "qps_cold": K / (cold["median"] * 1e-6), "qps_warm": K / (warm["median"] * 1e-6),
           "warm_vs_cold_max_dw": float((w_warm - w).abs().max())}
    if n_cold[2] or n_cold[3] or n_warm[2] or n_warm[3]:
        raise RuntimeError(f"solve_many: failed or invalid QPs {n_cold} {n_warm}")
    if K <= 4096:  # the same answers as the existing batched route
        lo.set_params(lm, lr, gamma_ref=g, validate=False)
        ref = lo.solve_batch(g, np.arange(K + 1, dtype=np.int64), want_set=False)
        row["max_dw_vs_solve_batch"] = float((ref["w"] - w_cold).abs().max())
    return row


def step_loop(ev, N, K):
    lo = make(ev, N)
    lm, lr, g, _ = inputs(ev, N, LOOP_QPS)
    lo.solve_lompc(lm[0], 0.0, g[0])  # warm-up
    t = []
    for k in range(LOOP_QPS):
        t0 = time.perf_counter()
        lo.solve_lompc(lm[k], 0.0, g[k])
        t.append((time.perf_counter() - t0) * 1e6)
    return {"solve_lompc_per_qp_wall_us": stat(t), "qps": 1e6 / float(np.median(t)),
            "note": f"wall time per QP over {LOOP_QPS} QPs; any K is extrapolated from it"}


def step_batch(ev, N, K, mode):
    import torch

    lo = make(ev, N, mode)
    dev = "cuda:0"
    lm, lr, g, _ = (torch.as_tensor(a, device=dev) for a in inputs(ev, N, K))
    off = np.arange(K + 1, dtype=np.int64)
    out = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        lo.set_params(lm, lr, gamma_ref=g, validate=False)
        lo.solve_batch(g, off, want_w=True, want_cost=True, want_status=True, want_set=False, out=out, check=False)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6

    _, first = once()
    if K > 4096 and first > 60e6:
        return {"skipped": "over 60 s", "first_call_wall_s": first * 1e-6}
    reps = SAMPLES if K <= 4096 or first < 1e6 else (3 if first < 10e6 else 1)
    ev_us, wall_us = zip(*[once() for _ in range(reps)])
    rep, fail, inv = lo.check_last()
    return {"events_us": stat(ev_us), "wall_us": stat(wall_us), "first_call_wall_us": first, "repaired": rep,
            "qps": K / (float(np.median(ev_us)) * 1e-6)}


def run_step(args):
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("many_timing: no HIP device (there is no CPU fallback)")
    torch.cuda.set_device(0)
    fn = {"many": step_many, "loop": step_loop, "path": lambda *a: step_batch(*a, "path"),
          "direct": lambda *a: step_batch(*a, "direct")}[args.step]
    row = fn(args.ev, args.N, args.K)
    row["device"] = torch.cuda.get_device_name(0)
    print("RESULT " + json.dumps(row))


def below(a, b):
    """Range a wholly below range b."""
    return a["max"] < b["min"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["many", "loop", "path", "direct"], help="(internal) one GPU step in this process")
    ap.add_argument("--ev", choices=list(TYPES))
    ap.add_argument("--N", type=int)
    ap.add_argument("--K", type=int)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    # the short steps first, the K = 262 144 runs of the existing routes last
    steps = [(ev, N, K, "many") for ev in TYPES for N in NS for K in KS]
    steps += [(ev, N, LOOP_QPS, "loop") for ev in TYPES for N in NS]
    steps += [(ev, N, KS[0], r) for ev in TYPES for N in NS for r in ("path", "direct")]
    steps += [(ev, N, KS[1], r) for r in ("path", "direct") for ev in TYPES for N in NS]
    limit = {"many": 240, "loop": 180, "path": 420, "direct": 420}
    res = {"date": datetime.date.today().isoformat(), "device": None, "rows": [], "stopped": None}

    def dump():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    for ev, N, K, step in steps:
        cmd = ["timeout", "-k", "10", str(limit[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--ev", ev,
               "--N", str(N), "--K", str(K)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            res["stopped"] = {"step": [ev, N, K, step], "exit": p.returncode, "stderr": p.stderr[-2000:]}
            break
        row = json.loads(line[-1][7:])
        res["device"] = row.pop("device")
        res["rows"].append({"ev": ev, "N": N, "K": K, "route": step, **row})
        dump()
    # the bar: at K = 4 096 solve_many's range lies wholly below each existing route's, for both N
    rows = {(r["ev"], r["N"], r["K"], r["route"]): r for r in res["rows"]}
    bar = []
    for ev in TYPES:
        for N in NS:
            m, lp = rows.get((ev, N, KS[0], "many")), rows.get((ev, N, LOOP_QPS, "loop"))
            pa, di = rows.get((ev, N, KS[0], "path")), rows.get((ev, N, KS[0], "direct"))
            if not (m and lp and pa and di):
                continue
            loop = {k: lp["solve_lompc_per_qp_wall_us"][k] * KS[0] for k in ("min", "median", "max")}
            for form in ("cold", "warm"):
                mr = m[f"solve_many_{form}_us"]
                bar.append({"ev": ev, "N": N, "K": KS[0], "form": form, "solve_many_us": mr,
                            "solve_lompc_loop_us_extrapolated": loop, "path_us": pa["events_us"], "direct_us": di["events_us"],
                            "below_all": bool(below(mr, loop) and below(mr, pa["events_us"]) and below(mr, di["events_us"]))})
    res["bar_K4096"] = bar
    res["bar_met"] = bool(bar) and all(b["below_all"] for b in bar) and len(bar) == 2 * len(TYPES) * len(NS)
    dump()
    print(json.dumps(res))
    if res["stopped"]:
        raise SystemExit(f"many_timing: stopped at {res['stopped']['step']} (exit {res['stopped']['exit']})")


if __name__ == "__main__":
    main()
