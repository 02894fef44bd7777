"""Timing of lompc_price_step_many (the price-gradient step of K QPs in one launch) against the only route such a
batch had before it, on the same seeded inputs, and of the per-EV price loops on top (personal_prices).  Not a
test; prints ONE JSON object (and writes it to --out).

Inputs per (EV type, N, K): lmbd ~ theta U[0,1]^{3N}, lmbd_r = 0, gamma ~ y_max U[0,1], w = lompc_solve_many's optimum
at them, w_ref = w_max (0.2 + 0.6 U[0,1]^N); both shipped EV types, N in {24, 48}, K in {4 096, 262 144}, r = 3N.

Routes
  price_step_many   lompc_price_step_many out of place with dec, state, iters and counts (no err: every QP steps): one
                    HIP-event pair around the call, median and range of 10 after one warm-up.  Beside it
                    lompc_solve_many (cold, with w and err) on the same batch, timed the same way.
  host route        what the parent offered: the D2H copy of w, a Python loop of the host lompc_price_step over the K
                    QPs, the H2D copy of the prices; wall time, K = 4 096 only (10 samples if one takes under 1 s,
                    else 3).  Any larger K is EXTRAPOLATED linearly from it.
  personal_prices   wall time of price_solver.personal_prices at K = 4 096, cap 60 (gamma = y_max (0.3 + 0.6 U)), after
                    one warm-up run; with the steps taken and the final states.

Every GPU step is a child process of its own under `timeout`; a step that ends abnormally (time limit, abort,
fault) ends the run: nothing more is started on the GPU, the object printed says where it stopped.

    python scripts/price_steps_timing.py [--out price_steps_timing.json]
"""
import argparse
import ctypes
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
SAMPLES = 10
CAP = 60
EPS_REG = 0.01


def inputs(ev, N, K):
    _, theta, y_max, w_max = TYPES[ev]
    rng = np.random.default_rng(9100 + N + (ev == "large"))  # (the K = 4 096 batch is the head of the larger one)
    lm = theta * rng.random((max(KS), 3 * N))[:K]
    g = y_max * rng.random(max(KS))[:K]
    wr = w_max * (0.2 + 0.6 * rng.random((max(KS), N))[:K])
    return lm, g, wr


def stat(x):
    x = np.asarray(x, dtype=float)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "samples": int(x.size)}


def make(ev, N):
    from lompc_amd import LoMPC, LoMPCConstants

    d, th, ym, wm = TYPES[ev]
    return LoMPC(N, LoMPCConstants(d, th, ym, wm, ev), device=0)


def solved(lo, ev, N, K):
    """The batch on the device with solve_many's optimum: (lm, g, wr, result)."""
    import torch

    lm, g, wr = (torch.as_tensor(a, device="cuda:0") for a in inputs(ev, N, K))
    return lm, g, wr, lo.solve_many(lm, 0.0, g, w_ref=wr, want_status=True)


def step_steps(ev, N, K):
    import torch

    lo = make(ev, N)
    dev = "cuda:0"
    lm, g, wr, sol = solved(lo, ev, N, K)
    w = sol["w"]
    nxt = torch.empty((K, 3 * N), dtype=torch.float64, device=dev)
    dec = torch.empty(K, dtype=torch.float64, device=dev)
    state = torch.zeros(K, dtype=torch.int8, device=dev)
    iters = torch.zeros(K, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    err = torch.empty(K, dtype=torch.float64, device=dev)
    w2 = torch.empty_like(w)
    stream = lo._stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call_step():
        rc = lo._lib.lompc_price_step_many(lo._ctx, K, 3 * N, EPS_REG, w.data_ptr(), wr.data_ptr(), lm.data_ptr(), 3 * N,
                                           None, None, 0.0, nxt.data_ptr(), 3 * N, dec.data_ptr(), state.data_ptr(),
                                           iters.data_ptr(), counts.data_ptr(), stream)
        if rc:
            raise RuntimeError(f"lompc_price_step_many -> {rc}")

    def call_many():
        rc = lo._lib.lompc_solve_many(lo._ctx, K, lm.data_ptr(), 3 * N, None, g.data_ptr(), wr.data_ptr(), None, 0,
                                      w2.data_ptr(), None, None, None, err.data_ptr(), None, None, stream)
        if rc:
            raise RuntimeError(f"lompc_solve_many -> {rc}")

    def timed(call, before=None):
        us = []
        for _ in range(SAMPLES + 1):  # the first is the warm-up
            if before:
                before()
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return stat(us[1:])

    t_step = timed(call_step, before=lambda: state.zero_())
    n = counts.cpu().numpy().tolist()
    if n[3] or sum(n) != K:  # (a QP without a certificate is reported in "states", not an error of the timing)
        raise RuntimeError(f"price_step_many: states {n}")
    t_many = timed(call_many)
    return {"price_step_many_us": t_step, "solve_many_cold_us": t_many, "states": n,
            "steps_per_s": K / (t_step["median"] * 1e-6)}


def step_host(ev, N, K):
    """The parent's route for the same K steps: w to the host, K host calls, the prices back."""
    import torch

    lo = make(ev, N)
    d, th, _, wm = TYPES[ev]
    lm, g, wr, sol = solved(lo, ev, N, K)
    lm_h, wr_h = lm.cpu().numpy(), wr.cpu().numpy()
    w_d = sol["w"]
    m = 2 * d * th ** 2
    lib = lo._lib
    out = np.empty((K, 3 * N))
    dec = ctypes.c_double(0.0)

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w_h = w_d.cpu().numpy()
        for k in range(K):
            rc = lib.lompc_price_step(N, 3 * N, th, wm, m, 0.0, EPS_REG, wr_h[k].ctypes.data, w_h[k].ctypes.data,
                                      lm_h[k].ctypes.data, out[k].ctypes.data, ctypes.byref(dec), None)
            if rc:
                raise RuntimeError(f"lompc_price_step -> {rc} at QP {k}")
        nxt = torch.as_tensor(out, device="cuda:0")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, nxt

    first, nxt = once()
    t = [once()[0] for _ in range(SAMPLES if first < 1e6 else 3)]
    # the same answers as the batched step
    res = lo.price_step_many(w_d, wr, lm, None, price_type="linear-convex")
    return {"host_route_wall_us": stat(t), "first_wall_us": first,
            "max_dx_vs_price_step_many": float((res["lmbd"] - nxt).abs().max()),
            "note": "D2H copy of w + a Python loop of lompc_price_step + H2D copy of the prices; any larger K is extrapolated"}


def step_loop(ev, N, K):
    import torch

    from lompc_amd.price_solver import personal_prices

    lo = make(ev, N)
    _, _, y_max, w_max = TYPES[ev]
    rng = np.random.default_rng(9200 + N + (ev == "large"))
    g = torch.as_tensor(y_max * (0.3 + 0.6 * rng.random(K)), device="cuda:0")
    wr = torch.as_tensor(w_max * (0.2 + 0.6 * rng.random((K, N))), device="cuda:0")
    t = []
    for _ in range(3):  # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = personal_prices(lo, "linear-convex", g, wr, 0.0, max_iter=CAP)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    it = res["iters"].cpu().numpy()
    return {"personal_prices_wall_us": stat(t[1:]), "cap": CAP, "solves": int(res["solves"]),
            "states": np.bincount(res["state"].cpu().numpy(), minlength=4).tolist(),
            "iters_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())],
            "wall_us_per_iteration": float(np.median(t[1:])) / max(1, int(res["solves"]))}


def run_step(args):
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("price_steps_timing: no HIP device (there is no CPU fallback)")
    torch.cuda.set_device(0)
    row = {"steps": step_steps, "host": step_host, "loop": step_loop}[args.step](args.ev, args.N, args.K)
    row["device"] = torch.cuda.get_device_name(0)
    print("RESULT " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["steps", "host", "loop"], help="(internal) one GPU step in this process")
    ap.add_argument("--ev", choices=list(TYPES))
    ap.add_argument("--N", type=int)
    ap.add_argument("--K", type=int)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    steps = [(ev, N, K, "steps") for ev in TYPES for N in NS for K in KS]
    steps += [(ev, N, KS[0], "host") for ev in TYPES for N in NS]
    steps += [(ev, N, KS[0], "loop") for ev in TYPES for N in NS]
    limit = {"steps": 180, "host": 240, "loop": 240}
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
    # the bar: at K = 4 096 the batched step's range lies wholly below the host route's, for both types and both N
    rows = {(r["ev"], r["N"], r["K"], r["route"]): r for r in res["rows"]}
    bar = []
    for ev in TYPES:
        for N in NS:
            s, h = rows.get((ev, N, KS[0], "steps")), rows.get((ev, N, KS[0], "host"))
            if not (s and h):
                continue
            big = rows.get((ev, N, KS[1], "steps"))
            scale = KS[1] / KS[0]
            bar.append({"ev": ev, "N": N, "K": KS[0], "price_step_many_us": s["price_step_many_us"],
                        "host_route_us": h["host_route_wall_us"],
                        "ratio_of_medians": h["host_route_wall_us"]["median"] / s["price_step_many_us"]["median"],
                        "below": bool(s["price_step_many_us"]["max"] < h["host_route_wall_us"]["min"]),
                        f"host_route_us_extrapolated_K{KS[1]}": h["host_route_wall_us"]["median"] * scale,
                        f"price_step_many_us_K{KS[1]}": big["price_step_many_us"]["median"] if big else None})
    res["bar_K4096"] = bar
    res["bar_met"] = bool(bar) and all(b["below"] for b in bar) and len(bar) == len(TYPES) * len(NS)
    dump()
    print(json.dumps(res))
    if res["stopped"]:
        raise SystemExit(f"price_steps_timing: stopped at {res['stopped']['step']} (exit {res['stopped']['exit']})")


if __name__ == "__main__":
    main()
