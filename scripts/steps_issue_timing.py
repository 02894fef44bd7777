"""Diagnostics: the HOST time of one 100-run lompc_plan_run_steps call at config 3, many samples.

    [LOMPC_LIB=<library in lompc_amd/>] python scripts/steps_issue_timing.py

bench.py's host_issue_us_per_step is one timing of one such call per run; a process lands in one of two
modes some 2.6 us per call apart, so single readings of two libraries cannot be told apart.
This times the same call (both EV types in one plan, 12 sets each, 4 cells, w rows, per-run set outputs, the
span events the bench carries) 300 times, synchronised between calls, and prints the quantiles in us per call
as one JSON line.  Compare two libraries over several alternated processes each.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "incentive-design-mpc_amd"))
from lompc_amd import BatchPlan, LoMPC, LoMPCConstants  # noqa: E402

N, P, M, K = 24, 12, 131072, 100
rng = np.random.default_rng(0)
cs = (LoMPCConstants(0.05, 10.0, 0.9, 0.25, "small"), LoMPCConstants(0.025, 50.0, 0.9, 0.15, "large"))
lompcs = [LoMPC(N, c, device=0) for c in cs]
off = np.array([(2 * M * p) // (2 * P) for p in range(2 * P + 1)], dtype=np.int64)
g = torch.as_tensor(np.concatenate([c.y_max - (0.3 + 0.2 * rng.random(M)) for c in cs]), device="cuda")
lm = torch.as_tensor(np.concatenate([c.theta * rng.random((K, P, 3 * N)) for c in cs], axis=1), device="cuda")
lr = torch.zeros((K, 2 * P), dtype=torch.float64, device="cuda")
plan = BatchPlan(lompcs, g, off, sets_per_ctx=[P, P], cells=4, want_w=True, want_cost=True, want_set=True)
plan.profile(enable=("k_eval",))
call, res = plan.steps_call(lm, lr, K, 2 * P * 3 * N, 2 * P, per_run_sets=True, span_events=True)
for _ in range(5):
    call()
    torch.cuda.synchronize()
ts = []
for _ in range(300):
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    plan.profile(read=True, reset=True, kernel="k_eval")
    ts.append((t1 - t0) * 1e6)
assert plan.check()[1:] == (0, 0)
q = np.percentile(np.array(ts), [0, 10, 25, 50, 75, 90])
print(json.dumps({"lib": os.environ.get("LOMPC_LIB") or "liblompc_amd.so",
                  "issue_us_per_call": {k: round(float(v), 2) for k, v in zip(("min", "p10", "p25", "p50", "p75", "p90"), q)}}))
