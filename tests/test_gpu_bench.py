"""bench.py's plain run on the device: the result line and ``--dump-outputs``.

One small run (4 096 EVs, 3 timed steps) in a process of its own, as the benchmark is started: the
line carries the headline fields and none of the ``--full`` legs, ``--steps`` is the number of timed
steps, and the dumped arrays are the last step's outputs — fp64, the plan's shapes, and consistent
with each other (every EV counted in its set, the set sums equal to the sums of the dumped rows at
the suite's tolerance for the fused reductions, tests/test_gpu_pipeline.py check_reductions).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lompc_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dump(gpu, tmp_path):
    B, N, P, K = 4096, 24, 12, 3
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if not k.startswith("LOMPC_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
                        "--evs-per-gpu", str(B), "--dump-outputs", str(out)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "LoMPC QP solves/sec" and line["unit"] == "QP/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["steps"] == K and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    np.testing.assert_allclose(line["value"], B / (line["ms_per_step"] * 1e-3), rtol=1e-9)
    for leg in ("kernels", "contracts", "cpu_baseline", "direct_mode", "bimpc", "collective"):
        assert leg not in line, leg
    assert line["verified_steps"] == 0

    assert sorted(os.listdir(out)) == ["cost.npy", "set_stats.npy", "set_sum_w.npy", "w.npy"]
    a = {k: np.load(out / f"{k}.npy") for k in ("w", "cost", "set_sum_w", "set_stats")}
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["w"].shape == (B, N) and a["cost"].shape == (B,)
    assert a["set_sum_w"].shape == (2 * P, N) and a["set_stats"].shape == (2 * P, _lib.LOMPC_SET_STATS)
    assert all(np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    # the benchmark's sets: P equal partitions of each EV type's half (small first)
    M = B // 2
    off = np.array([(M * p) // P for p in range(P + 1)] + [M + ((B - M) * p) // P for p in range(1, P + 1)])
    st = a["set_stats"]
    assert np.array_equal(st[:, _lib.LOMPC_STAT_COUNT], np.diff(off))
    assert not st[:, _lib.LOMPC_STAT_N_FAILED].any() and not st[:, _lib.LOMPC_STAT_N_INVALID].any()
    w_max = np.repeat([0.25, 0.15], [M, B - M])[:, None]  # (real_time_price_control.py:26-39)
    assert (a["w"] >= -1e-9).all() and (a["w"] <= w_max + 1e-9).all()
    for s in range(2 * P):
        rows = slice(off[s], off[s + 1])
        np.testing.assert_allclose(a["set_sum_w"][s], a["w"][rows].sum(0), rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(st[s, _lib.LOMPC_STAT_SUM_COST], a["cost"][rows].sum(), rtol=1e-11, atol=1e-9)
