"""CPU test of the scalar pass's C-ABI additions: constants only (no signature change, ABI version 5).

include/lompc_amd.h defines LOMPC_PLAN_SCALAR_PASS (64, a plan flag distinct from every other flag bit and
below the LOMPC_PLAN_CELLS field) and LOMPC_PLAN_K_SCALAR (3), LOMPC_PLAN_KERNELS is 4, and lompc_amd._lib
mirrors all three; BatchPlan names the kernel for profile()."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lompc_amd.h")


def defines():
    src = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"^#define (LOMPC_\w+)\s+(\d+)\b", src, flags=re.M)}


def test_header_defines_scalar_pass_constants():
    d = defines()
    assert d["LOMPC_PLAN_SCALAR_PASS"] == 64
    assert d["LOMPC_PLAN_K_SCALAR"] == 3
    assert d["LOMPC_PLAN_KERNELS"] == 4
    assert d["LOMPC_ABI_VERSION"] == 5
    flags = [d[n] for n in ("LOMPC_PLAN_WARM_START", "LOMPC_PLAN_DIAG_REPAIR", "LOMPC_PLAN_CLOSE_IN_EVAL",
                            "LOMPC_PLAN_SORTED_GAMMA", "LOMPC_PLAN_CLOSE_IN_FINALIZE", "LOMPC_PLAN_SCALAR_PASS")]
    assert all(f & (f - 1) == 0 for f in flags) and len(set(flags)) == len(flags)
    assert max(flags) < 1 << d["LOMPC_PLAN_CELLS_SHIFT"]
    assert sorted(d[n] for n in ("LOMPC_PLAN_K_PATH", "LOMPC_PLAN_K_EVAL", "LOMPC_PLAN_K_FINAL", "LOMPC_PLAN_K_SCALAR")) == \
        list(range(d["LOMPC_PLAN_KERNELS"]))


def test_lib_mirrors_scalar_pass_constants():
    from lompc_amd import _lib
    from lompc_amd.lompc import BatchPlan

    d = defines()
    for name in ("LOMPC_PLAN_SCALAR_PASS", "LOMPC_PLAN_K_SCALAR", "LOMPC_PLAN_KERNELS"):
        assert getattr(_lib, name) == d[name], name
    assert _lib.ABI_VERSION == 5
    assert BatchPlan.ALL_KERNELS.index("k_scalar") == _lib.LOMPC_PLAN_K_SCALAR
    assert len(BatchPlan.ALL_KERNELS) == _lib.LOMPC_PLAN_KERNELS
    assert BatchPlan.ALL_KERNELS[:3] == BatchPlan.KERNELS  # (the launch-count triples of the other tests)
