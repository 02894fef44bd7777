"""LOMPC_STEPS_SCALAR_PASS at the binding's surface (no GPU): the constant is the header's, distinct from the
other steps flags, the ABI version did not move, and the Python entry points take the new keyword."""
import inspect
import os
import re

from lompc_amd import BatchPlan, _lib
from lompc_amd.price_solver import PriceSolver

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lompc_amd.h")


def header_define(name):
    with open(HEADER) as f:
        m = re.search(rf"^#define {name} (\d+)\s*$", f.read(), re.M)
    assert m, f"{name} not defined in include/lompc_amd.h"
    return int(m.group(1))


def test_constant_is_the_headers():
    assert _lib.LOMPC_STEPS_SCALAR_PASS == header_define("LOMPC_STEPS_SCALAR_PASS") == 4
    for other in ("LOMPC_STEPS_PER_KERNEL", "LOMPC_STEPS_SPAN_EVENTS"):
        assert getattr(_lib, other) == header_define(other)


def test_flags_are_distinct_bits():
    flags = [_lib.LOMPC_STEPS_PER_KERNEL, _lib.LOMPC_STEPS_SPAN_EVENTS, _lib.LOMPC_STEPS_SCALAR_PASS]
    assert all(f > 0 and f & (f - 1) == 0 for f in flags) and len(set(flags)) == 3


def test_abi_version_stays():
    assert header_define("LOMPC_ABI_VERSION") == 5
    from lompc_amd import build

    build.build()
    assert _lib.ABI_VERSION == 5 and _lib.load().lompc_abi_version() == 5


def test_keywords():
    for fn in (BatchPlan.run_steps, BatchPlan.steps_call):
        p = inspect.signature(fn).parameters["scalar_pass"]
        assert p.default is False
    assert list(inspect.signature(PriceSolver.get_w0_price0_many).parameters) == ["self", "lmbds", "lmbd_r"]
    assert list(inspect.signature(PriceSolver.get_w0_price0_many_device).parameters) == ["self", "lmbds", "lmbd_r"]
