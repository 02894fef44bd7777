"""lompc_solve_many at the binding's surface (no GPU): the header declares the entry point and its flag, the
built library exports it, the ctypes signature has its 17 arguments, the ABI version did not move, and
LoMPC.solve_many takes the documented keywords."""
import inspect
import os
import re
import subprocess

from lompc_amd import LoMPC, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lompc_amd.h")


def header_text():
    with open(HEADER) as f:
        return f.read()


def header_define(name):
    m = re.search(rf"^#define {name} (\d+)\s*$", header_text(), re.M)
    assert m, f"{name} not defined in include/lompc_amd.h"
    return int(m.group(1))


def test_header_declares_and_library_exports():
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"^int lompc_solve_many\s*\((.*?)\);", src, flags=re.M | re.S)
    assert m, "include/lompc_amd.h does not declare lompc_solve_many"
    assert len(m.group(1).split(",")) == 17
    from lompc_amd import build

    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\sT\slompc_solve_many$", out, flags=re.M)


def test_signature_and_constant():
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert "lompc_solve_many" in sig
    res, args = sig["lompc_solve_many"]
    assert res is _lib._I and len(args) == 17
    assert args[1] is _lib._L and args[3] is _lib._L and args[8] is _lib._I  # K, lmbd_stride, flags
    assert all(a is _lib._P for i, a in enumerate(args) if i not in (1, 3, 8))
    assert _lib.LOMPC_MANY_WARM == header_define("LOMPC_MANY_WARM") == 1


def test_abi_version_stays():
    assert header_define("LOMPC_ABI_VERSION") == 5
    from lompc_amd import build

    build.build()
    assert _lib.ABI_VERSION == 5 and _lib.load().lompc_abi_version() == 5
    assert _lib.load().lompc_solve_many.argtypes == dict((n, a) for n, _, a in _lib.SIGNATURES)["lompc_solve_many"]


def test_keywords():
    p = inspect.signature(LoMPC.solve_many).parameters
    assert list(p) == ["self", "lmbd", "lmbd_r", "gamma", "w_ref", "ws", "warm", "want_w", "want_cost", "want_w0",
                       "want_price0", "want_status", "out", "check"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[4:])
    defaults = {"w_ref": None, "ws": None, "warm": False, "want_w": True, "want_cost": True, "want_w0": False,
                "want_price0": False, "want_status": False, "out": None, "check": True}
    assert {k: p[k].default for k in defaults} == defaults


def test_dropin_reexports_the_method():
    import importlib.util

    path = os.path.join(ROOT, "incentive-design-mpc_amd", "chargingstation", "lompc.py")
    spec = importlib.util.spec_from_file_location("_dropin_lompc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.LoMPC.solve_many is LoMPC.solve_many
