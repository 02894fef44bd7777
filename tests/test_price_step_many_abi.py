"""lompc_price_step_many at the binding's surface (no GPU): the header declares the entry point with its 18
arguments and the four LOMPC_STEP_* values, the built library exports it, the ctypes signature matches, the ABI
version did not move, LoMPC.price_step_many and price_solver.personal_prices take the documented keywords with
the documented defaults, and the drop-in LoMPC carries the method."""
import inspect
import os
import re
import subprocess

from lompc_amd import LoMPC, _lib, price_solver, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lompc_amd.h")
STATES = {"LOMPC_STEP_RUNNING": 0, "LOMPC_STEP_CONVERGED": 1, "LOMPC_STEP_FAILED": 2, "LOMPC_STEP_INVALID": 3}


def header_text():
    with open(HEADER) as f:
        return f.read()


def header_define(name):
    m = re.search(rf"^#define {name} (\d+)\s*$", header_text(), re.M)
    assert m, f"{name} not defined in include/lompc_amd.h"
    return int(m.group(1))


def test_header_declares_and_library_exports():
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"^int lompc_price_step_many\s*\((.*?)\);", src, flags=re.M | re.S)
    assert m, "include/lompc_amd.h does not declare lompc_price_step_many"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 18
    assert args[0] == "lompc_ctx* ctx" and args[1] == "int64_t K" and args[2] == "int r" and args[3] == "double eps_reg"
    assert args[7] == "int64_t lmbd_stride" and args[10] == "double tol" and args[12] == "int64_t next_stride"
    assert args[14] == "int8_t* state" and args[15] == "int32_t* iters" and args[16] == "int64_t* counts"
    assert args[17] == "void* stream"
    for name, value in STATES.items():
        assert header_define(name) == value
    from lompc_amd import build

    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\sT\slompc_price_step_many$", out, flags=re.M)


def test_signature_and_constants():
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert "lompc_price_step_many" in sig
    res, args = sig["lompc_price_step_many"]
    assert res is _lib._I and len(args) == 18
    longs, ints, doubles = (1, 7, 12), (2,), (3, 10)  # K and the strides; r; eps_reg and tol
    assert all(args[i] is _lib._L for i in longs) and all(args[i] is _lib._I for i in ints)
    assert all(args[i] is _lib._D for i in doubles)
    assert all(a is _lib._P for i, a in enumerate(args) if i not in longs + ints + doubles)
    for name, value in STATES.items():
        assert getattr(_lib, name) == value


def test_abi_version_stays():
    assert header_define("LOMPC_ABI_VERSION") == 5
    from lompc_amd import build

    build.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 and lib.lompc_abi_version() == 5
    assert lib.lompc_price_step_many.argtypes == dict((n, a) for n, _, a in _lib.SIGNATURES)["lompc_price_step_many"]
    assert lib.lompc_price_step_many.restype is _lib._I


def test_keywords_of_price_step_many():
    p = inspect.signature(LoMPC.price_step_many).parameters
    assert list(p) == ["self", "w", "w_ref", "lmbd", "lmbd_r", "price_type", "err", "tol", "state", "iters", "eps_reg",
                       "out", "in_place"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[5:])
    assert p["price_type"].default is inspect.Parameter.empty  # required
    defaults = {"err": None, "tol": 0.0, "state": None, "iters": None, "eps_reg": settings.PRICE_SOLVER_EPS_REG,
                "out": None, "in_place": False}
    assert {k: p[k].default for k in defaults} == defaults


def test_keywords_of_personal_prices():
    p = inspect.signature(price_solver.personal_prices).parameters
    assert list(p) == ["lompc", "price_type", "gamma", "w_ref", "lmbd_r", "lmbd0", "max_iter", "eps_tol", "eps_reg"]
    assert all(p[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(p)[:5])
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[5:])
    defaults = {"lmbd0": None, "max_iter": settings.MAX_PRICE_SOLVER_ITERATIONS, "eps_tol": settings.PRICE_SOLVER_EPS_TOL,
                "eps_reg": settings.PRICE_SOLVER_EPS_REG}
    assert {k: p[k].default for k in defaults} == defaults
    assert (defaults["max_iter"], defaults["eps_tol"], defaults["eps_reg"]) == (1000, 0.01, 0.01)  # settings.py:14-17


def test_dropin_reexports_the_method():
    import importlib.util

    path = os.path.join(ROOT, "incentive-design-mpc_amd", "chargingstation", "lompc.py")
    spec = importlib.util.spec_from_file_location("_dropin_lompc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.LoMPC.price_step_many is LoMPC.price_step_many
