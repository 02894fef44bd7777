"""lompc_price_loops at the binding's surface (no GPU): the symbol is exported and typed, the ctypes struct
has the layout of the header's lompc_price_loops_part, the ABI version did not move, and the Python entry
points exist with their keywords."""
import ctypes
import inspect
import os
import re

from lompc_amd import _lib, price_solver
from lompc_amd.charging_station import ChargingStation

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lompc_amd.h")

C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double}


def header_text():
    with open(HEADER) as f:
        return f.read()


def header_struct(name):
    """[(field, ctypes type)] of ``typedef struct name { ... } name;`` in the header, in order."""
    m = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header_text(), re.S)
    assert m, f"{name} not in include/lompc_amd.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:  # one pointer per declaration
            fields.append((decl.split("*")[-1].strip(), ctypes.c_void_p))
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", nm)
            fields.append((arr.group(1), C_TYPES[ctype] * int(arr.group(2))) if arr else (nm, C_TYPES[ctype]))
    return fields


def test_symbol_is_exported_and_typed():
    from lompc_amd import build

    build.build()
    lib = _lib.load()
    fn = lib.lompc_price_loops
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert re.search(r"int lompc_price_loops\(int n_parts, lompc_price_loops_part\* parts, int max_parts_per_launch,\s*"
                     r"int\* launches, void\* stream\);", header_text())


def test_struct_matches_the_header():
    want = header_struct("lompc_price_loops_part")
    got = list(_lib.PriceLoopsPart._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and ctypes.alignment(a) == ctypes.alignment(b), name

    class FromHeader(ctypes.Structure):
        _fields_ = want

    assert ctypes.sizeof(_lib.PriceLoopsPart) == ctypes.sizeof(FromHeader) == 120
    for name, _ in want:
        assert getattr(_lib.PriceLoopsPart, name).offset == getattr(FromHeader, name).offset, name
    # (the existing structs, read by the same parser: the parser itself is right)
    for struct, name in ((_lib.PriceLoopArgs, "lompc_price_loop_args"), (_lib.PriceChainPart, "lompc_price_chain_part")):
        assert [n for n, _ in struct._fields_] == [n for n, _ in header_struct(name)], name


def test_refusals_need_no_device():
    """n_parts < 0 and parts == NULL with n_parts > 0 are refused, n_parts == 0 is OK with *launches = 0:
    all before any device call."""
    from lompc_amd import build

    build.build()
    lib = _lib.load()
    launches = ctypes.c_int(7)
    assert lib.lompc_price_loops(-1, None, 0, ctypes.byref(launches), None) == _lib.LOMPC_ERR_INVALID_ARG
    assert lib.lompc_price_loops(2, None, 0, ctypes.byref(launches), None) == _lib.LOMPC_ERR_INVALID_ARG
    assert launches.value == 7
    arr = (_lib.PriceLoopsPart * 1)()  # (a NULL plan)
    assert lib.lompc_price_loops(1, ctypes.cast(arr, ctypes.c_void_p), 0, ctypes.byref(launches),
                                 None) == _lib.LOMPC_ERR_INVALID_ARG
    assert launches.value == 7
    assert lib.lompc_price_loops(0, None, 0, ctypes.byref(launches), None) == _lib.LOMPC_OK
    assert launches.value == 0
    assert lib.lompc_price_loops(0, None, 0, None, None) == _lib.LOMPC_OK


def test_abi_version_stays():
    assert re.search(r"^#define LOMPC_ABI_VERSION 5\s*$", header_text(), re.M)
    assert _lib.ABI_VERSION == 5


def test_python_entry_points():
    sig = inspect.signature(price_solver.compute_optimal_prices_parallel)
    assert list(sig.parameters)[:2] == ["jobs", "lmbd_r"]
    assert all(p.default is not inspect.Parameter.empty for p in list(sig.parameters.values())[2:])
    p = inspect.signature(ChargingStation.__init__).parameters["price_start"]
    assert p.default == "chained"
