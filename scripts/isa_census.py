#!/usr/bin/env python3
"""Static instruction census of the plan kernels (CPU only: no device needed).

Compiles the device code of csrc/lompc_plan.hip to gfx950 assembly with the product's flags
(lompc_amd/build.py: -O3 -std=c++17, plus any -D given here) and prints, per named kernel, the instruction
counts by broad class (by mnemonic prefix: v_ vector ALU, s_ scalar, ds_ LDS, buffer_/global_/flat_/scratch_
vector memory), the lane reads and writes (SGPR spills live in VGPR lanes), DPP moves, plain moves, the
register and spill counts and the static LDS from the code object's metadata.

    python scripts/isa_census.py [-D NAME[=V]] [--kernels 'k_evals<24>' ...] [--asm FILE] [--keep FILE] [--json]

The compile takes a few minutes (the file instantiates every plan kernel).  --asm reads an assembly file
written earlier (--keep) instead of compiling.

    python scripts/isa_census.py --diff PARENT.s BRANCH.s [--rename 'REGEX=REPL' ...]

compares two --keep files kernel by kernel, for a change that must leave the generated code as it is: the
kernels in only one file, those whose normalised text differs (with the first differing lines) and those whose
kernel descriptor or resource counts differ; the exit status is non-zero if a kernel of both files differs.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = os.path.join(ROOT, "incentive-design-mpc_amd")
sys.path.insert(0, PKG_ROOT)
from lompc_amd import build as B  # noqa: E402

DEFAULT = ["k_evals<24>", "k_eval<false, 24>", "k_evals<0>"]
VMEM = ("buffer_", "global_", "flat_", "scratch_")
COLUMNS = ["VALU", "SALU", "LDS", "VMEM", "v_writelane", "v_readlane", "v_mov_dpp", "v_mov_b32", "v_mov_b64",
           "vgpr", "vgpr_spill", "sgpr", "sgpr_spill", "lds_bytes"]


def compile_asm(defines, out):
    cmd = [B._hipcc(), "-O3", f"--offload-arch={B.ARCH}", "-std=c++17", "-fPIC", "-Wno-unused-result"] + \
        [f"-D{d}" for d in defines] + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "lompc_plan.hip"), "-o", out]
    print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


def demangle(names):
    tool = os.path.join(os.path.dirname(os.path.realpath(B._hipcc())), "..", "llvm", "bin", "llvm-cxxfilt")
    tool = tool if os.path.exists(tool) else (shutil.which("llvm-cxxfilt") or shutil.which("c++filt"))
    if not tool:
        raise RuntimeError("no llvm-cxxfilt / c++filt to demangle the kernels' names")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def norm(name):
    """'void k_evals<24>(EvalArgs, EvalsArgs)' -> 'k_evals<24>' (spaces dropped)."""
    name = re.sub(r"^void\s+", "", name).replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", name).replace(" ", "")


def census(asm_text, wanted):
    meta = {}  # symbol -> metadata of the code object's notes
    for blk in re.split(r"\n  - \.agpr_count:", asm_text)[1:]:
        sym = re.search(r"\n\s+\.symbol:\s+(\S+)\.kd", blk)
        if not sym:
            continue
        get = lambda k: int(re.search(rf"\n\s+\.{k}:\s+(\d+)", blk).group(1))
        meta[sym.group(1)] = dict(vgpr=get("vgpr_count"), vgpr_spill=get("vgpr_spill_count"), sgpr=get("sgpr_count"),
                                  sgpr_spill=get("sgpr_spill_count"), lds_bytes=get("group_segment_fixed_size"))
    names = demangle(sorted(meta))
    by_short = {norm(v): k for k, v in names.items()}
    rows = {}
    for want in wanted:
        sym = by_short.get(want.replace(" ", ""))
        if sym is None:
            raise SystemExit(f"no kernel {want!r}; the file has: {sorted(by_short)}")
        m = re.search(rf"\n{re.escape(sym)}:.*?\n\.Lfunc_end\d+:", asm_text, re.S)
        c = dict.fromkeys(COLUMNS, 0)
        for line in m.group(0).split("\n"):
            line = line.strip()
            if not line or line[0] in ".;" or line.endswith(":"):
                continue
            op = line.split()[0]
            if op.startswith("v_"):
                c["VALU"] += 1
                if op.startswith("v_writelane"):
                    c["v_writelane"] += 1
                elif op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
                    c["v_readlane"] += op.startswith("v_readlane")
                elif op.startswith("v_mov_b32"):
                    c["v_mov_dpp" if ("dpp" in op or "row_" in line or "quad_perm" in line or "wave_" in line) else "v_mov_b32"] += 1
                elif op.startswith("v_mov_b64"):
                    c["v_mov_b64"] += 1
            elif op.startswith("s_"):
                c["SALU"] += 1
            elif op.startswith("ds_"):
                c["LDS"] += 1
            elif op.startswith(VMEM):
                c["VMEM"] += 1
        c.update(meta[sym])
        rows[want] = c
    return rows


def split_kernels(asm_text, renames):
    """kernel symbol -> (normalised body lines, descriptor {directive: value}).  Normalised away, because a
    kernel's place in the file or a renamed template sets them: comments, trailing blanks, the function index of
    .LBB<n>_ / .Ltmp<n> / .Lfunc_end<n>, the file-wide counter of .Lpost_getpc<n> (renumbered from the kernel's
    first) and the --rename substitutions."""
    for pat, repl in renames:
        asm_text = re.sub(pat, repl, asm_text)
    out = {}
    for m in re.finditer(r"\n\t\.amdhsa_kernel (\S+)\n(.*?)\n\t\.end_amdhsa_kernel", asm_text, re.S):
        sym = m.group(1)
        desc = dict(line.split()[:2] for line in m.group(2).split("\n"))
        # (and the resource counts set behind the function: num_vgpr, num_agpr, numbered_sgpr, private_seg_size, ...)
        desc.update((".amdhsa_" + k, v) for k, v in re.findall(rf"\n\t\.set {re.escape(sym)}\.(\w+), (\S+)", asm_text))
        text = re.search(rf"\n{re.escape(sym)}:.*?\n\.Lfunc_end\d+:", asm_text, re.S).group(0)
        text = text.replace(m.group(0), "")  # (the descriptor sits inside the function's text: compared apart)
        getpc = {}
        body = []
        for line in text.split("\n"):
            line = re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+", r".\1#", line.split(";")[0].rstrip())
            line = re.sub(r"\.Lpost_getpc(\d+)", lambda g: ".Lpost_getpc#%d" % getpc.setdefault(g.group(1), len(getpc)), line)
            if line:
                body.append(line)
        out[sym] = (body, desc)
    return out


def diff_asm(parent, branch, renames):
    """Compare two --keep files kernel by kernel (text only); the exit status: 1 if a kernel of both differs."""
    with open(parent) as f:
        pk = split_kernels(f.read(), renames)
    with open(branch) as f:
        bk = split_kernels(f.read(), renames)
    names = demangle(sorted(set(pk) | set(bk)))
    short = lambda s: norm(names[s])
    for tag, only in (("parent", sorted(set(pk) - set(bk))), ("branch", sorted(set(bk) - set(pk)))):
        print(f"only in the {tag}: {len(only)}" + "".join(f"\n  {short(s)}" for s in only))
    both = sorted(set(pk) & set(bk))
    n_text = n_desc = 0
    for s in both:
        (pb, pd), (bb, bd) = pk[s], bk[s]
        if pb != bb:
            n_text += 1
            i = next((k for k, (x, y) in enumerate(zip(pb, bb)) if x != y), min(len(pb), len(bb)))
            print(f"text differs: {short(s)}: {len(pb)} -> {len(bb)} lines, first at line {i + 1}")
            for k in range(i, i + 3):
                print(f"  - {pb[k] if k < len(pb) else ''}\n  + {bb[k] if k < len(bb) else ''}")
        dd = [k for k in sorted(set(pd) | set(bd)) if pd.get(k) != bd.get(k)]
        if dd:
            n_desc += 1
            print(f"descriptor differs: {short(s)}: " + ", ".join(f"{k[8:]} {pd.get(k)} -> {bd.get(k)}" for k in dd))
    print(f"in both: {len(both)} kernels; instruction text differs in {n_text}; descriptor differs in {n_desc}")
    return 1 if n_text or n_desc else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--kernels", nargs="+", default=DEFAULT)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the assembly here")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--diff", nargs=2, metavar=("PARENT.s", "BRANCH.s"), help="compare two --keep files kernel by kernel")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="--diff: a symbol rename applied to both files before they are compared")
    a = ap.parse_args()
    if a.diff:
        sys.exit(diff_asm(a.diff[0], a.diff[1], [r.split("=", 1) for r in a.rename]))
    if a.asm:
        path = a.asm
    else:
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="isa_census_"), "lompc_plan.s")
        compile_asm(a.defines, path)
    with open(path) as f:
        rows = census(f.read(), a.kernels)
    if not a.asm and not a.keep:
        shutil.rmtree(os.path.dirname(path))
    if a.json:
        print(json.dumps(rows))
        return
    w = max(len(k) for k in rows) + 2
    print(" " * w + " ".join(f"{c:>11}" for c in COLUMNS))
    for k, c in rows.items():
        print(f"{k:<{w}}" + " ".join(f"{c[x]:>11}" for x in COLUMNS))


if __name__ == "__main__":
    main()
