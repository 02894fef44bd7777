"""Writes tests/golden/evals_bits.npz: the inputs and outputs of tests/test_gpu_evals_bits.py's cases.

Run on an MI355X, on the build whose outputs are to be kept (the shipped file: commit 8707e13's, before
the evaluation's instruction stream was trimmed):

    python tests/golden/make_evals_bits.py [--out FILE]

The cases, forms and what is recorded are test_gpu_evals_bits.py's (imported from it, so the generator and
the test cannot drift apart).  Before it records anything the generator asserts, from this build's statuses,
that every case holds REPAIRED and INVALID EVs and re-solved EVs in each type's family-priced set, and that
the forms which must agree bit for bit (wide, per kernel, single runs) do agree on this build.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "incentive-design-mpc_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_evals_bits as T  # noqa: E402
from lompc_amd import _lib as ST  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.FIXTURE)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    rec, problems = {}, []
    for name, (N, cells, sizes, wrap) in T.CASES.items():
        inp = T.make_inputs(name)
        cs = T.Case(name, inp)
        for k, v in inp.items():  # (K = 66: the prices of the runs whose reductions are kept; the test re-derives all)
            rec[f"{name}_{k}"] = v[T.WRAP_RUNS] if k == "lm" and wrap else v
        outs = {}
        for form in T.FORMS:
            if form == "wide66" and not wrap:
                continue
            o = T.run_form(cs, form)
            info, n = o.pop("_info"), o.pop("_n")
            print(f"{name} {form}: launches {n} (the test expects "
                  f"{T.expected_launches(form, T.KW if form == 'wide66' else T.K3, info['evals_staged'])}), info {info}, "
                  f"tallies {[v.tolist() for k, v in o.items() if 'tallies' in k]}", flush=True)
            outs[form] = o
        wide = outs["wide"]
        status, off = wide["status"], cs.off
        n_rep, n_inv = int(np.sum(status == ST.LOMPC_QP_REPAIRED)), int(np.sum(status == ST.LOMPC_QP_INVALID))
        n_failed = int(np.sum(status == ST.LOMPC_QP_FAILED))
        fam = {}
        for c, ms, s0 in zip(cs.cs, sizes, (0, len(sizes[0]))):
            s = s0 + list(ms).index(T.FAMILY[c.ev_type][1])
            fam[c.ev_type] = int(np.sum(status[0, off[s]:off[s + 1]] == ST.LOMPC_QP_REPAIRED))
        print(f"{name}: B {cs.B}, REPAIRED {n_rep}, INVALID {n_inv}, FAILED {n_failed}; REPAIRED in the family-priced "
              f"sets (run 0) {fam}; N_FAILED / N_INVALID per set (run 0) "
              f"{wide['set_stats'][0, :, ST.LOMPC_STAT_N_FAILED].astype(int).tolist()} / "
              f"{wide['set_stats'][0, :, ST.LOMPC_STAT_N_INVALID].astype(int).tolist()}", flush=True)
        if not (n_rep >= 3 * 3 and n_inv == 3 * 3):  # (asserted below, after every case has printed its line)
            problems.append((name, "REPAIRED / INVALID", n_rep, n_inv))
        if N >= 16 and sum(fam.values()) == 0:  # (the families leave EVs uncovered from N = 16 on)
            problems.append((name, "no re-solved EV in the family-priced sets", fam))
        if not np.all(np.isnan(wide["cost"][status == ST.LOMPC_QP_INVALID])):
            problems.append((name, "an INVALID EV's cost is not NaN"))
        for form in ("per_kernel", "single"):  # the forms that share the recorded arrays agree on this build
            for key, v in wide.items():
                if not np.array_equal(outs[form][key], v, equal_nan=v.dtype.kind == "f"):
                    problems.append((name, form, key))
        for form in ("wide", "wide66", "reductions"):
            if form in outs:
                for key, v in outs[form].items():
                    rec[f"{name}_{key}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(rec)} arrays")
    assert not problems, f"the recorded build does not exercise or agree on: {problems}"


if __name__ == "__main__":
    main()
