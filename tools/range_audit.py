"""Range audit of a tree (``HipContractor.audit``): for every plan step the kernel, which of its
operands run under one power of two per tensor in the executor's arithmetic, the ``crest_up`` of operands and result
(upper edge of the top binade over the rms: what one scale costs the tensor), the share of the big operand's
non-zero components more than 14 binades under the top, and ``kappa = |A| |B| (|B2|) / |C|``.

    python tools/range_audit.py                      # the table for the Sycamore m10 fixture and its golden inputs
    python tools/range_audit.py --record             # Sycamore m10 and a narrowed m20 on the benchmark's Gaussian
                                                     # inputs (seed 42, complex64, rescaled) -> profiles/range_audit.json,
                                                     # with the pass's time next to the max-abs pass over the same bytes
                                                     # (tools/ubench_range, built from tools/ubench_range.hip)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import cotengra_amd as ca  # noqa: E402
from cotengra_amd import rangeaudit as RA  # noqa: E402
from cotengra_amd.contractor import HipContractor  # noqa: E402

TREES = os.path.join(ROOT, "tests", "golden", "trees")
UBENCH = os.path.join(ROOT, "tools", "ubench_range")


def load_tree(name, width=None):
    tree = ca.tree_from_record(ca.load_network(os.path.join(TREES, name)))
    if width is not None and tree.max_size() > 2 ** width:
        tree = tree.slice(target_size=2 ** width)
    return tree


def bench_inputs(tree):
    return ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=42, dtype="complex64", rescale=True)


def audit(tree, arrays, slices, **kw):
    fn = HipContractor(tree, **kw)
    try:
        return fn.audit(*arrays, slices=slices)
    finally:
        fn.close()


def h2_rows(records, g=14):
    """What the JSON keeps: the steps with an operand under a per-tensor scale."""
    out = []
    for r in records:
        if not r["scaled"]:
            continue
        row = {"step": r["step"], "kernel": r["kernel"], "scaled": list(r["scaled"]), "kappa": r["kappa"]}
        for k in ("a", "b", "b2", "c"):
            t = r[k]
            row[k] = None if t is None else {"n": t.n, "crest_up": t.crest_up, f"below({g})": t.below(g), "eps_h2": t.eps_h2,
                                             "zeros": t.zeros, "nonfinite": t.nonfinite}
        out.append(row)
    return out


def pass_timing(log2_elems):
    if not os.path.exists(UBENCH):
        return None
    res = subprocess.run([UBENCH] + [str(x) for x in log2_elems], capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"{UBENCH} failed ({res.returncode}): {res.stdout[-500:]} {res.stderr[-500:]}")
    return [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write profiles/range_audit.json (needs an MI355X)")
    ap.add_argument("--m20-width", type=int, default=26, help="log2 of the widest intermediate of the narrowed m20 tree")
    ap.add_argument("--timing-log2", type=int, nargs="*", default=[20, 24, 28])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_audit.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("range_audit.py runs the audit on the GPU: none visible.")
    tree = load_tree("sycamore_m10.json")
    if not args.record:
        z = np.load(os.path.join(ROOT, "tests", "golden", "sycamore_m10_arrays.npz"))
        xs = [z[f"t{i}"].astype("complex64") for i in range(tree.N)]
        print(RA.format_table(audit(tree, xs, (0,))))
        return
    doc = {"inputs": "make_arrays_from_inputs(seed=42, complex64, rescale=True)", "arithmetic": "fp16x2", "trees": []}
    for name, width in (("sycamore_m10.json", None), ("sycamore_m20_native.json", args.m20_width)):
        tree = load_tree(name, width)
        last = int(min(tree.nslices, 2 ** 40)) - 1
        recs = audit(tree, bench_inputs(tree), (0, last) if last > 0 else (0,), stem_bf16x3="fp16x2")
        print(name, "width", width, "nslices", tree.nslices)
        print(RA.format_table(recs), flush=True)
        steps = h2_rows(recs)
        crest = [t["crest_up"] for s in steps for k in s["scaled"] for t in [s[k]] if t is not None]
        doc["trees"].append({"tree": name, "log2_width": width, "nslices": int(min(tree.nslices, 2 ** 62)), "slices_audited": [0, last],
                             "n_steps": len(recs), "fp16x2_steps": steps,
                             "largest_crest_up_of_a_scaled_operand": max(crest) if crest else None,
                             "steps_not_audited": sum(1 for r in recs if r["c"] is None)})
    doc["pass_timing"] = pass_timing(args.timing_log2)
    if doc["pass_timing"] is None:
        doc["pass_timing"] = "not measured: tools/ubench_range is not built"
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
