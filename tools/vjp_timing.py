"""Forward vs VJP time per slice, launches per slice and the VJP arena of C2 (lattice 8x8, d = 4) and C3
(Sycamore m10), complex64, torch tensors resident on the device.  ``--out FILE`` also writes the JSON rows.

    python tools/vjp_timing.py [--reps 20] [--out vjp_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cotengra_amd as ca  # noqa: E402
from cotengra_amd.contractor import HipContractor  # noqa: E402


def _configs():
    import golden_util as G

    case = next(c for c in G.cases("tree") if c["name"] == "C2_lattice8x8_d4")
    tree = G.tree_of(case)
    yield "C2", tree, G.arrays_of(case, "complex64", tree)
    rec = ca.load_network(os.path.join(ROOT, "tests", "golden", "trees", "sycamore_m10.json"))
    z = np.load(os.path.join(ROOT, "tests", "golden", "sycamore_m10_arrays.npz"))
    tree = ca.tree_from_record(rec)
    yield "C3", tree, [z[f"t{i}"].astype("complex64") for i in range(tree.N)]


def _time(f, reps):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for name, tree, arrays in _configs():
        xs = [torch.tensor(a, device="cuda") for a in arrays]
        h = torch.ones(tree.gathered_shape(), dtype=torch.complex64, device="cuda")
        fn = HipContractor(tree)
        fwd_ms = _time(lambda: fn(*xs), args.reps)
        vjp_ms = _time(lambda: fn.vjp(*xs, cotangent=h), args.reps)
        st_f = fn.setup(*xs)
        st_v = next(v for k, v in fn._execs.items() if "vjp" in k)
        pf, pv = st_f["plan"], st_v["plan"]
        row = {
            "config": name, "nslices": tree.nslices,
            "forward_ms_per_slice": fwd_ms / tree.nslices, "vjp_ms_per_slice": vjp_ms / tree.nslices,
            "ratio": vjp_ms / fwd_ms,
            "forward_steps_launches": st_f["exec"].launch_count(), "vjp_steps_launches": st_v["exec"].launch_count(),
            "forward_macs_per_slice": pf.macs_per_slice, "vjp_macs_per_slice": pv.macs_per_slice,
            "forward_arena_mib": pf.arena_elems * pf.itemsize / 2**20, "vjp_arena_mib": pv.arena_elems * pv.itemsize / 2**20,
        }
        rows.append(row)
        print(json.dumps(row), flush=True)
        fn.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
