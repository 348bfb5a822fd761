"""The requests of a pick carried down the tree (``chain=True``) against the sparse root step
alone (``chain=False``: the plan of before), in one process on one device; complex64.  The two plans alternate, the
median of ``--reps`` (5).

* The two-stem tree of ``tools/pick_timing.py`` part 2 at 2^10 and 2^16 requests.
* ``circuits.amplitudes_of`` on a random circuit of ``--qubits`` qubits, all open, 2^12 random bitstrings.

Per case and plan: every step's time from ``profile_slice`` (label, kernel, ms), the slice time, ``plan.arena_elems``
and the wall time of the first call of a new table (plan compilation, tables, executor, one contraction); per
``KERNEL_PICK_ROWS`` step its time against its moved-bytes floor -- (distinct A sub-tensors + distinct B sub-tensors
+ result) * 8 bytes at 6.1 TB/s.

    python tools/pick_chain_timing.py [--reps 5] [--qubits 22] [--dry] [--out profiles/pick_chain_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import cotengra_amd as ca  # noqa: E402
from cotengra_amd import plan as P  # noqa: E402
from cotengra_amd import runtime  # noqa: E402
from cotengra_amd.circuits import circuit_to_network  # noqa: E402

from pick_timing import COPY_RATE, cplx, two_stem_tree  # noqa: E402


def random_circuit(n, depth, seed):
    """Sycamore-style layers: a random single-qubit gate on every qubit, then fSim gates on a brick pattern."""
    rng = np.random.default_rng(seed)
    gates = []
    for d in range(depth):
        for q in range(n):
            name = ("x_1_2", "y_1_2", "hz_1_2", "rz")[int(rng.integers(0, 4))]
            gates.append((name, (q,), (float(rng.normal()),) if name == "rz" else ()))
        for q in range(d % 2, n - 1, 2):
            gates.append(("fs", (q, q + 1), (float(rng.normal()), float(rng.normal()))))
    return gates


def case(what, tree, arrays, coords, reps, fuse_min_elems, dry):
    rec = {"what": what, "dtype": "complex64", "M": int(len(coords)), "nslices": int(tree.nslices),
           "output_elems": int(np.prod(tree.gathered_shape(), dtype=np.float64)),
           "sparse_nodes": [[int(n), int(m), int(o), int(d)] for n, m, o, d in P.pick_chain_nodes(tree, coords, True)]}
    plans = {name: P.compile_tree(tree, "complex64", fuse_min_elems=fuse_min_elems, pick=coords, pick_chain=chain)
             for name, chain in (("chain_false", False), ("chain_true", True))}
    execs = {}
    for name, plan in plans.items():
        r = rec[name] = {"arena_elems": int(plan.arena_elems), "steps": len(plan.steps),
                         "pick_rows_steps": sum(1 for s in plan.steps if s.kernel == P.KERNEL_PICK_ROWS)}
        if dry:
            continue
        dp = runtime.DevicePlan(plan)
        ex = runtime.Executor(dp)
        ex.upload_host(arrays)
        ex.zero_result()
        ex.run_slices(0, 1, 1)
        ex.sync()
        execs[name] = (dp, ex)
    if dry:
        return rec
    ms = {name: [] for name in plans}
    for _ in range(reps):
        for name in plans:   # (alternating)
            ms[name].append(execs[name][1].profile_slice(0))
    for name, plan in plans.items():
        dp, ex = execs[name]
        all_ms = np.array(ms[name])
        med = np.median(all_ms, axis=0)
        names = ex.step_kernels()
        r = rec[name]
        r["slice_ms"] = float(np.median(all_ms.sum(axis=1)))
        r["slice_ms_spread"] = [float(all_ms.sum(axis=1).min()), float(all_ms.sum(axis=1).max())]
        r["step_ms"] = [{"step": i, "node": int(s.node), "label": s.label, "kernel": names[i], "ms": float(med[i])}
                        for i, s in enumerate(plan.steps)]
        r["pick_rows"] = []
        for i, s in enumerate(plan.steps):
            if s.kernel != P.KERNEL_PICK_ROWS:
                continue
            floor_ms = 1e3 * s.elems_rw * 8 / COPY_RATE
            r["pick_rows"].append({"step": i, "label": s.label, "kernel": names[i], "ms": float(med[i]),
                                   "route": P.pick_rows_route(s.row_lo, s.K, s.N, "complex64"),
                                   "moved_bytes_floor": int(s.elems_rw * 8), "floor_ms": floor_ms,
                                   "over_floor": float(med[i]) / floor_ms})
        ex.close()
        dp.close()
    rec["slice_chain_false_over_true"] = rec["chain_false"]["slice_ms"] / rec["chain_true"]["slice_ms"]
    # the first call of a new table, the two ways alternating on fresh trees
    first = {"chain_false": [], "chain_true": []}
    for _ in range(reps):
        for name, chain in (("chain_false", False), ("chain_true", True)):
            fresh = tree.copy()
            t0 = time.perf_counter()
            out = fresh.contract_pick(arrays, coords=coords, chain=chain)
            first[name].append(1e3 * (time.perf_counter() - t0))
            rec[name]["max_abs"] = float(np.abs(out).max())
            for f in list(fresh.contraction_cores.values()):
                f.close()
    for name in first:
        rec[name]["first_call_ms"] = float(np.median(first[name]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stem-qubits", type=int, default=22)
    ap.add_argument("--stem-log2m", type=int, nargs="*", default=[10, 16])
    ap.add_argument("--fuse-min-elems", type=int, default=1 << 16)
    ap.add_argument("--qubits", type=int, default=22, help="qubits of the random circuit, all open")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--log2m", type=int, default=12, help="bitstrings scored on the circuit")
    ap.add_argument("--dry", action="store_true", help="plans only: nothing touches a device, nothing is timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pick_chain_timing.json"))
    args = ap.parse_args()

    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        if not args.dry:
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)

    rng = np.random.default_rng(2)
    nq = args.stem_qubits
    tree = two_stem_tree(nq, [(3, 3), (5, 5), (5, 5), (6, 6)], 10)
    arrays = [cplx(rng, *s) / np.sqrt(2.0 ** (len(s) / 2)) for s in tree.get_shapes()]
    for lm in args.stem_log2m:
        r = np.random.default_rng(1)
        coords = np.stack([r.integers(0, d, 1 << lm) for d in tree.gathered_shape()], axis=1).astype(np.int64)
        emit(case(f"two stems of {nq} binary indices, root over 2^10", tree, arrays, coords, args.reps,
                  args.fuse_min_elems, args.dry))

    n = args.qubits
    inputs, output, sd, arrays = circuit_to_network(n, random_circuit(n, args.depth, 3), "?" * n, simplify=True,
                                                    dtype="complex64")
    tree = ca.array_contract_tree(inputs, output, sd)
    coords = np.random.default_rng(5).integers(0, 2, (1 << args.log2m, n)).astype(np.int64)
    emit(case(f"amplitudes_of: random circuit, {n} qubits all open, depth {args.depth}", tree, arrays, coords,
              args.reps, None, args.dry))


if __name__ == "__main__":
    main()
