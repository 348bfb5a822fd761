"""Chosen members of the output through the sparse root step (``HipContractor.pick``) against
what there was before, in one process on one device; complex64.

Part 1 -- a root of two children with 2^10 x K elements each, ``a[2^10, K] . c[2^10, K] -> (a, c)`` (both operands
contiguous along k: 16-byte loads; ``--cols`` adds ``b[K, 2^10]`` on the right, the general path), K in 2^6, 2^10,
2^14 and M in 2^10, 2^16, 2^20 uniformly random requests.  The inputs are resident ROCm tensors.  The two routes
alternate, the median of ``--reps`` (5):

* (a) what a user did before: the full contraction, download, numpy fancy index;
* (b) ``contract_pick`` and the download of its M values -- the whole call with the plan of the table cached, the
  first call of a new table (plan compilation, tables, executor), the pick step's own time from ``profile_slice``,
  and that time against the step's moved-bytes floor, (distinct A rows + distinct B rows) * K * 8 bytes at 6.1 TB/s.

Part 2 -- what the re-layout of the root's children costs their producers: trees whose root children are
intermediates (two stems of ``--stem-qubits`` binary indices that meet at the root over 2^10, fused stem steps from
``--fuse-min-elems`` on, at 2^10 and 2^16 requests; and the golden ``sycamore_m10_open8``), three plans each -- the ordinary plan, the pick plan
(children laid out for the root step) and the pick plan in the ordinary layout (``compile_tree(_pick_relayout=False)``,
an argument of this tool, not a product switch) -- every step timed by ``profile_slice``, median of ``--reps``.

    python tools/pick_timing.py [--reps 5] [--cols] [--dry] [--out profiles/pick_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import cotengra_amd as ca  # noqa: E402
from cotengra_amd import plan as P  # noqa: E402
from cotengra_amd import runtime  # noqa: E402
from cotengra_amd.contractor import _tree_contractor, pick_requests  # noqa: E402

COPY_RATE = 6.1e12   # bytes / s: the copy rate the project uses as the ceiling of a memory-bound step


def _summary(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": len(ts)}


def cplx(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype("complex64")


# ---- part 1 ------------------------------------------------------------------------------------------------------- #

def root_tree(K, cols, side=1 << 10):
    right = ("k", "c") if cols else ("c", "k")
    return ca.ContractionTree.from_path([("a", "k"), right], ("a", "c"), dict(a=side, k=K, c=side), path=[(0, 1)])


def part1_case(K, M, cols, reps, dry):
    import torch

    tree = root_tree(K, cols)
    rng = np.random.default_rng(K + M)
    coords = np.stack([rng.integers(0, 1 << 10, M), rng.integers(0, 1 << 10, M)], axis=1).astype(np.int64)
    rec = {"what": "root", "layout": "b[k, c] (general path)" if cols else "c[c, k] (contiguous along k)",
           "dtype": "complex64", "K": K, "M": M, "full_output_elems": 1 << 20}
    plan = P.compile_tree(tree, "complex64", pick=coords)
    (i_pick,) = [i for i, s in enumerate(plan.steps) if s.kernel == P.KERNEL_PICK]
    step = plan.steps[i_pick]
    rec["route"] = P.pick_route(M, K)
    rec["moved_bytes_floor"] = int(step.elems_rw - M) * 8
    rec["floor_ms"] = 1e3 * rec["moved_bytes_floor"] / COPY_RATE
    if dry:
        return rec
    arrays = [torch.tensor(cplx(rng, *s), device="cuda") for s in tree.get_shapes()]
    sel = tuple(coords.T)

    def route_a():
        return tree.contract(arrays).cpu().numpy()[sel]

    def route_b():
        return tree.contract_pick(arrays, coords=coords).cpu().numpy()

    t0 = time.perf_counter()
    b = route_b()
    rec["pick_first_call_ms"] = 1e3 * (time.perf_counter() - t0)
    a = route_a()
    scale = float(np.abs(a).max())
    rec["max_abs_difference_over_max_abs"] = float(np.abs(a - b).max() / scale)
    ta, tb = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        route_a()
        ta.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        route_b()
        tb.append(1e3 * (time.perf_counter() - t0))
    rec["full_contract_download_index"] = _summary(ta)
    rec["pick_whole_call"] = _summary(tb)
    rec["full_over_pick"] = rec["full_contract_download_index"]["median_ms"] / rec["pick_whole_call"]["median_ms"]
    fn = _tree_contractor(tree)._pick_contractor(pick_requests(tree, coords=coords))
    (st,) = fn._execs.values()
    rec["pick_kernel"] = st["exec"].step_kernels()[i_pick]
    ms = [st["exec"].profile_slice(0)[i_pick] for _ in range(reps)]
    rec["pick_step"] = _summary([float(x) for x in ms])
    rec["pick_step_over_floor"] = rec["pick_step"]["median_ms"] / rec["floor_ms"]
    for f in list(tree.contraction_cores.values()):
        f.close()
    return rec


# ---- part 2 ------------------------------------------------------------------------------------------------------- #

def two_stem_tree(nq, gates, k, seed=0):
    """Two stems -- a tensor of ``nq`` binary indices to which gate tensors ``(contracted, new)`` are applied one after
    the other -- whose results meet at the root over ``k`` indices; the output holds the ``2 (nq - k)`` others."""
    rng = np.random.default_rng(seed)

    def stem(tag):
        cur = [f"{tag}{i}" for i in range(nq)]
        inputs = [tuple(cur)]
        for g, (kin, nout) in enumerate(gates):
            sel = sorted(int(i) for i in rng.choice(len(cur), size=kin, replace=False))
            new = [f"{tag}g{g}_{j}" for j in range(nout)]
            inputs.append(tuple(cur[i] for i in rng.permutation(sel)) + tuple(new))
            cur = [c for i, c in enumerate(cur) if i not in sel] + new
        return inputs, cur

    left, cur_l = stem("l")
    right, cur_r = stem("r")
    rename = dict(zip(cur_r[-k:], cur_l[:k]))
    right = [tuple(rename.get(ix, ix) for ix in t) for t in right]
    cur_r = [rename.get(ix, ix) for ix in cur_r]
    inputs = left + right
    output = tuple(cur_l[k:]) + tuple(cur_r[:-k])
    ssa, nxt = [], len(inputs)
    heads = []
    for first, n in ((0, len(left)), (len(left), len(right))):
        cur_id = first
        for i in range(first + 1, first + n):
            ssa.append((cur_id, i))
            cur_id, nxt = nxt, nxt + 1
        heads.append(cur_id)
    ssa.append(tuple(heads))
    size_dict = {ix: 2 for t in inputs for ix in t}
    return ca.ContractionTree.from_path(inputs, output, size_dict, ssa_path=ssa)


def producers_of(plan, tree):
    """Per child of the root: the index of the step that writes its tensor (None for a leaf read in place)."""
    out = []
    for child in tree.children[tree.root]:
        idx = [i for i, s in enumerate(plan.steps) if s.node == child and s.kind in (P.KIND_PAIR, P.KIND_STEM2, P.KIND_SINGLE)]
        out.append(idx[-1] if idx else None)
    return out


def part2_case(what, tree, arrays, M, reps, fuse_min_elems, dry):
    rng = np.random.default_rng(1)
    shape = tree.gathered_shape()
    coords = np.stack([rng.integers(0, d, M) for d in shape], axis=1).astype(np.int64)
    rec = {"what": what, "dtype": "complex64", "M": M, "nslices": int(tree.nslices), "output_elems": int(np.prod(shape))}
    plans = {
        "ordinary": P.compile_tree(tree, "complex64", fuse_min_elems=fuse_min_elems),
        "pick_relayout": P.compile_tree(tree, "complex64", fuse_min_elems=fuse_min_elems, pick=coords),
        "pick_ordinary_layout": P.compile_tree(tree, "complex64", fuse_min_elems=fuse_min_elems, pick=coords,
                                               _pick_relayout=False),
    }
    kinds = ("single", "pair", "accum", "stem2")
    for name, plan in plans.items():
        prods = producers_of(plan, tree)
        (i_root,) = [i for i, s in enumerate(plan.steps) if s.node == tree.root and s.kind != P.KIND_ACCUM]
        r = rec[name] = {"producer_steps": prods, "root_step": i_root,
                         "producer_kinds": [None if i is None else kinds[plan.steps[i].kind] for i in prods],
                         "root_K": int(plan.steps[i_root].K)}
        if dry:
            continue
        dp = runtime.DevicePlan(plan)
        ex = runtime.Executor(dp)
        ex.upload_host(arrays)
        ex.zero_result()
        ex.run_slices(0, 1, 1)
        ex.sync()
        names = ex.step_kernels()
        ms = np.array([ex.profile_slice(0) for _ in range(reps)])
        med = np.median(ms, axis=0)
        r["producer_kernels"] = [None if i is None else names[i] for i in prods]
        r["producer_ms"] = [None if i is None else float(med[i]) for i in prods]
        r["producers_ms"] = float(sum(med[i] for i in prods if i is not None))
        r["root_kernel"] = names[i_root]
        r["root_ms"] = float(med[i_root])
        r["root_ms_spread"] = [float(ms[:, i_root].min()), float(ms[:, i_root].max())]
        r["slice_ms"] = float(med.sum())
        ex.close()
        dp.close()
    if not dry:
        a, b = rec["pick_relayout"], rec["pick_ordinary_layout"]
        rec["relayout_costs_the_producers_ms"] = a["producers_ms"] - b["producers_ms"]
        rec["relayout_saves_the_pick_step_ms"] = b["root_ms"] - a["root_ms"]
        rec["relayout_pays"] = rec["relayout_saves_the_pick_step_ms"] > rec["relayout_costs_the_producers_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2k", type=int, nargs="*", default=[6, 10, 14])
    ap.add_argument("--log2m", type=int, nargs="*", default=[10, 16, 20])
    ap.add_argument("--cols", action="store_true", help="also the general path: b[K, 2^10] on the right")
    ap.add_argument("--stem-qubits", type=int, default=22)
    ap.add_argument("--stem-log2m", type=int, nargs="*", default=[10, 16], help="requests of the two-stem tree")
    ap.add_argument("--fuse-min-elems", type=int, default=1 << 16)
    ap.add_argument("--dry", action="store_true", help="plans only: nothing touches a device, nothing is timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pick_timing.json"))
    args = ap.parse_args()

    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        if not args.dry:
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)

    for cols in ([False, True] if args.cols else [False]):
        for lk in args.log2k:
            for lm in args.log2m:
                if cols and lm > 16:
                    continue   # (8-byte gathers with a stride of 8 KiB: minutes of device time say nothing new)
                emit(part1_case(1 << lk, 1 << lm, cols, args.reps, args.dry))

    rng = np.random.default_rng(2)
    nq = args.stem_qubits
    tree = two_stem_tree(nq, [(3, 3), (5, 5), (5, 5), (6, 6)], 10)
    arrays = [cplx(rng, *s) / np.sqrt(2.0 ** (len(s) / 2)) for s in tree.get_shapes()]
    for lm in args.stem_log2m:
        emit(part2_case(f"two stems of {nq} binary indices, root over 2^10", tree, arrays, 1 << lm, args.reps,
                        args.fuse_min_elems, args.dry))
    here = os.path.join(ROOT, "tests", "golden")
    tree = ca.tree_from_record(ca.load_network(os.path.join(here, "trees", "sycamore_m10_open8.json")))
    z = np.load(os.path.join(here, "sycamore_m10_open8_arrays.npz"))
    arrays = [z[f"t{i}"].astype("complex64") for i in range(tree.N)]
    emit(part2_case("sycamore_m10_open8", tree, arrays, 256, args.reps, None, args.dry))


if __name__ == "__main__":
    main()
