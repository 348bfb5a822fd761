"""Top-k and marginals of a result tensor on the device (``ctg_exec_result_topk`` / ``ctg_exec_result_marginal``,
DESIGN.md section 12) against two yardsticks on the same tensor in the same process:

* the floor: ``prob_block_kernel`` alone (``sample_info``'s ``pass_ms[0]``) -- one read of the tensor;
* the route there was before: ``download_result`` and numpy (argpartition + lexsort / reshape + sum).

complex64 tensors of 2^20 / 2^24 / 2^28 elements behind a one-tensor tree whose result torch owns, so that events on
torch's current stream -- the executor's stream -- bracket a call: ``device_ms`` is the time between the two events
(kernels, the small copies and the host's round trips in between), ``wall_ms`` the host clock around the call (the
ordering of the k records on the host included).  Top-k at k = 1, 64, 4096 on Gaussian data and on an all-equal
tensor; marginals of extents all 2 keeping 2 high bits, 2 low bits and 6 bits split across both, and one shape that
is no power of two on the general route.  The three measurements of a case alternate; the median of ``--reps``
(11).  The numpy route of the 2^28 tensor takes seconds per repetition and is repeated ``--host-reps-large`` (3)
times.

    python tools/result_reduce_timing.py [--log2n 20 24 28] [--reps 11] [--out profiles/result_reduce.json]
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
from cotengra_amd.contractor import HipContractor  # noqa: E402


def _summary(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": len(ts)}


def resident(xt):
    """A contractor of the one-tensor tree and its executor with ``xt`` (a ROCm tensor) in the torch-owned result."""
    fn = HipContractor(ca.ContractionTree(["a"], "a", {"a": xt.numel()}))
    ex = fn.setup(xt)["exec"]
    ex.zero_result()
    ex.run_slices()
    ex.sync()
    return fn, ex


def measure(ex, device_call, host_call, reps, host_reps):
    """Alternating: the floor, the device call between two events, the numpy route."""
    import torch

    device_call()
    floor, dev, wall, host = [], [], [], []
    for r in range(reps):
        ex.result_stats()
        floor.append(float(ex.sample_info()[4][0]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        device_call()
        e1.record()
        e1.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(float(e0.elapsed_time(e1)))
        if r < host_reps:
            t0 = time.perf_counter()
            host_call()
            host.append(1e3 * (time.perf_counter() - t0))
    out = {"floor_prob_block_kernel": _summary(floor), "device_ms": _summary(dev), "wall_ms": _summary(wall),
           "download_plus_numpy": _summary(host)}
    out["device_over_floor"] = out["device_ms"]["median_ms"] / out["floor_prob_block_kernel"]["median_ms"]
    out["numpy_over_wall"] = out["download_plus_numpy"]["median_ms"] / out["wall_ms"]["median_ms"]
    out["slower_than_download_plus_numpy"] = out["wall_ms"]["median_ms"] > out["download_plus_numpy"]["median_ms"]
    return out


def host_topk(ex, k):
    x = ex.download_result().reshape(-1)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    p = re * re + im * im
    cand = np.argpartition(p, p.size - k)[p.size - k:] if k < p.size else np.arange(p.size)
    return cand[np.lexsort((cand, -p[cand]))]


def host_marginal(ex, shape, keep):
    x = ex.download_result().reshape(-1)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    other = tuple(a for a in range(len(shape)) if a not in keep)
    return (re * re + im * im).reshape(shape).sum(axis=other)


def emit(rows, row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def size_rows(log2n, reps, host_reps, rows):
    import torch

    n = 1 << log2n
    gen = torch.Generator(device="cuda").manual_seed(log2n)
    for data in ("gaussian", "all_equal"):
        if data == "gaussian":
            xt = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
        else:
            xt = torch.full((n,), 0.75 + 0.0j, device="cuda", dtype=torch.complex64)
        fn, ex = resident(xt)
        for k in (1, 64, 4096):
            m = measure(ex, lambda: ex.topk_result(k), lambda: host_topk(ex, k), reps, host_reps)
            emit(rows, dict({"what": "topk", "data": data, "dtype": "complex64", "log2_n": log2n, "k": k}, **m))
        if data == "gaussian":
            shape = (2,) * log2n
            L = log2n
            for name, keep in (("2_high_bits", (0, 1)), ("2_low_bits", (L - 2, L - 1)),
                               ("6_bits_split", (0, 1, 2, L - 3, L - 2, L - 1))):
                flags = [1 if a in keep else 0 for a in range(L)]
                m = measure(ex, lambda: ex.marginal_result(shape, flags), lambda: host_marginal(ex, shape, keep), reps, host_reps)
                emit(rows, dict({"what": "marginal", "route": "power_of_two", "keep": name, "dtype": "complex64",
                                 "log2_n": log2n}, **m))
        fn.close()
        del xt
        torch.cuda.empty_cache()


def general_row(reps, rows):
    import torch

    shape = (3, 5, 7, 11, 13, 17, 19)
    n = int(np.prod(shape))
    gen = torch.Generator(device="cuda").manual_seed(7)
    xt = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    fn, ex = resident(xt)
    keep = (1, 4)
    flags = [1 if a in keep else 0 for a in range(len(shape))]
    m = measure(ex, lambda: ex.marginal_result(shape, flags), lambda: host_marginal(ex, shape, keep), reps, reps)
    emit(rows, dict({"what": "marginal", "route": "general", "shape": list(shape), "keep": list(keep), "dtype": "complex64",
                     "elements": n}, **m))
    fn.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 24, 28])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps-large", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "result_reduce.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("result_reduce_timing.py measures on the GPU: none visible.")
    rows = []
    general_row(args.reps, rows)
    for log2n in args.log2n:
        size_rows(log2n, args.reps, args.reps if log2n < 28 else args.host_reps_large, rows)
        with open(args.out, "w") as f:   # (after every size: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
