"""Reduced density matrices above 64 rows on the device (``ctg_exec_result_rdm_wide``) against
the yardsticks of tools/rdm_timing.py, on the same tensor in the same process:

* the floor of one read: ``prob_block_kernel`` alone (``sample_info``'s ``pass_ms[0]``), listed next to the second
  statistics pass, which every call runs first;
* the matrix-work bound: ``8 n D / 2`` flops (the lower triangle of a complex rank-t update) at the fp64 matrix peak
  of the part, ``--fp64-matrix-tflops`` (78.6: v_mfma_f64_16x16x4_f64 on all CUs);
* the bytes the plan reads: every block reads its one or two 64-row panels once, ``panels + 1`` times the tensor in
  all (``reread_bytes``; how much of that comes from L2 / MALL is not measured here);
* the route there was before: ``download_result`` and numpy (``reshape``, ``transpose``, ``@``).

complex64 tensors of 2^20 / 2^24 / 2^28 elements, extents all 2, behind a one-tensor tree whose result torch owns, so
that events on torch's current stream -- the executor's stream -- bracket a call.  Per size: D = 128, 1024, 4096 with
the kept bits at the top and interleaved (every second bit from the lowest).  ``purity_only`` rows repeat the high-bit
case with ``matrix=False``.  The measurements of a case alternate; the median of ``--reps`` (11).  The numpy route of
the 2^28 tensor is repeated ``--host-reps-large`` (3) times.

No ratio is fixed in advance: a row records what multiple of ``max(floor, matrix bound)`` the device time is, and
whether the call is slower than download + numpy.

    python tools/rdm_wide_timing.py [--log2n 20 24 28] [--reps 11] [--out profiles/rdm_wide_timing.json]
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

from cotengra_amd import runtime  # noqa: E402
from rdm_timing import _summary, resident  # noqa: E402


def host_rdm(ex, shape, keep):
    x = ex.download_result().reshape(shape)
    other = [a for a in range(len(shape)) if a not in keep]
    X = x.transpose(list(keep) + other).reshape(2 ** len(keep), -1).astype(np.complex128)
    return X @ X.conj().T


def measure(ex, device_call, host_call, reps, host_reps, matrix_ms):
    """Alternating: the statistics passes, the device call between two events, the numpy route."""
    import torch

    device_call()
    floor, second, dev, wall, host = [], [], [], [], []
    for r in range(reps):
        ex.result_stats()
        floor.append(float(ex.sample_info()[4][0]))
        second.append(float(ex.sample_info()[4][1]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        device_call()
        e1.record()
        e1.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(float(e0.elapsed_time(e1)))
        if host_call is not None and r < host_reps:
            t0 = time.perf_counter()
            host_call()
            host.append(1e3 * (time.perf_counter() - t0))
    out = {"floor_prob_block_kernel": _summary(floor), "statistics_pass_2": _summary(second), "matrix_bound_ms": matrix_ms,
           "device_ms": _summary(dev), "wall_ms": _summary(wall)}
    bound = max(out["floor_prob_block_kernel"]["median_ms"], matrix_ms)
    out["device_over_max_of_bounds"] = out["device_ms"]["median_ms"] / bound
    out["binding_bound"] = "matrix" if matrix_ms > out["floor_prob_block_kernel"]["median_ms"] else "read"
    if host:
        out["download_plus_numpy"] = _summary(host)
        out["numpy_over_wall"] = out["download_plus_numpy"]["median_ms"] / out["wall_ms"]["median_ms"]
        out["slower_than_download_plus_numpy"] = out["wall_ms"]["median_ms"] > out["download_plus_numpy"]["median_ms"]
    return out


def cases(L):
    """Kept axes of the shape (2,) * L (axis 0 is the highest bit of the flat index)."""
    out = []
    for d in (7, 10, 12):
        out.append((f"{d}_high_bits", tuple(range(d))))
        if 2 * d <= L:   # (every second bit from the lowest)
            out.append((f"{d}_bits_interleaved", tuple(sorted(L - 1 - 2 * i for i in range(d)))))
    return out


def size_rows(log2n, reps, host_reps, tflops, rows):
    import torch

    n, L = 1 << log2n, log2n
    gen = torch.Generator(device="cuda").manual_seed(log2n)
    xt = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    fn, ex = resident(xt)
    shape = (2,) * L
    for name, keep in cases(L):
        flags = [1 if a in keep else 0 for a in range(L)]
        D = 2 ** len(keep)
        plan = runtime.rdm_wide_plan("complex64", shape, flags)
        matrix_ms = 1e3 * (8.0 * n * D / 2) / (tflops * 1e12)
        variants = [("rdm_wide", lambda: ex.rdm_wide_result(shape, flags), lambda: host_rdm(ex, shape, keep))]
        if name.endswith("high_bits"):
            variants.append(("rdm_wide_purity_only", lambda: ex.rdm_wide_result(shape, flags, matrix=False), None))
        for what, dev_call, host_call in variants:
            m = measure(ex, dev_call, host_call, reps, host_reps, matrix_ms)
            row = dict({"what": what, "kernel": ex.rdm_wide_variant(shape, flags), "keep": name, "D": D, "dtype": "complex64",
                        "log2_n": log2n, "plan": plan._asdict(), "reread_bytes": 8 * n * (plan.panels + 1)}, **m)
            rows.append(row)
            print(json.dumps(row), flush=True)
    fn.close()
    del xt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 24, 28])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps-large", type=int, default=3)
    ap.add_argument("--fp64-matrix-tflops", type=float, default=78.6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdm_wide_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rdm_wide_timing.py measures on the GPU: none visible.")
    rows = []
    for log2n in args.log2n:
        size_rows(log2n, args.reps, args.reps if log2n < 28 else args.host_reps_large, args.fp64_matrix_tflops, rows)
        with open(args.out, "w") as f:   # (after every size: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
