"""Drawing from a result tensor: the device route (``ctg_exec_sample_result``: three kernels next to the tensor,
only the draws come back) against the only route there was before it -- ``download_result`` and numpy's square /
cumsum / searchsorted on the same uniforms.  complex64 tensors of n = 2^16 ... 2^28 elements behind a one-tensor
tree, S = 1 and 2^16 draws; both routes in one process, alternating, after a warm-up of each; median and range over
the repetitions.  Also: the statistics call alone on the host clock, its pass 1 (prob_block_kernel) and pass 2
(prob_scan_kernel) by device events (``ctg_exec_sample_info``), pass 1 as bytes/s of the tensor next to the copy
ceiling of the chip, and the Sycamore m10 batch of 256 amplitudes contracted with and without 4096 draws.

    python tools/sample_timing.py [--log2n 16 20 24 28] [--reps 5] [--out profiles/sample_timing.json]
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

COPY_CEILING = 6.29e12   # bytes/s, float4 copy measured on MI355X (HBM3E: 8.0e12 by specification)


def _summary(ts):
    ts = sorted(ts)
    return {"median_ms": 1e3 * ts[len(ts) // 2], "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": len(ts)}


def host_route(ex, u):
    """What a caller had to do: the whole tensor over the bus, then numpy on one core."""
    x = ex.download_result().reshape(-1)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    c = np.cumsum(re * re + im * im)
    return np.searchsorted(c, u * c[-1], side="right")


def tensor_rows(log2n, reps, rows):
    n = 1 << log2n
    rng = np.random.default_rng(log2n)
    x = np.empty(n, np.complex64)
    x.real = rng.random(n, dtype=np.float32) - 0.5
    x.imag = rng.random(n, dtype=np.float32) - 0.5
    fn = HipContractor(ca.ContractionTree(["a"], "a", {"a": n}))
    ex = fn.setup(x)["exec"]
    ex.zero_result()
    ex.run_slices()
    ex.sync()
    del x
    nbytes = 8 * n
    ex.result_stats()
    ts, p1, p2 = [], [], []
    for _ in range(max(reps, 5)):
        t0 = time.perf_counter()
        ex.result_stats()
        ts.append(time.perf_counter() - t0)
        ms = ex.sample_info()[4]   # device events around pass 1 and pass 2 of that call
        p1.append(ms[0] * 1e-3)
        p2.append(ms[1] * 1e-3)
    stats, pass1, pass2 = _summary(ts), _summary(p1), _summary(p2)
    pass1_rate = nbytes / (pass1["median_ms"] * 1e-3)
    for S in (1, 1 << 16):
        u = np.random.default_rng(S).random(S)
        dev_idx = ex.sample_result(u)[0]
        ref_idx = host_route(ex, u)
        td, th = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ex.sample_result(u)
            td.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            host_route(ex, u)
            th.append(time.perf_counter() - t0)
        d, h = _summary(td), _summary(th)
        row = {
            "what": "tensor", "dtype": "complex64", "log2_n": log2n, "draws": S, "tensor_bytes": nbytes,
            "device_route": d, "host_route": h, "host_over_device": h["median_ms"] / d["median_ms"],
            "host_route_spread_ms": h["max_ms"] - h["min_ms"],
            "device_not_slower_than_host_beyond_its_spread": d["median_ms"] <= h["median_ms"] + (h["max_ms"] - h["min_ms"]),
            "draws_differing_from_numpy": int(np.count_nonzero(dev_idx != ref_idx)),
            "stats_call": stats, "pass1_prob_block_kernel": pass1, "pass2_prob_scan_kernel": pass2,
            "pass1_bytes_per_s": pass1_rate, "pass1_share_of_copy_ceiling": pass1_rate / COPY_CEILING,
            "copy_ceiling_bytes_per_s": COPY_CEILING,
        }
        rows.append(row)
        print(json.dumps(row), flush=True)
    fn.close()


def m10_row(reps, rows):
    tree = ca.tree_from_record(ca.load_network(os.path.join(ROOT, "tests", "golden", "trees", "sycamore_m10_open8.json")))
    z = np.load(os.path.join(ROOT, "tests", "golden", "sycamore_m10_open8_arrays.npz"))
    xs = [z[f"t{i}"].astype("complex64") for i in range(tree.N)]
    fn = HipContractor(tree)
    u = np.random.default_rng(0).random(4096)
    fn(*xs)
    fn.sample(*xs, n_samples=4096, uniforms=u)
    tc, ts = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(*xs)
        tc.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        fn.sample(*xs, n_samples=4096, uniforms=u)
        ts.append(time.perf_counter() - t0)
    c, s = _summary(tc), _summary(ts)
    row = {"what": "sycamore_m10_open8", "dtype": "complex64", "nslices": tree.nslices, "amplitudes": 256, "draws": 4096,
           "contract_and_download": c, "contract_and_sample": s, "sample_over_contract": s["median_ms"] / c["median_ms"]}
    rows.append(row)
    print(json.dumps(row), flush=True)
    fn.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20, 24, 28])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("sample_timing.py measures on the GPU: none visible.")
    rows = []
    m10_row(max(args.reps, 20), rows)
    for log2n in args.log2n:
        tensor_rows(log2n, args.reps, rows)
        with open(args.out, "w") as f:   # (after every size: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
