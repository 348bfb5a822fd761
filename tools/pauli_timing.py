"""Pauli-string expectation values of a result tensor on the device (``ctg_exec_result_pauli``)
against two yardsticks on the same tensor in the same process:

* the floor of the reads: the number of X-mask passes of the call (``ceil(strings / 32)`` per distinct X mask) times one
  read of the tensor, ``prob_block_kernel`` alone (``sample_info``'s ``pass_ms[0]``);
* the route there was before: ``download_result`` and numpy (``np.flip`` on the X / Y axes, a broadcast sign tensor over
  the Z / Y axes, ``np.vdot``) in complex64.

complex64 tensors of 2^20 / 2^24 / 2^28 elements, extents all 2, behind a one-tensor tree whose result torch owns, so
that events on torch's current stream -- the executor's stream -- bracket a call: ``device_ms`` is the time between
the two events (the statistics passes the call runs first, ``stats_ms`` of it; its kernels and the copy of the values),
``wall_ms`` the host clock around the call.  Five calls: one Z-type string; 32 and 64 Z-type strings (one X mask: one
and two passes); one weight-20 mixed string with X bits on both sides of bit 12; 16 strings with 16 different X masks.
The measurements of a call alternate; the median of ``--reps`` (11).  The numpy route of the 2^28 tensor takes seconds
per string and is repeated ``--host-reps-large`` (3) times; from 2^24 elements on it is timed on the first
``--host-strings`` (2) strings of a call and its numpy part is scaled to the call's number of strings (the download
counts once; ``host_extrapolated`` marks such a row).

No ratio is fixed in advance: a row records what multiple of the floor the device time is -- with and without the
statistics passes -- and whether the call is slower than download + numpy.

    python tools/pauli_timing.py [--log2n 20 24 28] [--reps 11] [--out profiles/pauli_timing.json]
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
from cotengra_amd import runtime  # noqa: E402
from cotengra_amd.contractor import HipContractor  # noqa: E402

CODE = {"I": 0, "X": 1, "Y": 2, "Z": 3}


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


def bit_string(L, letters):
    """Codes over the shape (2,) * L with ``letters[b]`` on bit ``b`` of the flat index (axis L - 1 - b)."""
    row = [0] * L
    for b, c in letters.items():
        row[L - 1 - b] = CODE[c]
    return row


def calls(L):
    """``(name, rows)`` per call."""
    zz = [bit_string(L, {k % L: "Z", (7 * k + 3 + (k // L)) % L: "Z"}) for k in range(64)]
    lo, hi = list(range(10)), list(range(L - 10, L))
    mixed = {b: "XYZ"[i % 3] for i, b in enumerate(lo + hi)}
    assert any(c in "XY" and b < 12 for b, c in mixed.items()) and any(c in "XY" and b >= 12 for b, c in mixed.items())
    masks = [bit_string(L, {k: "X", (k + 5) % L: "Z"}) for k in range(16)]
    return (("1_z_string", [bit_string(L, {0: "Z", 13: "Z", L - 1: "Z"})]), ("32_z_strings", zz[:32]), ("64_z_strings", zz),
            ("1_mixed_weight_20", [bit_string(L, mixed)]), ("16_strings_16_x_masks", masks))


def passes_of(shape, rows):
    groups = {}
    for xm, _, _ in runtime.pauli_masks(shape, rows):
        groups[xm] = groups.get(xm, 0) + 1
    return sum((c + 31) // 32 for c in groups.values())


def host_pauli(ex, shape, rows, cap):
    """Download + numpy for the first ``cap`` strings: ``(download ms, numpy ms, values)``."""
    t0 = time.perf_counter()
    x = ex.download_result().reshape(-1)
    t1 = time.perf_counter()
    xt = x.reshape(shape)
    out = []
    for row in rows[:cap]:
        y, sign, ny = xt, np.ones((1,) * len(shape), dtype=np.float32), 0
        for a, op in enumerate(row):
            if op in (2, 3):
                v = np.ones(2, dtype=np.float32)
                v[1] = -1.0
                sign = sign * v.reshape((1,) * a + (2,) + (1,) * (len(shape) - a - 1))
            if op in (1, 2):
                y = np.flip(y, axis=a)
            ny += op == 2
        if any(row):
            y = y * sign
        out.append(float(np.real(np.vdot(x, y.reshape(-1)) * (1.0, 1j, -1.0, -1j)[ny % 4])))
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), out


def measure(ex, shape, rows, reps, host_reps, host_cap):
    """Alternating: the floor, the device call between two events, the numpy route."""
    import torch

    ops = np.array(rows, dtype=np.uint8)
    values = ex.pauli_result(shape, ops)
    floor, dev, stats, wall, host = [], [], [], [], []
    cap = min(len(rows), host_cap)
    for r in range(reps):
        ex.result_stats()
        floor.append(float(ex.sample_info()[4][0]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        ex.pauli_result(shape, ops)
        e1.record()
        e1.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(float(e0.elapsed_time(e1)))
        stats.append(float(sum(ex.sample_info()[4])))
        if r < host_reps:
            dl, npy, vals = host_pauli(ex, shape, rows, cap)
            host.append(dl + npy * len(rows) / cap)
            # (the two routes answer the same question: complex64 sums on the host, so a loose check)
            norm = float(ex.sample_info()[0])
            assert all(abs(a - b) <= 1e-3 * norm for a, b in zip(vals, values[:cap])), (vals, values[:cap].tolist())
    passes = passes_of(shape, rows)
    f = _summary(floor)["median_ms"] * passes
    out = {"strings": len(rows), "x_mask_passes": passes, "floor_prob_block_kernel": _summary(floor), "floor_ms": f,
           "device_ms": _summary(dev), "stats_ms": _summary(stats), "wall_ms": _summary(wall),
           "download_plus_numpy": _summary(host), "host_strings_timed": cap, "host_extrapolated": cap < len(rows)}
    out["device_over_floor"] = out["device_ms"]["median_ms"] / f
    out["kernels_over_floor"] = (out["device_ms"]["median_ms"] - out["stats_ms"]["median_ms"]) / f
    out["numpy_over_wall"] = out["download_plus_numpy"]["median_ms"] / out["wall_ms"]["median_ms"]
    out["slower_than_download_plus_numpy"] = out["wall_ms"]["median_ms"] > out["download_plus_numpy"]["median_ms"]
    return out


def size_rows(log2n, reps, host_reps, host_cap, rows_out):
    import torch

    n, L = 1 << log2n, log2n
    gen = torch.Generator(device="cuda").manual_seed(log2n)
    xt = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    fn, ex = resident(xt)
    shape = (2,) * L
    for name, rows in calls(L):
        m = measure(ex, shape, rows, reps, host_reps, host_cap)
        row = dict({"what": "pauli", "kernel": ex.pauli_variant(shape, rows), "call": name, "dtype": "complex64",
                    "log2_n": log2n}, **m)
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    fn.close()
    del xt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 24, 28])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps-large", type=int, default=3)
    ap.add_argument("--host-strings", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pauli_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("pauli_timing.py measures on the GPU: none visible.")
    rows = []
    for log2n in args.log2n:
        size_rows(log2n, args.reps, args.reps if log2n < 28 else args.host_reps_large,
                  args.host_strings if log2n >= 24 else 1 << 30, rows)
        with open(args.out, "w") as f:   # (after every size: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
