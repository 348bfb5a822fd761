"""The Pauli spectrum of a result tensor on the device (``ctg_exec_result_pauli_spectrum``) against
three yardsticks on the same tensor in the same process:

* its floor of memory traffic: the tile pass reads the tensor (twice for ``xm != 0``: the partners) and writes ``8 n``
  bytes, every strided pass reads and writes ``8 n`` bytes.  One read of the tensor is ``prob_block_kernel`` alone
  (``sample_info``'s ``pass_ms[0]``); a read plus a write of ``8 n`` bytes is a plain fp64 copy of ``n`` doubles
  (``Tensor.copy_``), timed between events in the same run:
  ``floor = reads * prob_block + (passes + 1/2) * copy``;
* ``expectation``'s route (``ctg_exec_result_pauli``, which this change leaves untouched) for 32, 256 and 4096 Z-type
  strings, and the break-even number of strings: the spectrum's kernel time over the per-string time of the 4096-string
  call;
* ``download_result`` and numpy: ``u`` and an in-place Walsh-Hadamard transform in float64.

complex64 tensors of 2^20 / 2^24 / 2^28 elements, extents all 2, behind a one-tensor tree whose result torch owns, so
that events on torch's current stream -- the executor's stream -- bracket a call.  ``xm = 0`` and ``xm = 2^13 | 1`` (a
partner in another chunk).  The spectrum goes to ``dev_out`` (a torch buffer); ``select_wall_ms`` is the wall time of a
call that brings 4096 selected entries to the host instead.  Measurements alternate; the median of ``--reps`` (11).  The
numpy route is repeated ``--host-reps`` (3) times, once at 2^28.

No ratio is fixed in advance: a row records what multiple of the floor the device time is, with and without the
statistics passes.

    python tools/pauli_spectrum_timing.py [--log2n 20 24 28] [--reps 11] [--out profiles/pauli_spectrum_timing.json]
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


def z_strings(L, m):
    """``m`` different Z-type strings of weight 1 .. 6 as codes over the shape (2,) * L (``m`` far below ``2^L``)."""
    rng = np.random.default_rng(L)
    rows, seen = [], set()
    while len(rows) < m:
        bits = frozenset(rng.choice(L, size=int(rng.integers(1, 7)), replace=False).tolist())
        if bits in seen:
            continue
        seen.add(bits)
        row = [0] * L
        for b in bits:
            row[L - 1 - b] = 3
        rows.append(row)
    return np.array(rows, dtype=np.uint8)


def host_spectrum(ex, L, xm):
    """Download + numpy: ``(download ms, numpy ms, the spectrum)``."""
    t0 = time.perf_counter()
    x = ex.download_result().reshape(-1)
    t1 = time.perf_counter()
    if xm:
        p = x[np.arange(x.size) ^ xm]
        a, b, c, d = (t.astype(np.float64) for t in (p.real, p.imag, x.real, x.imag))
        v = (a * c + b * d) + (a * d - b * c)
    else:
        v = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2
    for b in range(L):
        t = v.reshape(-1, 2, 1 << b)
        lo = t[:, 0, :].copy()
        t[:, 0, :] += t[:, 1, :]
        np.subtract(lo, t[:, 1, :], out=t[:, 1, :])
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), v


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1)), 1e3 * (time.perf_counter() - t0)


def measure(ex, L, xm, reps, host_reps, expectation):
    import torch

    n = 1 << L
    shape = (2,) * L
    flips = [(xm >> (L - 1 - a)) & 1 for a in range(L)]
    plan = ex.pauli_spectrum_plan(shape, flips)
    buf = torch.empty(n, dtype=torch.float64, device="cuda")
    src = torch.zeros(n, dtype=torch.float64, device="cuda")
    dst = torch.empty(n, dtype=torch.float64, device="cuda")
    select = (np.arange(4096, dtype=np.int64) * 2654435761) % n
    ex.pauli_spectrum(shape, flips, dev_out=buf.data_ptr())
    read, copy, dev, stats, wall, sel_wall, host = [], [], [], [], [], [], []
    per = {m: [] for m in expectation}
    for r in range(reps):
        ex.result_stats()
        read.append(float(ex.sample_info()[4][0]))
        copy.append(timed(lambda: dst.copy_(src))[0])
        d, w = timed(lambda: ex.pauli_spectrum(shape, flips, dev_out=buf.data_ptr()))
        dev.append(d)
        wall.append(w)
        stats.append(float(sum(ex.sample_info()[4])))
        sel_wall.append(timed(lambda: ex.pauli_spectrum(shape, flips, select=select))[1])
        for m, ops in expectation.items():
            per[m].append(timed(lambda: ex.pauli_result(shape, ops))[0])
        print(f"2^{L} xm={xm:#x}: repetition {r + 1} of {reps}", file=sys.stderr, flush=True)
        if r < host_reps:
            dl, npy, v = host_spectrum(ex, L, xm)
            host.append(dl + npy)
            if r == 0:   # (the two routes answer the same question, up to the sign of the Y phases)
                got = buf.cpu().numpy()
                norm = float(ex.sample_info()[0])
                assert np.all(np.abs(np.abs(got) - np.abs(v)) <= 1e-9 * norm), float(np.abs(np.abs(got) - np.abs(v)).max())
            del v
    reads = 1 if xm == 0 else 2
    floor = reads * _summary(read)["median_ms"] + (plan.passes + 0.5) * _summary(copy)["median_ms"]
    out = {"log2_n": L, "dtype": "complex64", "xm": xm, "partner": plan.partner, "kernels": list(plan.kernels),
           "pass_bits": list(plan.pass_bits), "read_prob_block_kernel": _summary(read), "copy_8n_read_plus_write": _summary(copy),
           "tensor_reads": reads, "floor_ms": floor, "device_ms": _summary(dev), "stats_ms": _summary(stats), "wall_ms": _summary(wall),
           "select_wall_ms": _summary(sel_wall), "download_plus_numpy": _summary(host)}
    kernels = out["device_ms"]["median_ms"] - out["stats_ms"]["median_ms"]
    out["kernels_ms"] = kernels
    out["device_over_floor"] = out["device_ms"]["median_ms"] / floor
    out["kernels_over_floor"] = kernels / floor
    out["numpy_over_wall"] = out["download_plus_numpy"]["median_ms"] / out["wall_ms"]["median_ms"]
    for m in expectation:
        out[f"expectation_{m}_z_strings_device_ms"] = _summary(per[m])
    if expectation:
        big = max(expectation)
        per_string = _summary(per[big])["median_ms"] / big
        out["expectation_ms_per_string"] = per_string
        out["break_even_strings"] = out["device_ms"]["median_ms"] / per_string
    return out


def size_rows(log2n, reps, host_reps, rows_out):
    import torch

    n, L = 1 << log2n, log2n
    gen = torch.Generator(device="cuda").manual_seed(log2n)
    xt = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    fn, ex = resident(xt)
    for xm in (0, (1 << 13) | 1):
        expectation = {m: z_strings(L, m) for m in (32, 256, 4096)} if xm == 0 else {}
        row = dict({"what": "pauli_spectrum"}, **measure(ex, L, xm, reps, host_reps, expectation))
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    fn.close()
    del xt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 24, 28])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pauli_spectrum_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("pauli_spectrum_timing.py measures on the GPU: none visible.")
    rows = []
    for log2n in args.log2n:
        size_rows(log2n, args.reps, args.host_reps if log2n < 28 else 1, rows)
        with open(args.out, "w") as f:   # (after every size: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
