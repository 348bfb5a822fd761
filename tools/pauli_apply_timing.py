"""A Pauli sum applied to a result tensor on the device (``ctg_exec_result_pauli_apply``) against
two yardsticks on the same tensor in the same process, and the energy-and-gradient step built on it against the route
there was before.

The apply call, on complex64 tensors of 2^20 / 2^24 / 2^28 elements (extents all 2) behind a one-tensor tree whose
result torch owns, written into a torch buffer (``dev_out``); events on torch's current stream -- the executor's --
bracket a call:

* the floor of the traffic: ``(groups + 1)`` times one read of the tensor, ``prob_block_kernel`` alone
  (``sample_info``'s ``pass_ms[0]``) -- one read per X-mask group and the write of ``y``;
* the route there was before: ``download_result`` and numpy (``np.flip`` on the X / Y axes, a broadcast sign tensor over
  the Z / Y axes, the sum over the strings) in complex64; from 2^24 elements on it is timed on the first
  ``--host-strings`` (2) strings and its numpy part scaled to the call's number of strings (``host_extrapolated``).

Five calls: one Z-type string; 32 and 64 Z-type strings (one group: one and two passes); one weight-20 mixed string
with X bits on both sides of bit 12; 16 strings with 16 different X masks.  The measurements of a call alternate; the
median of ``--reps`` (11).

End to end, on a ``--qubits`` (22) qubit circuit of ``--depth`` (8) layers with every qubit open, the tree sliced to
``2^--target`` (18) elements, complex64, 24 random strings: ``HipContractor.energy`` with all gradients against
``contract`` -> download -> numpy ``H x`` -> ``contract_vjp`` with the uploaded cotangent.

No ratio is fixed in advance: a row records what it measured.

    python tools/pauli_apply_timing.py [--log2n 20 24 28] [--reps 11] [--out profiles/pauli_apply_timing.json]
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
from cotengra_amd import circuits, runtime  # noqa: E402
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
    masks = [bit_string(L, {k: "X", (k + 5) % L: "Z"}) for k in range(16)]
    return (("1_z_string", [bit_string(L, {0: "Z", 13: "Z", L - 1: "Z"})]), ("32_z_strings", zz[:32]), ("64_z_strings", zz),
            ("1_mixed_weight_20", [bit_string(L, mixed)]), ("16_strings_16_x_masks", masks))


def host_apply(x, shape, rows, coeffs, cap):
    """numpy ``H x`` in the tensor's own precision for the first ``cap`` strings: ``(ms, y)``."""
    t0 = time.perf_counter()
    xt = x.reshape(shape)
    real = xt.real.dtype
    y = np.zeros(shape, dtype=x.dtype)
    for row, c in zip(rows[:cap], coeffs[:cap]):
        sign, ny = np.ones((1,) * len(shape), dtype=real), 0
        for a, op in enumerate(row):
            if op in (2, 3):
                v = np.ones(2, dtype=real)
                v[1] = -1.0
                sign = sign * v.reshape((1,) * a + (2,) + (1,) * (len(shape) - a - 1))
            ny += op == 2
        flips = [a for a, op in enumerate(row) if op in (1, 2)]
        t = xt * sign if sign.ndim and sign.size > 1 else xt     # (the signs go by the element read, then the flips)
        t = np.flip(t, axis=flips) if flips else t
        y += t * np.asarray((1.0, 1j, -1.0, -1j)[ny % 4] * c, dtype=x.dtype)
    return 1e3 * (time.perf_counter() - t0), y


def measure(ex, shape, rows, reps, host_reps, host_cap):
    """Alternating: the floor, the device call between two events, the numpy route."""
    import torch

    ops = np.array(rows, dtype=np.uint8)
    coeffs = np.linspace(-1.0, 1.0, len(rows)) + 0.0625
    buf = torch.empty(shape, dtype=torch.complex64, device="cuda")
    ex.pauli_apply_result(shape, ops, coeffs, out_ptr=buf.data_ptr())
    floor, dev, stats, wall, host = [], [], [], [], []
    cap = min(len(rows), host_cap)
    for r in range(reps):
        ex.result_stats()
        floor.append(float(ex.sample_info()[4][0]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        ex.pauli_apply_result(shape, ops, coeffs, out_ptr=buf.data_ptr())
        e1.record()
        e1.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(float(e0.elapsed_time(e1)))
        stats.append(float(sum(ex.sample_info()[4])))
        if r < host_reps:
            t0 = time.perf_counter()
            x = ex.download_result().reshape(-1)
            dl = 1e3 * (time.perf_counter() - t0)
            npy, y = host_apply(x, shape, rows, coeffs, cap)
            host.append(dl + npy * len(rows) / cap)
            if cap == len(rows) and r == 0:
                # (the two routes answer the same question: complex64 sums on the host, so a loose check)
                got = buf.cpu().numpy()
                assert np.abs(got - y).max() <= 1e-4 * np.abs(coeffs).sum() * np.abs(x).max()
    groups = len({xm for xm, _, _ in runtime.pauli_masks(shape, rows)})
    f = _summary(floor)["median_ms"] * (groups + 1)
    out = {"strings": len(rows), "x_mask_groups": groups, "floor_prob_block_kernel": _summary(floor), "floor_ms": f,
           "device_ms": _summary(dev), "stats_ms": _summary(stats), "wall_ms": _summary(wall),
           "download_plus_numpy": _summary(host), "host_strings_timed": cap, "host_extrapolated": cap < len(rows)}
    out["device_over_floor"] = out["device_ms"]["median_ms"] / f
    out["kernel_over_floor"] = (out["device_ms"]["median_ms"] - out["stats_ms"]["median_ms"]) / f
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
        row = dict({"what": "pauli_apply", "kernel": ex.pauli_apply_variant(shape, rows), "call": name, "dtype": "complex64",
                    "log2_n": log2n}, **m)
        rows_out.append(row)
        print(json.dumps(row), flush=True)
    fn.close()
    del xt
    torch.cuda.empty_cache()


def random_circuit(n, depth, seed):
    rng = np.random.default_rng(seed)
    gates = []
    for d in range(depth):
        for q in range(n):
            name = ("x_1_2", "y_1_2", "hz_1_2", "rz")[int(rng.integers(0, 4))]
            gates.append((name, (q,), (float(rng.normal()),) if name == "rz" else ()))
        for q in range(d % 2, n - 1, 2):
            gates.append(("fs", (q, q + 1), (float(rng.normal()), float(rng.normal()))))
    return gates


def end_to_end(n, depth, target, reps, rows_out):
    """``energy`` with all gradients against contract -> download -> numpy ``H x`` -> ``contract_vjp``."""
    inputs, output, sd, arrays = circuits.circuit_to_network(n, random_circuit(n, depth, 22), "?" * n, simplify=True,
                                                             dtype="complex64")
    tree = ca.array_contract_tree(inputs, output, sd)
    tree = tree.slice(target_size=2 ** target)
    rng = np.random.default_rng(5)
    rows = [[0] * n] + rng.integers(0, 4, size=(7, n)).tolist()
    rows += [bit_string(n, {int(a): "Z", int(b): "Z"}) for a, b in (rng.choice(n, 2, replace=False) for _ in range(16))]
    texts = ["".join("IXYZ"[c] for c in row) for row in rows]
    coeffs = rng.standard_normal(len(rows))
    shape = (2,) * n
    new, old, parts = [], [], []
    tree.contract_energy(arrays, texts, coeffs=coeffs)   # (plans and executors exist from here on)
    tree.contract_vjp(arrays, np.zeros(shape, dtype="complex64"))
    for r in range(reps):
        t0 = time.perf_counter()
        res = tree.contract_energy(arrays, texts, coeffs=coeffs)
        new.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        x = np.asarray(tree.contract(arrays))
        t1 = time.perf_counter()
        npy, y = host_apply(x.reshape(-1), shape, rows, coeffs, len(rows))
        energy = float(np.real(np.vdot(x, y)))
        t2 = time.perf_counter()
        grads = tree.contract_vjp(arrays, np.conj(2.0 * y))
        t3 = time.perf_counter()
        old.append(1e3 * (t3 - t0))
        parts.append((1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
        if r == 0:
            assert abs(energy - res.energy) <= 1e-3 * np.abs(coeffs).sum()
            for g, h in zip(res.grads, grads):
                assert np.abs(g - np.conj(h)).max() <= 1e-3 * max(1.0, np.abs(g).max())
    med = lambda k: sorted(p[k] for p in parts)[len(parts) // 2]   # noqa: E731
    row = {"what": "energy_and_gradients", "qubits": n, "depth": depth, "dtype": "complex64", "leaves": tree.N,
           "nslices": int(tree.nslices), "strings": len(rows), "energy_ms": _summary(new), "before_ms": _summary(old),
           "before_contract_download_ms": med(0), "before_numpy_ms": med(1), "before_vjp_ms": med(2)}
    row["before_over_energy"] = row["before_ms"]["median_ms"] / row["energy_ms"]["median_ms"]
    rows_out.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 24, 28])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps-large", type=int, default=3)
    ap.add_argument("--host-strings", type=int, default=2)
    ap.add_argument("--qubits", type=int, default=22)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--target", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pauli_apply_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("pauli_apply_timing.py measures on the GPU: none visible.")
    rows = []
    for log2n in args.log2n:
        size_rows(log2n, args.reps, args.reps if log2n < 28 else args.host_reps_large,
                  args.host_strings if log2n >= 24 else 1 << 30, rows)
        with open(args.out, "w") as f:   # (after every size: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)
    if args.qubits:
        end_to_end(args.qubits, args.depth, args.target, min(args.reps, 5), rows)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
