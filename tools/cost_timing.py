"""The cost statistics of a result tensor on the device (``ctg_exec_result_cost``) against three
yardsticks on the same tensor in the same process:

* its floor of memory traffic: the vector is zeroed (a write of ``8 n`` bytes: half a copy), the tile pass and every
  strided pass read and write ``8 n`` bytes (a plain fp64 copy of ``n`` doubles, ``Tensor.copy_``, timed between events
  in the same run), and every digit pass and the final pass read ``(C, x)``, ``16 n`` bytes for complex64 -- twice the
  read of the tensor alone, which is ``prob_block_kernel`` (``sample_info``'s ``pass_ms[0]``):
  ``floor = (1/2 + 1 + passes) * copy + (digit launches + 1) * 2 * read``;
* ``expectation``'s route (``ctg_exec_result_pauli``) for the mean alone: the terms' values, summed on the host;
* ``download_result`` and numpy: the cost vector by an in-place transform, a stable argsort, a cumulative sum.

complex64 tensors of 2^20 / 2^24 / 2^28 elements, extents all 2, behind a one-tensor tree whose result torch owns, so
that events on torch's current stream -- the executor's stream -- bracket a call.  Two costs: the ring's MaxCut cost
(integer values, ``L / 2 + 1`` distinct ones: every lane of a wave adds into a few LDS bins) and 300 Gaussian terms (all
values distinct); one level (0.1) and four (2^-10, 0.1, 0.5, 1.0), lower tail, no histogram.  Measurements alternate; the
median of ``--reps`` (7).  The numpy route runs once per size up to ``--host-max-log2n`` (24).

No ratio is fixed in advance: a row records what multiple of the floor the device time is.

    python tools/cost_timing.py [--log2n 20 24 28] [--reps 7] [--out profiles/cost_timing.json]
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

LEVELS = {1: (0.1,), 4: (2.0 ** -10, 0.1, 0.5, 1.0)}


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


def cost_terms(kind, L):
    """``(ops, coeffs)``: the ring's MaxCut cost, or 300 Gaussian terms on random masks."""
    if kind == "ring":
        ops = np.zeros((L + 1, L), dtype=np.uint8)
        for q in range(L):
            ops[q + 1, q] = ops[q + 1, (q + 1) % L] = 3
        return ops, np.array([0.5 * L] + [-0.5] * L)
    rng = np.random.default_rng(L)
    return (rng.integers(0, 2, size=(300, L)) * 3).astype(np.uint8), rng.standard_normal(300)


def host_statistics(ex, L, ops, coeffs, levels):
    """Download + numpy: ``(ms, mean, thresholds)``."""
    t0 = time.perf_counter()
    x = ex.download_result().reshape(-1)
    p = x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2
    v = np.zeros(1 << L)
    bit = 1 << np.arange(L - 1, -1, -1)
    for row, c in zip(ops, coeffs):
        v[int(np.sum(bit[row == 3]))] += c
    for b in range(L):
        t = v.reshape(-1, 2, 1 << b)
        lo = t[:, 0, :].copy()
        t[:, 0, :] += t[:, 1, :]
        np.subtract(lo, t[:, 1, :], out=t[:, 1, :])
    order = np.argsort(v, kind="stable")
    cum = np.cumsum(p[order])
    ts = [float(v[order[min(int(np.searchsorted(cum, a * cum[-1])), v.size - 1)]]) for a in levels]
    mean = float(np.dot(p, v))
    return 1e3 * (time.perf_counter() - t0), mean, ts


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1)), 1e3 * (time.perf_counter() - t0), out


def measure(ex, L, reps, host):
    import torch

    n = 1 << L
    shape = (2,) * L
    src = torch.zeros(n, dtype=torch.float64, device="cuda")
    dst = torch.empty(n, dtype=torch.float64, device="cuda")
    cases = [(kind, nl) for kind in ("ring", "gaussian") for nl in (1, 4)]
    terms = {kind: cost_terms(kind, L) for kind in ("ring", "gaussian")}
    for kind, nl in cases:
        ex.cost_result(shape, ops=terms[kind][0], coeffs=terms[kind][1], levels=LEVELS[nl])
    read, copy, stats = [], [], []
    dev, wall = {c: [] for c in cases}, {c: [] for c in cases}
    expect = []
    last = {}
    for r in range(reps):
        ex.result_stats()
        read.append(float(ex.sample_info()[4][0]))
        copy.append(timed(lambda: dst.copy_(src))[0])
        for c in cases:
            ops, co = terms[c[0]]
            d, w, last[c] = timed(lambda: ex.cost_result(shape, ops=ops, coeffs=co, levels=LEVELS[c[1]]))
            dev[c].append(d)
            wall[c].append(w)
            stats.append(float(sum(ex.sample_info()[4])))
        expect.append(timed(lambda: ex.pauli_result(shape, terms["ring"][0]))[0])
        print(f"2^{L}: repetition {r + 1} of {reps}", file=sys.stderr, flush=True)
    rows = []
    read_ms, copy_ms = _summary(read)["median_ms"], _summary(copy)["median_ms"]
    for c in cases:
        kind, nl = c
        plan = ex.cost_plan(shape, "terms", nl, 0)
        floor = (1.5 + plan.passes) * copy_ms + (plan.digit_launches + 1) * 2 * read_ms
        row = {"what": "cost", "log2_n": L, "dtype": "complex64", "cost": kind, "levels": nl, "passes": plan.passes,
               "digit_launches": plan.digit_launches, "grid": plan.grid, "read_prob_block_kernel": _summary(read),
               "copy_8n_read_plus_write": _summary(copy), "floor_ms": floor, "device_ms": _summary(dev[c]), "wall_ms": _summary(wall[c]),
               "stats_ms": _summary(stats)}
        row["kernels_ms"] = row["device_ms"]["median_ms"] - row["stats_ms"]["median_ms"]
        row["device_over_floor"] = row["device_ms"]["median_ms"] / floor
        row["kernels_over_floor"] = row["kernels_ms"] / floor
        if kind == "ring":
            row["expectation_mean_alone_device_ms"] = _summary(expect)
        if host:
            ms, mean, ts = host_statistics(ex, L, terms[kind][0], terms[kind][1], LEVELS[nl])
            words = last[c][0]
            f = words.view(np.float64)
            norm = float(f[16])
            assert abs(float(f[2]) - mean) <= 1e-9 * norm * float(np.sum(np.abs(terms[kind][1]))), (float(f[2]), mean)
            row["download_plus_numpy_ms"] = ms
            row["numpy_over_wall"] = ms / row["wall_ms"]["median_ms"]
            row["thresholds_device"] = [float(f[25 + 5 * l]) for l in range(nl)]
            row["thresholds_numpy"] = ts
        rows.append(row)
        print(json.dumps(row), flush=True)
    for nl in (1, 4):
        ring = next(r for r in rows if r["cost"] == "ring" and r["levels"] == nl)
        gauss = next(r for r in rows if r["cost"] == "gaussian" and r["levels"] == nl)
        ring["ring_over_gaussian_kernels"] = ring["kernels_ms"] / gauss["kernels_ms"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 24, 28])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max-log2n", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cost_timing.py measures on the GPU: none visible.")
    rows = []
    for log2n in args.log2n:
        n = 1 << log2n
        gen = torch.Generator(device="cuda").manual_seed(log2n)
        xt = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
        fn, ex = resident(xt)
        rows += measure(ex, log2n, args.reps, log2n <= args.host_max_log2n)
        fn.close()
        del xt
        torch.cuda.empty_cache()
        with open(args.out, "w") as f:   # (after every size: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
