"""Dense local operators applied to a result tensor on the device (``ctg_exec_result_op_apply``)
against two other routes to the same ``y`` on the same tensor in the same process -- never against the kernel itself:

* download plus numpy: ``download_result`` and ``np.tensordot`` per term in complex64; for a call of several terms the
  numpy part is timed on the first ``--host-terms`` (2) terms and scaled to the call's number of terms
  (``host_extrapolated``);
* the Pauli route: the same Hermitian operator expanded into Pauli strings (``c_P = trace(P O) / 2^k``, strings whose
  coefficient is exactly zero left out) through ``Executor.pauli_apply_result`` (``ctg_exec_result_pauli_apply``,
  section 17).

One complex64 tensor of ``2^--log2n`` (28) elements (extents all 2) behind a one-tensor tree whose result torch owns;
``y`` is written into a torch buffer (``dev_out``); events on torch's current stream -- the executor's -- bracket a
call; the two device routes alternate; the median of ``--reps`` (7).  Both device calls run the statistics passes
first (``stats_ms``, inside both figures).

Seven calls, every matrix Hermitian: one dense two-qubit term on flat bits (0, 1), on bits (11, 12) -- across the chunk
boundary -- and on the two top bits; one diagonal two-qubit term; ``XX + YY + ZZ`` on a pair; one ``D = 64`` term on
six bits on both sides of bit 12; 27 dense nearest-neighbour terms on bits ``(k, k + 1)``.

No ratio is fixed in advance: a row records what it measured, and says which route was the fastest.

    python tools/op_apply_timing.py [--log2n 28] [--reps 7] [--out profiles/op_apply_timing.json]
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import cotengra_amd as ca  # noqa: E402
from cotengra_amd.contractor import HipContractor  # noqa: E402

PAULI = [np.eye(2, dtype=complex), np.array([[0, 1], [1, 0]], dtype=complex), np.array([[0, -1j], [1j, 0]]),
         np.array([[1, 0], [0, -1]], dtype=complex)]


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


def hermitian(rng, d):
    m = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (m + m.conj().T) / 2


def axes_of(L, bits):
    """Ascending axes of the shape (2,) * L for flat bits ``bits`` (bit b is axis L - 1 - b)."""
    return tuple(sorted(L - 1 - b for b in bits))


def calls(L, rng):
    """``(name, [(axes, matrix), ...])`` per call."""
    x, y, z = PAULI[1], PAULI[2], PAULI[3]
    heis = np.kron(x, x) + np.kron(y, y) + np.kron(z, z)
    six = (0, 3, 8, 12, L - 5, L - 1)
    return (("dense_2q_bits_0_1", [(axes_of(L, (0, 1)), hermitian(rng, 4))]),
            ("dense_2q_bits_11_12", [(axes_of(L, (11, 12)), hermitian(rng, 4))]),
            ("dense_2q_top_bits", [(axes_of(L, (L - 2, L - 1)), hermitian(rng, 4))]),
            ("diagonal_2q", [(axes_of(L, (5, L - 8)), np.diag(rng.standard_normal(4)).astype(complex))]),
            ("xx_yy_zz_pair", [(axes_of(L, (10, L - 8)), heis)]),
            ("d64_six_bits", [(axes_of(L, six), hermitian(rng, 64))]),
            ("27_nearest_neighbour", [(axes_of(L, (k, k + 1)), hermitian(rng, 4)) for k in range(27)]))


def pauli_expansion(L, terms):
    """``(rows, coeffs)``: the Hermitian ``terms`` over the shape (2,) * L as Pauli strings with real coefficients."""
    rows, coeffs = [], []
    for axes, mat in terms:
        k = len(axes)
        for letters in itertools.product(range(4), repeat=k):
            p = np.ones((1, 1), dtype=complex)
            for c in letters:
                p = np.kron(p, PAULI[c])
            c = np.sum(p.T * mat) / 2 ** k
            assert abs(c.imag) <= 1e-12 * max(1.0, np.abs(mat).max()), "a Hermitian matrix has real Pauli coefficients"
            if c.real != 0.0:
                row = [0] * L
                for a, letter in zip(axes, letters):
                    row[a] = letter
                rows.append(row)
                coeffs.append(float(c.real))
    return np.array(rows, dtype=np.uint8).reshape(-1, L), np.array(coeffs, dtype=np.float64)


def host_apply(x, shape, terms, cap):
    """numpy ``y`` in the tensor's own precision for the first ``cap`` terms: ``(ms, y)``."""
    t0 = time.perf_counter()
    xt = x.reshape(shape)
    y = np.zeros(shape, dtype=x.dtype)
    for axes, mat in terms[:cap]:
        k = len(axes)
        o = mat.astype(x.dtype).reshape((2,) * (2 * k))
        y += np.moveaxis(np.tensordot(o, xt, (list(range(k, 2 * k)), list(axes))), list(range(k)), list(axes))
    return 1e3 * (time.perf_counter() - t0), y


def measure(ex, shape, terms, reps, host_reps, host_cap):
    import torch

    L = len(shape)
    ops, coeffs = pauli_expansion(L, terms)
    buf = torch.empty(shape, dtype=torch.complex64, device="cuda")
    other = torch.empty(shape, dtype=torch.complex64, device="cuda")
    ex.op_apply_result(shape, terms, out_ptr=buf.data_ptr())                    # (warm: code objects, the scratch)
    ex.pauli_apply_result(shape, ops, coeffs, out_ptr=other.data_ptr())
    scale = float(sum(np.abs(m).sum() for _, m in terms))
    diff = float((buf - other).abs().max().item())
    assert diff <= 1e-4 * scale * float(buf.abs().max().item() + 1.0), diff       # (the two routes answer the same question)
    dev, pauli, stats, host = [], [], [], []
    cap = min(len(terms), host_cap)
    for r in range(reps):
        for sink, call in ((dev, lambda: ex.op_apply_result(shape, terms, out_ptr=buf.data_ptr())),
                           (pauli, lambda: ex.pauli_apply_result(shape, ops, coeffs, out_ptr=other.data_ptr()))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            sink.append(float(e0.elapsed_time(e1)))
        stats.append(float(sum(ex.sample_info()[4])))
        if r < host_reps:
            t0 = time.perf_counter()
            x = ex.download_result().reshape(-1)
            dl = 1e3 * (time.perf_counter() - t0)
            npy, y = host_apply(x, shape, terms, cap)
            host.append(dl + npy * len(terms) / cap)
            if cap == len(terms) and r == 0:
                assert np.abs(buf.cpu().numpy() - y).max() <= 1e-4 * scale * (np.abs(x).max() + 1.0)
            del x, y
    out = {"terms": len(terms), "dims": [int(m.shape[0]) for _, m in terms][:4], "pauli_strings": int(len(ops)),
           "op_apply_ms": _summary(dev), "pauli_apply_ms": _summary(pauli), "stats_ms": _summary(stats),
           "download_plus_numpy_ms": _summary(host), "host_terms_timed": cap, "host_extrapolated": cap < len(terms),
           "max_abs_difference_of_the_device_routes": diff}
    a, b, c = out["op_apply_ms"]["median_ms"], out["pauli_apply_ms"]["median_ms"], out["download_plus_numpy_ms"]["median_ms"]
    out["pauli_over_op_apply"] = b / a
    out["numpy_over_op_apply"] = c / a
    out["fastest"] = min((a, "op_apply"), (b, "pauli_apply"), (c, "download_plus_numpy"))[1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-terms", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "op_apply_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("op_apply_timing.py measures on the GPU: none visible.")
    L = args.log2n
    if L < 20:
        raise SystemExit("op_apply_timing.py: --log2n below 20 measures overheads.")
    gen = torch.Generator(device="cuda").manual_seed(L)
    xt = torch.view_as_complex(torch.randn((1 << L, 2), generator=gen, device="cuda", dtype=torch.float32))
    fn, ex = resident(xt)
    shape = (2,) * L
    rows = []
    for name, terms in calls(L, np.random.default_rng(19)):
        m = measure(ex, shape, terms, args.reps, args.host_reps, args.host_terms)
        row = dict({"what": "op_apply", "kernel": ex.op_apply_variant(shape, terms), "call": name, "dtype": "complex64",
                    "log2_n": L}, **m)
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(args.out, "w") as f:   # (after every call: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)
    fn.close()


if __name__ == "__main__":
    main()
