"""Reference of the range audit in numpy (tests/test_gpu_range_audit.py, tests/test_range_audit_host.py).

A tensor is read as its fp32 components (a complex64 tensor: re, im, re, im ...).  The reference is

    hist   = np.bincount((bits >> 23) & 0xff, minlength=256)
    zeros  = count of components whose bits without the sign are 0
    sumsq  = sum over the finite components of float64(x)^2, summed by numpy in float64

Counts are exact.  Each square is exact in float64 (a 24-bit significand squared has 48 bits), so the only error
of ``sumsq`` is that of adding n non-negative doubles: any order is within (n - 1) 2^-53 sum of the exact sum, and
the device and numpy each commit one such error.  Hence ``sumsq_tol = n 2^-53 sumsq`` -- the distance of two
summation orders (for n = 1 there is nothing to add and both are exact).  Nothing here comes from the device.
"""
import numpy as np

RANGE_WORDS = 260


def components(x):
    """The fp32 components of a float32 / complex64 array, in memory order."""
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.dtype("float32"), np.dtype("complex64")), x.dtype
    return x.reshape(-1).view(np.float32)


def reference(x):
    """``(hist[256], zeros, nonfinite-free sumsq, n)`` of the array's components."""
    f = components(x)
    bits = f.view(np.uint32)
    ex = (bits >> np.uint32(23)) & np.uint32(0xFF)
    hist = np.bincount(ex.astype(np.int64), minlength=256).astype(np.int64)
    zeros = int(np.count_nonzero((bits & np.uint32(0x7FFFFFFF)) == 0))
    finite = f[ex != 255].astype(np.float64)
    return hist, zeros, float(np.sum(finite * finite)), int(f.size)


def sumsq_tol(n, sumsq):
    return n * 2.0 ** -53 * sumsq


def reference_row(x):
    """The row the library returns for an audited tensor, and its sum of squares."""
    hist, zeros, sumsq, n = reference(x)
    row = np.zeros(RANGE_WORDS, dtype=np.int64)
    row[0], row[1], row[2] = 1, n, zeros
    row[4:] = hist
    return row, sumsq


def check_row(row, sumsq, x):
    """Assert that (row, sumsq) is the reference of the bytes of ``x``."""
    ref, ref_sq = reference_row(x)
    row = np.asarray(row)
    assert row[0] == 1 and row[3] == 0, row[:4]
    assert row[1] == ref[1], (row[1], ref[1])
    assert row[2] == ref[2], ("zeros", row[2], ref[2])
    bad = np.flatnonzero(row[4:] != ref[4:])
    assert bad.size == 0, [(int(b), int(row[4 + b]), int(ref[4 + b])) for b in bad[:8]]
    assert abs(sumsq - ref_sq) <= sumsq_tol(ref[1], ref_sq), (sumsq, ref_sq, sumsq_tol(ref[1], ref_sq))


def shifted_equal(hist, ref):
    """Is ``hist`` the histogram ``ref`` moved by one uniform number of bins (the upload's power of two), zeros
    staying in bin 0?  Returns the shift, or None.  (Exact values only: no component may cross into or out of the
    subnormals, which the callers' values -- 0, +-1/2, +-1, +-2 and their small sums of products -- never do.)"""
    hist, ref = np.asarray(hist), np.asarray(ref)
    if hist[0] != ref[0] or hist[255] != ref[255]:
        return None
    a, b = np.flatnonzero(hist[1:255]), np.flatnonzero(ref[1:255])
    if a.size != b.size:
        return None
    if a.size == 0:
        return 0
    shift = int(a[0] - b[0])
    if np.array_equal(a - shift, b) and np.array_equal(hist[1:255][a], ref[1:255][b]):
        return shift
    return None


def node_tensors(tree, arrays, slice_id=0, dtype="complex128"):
    """Every node's tensor of slice ``slice_id`` by plain einsum in ``dtype`` (the oracle's walk): ``{node: array}``
    with the leaves included.  A step's result is a transposition of its node's tensor, and a histogram does not
    see a transposition."""
    from oracle import contract_ref as orc

    xs = orc.slice_arrays(tree, [np.asarray(a).astype(dtype) for a in arrays], slice_id) if tree.sliced_inds else \
        [np.asarray(a).astype(dtype) for a in arrays]
    temps = dict(zip(tree.gen_leaves(), xs))
    for p, l, r in tree.traverse():
        temps[p] = orc.einsum(tree.get_einsum_eq(p), temps[l], temps[r])
    return temps


def small_exact_arrays(tree, seed, dtype="complex64"):
    """Inputs with components in {0, +-1/2, +-1, +-2}: every product and every sum of a small tree is exact in
    fp32 (and in fp16 x 2 and bf16 x 3 limbs), so all arithmetics and the float64 einsum hold the same values."""
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=np.float32)
    out = []
    for term in tree.inputs:
        shape = tuple(tree.size_dict[ix] for ix in term)
        if np.dtype(dtype).kind == "c":
            out.append((rng.choice(vals, size=shape) + 1j * rng.choice(vals, size=shape)).astype(dtype))
        else:
            out.append(rng.choice(vals, size=shape).astype(dtype))
    return out
