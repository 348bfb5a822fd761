"""Model and tolerance of the Pauli spectrum (tests/test_spectrum_host.py, tests/test_gpu_spectrum.py; DESIGN.md section
21): ``S[z] = <x| P(xm, z) |x>`` for all ``z`` by one Walsh-Hadamard transform.

Model: what ``ctg_exec_result_pauli_spectrum`` computes, operation for operation, in numpy -- ``u`` from ``p = x[j ^ xm]``
and ``w = x[j]`` with every product and sum a separate float64 ufunc (numpy contracts nothing), the butterflies over the
bits in ASCENDING order, ``(a, c) -> (a + c, a - c)``, the sign ``(-1)^ceil(ny / 2)`` as a negation, ``+0.0`` for odd
``ny`` of real data.  The device must equal it bit for bit on any data: ``assert_same_bits``.

Tolerance against ``pauli_util.pauli_reference``, derived as ``pauli_util.pauli_tol`` is and never from device output: a
value is a fixed-order sum of ``n`` terms, each carrying at most 8 rounded operations for complex data (4 products, 3
sums, the butterfly tree counted once per term) and 1 product for real data; by Cauchy-Schwarz ``sum |terms| <=
sqrt(2) sum |x|^2`` (complex: ``|re + im| <= sqrt(2) |conj(p) w|``) or ``sum |x|^2`` (real).  Two orders of summation are
each within ``(ops + 1) 2^-53`` of that, hence

    |got - ref| <= 2 (8 n + 1) 2^-53 sqrt(2) sum |x|^2   (complex),     2 (n + 1) 2^-53 sum |x|^2   (real).

No ``z`` is ever excluded."""
import numpy as np

import pauli_util as pu


def flip_mask(shape, flips):
    """``xm``: the flat-index bits (log2 of the row-major strides) of the axes with ``flips[a] = 1``."""
    xm, stride = 0, 1
    for d, f in zip(reversed(tuple(shape)), reversed(tuple(flips))):
        assert d in (1, 2) and f in (0, 1) and (d == 2 or not f), (d, f)
        if f:
            xm |= stride
        stride *= d
    return xm


def flips_of(L, xm):
    """The flips over the shape ``(2,) * L`` whose mask is ``xm`` (bit ``b`` is axis ``L - 1 - b``)."""
    return [(xm >> (L - 1 - a)) & 1 for a in range(L)]


def popcount(v):
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros(v.shape, dtype=np.int64)
    for b in range(64):
        out += ((v >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return out


def spectrum_model(x, shape, flips):
    """The float64 array of ``shape`` the device returns for the tensor ``x``, bit for bit."""
    x = np.asarray(x).reshape(-1)
    n = x.size
    L = n.bit_length() - 1
    assert n == 1 << L == int(np.prod(shape, dtype=np.int64))
    xm = flip_mask(shape, flips)
    j = np.arange(n, dtype=np.int64)
    p, w = x[j ^ xm], x
    if x.dtype.kind == "c":
        a, b, c, d = (t.astype(np.float64) for t in (p.real, p.imag, w.real, w.imag))
        u = (a * c + b * d) + (a * d - b * c)
    else:
        u = p.astype(np.float64) * w.astype(np.float64)
    v = u
    for b in range(L):
        t = v.reshape(-1, 2, 1 << b)
        v = np.stack([t[:, 0, :] + t[:, 1, :], t[:, 0, :] - t[:, 1, :]], axis=1).reshape(n)
    ny = popcount(j & xm)
    v = np.where(((ny + 1) // 2) % 2 == 1, -v, v)
    if x.dtype.kind != "c":
        v = np.where(ny % 2 == 1, 0.0, v)
    return np.ascontiguousarray(v, dtype=np.float64).reshape(tuple(shape))


def string_of(shape, flips, z):
    """The row of codes 0 .. 3 (I, X, Y, Z) of ``P(xm, z)`` over ``shape``: Y where the axis is flipped and the
    coordinate of ``z`` is 1, X where flipped and 0, Z where not flipped and 1."""
    coords = np.unravel_index(int(z), tuple(shape)) if len(shape) else ()
    return [(2 if c else 1) if f else (3 if c else 0) for f, c in zip(flips, coords)]


def spectrum_tol(x, n):
    """``2 (8 n + 1) 2^-53 sqrt(2) sum |x|^2`` for complex data, ``2 (n + 1) 2^-53 sum |x|^2`` for real data."""
    w = pu.widen(x).reshape(-1)
    if w.dtype.kind == "c":
        return 2.0 * (8 * n + 1) * 2.0 ** -53 * np.sqrt(2.0) * float(np.sum(w.real * w.real + w.imag * w.imag))
    return 2.0 * (n + 1) * 2.0 ** -53 * float(np.sum(w * w))


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and want.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    same = got.view(np.uint64) == want.view(np.uint64)
    if not same.all():
        bad = np.flatnonzero(~same.reshape(-1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} entries differ in their bits; first at {i}: "
                             f"{got.reshape(-1)[i]!r} vs {want.reshape(-1)[i]!r}")
