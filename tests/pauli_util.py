"""Reference and tolerance for expectation values of Pauli strings over the result tensor (tests/test_gpu_pauli.py,
tests/test_pauli_host.py).

Reference: ``value(P) = sum over j of conj(x[j]) (P x)[j]`` in complex128 / float64.  ``P x`` is formed on the tensor
reshaped to ``shape``: the sign vector ``(1, -1)`` along every Z and Y axis, ``np.flip`` along every X and Y axis
(``Y = i X Z``), the factor ``i^ny``; then ``np.vdot(x, P x).real``.  Codes: 0, 1, 2, 3 = I, X, Y, Z.

Tolerance, derived and not tuned: the value is a sum of ``n`` terms of one (real data) or two (complex data) real
products each, ``m = n`` or ``2 n`` products in all.  Each product is rounded at most once; by Cauchy-Schwarz the
absolute values of the terms sum to at most ``sum |x|^2``.  Any two orders of summation are each within ``(m + 1) 2^-53``
of that, so

    |got - ref| <= 2 (m + 1) 2^-53 sum |x|^2.

No string is ever excluded.  (tests/test_pauli_host.py compares two numpy summation orders at ``n = 2^18`` against this
bound and shows that one term of median size with the wrong sign exceeds it.)"""
import numpy as np

LETTERS = "IXYZ"
PAULI = (np.eye(2, dtype=complex), np.array([[0, 1], [1, 0]], dtype=complex),
         np.array([[0, -1j], [1j, 0]], dtype=complex), np.array([[1, 0], [0, -1]], dtype=complex))


def widen(x):
    x = np.asarray(x)
    return x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)


def apply_string(x, shape, row):
    """``P x`` (an array of ``shape``) for one row of codes over the widened tensor ``x``."""
    shape = tuple(int(d) for d in shape)
    y = x.reshape(shape)
    ny = 0
    for a, op in enumerate(row):
        if op == 0:
            continue
        assert shape[a] == 2, (a, shape[a], op)
        if op in (2, 3):
            sign = np.ones(2)
            sign[1] = -1.0
            y = y * sign.reshape((1,) * a + (2,) + (1,) * (len(shape) - a - 1))
        if op in (1, 2):
            y = np.flip(y, axis=a)
        ny += op == 2
    phase = (1.0, 1j, -1.0, -1j)[ny % 4]
    return y * phase if ny else y


def pauli_reference(x, shape, ops):
    """The float64 values of the strings ``ops`` (``(m, rank)`` codes, or one row: a 0-d result) on ``x`` of ``shape``."""
    w = widen(x).reshape(-1)
    rows = np.asarray(ops)
    single = rows.ndim == 1
    rows = rows.reshape(-1, len(tuple(shape)))
    out = np.empty(len(rows), dtype=np.float64)
    for s, row in enumerate(rows.tolist()):
        out[s] = float(np.real(np.vdot(w, apply_string(w, shape, row).reshape(-1))))
    return out[0] if single else out


def pauli_tol(x, n):
    """``2 (m + 1) 2^-53 sum |x|^2`` with ``m = 2 n`` products for complex data, ``n`` for real data."""
    w = widen(x).reshape(-1)
    m = 2 * n if w.dtype.kind == "c" else n
    norm = float(np.sum(w.real * w.real + (w.imag * w.imag if w.dtype.kind == "c" else 0.0)))
    return 2.0 * (m + 1) * 2.0 ** -53 * norm


def codes(text):
    """``"XIZY"`` -> ``[1, 0, 3, 2]``."""
    return [LETTERS.index(c) for c in text.upper()]


def bit_string(L, letters):
    """The row of codes over the shape ``(2,) * L`` with ``letters[b]`` on bit ``b`` of the flat index (axis
    ``L - 1 - b``)."""
    row = [0] * L
    for b, c in letters.items():
        assert 0 <= b < L and row[L - 1 - b] == 0, (b, L)
        row[L - 1 - b] = LETTERS.index(c)
    return row


def dense_string(row, shape):
    """The dense matrix of a string: the Kronecker product of its letters (identities of the axes' extents for I)."""
    P = np.ones((1, 1), dtype=complex)
    for op, d in zip(row, shape):
        P = np.kron(P, PAULI[op] if op else np.eye(int(d), dtype=complex))
    return P


def check_pauli(got, x, shape, ops, ref=None):
    """Assert every value of ``got`` within ``pauli_tol`` of the reference; returns the reference."""
    ref = pauli_reference(x, shape, ops) if ref is None else ref
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    n = int(np.prod(shape, dtype=np.int64))
    tol = pauli_tol(x, n)
    err = np.abs(got - ref)
    frac = float(err.max() / tol) if err.size and tol > 0 else 0.0
    print(f"pauli shape={tuple(shape) if len(shape) < 8 else (2, '...', len(shape))} strings={len(ref)} n={n} "
          f"max err/bound={frac:.3e}")
    assert np.all(err <= tol), (float(err.max()), tol, int(np.argmax(err)))
    return ref
