"""Reference and tolerance for reduced density matrices of the result tensor (tests/test_gpu_rdm.py,
tests/test_rdm_host.py).

Reference: ``rho_ref = X @ X.conj().T`` in complex128 / float64, ``X`` the tensor moved to ``(kept axes...,
other axes...)`` and reshaped to ``(D, t)``.

Tolerance, derived and not tuned: each real component of ``rho[a, b]`` is a sum of ``m`` products, ``m = 2 t`` for a
complex tensor and ``t`` for a real one.  Each product is rounded at most once and the sums are added in some order;
their absolute values sum to at most ``sqrt(rho[a, a] rho[b, b])`` (Cauchy-Schwarz).  The device and numpy each commit
at most ``(m + 1) 2^-53`` of that, so per component

    |got - ref| <= 2 (m + 1) 2^-53 sqrt(ref[a, a] ref[b, b]).

No entry is ever excluded.  (tests/test_rdm_host.py compares two numpy summation orders at ``t = 2^18`` against this
bound and prints the fraction of it they use.)"""
import numpy as np


def rdm_matrix(x, shape, keep_axes):
    """``x`` as the ``(D, t)`` matrix of a request, in complex128 / float64; kept axes in the order of ``keep_axes``."""
    x = np.asarray(x)
    wide = np.complex128 if x.dtype.kind == "c" else np.float64
    keep_axes = list(keep_axes)
    other = [a for a in range(len(shape)) if a not in keep_axes]
    d = int(np.prod([shape[a] for a in keep_axes], dtype=np.int64))
    return np.ascontiguousarray(x.reshape(tuple(shape)).transpose(keep_axes + other).reshape(d, -1)).astype(wide)


def rdm_reference(x, shape, keep_axes):
    X = rdm_matrix(x, shape, keep_axes)
    return X @ X.conj().T


def rdm_tol(ref, t):
    """Per real component: ``2 (m + 1) 2^-53 sqrt(ref[a, a] ref[b, b])``, ``m = 2 t`` (complex) or ``t`` (real)."""
    ref = np.asarray(ref)
    m = 2 * t if ref.dtype.kind == "c" else t
    d = np.sqrt(np.abs(np.diag(ref).real))
    return 2.0 * (m + 1) * 2.0 ** -53 * np.outer(d, d)


def rdm_errors(got, ref):
    """The larger of the real and the imaginary component's ``|got - ref|`` per entry."""
    diff = np.asarray(got) - np.asarray(ref)
    return np.maximum(np.abs(diff.real), np.abs(diff.imag)) if diff.dtype.kind == "c" else np.abs(diff)


def check_rdm(got, x, shape, keep_axes, ref=None):
    """Assert ``got`` within ``rdm_tol`` of the reference, every entry, per real component; returns the reference."""
    ref = rdm_reference(x, shape, keep_axes) if ref is None else ref
    got = np.asarray(got)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.dtype, ref.shape)
    t = int(np.prod(shape, dtype=np.int64)) // max(ref.shape[0], 1)
    err, tol = rdm_errors(got, ref), rdm_tol(ref, t)
    frac = float(np.max(err / np.where(tol > 0, tol, 1.0)))
    print(f"rdm shape={tuple(shape) if len(shape) < 8 else (2, '...', len(shape))} keep={list(keep_axes)} D={ref.shape[0]} "
          f"t={t} max err/bound={frac:.3e}")
    assert np.all(err <= tol), (float(err.max()), frac)
    return ref
