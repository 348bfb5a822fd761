"""References for top-k and marginals of the result tensor (tests/test_gpu_result_reduce.py,
tests/test_result_reduce_host.py), built on ``sample_util.probabilities``: ``p = re*re + im*im`` in float64.

Top-k is exact: ``p`` is the same double on both sides, so the device must return numpy's
``lexsort((index, -p))[:k]`` index for index and bit for bit.

A marginal is a sum of ``t`` non-negative doubles per output.  Any order of summing them is within
``(t - 1) 2^-53`` of the exact sum, relatively; the device's order and numpy's each commit one such error.  So the
tolerance is ``2 t 2^-53 ref`` PER OUTPUT -- derived, not tuned.  (Two different orders over 2^18 terms per output
differed by 2.7e-14 relative on the CPU, against a bound of 5.8e-11.)  No case is ever excluded from either check.
"""
import numpy as np

import sample_util as su


def topk_reference(x, k):
    """``(indices, p at them)`` of the first ``k`` members in the order p descending, lower index first."""
    p = su.probabilities(x)
    idx = np.lexsort((np.arange(p.size), -p))[:k].astype(np.int64)
    return idx, p[idx]


def marginal_reference(x, shape, keep_axes):
    """``p.reshape(shape)`` summed over the axes not in ``keep_axes`` (kept axes in the tensor's own order)."""
    p = su.probabilities(x).reshape(tuple(shape))
    other = tuple(a for a in range(len(shape)) if a not in set(keep_axes))
    return p.sum(axis=other) if other else p.copy()


def marginal_tol(ref, t):
    """Per output: ``2 t 2^-53 ref`` for ``t`` elements per output."""
    return 2.0 * t * 2.0 ** -53 * np.asarray(ref, dtype=np.float64)


def check_marginal(got, x, shape, keep_axes):
    """Assert ``got`` (kept axes in the tensor's order) within ``marginal_tol`` of the reference; returns it."""
    ref = marginal_reference(x, shape, keep_axes)
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    t = int(np.prod(shape, dtype=np.int64)) // max(int(ref.size), 1)
    err = np.abs(got - ref)
    tol = marginal_tol(ref, t)
    print(f"marginal shape={tuple(shape)} keep={sorted(keep_axes)} t={t} max err/ref="
          f"{float(np.max(err / np.where(ref > 0, ref, 1.0))):.3e} bound={2.0 * t * 2.0 ** -53:.3e}")
    assert np.all(err <= tol), (float(err.max()), float(np.max(tol)))
    return ref
