"""Reference sampler and the acceptance condition of one draw (tests/test_gpu_sample.py,
tests/test_sample_host.py).

The reference is numpy in float64: ``p = re^2 + im^2``, ``c = cumsum(p)``, target ``t = u c[-1]``.

Any order of summing n non-negative doubles is within (n - 1) 2^-53 sum(p) of the exact sum; the device and
numpy each commit one such error.  So with ``tol = 2 n 2^-53 c[-1]`` the index ``i`` the device returns for ``u``
must satisfy ``p[i] > 0`` and ``c[i-1] - tol <= t <= c[i] + tol`` (``c[-1] := 0``).  No draw is excluded.
"""
import numpy as np


def probabilities(x):
    """``|x|^2`` of every element in float64, as the library defines it: re*re + im*im."""
    x = np.asarray(x).reshape(-1)
    if np.iscomplexobj(x):
        re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
        return re * re + im * im
    x = x.astype(np.float64)
    return x * x


def reference(x, u):
    """``(p, c, t)``: probabilities, their cumulative sum and the targets of the uniforms ``u``."""
    p = probabilities(x)
    c = np.cumsum(p)
    return p, c, np.asarray(u, dtype=np.float64) * c[-1]


def default_tol(p, c):
    return 2.0 * p.size * 2.0 ** -53 * c[-1]


def reference_indices(c, t):
    return np.searchsorted(c, t, side="right")


def boundary_distance(c, t):
    """Distance of every target to the nearest CDF boundary (0 and every c[i])."""
    edges = np.concatenate(([0.0], c))
    j = np.clip(np.searchsorted(edges, t), 1, edges.size - 1)
    return np.minimum(np.abs(t - edges[j - 1]), np.abs(edges[j] - t))


def check_draws(x, u, idx, tol=None):
    """Assert the acceptance condition for every draw; returns ``(p, c, t)``."""
    p, c, t = reference(x, u)
    idx = np.asarray(idx)
    assert idx.shape == t.shape and idx.dtype == np.int64
    assert idx.min() >= 0 and idx.max() < p.size, (idx.min(), idx.max(), p.size)
    if tol is None:
        tol = default_tol(p, c)
    lower = np.where(idx > 0, c[np.maximum(idx - 1, 0)], 0.0)
    upper = c[idx]
    bad = ~((p[idx] > 0) & (lower - tol <= t) & (t <= upper + tol))
    assert not bad.any(), [
        (int(s), float(u[s]), int(idx[s]), float(p[idx[s]]), float(lower[s] - t[s]), float(t[s] - upper[s]), tol)
        for s in np.flatnonzero(bad)[:8]
    ]
    return p, c, t


def uniforms_257(seed):
    """257 uniforms that include 0.0 and the largest double below 1."""
    u = np.random.default_rng(seed).random(257)
    u[0] = 0.0
    u[-1] = np.nextafter(1.0, 0.0)
    return u
