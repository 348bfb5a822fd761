"""Model and bounds of the cost statistics (tests/test_cost_host.py, tests/test_gpu_cost.py): the
distribution of a classical cost ``C(z)`` under ``p(z) = |x_z|^2``.

Everything the device reports as an integer or as the bits of the cost vector has an exact model here: the cost vector
(scatter, the butterflies of ``spectrum_util.spectrum_model`` over the bits in ascending order, ``+ 0.0``), the integer
weights ``w = rint(p 2^s)``, the weighted select with Python integers and ``fractions.Fraction``, the histogram.  The
fp64 sums have bounds, derived on paper and never from device output:

``moment_tol``: a moment or a tail is a fixed-order sum of at most ``n`` terms ``p C`` or ``(p C) C``; a term carries at
most 5 rounded operations for complex data (two squares and a sum for ``p``, two products) and 3 for real data; two
orders of summation are each within ``(n + ops) 2^-53 sum |terms|`` of the exact sum, hence ``|got - ref| <= 2 (n + 5)
2^-53 sum p |C|^k``, as ``spectrum_util.spectrum_tol`` is built.

``cvar_tol``: the device forms ``CVaR = (tail + (a - b) t) / a`` with ``a = A 2^-s`` and ``b = below 2^-s``; the reference
is ``(tail' + (a' - b') t) / a'`` with ``a' = alpha sum p`` and ``b' = sum of p below t`` from numpy's doubles and the
model's threshold ``t`` (CVaR is continuous in the level, so a threshold one class off where ``a'`` leaves ``[b', b' +
at']`` costs at most the mass discrepancy times ``2 max |C|``).  Every ``w 2^-s`` is within ``2^-(s + 1)`` of its ``p``,
``A`` within 1 of ``alpha W``, numpy's sums within ``n 2^-53 sum p``: ``da = alpha n 2^-(s + 1) + 2^-s + n 2^-53 sum p``,
``db = n 2^-(s + 1) + n 2^-53 sum p``, and with ``|CVaR| <= max |C|``

    |got - ref| <= (moment_tol + 4 (da + db) max |C|) / (alpha sum p).

Input condition: every test tensor is scaled so that numpy's ``sum p`` lies in ``[0.7, 0.8]`` (``scaled``); the exponent
of the device's sum -- another order of the same doubles -- cannot differ then, and ``s = 62``."""
import fractions
import math

import numpy as np

import spectrum_util as spu


def scaled(x, dtype, target=0.75):
    """``x`` scaled so that ``sum |x|^2`` is ``target``, as ``dtype``."""
    x = np.asarray(x)
    s = float(np.sum(np.abs(x.astype(np.complex128)) ** 2))
    return (x * math.sqrt(target / s)).astype(dtype)


def probabilities(x):
    """``p`` as ``SampleElem`` forms it: products and the sum in float64, each rounded once."""
    x = np.asarray(x).reshape(-1)
    if x.dtype.kind == "c":
        a, b = x.real.astype(np.float64), x.imag.astype(np.float64)
        return a * a + b * b
    a = x.astype(np.float64)
    return a * a


def term_masks(L, terms):
    """The flat-index masks of ``terms``, each a tuple of qubits over the shape ``(2,) * L`` (qubit ``q`` is axis ``q``: bit
    ``L - 1 - q``)."""
    return [sum(1 << (L - 1 - q) for q in t) for t in terms]


def term_ops(L, terms):
    """The ``(m, L)`` code rows (0 = I, 3 = Z) of ``terms``."""
    ops = np.zeros((len(terms), L), dtype=np.uint8)
    for r, t in enumerate(terms):
        for q in t:
            ops[r, q] = 3
    return ops


def cost_model(masks, coeffs, L):
    """The cost vector the device forms from ``(masks, coeffs)``, bit for bit: equal masks added in ascending term
    order, scatter, the butterflies over the bits 0 .. L - 1 ascending, ``+ 0.0``."""
    n = 1 << L
    merged = {}
    for m, c in zip(masks, np.asarray(coeffs, dtype=np.float64).tolist()):
        merged[int(m)] = merged[int(m)] + np.float64(c) if int(m) in merged else np.float64(c)
    v = np.zeros(n, dtype=np.float64)
    for m, c in merged.items():
        v[m] = c
    for b in range(L):
        t = v.reshape(-1, 2, 1 << b)
        v = np.stack([t[:, 0, :] + t[:, 1, :], t[:, 0, :] - t[:, 1, :]], axis=1).reshape(n)
    return np.ascontiguousarray(v + 0.0, dtype=np.float64)


def cost_direct(masks, coeffs, L):
    """``C(z) = sum_s c_s (-1)^popcount(z & m_s)`` term by term."""
    z = np.arange(1 << L, dtype=np.int64)
    out = np.zeros(1 << L, dtype=np.float64)
    for m, c in zip(masks, coeffs):
        out += float(c) * (1 - 2 * (spu.popcount(z & int(m)) % 2))
    return out


def weights(x):
    """``(S, s, w)``: numpy's ``sum p``, ``s = 62 - e`` for ``S = f 2^e``, and ``w = rint(p 2^s)`` as uint64."""
    p = probabilities(x)
    S = float(np.sum(p))
    if S == 0.0:
        return S, 0, np.zeros(p.shape, dtype=np.uint64)
    s = 62 - math.frexp(S)[1]
    return S, s, np.rint(np.ldexp(p, s)).astype(np.uint64)


def select_model(C, w, alpha, tail):
    """``dict(A, t, below, at)`` of one level, exact: a stable argsort by ``C`` (by ``-C`` for ``tail = +1``) and an
    integer cumulative sum."""
    C = np.asarray(C, dtype=np.float64).reshape(-1) + 0.0
    w = np.asarray(w, dtype=np.uint64).reshape(-1)
    W = int(w.sum(dtype=np.uint64))
    assert W < 2 ** 63
    A = math.ceil(fractions.Fraction(alpha) * W)
    if W == 0:
        return dict(A=0, t=0.0, below=0, at=0)
    order = np.argsort(-C if tail > 0 else C, kind="stable")
    cum = np.cumsum(w[order], dtype=np.uint64)
    t = float(C[order[int(np.searchsorted(cum, np.uint64(A), side="left"))]])
    inside = C > t if tail > 0 else C < t
    return dict(A=A, t=t, below=int(w[inside].sum(dtype=np.uint64)), at=int(w[C == t].sum(dtype=np.uint64)))


def hist_model(C, w, edges):
    """The ``len(edges) + 1`` integer masses: entry ``k`` holds the ``w`` of ``searchsorted(edges, C, "right") == k``."""
    C = np.asarray(C, dtype=np.float64).reshape(-1)
    out = np.zeros(len(edges) + 1, dtype=np.uint64)
    np.add.at(out, np.searchsorted(np.asarray(edges, dtype=np.float64), C, side="right"), np.asarray(w, dtype=np.uint64).reshape(-1))
    return out.astype(np.int64)


def moment_tol(x, C, k):
    """``2 (n + 5) 2^-53 sum p |C|^k``."""
    p = probabilities(x)
    C = np.abs(np.asarray(C, dtype=np.float64).reshape(-1))
    return 2.0 * (p.size + 5) * 2.0 ** -53 * float(np.sum(p * C ** k))


def cvar_reference(x, C, t, alpha, tail):
    """``(tail' + (alpha S - b') t) / (alpha S)`` from numpy's doubles and the threshold ``t``; also ``tail'``."""
    p = probabilities(x)
    C = np.asarray(C, dtype=np.float64).reshape(-1)
    inside = C > t if tail > 0 else C < t
    S = float(np.sum(p))
    tl = float(np.sum(p[inside] * C[inside]))
    return (tl + (alpha * S - float(np.sum(p[inside]))) * t) / (alpha * S), tl


def cvar_tol(x, C, s, alpha):
    """The bound of the module's docstring."""
    p = probabilities(x)
    n, S = p.size, float(np.sum(p))
    cmax = float(np.max(np.abs(C)))
    da = alpha * n * 2.0 ** -(s + 1) + 2.0 ** -s + n * 2.0 ** -53 * S
    db = n * 2.0 ** -(s + 1) + n * 2.0 ** -53 * S
    return (moment_tol(x, C, 1) + 4.0 * (da + db) * cmax) / (alpha * S)


def ring_terms(L):
    """The ring's MaxCut cost as ``(terms, coeffs)``: a constant and ``-1/2`` per edge ``(q, q + 1 mod L)``."""
    edges = [(q, (q + 1) % L) for q in range(L)] if L > 2 else [(0, 1)][: max(L - 1, 0)]
    return [()] + edges, [0.5 * len(edges)] + [-0.5] * len(edges)

