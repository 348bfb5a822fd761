"""Reference and tolerance for dense local operators applied to the result tensor and for the energy gradients built
on them (tests/test_op_apply_host.py, tests/test_gpu_op_apply.py).

A request here is ``(axes, matrix)``: ``axes`` positions in the tensor's shape in the order the rows and columns of the
``(D, D)`` matrix run over them (row-major), not necessarily ascending.

Reference: ``y = sum over requests of (O (x) 1) x`` in complex128 / float64, request after request in the caller's
order, each by ``np.tensordot`` over the request's axes.

Tolerance per real component of ``y[j]``, derived and not tuned -- the reasoning of tests/pauli_apply_util.py.  Both the
reference and the device form ``y[j]`` from the same real products ``W component`` of the ``N = sum over t of D_t``
(entry, partner) pairs, ``W = O_t[a(j), b]`` and ``p = x[partner(j, b)]``: each product is rounded once, the two
products of a complex component are combined once and the terms are added one by one, in two associations (tensordot
sums a term first and adds the terms; the device keeps one accumulator; requests on one axis set are added as matrices
first on the way through the layers) -- at most ``N + 2`` roundings on any term on either side, first order.  Every term
is bounded by ``(|Re W| + |Im W|)(|Re p| + |Im p|)``, so

    |got - ref| <= 2 (N + 2) 2^-53 sum over t, b of (|Re W| + |Im W|)(|Re p| + |Im p|) + u |ref|

with ``u`` the unit roundoff of the plan's components (``2^-24`` single, ``2^-53`` double): the one rounding of the
accumulator to the plan's dtype.

Gradients: CPU torch autograd through the per-op plug-in, as tests/pauli_apply_util.py, applied to ``E = Re vdot(x, H
x)`` with ``H x`` from ``torch.tensordot``."""
import numpy as np

import pauli_util as pu


def _apply_one(w, axes, mat, xp=np):
    """``(O (x) 1) w`` for one request: contract the columns of ``O`` with ``axes`` of ``w``, put the rows back."""
    axes = [int(a) for a in axes]
    dims = tuple(w.shape[a] for a in axes)
    k = len(axes)
    o = mat.reshape(dims + dims)
    t = xp.tensordot(o, w, (list(range(k, 2 * k)), axes))     # rows first, then the other axes in order
    return xp.moveaxis(t, list(range(k)), axes) if xp is np else t.movedim(list(range(k)), axes)


def op_apply_reference(x, shape, requests):
    """``sum over requests of (O (x) 1) x`` as a complex128 / float64 array of ``shape``."""
    shape = tuple(int(d) for d in shape)
    w = pu.widen(x).reshape(shape)
    y = np.zeros(shape, dtype=w.dtype)
    for axes, mat in requests:
        mat = np.asarray(mat)
        if w.dtype.kind != "c":
            assert not np.iscomplexobj(mat) or not np.any(mat.imag), "O x of a real tensor with a complex O is not real"
            mat = np.real(mat)
        y = y + _apply_one(w, axes, np.asarray(mat, dtype=w.dtype))
    return y


def op_apply_tol(x, shape, requests, dtype=None, ref=None):
    """The bound of the module docstring per real component: an array of ``shape``."""
    shape = tuple(int(d) for d in shape)
    w = pu.widen(x).reshape(shape)
    mag = np.abs(w.real) + (np.abs(w.imag) if w.dtype.kind == "c" else 0.0)
    tot = np.zeros(shape)
    N = 0
    for axes, mat in requests:
        mat = np.asarray(mat, dtype=np.complex128)
        tot += _apply_one(mag, axes, np.abs(mat.real) + np.abs(mat.imag))
        N += mat.shape[0]
    single = np.dtype(dtype if dtype is not None else np.asarray(x).dtype).name in ("float32", "complex64")
    u = 2.0 ** -24 if single else 2.0 ** -53
    ref = op_apply_reference(x, shape, requests) if ref is None else ref
    return 2.0 * (N + 2) * 2.0 ** -53 * tot + u * np.abs(ref)


def check_op_apply(got, x, shape, requests):
    """Assert every real component of ``got`` within ``op_apply_tol`` of the reference; returns the reference."""
    shape = tuple(int(d) for d in shape)
    ref = op_apply_reference(x, shape, requests)
    got = np.asarray(got)
    assert got.dtype == np.asarray(x).dtype and got.shape == shape, (got.dtype, got.shape, shape)
    tol = op_apply_tol(x, shape, requests, ref=ref)
    g = pu.widen(got)
    err = np.maximum(np.abs((g - ref).real), np.abs((g - ref).imag)) if ref.dtype.kind == "c" else np.abs(g - ref)
    pos = tol > 0
    frac = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    print(f"op_apply shape={shape if len(shape) < 8 else (shape[0], '...', len(shape))} requests={len(requests)} "
          f"dtype={got.dtype} max err/bound={frac:.3e}")
    assert np.all(err <= tol), (float(err.max()), int(np.argmax(err - tol)))
    return ref


def bits_mirror(x, shape, terms, dtype):
    """The definition of the bits of csrc/ctg_op_apply.hip in numpy, element by element: a complex fp64 accumulator
    from +0, terms in order, ``b`` ascending, four products, the difference / sum and the addition each rounded once,
    one rounding to ``dtype`` at the end.  ``terms``: ascending axes.  For small tensors."""
    shape = tuple(int(d) for d in shape)
    cplx = np.dtype(dtype).kind == "c"
    w = pu.widen(np.asarray(x, dtype=dtype)).reshape(shape)
    acc_re, acc_im = np.zeros(shape), np.zeros(shape)
    for axes, mat in terms:
        axes = [int(a) for a in axes]
        dims = tuple(shape[a] for a in axes)
        D = int(np.prod(dims))
        mat = np.asarray(mat, dtype=np.complex128)
        rest = [a for a in range(len(shape)) if a not in axes]
        perm = axes + rest
        inv = np.argsort(perm)
        wt = w.transpose(perm).reshape(D, -1)             # [b, r]
        are = acc_re.transpose(perm).reshape(D, -1).copy()
        aim = acc_im.transpose(perm).reshape(D, -1).copy()
        for b in range(D):
            p = wt[b]
            for a in range(D):
                wre, wim = mat[a, b].real, mat[a, b].imag
                if cplx:
                    tr = wre * p.real - wim * p.imag
                    ti = wre * p.imag + wim * p.real
                    are[a] = are[a] + tr
                    aim[a] = aim[a] + ti
                else:
                    are[a] = are[a] + wre * p
        full = tuple(shape[a] for a in perm)
        acc_re = are.reshape(full).transpose(inv)
        acc_im = aim.reshape(full).transpose(inv)
    return (acc_re + 1j * acc_im).astype(dtype) if cplx else acc_re.astype(dtype)


def reference_energy_grads(tree, arrays, requests, normalize=False):
    """``(energy, [dE / d Re x_i + i dE / d Im x_i per leaf])`` by CPU torch autograd in complex128 / float64 through
    the per-op plug-in (zeros for a leaf the energy does not depend on); ``requests`` as ``(axes, matrix)`` over
    ``tree.gathered_shape()``."""
    import torch

    xs = [torch.tensor(pu.widen(a)).requires_grad_(True) for a in arrays]
    cplx = any(x.is_complex() for x in xs)
    out = tree.contract([x.to(torch.complex128) if cplx else x for x in xs], implementation=(torch.einsum, torch.tensordot))
    out = out.reshape(tuple(tree.gathered_shape()))
    hx = torch.zeros_like(out)
    for axes, mat in requests:
        m = torch.tensor(np.asarray(mat, dtype=np.complex128 if cplx else np.float64))
        hx = hx + _apply_one(out, axes, m, xp=torch)
    energy = torch.real(torch.sum(out.conj() * hx))
    if normalize:
        energy = energy / torch.real(torch.sum(out.conj() * out))
    grads = torch.autograd.grad(energy, xs, allow_unused=True)
    return float(energy.detach()), [np.zeros(a.shape, x.detach().numpy().dtype) if g is None else g.resolve_conj().numpy()
                                    for g, a, x in zip(grads, arrays, xs)]
