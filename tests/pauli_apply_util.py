"""Reference and tolerance for a Pauli sum applied to the result tensor and for the energy gradients built on it
(tests/test_pauli_apply_host.py, tests/test_gpu_pauli_apply.py).

Reference: ``y = sum over s of c_s P_s x`` in complex128 / float64, string after string in the caller's order, ``P_s x``
by ``pauli_util.apply_string`` (``Y = [[0, -i], [i, 0]]``).

Tolerance per real component of ``y[j]``, derived and not tuned.  Both the reference and the device form ``y[j]`` from
the ``m`` real numbers ``+-c_s`` and the components of ``x[j ^ xm_s]``: the reference rounds every product ``c_s
component`` once and adds the terms one by one (at most ``m + 1`` roundings on any term); the device adds the ``+-c_s``
of a group first (at most ``m - 1`` roundings), multiplies once, combines the two products of a complex component once
and adds the groups (at most ``m + 2`` roundings on any term, first order).  Every term is bounded by ``|c_s| (|Re| +
|Im|)(x[j ^ xm_s])``, so

    |got - ref| <= 2 (m + 2) 2^-53 sum over s of |c_s| (|Re| + |Im|)(x[j ^ xm_s]) + u |ref|

with ``u`` the unit roundoff of the plan's components (``2^-24`` single, ``2^-53`` double): the one rounding of the
accumulator to the plan's dtype.

Gradients: CPU torch autograd through the per-op plug-in, as tests/vjp_util.py, applied to ``E = Re vdot(O, H O)`` built
from torch ops; torch's gradient of a real loss is ``dE / d Re x + i dE / d Im x``."""
import numpy as np

import pauli_util as pu


def pauli_apply_reference(x, shape, ops, coeffs):
    """``sum over s of coeffs[s] P_s x`` as a complex128 / float64 array of ``shape``."""
    shape = tuple(int(d) for d in shape)
    w = pu.widen(x).reshape(shape)
    rows = np.asarray(ops).reshape(-1, len(shape))
    y = np.zeros(shape, dtype=w.dtype)
    for row, c in zip(rows.tolist(), np.asarray(coeffs, dtype=np.float64).tolist()):
        t = pu.apply_string(w, shape, row)
        if w.dtype.kind != "c":
            assert sum(op == 2 for op in row) % 2 == 0, "P x of a real tensor with an odd number of Y is not real"
            t = np.real(t)
        y = y + c * t
    return y


def pauli_apply_tol(x, shape, ops, coeffs, dtype=None, ref=None):
    """The bound of the module docstring per real component: an array of ``shape``."""
    shape = tuple(int(d) for d in shape)
    w = pu.widen(x).reshape(shape)
    rows = np.asarray(ops).reshape(-1, len(shape))
    mag = np.abs(w.real) + (np.abs(w.imag) if w.dtype.kind == "c" else 0.0)
    tot = np.zeros(shape)
    for row, c in zip(rows.tolist(), np.asarray(coeffs, dtype=np.float64).tolist()):
        flip = [a for a, op in enumerate(row) if op in (1, 2)]
        tot += abs(c) * (np.flip(mag, axis=flip) if flip else mag)
    m = len(rows)
    single = np.dtype(dtype if dtype is not None else np.asarray(x).dtype).name in ("float32", "complex64")
    u = 2.0 ** -24 if single else 2.0 ** -53
    ref = pauli_apply_reference(x, shape, ops, coeffs) if ref is None else ref
    return 2.0 * (m + 2) * 2.0 ** -53 * tot + u * np.abs(ref)


def check_apply(got, x, shape, ops, coeffs):
    """Assert every real component of ``got`` within ``pauli_apply_tol`` of the reference; returns the reference."""
    shape = tuple(int(d) for d in shape)
    ref = pauli_apply_reference(x, shape, ops, coeffs)
    got = np.asarray(got)
    assert got.dtype == np.asarray(x).dtype and got.shape == shape, (got.dtype, got.shape, shape)
    tol = pauli_apply_tol(x, shape, ops, coeffs, ref=ref)
    g = pu.widen(got)
    err = np.maximum(np.abs((g - ref).real), np.abs((g - ref).imag)) if ref.dtype.kind == "c" else np.abs(g - ref)
    pos = tol > 0
    frac = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    print(f"apply shape={shape if len(shape) < 8 else (2, '...', len(shape))} strings={len(np.asarray(ops))} "
          f"dtype={got.dtype} max err/bound={frac:.3e}")
    assert np.all(err <= tol), (float(err.max()), int(np.argmax(err - tol)))
    return ref


def energy_numpy(out, ops, coeffs, normalize=False):
    """``Re vdot(O, H O)`` (divided by ``vdot(O, O)`` under ``normalize``) of the numpy result ``out``."""
    y = pauli_apply_reference(out, out.shape, ops, coeffs)
    e = float(np.real(np.vdot(pu.widen(out), y)))
    return e / float(np.real(np.vdot(out, out))) if normalize else e


def torch_apply(o, ops, coeffs):
    """``H o`` from torch ops (differentiable): sign vectors along Z / Y axes, flips along X / Y axes, ``i^ny``."""
    import torch

    total = torch.zeros_like(o)
    for row, c in zip(np.asarray(ops).reshape(-1, o.ndim).tolist(), np.asarray(coeffs, dtype=np.float64).tolist()):
        t, ny = o, 0
        for a, op in enumerate(row):
            if op in (2, 3):
                sign = torch.tensor([1.0, -1.0], dtype=torch.float64).reshape((1,) * a + (2,) + (1,) * (o.ndim - a - 1))
                t = t * sign
            if op in (1, 2):
                t = torch.flip(t, dims=(a,))
            ny += op == 2
        if ny:
            phase = (1.0, 1j, -1.0, -1j)[ny % 4]
            t = t * phase if o.is_complex() else t * float(np.real(phase))
        total = total + c * t
    return total


def reference_energy_grads(tree, arrays, ops, coeffs, normalize=False):
    """``(energy, [dE / d Re x_i + i dE / d Im x_i per leaf])`` by CPU torch autograd in complex128 / float64 through
    the per-op plug-in (zeros for a leaf the energy does not depend on)."""
    import torch

    xs = [torch.tensor(pu.widen(a)).requires_grad_(True) for a in arrays]
    cplx = any(x.is_complex() for x in xs)
    out = tree.contract([x.to(torch.complex128) if cplx else x for x in xs], implementation=(torch.einsum, torch.tensordot))
    out = out.reshape(tuple(tree.gathered_shape()))
    energy = torch.real(torch.sum(out.conj() * torch_apply(out, ops, coeffs)))
    if normalize:
        energy = energy / torch.real(torch.sum(out.conj() * out))
    grads = torch.autograd.grad(energy, xs, allow_unused=True)
    return float(energy.detach()), [np.zeros(a.shape, x.detach().numpy().dtype) if g is None else g.resolve_conj().numpy()
                                    for g, a, x in zip(grads, arrays, xs)]
