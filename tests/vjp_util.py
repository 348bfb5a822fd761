"""Reference vector-Jacobian products for the gradient tests: torch autograd on the CPU through the
per-op plug-in ``implementation=(torch.einsum, torch.tensordot)``.

``G_i = conj(autograd.grad(O, x_i, grad_outputs=conj(h)))`` -- JAX's convention (no conjugation), the one
``compile_vjp`` and ``HipContractor.vjp`` compute."""
import numpy as np

from cotengra_amd.contractor import _chunk_index

MAX_ALL_SLICES = 64


def slice_ids_of(tree, case_ids=()):
    """All slices if there are at most 64, else the case's own list."""
    if tree.multiplicity <= MAX_ALL_SLICES:
        return None
    return [int(i) for i in case_ids]


def cotangent(tree, dtype, seed=7):
    rng = np.random.default_rng(seed)
    shape = tree.gathered_shape()
    h = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        h = h + 1j * rng.standard_normal(shape)
    return np.asarray(h, dtype=dtype)


def reference_vjp(tree, arrays, h, ids=None):
    """Gradients of every leaf (numpy, complex128 / float64): of the whole contraction, or of the sum of
    the slices ``ids`` (each slice's chunk of ``h`` as its cotangent)."""
    import torch

    impl = (torch.einsum, torch.tensordot)
    xs = [torch.tensor(np.asarray(a), requires_grad=True) for a in arrays]
    ht = torch.tensor(np.asarray(h))
    if ids is None:
        out = tree.contract(xs, implementation=impl)
        outs, hs = [out], [ht.reshape(out.shape)]
    else:
        outs, hs = [], []
        for i in ids:
            o = tree.contract_core(tree.slice_arrays(xs, i), implementation=impl)
            outs.append(o)
            hs.append(ht[_chunk_index(tree, tree.slice_key(i))].reshape(o.shape))
    grads = torch.autograd.grad(outs, xs, grad_outputs=[x.conj() for x in hs], allow_unused=True)
    return [np.zeros(a.shape, a.dtype) if g is None else g.conj().resolve_conj().numpy() for g, a in zip(grads, arrays)]


def split_grads(plan, flat, shapes):
    """The gradients of a VJP plan's flat result, one per leaf (None for leaves not in ``wrt``)."""
    flat = np.asarray(flat).reshape(-1)
    out = []
    for i, shape in enumerate(shapes):
        off = plan.grad_offsets.get(i)
        n = int(np.prod(shape, dtype=np.int64))
        out.append(None if off is None else flat[off:off + n].reshape(shape))
    return out
