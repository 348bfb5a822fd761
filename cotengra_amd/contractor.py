"""The whole-tree HIP contractor and the execution drivers behind
``ContractionTree.contract / contract_core / contract_slice / gather_slices``.

The reference offers two plug-in points for execution:
per-op ``implementation=(einsum, tensordot)`` and the whole-tree backend
``CuQuantumContractor`` chosen in ``make_contractor``
(``cotengra/contract.py:840-1006``).  ``HipContractor`` fills the second slot
for MI355X: it is built once from a tree, lazily set up on the first call
(plan compilation + device residency), and then called with the arrays.

Arrays may be numpy arrays (copied host->device once per call) or torch
tensors already on a ROCm device (device-to-device copy into the executor's
input space, result returned as a torch tensor on the same device).
"""

from __future__ import annotations

import collections
import os
import time

import threading

import numpy as np

from . import runtime
from .plan import DTYPE_CODES, PICK_MAX, compile_tree
from .utils import prod

_SUPPORTED = tuple(DTYPE_CODES)

# Held from looking a pick contractor up on its tree until its call has returned, and while one is replaced or
# closed: no caller runs on a pick contractor that another thread has just closed.  (Taken before, never inside,
# a contractor's own lock.)
_PICK_LOCK = threading.RLock()


class _Progress:
    """Slice counter of a long sliced run: a ``tqdm`` bar when tqdm is importable (the
    reference's ``progbar``, contract.py:785-790 / core.py:4010-4013), plain lines on
    stderr otherwise.  ``progbar`` may also be a callable ``f(done, total)``."""

    def __init__(self, progbar, total, desc="slices"):
        self.total, self.done, self.bar, self.call = int(total), 0, None, None
        if callable(progbar):
            self.call = progbar
        elif progbar:
            try:
                from tqdm import tqdm

                self.bar = tqdm(total=self.total, desc=desc, unit="slice")
            except ImportError:
                self.bar = False

    @property
    def active(self):
        return self.call is not None or self.bar is not None

    def update(self, n):
        self.done += n
        if self.call is not None:
            self.call(self.done, self.total)
        elif self.bar:
            self.bar.update(n)
        elif self.bar is False:
            import sys

            print(f"  {self.done} / {self.total} slices", file=sys.stderr, flush=True)

    def close(self):
        if self.bar:
            self.bar.close()


def inputs_digest(arrays):
    """sha256 over the shapes, dtypes and bytes of the input tensors (a sliced Sycamore
    network: 195 KB): what makes a checkpoint belong to THESE inputs, not just this tree."""
    import hashlib

    h = hashlib.sha256()
    for x in arrays:
        if _is_torch(x):
            x = x.detach().cpu().numpy()
        x = np.ascontiguousarray(np.asarray(x))
        h.update(repr((x.shape, str(x.dtype))).encode())
        h.update(x.tobytes())
    return h.hexdigest()


def _current_device():
    """The process's current ROCm device (one process per GPU sets it with
    ``torch.cuda.set_device(LOCAL_RANK)``); 0 without torch."""
    try:
        import torch

        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except ImportError:
        pass
    return 0


def _release_execs(fn):
    """Close the idle executors of contractor ``fn``: not those another thread is inside
    of (its lock is held), nor those a suspended ``gen_output_chunks`` generator or a
    caller-visible state still uses (``pinned``).  True if anything was freed."""
    execs = getattr(fn, "_execs", None)
    lock = getattr(fn, "_lock", None)
    if not execs or lock is None or not lock.acquire(blocking=False):
        return False
    freed = False
    try:
        for key in [k for k, st in execs.items() if not st.get("pinned")]:
            st = execs.pop(key)
            st["exec"].close()
            st.pop("result", None)
            freed = True
    finally:
        lock.release()
    return freed


def _is_out_of_memory(exc):
    return isinstance(exc, MemoryError) or "out of memory" in str(exc).lower()


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _result_dtype(arrays):
    names = []
    for x in arrays:
        dt = str(x.dtype).replace("torch.", "")
        names.append(dt)
    dt = np.result_type(*[np.dtype(n) for n in names]).name
    if dt not in _SUPPORTED:
        # integers / half precision are promoted like numpy would for matmul
        dt = np.result_type(np.dtype(dt), np.float32).name
        if dt not in _SUPPORTED:
            raise TypeError(f"Unsupported array dtype {dt}.")
    return dt


def _device_copies(arrays, device, dtype):
    """Contiguous tensors of ``dtype`` on ``device`` whose memory holds the values: a conjugate or
    negative view keeps its bit through ``.to()`` / ``.contiguous()`` and would be read unconjugated."""
    import torch

    tdt = getattr(torch, dtype)
    keep = []
    for x in arrays:
        if not _is_torch(x):
            x = torch.as_tensor(np.asarray(x))
        keep.append(x.detach().to(device=device, dtype=tdt).resolve_conj().resolve_neg().contiguous())
    return keep


def _host_copies(arrays):
    return [x.detach().resolve_conj().resolve_neg().cpu().numpy() if _is_torch(x) else np.asarray(x)
            for x in arrays]


def _cast_like(g, x):
    """Gradient ``g`` in the dtype of input ``x``: the real part for a real leaf of a complex contraction,
    cast back for a promoted half-precision one."""
    if _is_torch(g):
        import torch

        dt = x.dtype if _is_torch(x) else getattr(torch, np.asarray(x).dtype.name)
        if g.is_complex() and not dt.is_complex:
            g = g.real
        return g.to(dt)
    dt = np.dtype(str(x.dtype).replace("torch.", "")) if _is_torch(x) else np.asarray(x).dtype
    if np.iscomplexobj(g) and dt.kind != "c":
        g = g.real
    return g.astype(dt)


def _wants_grad(arrays):
    """ROCm tensors, grad mode on and some input requiring grad: the autograd route."""
    if not any(_is_torch(x) for x in arrays):
        return False
    import torch

    return (torch.is_grad_enabled() and any(_is_torch(x) and x.is_cuda for x in arrays)
            and any(_is_torch(x) and x.requires_grad for x in arrays))


_ContractFunction = None


def _autograd_function():
    """The ``torch.autograd.Function`` of a whole-tree contraction (built on first use: torch is
    optional).  The forward is the executor's own path -- the same bits as without autograd; the
    backward is one VJP plan at the cotangent ``conj(grad_output)``, conjugated back (torch's
    convention), for the inputs autograd asks for."""
    global _ContractFunction
    if _ContractFunction is not None:
        return _ContractFunction
    import torch
    from torch.autograd.function import once_differentiable

    class ContractFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fn, progbar, check_zero, *arrays):
            ctx.fn = fn
            ctx.arrays = [x.detach() if _is_torch(x) else x for x in arrays]
            return fn._contract(ctx.arrays, progbar, check_zero, False)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            wrt = [i for i, need in enumerate(ctx.needs_input_grad[3:]) if need]
            grads = ctx.fn.vjp(*ctx.arrays, cotangent=grad_output.conj(), wrt=wrt)
            return (None, None, None) + tuple(None if g is None else g.conj().resolve_conj() for g in grads)

    _ContractFunction = ContractFunction
    return ContractFunction


_EnergyFunction = None


def _energy_function():
    """The ``torch.autograd.Function`` of ``HipContractor.energy_autograd`` (built on first use).  The forward is
    :meth:`HipContractor._energy_forward` -- the bits of the call without autograd -- and saves ``y``; the backward
    takes the real ``grad_output`` and runs one VJP plan at the cotangent ``grad_output conj(2 y)``."""
    global _EnergyFunction
    if _EnergyFunction is not None:
        return _EnergyFunction
    import torch
    from torch.autograd.function import once_differentiable

    class EnergyFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fn, ops, coeffs, normalize, box, *arrays):
            ctx.fn = fn
            ctx.arrays = [x.detach() if _is_torch(x) else x for x in arrays]
            energy, box["values"], box["norm"], ctx.y = fn._energy_forward(ctx.arrays, ops, coeffs, normalize)
            return torch.tensor(energy, dtype=torch.float64, device=ctx.y.device)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            wrt = tuple(i for i, need in enumerate(ctx.needs_input_grad[5:]) if need)
            grads = ctx.fn._energy_grads(ctx.arrays, ctx.y, wrt, scale=grad_output.real) if wrt else [None] * len(ctx.arrays)
            return (None,) * 5 + tuple(grads)

    _EnergyFunction = EnergyFunction
    return EnergyFunction


class ApplyResult(collections.namedtuple("ApplyResult", "y norm exponent")):
    """What ``HipContractor.apply_paulis`` returns: ``y = (sum over s of coeffs[s] P_s) x`` in the result's shape and
    dtype (numpy for numpy inputs, a tensor on the device for ROCm torch inputs); ``norm`` = ``sum |x|^2`` of the
    result ``x``; the base-10 ``exponent`` taken out under ``strip_exponent`` (0.0 otherwise: the true ``y`` is ``y
    10^exponent``)."""

    __slots__ = ()


class EnergyResult(collections.namedtuple("EnergyResult", "energy values norm grads")):
    """What ``HipContractor.energy`` returns: ``energy`` = ``sum over s of coeffs[s] values[s]`` (divided by ``norm``
    under ``normalize``; a 0-d float64 tensor with a ``grad_fn`` under torch autograd); ``values`` the float64 array
    of ``<x| P_s |x>`` per requested string, NOT normalised, the bits ``HipContractor.expectation`` returns (a 0-d
    float for a single request); ``norm`` = ``sum |x|^2``; ``grads`` one gradient of ``energy`` per leaf -- ``d / d Re
    x_i + i d / d Im x_i``, in the leaf's dtype and shape -- and ``None`` for a leaf outside ``wrt`` (``None``
    altogether under autograd, which carries them)."""

    __slots__ = ()


class SampleResult(collections.namedtuple(
        "SampleResult", "indices coords amplitudes p norm sum_p2 max_p argmax exponent")):
    """What ``HipContractor.sample`` returns: ``indices`` ``(n,)`` int64 flat row-major positions in the result
    (``tree.gathered_shape()``), ``coords`` ``(n, len(output))`` the same as one value per output index,
    ``amplitudes`` / ``p`` the elements drawn and their ``|x|^2`` (float64); and of the whole result ``norm`` =
    ``sum |x|^2``, ``sum_p2`` = ``sum |x|^4``, ``max_p`` with its lowest flat index ``argmax``, and the
    base-10 ``exponent`` taken out under ``strip_exponent`` (0.0 otherwise)."""

    __slots__ = ()


class TopKResult(collections.namedtuple("TopKResult", "indices coords amplitudes p norm sum_p2 exponent")):
    """What ``HipContractor.topk`` returns: the ``k`` most probable members of the result, ``p`` descending and the
    lower flat index first among equal ``p`` -- ``indices`` ``(k,)`` int64 flat row-major positions in the result
    (``tree.gathered_shape()``), ``coords`` ``(k, len(output))``, ``amplitudes`` and their ``p = |x|^2`` (float64);
    and of the whole result ``norm`` = ``sum |x|^2``, ``sum_p2`` = ``sum |x|^4`` and the base-10 ``exponent`` taken
    out under ``strip_exponent`` (0.0 otherwise)."""

    __slots__ = ()


class MarginalResult(collections.namedtuple("MarginalResult", "p norm exponent")):
    """What ``HipContractor.marginal`` returns: ``p`` the array of ``sum |x|^2`` over the output indices not kept,
    its axes in the order the caller named the labels (a list of such arrays for a list of requests); ``norm`` =
    ``sum |x|^2`` of the whole result; the base-10 ``exponent`` taken out under ``strip_exponent`` (0.0 otherwise:
    true values are ``p 10^(2 exponent)``)."""

    __slots__ = ()


class RdmResult(collections.namedtuple("RdmResult", "rho dims norm exponent")):
    """What ``HipContractor.rdm`` returns: ``rho`` the ``(D, D)`` reduced density matrix of the kept output indices
    (complex128, float64 for a real contraction), rows and columns row-major over the labels in the order the caller
    named them, exactly Hermitian and NOT normalised (a list of such matrices for a list of requests); ``dims`` the
    kept extents in that order (a list of tuples for a list of requests); ``norm`` = ``sum |x|^2`` of the whole
    result = ``trace(rho)`` up to rounding; the base-10 ``exponent`` taken out under ``strip_exponent`` (0.0
    otherwise: true values are ``rho 10^(2 exponent)``)."""

    __slots__ = ()


class RdmWideResult(collections.namedtuple("RdmWideResult", "rho dims purity norm exponent")):
    """What ``HipContractor.rdm_wide`` returns: ``rho`` the ``(D, D)`` reduced density matrix of the kept output
    indices, ``64 < D <= 4096``, as :class:`RdmResult` describes it, or ``None`` with ``matrix=False``; ``dims`` the
    kept extents in the caller's order; ``purity`` = ``sum |rho[a, b]|^2`` summed on the device, raw: divide by
    ``norm ** 2``; ``norm`` = ``sum |x|^2`` of the whole result; the base-10 ``exponent`` taken out under
    ``strip_exponent`` (0.0 otherwise: true values are ``rho 10^(2 exponent)``, ``purity 10^(4 exponent)``)."""

    __slots__ = ()


def _marginal_requests(tree, keep):
    """``keep`` of ``HipContractor.marginal`` as ``(several?, [(labels, keep flags per output axis, shape in the
    tensor's order, permutation to the caller's order), ...])`` -- host only; ``ValueError`` for a label that is
    not an output index of ``tree`` or that is named twice."""
    output = list(tree.output)
    shape = tuple(tree.gathered_shape())
    if isinstance(keep, (str, bytes)) or not hasattr(keep, "__iter__"):
        raise ValueError(f"keep = {keep!r}: give a sequence of output index labels, or a list of such sequences.")
    keep = list(keep)
    several = bool(keep) and all(isinstance(q, (list, tuple, set, frozenset)) for q in keep)
    reqs = []
    for labels in (keep if several else [keep]):
        labels = list(labels)
        for ix in labels:
            if ix not in output:
                raise ValueError(f"keep: {ix!r} is not an output index of the tree (output: {output}).")
        if len(set(labels)) != len(labels):
            raise ValueError(f"keep: {labels} repeats a label.")
        flags = [1 if ix in labels else 0 for ix in output]
        kept = [ix for ix in output if ix in labels]                 # (the tensor's own order)
        kshape = tuple(d for d, f in zip(shape, flags) if f)
        perm = tuple(kept.index(ix) for ix in labels)
        reqs.append((labels, flags, kshape, perm))
    return several, reqs


def pick_requests(tree, coords=None, indices=None):
    """The request table of ``HipContractor.pick`` as ``(M, len(tree.output))`` int64 coordinates, one column per
    output index in ``tree.output`` order -- host only.  Exactly one of ``coords`` (that table) and ``indices``
    (``(M,)`` flat row-major positions in ``tree.gathered_shape()``) is given.  ``ValueError`` for both or
    neither, a wrong width or dimension, a non-integer dtype, a value outside its extent, more than ``PICK_MAX``
    requests, and a tree whose output holds a sliced index."""
    if (coords is None) == (indices is None):
        raise ValueError("pick: give exactly one of coords and indices.")
    out_sliced = [ix for ix in tree.output if ix in tree.sliced_inds]
    if out_sliced:
        raise ValueError(f"pick: the output indices {out_sliced} of the tree are sliced (projected or not); "
                         "picking members of a sliced output is not supported -- slice inner indices only.")
    shape = tuple(int(d) for d in tree.gathered_shape())
    given = coords if coords is not None else indices
    if _is_torch(given):
        given = given.detach().cpu().numpy()
    given = np.asarray(given)
    if given.size and not np.issubdtype(given.dtype, np.integer):
        raise ValueError(f"pick: requests of dtype {given.dtype}; integers are expected.")
    if coords is not None:
        if given.ndim != 2 or given.shape[1] != len(shape):
            raise ValueError(f"pick: coords of shape {given.shape}; expected (M, {len(shape)}), one column per "
                             f"output index {list(tree.output)}.")
        req = np.ascontiguousarray(given, dtype=np.int64)
        for j, (ix, d) in enumerate(zip(tree.output, shape)):
            if len(req) and (req[:, j].min() < 0 or req[:, j].max() >= d):
                raise ValueError(f"pick: a coordinate of output index {ix!r} lies outside [0, {d}).")
    else:
        if given.ndim != 1:
            raise ValueError(f"pick: indices of shape {given.shape}; expected (M,).")
        n = prod(shape)
        flat = np.ascontiguousarray(given, dtype=np.int64)
        if len(flat) and (flat.min() < 0 or flat.max() >= n):
            raise ValueError(f"pick: an index lies outside [0, {n}), the elements of the result.")
        req = (np.stack(np.unravel_index(flat, shape), axis=1).astype(np.int64) if shape
               else np.zeros((len(flat), 0), dtype=np.int64))
    if len(req) > PICK_MAX:
        raise ValueError(f"pick: {len(req)} requests; at most {PICK_MAX} are taken by one call.")
    return req


_PAULI_CODE = {"I": 0, "X": 1, "Y": 2, "Z": 3}


def pauli_requests(tree, paulis, max_requests=None):
    """``paulis`` of ``HipContractor.expectation`` as ``(several?, ops)`` with ``ops`` a uint8 array of shape
    ``(m, len(tree.output))`` over ``tree.gathered_shape()``: 0, 1, 2, 3 = I, X, Y, Z per output index -- host only.
    A request is a ``str`` of ``len(tree.output)`` letters over ``IXYZ`` (any case), one per output index in
    ``tree.output`` order; a mapping ``{label: letter}``; or a sequence of ``(label, letter)`` pairs; labels not named
    are I.  ``paulis`` is one request or a list of requests.  ``ValueError`` for an unknown or repeated label, a letter
    outside ``IXYZ``, a string of the wrong length, a letter other than I on an output index whose extent is not 2 and
    more than ``max_requests`` (default ``Executor.PAULI_MAX_STRINGS``) requests."""
    import collections.abc as cabc

    if max_requests is None:
        max_requests = runtime.Executor.PAULI_MAX_STRINGS

    output = list(tree.output)
    shape = tuple(int(d) for d in tree.gathered_shape())
    rank = len(output)

    def is_pair(p):
        return isinstance(p, (tuple, list)) and len(p) == 2 and isinstance(p[1], str)

    def code(letter):
        if not isinstance(letter, str) or letter.upper() not in _PAULI_CODE:
            raise ValueError(f"paulis: {letter!r} is none of the letters I, X, Y, Z.")
        return _PAULI_CODE[letter.upper()]

    if isinstance(paulis, (str, cabc.Mapping)):
        several, reqs = False, [paulis]
    elif isinstance(paulis, (list, tuple)):
        if len(paulis) and all(is_pair(p) for p in paulis):
            several, reqs = False, [paulis]
        else:
            several, reqs = True, list(paulis)
    else:
        raise ValueError(f"paulis = {paulis!r}: give a string over IXYZ, a mapping {{label: letter}}, a sequence of "
                         "(label, letter) pairs, or a list of such requests.")
    if len(reqs) > max_requests:
        raise ValueError(f"paulis: {len(reqs)} requests; at most {max_requests} are taken by one call.")
    ops = np.zeros((len(reqs), rank), dtype=np.uint8)
    for r, req in enumerate(reqs):
        if isinstance(req, str):
            if len(req) != rank:
                raise ValueError(f"paulis: {req!r} has {len(req)} letters; one per output index {output} is expected.")
            pairs = list(zip(output, req))
        elif isinstance(req, cabc.Mapping):
            pairs = list(req.items())
        elif isinstance(req, (list, tuple)) and all(is_pair(p) for p in req):
            pairs = [tuple(p) for p in req]
        else:
            raise ValueError(f"paulis: the request {req!r} is no string, mapping or sequence of (label, letter) pairs.")
        seen = set()
        for ix, letter in pairs:
            if ix not in output:
                raise ValueError(f"paulis: {ix!r} is not an output index of the tree (output: {output}).")
            if ix in seen:
                raise ValueError(f"paulis: the label {ix!r} is named twice in one request.")
            seen.add(ix)
            a = output.index(ix)
            c = code(letter)
            if c and shape[a] != 2:
                raise ValueError(f"paulis: {letter!r} on output index {ix!r} of extent {shape[a]}; only an index of "
                                 "extent 2 carries X, Y or Z.")
            ops[r, a] = c
    return several, ops


def operator_requests(tree, operators):
    """``operators`` of ``HipContractor.apply_operators`` as ``(several?, canon, terms)`` -- host only.  A request is
    ``(labels, matrix)``: ``labels`` a sequence of distinct output index labels of any extent ``d_1 .. d_k`` (one
    label alone may be given bare), ``matrix`` of shape ``(D, D)`` with ``D = d_1 ... d_k`` or ``(d_1 .. d_k, d_1 ..
    d_k)``, rows and columns row-major over the labels in the order named.  ``operators`` is one request or a list of
    requests.  ``canon`` holds per request ``(axes, matrix)`` with ``axes`` the ascending positions of its labels in
    ``tree.output`` and ``matrix`` the complex128 ``(D, D)`` matrix permuted to that order; ``terms`` the same with
    the requests on one axis set summed (complex128, in the caller's order) into one term, in order of first
    appearance: what ``ctg_exec_result_op_apply`` takes, each axis set once.  ``ValueError`` for an unknown or
    repeated label, a label that is not an output index, no label, a matrix of another shape, an entry that is not
    finite, ``D`` above ``Executor.OP_MAX_DIM``, more than ``Executor.OP_MAX_TERMS`` terms and more than
    ``Executor.OP_MAX_ENTRIES`` matrix entries in all."""
    output = list(tree.output)
    shape = tuple(int(d) for d in tree.gathered_shape())

    def as_matrix(m):
        if _is_torch(m):
            m = m.detach().cpu().numpy()
        try:
            arr = np.asarray(m)
        except ValueError:
            return None
        return arr if arr.dtype.kind in "iufbc" and arr.ndim >= 2 else None

    def is_request(p):
        return isinstance(p, (tuple, list)) and len(p) == 2 and as_matrix(p[1]) is not None

    if is_request(operators):
        several, reqs = False, [operators]
    elif isinstance(operators, (list, tuple)):
        several, reqs = True, list(operators)
    else:
        raise ValueError(f"operators = {operators!r}: give a (labels, matrix) pair or a list of such pairs.")
    canon, merged = [], {}
    for req in reqs:
        if not is_request(req):
            raise ValueError(f"operators: the request {req!r} is no (labels, matrix) pair with a numeric matrix.")
        labels, mat = req[0], as_matrix(req[1])
        labels = [labels] if isinstance(labels, (str, bytes)) or not hasattr(labels, "__iter__") else list(labels)
        if not labels:
            raise ValueError("operators: a request names no label.")
        pos = []
        for ix in labels:
            if ix not in output:
                raise ValueError(f"operators: {ix!r} is not an output index of the tree (output: {output}).")
            if output.index(ix) in pos:
                raise ValueError(f"operators: the label {ix!r} is named twice in one request.")
            pos.append(output.index(ix))
        dims = tuple(shape[a] for a in pos)
        D = prod(dims)
        if D > runtime.Executor.OP_MAX_DIM:
            raise ValueError(f"operators: the extents {dims} of {labels} multiply to {D}; at most "
                             f"{runtime.Executor.OP_MAX_DIM} are taken by one request.")
        if mat.shape != (D, D) and mat.shape != dims + dims:
            raise ValueError(f"operators: a matrix of shape {mat.shape} on {labels}; ({D}, {D}) or {dims + dims} is expected.")
        mat = np.asarray(mat, dtype=np.complex128)
        if not np.all(np.isfinite(mat)):
            raise ValueError(f"operators: the matrix on {labels} has an entry that is not finite.")
        # rows and columns from the caller's order of the labels to ascending axis position
        k = len(pos)
        order = tuple(sorted(range(k), key=lambda i: pos[i]))
        mat = mat.reshape(dims + dims).transpose(order + tuple(k + i for i in order)).reshape(D, D)
        axes = tuple(pos[i] for i in order)
        mat = np.array(mat, order="C")
        canon.append((axes, mat))
        merged[axes] = merged[axes] + mat if axes in merged else mat.copy()
    if len(merged) > runtime.Executor.OP_MAX_TERMS:
        raise ValueError(f"operators: {len(merged)} distinct axis sets; at most {runtime.Executor.OP_MAX_TERMS} are taken by one call.")
    if sum(m.size for m in merged.values()) > runtime.Executor.OP_MAX_ENTRIES:
        raise ValueError(f"operators: more than {runtime.Executor.OP_MAX_ENTRIES} matrix entries in all.")
    return several, canon, list(merged.items())


_OperatorEnergyFunction = None


def _operator_energy_function():
    """The ``torch.autograd.Function`` of ``HipContractor.operator_energy_autograd`` (built on first use): the pattern
    of :func:`_energy_function` with :meth:`HipContractor._operator_energy_forward` as the forward."""
    global _OperatorEnergyFunction
    if _OperatorEnergyFunction is not None:
        return _OperatorEnergyFunction
    import torch
    from torch.autograd.function import once_differentiable

    class OperatorEnergyFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fn, canon, terms, normalize, box, *arrays):
            ctx.fn = fn
            ctx.arrays = [x.detach() if _is_torch(x) else x for x in arrays]
            energy, box["values"], box["norm"], ctx.y = fn._operator_energy_forward(ctx.arrays, canon, terms, normalize)
            return torch.tensor(energy, dtype=torch.float64, device=ctx.y.device)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            wrt = tuple(i for i, need in enumerate(ctx.needs_input_grad[5:]) if need)
            grads = ctx.fn._energy_grads(ctx.arrays, ctx.y, wrt, scale=grad_output.real) if wrt else [None] * len(ctx.arrays)
            return (None,) * 5 + tuple(grads)

    _OperatorEnergyFunction = OperatorEnergyFunction
    return OperatorEnergyFunction


class ExpectationResult(collections.namedtuple("ExpectationResult", "values norm exponent")):
    """What ``HipContractor.expectation`` returns: ``values`` the float64 array of ``<x| P |x> = sum over j of
    conj(x[j]) (P x)[j]`` per requested Pauli string, in the caller's order and NOT normalised (a 0-d float for a
    single request); ``norm`` = ``sum |x|^2`` of the whole result, the value of the all-identity string up to
    rounding; the base-10 ``exponent`` taken out under ``strip_exponent`` (0.0 otherwise: true values are ``values
    10^(2 exponent)``)."""

    __slots__ = ()


class SpectrumResult(collections.namedtuple("SpectrumResult", "values norm exponent")):
    """What ``HipContractor.pauli_spectrum`` returns: ``values`` the float64 values ``<x| P |x>``, NOT normalised --
    without ``paulis`` an array of ``tree.gathered_shape()`` over ALL strings of the X / Y pattern ``flips`` (entry
    ``b``: Y on the flipped axes where ``b`` is 1, X on the others, Z on the unflipped axes where ``b`` is 1; a tensor
    on the device for ROCm torch inputs), with ``paulis`` one value per request in the caller's order (a 0-d float
    for a single request); ``norm`` = ``sum |x|^2`` of the whole result; the base-10 ``exponent`` taken out under
    ``strip_exponent`` (0.0 otherwise: true values are ``values 10^(2 exponent)``)."""

    __slots__ = ()


class CostResult(collections.namedtuple(
        "CostResult", "mean variance minimum maximum argmin argmax support_min support_max p_min p_max thresholds cvar hist "
                      "values norm exponent raw")):
    """What ``HipContractor.cost`` returns for a classical cost ``C(z)`` under ``p(z) = |x_z|^2 / norm`` (DESIGN.md section
    22): ``mean`` and ``variance`` of ``C``; ``minimum`` / ``maximum`` of ``C`` over ALL bitstrings with ``argmin`` /
    ``argmax`` their coordinates in ``tree.gathered_shape()`` (the lowest flat index among ties); ``support_min`` /
    ``support_max`` the extremes over the bitstrings of non-zero weight and ``p_min`` / ``p_max`` the probability of
    sampling a bitstring of that cost; per level ``thresholds`` (the quantile ``t_l``) and ``cvar`` (float64 arrays in
    the order of ``levels``); ``hist`` the probability per bin ``edges[b] <= C < edges[b + 1]`` (``None`` without
    edges; the outer masses are in ``raw``); ``values`` the cost vector in ``tree.gathered_shape()`` with
    ``keep_values`` (a tensor on the device for ROCm torch inputs), else ``None``; ``norm`` = ``sum |x|^2``; the base-10
    ``exponent`` taken out under ``strip_exponent``.  ``raw``: a dict of the integers every mass comes from -- ``s``,
    ``W``, per level ``A``, ``below``, ``at`` and the fp64 ``tail``, ``argmin_flat`` / ``argmax_flat`` /
    ``support_argmin`` / ``support_argmax`` (flat indices; -1 without support), ``mass_min`` / ``mass_max``, ``hist``
    (``len(edges) + 1`` integers: below the first edge, the bins, at or above the last), ``sum_pc`` / ``sum_pcc``; a
    mass is its integer times ``2^-s``.  An all-zero result (``W = 0``): ``mean``, ``variance``, every probability,
    threshold and ``cvar`` are 0.0, ``support_min`` / ``support_max`` 0.0."""

    __slots__ = ()


def cost_requests(tree, terms, coeffs=None):
    """``terms`` and ``coeffs`` of ``HipContractor.cost`` as ``(ops, coeffs)`` -- host only: ``ops`` the uint8 ``(m,
    len(tree.output))`` array of codes 0 = I and 3 = Z of :func:`pauli_requests` (one request or a list of requests,
    up to ``Executor.COST_MAX_TERMS``), ``coeffs`` the float64 ``(m,)`` array (``None``: ones).  ``ValueError`` for what
    :func:`pauli_requests` refuses, a letter X or Y (no classical cost), an output index of extent above 2, ``coeffs``
    of another length and a coefficient that is not finite."""
    output = list(tree.output)
    for ix, d in zip(output, tree.gathered_shape()):
        if int(d) > 2:
            raise ValueError(f"cost: output index {ix!r} has extent {int(d)}; with terms every extent must be 1 or 2.")
    several, ops = pauli_requests(tree, terms, max_requests=runtime.Executor.COST_MAX_TERMS)
    if ((ops == 1) | (ops == 2)).any():
        r = int(np.flatnonzero(((ops == 1) | (ops == 2)).any(axis=1))[0])
        raise ValueError(f"cost: term {r} carries X or Y; a classical cost has I and Z only.")
    return ops, runtime.pauli_apply_coeffs(coeffs, len(ops))


def spectrum_requests(tree, flips, paulis=None):
    """``flips`` and ``paulis`` of ``HipContractor.pauli_spectrum`` as ``(flags, several?, select)`` -- host only:
    ``flags`` 0 / 1 per output index of ``tree.gathered_shape()``, ``select`` the flat indices of the requested
    strings in the spectrum (``None`` without ``paulis``).  ``ValueError`` for an output index of extent above 2, a
    label of ``flips`` that is unknown, repeated or of extent 1, what :func:`pauli_requests` refuses (up to
    ``Executor.PAULI_SPECTRUM_MAX_SELECT`` requests are taken) and a request whose X / Y letters are not exactly on
    ``flips``."""
    output = list(tree.output)
    shape = tuple(int(d) for d in tree.gathered_shape())
    for ix, d in zip(output, shape):
        if d > 2:
            raise ValueError(f"pauli_spectrum: output index {ix!r} has extent {d}; every extent must be 1 or 2.")
    flags = [0] * len(output)
    for ix in ([flips] if isinstance(flips, (str, bytes)) else list(flips)):
        if ix not in output:
            raise ValueError(f"flips: {ix!r} is not an output index of the tree (output: {output}).")
        a = output.index(ix)
        if flags[a]:
            raise ValueError(f"flips: the label {ix!r} is named twice.")
        if shape[a] != 2:
            raise ValueError(f"flips: output index {ix!r} has extent {shape[a]}; only an index of extent 2 carries X or Y.")
        flags[a] = 1
    if paulis is None:
        return flags, True, None
    several, ops = pauli_requests(tree, paulis, max_requests=runtime.Executor.PAULI_SPECTRUM_MAX_SELECT)
    flipped = (ops == 1) | (ops == 2)
    wrong = np.flatnonzero((flipped != np.asarray(flags, dtype=bool)[None, :]).any(axis=1))
    if wrong.size:
        raise ValueError(f"paulis: request {int(wrong[0])} does not have its X / Y letters exactly on flips = "
                         f"{[ix for ix, f in zip(output, flags) if f]}.")
    stride = np.ones(len(shape), dtype=np.int64)
    for a in range(len(shape) - 2, -1, -1):
        stride[a] = stride[a + 1] * shape[a + 1]
    select = (((ops == 2) | (ops == 3)).astype(np.int64) * stride[None, :]).sum(axis=1) if len(shape) else np.zeros(len(ops), np.int64)
    return flags, several, np.ascontiguousarray(select, dtype=np.int64)


def _cost_result(words, hist, nl, shape, values, exponent):
    """The :class:`CostResult` of the words and integer masses of ``Executor.cost_result``."""
    f = words.view(np.float64)
    s, W, norm = int(words[0]), int(words[1]), float(f[16])
    unit = 2.0 ** -s

    def coords(flat):
        return tuple(int(c) for c in np.unravel_index(flat, shape)) if shape and flat >= 0 else ()

    w0, wn = runtime.COST_LEVEL_WORD0, runtime.COST_LEVEL_WORDS
    A = [int(words[w0 + wn * l]) for l in range(nl)]
    t = np.array([f[w0 + wn * l + 1] for l in range(nl)], dtype=np.float64)
    below = [int(words[w0 + wn * l + 2]) for l in range(nl)]
    at = [int(words[w0 + wn * l + 3]) for l in range(nl)]
    tails = np.array([f[w0 + wn * l + 4] for l in range(nl)], dtype=np.float64)
    cvar = np.zeros(nl, dtype=np.float64)
    for l in range(nl):
        if A[l] > 0:
            cvar[l] = (tails[l] + ((A[l] - below[l]) * unit) * t[l]) / (A[l] * unit)
    live = W > 0 and norm > 0
    mean = float(f[2]) / norm if live else 0.0
    var = float(f[3]) / norm - mean * mean if live else 0.0
    raw = dict(s=s, W=W, A=A, below=below, at=at, tail=tails, argmin_flat=int(words[5]), argmax_flat=int(words[7]),
               support_argmin=int(words[9]), support_argmax=int(words[12]), mass_min=int(words[10]), mass_max=int(words[13]),
               hist=None if hist is None else hist.copy(), sum_pc=float(f[2]), sum_pcc=float(f[3]))
    prob = (lambda m: m * unit / norm) if live else (lambda m: 0.0)
    return CostResult(
        mean=mean, variance=var, minimum=float(f[4]), maximum=float(f[6]), argmin=coords(int(words[5])), argmax=coords(int(words[7])),
        support_min=float(f[8]), support_max=float(f[11]), p_min=prob(int(words[10])), p_max=prob(int(words[13])),
        thresholds=t, cvar=cvar, hist=None if hist is None else np.array([prob(int(m)) for m in hist[1:-1]], dtype=np.float64),
        values=values, norm=norm, exponent=exponent, raw=raw)


class HipContractor:
    """Callable performing the contraction of ``tree`` on an MI355X.

    Parameters
    ----------
    tree : ContractionTree
    order : str or callable, optional
        Traversal order (``ContractionTree.traverse``).
    strip_exponent, check_zero, progbar
        Defaults that a call may override, as for the reference's
        ``Contractor`` (contract.py:718-742).
    handle_slicing : bool
        True: calls take the *unsliced* arrays and return the full output
        (all slices run and are gathered on the device).  False: calls take
        arrays that were already sliced (``tree.contract_core`` semantics,
        core.py:3724-3773).
    device : int, optional
        GPU ordinal for numpy inputs (torch inputs bring their own device).
    """

    def __init__(
        self,
        tree,
        order=None,
        strip_exponent=False,
        check_zero=False,
        progbar=False,
        handle_slicing=True,
        device=None,
        force_kernel=None,
        fuse=None,
        fuse_min_elems=None,
        stem_bf16x3=None,
        crest_limit=None,
        pick=None,
        pick_chain=False,
    ):
        # a request table (``pick_requests``): the contractor computes those members of the output only, its
        # result is the ``(M,)`` vector of them (``HipContractor.pick`` builds and caches such contractors)
        self._pick = pick
        # ... with the requests carried down the tree as row-sparse intermediates (compile_tree(pick_chain=...))
        self._pick_chain = pick_chain
        # the pick contractor this one built last (``_pick_contractor``): closed with it
        self._picker = None
        self._origin = tree  # whose ``contraction_cores`` hold this contractor's siblings
        if handle_slicing or not tree.sliced_inds:
            self.tree = tree
        else:
            self.tree = _sliced_twin(tree)
        self.order = order
        self.strip_exponent = strip_exponent
        self.check_zero = check_zero
        self.progbar = progbar
        self.device = device
        self.force_kernel = force_kernel
        # fused stem pairs (plan.compile_tree): None = the default rule
        self.fuse = fuse
        self.fuse_min_elems = fuse_min_elems
        # arithmetic of the fused pairs: bf16 x 3 -- fp32 operands split exactly three ways, products on
        # the bf16 matrix cores -- unless switched off here (False) or by CTG_STEM_BF16X3=0
        # in the environment, which the kernel launcher reads at every launch and which wins
        # (round 6) a string names the arithmetic outright: "fp32", "bf16x3" (three exact limbs, six products) or
        # "fp16x2" (two limbs, three products: what an executor takes when nothing is said); True / False as
        # before: bf16 x 3 / fp32
        # "auto" (with crest_limit=L, required -- no threshold has been measured, so there is no default): every call
        # audits slice 0 in bf16 x 3 and takes fp16 x 2 only if every tensor it would scale per tensor has
        # crest_up <= L and no inf / NaN (rangeaudit.auto_choice); CTG_STEM_ARITH in the environment wins
        self.auto_arith = stem_bf16x3 == "auto"
        if self.auto_arith:
            if crest_limit is None:
                raise ValueError('stem_bf16x3="auto" needs crest_limit (there is no default: no threshold has been measured).')
            stem_bf16x3 = "bf16x3"
        elif crest_limit is not None:
            raise ValueError('crest_limit is the threshold of stem_bf16x3="auto" only.')
        self.crest_limit = None if crest_limit is None else float(crest_limit)
        self.last_audit = None
        self.arithmetic_chosen = None
        self.stem_arith = stem_bf16x3 if isinstance(stem_bf16x3, str) else None
        if isinstance(stem_bf16x3, str):
            stem_bf16x3 = stem_bf16x3 != "fp32"
        self.stem_bf16x3 = None if stem_bf16x3 is None else bool(stem_bf16x3)
        self._plans = {}  # dtype -> (Plan, DevicePlan)
        self._execs = {}  # (dtype, device, torch?) -> state dict
        # A ctg_exec is confined to one host thread at a time (include/ctg_hip.h); contractors
        # are cached on the tree and in the expression cache, and the reference's callers may
        # be multi-threaded (presets.py:77-88): upload -> run -> fetch is one critical section.
        self._lock = threading.RLock()
        # (executor state, strip_exponent) of the call made last if it left the whole contraction in the result
        # tensor (__call__, sample, topk, marginal, rdm, expectation), None after anything else: what reuse=True reads
        # (under _lock)
        self._reusable = None

    # ------------------------------------------------------------------ #

    def host_plan(self, dtype):
        """The compiled plan alone -- pure Python, no native library: what a caller needs that only asks how
        the slices are dealt to ranks (``Plan.rank_slice_ids``)."""
        try:
            return self._plans[dtype][0]
        except KeyError:
            pass
        try:
            return self._host_plans[dtype]
        except (KeyError, AttributeError):
            if not hasattr(self, "_host_plans"):
                self._host_plans = {}
            plan = self._host_plans[dtype] = compile_tree(
                self.tree, dtype, order=self.order, force_kernel=self.force_kernel,
                fuse=self.fuse, fuse_min_elems=self.fuse_min_elems, stem_bf16x3=self.stem_bf16x3,
                **({} if self._pick is None else {"pick": self._pick, "pick_chain": self._pick_chain}),
            )
            return plan

    def get_plan(self, dtype):
        try:
            return self._plans[dtype]
        except KeyError:
            plan = self.host_plan(dtype)
            entry = self._plans[dtype] = (plan, runtime.DevicePlan(plan))
            return entry

    def get_vjp_plan(self, dtype, wrt):
        """The VJP plan of the leaves ``wrt`` (a sorted tuple) and its device plan."""
        key = ("vjp", dtype, wrt)
        try:
            return self._plans[key]
        except KeyError:
            from .vjp import compile_vjp

            plan = compile_vjp(self.tree, dtype, wrt=wrt, order=self.order)
            entry = self._plans[key] = (plan, runtime.DevicePlan(plan))
            return entry

    def _get_exec(self, dtype, device, use_torch, wrt=None):
        key = (dtype, device, use_torch) if wrt is None else (dtype, device, use_torch, "vjp", wrt)
        try:
            return self._execs[key]
        except KeyError:
            pass
        plan, dplan = self.get_plan(dtype) if wrt is None else self.get_vjp_plan(dtype, wrt)
        try:
            st = self._new_exec(plan, dplan, dtype, device, use_torch, vjp=wrt is not None)
        except (MemoryError, RuntimeError) as exc:
            # Every cached contractor of a tree (``contract`` and ``contract_core``,
            # each dtype) keeps its own arena resident -- tens of GiB for a wide tree.
            # When the device is full, give up the siblings' executors (they are
            # rebuilt on demand) and try once more.
            if not _is_out_of_memory(exc):
                raise
            # (also the one-shot expressions the einsum / tensordot front ends keep)
            from .interface import evict_expression_cache

            freed = self._evict_siblings()
            freed = evict_expression_cache(keep=self) or freed
            if not freed:
                raise
            st = self._new_exec(plan, dplan, dtype, device, use_torch, vjp=wrt is not None)
        self._execs[key] = st
        return st

    def _evict_siblings(self):
        """Close the executors of the other contractors cached on the same tree
        (and this contractor's own executors for other dtypes / devices).
        Returns True if anything was freed."""
        freed = False
        cores = getattr(self._origin, "contraction_cores", {})
        for other in list(cores.values()) + [self]:
            freed = _release_execs(other) or freed
        if freed:
            try:
                import torch

                torch.cuda.empty_cache()  # result tensors went through torch's allocator
            except ImportError:
                pass
        return freed

    def _new_exec(self, plan, dplan, dtype, device, use_torch, vjp=False):
        st = {"plan": plan}
        if use_torch:
            import torch

            dev = torch.device("cuda", device)
            res = torch.zeros(
                plan.result_shape, dtype=getattr(torch, dtype), device=dev
            )
            stream = torch.cuda.current_stream(dev).cuda_stream
            st["result"] = res
            st["stream"] = stream
            st["exec"] = runtime.Executor(
                dplan, device=device, stream=stream, result_ptr=res.data_ptr()
            )
        else:
            st["exec"] = runtime.Executor(dplan, device=device)
        if self.auto_arith and (vjp or os.environ.get("CTG_STEM_ARITH")):
            # (the environment's arithmetic, which the executor took when it was created; a VJP executor: below)
            if vjp:
                st["exec"].set_stem_arithmetic("bf16x3")
        elif self.stem_arith is not None:
            st["exec"].set_stem_arithmetic(self.stem_arith)
        elif self.stem_bf16x3 is not None:
            st["exec"].set_stem_arithmetic(self.stem_bf16x3)
        elif vjp:
            # (a VJP executor is uploaded with a new cotangent on every call; fp16 x 2 keeps per-tensor
            # maxima across uploads, which could split a smaller cotangent under a stale scale)
            st["exec"].set_stem_arithmetic("bf16x3")
        return st

    def setup(self, *arrays):
        """Make ``arrays`` resident and return the executor state (the
        analogue of ``CuQuantumContractor.setup``, contract.py:883-899)."""
        self._reusable = None
        if len(arrays) != self.tree.N:
            raise ValueError(
                f"Expected {self.tree.N} arrays, got {len(arrays)}."
            )
        shapes = self.tree.get_shapes()
        for i, (x, s) in enumerate(zip(arrays, shapes)):
            if tuple(x.shape) != tuple(s):
                raise ValueError(
                    f"Array {i} has shape {tuple(x.shape)} but the tree "
                    f"expects {tuple(s)}."
                )
        dtype = _result_dtype(arrays)
        torch_in = [x for x in arrays if _is_torch(x) and x.is_cuda]
        if torch_in:
            import torch

            device = torch_in[0].device.index or 0
            st = self._get_exec(dtype, device, True)
            # the executor follows torch's *current* stream: uploads, kernels and the
            # caller's own tensor ops (input conversion, result clone) stay ordered
            cur = torch.cuda.current_stream(torch_in[0].device).cuda_stream
            if cur != st["stream"]:
                st["exec"].set_stream(cur)
                st["stream"] = cur
            keep = _device_copies(arrays, torch_in[0].device, dtype)
            st["exec"].upload_device(
                [t.data_ptr() for t in keep], [t.numel() for t in keep]
            )
            st["keep"] = keep
        else:
            device = self.device if self.device is not None else _current_device()
            st = self._get_exec(dtype, device, False)
            st["exec"].upload_host(_host_copies(arrays))
        return st

    # ---- gradients (cotengra_amd/vjp.py) ------------------------------------------------------------- #

    def _vjp_state(self, arrays, cotangent, wrt):
        """Upload ``arrays`` and ``cotangent`` to the VJP executor of ``wrt`` (cached in ``_execs`` with
        the mask in the key, so that the out-of-memory eviction covers it) and return its state."""
        tree = self.tree
        self._reusable = None
        if len(arrays) != tree.N:
            raise ValueError(f"Expected {tree.N} arrays, got {len(arrays)}.")
        for i, (x, s) in enumerate(zip(arrays, tree.get_shapes())):
            if tuple(x.shape) != tuple(s):
                raise ValueError(f"Array {i} has shape {tuple(x.shape)} but the tree expects {tuple(s)}.")
        gshape = tuple(tree.gathered_shape())
        if tuple(cotangent.shape) != gshape:
            raise ValueError(f"cotangent has shape {tuple(cotangent.shape)}, the result {gshape}.")
        everything = list(arrays) + [cotangent]
        dtype = _result_dtype(everything)
        torch_in = [x for x in everything if _is_torch(x) and x.is_cuda]
        if torch_in:
            import torch

            device = torch_in[0].device.index or 0
            st = self._get_exec(dtype, device, True, wrt=wrt)
            cur = torch.cuda.current_stream(torch_in[0].device).cuda_stream
            if cur != st["stream"]:
                st["exec"].set_stream(cur)
                st["stream"] = cur
            keep = _device_copies(everything, torch_in[0].device, dtype)
            st["exec"].upload_device([t.data_ptr() for t in keep], [t.numel() for t in keep])
            st["keep"] = keep
        else:
            device = self.device if self.device is not None else _current_device()
            st = self._get_exec(dtype, device, False, wrt=wrt)
            st["exec"].upload_host(_host_copies(everything))
        return st

    def vjp(self, *arrays, cotangent, wrt=None):
        """Vector-Jacobian product of the contraction: ``G_i = sum_o h[o] dO[o] / dx_i`` for ``h =
        cotangent`` (the result's shape), summed over all slices -- JAX's convention, nothing conjugated.
        Returns one gradient per leaf of ``wrt`` (default: all) and ``None`` for the others, each in its
        input's dtype (the real part for a real leaf of a complex contraction).  numpy in, numpy out;
        ROCm torch tensors in, tensors on that device out."""
        if self.strip_exponent:
            raise ValueError("vjp does not support strip_exponent.")
        N = self.tree.N
        wrt = tuple(range(N)) if wrt is None else tuple(sorted(set(int(i) for i in wrt)))
        if not wrt:
            return [None] * N
        if wrt[0] < 0 or wrt[-1] >= N:
            raise IndexError(f"wrt {wrt} outside the {N} leaves")
        with self._lock:
            st = self._vjp_state(arrays, cotangent, wrt)
            ex = st["exec"]
            ex.set_strip_exponent(False, False)
            ex.zero_result()
            self.run_share(ex, 0, 1, False)
            flat = st["result"].clone() if "result" in st else ex.download_result()
        plan = st["plan"]
        out = [None] * N
        for i in wrt:
            off, n = plan.grad_offsets[i], plan.input_sizes[i]
            out[i] = _cast_like(flat[off:off + n].reshape(tuple(arrays[i].shape)), arrays[i])
        return out

    def _finish(self, st, strip_exponent, check_zero, index=None):
        """Fetch the result; with ``strip_exponent`` return ``(mantissa,
        exponent)`` as accumulated on the device (reference contract.py:834-835
        and core.py:125-172)."""
        if "result" in st:
            out = st["result"]
            out = out[index] if index is not None else out
            out = out.clone()
        else:
            out = st["exec"].download_result()
            if index is not None:
                out = out[index]
            if out.ndim == 0 and not strip_exponent:
                return out[()]
        if not strip_exponent:
            return out
        exponent, zero = st["exec"].get_exponent()
        if zero and check_zero and exponent == float("-inf"):
            return 0.0, float("-inf")
        if not _is_torch(out) and out.ndim == 0:
            out = out[()]
        return out, exponent

    def run_slices(self, ex, first, count, stride, progbar=False):
        """``count`` slices ``first, first + stride, ...``; with ``progbar`` in chunks (a
        multiple of the executor's slice batch, sized for a few updates per second) with a
        synchronisation in between, so that the counter shows slices that are DONE."""
        prog = _Progress(progbar, count) if progbar and count > 1 else None
        plan = ex.plan
        ids = None
        if plan.group_size > 1 and count > 1:
            # slice groups: the slices asked for, group by group (what a group shares is computed once
            # per group among them) -- in one call, or in chunks of whole groups under a progress bar
            ids = np.arange(first, first + count * stride, stride, dtype=np.int64)
            ids = ids[np.lexsort((ids, plan.group_of(ids)))]
        if prog is None or not prog.active:
            if ids is None:
                ex.run_slices(first, count, stride)
            else:
                ex.run_slice_list(ids)
            return
        import time

        chunk = max(int(ex.batch), 1) if ids is None else int(plan.group_size)
        done = 0
        try:
            while done < count:
                n = min(chunk, count - done)
                t0 = time.perf_counter()
                if ids is not None:
                    ex.run_slice_list(ids[done:done + n])
                else:
                    ex.run_slices(first + done * stride, n, stride)
                ex.sync()
                dt = time.perf_counter() - t0
                done += n
                prog.update(n)
                if dt < 0.1:   # tiny slices: fewer, larger chunks
                    chunk *= 2
        finally:
            prog.close()

    def run_share(self, ex, rank=0, world=1, progbar=False):
        """``rank``'s share of the slices (``Plan.share_units``: whole slice groups ``rank, rank + world,
        ...``; ``contract_mpi``'s round-robin, core.py:4070, for a plan without groups) through
        ``ctg_exec_run_share`` -- in one call, or under ``progbar`` in chunks of whole units with a
        synchronisation in between, so that the counter shows slices that are DONE."""
        units, gs = ex.plan.share_units(rank, world)
        prog = _Progress(progbar, units * gs) if progbar and units * gs > 1 else None
        if prog is None or not prog.active:
            ex.run_share(rank, world, 0, units)
            return
        import time

        chunk = max(int(ex.batch) // gs, 1)
        done = 0
        try:
            while done < units:
                n = min(chunk, units - done)
                t0 = time.perf_counter()
                ex.run_share(rank, world, done, n)
                ex.sync()
                dt = time.perf_counter() - t0
                done += n
                prog.update(n * gs)
                if dt < 0.1:   # tiny slices: fewer, larger chunks
                    chunk *= 2
        finally:
            prog.close()

    def __call__(self, *arrays, **kwargs):
        backend = kwargs.pop("backend", None)  # noqa: F841  (inferred from arrays)
        progbar = kwargs.pop("progbar", self.progbar)
        check_zero = kwargs.pop("check_zero", self.check_zero)
        strip_exponent = kwargs.pop("strip_exponent", self.strip_exponent)
        kwargs.pop("implementation", None)
        if kwargs:
            raise TypeError(f"Unknown keyword arguments: {kwargs}.")
        if not strip_exponent and _wants_grad(arrays):
            return _autograd_function().apply(self, progbar, check_zero, *arrays)
        return self._contract(arrays, progbar, check_zero, strip_exponent)

    # ---- range audit (csrc/ctg_range.hip, cotengra_amd/rangeaudit.py) ----------------------- #

    def _audit_resident(self, ex, slices):
        """Audit ``slices`` of the inputs resident in ``ex`` in its current arithmetic; the result is left zeroed."""
        from . import rangeaudit

        ex.set_strip_exponent(False, False)
        names = ex.step_kernels()
        audits = []
        try:
            for s in slices:
                ex.zero_result()
                audits.append(ex.range_audit(int(s)))
        finally:
            ex.zero_result()
        return rangeaudit.step_records(ex.plan, names, audits)

    def audit(self, *arrays, slices=(0,)):
        """Upload ``arrays``, run the slices ``slices`` step by step in the executor's current arithmetic and read
        every tensor on the way (``ctg_exec_range_audit``): one record per plan step -- the kernel name, a
        ``rangeaudit.RangeSummary`` of operands ``a``, ``b`` (``b2`` of a fused pair) and of the result ``c``
        (``None``: not materialised, e.g. a member of an LDS-resident subtree), ``scaled``: the operands that
        run under a per-tensor scale, and ``kappa = |A| |B| (|B2|) / |C|``.  Several slices: the worst value per
        field.  float32 / complex64 only.  The result tensor is left zeroed."""
        with self._lock:
            st = self.setup(*arrays)
            return self._audit_resident(st["exec"], tuple(slices))

    def _choose_arithmetic(self, ex):
        """``stem_bf16x3="auto"``: set the arithmetic of ``ex`` for the inputs resident in it."""
        if not self.auto_arith:
            return
        from . import rangeaudit

        if os.environ.get("CTG_STEM_ARITH"):
            self.arithmetic_chosen = "environment"
            return
        if ex.plan.dtype not in ("float32", "complex64"):
            # (double precision has no reduced arithmetic: nothing to choose)
            self.arithmetic_chosen = "bf16x3"
            return
        ex.set_stem_arithmetic("fp16x2")
        h2_names = ex.step_kernels()
        ex.set_stem_arithmetic("bf16x3")
        self.last_audit = self._audit_resident(ex, (0,))
        self.arithmetic_chosen = rangeaudit.auto_choice(h2_names, self.last_audit, self.crest_limit)
        ex.set_stem_arithmetic(self.arithmetic_chosen)

    def _contract(self, arrays, progbar, check_zero, strip_exponent):
        with self._lock:
            st = self.setup(*arrays)
            ex = st["exec"]
            self._choose_arithmetic(ex)
            ex.set_strip_exponent(strip_exponent, check_zero)
            ex.zero_result()
            self.run_share(ex, 0, 1, progbar)
            self._reusable = (st, bool(strip_exponent))
            return self._finish(st, strip_exponent, check_zero)

    def contract_slice(self, arrays, i, strip_exponent=False, check_zero=False):
        """Output of slice ``i`` only (sliced output indices removed)."""
        with self._lock:
            st = self.setup(*arrays)
            ex = st["exec"]
            self._choose_arithmetic(ex)
            ex.set_strip_exponent(strip_exponent, check_zero)
            ex.zero_result()
            ex.run_slices(int(i), 1, 1)
            index = _chunk_index(self.tree, self.tree.slice_key(int(i)))
            return self._finish(st, strip_exponent, check_zero, index=index)

    def sample(self, *arrays, n_samples, seed=None, uniforms=None, strip_exponent=False, check_zero=False):
        """Contract (all slices, as a call does) and draw ``n_samples`` members of the result from
        ``p = |x|^2 / sum |x|^2`` on the device -- the result tensor is never copied to the host
        (``ctg_exec_sample_result``).  The draws are the inverse CDF at ``uniforms``
        (values in ``[0, 1)``; default ``np.random.default_rng(seed).random(n_samples)``): the same inputs and
        uniforms give the same draws.  Returns a :class:`SampleResult`.  With ``strip_exponent`` the amplitudes,
        ``p``, ``norm``, ``sum_p2`` and ``max_p`` are the mantissa's (true values: ``x 10^exponent``,
        ``10^(2 exponent)``, ``10^(2 exponent)``, ``10^(4 exponent)``, ``10^(2 exponent)``).  ``ValueError``
        when the result is all zero or not finite.  Not differentiable."""
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples = {n_samples} is negative.")
        if uniforms is None:
            u = np.random.default_rng(seed).random(n_samples)
        else:
            u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
            if u.size != n_samples:
                raise ValueError(f"{u.size} uniforms for n_samples = {n_samples}.")
        if not np.all((u >= 0.0) & (u < 1.0)):   # (also refuses NaN; the library checks again)
            raise ValueError("uniforms must lie in [0, 1).")
        with self._lock:
            st = self.setup(*arrays)
            ex = st["exec"]
            self._choose_arithmetic(ex)
            ex.set_strip_exponent(strip_exponent, check_zero)
            ex.zero_result()
            self.run_share(ex, 0, 1, False)
            if n_samples:
                idx, amps, p = ex.sample_result(u)
                norm, sum_p2, max_p, argmax = ex.sample_info()[:4]   # (of the passes the draws just ran)
            else:
                idx, amps, p = ex.sample_result(u)
                norm, sum_p2, max_p, argmax = ex.result_stats()
            exponent = ex.get_exponent()[0] if strip_exponent else 0.0
            self._reusable = (st, bool(strip_exponent))
        shape = tuple(self.tree.gathered_shape())
        coords = np.stack(np.unravel_index(idx, shape), axis=1).astype(np.int64) if shape else np.zeros((idx.size, 0), np.int64)
        return SampleResult(indices=idx, coords=coords, amplitudes=amps, p=p, norm=norm, sum_p2=sum_p2, max_p=max_p,
                            argmax=argmax, exponent=exponent)

    # ---- chosen members of the output: a sparse root step (csrc/ctg_pick.hip) -------------------- #

    def _pick_contractor(self, req, chain=False):
        """The contractor of the request table ``req``, cached on the tree under ``("hip-pick", order, sha1 of
        the int64 coords, chain)``; it replaces -- and closes -- the pick contractor cached before it (its tables cost
        24 bytes per request and plan on the device, and there is no reason to keep many).  Under ``_PICK_LOCK``,
        which the caller keeps until the call on the returned contractor is over.  The contractor lives until
        another table replaces it or the contractor that built it is closed."""
        import hashlib

        cores = self._origin.contraction_cores
        order = self.order if not callable(self.order) else id(self.order)
        chain = chain if chain is True else int(chain)   # (False and 0 are one key: no chain)
        # (True and 1 are equal as keys, and are different plans)
        key = ("hip-pick", order, hashlib.sha1(np.ascontiguousarray(req, dtype=np.int64).tobytes()).hexdigest(),
               "all" if chain is True else chain)
        fn = cores.get(key)
        if fn is not None and fn.tree is self.tree:
            return fn
        for k in [k for k in cores if isinstance(k, tuple) and k and k[0] == "hip-pick"]:
            cores.pop(k).close()
        arith = "auto" if self.auto_arith else (self.stem_arith if self.stem_arith is not None else self.stem_bf16x3)
        fn = cores[key] = HipContractor(
            self.tree, order=self.order, handle_slicing=True, device=self.device, force_kernel=self.force_kernel,
            fuse=self.fuse, fuse_min_elems=self.fuse_min_elems, stem_bf16x3=arith, crest_limit=self.crest_limit,
            pick=req, pick_chain=chain,
        )
        self._picker = fn
        return fn

    def pick(self, *arrays, coords=None, indices=None, strip_exponent=False, check_zero=False, chain=False):
        """Contract (all slices, as a call does) only the requested members of the output: ``coords``, ``(M,
        len(tree.output))`` integers, one column per output index in ``tree.output`` order, or ``indices``,
        ``(M,)`` flat row-major positions in ``tree.gathered_shape()`` -- the two forms ``SampleResult`` and
        ``TopKResult`` carry.  Duplicates are allowed, the order is kept.  Everything below the root of the tree
        runs as usual; the root is one sparse step whose cost follows ``M``, and the full output tensor never
        exists (``compile_tree(pick=...)``).  Returns the ``(M,)`` array of amplitudes in
        the result dtype (a torch tensor for ROCm torch inputs); with ``strip_exponent`` ``(mantissa,
        exponent)`` as a call does.  ``M = 0``: an empty array, the device is not touched.  ``ValueError`` --
        before the device is touched -- for what :func:`pick_requests` refuses.  The result tensor of this
        contractor is not touched, but ``reuse=True`` of :meth:`topk` / :meth:`marginal` / :meth:`rdm` / :meth:`expectation` refuses to read it after
        a pick.  Not differentiable.

        ``chain`` (``True``, or an ``int``: at most that many levels below the root): the requests are carried
        down the tree -- a node below the root whose output legs the table addresses at few distinct projections
        (``plan.pick_chain_nodes``: ``PICK_CHAIN_GAIN * M_c <= O_c``, its parent sparse too) is stored as ``M_c`` rows
        of its other legs and computed by one row-sparse step, so cost and memory follow the
        table, not ``2^k``.  Which nodes are sparse depends on the table through that rule: a request's bits are
        therefore independent of the table's order and of duplicates, but not of which other requests are present."""
        req = pick_requests(self.tree, coords, indices)
        with self._lock:
            self._reusable = None
        if len(req) == 0:
            dtype = _result_dtype(arrays) if arrays else "complex64"
            torch_in = [x for x in arrays if _is_torch(x) and x.is_cuda]
            if torch_in:
                import torch

                out = torch.zeros((0,), dtype=getattr(torch, dtype), device=torch_in[0].device)
            else:
                out = np.zeros((0,), dtype=dtype)
            return (out, float("-inf")) if strip_exponent else out
        with _PICK_LOCK:
            fn = self._pick_contractor(req, chain)
            return fn._contract(arrays, False, check_zero, strip_exponent)

    # ---- top-k, marginals, reduced density matrices and Pauli expectation values of the result on the device (DESIGN
    # 12, 15, 16) -------- #

    def _reduce_state(self, arrays, strip_exponent, check_zero, reuse):
        """Under the lock: the executor state whose result tensor holds the whole contraction, and whether it was
        run under ``strip_exponent`` -- contracted now from ``arrays``, or (``reuse``) left by the call before."""
        if reuse:
            if self._reusable is None:
                raise RuntimeError("reuse=True: the call made last on this contractor left no result to read "
                                   "(none was made, or another call -- audit, vjp, contract_slice, ... -- came between).")
            st, strip = self._reusable
            if not getattr(st["exec"], "handle", None):
                self._reusable = None
                raise RuntimeError("reuse=True: the executor that held the result has been released.")
            return st, strip
        st = self.setup(*arrays)
        ex = st["exec"]
        self._choose_arithmetic(ex)
        ex.set_strip_exponent(strip_exponent, check_zero)
        ex.zero_result()
        self.run_share(ex, 0, 1, False)
        self._reusable = (st, bool(strip_exponent))
        return st, bool(strip_exponent)

    def topk(self, *arrays, k, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return the ``k`` most probable members of the result --
        ``p = |x|^2`` descending, the lower flat index first among equal ``p``, exactly numpy's
        ``lexsort((index, -p))[:k]`` -- selected on the device; the result tensor is never copied to the host
        (``ctg_exec_result_topk``).  Returns a :class:`TopKResult`.  With
        ``strip_exponent`` the amplitudes, ``p``, ``norm`` and ``sum_p2`` are the mantissa's.  ``reuse=True``
        (no arrays): read the result tensor left by the call made directly before on this contractor
        (``__call__``, ``sample``, ``topk``, ``marginal``, ``rdm`` or ``expectation``; its ``strip_exponent`` applies) instead of
        contracting again; ``RuntimeError`` when there is none or another call came between.  ``ValueError`` for
        ``k < 1`` or above the number of elements or 2^20, and when the result holds a NaN or inf.  An all-zero
        result is no error.  Not differentiable."""
        k = runtime.check_topk_k(k)
        n = prod(self.tree.gathered_shape())
        if k > n or k > runtime.Executor.TOPK_MAX:
            raise ValueError(f"k = {k}: the result has {n} elements and at most {runtime.Executor.TOPK_MAX} are returned.")
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            idx, amps, p = ex.topk_result(k)
            norm, sum_p2 = ex.sample_info()[:2]   # (of the statistics passes the call just ran)
            exponent = ex.get_exponent()[0] if strip else 0.0
        shape = tuple(self.tree.gathered_shape())
        coords = np.stack(np.unravel_index(idx, shape), axis=1).astype(np.int64) if shape else np.zeros((idx.size, 0), np.int64)
        return TopKResult(indices=idx, coords=coords, amplitudes=amps, p=p, norm=norm, sum_p2=sum_p2, exponent=exponent)

    def marginal(self, *arrays, keep, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return the marginal of ``p = |x|^2`` over the output indices
        ``keep`` -- ``p`` summed over every other output index, in double with a fixed order, on the device
        (``ctg_exec_result_marginal``).  ``keep``: a sequence of output index labels, or
        a list of such sequences (several marginals of one contraction; ``p`` is a list then).  The axes of an
        array are in the order the labels were named; an output index projected onto one value keeps its size-1
        axis; no label: a 0-d array, ``sum p``.  Returns a :class:`MarginalResult`.  ``ValueError`` -- before the
        device is touched -- for a label that is unknown, not an output index, or repeated.  ``reuse=True``: as
        for :meth:`topk`.  Not differentiable."""
        several, reqs = _marginal_requests(self.tree, keep)
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        shape = tuple(self.tree.gathered_shape())
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            outs = []
            for labels, flags, kshape, perm in reqs:
                flat = ex.marginal_result(shape, flags)
                outs.append(np.array(flat.reshape(kshape).transpose(perm), order="C"))   # (0-d for no label)
            norm = ex.sample_info()[0]
            exponent = ex.get_exponent()[0] if strip else 0.0
        return MarginalResult(p=outs if several else outs[0], norm=norm, exponent=exponent)

    def rdm(self, *arrays, keep, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return the reduced density matrix of the output indices
        ``keep`` -- ``rho[a, b] = sum over r of x[a, r] conj(x[b, r])``, ``r`` over every other output index, every
        product and sum in double with a fixed order, on the device (``ctg_exec_result_rdm``, DESIGN.md section
        15).  ``keep``: as for :meth:`marginal` -- a sequence of output index labels, or a list of such sequences
        (several matrices of one contraction; ``rho`` and ``dims`` are lists then).  Rows and columns are row-major
        over the labels in the order they were named; no label: the ``(1, 1)`` matrix ``sum p``.  Returns an
        :class:`RdmResult`.  ``ValueError`` -- before the device is touched -- for a label that is unknown, not an
        output index, or repeated, and for kept extents whose product exceeds 64.  ``reuse=True``: as for
        :meth:`topk`.  Not differentiable."""
        several, reqs = _marginal_requests(self.tree, keep)
        shape = tuple(self.tree.gathered_shape())
        for labels, flags, kshape, perm in reqs:
            runtime.rdm_dim(shape, flags)
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            rhos, dims = [], []
            for labels, flags, kshape, perm in reqs:
                rho = ex.rdm_result(shape, flags)
                d = rho.shape[0]
                # rows and columns from the tensor's order of the kept axes to the caller's
                rho = rho.reshape(kshape + kshape).transpose(perm + tuple(len(perm) + p for p in perm))
                rhos.append(np.array(rho.reshape(d, d), order="C"))
                dims.append(tuple(kshape[p] for p in perm))
            norm = ex.sample_info()[0]
            exponent = ex.get_exponent()[0] if strip else 0.0
        return RdmResult(rho=rhos if several else rhos[0], dims=dims if several else dims[0], norm=norm, exponent=exponent)

    def rdm_wide(self, *arrays, keep, matrix=True, strip_exponent=False, check_zero=False, reuse=False):
        """:meth:`rdm` for kept extents whose product ``D`` is above 64 and at most 4096 -- the smaller side of a cut
        of the whole system -- tiled over the lower triangle on the device (``ctg_exec_result_rdm_wide``, DESIGN.md
        section 20).  ``keep``: ONE sequence of output index labels; a list of requests is a ``ValueError`` (a matrix
        of up to 256 MiB per request is not a batch).  Rows and columns are row-major over the labels in the order
        they were named.  ``matrix=False``: ``rho`` is ``None`` and only ``purity = sum |rho[a, b]|^2`` comes back
        from the device, the same bits as with the matrix.  Returns an :class:`RdmWideResult`.  ``ValueError`` --
        before the device is touched -- for what :meth:`rdm` refuses of the labels and for ``D`` outside ``65 ..
        4096`` (up to 64 it is :meth:`rdm`'s).  Leaves a result that ``reuse=True`` can read, and takes
        ``reuse=True`` as :meth:`topk` does.  Not differentiable."""
        several, reqs = _marginal_requests(self.tree, keep)
        if several:
            raise ValueError("rdm_wide: one request per call; a list of requests was given.")
        labels, flags, kshape, perm = reqs[0]
        shape = tuple(self.tree.gathered_shape())
        runtime.rdm_wide_dim(shape, flags)
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            rho, purity = ex.rdm_wide_result(shape, flags, matrix=matrix)
            if rho is not None:
                d = rho.shape[0]
                # rows and columns from the tensor's order of the kept axes to the caller's
                rho = rho.reshape(kshape + kshape).transpose(perm + tuple(len(perm) + p for p in perm))
                rho = np.array(rho.reshape(d, d), order="C")
            norm = ex.sample_info()[0]
            exponent = ex.get_exponent()[0] if strip else 0.0
        return RdmWideResult(rho=rho, dims=tuple(kshape[p] for p in perm), purity=purity, norm=norm, exponent=exponent)

    def expectation(self, *arrays, paulis, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return ``<x| P |x> = sum over j of conj(x[j]) (P x)[j]`` of the
        result for the Pauli strings ``paulis`` over the output indices -- every product and sum in double with a
        fixed order, on the device; the result tensor is never copied to the host (``ctg_exec_result_pauli``,
        DESIGN.md section 16).  ``paulis``: one request or a list of requests (:func:`pauli_requests`): a ``str`` of
        one letter over ``IXYZ`` per output index in ``tree.output`` order, a mapping ``{label: letter}`` or a
        sequence of ``(label, letter)`` pairs; labels not named are I.  Strings that share their X / Y positions
        share one read of the tensor (all Z-type terms of an Ising cost function, say); the bits of a value do not
        depend on the other strings of the call.  Values are NOT normalised: divide by ``norm``.  Returns an
        :class:`ExpectationResult`.  ``ValueError`` -- before the device is touched -- for what
        :func:`pauli_requests` refuses.  ``reuse=True``: as for :meth:`topk`.  Not differentiable."""
        several, ops = pauli_requests(self.tree, paulis)
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        shape = tuple(self.tree.gathered_shape())
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            values = ex.pauli_result(shape, ops)
            if len(values):
                norm = ex.sample_info()[0]   # (of the statistics passes the call just ran)
            else:
                norm = ex.result_stats()[0]
            exponent = ex.get_exponent()[0] if strip else 0.0
        return ExpectationResult(values=values if several else np.float64(values[0]), norm=norm, exponent=exponent)

    def pauli_spectrum(self, *arrays, flips=(), paulis=None, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return ``<x| P |x>`` for ALL Pauli strings that carry X or Y
        exactly on the output indices ``flips`` (labels; none: all Z-type strings) -- one Walsh-Hadamard transform on
        the device, ``2^L`` values for a few passes over the tensor where :meth:`expectation` takes one pass per 32
        strings (``ctg_exec_result_pauli_spectrum``).  Every output index must have extent 1 or
        2.  Without ``paulis``: ``values`` has ``tree.gathered_shape()``; entry ``b`` is the string with Y on the
        flipped indices where ``b`` is 1 and X where 0, Z on the other indices where ``b`` is 1; numpy for numpy
        inputs, a float64 tensor on the device for ROCm torch inputs.  With ``paulis`` (requests as for
        :meth:`expectation`, up to 2^24): ``values[s]`` is the value of request ``s`` in the caller's order -- the same
        quantity as :meth:`expectation`, in other bits; every request must have its X / Y exactly on ``flips``.
        Values are NOT normalised: divide by ``norm``.  Returns a :class:`SpectrumResult`.  ``ValueError`` -- before
        the device is touched -- for what :func:`spectrum_requests` refuses.  ``reuse=True``: as for :meth:`topk`.
        Not differentiable."""
        flags, several, select = spectrum_requests(self.tree, flips, paulis)
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        shape = tuple(int(d) for d in self.tree.gathered_shape())
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            if select is None and "result" in st:
                import torch

                values = torch.empty(shape, dtype=torch.float64, device=st["result"].device)
                ex.pauli_spectrum(shape, flags, dev_out=values.data_ptr())
            else:
                values = ex.pauli_spectrum(shape, flags, select=select)
            norm = ex.sample_info()[0]   # (of the statistics passes the call just ran)
            exponent = ex.get_exponent()[0] if strip else 0.0
        return SpectrumResult(values=values if several else np.float64(values[0]), norm=norm, exponent=exponent)

    # ---- the distribution of a classical cost over the result ------------------------------- #

    def cost(self, *arrays, terms=None, coeffs=None, values=None, levels=(), edges=None, tail="lower", keep_values=False,
             strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return the statistics of a classical cost ``C(z)`` under the
        output distribution ``p(z) = |x_z|^2 / norm`` -- mean, variance, ``CVaR_alpha`` and quantiles at ``levels``, a
        histogram over ``edges``, the optimum of ``C`` over all bitstrings and the probability of sampling it -- on the
        device; neither the tensor nor the cost vector crosses the bus (``ctg_exec_result_cost``).
        The cost is either ``terms`` with real ``coeffs`` (default: ones): Z-type requests as for :meth:`expectation`,
        ``C(z) = sum_s coeffs[s] (-1)^popcount(z & m_s)``, every output index of extent 1 or 2; or ``values``: an
        array of ``tree.gathered_shape()`` real numbers (numpy, or a ROCm torch tensor), any extents.  ``levels``: up
        to 8 numbers in (0, 1]; ``tail``: ``"lower"`` (minimisation: the best ``alpha`` mass is the lowest costs) or
        ``"upper"``; ``edges``: 2 .. 4097 ascending finite bin edges.  Every probability is a sum of integer weights
        ``rint(p 2^s)`` (exact, order-free); ``keep_values=True`` also returns the cost vector.  Returns a
        :class:`CostResult`.  ``ValueError`` -- before the device is touched -- for what :func:`cost_requests` refuses,
        both or neither source, ``values`` of another shape, complex or not finite (a device tensor's entries are checked
        on the device), a level outside (0, 1], more than 8 levels, edges that are not ascending and finite and a
        ``tail`` that is neither ``"lower"`` nor ``"upper"``.  ``reuse=True``: as for :meth:`topk`.  Not differentiable."""
        shape = tuple(int(d) for d in self.tree.gathered_shape())
        if (terms is None) == (values is None):
            raise ValueError("cost: give exactly one of terms and values.")
        if tail not in ("lower", "upper"):
            raise ValueError(f"cost: tail = {tail!r} is neither 'lower' nor 'upper'.")
        ops = co = None
        if terms is not None:
            ops, co = cost_requests(self.tree, terms, coeffs)
        else:
            if coeffs is not None:
                raise ValueError("cost: coeffs belong to terms, not to values.")
            if not _is_torch(values):
                values = np.asarray(values)
            if tuple(values.shape) != shape:
                raise ValueError(f"cost: values of shape {tuple(values.shape)}; the result has {shape}.")
            if not _is_torch(values):
                if values.dtype.kind not in "iufb":
                    raise ValueError(f"cost: values of dtype {values.dtype}; real numbers are expected.")
                values = np.ascontiguousarray(values, dtype=np.float64)
                if not np.all(np.isfinite(values)):
                    raise ValueError("cost: a value is not finite.")
            elif values.is_complex():
                raise ValueError(f"cost: values of dtype {values.dtype}; real numbers are expected.")
        lev = np.asarray(levels, dtype=np.float64).reshape(-1)
        if lev.size > runtime.Executor.COST_MAX_LEVELS:
            raise ValueError(f"cost: {lev.size} levels; at most {runtime.Executor.COST_MAX_LEVELS} are taken by one call.")
        if not np.all((lev > 0.0) & (lev <= 1.0)):
            raise ValueError(f"cost: the levels {lev.tolist()} are not all in (0, 1].")
        ed = None
        if edges is not None:
            ed = np.asarray(edges, dtype=np.float64).reshape(-1)
            if ed.size < 2 or ed.size > runtime.Executor.COST_MAX_EDGES:
                raise ValueError(f"cost: {ed.size} edges; between 2 and {runtime.Executor.COST_MAX_EDGES} are taken.")
            if not np.all(np.isfinite(ed)) or not np.all(ed[1:] > ed[:-1]):
                raise ValueError("cost: the edges are not finite and strictly ascending.")
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            dev_vals = out_vals = None
            if values is not None or keep_values:
                import torch

                dev = st["result"].device if "result" in st else torch.device("cuda", ex.device)
                if values is not None:
                    dev_vals = torch.as_tensor(values).to(device=dev, dtype=torch.float64).contiguous()
                if keep_values:
                    out_vals = torch.empty(shape, dtype=torch.float64, device=dev)
                torch.cuda.current_stream(dev).synchronize()
            words, hist = ex.cost_result(
                shape, ops=ops, coeffs=co, dev_cost=None if dev_vals is None else dev_vals.data_ptr(),
                tail=-1 if tail == "lower" else 1, levels=lev, edges=ed,
                dev_cost_out=None if out_vals is None else out_vals.data_ptr())
            exponent = ex.get_exponent()[0] if strip else 0.0
        if out_vals is not None and "result" not in st:
            out_vals = out_vals.cpu().numpy()
        return _cost_result(words, hist, lev.size, shape, out_vals, exponent)

    # ---- a Pauli sum applied to the result, energies and their gradients ------------------- #

    def apply_paulis(self, *arrays, paulis, coeffs=None, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return ``y = (sum over s of coeffs[s] P_s) x`` of the result
        ``x`` for the Pauli strings ``paulis`` over the output indices (:func:`pauli_requests`) and real ``coeffs``
        (default: ones) -- formed on the device next to ``x``, which is not written (``ctg_exec_result_pauli_apply``,
        DESIGN.md section 17).  ``y`` has the result's shape: numpy for numpy inputs, a tensor on the device for ROCm
        torch inputs.  Returns an :class:`ApplyResult`.  ``ValueError`` -- before the device is touched -- for what
        :func:`pauli_requests` refuses, ``coeffs`` of another length or not finite and, in a real contraction, a
        string with an odd number of Y.  ``reuse=True``: as for :meth:`topk`; the result stays reusable."""
        several, ops = pauli_requests(self.tree, paulis)
        c = runtime.pauli_apply_coeffs(coeffs, len(ops))
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        shape = tuple(int(d) for d in self.tree.gathered_shape())
        if arrays:
            runtime.pauli_apply_variant(_result_dtype(arrays), shape, ops)   # (odd Y in a real contraction)
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            y = self._apply_on(st, shape, ops, c)
            norm = ex.sample_info()[0] if len(ops) else ex.result_stats()[0]
            exponent = ex.get_exponent()[0] if strip else 0.0
        return ApplyResult(y=y, norm=norm, exponent=exponent)

    @staticmethod
    def _apply_on(st, shape, ops, coeffs):
        """``y`` of ``Executor.pauli_apply_result`` for the executor state ``st``: a tensor next to a torch-owned
        result (``dev_out``), numpy otherwise (``host_out``)."""
        ex = st["exec"]
        if "result" in st:
            import torch

            y = torch.empty(shape, dtype=st["result"].dtype, device=st["result"].device)
            ex.pauli_apply_result(shape, ops, coeffs, out_ptr=y.data_ptr())
            return y
        return ex.pauli_apply_result(shape, ops, coeffs)

    def _energy_forward(self, arrays, ops, coeffs, normalize):
        """One contraction, the values of the strings and ``y`` with ``dE = 2 Re <y| dx>``: ``(energy, values, norm,
        y)``; ``y`` has the result's shape and dtype (zeros when no string is left to apply)."""
        shape = tuple(int(d) for d in self.tree.gathered_shape())
        real = np.dtype(_result_dtype(arrays)).kind != "c"
        with self._lock:
            st, _ = self._reduce_state(arrays, False, False, False)
            ex = st["exec"]
            values = ex.pauli_result(shape, ops)
            norm = ex.sample_info()[0] if len(values) else ex.result_stats()[0]
            energy = 0.0
            for c, v in zip(coeffs.tolist(), values.tolist()):
                energy += c * v
            use, cs = ops, coeffs
            if real:
                # (a string with an odd number of Y: its value and its gradient are exactly zero)
                even = (ops == 2).sum(axis=1) % 2 == 0
                use, cs = ops[even], coeffs[even]
            if normalize:
                if not norm > 0:
                    raise ValueError("energy: normalize=True and the result has norm zero.")
                energy = energy / norm
                # d (E / N) = 2 Re <(H - (E / N) I) x / N | dx>
                # (the identity term goes into the first all-identity string, if there is one: never more than the
                # caller's strings plus one, which _energy_requests has checked)
                cs = cs / norm
                ident = np.flatnonzero(~use.any(axis=1))
                if ident.size:
                    cs[ident[0]] += -energy / norm
                else:
                    use = np.concatenate([use, np.zeros((1, ops.shape[1]), dtype=np.uint8)])
                    cs = np.concatenate([cs, [-energy / norm]])
            y = self._apply_on(st, shape, use, cs)
        return energy, values, norm, y

    def _energy_grads(self, arrays, y, wrt, scale=None):
        """The VJP run of :meth:`energy`: cotangent ``conj(2 y)`` (times the real ``scale``), gradients conjugated
        back (torch's convention for a real loss)."""
        if _is_torch(y):
            cot = (2.0 * y).conj().resolve_conj()
            if scale is not None:
                cot = cot * scale.to(device=cot.device, dtype=cot.real.dtype)
        else:
            cot = np.conj(2.0 * y)
        grads = self.vjp(*arrays, cotangent=cot, wrt=wrt)
        out = []
        for g in grads:
            if g is None:
                out.append(None)
            elif _is_torch(g):
                out.append(g.conj().resolve_conj() if g.is_complex() else g)
            else:
                out.append(np.conj(g) if np.iscomplexobj(g) else g)
        return out

    def _energy_requests(self, paulis, coeffs, normalize):
        """``(several?, ops, coeffs)`` of an energy request -- host only.  ``ValueError`` under ``strip_exponent``, for
        what :func:`pauli_requests` and ``runtime.pauli_apply_coeffs`` refuse, and for ``normalize`` with
        ``Executor.PAULI_MAX_STRINGS`` strings none of which is the identity: the apply call takes the identity term
        of ``(H - (E / N) I) / N`` in the first all-identity string, or as one string more."""
        if self.strip_exponent:
            raise ValueError("energy does not support strip_exponent.")
        several, ops = pauli_requests(self.tree, paulis)
        c = runtime.pauli_apply_coeffs(coeffs, len(ops))
        if normalize and len(ops) >= runtime.Executor.PAULI_MAX_STRINGS and ops.any(axis=1).all():
            raise ValueError(f"energy: normalize=True adds an identity string to the {len(ops)} requests, none of which "
                             f"is the identity; at most {runtime.Executor.PAULI_MAX_STRINGS} are taken by one call.")
        return several, ops, c

    def energy(self, *arrays, paulis, coeffs=None, wrt=None, normalize=False):
        """Energy and gradient in one step on the device: ``E = sum over s of coeffs[s] <x| P_s |x>`` of the result
        ``x`` and ``dE / d(every leaf)``.  One contraction; one ``ctg_exec_result_pauli`` call
        for ``values`` (the bits :meth:`expectation` returns); ``energy`` is their sum with ``coeffs`` (default:
        ones) in the caller's order on the host -- divided by ``norm`` under ``normalize``; one
        ``ctg_exec_result_pauli_apply`` call forms ``y = H x`` (``(H - (E / N) I) x / N`` under ``normalize``) in a
        device buffer; one VJP run with the cotangent ``conj(2 y)`` gives the gradients.  ``grads[i] = dE / d Re x_i +
        i dE / d Im x_i`` (torch's convention for a real loss; ``dE / d x_i`` for a real leaf), in leaf ``i``'s dtype
        and shape, ``None`` for a leaf outside ``wrt`` (default: all leaves).  In a real contraction a string with an
        odd number of Y has value and gradient exactly zero and is left out of the apply call.  Works on sliced and
        output-sliced trees.  Returns an :class:`EnergyResult`.  ``ValueError`` -- before the device is touched -- for
        what :func:`pauli_requests` refuses, ``coeffs`` of another length or not finite, under ``strip_exponent``,
        and for ``normalize`` with 4096 strings none of which is the identity (its identity term needs a string);
        ``IndexError`` for ``wrt`` outside the leaves; ``ValueError`` for ``normalize`` with norm zero."""
        several, ops, c = self._energy_requests(paulis, coeffs, normalize)
        N = self.tree.N
        wrt = tuple(range(N)) if wrt is None else tuple(sorted(set(int(i) for i in wrt)))
        if wrt and (wrt[0] < 0 or wrt[-1] >= N):
            raise IndexError(f"wrt {wrt} outside the {N} leaves")
        with self._lock:
            energy, values, norm, y = self._energy_forward(arrays, ops, c, normalize)
            grads = self._energy_grads(arrays, y, wrt) if wrt else [None] * N
        return EnergyResult(energy=energy, values=values if several else np.float64(values[0]), norm=norm, grads=grads)

    def energy_autograd(self, *arrays, paulis, coeffs=None, normalize=False):
        """:meth:`energy` under torch autograd: ``energy`` is a 0-d float64 tensor on the device with a ``grad_fn``
        (the same bits as without autograd) and ``grads`` is ``None``; the forward saves ``y``, the backward runs the
        one VJP plan for the inputs autograd asks for."""
        several, ops, c = self._energy_requests(paulis, coeffs, normalize)
        box = {}
        energy = _energy_function().apply(self, ops, c, bool(normalize), box, *arrays)
        values = box["values"]
        return EnergyResult(energy=energy, values=values if several else np.float64(values[0]), norm=box["norm"], grads=None)

    # ---- dense local operators on the result: apply, expectation, energy ------------------- #

    def apply_operators(self, *arrays, operators, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return ``y = (sum over requests of O (x) 1) x`` of the result
        ``x`` for the dense matrices ``operators`` on named output indices of any extent
        (:func:`operator_requests`) -- formed on the device next to ``x``, which is not written
        (``ctg_exec_result_op_apply``).  ``y`` has the result's shape: numpy for numpy inputs,
        a tensor on the device for ROCm torch inputs.  Returns an :class:`ApplyResult`.  ``ValueError`` -- before
        the device is touched -- for what :func:`operator_requests` refuses and, in a real contraction, a matrix
        with an imaginary part.  ``reuse=True``: as for :meth:`topk`; the result stays reusable."""
        several, canon, terms = operator_requests(self.tree, operators)
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        shape = tuple(int(d) for d in self.tree.gathered_shape())
        if arrays:
            runtime.op_apply_terms(_result_dtype(arrays), shape, terms)   # (a complex matrix in a real contraction)
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            y = self._op_apply_on(st, shape, terms)
            norm = ex.sample_info()[0] if terms else ex.result_stats()[0]
            exponent = ex.get_exponent()[0] if strip else 0.0
        return ApplyResult(y=y, norm=norm, exponent=exponent)

    @staticmethod
    def _op_apply_on(st, shape, terms):
        """``y`` of ``Executor.op_apply_result`` for the executor state ``st``: a tensor next to a torch-owned
        result (``dev_out``), numpy otherwise (``host_out``)."""
        ex = st["exec"]
        if "result" in st:
            import torch

            y = torch.empty(shape, dtype=st["result"].dtype, device=st["result"].device)
            ex.op_apply_result(shape, terms, out_ptr=y.data_ptr())
            return y
        return ex.op_apply_result(shape, terms)

    @staticmethod
    def _operator_values(ex, shape, canon):
        """``<x| O |x> = sum over a, b of O[a, b] rho[b, a]`` per request of ``canon``: one ``rdm_result`` per distinct
        axis set, the trace on the host row after row (a fixed order).  complex128, NOT normalised."""
        rhos, values = {}, np.zeros(len(canon), dtype=np.complex128)
        for r, (axes, mat) in enumerate(canon):
            if axes not in rhos:
                rhos[axes] = ex.rdm_result(shape, [1 if a in axes else 0 for a in range(len(shape))])
            rho = rhos[axes]
            v = 0.0 + 0.0j
            for a in range(mat.shape[0]):
                v += complex(np.dot(mat[a, :], rho[:, a]))
            values[r] = v
        return values

    def operator_expectation(self, *arrays, operators, strip_exponent=False, check_zero=False, reuse=False):
        """Contract (all slices, as a call does) and return ``<x| O |x>`` of the result for the dense matrices
        ``operators`` on named output indices of any extent (:func:`operator_requests`): ``sum over a, b of O[a, b]
        rho[b, a]`` with ``rho`` the exact fp64 reduced density matrix of the request's indices from the device
        (``ctg_exec_result_rdm``, one per distinct set of indices of the call) and the trace on the host in a fixed
        order; the result tensor is never copied to the host.  ``values`` is complex128 (real up to rounding for a
        Hermitian matrix), one per request, NOT normalised: divide by ``norm``.  Returns an
        :class:`ExpectationResult`.  ``ValueError`` -- before the device is touched -- for what
        :func:`operator_requests` refuses.  ``reuse=True``: as for :meth:`topk`.  Not differentiable."""
        several, canon, terms = operator_requests(self.tree, operators)
        if reuse and arrays:
            raise ValueError("reuse=True reads the result of the call before: give no arrays.")
        shape = tuple(int(d) for d in self.tree.gathered_shape())
        with self._lock:
            st, strip = self._reduce_state(arrays, strip_exponent, check_zero, reuse)
            ex = st["exec"]
            values = self._operator_values(ex, shape, canon)
            norm = ex.sample_info()[0] if len(values) else ex.result_stats()[0]
            exponent = ex.get_exponent()[0] if strip else 0.0
        return ExpectationResult(values=values if several else np.complex128(values[0]), norm=norm, exponent=exponent)

    def _operator_energy_requests(self, operators, normalize):
        """``(several?, canon, terms)`` of an operator-energy request, every matrix replaced by its Hermitian part
        -- host only.  ``ValueError`` under ``strip_exponent``, for what :func:`operator_requests` refuses, for a
        request that is not Hermitian (``max |O - O^H| > 1e-12 max |O|``) and for ``normalize`` when the identity
        term of ``(H - (E / N) 1) / N`` -- a one-axis term on axis 0 -- finds no room."""
        if self.strip_exponent:
            raise ValueError("operator_energy does not support strip_exponent.")
        several, canon, _ = operator_requests(self.tree, operators)
        herm, merged = [], {}
        for axes, mat in canon:
            dev = np.abs(mat - mat.conj().T).max()
            if dev > 1e-12 * np.abs(mat).max():
                raise ValueError(f"operator_energy: the matrix on the output axes {axes} is not Hermitian: max |O - O^H| = {dev:.3g}.")
            h = 0.5 * (mat + mat.conj().T)
            herm.append((axes, h))
            merged[axes] = merged[axes] + h if axes in merged else h.copy()
        if normalize and canon:
            shape = tuple(int(d) for d in self.tree.gathered_shape())
            if shape[0] > runtime.Executor.OP_MAX_DIM:
                raise ValueError(f"operator_energy: normalize=True puts its identity term on output axis 0, whose extent {shape[0]} "
                                 f"exceeds {runtime.Executor.OP_MAX_DIM}.")
            if (0,) not in merged and len(merged) >= runtime.Executor.OP_MAX_TERMS:
                raise ValueError(f"operator_energy: normalize=True adds a term to the {len(merged)} of the call; at most "
                                 f"{runtime.Executor.OP_MAX_TERMS} are taken.")
        return several, herm, list(merged.items())

    def _operator_energy_forward(self, arrays, canon, terms, normalize):
        """One contraction, the values of the requests and ``y`` with ``dE = 2 Re <y| dx>``: ``(energy, values, norm,
        y)``; ``y`` has the result's shape and dtype."""
        shape = tuple(int(d) for d in self.tree.gathered_shape())
        real = np.dtype(_result_dtype(arrays)).kind != "c"
        with self._lock:
            st, _ = self._reduce_state(arrays, False, False, False)
            ex = st["exec"]
            values = self._operator_values(ex, shape, canon)
            norm = ex.sample_info()[0] if len(values) else ex.result_stats()[0]
            energy = 0.0
            for v in values.tolist():
                energy += v.real
            use = [(axes, mat) for axes, mat in terms]
            if real:
                # (x^T O x of a real x sees the real symmetric part of a Hermitian O alone: so does the gradient)
                use = [(axes, np.array(mat.real, dtype=np.complex128)) for axes, mat in use]
            if normalize:
                if not norm > 0:
                    raise ValueError("operator_energy: normalize=True and the result has norm zero.")
                energy = energy / norm
                # d (E / N) = 2 Re <(H - (E / N) 1) x / N | dx>; the identity as a multiple of the unit matrix on axis 0
                use = [(axes, mat / norm) for axes, mat in use]
                if use:
                    ident = (-energy / norm) * np.eye(shape[0], dtype=np.complex128)
                    at = [i for i, (axes, _) in enumerate(use) if axes == (0,)]
                    if at:
                        use[at[0]] = ((0,), use[at[0]][1] + ident)
                    else:
                        use.append(((0,), ident))
            y = self._op_apply_on(st, shape, use)
        return energy, values, norm, y

    def operator_energy(self, *arrays, operators, wrt=None, normalize=False):
        """Energy and gradient in one step on the device for a Hamiltonian of dense local terms on output indices of
        any extent: ``E = sum over requests of Re <x| O |x>`` of the result ``x`` and ``dE / d(every leaf)``
        (DESIGN.md section 19).  One contraction; the values as :meth:`operator_expectation` forms them; ``energy``
        their real parts summed in the caller's order -- divided by ``norm`` under ``normalize``; one
        ``ctg_exec_result_op_apply`` call forms ``y = H x`` (``(H - (E / N) 1) x / N`` under ``normalize``, the
        identity folded into a one-axis term on axis 0) in a device buffer; one VJP run with the cotangent ``conj(2
        y)`` gives the gradients, as for :meth:`energy`.  Every request must be Hermitian (``max |O - O^H| <= 1e-12
        max |O|``); its Hermitian part is used.  Returns an :class:`EnergyResult` (``values`` complex128).
        ``ValueError`` -- before the device is touched -- for what :func:`operator_requests` refuses, a request that
        is not Hermitian and under ``strip_exponent``; ``IndexError`` for ``wrt`` outside the leaves; ``ValueError``
        for ``normalize`` with norm zero."""
        several, canon, terms = self._operator_energy_requests(operators, normalize)
        N = self.tree.N
        wrt = tuple(range(N)) if wrt is None else tuple(sorted(set(int(i) for i in wrt)))
        if wrt and (wrt[0] < 0 or wrt[-1] >= N):
            raise IndexError(f"wrt {wrt} outside the {N} leaves")
        with self._lock:
            energy, values, norm, y = self._operator_energy_forward(arrays, canon, terms, normalize)
            grads = self._energy_grads(arrays, y, wrt) if wrt else [None] * N
        return EnergyResult(energy=energy, values=values if several else np.complex128(values[0]), norm=norm, grads=grads)

    def operator_energy_autograd(self, *arrays, operators, normalize=False):
        """:meth:`operator_energy` under torch autograd: ``energy`` is a 0-d float64 tensor on the device with a
        ``grad_fn`` (the same bits as without autograd) and ``grads`` is ``None``; the forward saves ``y``, the
        backward runs the one VJP plan for the inputs autograd asks for."""
        several, canon, terms = self._operator_energy_requests(operators, normalize)
        box = {}
        energy = _operator_energy_function().apply(self, canon, terms, bool(normalize), box, *arrays)
        values = box["values"]
        return EnergyResult(energy=energy, values=values if several else np.complex128(values[0]), norm=box["norm"], grads=None)

    def profile(self, arrays, slice_id=0):
        """Per-step milliseconds for one slice (see ``Plan.describe_steps``)."""
        with self._lock:
            st = self.setup(*arrays)
            return st["plan"], st["exec"].profile_slice(slice_id)

    def close(self):
        with _PICK_LOCK:
            fn, self._picker = self._picker, None
            if fn is not None:
                cores = getattr(self._origin, "contraction_cores", None) or {}
                for k in [k for k, v in cores.items() if v is fn]:
                    del cores[k]
                fn.close()
        with self._lock:
            self._reusable = None
            for st in self._execs.values():
                st["exec"].close()
            self._execs.clear()
            for _, dplan in self._plans.values():
                dplan.close()
            self._plans.clear()


class PerOpContractor:
    """The reference's per-op plug-in point: ``implementation=(einsum,
    tensordot)`` (``cotengra/contract.py:775-776`` -- in that order).  The tree
    is walked on the host and every pairwise step is handed to the caller's two
    functions:

    * ``tensordot(a, b, (axes_a, axes_b))`` for steps that are plain tensor
      products over shared indices, the result being ``[free-a..., free-b...]``
      and then transposed to the parent's index order (contract.py:808-812);
    * ``einsum(eq, a, b)`` for steps with batch / hyper indices, and
      ``einsum(eq, x)`` for single-tensor preprocessing (contract.py:795-800, 814).

    Passing this package's own pair, ``(cotengra_amd.einsum,
    cotengra_amd.tensordot)``, runs every step as its own small HIP plan --
    correct but one materialised tensor per step, which is what the whole-tree
    ``HipContractor`` exists to avoid (SURVEY section 8b calls this slot the
    fallback boundary).  Arrays are whatever the two functions accept; the only
    things asked of the arrays themselves are ``.transpose(*perm)`` / ``.permute``
    and, with ``strip_exponent``, ``abs(x).max()`` and division by a scalar.
    """

    def __init__(self, tree, implementation, order=None, prefer_einsum=False,
                 strip_exponent=False, check_zero=False):
        try:
            self._einsum, self._tensordot = implementation
        except (TypeError, ValueError):
            raise ValueError(
                "implementation must be 'hip' or a pair of callables (einsum, tensordot), "
                f"got {implementation!r}."
            ) from None
        if not (callable(self._einsum) and callable(self._tensordot)):
            raise ValueError("implementation=(einsum, tensordot) must be two callables.")
        self.strip_exponent = strip_exponent
        self.check_zero = check_zero
        self.n_inputs = tree.N
        # schedule: ("pair", out, left, right, axes | None, eq | None, perm | None)
        self.schedule = []
        if tree.N == 1:
            self.single = tree.get_eq_sliced()
            return
        self.single = None
        slot = {leaf: i for i, leaf in enumerate(tree.gen_leaves())}
        nxt = len(slot)
        for parent, left, right in tree.traverse(order=order):
            a, b = slot.pop(left), slot.pop(right)
            slot[parent] = nxt
            if not prefer_einsum and tree.get_can_dot(parent):
                self.schedule.append(
                    (nxt, a, b, tree.get_tensordot_axes(parent), None, tree.get_tensordot_perm(parent))
                )
            else:
                self.schedule.append((nxt, a, b, None, tree.get_einsum_eq(parent), None))
            nxt += 1
        self.root = nxt - 1
        # (filled lazily by the index queries above, so read afterwards)
        self.pre = dict(tree.preprocessing)

    @staticmethod
    def _transpose(x, perm):
        if hasattr(x, "permute"):
            return x.permute(*perm)
        return x.transpose(*perm)

    def __call__(self, *arrays, **kwargs):
        kwargs.pop("backend", None)
        kwargs.pop("progbar", None)
        strip = kwargs.pop("strip_exponent", self.strip_exponent)
        check_zero = kwargs.pop("check_zero", self.check_zero)
        if kwargs:
            raise TypeError(f"Unknown keyword arguments: {kwargs}.")
        if len(arrays) != self.n_inputs:
            raise ValueError(f"Expected {self.n_inputs} arrays, got {len(arrays)}.")
        import math

        exponent = 0.0
        if self.single is not None:
            out = self._einsum(self.single, arrays[0])
            return (out, exponent) if strip else out
        live = dict(enumerate(arrays))
        for i, eq in self.pre.items():
            live[i] = self._einsum(eq, live[i])
        for out_id, a, b, axes, eq, perm in self.schedule:
            x, y = live.pop(a), live.pop(b)
            if axes is not None:
                z = self._tensordot(x, y, axes)
                if perm:
                    z = self._transpose(z, perm)
            else:
                z = self._einsum(eq, x, y)
            if strip:
                # contract.py:816-829
                fac = float(abs(z).max())
                if check_zero and fac == 0.0:
                    return 0.0, float("-inf")
                exponent += math.log10(fac)
                z = z / fac
            live[out_id] = z
        out = live[self.root]
        return (out, exponent) if strip else out


def _chunk_index(tree, loc):
    """Position of a slice's output inside the full result tensor: sliced
    output indices are fixed (a projected one sits at 0 of its size-1 axis),
    the others span their axis."""
    index = []
    for ix in tree.output:
        si = tree.sliced_inds.get(ix)
        if si is None:
            index.append(slice(None))
        else:
            index.append(0 if si.project is not None else loc[ix])
    return tuple(index)


def _sliced_twin(tree):
    """The same contraction schedule seen from inside one slice: sliced
    indices are removed from every term, nothing is sliced."""
    from .tree import ContractionTree

    twin = ContractionTree(
        tree.get_inputs_sliced(), tree.get_output_sliced(), tree.size_dict
    )
    twin.children = dict(tree.children)
    twin._extent = dict(tree._extent)
    twin._next_ssa = tree._next_ssa
    # indices sliced away no longer count as appearances
    # (explicit index orders -- ``sort_contraction_indices`` -- are part of the schedule)
    for node, d in tree._info.items():
        if "inds" in d:
            twin._info.setdefault(node, {})["inds"] = d["inds"]
    return twin


def make_contractor(
    tree,
    order=None,
    prefer_einsum=False,
    strip_exponent=False,
    check_zero=False,
    implementation=None,
    autojit=False,
    progbar=False,
    handle_slicing=False,
):
    """Reference ``make_contractor`` (contract.py:925-1006) with the MI355X
    executor as the only engine.  ``prefer_einsum`` and ``autojit`` are
    accepted for signature compatibility and have no effect: the plan never
    distinguishes tensordot from einsum steps and is already compiled."""
    if isinstance(implementation, (tuple, list)):
        # per-op plug-in (contract.py:775-776): the caller's (einsum, tensordot)
        return PerOpContractor(
            tree if (handle_slicing or not tree.sliced_inds) else _sliced_twin(tree),
            implementation, order=order, prefer_einsum=prefer_einsum,
            strip_exponent=strip_exponent, check_zero=check_zero,
        )
    if implementation not in (None, "auto", "hip"):
        raise ValueError(
            f"implementation={implementation!r} is not available: cotengra_amd "
            "executes whole trees with its HIP backend ('hip') or with a caller's "
            "(einsum, tensordot) pair."
        )
    return HipContractor(
        tree,
        order=order,
        strip_exponent=strip_exponent,
        check_zero=check_zero,
        progbar=progbar,
        handle_slicing=handle_slicing,
    )


def _tree_contractor(tree, order=None):
    """Cached slicing-aware contractor of a tree."""
    key = ("hip-sliced", order if not callable(order) else id(order))
    try:
        return tree.contraction_cores[key]
    except KeyError:
        fn = tree.contraction_cores[key] = HipContractor(
            tree, order=order, handle_slicing=True
        )
        return fn


def contract_tree(
    tree,
    arrays,
    order=None,
    prefer_einsum=False,
    strip_exponent=False,
    check_zero=False,
    backend=None,
    implementation=None,
    autojit="auto",
    progbar=False,
):
    """``ContractionTree.contract`` (core.py:3943-4030): every slice runs on
    the device and accumulates into the resident output tensor."""
    if isinstance(implementation, (tuple, list)):
        # per-op plug-in: the host walks slices and steps (core.py:4002-4030)
        core = tree.get_contractor(
            order=order, prefer_einsum=prefer_einsum, strip_exponent=strip_exponent is not False,
            check_zero=check_zero, implementation=implementation,
        )
        if not tree.sliced_inds:
            return core(*arrays)
        slices = (core(*tree.slice_arrays(arrays, i)) for i in range(tree.multiplicity))
        return gather_slices(tree, slices, progbar=progbar)
    if implementation not in (None, "auto", "hip"):
        raise ValueError(f"implementation={implementation!r} is not available.")
    fn = _tree_contractor(tree, order)
    return fn(
        *arrays,
        strip_exponent=strip_exponent is not False,
        check_zero=check_zero,
        progbar=progbar,
    )


def contract_slice(tree, arrays, i, **kwargs):
    """``ContractionTree.contract_slice`` (core.py:3821-3823)."""
    order = kwargs.pop("order", None)
    strip_exponent = kwargs.pop("strip_exponent", False)
    check_zero = kwargs.pop("check_zero", False)
    implementation = kwargs.pop("implementation", None)
    prefer_einsum = kwargs.pop("prefer_einsum", False)
    for k in ("backend", "autojit", "progbar"):
        kwargs.pop(k, None)
    if kwargs:
        raise TypeError(f"Unknown keyword arguments: {kwargs}.")
    if not 0 <= i < tree.multiplicity:
        raise IndexError(f"slice {i} out of range [0, {tree.multiplicity})")
    if isinstance(implementation, (tuple, list)):
        return tree.contract_core(
            tree.slice_arrays(arrays, i), order=order, prefer_einsum=prefer_einsum,
            strip_exponent=strip_exponent, check_zero=check_zero, implementation=implementation,
        )
    fn = _tree_contractor(tree, order)
    return fn.contract_slice(
        arrays, i, strip_exponent=strip_exponent is not False, check_zero=check_zero
    )


def _add_maybe_stripped(x, y):
    """Exponent-aware sum of two slice outputs (core.py:125-172)."""
    xt, yt = isinstance(x, tuple), isinstance(y, tuple)
    if not (xt or yt):
        return x + y
    xm, xe = x if xt else (x, 0.0)
    ym, ye = y if yt else (y, 0.0)
    e = max(xe, ye)
    return xm * 10 ** (xe - e) + ym * 10 ** (ye - e), e


def gather_slices(tree, slices, backend=None, progbar=False):
    """Host-side gather of explicitly computed slice outputs
    (core.py:3825-3882); ``tree.contract`` never needs it because the device
    accumulates, but it is part of the public surface."""
    if progbar:
        prog = _Progress(progbar, tree.nslices)

        def counted(it):
            try:
                for x in it:
                    yield x
                    prog.update(1)
            finally:
                prog.close()

        slices = counted(slices)
    output_pos = {
        ix: i for i, ix in enumerate(tree.output) if ix in tree.sliced_inds
    }
    if not output_pos:
        import functools

        return functools.reduce(_add_maybe_stripped, slices)
    chunks = {}
    for i, s in enumerate(slices):
        ks = tree.slice_key(i)
        key = tuple(ks[ix] for ix in output_pos)
        chunks[key] = _add_maybe_stripped(chunks[key], s) if key in chunks else s
    if isinstance(next(iter(chunks.values())), tuple):
        emax = max(v[1] for v in chunks.values())
        chunks = {k: m * 10 ** (e - emax) for k, (m, e) in chunks.items()}
    else:
        emax = None
    first = next(iter(chunks.values()))
    if _is_torch(first):
        import torch

        stack_fn = lambda arrs, ax: torch.stack(arrs, ax)  # noqa: E731
    else:
        stack_fn = lambda arrs, ax: np.stack(arrs, ax)  # noqa: E731

    def stack(loc, remaining):
        if not remaining:
            return chunks[loc]
        arrs = [
            stack(loc + (d,), remaining[1:])
            for d in tree.sliced_inds[remaining[0]].sliced_range
        ]
        return stack_fn(arrs, output_pos[remaining[0]] - len(loc))

    result = stack((), tuple(output_pos))
    return (result, emax) if emax is not None else result


def gen_output_chunks(tree, arrays, with_key=False, progbar=False, **contract_opts):
    """core.py:3884-3941: one chunk per combination of outer sliced indices,
    inner slices summed on the device."""
    order = contract_opts.pop("order", None)
    fn = _tree_contractor(tree, order)
    stepsize = prod(si.size for si in tree.sliced_inds.values() if si.inner)
    st = fn.setup(*arrays)
    ex = st["exec"]
    ex.set_strip_exponent(False)
    prog = _Progress(progbar, tree.nslices)
    st["pinned"] = st.get("pinned", 0) + 1   # (a suspended generator keeps its executor)
    try:
        for o in range(tree.nslices // stepsize):
            with fn._lock:
                ex.zero_result()
                ex.run_slices(o * stepsize, stepsize, 1)
                loc = tree.slice_key(o * stepsize)
                index = _chunk_index(tree, loc)
                chunk = fn._finish(st, False, False, index=index)
            if prog.active:
                prog.update(stepsize)
            if with_key:
                yield chunk, {ix: x for ix, x in loc.items() if ix in tree.output}
            else:
                yield chunk
    finally:
        st["pinned"] -= 1
        prog.close()


def benchmark_tree(
    tree, dtype="float64", max_time=60, min_reps=3, max_reps=100, warmup=True,
    **contract_opts,
):
    """``ContractionTree.benchmark`` (core.py:4092-4164) on the device: the
    inputs are made resident once, then ``contract_slice`` work is timed."""
    from .utils import make_arrays_from_inputs

    arrays = make_arrays_from_inputs(tree.inputs, tree.size_dict, dtype=dtype)
    fn = _tree_contractor(tree, contract_opts.pop("order", None))
    st = fn.setup(*arrays)
    ex = st["exec"]
    ex.set_strip_exponent(False)
    # slices are timed the way ``contract`` runs them: as many per launch sequence as
    # the executor batches (1 for wide trees, up to 64 for narrow ones)
    nb = max(1, min(int(ex.batch), tree.nslices))
    nstart = max(tree.nslices - nb + 1, 1)
    for i in range(int(warmup)):
        ex.run_slices((i * nb) % nstart, nb, 1)
    ex.sync()
    t0 = ti = time.time()
    i = 0
    while (ti - t0 < max_time) or (i < min_reps):
        ex.run_slices((i * nb) % nstart, nb, 1)
        ex.sync()
        ti = time.time()
        i += 1
        if i >= max_reps:
            break
    time_per_slice = (ti - t0) / (i * nb)
    est_time_total = time_per_slice * tree.nslices
    return {
        "time_per_slice": time_per_slice,
        "est_time_total": est_time_total,
        "est_gigaflops": tree.total_flops(dtype=dtype) / (1e9 * est_time_total),
    }


# ---------------------------------------------------------------------- #
# checkpoint / resume of a sliced run
# ---------------------------------------------------------------------- #
#
# The reference sums slices one after another into a running result
# (``gather_slices``, core.py:3842-3844; ``contract_mpi``, core.py:4073-4076) and
# keeps nothing else between slices, so (how many of my slices are done, the
# partial sum[, its exponent]) is the complete state of a run.  A Sycamore m20
# amplitude is days of GPU time: the state is written every so often and a
# restarted process continues from it -- bit-identically, because the slices
# are added in the same order onto the same bits.


def tree_signature(tree, dtype, rank=0, world=1, strip_exponent=False, check_zero=False, order=None,
                   arrays=None, groups=None):
    """Digest of everything a partial sum depends on: network, schedule,
    slicing, element type, which share of the slices, stripping options -- and,
    with ``arrays``, the input tensors themselves (``inputs_digest``): the same
    Sycamore tree contracted for another bitstring must not resume this sum."""
    import hashlib
    import json

    doc = {
        "inputs": [list(map(str, t)) for t in tree.inputs],
        "output": list(map(str, tree.output)),
        "sizes": sorted((str(k), int(v)) for k, v in tree.size_dict.items()),
        "ssa_path": [list(p) for p in tree.get_ssa_path(order=order)] if tree.N > 1 else [],
        "sliced": [[str(si.ind), si.project] for si in tree.sliced_inds.values()],
        "dtype": str(dtype),
        "share": [int(rank), int(world)],
        "strip": [bool(strip_exponent), bool(check_zero)],
        "arrays": inputs_digest(arrays) if arrays is not None else None,
    }
    if groups:   # (the order in which a rank's slices are summed follows the slice groups)
        doc["groups"] = [str(ix) for ix in groups]
    return hashlib.sha256(json.dumps(doc, sort_keys=True).encode()).hexdigest()


def save_checkpoint(path, signature, done, result, exponent=0.0, zero=False):
    """Atomically replace ``path`` (write to a sibling, fsync, rename): a crash
    while writing leaves the previous checkpoint intact."""
    import os
    import tempfile

    d = os.path.dirname(os.path.abspath(path)) or "."
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=d)
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez(
                f, signature=np.array(signature), done=np.int64(done), result=np.asarray(result),
                exponent=np.float64(exponent), zero=np.bool_(zero),
            )
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def load_checkpoint(path, signature):
    """``(done, result, exponent, zero)`` or None when there is no checkpoint;
    ``ValueError`` when the file belongs to a different contraction."""
    import os

    if not os.path.exists(path):
        return None
    with np.load(path, allow_pickle=False) as z:
        if str(z["signature"]) != signature:
            raise ValueError(
                f"checkpoint {path} was written for a different tree / dtype / rank layout / "
                "set of input tensors (signature mismatch); remove it to start over."
            )
        return int(z["done"]), z["result"].copy(), float(z["exponent"]), bool(z["zero"])


def contract_resumable(
    tree, arrays, checkpoint, every=64, order=None, strip_exponent=False, check_zero=False,
    rank=0, world=1, stop_after=None, keep=False, progbar=False,
):
    """``tree.contract(arrays)`` that survives being killed.

    This rank's slices (``rank, rank + world, ...``: ``world=1`` is all of
    them) run in chunks of ``every``; after each chunk the partial sum is
    downloaded (``ctg_exec_get_state``) and written to ``checkpoint``.  If the
    file already exists the run restores it (``ctg_exec_set_state``) and
    continues with the first slice not yet summed.  ``stop_after=n`` ends this
    call after at most ``n`` more slices (returns None unless that completed
    the run) -- what a job-time limit or a test uses.  The file is removed when
    the run completes unless ``keep`` (that removal is housekeeping, not a
    guard: what ties a file to a run is its signature, which covers the tree,
    the options, the rank's share AND the bytes of the input tensors).  Returns
    what ``contract`` returns (this rank's share when ``world > 1``: feed it to
    the collective)."""
    import os

    fn = _tree_contractor(tree, order)
    with fn._lock:
        return _contract_resumable_locked(
            fn, tree, arrays, checkpoint, every, order, strip_exponent, check_zero, rank, world,
            stop_after, keep, progbar,
        )


def _contract_resumable_locked(fn, tree, arrays, checkpoint, every, order, strip_exponent, check_zero,
                               rank, world, stop_after, keep, progbar):
    import os

    st = fn.setup(*arrays)
    ex = st["exec"]
    ex.set_strip_exponent(strip_exponent, check_zero)
    plan = st["plan"]
    # this rank's share is what the library deals it (Plan.share_units: whole slice groups rank, rank + world,
    # ... -- single slices without group indices); the count of the checkpoint runs along that order and
    # chunks are whole units
    units, gs = plan.share_units(rank, world)
    total = units * gs
    grouped = gs > 1
    every = gs * max(1, -(-int(every) // gs))

    def ids_at(start, n):
        u0, u1 = start // gs, -(-(start + n) // gs)
        return plan.rank_slice_ids(rank, world, u0, u1 - u0)[start - u0 * gs: start - u0 * gs + n]
    sig = tree_signature(tree, st["plan"].dtype, rank, world, strip_exponent, check_zero, order,
                         arrays=arrays, groups=plan.group_inds if grouped else None)
    saved = load_checkpoint(checkpoint, sig)
    if saved is None:
        done = 0
        ex.zero_result()
    else:
        done, result, exponent, zero = saved
        if not 0 <= done <= total:
            raise ValueError(f"checkpoint {checkpoint} claims {done} of {total} slices")
        ex.set_state(result, exponent, zero)
    budget = total - done if stop_after is None else min(int(stop_after), total - done)
    prog = _Progress(progbar, total)
    if prog.active and done:
        prog.update(done)
    try:
        while budget > 0:
            n = min(int(every), budget)
            if done % gs == 0 and n % gs == 0:
                ex.run_share(rank, world, done // gs, n // gs)
            else:   # (a run stopped inside a group by ``stop_after``)
                ex.run_slice_list(ids_at(done, n))
            done += n
            budget -= n
            # (the running sum in the precision the executor carries it in: double for single-precision trees)
            result, exponent, zero = ex.get_state_wide()
            save_checkpoint(checkpoint, sig, done, result, exponent, zero)
            if prog.active:
                prog.update(n)
    finally:
        prog.close()
    if done < total:
        return None
    out = fn._finish(st, strip_exponent, check_zero)
    if not keep and os.path.exists(checkpoint):
        os.unlink(checkpoint)
    return out
