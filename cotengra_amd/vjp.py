"""Compile the vector-Jacobian product of a (sliced) contraction tree into a device plan.

For a tree with leaves ``x_0 .. x_{N-1}`` and result ``O`` (the gathered shape: output-sliced axes
stacked, projected axes of size 1) and a cotangent ``h`` of ``O``'s shape, the VJP (JAX's convention,
no conjugation) is

    G_i = sum_o h[o] dO[o] / dx_i        (shape of x_i, summed over all slices)

Per slice, the reverse sweep seeds ``H_root`` with the slice's chunk of ``h`` and, for every node
``p = (l, r)`` from the root down, forms ``H_l = pair(H_p, T_r -> legs(l))`` and
``H_r = pair(H_p, T_l -> legs(r))``; ``legs(l)`` is a subset of ``legs(p) | legs(r)`` for every node of a
tree (hyper-indices included), so each is an ordinary gather-GEMM step (``plan.build_pair_step``).  A
leaf's ``H`` is added into ``G_i`` at that slice's offsets by a ``KIND_ACCUM`` whose result operand names
leaf ``i``; its row tables undo the leaf's preprocessing: an index preprocessing summed away has stride 0
on the read side (broadcast), a repeated index has its strides summed on the write side (the diagonal).

So a gradient is one more plan: slice batching, the double-precision slice sum, ``run_share``, the RCCL
reduce and checkpoints apply to it unchanged.  Inputs are the N leaves and the cotangent (input N, read
in place through the forward's output slice strides); the result is the gradients of the ``wrt`` leaves
back to back, each in its leaf's full row-major layout (``Plan.grad_offsets``).  No step conjugates
anything: the torch layer conjugates the cotangent on the way in and the gradients on the way out.
"""

from __future__ import annotations

import math

import numpy as np

from .plan import (
    ARENA_ALIGN,
    KIND_ACCUM,
    KIND_PAIR,
    LEVEL_ORDER_MAX_ELEMS,
    MAX_TENSOR_ELEMS,
    SPACE_ARENA,
    SPACE_INPUTS,
    SPACE_RESULT,
    Arena,
    Plan,
    Step,
    TensorRef,
    _row_major_strides,
    _rows_two_level,
    build_pair_step,
    build_single_step,
)
from .utils import prod


def _align(n):
    return (n + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN


def leaf_accum_step(size_dict, src, term, sliced, offset, leaf, size):
    """``result[offset + slice offset of leaf + pos(o)] += src[o]`` over the leaf's unsliced indices
    ``o``: an index ``src`` lacks (summed away by preprocessing) is read with stride 0, a repeated index
    of ``term`` is written with its strides summed (the diagonal)."""
    full = _row_major_strides([size_dict[ix] for ix in term])
    rows_g = [ix for ix in dict.fromkeys(term) if ix not in sliced]
    res = TensorRef(
        SPACE_RESULT, offset, leaf, tuple(rows_g),
        tuple(sum(s for i, s in zip(term, full) if i == ix) for ix in rows_g), size,
    )
    acc = Step(kind=KIND_ACCUM, a=src, c=res, node=leaf, label=f"gradient {leaf}")
    ext = [size_dict[ix] for ix in rows_g]
    acc.R = prod(ext)
    acc.row_lo, (acc.rows["A"], acc.rows["C"]) = _rows_two_level(
        ext, [[src.stride_of(ix) for ix in rows_g], [res.stride_of(ix) for ix in rows_g]]
    )
    acc.elems_rw = 0
    return acc


def compile_vjp(tree, dtype, wrt=None, order=None):
    """A :class:`Plan` that computes, per slice, the forward intermediates the reverse sweep needs, the
    sweep itself and one ``KIND_ACCUM`` per leaf of ``wrt`` (default: all leaves) into its gradient.

    Inputs: the N leaves, then the cotangent (shape ``tree.gathered_shape()``).  Result: flat, the
    gradients back to back at ``plan.grad_offsets[i]`` (64-element aligned, the leaf's full layout).
    Forward steps are unfused (no stem pairs, LDS-resident subtrees or slice groups); slice-invariant
    ones run once per upload.  Every intermediate the backward reads stays alive until its last reader.
    """
    N = tree.N
    wrt = tuple(range(N)) if wrt is None else tuple(sorted(set(int(i) for i in wrt)))
    if not wrt or wrt[0] < 0 or wrt[-1] >= N:
        raise ValueError(f"wrt must name at least one of the {N} leaves, got {wrt}")
    size_dict = tree.size_dict
    if N > 1 and tree.max_size() > MAX_TENSOR_ELEMS:
        raise MemoryError(
            f"the largest intermediate of one slice has 2^{math.log2(tree.max_size()):.1f} elements; "
            f"slice the tree (ContractionTree.slice / pathfind.slice_tree) to at most "
            f"2^{int(math.log2(MAX_TENSOR_ELEMS))} before contracting on one device"
        )
    plan = Plan(dtype)
    sliced_map = tree.sliced_inds

    # -- inputs space: the leaves, then the cotangent
    cursor = 0
    for term in tree.inputs:
        n = prod(size_dict[ix] for ix in term)
        plan.input_sizes.append(n)
        plan.input_offsets.append(cursor)
        cursor += _align(n)
    gshape = tuple(tree.gathered_shape())
    plan.input_sizes.append(prod(gshape))
    plan.input_offsets.append(cursor)
    cursor += _align(prod(gshape))
    plan.inputs_elems = max(cursor, ARENA_ALIGN)
    out_strides = dict(zip(tree.output, _row_major_strides(gshape)))

    # -- result: the gradients of the wrt leaves back to back
    plan.grad_offsets = {}
    rcur = 0
    for i in wrt:
        plan.grad_offsets[i] = rcur
        rcur += _align(plan.input_sizes[i])
    plan.result_elems = rcur
    plan.result_shape = (rcur,)

    # -- slicing: rows 0..N-1 the leaves, N the cotangent (the forward's output row), N+1 the pseudo-leaf
    sliced = list(sliced_map.values())
    plan.nslices = tree.multiplicity
    plan.slice_sizes = [si.size for si in sliced]
    plan.slice_fixed = [(-1 if si.project is None else si.project) for si in sliced]
    strides = np.zeros((N + 2, len(sliced)), dtype=np.int64)
    for i, term in enumerate(tree.inputs):
        st = _row_major_strides([size_dict[ix] for ix in term])
        for j, si in enumerate(sliced):
            strides[i, j] = sum(s for ix, s in zip(term, st) if ix == si.ind)
    for j, si in enumerate(sliced):
        strides[N, j] = 0 if si.project is not None else out_strides.get(si.ind, 0)
    plan.slice_strides = strides

    root_order = tuple(ix for ix in tree.output if ix not in sliced_map)
    cot = TensorRef(
        SPACE_INPUTS, plan.input_offsets[N], N, root_order,
        tuple(out_strides[ix] for ix in root_order), plan.input_sizes[N],
    )

    def add(step):
        plan.steps.append(step)
        plan.macs_per_slice += step.macs
        plan.elems_rw_per_slice += step.elems_rw
        plan.elems_moved_per_slice += step.elems_rw

    def view(i):
        term = tree.inputs[i]
        st = _row_major_strides([size_dict[ix] for ix in term])
        kept = [(ix, s) for ix, s in zip(term, st) if ix not in sliced_map]
        return TensorRef(
            SPACE_INPUTS, plan.input_offsets[i], i, tuple(ix for ix, _ in kept),
            tuple(s for _, s in kept), plan.input_sizes[i],
        )

    if N == 1:
        # the gradient of a single-term einsum is the cotangent broadcast / put on the diagonal
        add(leaf_accum_step(size_dict, cot, tree.inputs[0], sliced_map, plan.grad_offsets[0], 0,
                            plan.input_sizes[0]))
        plan.arena_elems = ARENA_ALIGN
        return plan

    # -- which tensors the sweep needs
    nodes = list(tree.traverse(order=order))
    level = None
    if order is None and N > 3 and tree.max_size() <= LEVEL_ORDER_MAX_ELEMS:
        level = {}
        for p, l, r in tree.traverse():
            level[p] = 1 + max(level.get(l, 0), level.get(r, 0))
        nodes = list(tree.traverse(order=lambda node: (level[node], tree.get_flops(node))))
    kids = {p: (l, r) for p, l, r in nodes}
    wset = set(wrt)
    has_wrt = {i: i in wset for i in range(N)}
    depends = {i: i in tree.sliced_inputs for i in range(N)}
    for p, l, r in tree.traverse():
        has_wrt[p] = has_wrt[l] or has_wrt[r]
        depends[p] = depends[l] or depends[r]
    use_invariants = tree.multiplicity > 1
    need_t = {tree.root: False}
    for p, l, r in reversed(nodes):
        need_t[l] = has_wrt[r] or need_t[p]
        need_t[r] = has_wrt[l] or need_t[p]

    # -- the schedule: (kind, node, keys read, wave); keys ("T", node) / ("H", node)
    ops = []
    for i in range(N):
        tree.get_legs(i)   # (fills tree.preprocessing)
        if need_t[i] and i in tree.preprocessing:
            ops.append(("single", i, [], ("F", 0)))
    for p, l, r in nodes:
        if p != tree.root and need_t[p]:
            ops.append(("pair", p, [("T", l), ("T", r)], ("F", level[p] if level else 0)))
    if level is not None:
        back = sorted(nodes, key=lambda x: (-level[x[0]], tree.get_flops(x[0])))
    else:
        back = list(reversed(nodes))
    for p, l, r in back:
        for c, sib in ((l, r), (r, l)):
            if has_wrt[c]:
                ops.append(("back", c, [("H", p), ("T", sib)], ("B", -level[p] if level else 0)))
    for i in wrt:
        ops.append(("accum", i, [("H", i)], ("A", 0)))
    last = {}
    for k, (_, _, reads, _) in enumerate(ops):
        for key in reads:
            last[key] = k

    arena, parena = Arena(), Arena()
    live = {}          # id(TensorRef) -> (offset, n)
    persistent = []    # TensorRefs of slice-invariant results (placed behind the per-slice arena)
    per_slice = []

    def factory(invariant):
        def make(inds, natural):
            shape = [size_dict[ix] for ix in natural]
            n = prod(shape)
            pool = parena if invariant else arena
            ref = TensorRef(SPACE_ARENA, pool.alloc(n), -1, tuple(natural), _row_major_strides(shape), n)
            (persistent if invariant else per_slice).append(ref)
            if not invariant:
                live[id(ref)] = (ref.offset, n)
            return ref

        return make

    def release(ref):
        if ref.space == SPACE_ARENA and id(ref) in live:
            arena.release(*live.pop(id(ref)))

    tensors = {("H", tree.root): cot}
    for i in range(N):
        if not (need_t[i] and i in tree.preprocessing):
            tensors[("T", i)] = view(i)
    pending, wave = [], None
    for k, (kind, node, reads, w) in enumerate(ops):
        if level is not None and w != wave:
            for ref in pending:
                release(ref)
            pending, wave = [], w
        if kind == "single":
            inv = use_invariants and not depends[node]
            step = build_single_step(size_dict, view(node), tuple(tree.get_legs(node)), factory(inv), node=node)
            step.invariant = inv
            tensors[("T", node)] = step.c
        elif kind == "pair":
            inv = use_invariants and not depends[node]
            l, r = kids[node]
            step = build_pair_step(dtype, size_dict, tensors[("T", l)], tensors[("T", r)],
                                   tuple(tree.get_legs(node)), factory(inv), node=node)
            step.invariant = inv
            tensors[("T", node)] = step.c
        elif kind == "back":
            hp, ts = (tensors[key] for key in reads)
            step = build_pair_step(dtype, size_dict, hp, ts, tuple(tree.get_legs(node)), factory(False), node=node)
            step.label = "grad " + step.label
            tensors[("H", node)] = step.c
        else:
            step = leaf_accum_step(size_dict, tensors[("H", node)], tree.inputs[node], sliced_map,
                                   plan.grad_offsets[node], node, plan.input_sizes[node])
        add(step)
        for key in reads:
            if last[key] == k:
                ref = tensors.pop(key)
                if level is not None:
                    pending.append(ref)
                else:
                    release(ref)
    for ref in pending:
        release(ref)

    slice_peak = max(arena.peak, ARENA_ALIGN)
    for ref in persistent:
        ref.offset += slice_peak
    plan.arena_elems = slice_peak + parena.peak
    return plan


def pair_steps(plan):
    """Number of pair steps of ``plan`` (forward and backward)."""
    return sum(1 for s in plan.steps if s.kind == KIND_PAIR)
