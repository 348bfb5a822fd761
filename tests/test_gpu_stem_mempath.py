"""Stem kernels with gathers in portions and non-temporal stores (csrc/ctg_stem_impl.h: CTG_STEM_GATHER_PORTIONS,
CTG_STEM_NT_STORES).

The 16-bit kernels refill a task's gather registers one or two pairs in front of each product instead of all four
behind the split, and every stem kernel stores its result with the non-temporal hint.  Neither changes which products an
accumulator sees or their order; what can go wrong is a register pair refilled before the split has read it or while
a product still needs it, a wait that counts the wrong loads, or a store that is lost.  (How a consumer hands out its
pending stores is NOT changed and not what these cases are about: they run the consumers' paths because that is where
the stores are issued.)

One stem pair (or single step) per case:

    k32 n32 | k64 n64    one column group per task; the consumers' ``item2k`` with four chunks
    k64 n64 | k32 n32    a task multiplied into two column groups (two MFMA loops per product), B1 from LDS
    k16 n16 | k32 n32    16 columns in step 1 (two MFMAs per product), two row tiles per producer
    k32 n32 | k16 n16    16 columns in step 2: stores of two rows per instruction
    k64 | n128           a single step: gathers and deferred stores in one instruction stream

each on a running tensor of 2^21 elements per slice (one tile per workgroup, two for the single step: the peeled
entry and the tail alone) and of 2^23 (four and more: the steady state) -- asserted from the plan's tile count --, in
fp16 x 2, bf16 x 3 and fp32.  The network
has one sliced index: the sum of its two slices is held to the complex128 oracle under the suite's single-precision
gate, and in the 16-bit arithmetics slice 1 alone must equal, bit for bit, the unsliced stem it is -- the same network
with the sliced index fixed at 1 -- run by the same kernels."""
import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd.contractor import HipContractor
from oracle import contract_ref as orc

import golden_util as G

pytestmark = pytest.mark.gpu

# name -> (gates of the step(s), seed with which the planner takes the shape the name says, the step's label)
CASES = {
    "k32n32_k64n64": ([(5, 5), (6, 6)], 1, "stem2 k32 n32 | k64 n64"),
    "k64n64_k32n32": ([(6, 6), (5, 5)], 1, "stem2 k64 n64 | k32 n32"),
    "k16n16_k32n32": ([(4, 4), (5, 5)], 2, "stem2 k16 n16 | k32 n32"),
    "k32n32_k16n16": ([(5, 5), (4, 4)], 1, "stem2 k32 n32 | k16 n16"),
    # (a seed whose contracted indices leave the stride-1 index open: the 16-byte-gather layout of this shape has no
    # 16-bit single-step kernel and runs with fp32 products in every arithmetic)
    "k64n128": ([(6, 7)], 2, "stem1 k64 n128"),
}
SIZES_LOG2 = [21, 23]
ARITHS = ["fp16x2", "bf16x3", "fp32"]
OPTS = dict(fuse=True, fuse_min_elems=1 << 10)


@pytest.fixture
def stem_env(monkeypatch):
    """Every capable step on the stem kernels (single steps too), nothing in the environment names an arithmetic."""
    from cotengra_amd import stem
    G.fuse_whatever_fits(monkeypatch, h2_all=True)
    monkeypatch.setattr(stem, "single_seconds", lambda *a, **k: 0.0)
    monkeypatch.delenv("CTG_STEM_FORM", raising=False)


def fixed_at(tree, arrays, key):
    """The network of ``tree`` with its sliced indices fixed at ``key``: an unsliced tree with the same chain."""
    inputs = [tuple(ix for ix in t if ix not in key) for t in tree.inputs]
    output = tuple(ix for ix in tree.output if ix not in key)
    sub = [np.ascontiguousarray(a[tuple(key[ix] if ix in key else slice(None) for ix in t)])
           for a, t in zip(arrays, tree.inputs)]
    size_dict = {ix: 2 for t in inputs for ix in t}
    ssa, cur, nxt = [], 0, len(inputs)
    for i in range(1, len(inputs)):
        ssa.append((cur, i))
        cur, nxt = nxt, nxt + 1
    return ca.ContractionTree.from_path(inputs, output, size_dict, ssa_path=ssa), sub


_REF = {}


def reference(case, size_log2):
    """(tree, arrays, complex128 oracle, numpy's complex64 result, slice 1 as an unsliced tree and its arrays): computed
    once per case and size, shared by the arithmetics, never modified."""
    if (case, size_log2) not in _REF:
        gates, seed, _ = CASES[case]
        tree = G.stem_network(size_log2 + 1, [(3, 3)] + gates, seed, sliced=1)
        arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=7, dtype="complex64")
        for a in arrays:
            a.setflags(write=False)
        ref = np.asarray(orc.contract(tree, [a.astype("complex128") for a in arrays]))
        np64 = np.asarray(orc.contract(tree, arrays))
        one, sub = fixed_at(tree, arrays, orc.slice_key(tree, 1))
        for a in sub:
            a.setflags(write=False)
        _REF[(case, size_log2)] = (tree, arrays, ref, np64, one, sub)
    return _REF[(case, size_log2)]


def contractor(tree, arith, monkeypatch):
    if arith == "fp32":
        monkeypatch.setenv("CTG_STEM_BF16X3", "0")
    return HipContractor(tree, **OPTS, **({"stem_bf16x3": "bf16x3"} if arith == "bf16x3" else {}))


def stem_names(fn, arrays):
    return [n for n in fn.setup(*arrays)["exec"].step_kernels() if n.startswith(("stem2_kernel", "stem2h_kernel"))]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("size_log2", SIZES_LOG2)
@pytest.mark.parametrize("case", list(CASES))
def test_stem_step_with_portioned_memory_instructions(case, size_log2, arith, stem_env, monkeypatch):
    tree, arrays, ref, np64, one, sub = reference(case, size_log2)
    assert tree.nslices == 2 and one.nslices == 1
    fn = contractor(tree, arith, monkeypatch)
    try:
        got = np.asarray(fn(*arrays))
        names = stem_names(fn, arrays)
        steps = fn.setup(*arrays)["plan"].steps
        labels = [s.label for s in steps]
        slice1 = np.asarray(fn.contract_slice(arrays, 1)) if arith != "fp32" else None
    finally:
        fn.close()
    print(case, size_log2, arith, names)
    # the step this case is about ran, on the kernel of its arithmetic
    assert any(lb.startswith(CASES[case][2] + " rows") for lb in labels), labels
    assert len(names) == 1, names
    # tiles per workgroup (a launch has min(tiles, 256) workgroups): at most two, or at least four
    (tiles,) = [s.stem["n_tiles"] for s in steps if s.label.startswith(CASES[case][2] + " rows")]
    assert (256 <= tiles <= 512) if size_log2 == 21 else tiles >= 4 * 256, tiles
    flags = G.stem_flags(names[0])
    assert names[0].startswith("stem2h_kernel" if arith == "fp16x2" else "stem2_kernel"), names
    assert flags["bf3"] == (arith != "fp32") and flags["one"] == (case == "k64n128"), names
    if arith == "fp16x2" and case != "k64n128":
        assert flags["ws"], names
    err, gate = G.relerr(got, ref), G.single_gate(ref, np64)
    print("relerr", err, "gate", gate)
    assert err <= gate, (err, gate)
    if slice1 is None:
        return
    # slice 1 alone is the unsliced stem with the index fixed: the same kernel, the same bits
    fn1 = contractor(one, arith, monkeypatch)
    try:
        alone = np.asarray(fn1(*sub))
        names1 = stem_names(fn1, sub)
    finally:
        fn1.close()
    assert names1 == names, (names1, names)
    assert alone.shape == slice1.shape
    assert np.array_equal(alone, slice1), float(np.abs(alone - slice1).max())
