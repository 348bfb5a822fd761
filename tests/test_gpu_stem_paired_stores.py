"""Paired stores of the stem kernels on the device (csrc/ctg_stem_impl.h: stem2h_kernel_p16).

A specialised-wave consumer that holds both 32-column groups of a row tile deals the result's columns to the groups
alternately and writes two adjacent columns of a row as one 16-byte store, where the step's tables allow it.  Same
products in the same order: the numbers must be those of the 8-byte form BIT FOR BIT.  The cases of
tests/stem_paired_cases.py (planned as they say: tests/test_stem_paired_stores_host.py), each a small stem with a running
tensor of 2^15 or 2^16 elements -- one of 2^22, two tiles per workgroup, integer data only -- checked like the rows of
tests/test_gpu_stem_variants.py:

form      in fp16 x 2 the LAUNCHER recorded of every stem step what the case says (``ctg_exec_step_paired_stores``
          reports which kernel the step's last launch took, written down where the kernel is chosen), in bf16 x 3 and
          with fp32 products no step pairs, and the kernel names are what they are without pairs;
integer   inputs with parts in {-1, 0, 1}: the oracle's integers bit for bit, in all three arithmetics (the argument
          of tests/test_gpu_stem_variants.py; the gate behind the pair of a ``_tail`` case has K = 8: its sums stay
          below 2^24, asserted from the oracle's result);
random    complex64 data against the complex128 oracle under the suite's single-precision gate;
same      fp16 x 2, random data: the result with pairs and the result under CTG_STEM_NO_PAIR16=1 (8-byte stores, read
          per launch) are the same bits -- on ``chain`` too, whose second pair splits its big operand by the largest
          element the first one recorded while it stored;
maximum   the record itself (StemArgs::cmax, read back with ``ctg_exec_step_stem_max``): of every stem step the same
          float with pairs and without, and -- where the step's result is still in the arena behind the run: the last
          stem step of an unsliced case -- equal to the largest |real or imaginary part| of what was stored;
strip     ``strip_exponent`` on one case (no fp16 x 2 there: the pair runs in bf16 x 3 on 8-byte stores; the scaled
          variant of the paired consumer loop is therefore never run by any launch: fp16 x 2 always scales, its
          kernels take the one path).
"""
import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd.plan import KIND_STEM2, SPACE_ARENA
from oracle import contract_ref as orc

import golden_util as G
import stem_paired_cases as P
from test_gpu_stem_valu_paths import stem_env  # noqa: F401  (the fixture: every capable step on the stem kernels)
from test_gpu_stem_variants import assert_exact, contractor, integer_arrays, stem_names, top_of

pytestmark = pytest.mark.gpu

ARITHS = ("fp32", "bf16x3", "fp16x2")
SMALL = [c for c in P.CASES if c.nq - c.sliced <= 16 and c.id != "chain"]

_DATA = {}


def data_of(case, random=True):
    """(tree, random arrays, complex128 reference, numpy's complex64 result, integer arrays, integer reference): once
    per case, never modified."""
    if case.id not in _DATA:
        tree = case.tree()
        arrays = ref = np64 = None
        if random:
            arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=7, dtype="complex64")
            ref = np.asarray(orc.contract(tree, [a.astype("complex128") for a in arrays]))
            np64 = np.asarray(orc.contract(tree, arrays))
        ints = integer_arrays(tree, 11 + case.seed)
        i128 = [a.astype("complex128") for a in ints]
        iref = np.asarray(orc.contract(tree, i128))
        # exact in fp32 in any order: a gate that contracts k indices of a tensor with components of at most `top` in
        # magnitude (its own are at most 1) has partial sums of at most 2^k x 2 x top -- kept below 2^24 from the
        # oracle's results of the chain's prefixes, slice by slice; and something to compare
        gates = [(3, 3)] + case.gates
        for upto in range(1, len(gates)):
            prefix = case.tree(upto=upto)
            top = max(top_of(orc.contract_slice(prefix, i128[:upto + 1], i)) for i in range(prefix.nslices))
            assert (2 << gates[upto][0]) * top < 1 << 24, (case.id, upto, top)
        assert top_of(iref) * tree.nslices < 1 << 24 and np.count_nonzero(iref) > iref.size // 2, case.id
        assert np.array_equal(iref, np.round(iref.real) + 1j * np.round(iref.imag))
        iref = iref.astype("complex64")
        for x in (arrays or []) + ints + [iref]:
            x.setflags(write=False)
        _DATA[case.id] = (tree, arrays, ref, np64, ints, iref)
    return _DATA[case.id]


def clean_env(monkeypatch):
    for k in ("CTG_STEM_FORM", "CTG_STEM_GENERIC", "CTG_STEM_NO_RI2", "CTG_STEM_NO_PAIR16"):
        monkeypatch.delenv(k, raising=False)


def paired_steps(fn, arrays):
    """Which form the last launch of each stem step took, in step order (call it behind a run)."""
    ex = fn.setup(*arrays)["exec"]
    names, flags = ex.step_kernels(), ex.step_paired_stores()
    return [f for n, f in zip(names, flags) if n.startswith(("stem2_kernel", "stem2h_kernel"))]


def recorded_maxima(fn, arrays, stored=False):
    """The maximum each stem step recorded in its last launch (slice 0 of the batch), in step order; ``stored``: also
    the largest |component| of the last stem step's result as it lies in the arena."""
    st = fn.setup(*arrays)
    ex, plan = st["exec"], st["plan"]
    stems = [i for i, s in enumerate(plan.steps) if s.kind == KIND_STEM2]
    rec = [ex.step_stem_max(i) for i in stems]
    if not stored:
        return rec
    c = plan.steps[stems[-1]].c
    assert c.space == SPACE_ARENA and c.leaf < 0
    return rec, top_of(ex.download_arena(c.offset, c.size))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_cases_in_the_three_arithmetics(case, arith, stem_env, monkeypatch):
    tree, arrays, ref, np64, ints, iref = data_of(case)
    clean_env(monkeypatch)
    fn = contractor(tree, arith)
    try:
        got = np.asarray(fn(*arrays))
        names, paired = stem_names(fn, arrays), paired_steps(fn, arrays)
        exact = np.asarray(fn(*ints))
    finally:
        fn.close()
    monkeypatch.setenv("CTG_STEM_NO_PAIR16", "1")
    fn = contractor(tree, arith)   # (a fresh executor: every step is launched again)
    try:
        again = np.asarray(fn(*arrays))
        names_off, paired_off = stem_names(fn, arrays), paired_steps(fn, arrays)
    finally:
        fn.close()
    print(case.id, arith, names, paired)
    assert len(names) == len(case.shapes)
    assert paired == (case.paired if arith == "fp16x2" else [False] * len(case.shapes)), (case.id, arith, paired)
    # (the switch is read per launch, and the name the executor reports does not depend on the form)
    assert paired_off == [False] * len(case.shapes) and names_off == names
    assert np.array_equal(again, got)
    err, gate = G.relerr(got, ref), G.single_gate(ref, np64)
    print(case.id, arith, "relerr", err, "gate", gate)
    assert err <= gate, (err, gate)
    assert_exact(case, arith, exact, iref)


@pytest.mark.parametrize("case", [c for c in P.CASES if any(c.paired) and c.nq <= 16], ids=repr)
def test_same_bits_with_and_without_pairs(case, stem_env, monkeypatch):
    tree, arrays, ref, np64, _, _ = data_of(case)
    clean_env(monkeypatch)
    fn = contractor(tree, "fp16x2")
    try:
        unsliced = tree.nslices == 1
        with_pairs = np.asarray(fn(*arrays)).copy()
        paired = paired_steps(fn, arrays)
        rec_on = recorded_maxima(fn, arrays, stored=unsliced)
    finally:
        fn.close()
    monkeypatch.setenv("CTG_STEM_NO_PAIR16", "1")
    fn = contractor(tree, "fp16x2")   # (a fresh executor: every step is launched again)
    try:
        without = np.asarray(fn(*arrays)).copy()
        paired_off = paired_steps(fn, arrays)
        rec_off = recorded_maxima(fn, arrays, stored=unsliced)
    finally:
        fn.close()
    assert paired == case.paired and not any(paired_off), (case.id, paired, paired_off)
    print(case.id, "recorded maxima", rec_on, rec_off)
    assert rec_on == rec_off, (case.id, rec_on, rec_off)
    if unsliced:
        (rec, top), (rec8, top8) = rec_on, rec_off
        assert all(r > 0 for r in rec) and rec[-1] == top == top8 == rec8[-1], (case.id, rec, top, rec8, top8)
    else:
        assert all(r > 0 for r in rec_on)
    err, gate = G.relerr(with_pairs, ref), G.single_gate(ref, np64)
    print(case.id, "relerr", err, "gate", gate)
    assert err <= gate, (err, gate)
    assert_exact(case, "16-byte against 8-byte stores", with_pairs, without)


def test_two_tiles_per_workgroup(stem_env, monkeypatch):
    case = P.by_id("deep512")
    tree, _, _, _, ints, iref = data_of(case, random=False)
    clean_env(monkeypatch)
    fn = contractor(tree, "fp16x2")
    try:
        exact = np.asarray(fn(*ints))
        paired = paired_steps(fn, ints)
    finally:
        fn.close()
    assert paired == case.paired
    assert_exact(case, "fp16x2", exact, iref)


def test_slices_one_by_one(stem_env, monkeypatch):
    case = P.by_id("sliced")
    tree, arrays, _, _, _, _ = data_of(case)
    assert tree.nslices == 2
    clean_env(monkeypatch)
    fn = contractor(tree, "fp16x2")
    try:
        parts = [np.asarray(fn.contract_slice(arrays, i)).copy() for i in range(2)]
        paired = paired_steps(fn, arrays)
    finally:
        fn.close()
    assert paired == case.paired
    a128 = [a.astype("complex128") for a in arrays]
    for i, part in enumerate(parts):
        want = np.asarray(orc.contract_slice(tree, a128, i))
        err, gate = G.relerr(part, want), G.single_gate(want, np.asarray(orc.contract_slice(tree, arrays, i)))
        print(case.id, "slice", i, "relerr", err, "gate", gate)
        assert err <= gate, (i, err, gate)


def test_strip_exponent(stem_env, monkeypatch):
    case = P.by_id("k32n32_k64n64_tail")
    tree, arrays, ref, np64, _, _ = data_of(case)
    clean_env(monkeypatch)
    fn = contractor(tree, "fp16x2")
    try:
        m, e = fn(*arrays, strip_exponent=True)
        got = np.asarray(m) * 10.0 ** e
        paired = paired_steps(fn, arrays)
    finally:
        fn.close()
    assert paired == [False]   # (a scale per step: the pair runs in bf16 x 3)
    err, gate = G.relerr(got, ref), G.single_gate(ref, np64)
    print(case.id, "strip_exponent relerr", err, "gate", gate)
    assert err <= gate, (err, gate)
