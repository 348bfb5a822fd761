"""GPU suite: every variant of the complex64 pair kernels (csrc/ctg_pair_mfma.hip) -- the streaming kernel in its
thirty reachable instantiations and with its task loop going round, the k-streaming kernel, the tiled kernels on
16, 32, 64 and 128 columns with and without 16-byte gathers and k-splits, the 16-bit pipe, and every instantiation
of the skinny and the row-wise kernel.

Every case first asserts the kernel the executor names for its step (tests/golden_util.py: pair_flags_c64) and then
compares the result element-wise with ``numpy.einsum`` in complex128 under ``G.single_gate`` against numpy's own
complex64 einsum, the suite's one rule for single precision.  One wrong row offset, one dropped k or one transposed
accumulator register is an error of order 1 against that gate.  The tables are in tests/pair_variant_cases_c64.py;
tests/test_pair_variant_plans.py pins their plans on the host; profiles/pair_variants_c64.txt records what ran."""
import numpy as np
import pytest

import golden_util as G
import pair_variant_cases_c64 as C
from cotengra_amd.contractor import HipContractor

pytestmark = pytest.mark.gpu

DTYPE = "complex64"
_DATA = {}


def einsum_ref(eq, a, b):
    """``numpy.einsum`` of the pair.  An index that both operands and the result carry (a batch index) is looped over,
    one einsum per entry: numpy then multiplies every entry through BLAS where it would otherwise run the whole
    contraction in its scalar loop (16 s for the largest batched row)."""
    (ta, tb), out = eq.split("->")[0].split(","), eq.split("->")[1]
    batch = [ix for ix in out if ix in ta and ix in tb]
    if not batch:
        return np.einsum(eq, a, b, optimize=True)
    x = batch[0]
    sub = eq.replace(x, "")
    parts = [einsum_ref(sub, np.take(a, i, axis=ta.index(x)), np.take(b, i, axis=tb.index(x)))
             for i in range(a.shape[ta.index(x)])]
    return np.stack(parts, axis=out.index(x))


def data(case):
    """``(operands, reference, gate)`` of a case: computed once, shared by the tests that follow one another on the
    same operands (the last two are kept: the references of the deep rows are hundreds of megabytes).  Rows derived
    from one another by reshaping an index (sliced_rows, split_contracted) share extents, seed and numbers."""
    key = (case.eq, tuple(sorted(case.sizes.items())), case.seed)
    if key not in _DATA:
        while len(_DATA) >= 2:
            _DATA.pop(next(iter(_DATA)))
        arrays = case.arrays(DTYPE)
        ref = einsum_ref(case.eq, *[x.astype("complex128") for x in arrays])
        tol = G.single_gate(ref, einsum_ref(case.eq, *arrays))
        ref.setflags(write=False)
        _DATA[key] = (arrays, ref, tol)
    return _DATA[key]


def set_env(monkeypatch, case, **more):
    for k, v in dict(case.env, **more).items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def contract(case, strip_exponent=False, tag=""):
    """``(flags of the pair step, its name, result, slices per launch)`` -- the name is read before anything runs."""
    arrays, _, _ = data(case)
    fn = HipContractor(case.tree(sliced=case.sliced))
    try:
        ex = fn.setup(*arrays)["exec"]
        names = [n for n in ex.step_kernels() if n.startswith("pair_")]
        assert len(names) == 1, names
        print(f"KERNEL {case.id} {'strip ' if strip_exponent else ''}{tag}{names[0]}")
        flags = G.pair_flags_c64(names[0])
        batch = ex.batch
        if strip_exponent:
            m, e = fn(*arrays, strip_exponent=True)
            got = np.asarray(m) * 10.0 ** e
        else:
            got = np.asarray(fn(*arrays))
    finally:
        fn.close()
    return flags, names[0], got, batch


def step_name(case):
    """The name of the row's pair step, from an executor that runs nothing (zero operands of the row's shapes)."""
    fn = HipContractor(case.tree(sliced=case.sliced))
    try:
        ex = fn.setup(*[np.zeros([case.sizes[i] for i in t], dtype=DTYPE) for t in (case.ta, case.tb)])["exec"]
        names = [n for n in ex.step_kernels() if n.startswith("pair_")]
    finally:
        fn.close()
    assert len(names) == 1, names
    return names[0]


def assert_variant(flags, case):
    if case.kernel is None:
        assert flags["kernel"] in (C.C64, C.FAST), flags
    else:
        assert flags["kernel"] == case.kernel, (flags, case.kernel)
    if case.args:
        assert flags["args"] == case.args, (flags, case.args)
    if case.vec is not None:
        assert flags["vec"] is case.vec, (flags, case.vec)
    if flags["splits"] > 1:
        print(f"SPLITS {case.id} {flags['splits']}")
    assert (flags["splits"] > 1) is bool(case.ksplit), (flags, case.ksplit)


def assert_close(got, case):
    _, ref, tol = data(case)
    err = G.relerr(got, ref)
    print(f"ERROR {case.id} {err:.3e} gate {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("case", C.ORDINARY_CASES + [C.KSTREAM_REFUSED], ids=repr)
def test_variant(case, monkeypatch):
    """Every row of the five tables on the instantiation its table records."""
    set_env(monkeypatch, case)
    flags, _, got, _ = contract(case)
    assert_variant(flags, case)
    assert_close(got, case)


@pytest.mark.parametrize("case", C.PIPE16_CASES, ids=repr)
def test_16_bit_pipe(case, monkeypatch):
    """The smallest step the 16-bit pipe takes, in fp16 x 2 (the default), bf16 x 3 and on the fp32 kernel; the same
    gate for all of them."""
    set_env(monkeypatch, case)
    flags, _, got, _ = contract(case)
    assert_variant(flags, case)
    assert_close(got, case)


@pytest.mark.parametrize("case", C.DEEP_CASES, ids=repr)
def test_deep_streaming(case):
    """Every wave owns more tasks than twice the number it keeps in flight: the loop over tasks goes round, the
    register sets rotate, one wave has a group more than the others."""
    flags, _, got, _ = contract(case)
    assert_variant(flags, case)
    assert_close(got, case)


@pytest.mark.parametrize("ident", C.STRIP_IDS)
def test_strip_exponent(ident, monkeypatch):
    """Under strip_exponent a step scales what it stores by 1 / (facA facB) (step_alpha), the reduction of the slabs
    included: mantissa times 10^exponent meets the same gate, on the same kernel."""
    case = C.by_id(ident)
    set_env(monkeypatch, case)
    flags, _, got, _ = contract(case, strip_exponent=True)
    assert_variant(flags, case)
    assert_close(got, case)


@pytest.mark.parametrize("ident", C.SLICE_BATCH_IDS)
def test_slice_batches(ident, monkeypatch):
    """Four slices of the row index through one launch and one by one: the same name as the unsliced row's, the same
    bits, and the numbers of the reference with four times the rows."""
    base = C.by_id(ident)
    case = C.sliced_rows(base)
    set_env(monkeypatch, base)
    outs, names = [], [step_name(base)]
    for cap in ("1", "4"):
        set_env(monkeypatch, case, CTG_SLICE_BATCH=cap)
        flags, name, got, batch = contract(case, tag=f"batch{cap} ")
        assert batch == int(cap)
        assert_variant(flags, case)
        outs.append(got)
        names.append(name)
    assert names[0] == names[1] == names[2], names   # (the split count included)
    assert np.array_equal(outs[0], outs[1])
    assert_close(outs[1], case)


@pytest.mark.parametrize("fast", [False, True], ids=["slow", "fast"])
@pytest.mark.parametrize("ident", C.SPLIT_K_IDS)
def test_part_of_the_contraction_sliced(ident, fast):
    """Half of the contraction sliced.  As the slower part of k the name is the one of the step with half the
    contraction (the row's own: its k-chunks are whole either way); as the fastest index of A every other slice
    starts at an odd element and pairs of A are two elements apart: no 16-byte gathers.  The sum over the slices is
    the unsliced row's result."""
    base = C.by_id(ident)
    cut = C.split_contracted(base, fast)
    cut = base.like(cut.id, cut.eq, cut.sizes, cut.step, sliced=("s",))
    assert cut.ta[-1] == "s" if fast else cut.ta[-1] != "s"
    flags, _, got, _ = contract(cut)
    if fast:
        assert flags["kernel"] in ((C.STREAM,) if base.kernel == C.STREAM else (C.FAST, C.C64)), flags
        vec = flags["args"][1] if base.kernel == C.STREAM else flags["vec"]
        assert vec is False, flags
    else:
        assert_variant(flags, base)
    assert_close(got, cut)
