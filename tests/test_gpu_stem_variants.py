"""Every instantiation of the fused stem kernel (csrc/ctg_stem_impl.h: launch_stem), by name and by value.

The rows of tests/stem_variant_cases.py -- the 47 static pairs with fp32 products, the 38 geometries in bf16 x 3 and in
fp16 x 2 (the specialised-wave ones again in the symmetric form), the 10 static single steps in the three arithmetics
and the run-time-count variants -- each run as one small stem on one contractor, with three checks:

name     exactly one step runs a stem kernel, and every template argument the executor names is the one the header's
         rules give for the row (stem_variant_cases.expected): a case that drifts to another instantiation fails;
random   complex64 data of make_arrays_from_inputs against the complex128 oracle under the suite's single-precision gate;
integer  every input -- the state, the (3, 3) gate, the small operands -- has real and imaginary parts in {-1, 0, 1},
         and the device must return the oracle's integers BIT FOR BIT in all three arithmetics.  Why that is owed: a
         component of a product of two such numbers is at most 2 in magnitude, so a component is at most 8 x 2 = 16
         after the first gate (K = 8), at most 128 x 2 x 16 = 2^12 after step 1 (K1 <= 128) and at most 128 x 2 x 2^12
         = 2^20 after step 2 (asserted below from the oracle's results of the chain's prefixes, together with a result
         that is not all zero).  Every partial sum is an integer below 2^24 times a power of two, so every fp32 sum is
         exact in any order.  The 16-bit arithmetics split operands into limbs of 11 (fp16) or 8 (bf16) significant bits
         under power-of-two scales: the small operands (<= 1) and the big operand (<= 16) fit one limb; the
         intermediate (13 bits) fits two fp16 limbs or two bf16 limbs, and meets a one-limb B2 -- the only product
         fp16 x 2 leaves out, second limb x second limb, is zero.  So no rounding happens anywhere, in any form, and
         what differs from the oracle is a missing chunk, a wrong item or column group, a stale LDS plane, a wrong
         limb pairing or a lost store -- most of which the 1e-5 gate cannot see (a dropped limb product is 2^-22).
         What this data cannot see either: the planes of the second and third limbs of B1, B2 and the state hold
         zeros, so a product that pairs them wrongly reads zeros where zeros are expected.  Operands with every limb
         populated, still bit for bit: tests/test_gpu_limb_probes.py.

Running tensors of 2^15 to 2^18 elements: fewer than 256 tiles, one pass of every workgroup's loop.  The deep rows run
512 and 1024 tiles (two and four per workgroup: the steady state, asserted from the plan) for the loop structures that
tests/test_gpu_stem_mempath.py and tests/test_gpu_stem_shared_rows.py do not run -- integer data only.  The sliced rows
slice one index of the first tensor: every slice against the oracle's slice, the sum bit for bit on integer data."""
from collections import OrderedDict

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd.contractor import HipContractor
from cotengra_amd.plan import KIND_STEM2
from oracle import contract_ref as orc

import golden_util as G
import stem_variant_cases as V
from test_gpu_stem_valu_paths import stem_env  # noqa: F401  (the fixture: every capable step on the stem kernels)

pytestmark = pytest.mark.gpu

# largest |component| the argument above allows: behind the first gate, behind step 1, behind step 2
BOUNDS = (16, 1 << 12, 1 << 20)


def top_of(x):
    x = np.asarray(x)
    return float(max(np.abs(x.real).max(), np.abs(x.imag).max()))


def integer_arrays(tree, seed):
    rng = np.random.default_rng(seed)
    out = []
    for t in tree.inputs:
        shape = tuple(tree.size_dict[ix] for ix in t)
        out.append((rng.integers(-1, 2, size=shape) + 1j * rng.integers(-1, 2, size=shape)).astype("complex64"))
    return out


def integer_reference(row, tree, arrays):
    """The oracle's result of the integer data as complex64 (exact: asserted), after checking on the host that every
    intermediate of every slice stays inside BOUNDS and that the result is not all zero."""
    a128 = [a.astype("complex128") for a in arrays]
    n = len(arrays)
    for upto, bound in zip(range(2, n + 1), BOUNDS):
        prefix = row.tree(upto=upto - 1)   # (the state and the first upto - 1 gates)
        assert prefix.inputs == tree.inputs[:upto]
        for i in range(prefix.nslices):
            part = np.asarray(orc.contract_slice(prefix, a128[:upto], i))
            assert top_of(part) <= bound, (row.id, upto, top_of(part))
    ref = np.asarray(orc.contract(tree, a128))
    assert top_of(ref) * tree.nslices < 1 << 24 and np.count_nonzero(ref) > ref.size // 2, row.id
    assert np.array_equal(ref, np.round(ref.real) + 1j * np.round(ref.imag))
    ref64 = ref.astype("complex64")
    assert np.array_equal(ref64.astype("complex128"), ref)
    return ref64


_DATA = OrderedDict()


def data_of(row, random=True):
    """(tree, random arrays, complex128 reference, numpy's complex64 result, integer arrays, integer reference): computed
    once per network (rows of one network follow each other), never modified."""
    key = row.network
    if key not in _DATA:
        tree = row.tree()
        arrays = ref = np64 = None
        if random:
            arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=7, dtype="complex64")
            ref = np.asarray(orc.contract(tree, [a.astype("complex128") for a in arrays]))
            np64 = np.asarray(orc.contract(tree, arrays))
        ints = integer_arrays(tree, 11 + row.seed)
        iref = integer_reference(row, tree, ints)
        for x in (arrays or []) + ints + [iref]:
            x.setflags(write=False)
        _DATA[key] = (tree, arrays, ref, np64, ints, iref)
        while len(_DATA) > 4:
            _DATA.popitem(last=False)
    return _DATA[key]


def set_env(monkeypatch, row):
    for k in ("CTG_STEM_FORM", "CTG_STEM_GENERIC", "CTG_STEM_NO_RI2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)


def contractor(tree, arith):
    return HipContractor(tree, fuse=True, fuse_min_elems=1 << 10, stem_bf16x3=arith)


def stem_names(fn, arrays):
    return [n for n in fn.setup(*arrays)["exec"].step_kernels() if n.startswith(("stem2_kernel", "stem2h_kernel"))]


def assert_named(row, arith, names):
    """Exactly one stem step, on the kernel and with the template arguments the header's rules give the row."""
    assert len(names) == 1, names
    kernel, flags = V.expected(row, arith)
    print(row.id, arith, names[0])
    assert names[0].split("<")[0] == kernel, (names, kernel)
    got = G.stem_flags(names[0])
    assert got == flags, (names, {k: (got[k], flags[k]) for k in flags if got[k] != flags[k]})


def assert_exact(row, what, got, want):
    got = np.asarray(got)
    assert got.shape == want.shape
    bad = int(np.count_nonzero(got != want))
    print(row.id, what, "elements that differ", bad, "of", got.size)
    assert bad == 0 and np.array_equal(got, want), (row.id, what, bad, float(np.abs(got - want).max()))


@pytest.mark.parametrize("row,arith", V.DEVICE_CASES, ids=[f"{r.id}-{a}" for r, a in V.DEVICE_CASES])
def test_stem_instantiation(row, arith, stem_env, monkeypatch):
    tree, arrays, ref, np64, ints, iref = data_of(row)
    set_env(monkeypatch, row)
    fn = contractor(tree, arith)
    try:
        got = np.asarray(fn(*arrays))
        names = stem_names(fn, arrays)
        exact = np.asarray(fn(*ints))
        names_i = stem_names(fn, ints)
    finally:
        fn.close()
    assert_named(row, arith, names)
    assert names_i == names
    err, gate = G.relerr(got, ref), G.single_gate(ref, np64)
    print(row.id, arith, "relerr", err, "gate", gate)
    assert err <= gate, (err, gate)
    assert_exact(row, arith, exact, iref)


@pytest.mark.parametrize("row", V.DEEP_ROWS, ids=repr)
def test_more_than_one_tile_per_workgroup(row, stem_env, monkeypatch):
    tree, _, _, _, ints, iref = data_of(row, random=False)
    set_env(monkeypatch, row)
    fn = contractor(tree, row.arith)
    try:
        exact = np.asarray(fn(*ints))
        names = stem_names(fn, ints)
        tiles = [s.stem["n_tiles"] for s in fn.setup(*ints)["plan"].steps if s.kind == KIND_STEM2]
    finally:
        fn.close()
    assert_named(row, row.arith, names)
    assert tiles == [row.tiles], tiles
    assert_exact(row, row.arith, exact, iref)


@pytest.mark.parametrize("row", V.SLICED_ROWS, ids=repr)
def test_one_index_of_the_first_tensor_sliced(row, stem_env, monkeypatch):
    tree, arrays, ref, np64, ints, iref = data_of(row)
    assert tree.nslices == 2
    set_env(monkeypatch, row)
    fn = contractor(tree, row.arith)
    try:
        parts = [np.asarray(fn.contract_slice(arrays, i)) for i in range(2)]
        names = stem_names(fn, arrays)
        exact = np.asarray(fn(*ints))
    finally:
        fn.close()
    assert_named(row, row.arith, names)
    a128 = [a.astype("complex128") for a in arrays]
    for i, part in enumerate(parts):
        want = np.asarray(orc.contract_slice(tree, a128, i))
        err, gate = G.relerr(part, want), G.single_gate(want, np.asarray(orc.contract_slice(tree, arrays, i)))
        print(row.id, row.arith, "slice", i, "relerr", err, "gate", gate)
        assert err <= gate, (i, err, gate)
    assert_exact(row, row.arith + " sum of the slices", exact, iref)
