"""GPU suite: every step form of the LDS-resident subtree kernel (csrc/ctg_lds_run.hip: lds_run_kernel<T>) -- loads that
gather and loads that sum, VALU pairs on one, two and four columns per lane, complex64 pairs on the matrix cores with
columns or rows on the lanes, dealt to one wave or shared by sixteen, with either row division, as interior steps
and as a component's root.

Every case first reads the forms from an executor that has run nothing (``Executor.lds_forms()``: what
csrc/ctg_lds_host.hip's lds_record_form decided for the packer) and asserts them against its row of
tests/lds_variant_cases.py; then it compares the result with ``numpy.einsum`` in double precision on random operands
(``G.single_gate`` in single precision, 1e-10 in double) and -- the check without a tolerance -- BIT FOR BIT on
operands of whole numbers from [-3, 3], whose partial sums all stay below 2^24 (tests/test_lds_variant_plans.py): one
wrong row offset, one dropped k, a swapped Re / Im register changes an integer.  Last the kernel's own contract: with
CTG_NO_LDS_RUNS=1 no step is the kernel's, a component gives the bits of its steps launched one by one on the
thread-per-output kernels, and with CTG_LDS_NO_MFMA=1 a matrix-core record takes its VALU form and those bits.
profiles/lds_variants.txt records what ran."""
import numpy as np
import pytest

import golden_util as G
import lds_variant_cases as V
from cotengra_amd.contractor import HipContractor

pytestmark = pytest.mark.gpu

WIDE = {"complex64": "complex128", "complex128": "complex128", "float32": "float64", "float64": "float64"}
SWITCHES = ("CTG_NO_LDS_RUNS", "CTG_LDS_NO_MFMA", "CTG_LDS_RUNS", "CTG_SLICE_BATCH")
_DATA = {}


def data(row, dtype):
    """``(operands, reference, gate, integer operands, integer reference)`` of a row in a type, computed once: the
    references are numpy's einsum in double precision and the int64 contraction; they are never written again."""
    key = (row.id, dtype)
    if key not in _DATA:
        while len(_DATA) >= 4:
            _DATA.pop(next(iter(_DATA)))
        arrays = row.arrays(dtype)
        # (the reference is of the operands the device gets: in single precision, of the rounded ones)
        ref = np.einsum(row.eq, *[x.astype(WIDE[dtype]) for x in arrays], optimize=True)
        gate = G.single_gate(ref, np.einsum(row.eq, *arrays, optimize=True)) if dtype != WIDE[dtype] else 1e-10
        ints = row.arrays(dtype, integer=True)
        iref, bound = V.int_reference(row, "complex" in dtype)
        assert bound < 2 ** 24
        iref = iref.astype(dtype)
        ref.setflags(write=False)
        iref.setflags(write=False)
        _DATA[key] = (arrays, ref, gate, ints, iref)
    return _DATA[key]


class Run:
    """A contractor of the row under ``env``, its executor's names and forms read before anything runs."""

    def __init__(self, row, dtype, monkeypatch, tag="", **env):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.row, self.dtype = row, dtype
        self.fn = HipContractor(row.tree())
        st = self.fn.setup(*data(row, dtype)[0])
        self.ex, self.plan = st["exec"], st["plan"]
        self.kernels = self.ex.step_kernels()
        self.forms = self.ex.lds_forms()
        self.batch = self.ex.batch
        for c, recs in enumerate(self.forms):
            for name, main in recs:
                print(f"KERNEL {row.id} {dtype} {tag}lds_run_kernel[{c}] step {main}: {name}")

    def __call__(self, arrays):
        return np.asarray(self.fn(*arrays))

    def slices(self, arrays, ids):
        ex = self.fn.setup(*arrays)["exec"]
        ex.zero_result()
        ex.run_slice_list(list(ids))
        return np.asarray(ex.download_result()).copy()

    def close(self):
        self.fn.close()


def assert_forms(run, names):
    """The device's report against the table: per packed component the names in record order, every record's step a
    member that step_kernels() gives to that component, every member with at least one record."""
    assert [[n for n, _ in recs] for recs in run.forms] == names, (run.forms, names)
    for c, recs in enumerate(run.forms):
        for name, main in recs:
            G.lds_form(name)
            assert run.kernels[main] == f"lds_run_kernel[{c}]", (c, name, main, run.kernels)
        members = {i for i, k in enumerate(run.kernels) if k == f"lds_run_kernel[{c}]"}
        assert members == {main for _, main in recs}, (members, recs)


def assert_close(got, row, dtype, tag=""):
    _, ref, gate, _, _ = data(row, dtype)
    err = G.relerr(got, ref)
    print(f"ERROR {row.id} {dtype} {tag}{err:.3e} gate {gate:.3e}")
    assert err <= gate, (err, gate)


def assert_exact(got, row, dtype, tag=""):
    iref = data(row, dtype)[4]
    assert got.dtype == iref.dtype and got.shape == iref.shape
    wrong = int(np.count_nonzero(got != iref))
    print(f"EXACT {row.id} {dtype} {tag}{wrong} of {iref.size} differ")
    assert np.array_equal(got, iref), (wrong, np.argwhere(got != iref)[:8].tolist())


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("row", V.ALL_ROWS, ids=repr)
def test_form(row, dtype, monkeypatch):
    arrays, _, _, ints, _ = data(row, dtype)
    on_cores = row.mfma and dtype == "complex64"
    # 1. the forms, before anything runs
    run = Run(row, dtype, monkeypatch)
    try:
        assert_forms(run, row.forms(dtype))
        assert any(f.startswith("pair_mfma") for recs in run.forms for f, _ in recs) == on_cores
        if row.sliced:
            assert run.batch > 1, run.batch
        # 2. random operands against numpy; 3. whole numbers, bit for bit
        got = run(arrays)
        assert_close(got, row, dtype)
        assert_exact(run(ints), row, dtype)
        members = [i for i, k in enumerate(run.kernels) if k.startswith("lds_run_kernel")]
        # 5. the sliced row: the slices in another order
        if row.sliced:
            n = run.plan.nslices
            order = [i for i in range(n) if i % 2 == 0][::-1] + [i for i in range(n) if i % 2]   # 2 0 1 3 | 4 2 0 1 3 5
            assert_close(run.slices(arrays, order), row, dtype, "slices reordered ")
            assert_exact(run.slices(ints, order), row, dtype, "slices reordered ")
    finally:
        run.close()
    # 4. the kernel's contract: the ordinary steps, and -- matrix-core records -- the VALU form of the same component
    old = Run(row, dtype, monkeypatch, tag="steps ", CTG_NO_LDS_RUNS="1")
    try:
        assert old.forms == [] and not any(k.startswith("lds_run_kernel") for k in old.kernels), old.kernels
        for i in members:
            print(f"KERNEL {row.id} {dtype} steps step {i}: {old.kernels[i]}")
        same_order = all(old.kernels[i] in ("pair_valu_kernel", "single_kernel") and old.plan.steps[i].K < 256
                         for i in members)
        step_path = old(arrays)
        assert_close(step_path, row, dtype, "steps ")
        assert_exact(old(ints), row, dtype, "steps ")
    finally:
        old.close()
    if on_cores:
        plain = Run(row, dtype, monkeypatch, tag="no_mfma ", CTG_LDS_NO_MFMA="1")
        try:
            assert_forms(plain, row.forms("float32"))
            vector = plain(arrays)
            assert_exact(plain(ints), row, dtype, "no_mfma ")
        finally:
            plain.close()
        assert_close(vector, row, dtype, "no_mfma ")
    else:
        vector = got
    print(f"SAME_ORDER {row.id} {dtype} {same_order}")
    if same_order:
        assert np.array_equal(vector, step_path), int(np.count_nonzero(vector != step_path))


@pytest.mark.parametrize("magic", [False, True], ids=["shift", "magic"])
@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("ident", V.RECUT_IDS)
def test_two_level_rows_through_the_c_abi(ident, dtype, magic, monkeypatch):
    """No plan cuts a record's rows in two (lds_variant_cases.UNREACHABLE), so above the quotient of the row division
    is always zero.  Here the rows of every record are re-cut as (R / d) x d after the fact (recut_rows: d the smallest
    divisor that is / is not a power of two), which the C ABI accepts: the high row table has R / d entries and both
    divisions produce every quotient up to R / d - 1.  The forms are the row's own but for the division; the numbers
    against numpy, and bit for bit on whole numbers."""
    from cotengra_amd import plan as P, runtime

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    row = V.by_id(ident)
    arrays, _, _, ints, _ = data(row, dtype)
    recut, cuts = V.recut_rows(P.compile_tree(row.tree(), dtype), magic)
    want = [[" ".join(n.split(" ")[:-1] + ["magic" if d & (d - 1) else "shift"]) for n, d in zip(names, ds)]
            for names, ds in zip(row.forms(dtype), cuts)]
    dplan = runtime.DevicePlan(recut)
    ex = runtime.Executor(dplan)
    try:
        forms = ex.lds_forms()
        for c, recs in enumerate(forms):
            for (name, main), d in zip(recs, cuts[c]):
                print(f"KERNEL {row.id} {dtype} recut row_lo={d} lds_run_kernel[{c}] step {main}: {name}")
        assert [[n for n, _ in recs] for recs in forms] == want, (forms, want)
        outs = []
        for xs in (arrays, ints):
            ex.upload_host(xs)
            ex.zero_result()
            ex.run_slices()
            outs.append(np.asarray(ex.download_result()).copy())
    finally:
        ex.close()
        dplan.close()
    tag = f"recut {'magic' if magic else 'shift'} "
    assert_close(outs[0], row, dtype, tag)
    assert_exact(outs[1], row, dtype, tag)
