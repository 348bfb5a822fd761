"""The step forms of the LDS-resident subtree kernel (csrc/ctg_lds_run.hip: lds_run_kernel<T>), one row per form.
Inside one launch every shadow record of a component runs as a load (a plain gather or a gather-and-sum), a pair on
the vector units (run_pair<T, 1 | 2 | 4>) or a complex64 pair on the matrix cores (run_pair_mfma, columns or rows on the
lanes); it is dealt to one wave or shared by the sixteen of the workgroup, and divides its row number by a shift or by
a multiply-high.  csrc/ctg_lds_host.hip: lds_record_form decides all of that for the packer and for the names
``Executor.lds_forms()`` reports (include/ctg_hip.h: ctg_exec_lds_form).

tests/test_lds_variant_plans.py checks on the host that the planner gives every row the components and the records
this table writes down; tests/test_gpu_lds_variants.py reads the forms from the device, asserts them against the
table and compares the numbers with numpy.  The forms are asserted on the device and nowhere computed in Python.

A row is a chain of four to six tensors with a matrix (or a batch of matrices) as its result, so that every element of
every step shows in the output; the planner makes components only for trees of more than three leaves.  Extents are
the smallest that still take the form."""
import numpy as np

import cotengra_amd as ca

DTYPES = ("complex64", "complex128", "float32", "float64")


class Row:
    """``terms -> out`` contracted along ``ssa``; ``recs``: per component the shadow records in the order the
    workgroup walks them, each ``(form in complex64, form in the other three types, (R, K, N, row_lo, phase))`` -- the
    second form None where it is the first.  ``marks``: what the row is in the table for (a reader's index; the test
    that every listed form has a row reads it)."""

    def __init__(self, ident, eq, sizes, ssa, recs, marks=(), sliced=(), seed=0):
        self.id, self.eq, self.sizes, self.ssa = ident, eq, dict(sizes), [tuple(p) for p in ssa]
        self.recs, self.marks, self.sliced, self.seed = recs, tuple(marks), tuple(sliced), seed
        self.terms, self.out = ca.eq_to_inputs_output(eq)

    def tree(self):
        tree = ca.ContractionTree.from_path(self.terms, self.out, self.sizes, ssa_path=self.ssa)
        for ix in self.sliced:
            tree.remove_ind_(ix)
        return tree

    def forms(self, dtype):
        """Per component the expected names, in record order."""
        return [[(c64 if dtype == "complex64" or other is None else other) for c64, other, _ in comp]
                for comp in self.recs]

    def shapes(self):
        return [[shape for _, _, shape in comp] for comp in self.recs]

    @property
    def mfma(self):
        return any(f.startswith("pair_mfma") for comp in self.recs for f, _, _ in comp)

    def arrays(self, dtype, integer=False):
        """Operands seeded by the row: standard normal, or -- ``integer`` -- whole numbers from [-3, 3] in the real
        and the imaginary part (every sum of products of them is exact in every type while it stays below 2^24)."""
        rng = np.random.default_rng(self.seed + (5000 if integer else 0))
        out = []
        for t in self.terms:
            shape = [self.sizes[i] for i in t]
            draw = (lambda: rng.integers(-3, 4, size=shape).astype("float64")) if integer else (
                lambda: rng.standard_normal(shape))
            x = draw()
            y = draw()   # (drawn for the real types as well: one stream of numbers per row)
            out.append((x + 1j * y).astype(dtype) if "complex" in dtype else x.astype(dtype))
        return out

    def __repr__(self):
        return self.id


def int_reference(row, cplx):
    """The row's contraction on its integer operands in int64, pair by pair along its path: ``(result, bound)`` --
    the result as float64 / complex128 (exact), and the largest value of sum |a| |b| over every intermediate and
    the result, with |z| = |Re z| + |Im z|: no partial sum of any step, of its real or imaginary part, in any order
    of the additions and however the sliced index is cut, exceeds it."""
    live = {}
    for i, (t, x) in enumerate(zip(row.terms, row.arrays("complex128", integer=True))):
        re = np.rint(x.real).astype(np.int64)
        im = np.rint(x.imag).astype(np.int64) if cplx else np.zeros_like(re)
        live[i] = ("".join(t), re, im, np.abs(re) + np.abs(im))
    bound, nxt = 0, len(live)
    for i, j in row.ssa:
        (ta, are, aim, ab), (tb, bre, bim, bb) = live.pop(i), live.pop(j)
        rest = set(row.out) | {ix for t, *_ in live.values() for ix in t}
        tc = "".join(ix for ix in dict.fromkeys(ta + tb) if ix in rest)
        eq = f"{ta},{tb}->{tc}"
        re = np.einsum(eq, are, bre) - np.einsum(eq, aim, bim)
        im = np.einsum(eq, are, bim) + np.einsum(eq, aim, bre)
        cb = np.einsum(eq, ab, bb)
        bound = max(bound, int(cb.max()))
        live[nxt] = (tc, re, im, cb)
        nxt += 1
    (tc, re, im, _), = live.values()
    perm = [tc.index(ix) for ix in row.out]
    re, im = re.transpose(perm), im.transpose(perm)
    return (re + 1j * im if cplx else re.astype(np.float64)), bound


def ld(wave, div, R, K=1):
    """A load record: R outputs, each the sum of K elements; always dealt to one wave (LOAD_SHARED below)."""
    return (f"load<{'gather' if K == 1 else 'sum'}> wave={wave} {div}", None, (R, K, 1, R, 0))


def pr(form, other, R, K, N, phase):
    """A pair record.  (In every row the rows are one group of at most 4096: row_lo = R, one high entry -- ROW_HI.)"""
    return (form, other, (R, K, N, R, phase))


CHAIN = [(0, 1), (4, 2), (5, 3)]   # ((t0 t1) t2) t3

# ---------------------------------------------------------------------------------------------------------------- #
# Matrix-core rows (run_pair_mfma<ROWS_ON_LANES>): complex64 only; float32, float64 and complex128 report the VALU form
# of the same record.  A record is on the matrix cores from N >= 8 and R >= 16 when B does not depend on the row;
# rows go on the lanes when the low row table of C is at least as dense as its column table.  A tile is 32 rows x 16
# columns; one tile is dealt to a wave, more are shared ("all rot=R").  k runs in loops of 16, 4 and 1.
# ---------------------------------------------------------------------------------------------------------------- #
MFMA_ROWS = [
    # rows on the lanes, multiply-high division, K = 23 and 21 = 16 + 4 + (3 | 1): the three k loops one after the
    # other, R = 45 and N = 21 | 19 ragged in both tiles, an interior LDS store; s sliced: four slices in one launch
    Row("M_rows_magic", "abs,bcs,cd,de->ae", dict(a=45, b=23, c=21, d=19, e=4, s=4), CHAIN, [[
        ld(0, "magic", 1035), ld(1, "magic", 483), ld(2, "magic", 399), ld(3, "magic", 76),
        pr("pair_mfma<rows> all rot=0 magic", "pair<4> all magic", 45, 23, 21, 1),
        pr("pair_mfma<rows> all rot=0 magic", "pair<4> all magic", 45, 21, 19, 2),
        pr("pair<4> wave=0 magic", None, 45, 19, 4, 3),
    ]], marks=("mfma rows magic interior", "mfma k 16+4+1", "sliced"), sliced=("s",), seed=1),
    # rows on the lanes as the component's root (the 8-byte global store), shift division; two matrix-core records
    # in phase 1, the second starts at wave 2
    Row("M_rows_root", "ba,cb,dc,ed->ea", dict(a=64, b=16, c=32, d=16, e=32), [(2, 3), (0, 1), (5, 4)], [[
        ld(0, "shift", 512), ld(1, "shift", 512), ld(2, "shift", 1024), ld(3, "shift", 512),
        pr("pair_mfma<cols> all rot=0 shift", "pair<4> all shift", 32, 16, 32, 1),
        pr("pair_mfma<rows> all rot=2 shift", "pair<4> all shift", 64, 16, 32, 1),
        pr("pair_mfma<rows> all rot=0 shift", "pair<4> all shift", 64, 32, 32, 2),
    ]], marks=("mfma rows shift root", "mfma cols shift interior", "mfma k 16 exactly"), seed=2),
    # columns on the lanes as root, K = 37 = 2 x 16 + 4 + 1, in two components: multiply-high and shared, shift and dealt
    Row("M_cols_k37", "ab,bc,cd,de->ae", dict(a=48, b=37, c=32, d=37, e=16), [(0, 1), (2, 3), (4, 5)], [[
        ld(0, "magic", 1776), ld(1, "magic", 1184),
        pr("pair_mfma<cols> all rot=0 magic", "pair<4> all magic", 48, 37, 32, 1),
    ], [
        ld(0, "magic", 1184), ld(1, "magic", 592),
        pr("pair_mfma<cols> wave=0 shift", "pair<4> wave=0 shift", 32, 37, 16, 1),
    ]], marks=("mfma cols magic root", "mfma k 16+4+1"), seed=3),
    # 4 x 5 = 20 tiles on 16 waves: the task loop goes round; the root has K = 4, the loop of four alone
    Row("M_tasks", "ab,bc,cd,de->ae", dict(a=98, b=6, c=66, d=4, e=8), CHAIN, [[
        ld(0, "magic", 588), ld(1, "magic", 396), ld(2, "magic", 264), ld(3, "shift", 32),
        pr("pair_mfma<rows> all rot=0 magic", "pair<4> all magic", 98, 6, 66, 1),
        pr("pair<4> wave=0 magic", None, 98, 66, 4, 2),
        pr("pair_mfma<cols> all rot=0 magic", "pair<4> all magic", 98, 4, 8, 3),
    ]], marks=("mfma task loop",), seed=4),
    # two matrix-core records in one phase: the second starts where the first one's 2 x 2 tiles end; K = 17 = 16 + 1
    # (c = f = 17, not more: five tensors of whole numbers up to 3 reach 2^24 at 24)
    Row("M_rot", "ab,bc,de,ef,cf->ad", dict(a=40, d=40, b=9, e=5, c=17, f=17), [(0, 1), (2, 3), (5, 4), (7, 6)], [[
        ld(0, "magic", 200), ld(1, "magic", 85), ld(2, "magic", 360), ld(3, "magic", 153), ld(4, "magic", 289),
        pr("pair_mfma<rows> all rot=0 magic", "pair<4> all magic", 40, 5, 17, 1),
        pr("pair_mfma<rows> all rot=4 magic", "pair<4> all magic", 40, 9, 17, 1),
        pr("pair_mfma<rows> all rot=0 magic", "pair<4> all magic", 40, 17, 17, 2),
        pr("pair_mfma<cols> all rot=0 magic", "pair<4> all magic", 40, 17, 40, 3),
    ]], marks=("mfma rot",), seed=5),
    # one tile of 20 rows x 8 columns dealt to one wave: both axes clamped
    Row("M_one_tile", "ab,bc,cd,de->ae", dict(a=20, b=5, c=8, d=3, e=6), CHAIN, [[
        ld(0, "magic", 100), ld(1, "magic", 40), ld(2, "magic", 24), ld(3, "magic", 18),
        pr("pair_mfma<rows> wave=0 magic", "pair<4> wave=0 magic", 20, 5, 8, 1),
        pr("pair<4> wave=0 magic", None, 20, 8, 3, 2),
        pr("pair<4> wave=0 magic", None, 20, 3, 6, 3),
    ]], marks=("mfma one tile dealt",), seed=6),
    # K = 3 (the loop of one alone), K = 16 exactly, K = 12 (the loop of four alone)
    Row("M_ktails", "ab,bc,cd,de->ae", dict(a=24, b=3, c=16, d=12, e=9), CHAIN, [[
        ld(0, "magic", 72), ld(1, "magic", 48), ld(2, "magic", 192), ld(3, "magic", 108),
        pr("pair_mfma<rows> wave=0 magic", "pair<4> wave=0 magic", 24, 3, 16, 1),
        pr("pair_mfma<rows> wave=0 magic", "pair<4> wave=0 magic", 24, 16, 12, 2),
        pr("pair_mfma<cols> wave=0 magic", "pair<4> wave=0 magic", 24, 12, 9, 3),
    ]], marks=("mfma k < 4", "mfma k 16 exactly"), seed=7),
]

# ---------------------------------------------------------------------------------------------------------------- #
# VALU rows (run_pair<T, TN>): TN = 1, 2 for N = 1, 2 and 4 from N = 3 on (the last column group ragged unless 4 | N);
# four k per pass and a k tail; dealt to one wave up to 128 items of R x ceil(N / TN), shared above.  The same forms
# in all four types.
# ---------------------------------------------------------------------------------------------------------------- #
VALU_ROWS = [
    # a batch index: B depends on the row, which keeps complex64 off the matrix cores at N = 12 and 9
    Row("V_batch", "xab,xbc,xcd,xde->xae", dict(x=3, a=20, b=5, c=12, d=9, e=2), CHAIN, [[
        ld(0, "magic", 300), ld(1, "magic", 180), ld(2, "magic", 324), ld(3, "magic", 54),
        pr("pair<4> all magic", None, 60, 5, 12, 1),
        pr("pair<4> all magic", None, 60, 12, 9, 2),
        pr("pair<2> wave=0 magic", None, 60, 9, 2, 3),
    ]], marks=("batch",), seed=10),
    # pair<1>: K = 3 (tail only), 64 (4 k), 5 (4 k + 1); shared and dealt; both divisions; the root dealt
    Row("V1", "xab,xb,xac,xcd->xd", dict(x=4, a=64, b=3, c=5, d=8), CHAIN, [[
        ld(0, "magic", 768), ld(1, "magic", 12), ld(2, "magic", 1280), ld(3, "magic", 160),
        pr("pair<1> all shift", None, 256, 3, 1, 1),
        pr("pair<1> wave=0 magic", None, 20, 64, 1, 2),
        pr("pair<1> wave=0 shift", None, 32, 5, 1, 3),
    ]], seed=11),
    # pair<1>: shared under the multiply-high division, interior and as root
    Row("V1b", "xab,xb,xac,xcd->xd", dict(x=3, a=50, b=4, c=4, d=50), CHAIN, [[
        ld(0, "magic", 600), ld(1, "magic", 12), ld(2, "magic", 600), ld(3, "magic", 600),
        pr("pair<1> all magic", None, 150, 4, 1, 1),
        pr("pair<1> wave=0 magic", None, 12, 50, 1, 2),
        pr("pair<1> all magic", None, 150, 4, 1, 3),
    ]], seed=12),
    # pair<2>: K = 2 (tail only), 150 (4 k + 2), 4; shared as root
    Row("V2", "ab,bc,cd,de->ae", dict(a=2, b=2, c=150, d=4, e=200), CHAIN, [[
        ld(0, "magic", 300), ld(1, "shift", 4), ld(2, "magic", 600), ld(3, "magic", 800),
        pr("pair<2> all magic", None, 150, 2, 2, 1),
        pr("pair<2> wave=0 shift", None, 4, 150, 2, 2),
        pr("pair<2> all magic", None, 200, 4, 2, 3),
    ]], seed=13),
    # pair<2>: dealt, shift and multiply-high, K = 5, 64, 9; dealt as root
    Row("V2b", "ab,bc,cd,de->ae", dict(a=2, b=5, c=64, d=9, e=24), CHAIN, [[
        ld(0, "magic", 320), ld(1, "magic", 10), ld(2, "magic", 576), ld(3, "magic", 216),
        pr("pair<2> wave=0 shift", None, 64, 5, 2, 1),
        pr("pair<2> wave=0 magic", None, 9, 64, 2, 2),
        pr("pair<2> wave=0 magic", None, 24, 9, 2, 3),
    ]], seed=14),
    # pair<4> with N = 3: one column group with one column missing; K = 6, 40, 8; shared as root
    Row("V4_n3", "ab,bc,cd,de->ae", dict(a=3, b=6, c=40, d=8, e=200), CHAIN, [[
        ld(0, "magic", 240), ld(1, "magic", 18), ld(2, "magic", 320), ld(3, "magic", 1600),
        pr("pair<4> wave=0 magic", None, 40, 6, 3, 1),
        pr("pair<4> wave=0 shift", None, 8, 40, 3, 2),
        pr("pair<4> all magic", None, 200, 8, 3, 3),
    ]], seed=15),
    # N = 5: the second column group holds one column; K = 3 (tail only), 70, 8
    Row("V4_n5", "ab,bc,cd,de->ae", dict(a=5, b=3, c=70, d=8, e=128), CHAIN, [[
        ld(0, "magic", 210), ld(1, "magic", 15), ld(2, "magic", 560), ld(3, "shift", 1024),
        pr("pair<4> all magic", None, 70, 3, 5, 1),
        pr("pair<4> wave=0 shift", None, 8, 70, 5, 2),
        pr("pair<4> all shift", None, 128, 8, 5, 3),
    ]], seed=16),
    # N = 7: the second column group holds three; dealt as root
    Row("V4_n7", "ab,bc,cd,de->ae", dict(a=7, b=9, c=16, d=33, e=18), CHAIN, [[
        ld(0, "magic", 144), ld(1, "magic", 63), ld(2, "magic", 528), ld(3, "magic", 594),
        pr("pair<4> wave=0 shift", None, 16, 9, 7, 1),
        pr("pair<4> wave=0 magic", None, 33, 16, 7, 2),
        pr("pair<4> wave=0 magic", None, 18, 33, 7, 3),
    ]], seed=17),
    # N = 21: six column groups, the last with one column; a batch index keeps complex64 on the vector units
    Row("V4_n21", "xab,xbc,xcd,xde->xae", dict(x=2, a=21, b=3, c=24, d=8, e=32), CHAIN, [[
        ld(0, "magic", 144), ld(1, "magic", 126), ld(2, "magic", 384), ld(3, "shift", 512),
        pr("pair<4> all magic", None, 48, 3, 21, 1),
        pr("pair<4> wave=0 magic", None, 42, 24, 8, 2),
        pr("pair<4> all shift", None, 64, 8, 21, 3),
    ]], marks=("batch",), seed=18),
]

# ---------------------------------------------------------------------------------------------------------------- #
# Loads (run_load): the plain gather (K = 1: four loads in flight per lane, rounds of 256 outputs a wave, the last
# round partial wherever 256 does not divide R -- every row above) and the gather that sums.
# ---------------------------------------------------------------------------------------------------------------- #
LOAD_ROWS = [
    # the diagonal of a leaf summed (a trace): K = 37 along stride 24 x 37 + 24; both divisions
    Row("L_trace", "aab,bc,cd,def->ef", dict(a=37, b=24, c=5, d=6, e=7, f=8), CHAIN, [[
        ld(0, "magic", 120), ld(1, "magic", 24, K=37), ld(2, "magic", 30), ld(3, "magic", 336),
        pr("pair<1> wave=0 magic", None, 5, 24, 1, 1),
        pr("pair<1> wave=0 magic", None, 6, 5, 1, 2),
        pr("pair<1> wave=0 magic", None, 56, 6, 1, 3),
    ]], marks=("load sum trace",), seed=20),
    Row("L_trace_p2", "aab,bc,cd,def->ef", dict(a=37, b=32, c=5, d=6, e=7, f=8), CHAIN, [[
        ld(0, "magic", 160), ld(1, "shift", 32, K=37), ld(2, "magic", 30), ld(3, "magic", 336),
        pr("pair<1> wave=0 magic", None, 5, 32, 1, 1),
        pr("pair<1> wave=0 magic", None, 6, 5, 1, 2),
        pr("pair<1> wave=0 magic", None, 56, 6, 1, 3),
    ]], marks=("load sum trace",), seed=21),
    # an index only the leaf carries, summed: K = 300; both divisions
    Row("L_sum", "zab,bc,cd,de->ae", dict(z=300, a=12, b=8, c=5, d=6, e=7), CHAIN, [[
        ld(0, "magic", 96, K=300), ld(1, "magic", 40), ld(2, "magic", 30), ld(3, "magic", 42),
        pr("pair<4> wave=0 magic", None, 12, 8, 5, 1),
        pr("pair<4> wave=0 magic", None, 12, 5, 6, 2),
        pr("pair<4> wave=0 magic", None, 12, 6, 7, 3),
    ]], marks=("load sum index",), seed=22),
    Row("L_sum_p2", "zab,bc,cd,de->ae", dict(z=300, a=16, b=8, c=5, d=6, e=7), CHAIN, [[
        ld(0, "shift", 128, K=300), ld(1, "magic", 40), ld(2, "magic", 30), ld(3, "magic", 42),
        pr("pair<4> wave=0 shift", None, 16, 8, 5, 1),
        pr("pair<4> wave=0 shift", None, 16, 5, 6, 2),
        pr("pair<4> wave=0 shift", None, 16, 6, 7, 3),
    ]], marks=("load sum index",), seed=23),
]

# ---------------------------------------------------------------------------------------------------------------- #
# An operand a slice group shares (LdsStepDev.gzq > 1): s and g are sliced, g is a group index; the first step does
# not carry g, runs once per group of three slices outside the component, and the component of every slice gathers its
# result from the arena replica of the first slice of its group.
# ---------------------------------------------------------------------------------------------------------------- #
GROUP_ROWS = [
    Row("G_shared", "sab,bc,gcd,de,ef->af", dict(s=2, g=3, a=20, b=7, c=12, d=9, e=5, f=6),
        [(0, 1), (5, 2), (6, 3), (7, 4)], [[
            ld(0, "magic", 240), ld(1, "magic", 108), ld(2, "magic", 45), ld(3, "magic", 30),
            pr("pair_mfma<rows> wave=0 magic", "pair<4> wave=0 magic", 20, 12, 9, 1),
            pr("pair<4> wave=0 magic", None, 20, 9, 5, 2),
            pr("pair<4> wave=0 magic", None, 20, 5, 6, 3),
        ]], marks=("group-shared operand", "sliced"), sliced=("s", "g"), seed=30),
]

ALL_ROWS = MFMA_ROWS + VALU_ROWS + LOAD_ROWS + GROUP_ROWS


def by_id(ident):
    return next(r for r in ALL_ROWS if r.id == ident)


# ---------------------------------------------------------------------------------------------------------------- #
# Branches of the kernel and the packer that no plan reaches (tests/test_lds_variant_plans.py checks the arithmetic
# of each reason against the planner's constants).
# ---------------------------------------------------------------------------------------------------------------- #
UNREACHABLE = {
    # run_step with kind == 0 and wave == -1 (run_load with n_lanes = 1024, its four-way unrolled gather with a partial
    # last round there): the packer shares a load only above 4096 outputs, and the planner charges a component's
    # table budget (ldsrun.LDS_TABLE_BYTES = 32 KiB) two 4-byte words per element of every tensor it loads -- a load
    # of 4096 elements alone is the whole budget.  Every load is dealt to one wave.
    "LOAD_SHARED": "load<...> all: a load of more than 4096 outputs exceeds the component's 32 KiB table budget",
    # rhi[hi] with hi > 0, in loads and pairs: a record's rows are cut in two levels only above plan.LO_MAX = 4096
    # rows, and 4096 rows are 3 x 4096 table words (pairs) or 2 x 4096 (loads), again more than the budget.
    "ROW_HI": "a row table with more than one high entry: needs more than 4096 rows, more than the table budget",
    # ctg_lds_build's `R >= 65536` under the multiply-high division (exact only below 2^16): follows from ROW_HI.
    "MAGIC_R_65536": "R >= 65536 under the multiply-high division: R stays below 4096",
}

# ---------------------------------------------------------------------------------------------------------------- #
# Two-level rows.  The planner never cuts the rows of a shadow record in two (UNREACHABLE["ROW_HI"]), so in every plan
# the quotient of the row division is zero: neither `rhi[hi]` with hi > 0 nor a multiply-high that has to produce
# anything but zero ever runs.  The C ABI takes such records, though (ctg_lds_validate asks only that
# row_lo x row_hi = R), and the kernel has the code; RECUT_IDS run it: the rows of every record of these rows' plans
# are re-cut as R = (R / d) x d after the fact, for the smallest divisor d > 1 of either kind -- a power of two and
# not one -- under which every row table stays a sum of a high and a low entry.
# ---------------------------------------------------------------------------------------------------------------- #
RECUT_IDS = ["M_rows_magic", "M_rows_root", "M_cols_k37", "M_tasks", "V_batch", "V1", "V2", "V4_n21", "L_trace", "L_sum_p2"]


class RecutPlan:
    """``plan`` with other words in its serialised form (what comes through the C ABI is data, not a Plan)."""

    def __init__(self, plan, ser):
        self._plan, self._ser = plan, ser

    def serialise(self):
        return self._ser

    def __getattr__(self, name):
        return getattr(self._plan, name)


def recut_rows(plan, magic):
    """``(RecutPlan, per component the new row_lo of every record)``: every shadow record's rows as two levels with a
    low table of ``d`` entries, d the smallest divisor of R with 1 < d < R that is (``magic``) no power of two / is one
    and keeps every operand's offsets what they were; a record without such a divisor stays as it is."""
    from cotengra_amd import ldsrun as L
    from cotengra_amd import plan as P

    ser = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in plan.serialise().items()}
    steps = ser["steps"].reshape(-1, P.STEP_WORDS)
    tables = [int(x) for x in ser["tables"]]
    descs = sorted({int(s[P.W_LDS_DESC]) for s in steps if s[P.W_LDS_COMP] > 0})
    cuts = []
    for d0 in descs:
        cuts.append([])
        for i in range(tables[d0 + 1]):
            q = d0 + L.LR_HEAD_WORDS + i * L.LR_WORDS
            R, row_lo, hi_len = tables[q + 10], tables[q + 13], tables[q + 14]
            assert row_lo == R and hi_len == 1
            ops = [(w_hi, w_lo) for w_hi, w_lo in ((17, 18), (19, 20), (21, 22)) if tables[q + w_lo] >= 0]
            old = {w: (tables[tables[q + w[0]]], tables[tables[q + w[1]]: tables[q + w[1]] + R]) for w in ops}

            def fits(d):
                return all(t[j * d + k] - t[j * d] == t[k] - t[0] and t[k] >= t[0]
                           for _, t in old.values() for j in range(R // d) for k in range(d))

            d = next((d for d in range(2, R) if R % d == 0 and bool(d & (d - 1)) == magic and fits(d)), None)
            cuts[-1].append(d or row_lo)
            if d is None:
                continue
            tables[q + 13], tables[q + 14] = d, R // d
            for w, (h0, t) in old.items():
                tables[q + w[0]] = len(tables)
                tables += [h0 + t[j * d] for j in range(R // d)]
                tables[q + w[1]] = len(tables)
                tables += [t[k] - t[0] for k in range(d)]
    ser["tables"] = np.array(tables, dtype=np.int64)
    return RecutPlan(plan, ser), cuts




