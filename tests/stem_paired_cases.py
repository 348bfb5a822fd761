"""Cases and rules of the paired stores of the stem kernels (csrc/ctg_stem_impl.h: stem2h_kernel_p16), shared by
tests/test_stem_paired_stores_host.py (no device) and tests/test_gpu_stem_paired_stores.py.

A case is a small stem of tests/golden_util.py: stem_network -- ``[(3, 3)] + gates`` applied to a tensor of ``nq``
binary indices, planned with the pairing model opened up as tests/stem_variant_cases.py plans its rows -- with what
its stem steps must be: their shapes ``(K1, N1, K2, N2)``, their tile counts, whether the result's TABLES allow
16-byte stores (``tables_ok``) and whether the launch PAIRS (``paired``: the tables allow it and the kernel is one whose
consumers hold both column groups of a row tile).  A gate behind the pair (the ``_tail`` cases, ``chain``) makes the
pair's result an intermediate, which the planner lays out ``[rows][N2]``; the result of a tree's last step is laid
out as the caller asked, which scatters the columns of ``scattered``.

The two rules, restated from the C side:

tables_allow    csrc/ctg_runtime.hip: stem_pair16_ok -- columns 2 j, 2 j + 1 of the result exactly one element apart,
                column 2 j even, every row and tile offset even, the result's place in its space even, the arena's
                size even (the replicas of a slice batch) and every slice stride of the result even.
kernel_pairs    csrc/ctg_stem_impl.h: stem_pair16_shape with form 3 of the fp16 x 2 arithmetic (tests/
                stem_variant_cases.py: form_of) -- four row tiles of 64 columns, K2 = 64: a specialised-wave consumer's
                two items are the two column groups of one row tile (item2k, four chunks).  It is the only shape that
                reaches item2k: a tile of such a kernel has rows2 x K2 = 8192 elements.  The symmetric kernels with two
                items per wave (the ``_sym`` cases) pair in an experiment build only (-DCTG_STEM_PAIR16_SYM: they
                spill for it, profiles/stem_paired_stores.txt section 8); the product keeps them on 8-byte stores.
"""
import numpy as np

from cotengra_amd.plan import SPACE_ARENA
from cotengra_amd.stem import TAB_ORDER   # noqa: F401  (order of the 14 table offsets of a descriptor)

import stem_variant_cases as V

# words of a step record and of a stem descriptor (csrc/ctg_common.h: StepWord, StemWord)
STEP_WORDS, W_C_SPACE, W_C_OFF, W_C_LEAF, W_STEM = 48, 8, 9, 10, 43
SW_N2, SW_ROWS2, SW_NTILES, SW_GLO, SW_ONE, SW_TABS, SW_TRI = 4, 6, 8, 9, 18, 20, 39


class Case:
    def __init__(self, ident, nq, gates, seed, shapes, tiles, tables_ok, paired, sliced=0):
        self.id, self.nq, self.gates, self.seed, self.sliced = ident, nq, [tuple(g) for g in gates], seed, sliced
        self.shapes, self.tiles, self.tables_ok, self.paired = list(shapes), list(tiles), list(tables_ok), list(paired)

    def __repr__(self):
        return self.id

    @property
    def network(self):
        return (self.nq, tuple(self.gates), self.seed, self.sliced)

    def tree(self, upto=None):
        import golden_util as G
        return G.stem_network(self.nq, ([(3, 3)] + self.gates)[:upto], self.seed, sliced=self.sliced)


T, F = True, False
CASES = [
    # the three shapes of the headline's k64 n64 second steps (item2k, four chunks)
    Case("k32n32_k64n64", 15, [(5, 5), (6, 6)], 0, [(32, 32, 64, 64)], [4], [T], [T]),
    Case("k32n64_k64n64", 15, [(5, 6), (6, 6)], 0, [(32, 64, 64, 64)], [8], [T], [T]),       # CS1 = 2 producers
    Case("k64n32_k64n64", 15, [(6, 5), (6, 6)], 0, [(64, 32, 64, 64)], [2], [T], [T]),
    Case("k32n32_k64n64_tail", 15, [(5, 5), (6, 6), (3, 3)], 0, [(32, 32, 64, 64)], [4], [T], [T]),
    # two items of 32 columns per wave: the symmetric kernels, which keep 8-byte stores whatever the tables say
    Case("k32n32_k32n64_sym", 15, [(5, 5), (5, 6), (3, 3)], 0, [(32, 32, 32, 64)], [4], [T], [F]),
    Case("k32n32_k64n128_sym", 15, [(5, 5), (6, 7)], 0, [(32, 32, 64, 128)], [4], [T], [F]),
    # two tiles per workgroup (a launch has min(tiles, 256) workgroups; tile counts are powers of two, so a grid always
    # divides them: what can be run is the steady state and the last tile of a workgroup's loop)
    Case("deep512", 22, [(5, 5), (6, 6), (3, 3)], 0, [(32, 32, 64, 64)], [512], [T], [T]),
    # one index of the first tensor sliced: slice offsets
    Case("sliced", 16, [(5, 5), (6, 6)], 2, [(32, 32, 64, 64)], [4], [T], [T], sliced=1),
    # the tree's result written by the pair itself, in the caller's order: paired columns not adjacent
    Case("scattered", 15, [(5, 5), (6, 6)], 1, [(32, 32, 64, 64)], [4], [F], [F]),
    # two pairs in a row: the second one splits its big operand by the maximum the first one recorded
    Case("chain", 15, [(5, 5), (6, 6), (5, 5), (6, 6), (3, 3)], 0, [(32, 32, 64, 64), (32, 32, 64, 64)], [4, 4], [T, T], [T, T]),
]


def by_id(ident):
    return next(c for c in CASES if c.id == ident)


def _rule(N2, out_col, out_row, gc_hi, gc_lo, c_space, c_off, arena_elems, leaf_strides):
    oc = np.asarray(out_col, dtype=np.int64)
    if N2 < 2 or N2 % 2:
        return False
    if not all(oc[j] % 2 == 0 and oc[j + 1] == oc[j] + 1 for j in range(0, N2, 2)):
        return False
    if any((np.asarray(t, dtype=np.int64) % 2 != 0).any() for t in (out_row, gc_hi, gc_lo)):
        return False
    if c_off % 2 or (c_space == SPACE_ARENA and arena_elems % 2):
        return False
    return all(int(s) % 2 == 0 for s in leaf_strides)


def tables_allow(plan, step):
    """The rule on a plan's step (``step.stem`` as cotengra_amd/stem.py builds it)."""
    st = step.stem
    if st.get("one") or st.get("tri"):
        return False
    t = st["tabs"]
    strides = [] if step.c.leaf < 0 else np.asarray(plan.slice_strides).reshape(-1, len(plan.slice_sizes))[step.c.leaf]
    return _rule(st["N2"], t["out_col"], t["out_row"], t["gC_hi"], t["gC_lo"], step.c.space, step.c.offset,
                 plan.arena_elems, strides)


def serial_allows(s, step):
    """The same rule on a serialised plan (what crosses the C ABI): ``s`` of Plan.serialise, step number ``step``."""
    r = np.asarray(s["steps"]).reshape(-1, STEP_WORDS)[step]
    t = np.asarray(s["tables"])
    h = int(r[W_STEM])
    if t[h + SW_ONE] == 1 or t[h + SW_TRI] == 1:
        return False
    N2, rows2, n_tiles, g_lo = (int(t[h + w]) for w in (SW_N2, SW_ROWS2, SW_NTILES, SW_GLO))

    def tab(name, n):
        o = int(t[h + SW_TABS + TAB_ORDER.index(name)])
        return t[o:o + n]

    n_sl = len(s["slice_sizes"])
    strides = [] if r[W_C_LEAF] < 0 else np.asarray(s["slice_strides"]).reshape(-1, n_sl)[int(r[W_C_LEAF])]
    return _rule(N2, tab("out_col", N2), tab("out_row", rows2), tab("gC_hi", n_tiles // g_lo), tab("gC_lo", g_lo),
                 int(r[W_C_SPACE]), int(r[W_C_OFF]), int(s["arena_elems"]), strides)


def kernel_pairs(st):
    """Does the fp16 x 2 launch of a pair with stem record ``st`` run a kernel that pairs (given tables that allow it)?"""
    if st.get("one") or st.get("tri"):
        return False
    rec = dict(K1=st["K1"], N1=st["N1"], K2=st["K2"], N2=st["N2"], nr1=st["nr1"], items=st["items"], ng2=st["ng2"],
               vec=int(st["vec"]), one=0, rows2=st["rows2"], ld2=st["ld2"])
    if not V.has_16bit(rec):
        return False
    if V.form_of("fp16x2", V.geo_of(V.stem_shape(rec))) != 3:
        return False
    n_rt2 = st["rows2"] // 32
    return n_rt2 == V.SW // 2 and st["ng2"] == 2 and st["N2"] == 64 and st["K2"] == 64
