"""What every word of a plan descriptor is, written down once: the contract ``ctg_plan_create`` validates
(include/ctg_hip.h, "Words of a step record"; csrc/ctg_runtime.hip: validate_plan / validate_stem / step_tables;
csrc/ctg_lds_host.hip: ctg_lds_validate).  tests/test_plan_validation.py derives every hostile value from this map and
tests/cabi_validate_fuzz.cpp replays them, so a word that is missing here is a word nobody attacks:
``test_the_map_covers_every_word`` holds the four maps to the library's own record lengths.

A word is a ``W(name, cls, ...)``:

  ENUM    a code; ``lo`` / ``hi`` its range (``exact``: it must keep its value -- a magic number, a component's id)
  SPACE   which buffer an operand lives in (0 inputs, 1 arena, 2 result)
  LEAF    the input whose slice offset moves the operand (-1 none; n_inputs: the result's chunk offset)
  OFFSET  element offset of an operand in its space           SIZE  its elements: [offset, offset + size) inside the space
  EXTENT  a loop extent or one half of a two-level split (``split``: with its partner it multiplies to another word)
  TABLE   word offset of an offset table in the blob; ``op`` the operand whose address it enters, ``length`` the word(s)
          whose value (product) is its length, ``reads`` who reads it (see ``table_is_read``)
  STEP    a step index: ``strict`` -- it must name a member step --, else a producer word, where anything outside
          [0, n_steps) means "no producer" and is tolerated by design
  DESC    word offset of a descriptor in the blob (``length`` words), read when ``when`` says so
  FREE    read by nothing: bookkeeping (macs, elems_rw, node, lds_bytes, phases) and reserved words

An operand a record does not have (B of a single-term or an accumulate step, B of a load record, B2 of a single stem
step) is written in one way only -- space -1 (0 in the two descriptors), offset 0, leaf -1, size 0 -- and the words of a
stage a stem descriptor does not have are zeros: every other value is refused.
"""
from collections import namedtuple

from cotengra_amd import ldsrun, plan as P, stem

ENUM, SPACE, LEAF, OFFSET, SIZE, EXTENT, TABLE, STEP, DESC, FREE = (
    "enum", "space", "leaf", "offset", "size", "extent", "table", "step", "desc", "free")
CLASSES = (ENUM, SPACE, LEAF, OFFSET, SIZE, EXTENT, TABLE, STEP, DESC, FREE)

_W = namedtuple("W", "name cls lo hi exact op length reads split strict when")


def W(name, cls, lo=None, hi=None, exact=False, op=None, length=None, reads=None, split=None, strict=False, when=None):
    assert cls in CLASSES
    return _W(name, cls, lo, hi, exact, op, length, reads, split, strict, when)


KIND_SINGLE, KIND_PAIR, KIND_ACCUM, KIND_STEM2 = P.KIND_SINGLE, P.KIND_PAIR, P.KIND_ACCUM, P.KIND_STEM2
KERNEL_VALU, KERNEL_MFMA, KERNEL_PICK, KERNEL_PICK_ROWS = 0, 1, 2, 3

# ---- step record (csrc/ctg_common.h: StepWord) ------------------------------------------------------------------ #
# ``reads``: "all" every ordinary step, "pair" pair steps, "thread" pair steps not on the matrix cores (VALU, pick, pick
# rows: B moves with the row), "sum" single-term and pair steps (a contraction), "mfma" matrix-core pair steps (the batch
# tables).  Nothing reads the table words of a stem record (kind 3).
STEP_RECORD = {
    0: W("kind", ENUM, lo=0, hi=3), 1: W("kernel", ENUM, lo=0, hi=3),
    2: W("a.space", SPACE, op="A"), 3: W("a.offset", OFFSET, op="A"), 4: W("a.leaf", LEAF, op="A"),
    5: W("b.space", SPACE, op="B"), 6: W("b.offset", OFFSET, op="B"), 7: W("b.leaf", LEAF, op="B"),
    8: W("c.space", SPACE, op="C"), 9: W("c.offset", OFFSET, op="C"), 10: W("c.leaf", LEAF, op="C"),
    11: W("R", EXTENT, split=(15, 16)), 12: W("Bt", EXTENT), 13: W("K", EXTENT, split=(36, 39)), 14: W("N", EXTENT),
    15: W("row_lo", EXTENT, split=(15, 16)), 16: W("row_hi_len", EXTENT, split=(15, 16)),
    17: W("rowA_hi", TABLE, op="A", length=(16,), reads="all"), 18: W("rowA_lo", TABLE, op="A", length=(15,), reads="all"),
    19: W("rowB_hi", TABLE, op="B", length=(16,), reads="thread"), 20: W("rowB_lo", TABLE, op="B", length=(15,), reads="thread"),
    21: W("rowC_hi", TABLE, op="C", length=(16,), reads="all"), 22: W("rowC_lo", TABLE, op="C", length=(15,), reads="all"),
    23: W("kA_lo", TABLE, op="A", length=(36,), reads="sum"), 24: W("kB_lo", TABLE, op="B", length=(36,), reads="pair"),
    25: W("nB", TABLE, op="B", length=(14,), reads="pair"), 26: W("nC", TABLE, op="C", length=(14,), reads="pair"),
    27: W("bA", TABLE, op="A", length=(12,), reads="mfma"), 28: W("bB", TABLE, op="B", length=(12,), reads="mfma"),
    29: W("bC", TABLE, op="C", length=(12,), reads="mfma"),
    30: W("a.size", SIZE, op="A"), 31: W("b.size", SIZE, op="B"), 32: W("c.size", SIZE, op="C"),
    33: W("macs", FREE), 34: W("elems_rw", FREE), 35: W("node", FREE),
    36: W("k_lo", EXTENT, split=(36, 39)),
    37: W("kA_hi", TABLE, op="A", length=(39,), reads="sum"), 38: W("kB_hi", TABLE, op="B", length=(39,), reads="pair"),
    39: W("k_hi_len", EXTENT, split=(36, 39)),
    40: W("a.producer", STEP), 41: W("b.producer", STEP),
    42: W("sharing", ENUM, lo=0, hi=2),
    43: W("stem", DESC, length=stem.DESC_WORDS, when="kind 3"),
    44: W("lds_comp", ENUM, lo=0, hi="components"),
    45: W("lds_desc", DESC, length=ldsrun.LR_HEAD_WORDS, when="lds_comp > 0"),
    46: W("reserved", FREE), 47: W("reserved", FREE),
}


def table_is_read(kind, kernel, reads):
    """Does any kernel (or host code of the executor) read a table of class ``reads`` for a step of this kind and kernel?"""
    if kind == KIND_STEM2:
        return False
    pair = kind == KIND_PAIR
    return {"all": True, "pair": pair, "thread": pair and kernel != KERNEL_MFMA, "sum": kind != KIND_ACCUM,
            "mfma": pair and kernel == KERNEL_MFMA}[reads]


def absent_is_legal(kind, kernel, reads, length):
    """May the table word be negative ("absent")?  Only where nothing reads the table, or where its length is 1 (the
    executor points it at one zero word) and no host code of the executor indexes the record's tables itself -- which
    it does for everything but the thread-per-output route (the gather orders of the matrix-core kernels, the vector
    test of the pick kernels)."""
    if not table_is_read(kind, kernel, reads):
        return True
    return length == 1 and not (kind == KIND_PAIR and kernel != KERNEL_VALU)


# ---- stem descriptor (csrc/ctg_common.h: StemWord) and its table lists ------------------------------------------- #
# lengths of the 14 tables at words 20..33 as functions of the header; ``one``: a single stem step
def stem_table_lengths(h):
    K1, N1, K2, N2, nr1, rows2, n_tiles, g_lo, one = h[1], h[2], h[3], h[4], h[5], h[6], h[8], h[9], h[18] == 1
    rows1 = 1 << nr1
    return [n_tiles // g_lo, g_lo, n_tiles // g_lo, g_lo, 8, 64, rows1 // 32, K1 // 16, K1 * N1,
            1 if one else K2 * N2, 1 if one else rows1, 1 if one else N1, rows1 if one else rows2, N1 if one else N2]


def stem_middle_lengths(h):
    return [h[34] * h[35], h[36], h[35]]   # bm_off [KM * NM], mid2_row [rowsM], mid2_col [NM]


STEM_TABLE_NAMES = ("gA_hi", "gA_lo", "gC_hi", "gC_lo", "kj_a", "lane_a", "rt_a", "chunk_a", "b1_off", "b2_off", "mid_row",
                    "mid_col", "out_row", "out_col")
STEM_DESC = {
    0: W("magic", ENUM, exact=True),
    1: W("K1", EXTENT), 2: W("N1", EXTENT), 3: W("K2", EXTENT), 4: W("N2", EXTENT), 5: W("nr1", EXTENT),
    6: W("rows2", EXTENT), 7: W("ng2", EXTENT), 8: W("n_tiles", EXTENT), 9: W("g_lo", EXTENT), 10: W("ld2", EXTENT),
    11: W("lds_bytes", FREE),
    12: W("b2.space", SPACE, op="b"), 13: W("b2.offset", OFFSET, op="b"), 14: W("b2.leaf", LEAF, op="b"),
    15: W("b2.size", SIZE, op="b"), 16: W("b2.producer", STEP),
    17: W("vec", ENUM, lo=0, hi=1), 18: W("one", ENUM, lo=0, hi=1), 19: W("reserved", FREE),
    **{20 + t: W(name, TABLE, length=t, reads="stem") for t, name in enumerate(STEM_TABLE_NAMES)},
    34: W("KM", EXTENT, when="tri"), 35: W("NM", EXTENT, when="tri"), 36: W("rowsM", EXTENT, when="tri"),
    37: W("ngM", EXTENT, when="tri"), 38: W("ldM", EXTENT, when="tri"), 39: W("tri", ENUM, lo=0, hi=1),
    40: W("bm.space", SPACE, op="m", when="tri"), 41: W("bm.offset", OFFSET, op="m", when="tri"),
    42: W("bm.leaf", LEAF, op="m", when="tri"), 43: W("bm.size", SIZE, op="m", when="tri"),
    44: W("bm.producer", STEP, when="tri"),
    45: W("bm_off", TABLE, length=0, reads="middle", when="tri"), 46: W("mid2_row", TABLE, length=1, reads="middle", when="tri"),
    47: W("mid2_col", TABLE, length=2, reads="middle", when="tri"),
    **{w: W("reserved", FREE) for w in range(48, 56)},
}

# ---- LDS component: header and record (csrc/ctg_lds.h: LdsHeadWord / LdsRecWord) --------------------------------- #
LDS_HEAD = {
    0: W("magic", ENUM, exact=True), 1: W("n_rec", EXTENT), 2: W("elems", SIZE), 3: W("phases", FREE),
    4: W("id", ENUM, exact=True), 5: W("reserved", FREE), 6: W("reserved", FREE), 7: W("reserved", FREE),
}
# ``reads``: "rec" every record, "pair" pair records (kind 1) -- the packer indexes these itself: none may be absent
LDS_RECORD = {
    0: W("kind", ENUM, lo=0, hi=1), 1: W("phase", EXTENT), 2: W("main", STEP, strict=True), 3: W("global_operand", ENUM, lo=-1, hi=2),
    4: W("a.lds", ENUM, lo=0, hi=1), 5: W("a.offset", OFFSET, op="A"),
    6: W("b.lds", ENUM, lo=0, hi=1), 7: W("b.offset", OFFSET, op="B"),
    8: W("c.lds", ENUM, lo=0, hi=1), 9: W("c.offset", OFFSET, op="C"),
    10: W("R", EXTENT, split=(13, 14)), 11: W("K", EXTENT, split=(15, 16)), 12: W("N", EXTENT),
    13: W("row_lo", EXTENT, split=(13, 14)), 14: W("row_hi_len", EXTENT, split=(13, 14)),
    15: W("k_lo", EXTENT, split=(15, 16)), 16: W("k_hi_len", EXTENT, split=(15, 16)),
    17: W("rowA_hi", TABLE, op="A", length=(14,), reads="rec"), 18: W("rowA_lo", TABLE, op="A", length=(13,), reads="rec"),
    19: W("rowB_hi", TABLE, op="B", length=(14,), reads="pair"), 20: W("rowB_lo", TABLE, op="B", length=(13,), reads="pair"),
    21: W("rowC_hi", TABLE, op="C", length=(14,), reads="rec"), 22: W("rowC_lo", TABLE, op="C", length=(13,), reads="rec"),
    23: W("kA_hi", TABLE, op="A", length=(16,), reads="rec"), 24: W("kA_lo", TABLE, op="A", length=(15,), reads="rec"),
    25: W("kB_hi", TABLE, op="B", length=(16,), reads="pair"), 26: W("kB_lo", TABLE, op="B", length=(15,), reads="pair"),
    27: W("nB", TABLE, op="B", length=(12,), reads="pair"), 28: W("nC", TABLE, op="C", length=(12,), reads="pair"),
    29: W("a.size", SIZE, op="A"), 30: W("b.size", SIZE, op="B"), 31: W("c.size", SIZE, op="C"),
    32: W("macs", FREE), **{w: W("reserved", FREE) for w in range(33, 40)},
}

RECORD_TYPES = {"step": STEP_RECORD, "stem": STEM_DESC, "lds_head": LDS_HEAD, "lds_record": LDS_RECORD}

INT64_MAX = (1 << 63) - 1
