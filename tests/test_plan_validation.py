"""CPU suite: ``ctg_plan_create`` against hostile descriptors, word by word (no GPU work).

A plan is the one thing a C caller hands over that turns into device addresses, so every word of it is attacked here:
tests/plan_words.py classifies each word of the four record types, this module derives the hostile values of every class
for the first step of every (kind, kernel) and the first LDS record of every form in a set of planner-written fixtures,
and asserts what the contract says -- CTG_E_INVALID / CTG_E_BOUNDS with a message that names the step or component, or
acceptance with unchanged answers for the free and the tolerated words.  ``rows_of`` is the one list of mutants; the
stand-alone sanitizer program (tests/cabi_validate_fuzz.cpp, tests/test_cabi_validate_fuzz.py) replays the same list.

NEVER AN EXECUTOR: a mutated plan goes to ``ctg_plan_create`` and, when accepted, to the host-only plan queries --
never to ``ctg_exec_create``, on any machine.  An accepted bad word is a device fault waiting to happen, and provoking
one is not a test.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
import golden_util as G
import plan_words as PW
from cotengra_amd import ldsrun, runtime
from cotengra_amd.plan import STEP_WORDS, compile_tree
from cotengra_amd.vjp import compile_vjp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_BOUNDS = -1, -4
MAX = PW.INT64_MAX
BIG = 1 << 40
ARRAYS = ("input_sizes", "input_offsets", "steps", "tables", "slice_sizes", "slice_fixed", "slice_strides", "slice_group")
SCALARS = ("dtype", "inputs_elems", "arena_elems", "result_elems")
FIELDS = ARRAYS + SCALARS   # (a field's position here is its code in the mutation list of the sanitizer program)


# ---- fixtures: planner-written plans, serialised ---------------------------------------------------------------- #

class Fixture:
    def __init__(self, name, plan):
        s = plan.serialise()
        self.name = name
        self.f = {k: np.ascontiguousarray(s[k], dtype=np.int64).copy() for k in ARRAYS}
        self.f.update(dtype=int(s["dtype"]), inputs_elems=int(plan.inputs_elems), arena_elems=int(s["arena_elems"]),
                      result_elems=int(s["result_elems"]))
        self.n_steps, self.n_inputs, self.n_sliced = int(s["n_steps"]), len(s["input_sizes"]), len(s["slice_sizes"])
        self.recs = self.f["steps"].reshape(-1, STEP_WORDS)
        self.T = self.f["tables"]
        self.blob = len(self.T)
        self.n_comps = len(plan.lds_runs or [])
        # the largest slice offset of every leaf, as validate_plan sums it
        st = self.f["slice_strides"].reshape(self.n_inputs + 1, self.n_sliced)
        digit = np.where(self.f["slice_fixed"] >= 0, self.f["slice_fixed"], self.f["slice_sizes"] - 1)
        self.max_soff = [int((st[l] * digit).sum()) for l in range(self.n_inputs + 1)]
        # how many table words of the whole descriptor point at a blob offset (the planner shares its one-word zero table)
        self.table_refs = {}
        for r in self.recs:
            words = [int(r[w]) for w, word in PW.STEP_RECORD.items() if word.cls == PW.TABLE]
            if r[0] == PW.KIND_STEM2:
                h = self.T[r[43]:r[43] + PW.stem.DESC_WORDS]
                words += [int(h[w]) for w, word in PW.STEM_DESC.items() if word.cls == PW.TABLE and (word.when != "tri" or h[39] == 1)]
            for o in words:
                self.table_refs[o] = self.table_refs.get(o, 0) + 1
        for d in sorted({int(r[45]) for r in self.recs if r[44] > 0}):
            for i in range(int(self.T[d + 1])):
                at = d + ldsrun.LR_HEAD_WORDS + i * ldsrun.LR_WORDS
                for w, word in PW.LDS_RECORD.items():
                    if word.cls == PW.TABLE:
                        o = int(self.T[at + w])
                        self.table_refs[o] = self.table_refs.get(o, 0) + 1
        self.base = self.create(())
        assert self.base[0] == 0, (name, self.base)

    def cap(self, space):
        return {0: self.f["inputs_elems"], 1: self.f["arena_elems"], 2: self.f["result_elems"]}[int(space)]

    def create(self, edits):
        """``ctg_plan_create`` on the fixture with ``edits`` [(field, index, value)] applied; -> (rc, message, nslices,
        workspace bytes).  The plan is destroyed again; it never reaches an executor."""
        f = dict(self.f)
        for field, idx, val in edits:
            if field in SCALARS:
                f[field] = val
            else:
                if f[field] is self.f[field]:
                    f[field] = self.f[field].copy()
                f[field][idx] = val
        lib = runtime.load()
        d = runtime.PlanDesc()
        d.dtype, d.n_inputs = f["dtype"], self.n_inputs
        d.input_sizes, d.input_offsets = runtime._i64p(f["input_sizes"]), runtime._i64p(f["input_offsets"])
        d.inputs_elems, d.arena_elems, d.result_elems = f["inputs_elems"], f["arena_elems"], f["result_elems"]
        d.n_steps, d.steps = self.n_steps, runtime._i64p(f["steps"])
        d.n_table_words, d.tables = self.blob, runtime._i64p(f["tables"])
        d.n_sliced = self.n_sliced
        d.slice_sizes, d.slice_fixed = runtime._i64p(f["slice_sizes"]), runtime._i64p(f["slice_fixed"])
        d.slice_strides, d.slice_group = runtime._i64p(f["slice_strides"]), runtime._i64p(f["slice_group"])
        h = C.c_void_p()
        rc = lib.ctg_plan_create(C.byref(d), C.byref(h))
        if rc != 0:
            return rc, lib.ctg_last_error().decode("utf-8", "replace"), None, None
        n, ws = C.c_int64(), (C.c_int64 * 4)()
        assert lib.ctg_plan_nslices(h, C.byref(n)) == 0 and lib.ctg_plan_workspace_bytes(h, ws) == 0
        lib.ctg_plan_destroy(h)
        return 0, "", n.value, tuple(ws)


def chain3():
    """``x[o1,a,k] y[o2,k,b] -> p``, ``p z[o3,a,b] -> (o1,o2,o3)`` and 23 requests on 16 distinct (o1, o2): a sparse
    root step over a row-sparse node (tests/test_pick_chain_host.py)."""
    tree = ca.ContractionTree.from_path([("o1", "a", "k"), ("o2", "k", "b"), ("o3", "a", "b")], ("o1", "o2", "o3"),
                                        dict(o1=8, o2=8, o3=4, a=3, b=5, k=6), ssa_path=[(0, 1), (3, 2)])
    rng = np.random.default_rng(0)
    pairs = rng.permutation(64)[:16]
    which = np.concatenate([np.arange(16), rng.integers(0, 16, 7)])
    rng.shuffle(which)
    return tree, np.stack([pairs[which] // 8, pairs[which] % 8, rng.integers(0, 4, 23)], axis=1).astype(np.int64)


_FIXTURES = {}


def fixtures():
    """name -> Fixture; between them every record kind the planner writes (asserted by test_fixtures_hold_every_kind)."""
    if _FIXTURES:
        return _FIXTURES
    import lds_variant_cases as LV
    import stem_variant_cases as SV
    from cotengra_amd import stem

    def golden(name):
        return G.tree_of(next(c for c in G.cases("tree") if c["name"] == name))

    plans = {
        # thread-per-output pairs, the accumulate step, two sliced indices with a slice group, LDS loads and pairs
        "lattice4x4_sliced": compile_tree(golden("lattice4x4_sliced"), "complex64"),
        # a projected index
        "project_1": compile_tree(golden("project_1"), "complex128"),
        # single-term steps (leaf preprocessing), as ordinary steps and inside an LDS component
        "preproc_s0_a": compile_tree(golden("preproc_s0_a"), "float32"),
        "single_diag_slice_a": compile_tree(golden("single_diag_slice_a"), "float64"),
        # a gradient plan: a run of accumulate steps, results in the leaves' own ranges
        "vjp_lattice4x4_sliced": compile_vjp(golden("lattice4x4_sliced"), "complex64"),
    }
    # matrix-core pairs with batch tables, complex64 (gather orders on the host) and float32 (the 16-byte gather test)
    batched = ca.ContractionTree.from_path([("b", "a", "k"), ("b", "k", "n")], ("b", "a", "n"), dict(b=3, a=128, k=32, n=32),
                                           path=[(0, 1)])
    plans["mfma_batched_c64"] = compile_tree(batched, "complex64", force_kernel=PW.KERNEL_MFMA)
    plans["mfma_batched_f32"] = compile_tree(batched, "float32", force_kernel=PW.KERNEL_MFMA)
    # a sparse root step (kernel 2) over a row-sparse step (kernel 3)
    tree, coords = chain3()
    plans["pick_chain3"] = compile_tree(tree, "complex64", pick=coords, pick_chain=True)
    # an LDS component with matrix-core pair records
    plans["lds_mfma"] = compile_tree(LV.MFMA_ROWS[0].tree(), "complex64")
    # a fused stem pair and a single stem step: the pairing model opened up as tests/test_stem_variant_plans.py does
    with pytest.MonkeyPatch.context() as mp:
        G.fuse_whatever_fits(mp, h2_all=True)
        mp.setattr(stem, "single_seconds", lambda *a, **k: 0.0)
        plans["stem_pair"] = compile_tree(SV.INST_ROWS[0].tree(), "complex64", fuse=True, fuse_min_elems=1 << 10, stem_bf16x3=True)
        plans["stem_one"] = compile_tree(SV.ONE_ROWS[0].tree(), "complex64", fuse=True, fuse_min_elems=1 << 10, stem_bf16x3=True)
        plans["stem_pair_sliced"] = compile_tree(SV.SLICED_ROWS[0].tree(), "complex64", fuse=True, fuse_min_elems=1 << 10,
                                                 stem_bf16x3=True)
    # (three-step stem tiles: the default library is built without them -- ctg_stem_triple_instantiated is 0 for every
    # shape -- and the planner emits none)
    for name, plan in plans.items():
        _FIXTURES[name] = Fixture(name, plan)
    return _FIXTURES


FIXTURE_NAMES = ("lattice4x4_sliced", "project_1", "preproc_s0_a", "single_diag_slice_a", "vjp_lattice4x4_sliced",
                 "mfma_batched_c64", "mfma_batched_f32", "pick_chain3", "lds_mfma", "stem_pair", "stem_one", "stem_pair_sliced")


# ---- which records are attacked --------------------------------------------------------------------------------- #

def stem_form(fx, r):
    h = fx.T[r[43]:r[43] + PW.stem.DESC_WORDS]
    return "one" if h[18] == 1 else ("tri" if h[39] == 1 else "pair")


def step_key(fx, s):
    r = fx.recs[s]
    return (int(r[0]), stem_form(fx, r)) if r[0] == PW.KIND_STEM2 else (int(r[0]), int(r[1]))


def chosen_steps(fx):
    """The first step of every (kind, kernel) -- of every stem form --, and the first member of an LDS component."""
    first = {}
    for s in range(fx.n_steps):
        first.setdefault(step_key(fx, s), s)
        if fx.recs[s][44] > 0:
            first.setdefault("member", s)
    return sorted(set(first.values()))


def lds_components(fx):
    """descriptor offset of every LDS component of the fixture"""
    return sorted({int(r[45]) for r in fx.recs if r[44] > 0})


def lds_record(fx, d, i):
    at = d + ldsrun.LR_HEAD_WORDS + i * ldsrun.LR_WORDS
    return at, fx.T[at:at + ldsrun.LR_WORDS]


def lds_form(fx, q):
    """(kind, global operand, matrix cores?) of a record: csrc/ctg_lds_host.hip, lds_record_form"""
    mfma = False
    if q[0] == 1 and fx.f["dtype"] == 2 and q[12] >= 8 and q[10] >= 16:
        mfma = not fx.T[q[19]:q[19] + q[14]].any() and not fx.T[q[20]:q[20] + q[13]].any()
    return int(q[0]), int(q[3]), bool(mfma)


def chosen_lds_records(fx):
    """(descriptor, record) of the first record of every form"""
    first = {}
    for d in lds_components(fx):
        for i in range(int(fx.T[d + 1])):
            first.setdefault(lds_form(fx, lds_record(fx, d, i)[1]), (d, i))
    return sorted(set(first.values()))


# ---- the mutants: (id, edits, expect) ---------------------------------------------------------------------------- #
# expect: "reject" -- CTG_E_INVALID or CTG_E_BOUNDS --, or "accept" -- created, nslices and workspace as the fixture's.
# A hostile value that happens to be the word's own value is no mutant: it is listed as accepted.

def _range_values(cls, off, size, cap):
    """Hostile values of an offset or a size word of an operand of ``size`` elements at ``off`` in a buffer of ``cap``:
    one below zero, the first value that leaves the buffer, one beyond it, 2^40, INT64_MAX."""
    first_out = cap - size + 1 if cls == PW.OFFSET else cap - off + 1
    return (-1, first_out, cap + 1, BIG, MAX)


def _table_values(length, blob):
    return (-1, -7, blob - length + 1, blob, BIG, MAX - length + 1, MAX)


def _emit(rows, ident, field, idx, cur, values, expect):
    for v in dict.fromkeys(int(v) for v in values):
        rows.append((f"{ident}={v}", ((field, int(idx), v),), "accept" if v == int(cur) else expect))


def reach_rows(fx, rows, ident, tabs, base, limit, size_edit=None, raise_ok=True):
    """The checks that keep table-formed addresses inside an operand.  ``tabs``: the (name, offset, length) of the tables
    whose largest entries, with ``base`` (the leaf's largest slice offset), sum to the operand's top address, which must
    stay below ``limit`` (the operand's size word; the elements of an LDS tile).  Per table: its largest entry raised
    until the top address is ``limit`` (first out: refused) and ``limit - 1`` (last in: accepted -- listed where the
    table belongs to this word alone and, ``raise_ok``, no other rule reads its entries).  ``size_edit`` (field, index) of
    the size word: shrunk to the top address (one too small: refused) and to one more (just enough: accepted)."""
    top = base + sum(int(fx.T[o:o + n].max()) for _, o, n in tabs)
    assert top < limit, (ident, top, limit)
    for name, o, n in tabs:
        t = fx.T[o:o + n]
        at, mx = o + int(t.argmax()), int(t.max())
        rows.append((f"{ident}.{name}.max->size", (("tables", at, mx + limit - top),), "reject"))
        if raise_ok and fx.table_refs.get(o, 0) == 1:
            rows.append((f"{ident}.{name}.max->size-1", (("tables", at, mx + limit - 1 - top),), "accept"))
    if size_edit is not None:
        rows.append((f"{ident}.size=top", ((size_edit[0], size_edit[1], top),), "reject"))
        rows.append((f"{ident}.size=top+1", ((size_edit[0], size_edit[1], top + 1),), "accept"))


def step_rows(fx, s, rows):
    r = fx.recs[s]
    kind, kernel = int(r[0]), int(r[1])
    stem_rec = kind == PW.KIND_STEM2
    used = {"A": True, "B": kind in (PW.KIND_PAIR, PW.KIND_STEM2), "C": True}
    words = {"A": (2, 3, 4, 30), "B": (5, 6, 7, 31), "C": (8, 9, 10, 32)}
    for w, word in PW.STEP_RECORD.items():
        ident, cur, at = f"step{s}{step_key(fx, s)}.{word.name}[{w}]", int(r[w]), s * STEP_WORDS + w
        emit = lambda values, expect: _emit(rows, ident, "steps", at, cur, values, expect)   # noqa: E731
        if word.cls == PW.ENUM:
            hi = fx.n_comps if word.hi == "components" else word.hi
            emit((word.lo - 1, hi + 1), "reject")
        elif word.cls in (PW.SPACE, PW.LEAF, PW.OFFSET, PW.SIZE):
            sp, ow, lw, zw = words[word.op]
            if word.cls == PW.SPACE:
                emit((-1, 3), "reject")
            elif word.cls == PW.LEAF:
                emit((-2, fx.n_inputs + 1), "reject")
            elif used[word.op]:
                emit(_range_values(word.cls, int(r[ow]), int(r[zw]), fx.cap(r[sp])), "reject")
            else:
                emit((-1, 1, BIG, MAX), "reject")   # (an operand the step does not have: offset 0, size 0)
        elif word.cls == PW.EXTENT:
            # (a stem record's extents restate its descriptor: every other value is refused)
            emit((0, -1, BIG) + ((cur + 1,) if word.split or stem_rec else ()), "reject")
        elif word.cls == PW.TABLE:
            length = int(np.prod([int(r[i]) for i in word.length]))
            read = PW.table_is_read(kind, kernel, word.reads)
            legal = PW.absent_is_legal(kind, kernel, word.reads, length)
            vals = _table_values(length if read else 1, fx.blob)
            emit(vals[:2], "accept" if legal else "reject")
            emit(vals[2:], "reject")
        elif word.cls == PW.STEP:
            emit((-7, fx.n_steps, BIG), "accept")   # tolerated by design: "no producer"
        elif word.cls == PW.DESC:
            if (w == 43 and stem_rec) or (w == 45 and r[44] > 0):
                emit(_table_values(word.length, fx.blob), "reject")
            else:
                emit((-7, BIG, MAX), "accept")
        else:
            assert word.cls == PW.FREE
            emit((-7, BIG, MAX), "accept")
    if not stem_rec:
        table_content_rows(fx, s, rows)


def table_content_rows(fx, s, rows):
    """Per table the step reads: its smallest entry set to -1; its largest raised until the operand's top address is
    the capacity of its space, one past the last element."""
    r = fx.recs[s]
    kind, kernel = int(r[0]), int(r[1])
    ops = {"A": (2, 3, 4), "B": (5, 6, 7), "C": (8, 9, 10)}
    tabs = {}
    for w, word in PW.STEP_RECORD.items():
        if word.cls == PW.TABLE and PW.table_is_read(kind, kernel, word.reads) and r[w] >= 0:
            tabs.setdefault(word.op, []).append((w, word, int(r[w]), int(np.prod([int(r[i]) for i in word.length]))))
    for op, lst in tabs.items():
        sp, ow, lw = ops[op]
        top = int(r[ow]) + (fx.max_soff[r[lw]] if r[lw] >= 0 else 0) + sum(int(fx.T[o:o + n].max()) for _, _, o, n in lst)
        for w, word, o, n in lst:
            ident = f"step{s}{step_key(fx, s)}.{word.name}[{w}]"
            t = fx.T[o:o + n]
            rows.append((f"{ident}.min=-1", (("tables", o + int(t.argmin()), -1),), "reject"))
            rows.append((f"{ident}.max->cap", (("tables", o + int(t.argmax()), int(t.max()) + fx.cap(r[sp]) - top),), "reject"))
        zw = {"A": 30, "B": 31, "C": 32}[op]
        reach_rows(fx, rows, f"step{s}{step_key(fx, s)}.{op}", [(word.name, o, n) for _, word, o, n in lst],
                   fx.max_soff[r[lw]] if r[lw] >= 0 else 0, int(r[zw]), ("steps", s * STEP_WORDS + zw))


def stem_rows(fx, s, rows):
    d = int(fx.recs[s][43])
    h = fx.T[d:d + PW.stem.DESC_WORDS]
    one, tri = h[18] == 1, h[39] == 1
    lens = PW.stem_table_lengths(h)
    for w, word in PW.STEM_DESC.items():
        ident, cur = f"step{s}.stem[{stem_form(fx, fx.recs[s])}].{word.name}[{w}]", int(h[w])
        emit = lambda values, expect: _emit(rows, ident, "tables", d + w, cur, values, expect)   # noqa: E731
        if word.when == "tri" and not tri:
            emit((-7, 1, BIG), "reject")   # (no middle stage: zeros)
        elif word.cls == PW.ENUM:
            emit((cur - 1, cur + 1) if word.exact else (word.lo - 1, word.hi + 1), "reject")
        elif word.cls == PW.EXTENT:
            emit((0, -1, BIG), "reject")
        elif word.cls == PW.SPACE:
            emit((-1, 3), "reject")
        elif word.cls == PW.LEAF:
            emit((-2, fx.n_inputs + 1), "reject")
        elif word.cls in (PW.OFFSET, PW.SIZE):
            if one:
                emit((-1, 1, BIG, MAX), "reject")   # (no second small operand: offset 0, size 0)
            else:
                emit(_range_values(word.cls, int(h[13]), int(h[15]), fx.cap(h[12])), "reject")
        elif word.cls == PW.TABLE:
            emit(_table_values(lens[word.length], fx.blob), "reject")   # (a stem descriptor has no absent tables)
            o, n = cur, lens[word.length]
            rows.append((f"{ident}.min=-1", (("tables", o + int(fx.T[o:o + n].argmin()), -1),), "reject"))
        elif word.cls == PW.STEP:
            emit((-7, fx.n_steps, BIG), "accept")
        else:
            assert word.cls == PW.FREE
            emit((-7, BIG, MAX), "accept")
    if tri:
        return
    # every address the tables form stays inside the operand (csrc/ctg_runtime.hip: validate_stem, the operand loop):
    # the big operand A, the small operands B1 and B2, the result C -- and the intermediate tile inside its LDS
    r, ident = fx.recs[s], f"step{s}.stem[{stem_form(fx, fx.recs[s])}]"
    name = PW.STEM_TABLE_NAMES
    tab = lambda *ts: [(name[t], int(h[20 + t]), lens[t]) for t in ts]   # noqa: E731
    soff = lambda leaf: fx.max_soff[leaf] if leaf >= 0 else 0            # noqa: E731
    # (16-byte gathers hold the big operand's tables to even entries and paired slots: no "last in" row by a raised entry)
    reach_rows(fx, rows, ident + ".A", tab(0, 1, 6, 7, 4, 5), soff(r[4]), int(r[30]), ("steps", s * STEP_WORDS + 30),
               raise_ok=h[17] == 0)
    reach_rows(fx, rows, ident + ".B1", tab(8), soff(r[7]), int(r[31]), ("steps", s * STEP_WORDS + 31))
    if not one:
        reach_rows(fx, rows, ident + ".B2", tab(9), soff(h[14]), int(h[15]), ("tables", d + 15))
        reach_rows(fx, rows, ident + ".tile", tab(10, 11), 0, int(h[6]) * (int(h[3]) + 4))
    reach_rows(fx, rows, ident + ".C", tab(2, 3, 12, 13), soff(r[10]), int(r[32]), ("steps", s * STEP_WORDS + 32))


def lds_rows(fx, d, i, rows):
    at, q = lds_record(fx, d, i)
    kind = int(q[0])
    m = fx.recs[int(q[2])]
    elems = int(fx.T[d + 2])
    gop = int(q[3])
    main_words = {"A": (5, 6, 7) if gop == 1 else (2, 3, 4), "C": (8, 9, 10)}
    ops = {"A": (4, 5, 29, True), "B": (6, 7, 30, kind == 1), "C": (8, 9, 31, True)}
    for w, word in PW.LDS_RECORD.items():
        ident, cur = f"lds@{d}.rec{i}{lds_form(fx, q)}.{word.name}[{w}]", int(q[w])
        emit = lambda values, expect: _emit(rows, ident, "tables", at + w, cur, values, expect)   # noqa: E731
        if word.cls == PW.ENUM:
            emit((word.lo - 1, word.hi + 1), "reject")
        elif word.cls == PW.STEP:
            emit((-1, fx.n_steps, BIG), "reject")   # (strict: the record belongs to a member step)
        elif word.cls in (PW.OFFSET, PW.SIZE):
            lw, ow, zw, used = ops[word.op]
            if used and q[lw] == 1:
                emit(_range_values(word.cls, int(q[ow]), int(q[zw]), elems), "reject")
            elif used and word.cls == PW.SIZE:   # the global side: the member step's own space and offset
                sp, mo, _ = main_words[word.op]
                emit(_range_values(word.cls, int(m[mo]), int(q[zw]), fx.cap(m[sp])), "reject")
            else:
                emit((-1, 1, BIG, MAX), "reject")   # (the offset of a global side, an operand a load does not have: 0)
        elif word.cls == PW.EXTENT:
            emit((0, -1, BIG) + ((cur + 1,) if word.split else ()), "reject")
        elif word.cls == PW.TABLE:
            length = int(np.prod([int(q[j]) for j in word.length]))
            read = word.reads == "rec" or kind == 1
            vals = _table_values(length if read else 1, fx.blob)
            emit(vals[:2], "reject" if read else "accept")   # (the packer indexes what it reads: never absent)
            emit(vals[2:], "reject")
            if read:
                o = cur
                rows.append((f"{ident}.min=-1", (("tables", o + int(fx.T[o:o + length].argmin()), -1),), "reject"))
        else:
            assert word.cls == PW.FREE
            emit((-7, BIG, MAX), "accept")
    # every address the tables form stays inside the operand: in LDS inside its size word (and so inside the data
    # area), on the global side -- with the leaf's largest slice offset -- inside the size word as well
    for op, (lw, ow, zw, used) in ops.items():
        if not used:
            continue
        tabs = [(word.name, int(q[w]), int(np.prod([int(q[j]) for j in word.length])))
                for w, word in PW.LDS_RECORD.items() if word.cls == PW.TABLE and word.op == op and (word.reads == "rec" or kind == 1)]
        base = 0
        if q[lw] != 1:
            leaf = int(m[main_words[op][2]])
            base = fx.max_soff[leaf] if leaf >= 0 else 0
        reach_rows(fx, rows, f"lds@{d}.rec{i}{lds_form(fx, q)}.{op}[{'lds' if q[lw] == 1 else 'global'}]", tabs, base,
                   int(q[zw]), ("tables", at + zw))
        if q[lw] == 1:
            # ... and inside the component's data area, whatever the size word says: the data area shrunk to the operand's
            # last element (the size word no longer fits: refused)
            top = int(q[ow]) + sum(int(fx.T[o:o + n].max()) for _, o, n in tabs)
            rows.append((f"lds@{d}.rec{i}.{op}.elems=top", (("tables", d + 2, top),), "reject"))


def lds_head_rows(fx, d, rows):
    isz = (4, 8, 8, 16)[fx.f["dtype"]]
    for w, word in PW.LDS_HEAD.items():
        ident, cur = f"lds@{d}.head.{word.name}[{w}]", int(fx.T[d + w])
        emit = lambda values, expect: _emit(rows, ident, "tables", d + w, cur, values, expect)   # noqa: E731
        if word.cls == PW.ENUM:
            emit((cur - 1, cur + 1), "reject")
        elif word.cls == PW.EXTENT:
            emit((0, -1, BIG), "reject")
        elif word.cls == PW.SIZE:
            emit((-1, 160 * 1024 // isz + 1, BIG, MAX), "reject")   # (more than the LDS of a compute unit)
        else:
            assert word.cls == PW.FREE
            emit((-7, BIG, MAX), "accept")


def header_rows(fx, rows):
    """The arrays and sizes of the descriptor itself."""
    cap = fx.f["inputs_elems"]
    for i in (0, fx.n_inputs - 1):
        size, off = int(fx.f["input_sizes"][i]), int(fx.f["input_offsets"][i])
        _emit(rows, f"input_sizes[{i}]", "input_sizes", i, size, (0, -1, cap - off + 1, cap + 1, BIG, MAX), "reject")
        _emit(rows, f"input_offsets[{i}]", "input_offsets", i, off, _range_values(PW.OFFSET, off, size, cap), "reject")
    for field in ("inputs_elems", "arena_elems", "result_elems"):
        for v in (0, -1, (1 << 56) + 1, MAX):
            rows.append((f"{field}={v}", ((field, 0, v),), "reject"))
    for v in (-1, 4):
        rows.append((f"dtype={v}", (("dtype", 0, v),), "reject"))
    st = fx.f["slice_strides"].reshape(fx.n_inputs + 1, fx.n_sliced)
    for j in range(fx.n_sliced):
        d, f = int(fx.f["slice_sizes"][j]), int(fx.f["slice_fixed"][j])
        # (an extent of 2^40 moves every leaf that carries the index far outside its tensor)
        _emit(rows, f"slice_sizes[{j}]", "slice_sizes", j, d, (0, -1, BIG, MAX), "reject")
        _emit(rows, f"slice_fixed[{j}]", "slice_fixed", j, f, (-2, BIG, MAX) + ((0,) if d > 1 else ()), "reject")
        _emit(rows, f"slice_group[{j}]", "slice_group", j, int(fx.f["slice_group"][j]), (-1, 2) + ((1,) if f >= 0 else ()), "reject")
        digit = f if f >= 0 else d - 1
        for l in range(fx.n_inputs + 1):
            if st[l, j] == 0 and l not in (0, fx.n_inputs):
                continue   # (every leaf that carries the index, and the first and the last row whatever they carry)
            at = l * fx.n_sliced + j
            # a stride times (extent - 1) that leaves 64 bits (2^62, 2^63 - 1), and one that stays inside them but
            # moves the leaf out of its tensor (2^40); harmless only where the index has a single position, 0
            _emit(rows, f"slice_strides[{l},{j}]", "slice_strides", at, int(st[l, j]), (-1,), "reject")
            _emit(rows, f"slice_strides[{l},{j}]", "slice_strides", at, int(st[l, j]), (BIG, 1 << 62, MAX),
                  "reject" if digit > 0 else "accept")


_ROWS = {}


def rows_of(fx):
    if fx.name not in _ROWS:
        rows = []
        for s in chosen_steps(fx):
            step_rows(fx, s, rows)
            if fx.recs[s][0] == PW.KIND_STEM2:
                stem_rows(fx, s, rows)
        for d in lds_components(fx)[:1]:
            lds_head_rows(fx, d, rows)
        for d, i in chosen_lds_records(fx):
            lds_rows(fx, d, i, rows)
        header_rows(fx, rows)
        _ROWS[fx.name] = rows
    return _ROWS[fx.name]


def judge(fx, row):
    """None if the library treats the mutant as the contract says, else what it did."""
    ident, edits, expect = row
    rc, msg, nsl, ws = fx.create(edits)
    if expect == "reject":
        if rc == 0:
            return "ACCEPTED"
        if rc not in (E_INVALID, E_BOUNDS):
            return f"rc {rc}: {msg}"
        # the message names the step or the component (the descriptor's own arrays: the input, slice or buffer)
        if not re.search(r"step|component|input|slice|buffer|leaf|dtype|projected|plan", msg):
            return f"message names nothing: {msg!r}"
        if edits[0][0] in ("steps", "tables") and not re.search(r"steps? \d+|component \d+|leaf \d+", msg):
            return f"message names no step or component: {msg!r}"
        return None
    if rc != 0:
        return f"rejected ({rc}): {msg}"
    if (nsl, ws) != fx.base[2:]:
        return f"answers changed: nslices {nsl}, workspace {ws}"
    return None


# ---- tests ------------------------------------------------------------------------------------------------------- #

def header_constant(path, name):
    text = open(os.path.join(ROOT, path)).read()
    return int(re.search(rf"\b{name}\s*=\s*(\d+)", text).group(1))


def test_the_map_covers_every_word():
    """No word of any record type can be left out silently: the lengths are the library's own."""
    counts = {"step": header_constant("cotengra_amd/csrc/ctg_common.h", "STEP_WORDS"),
              "stem": header_constant("cotengra_amd/csrc/ctg_common.h", "STEM_WORDS"),
              "lds_head": header_constant("cotengra_amd/csrc/ctg_lds.h", "LR_HEAD_WORDS"),
              "lds_record": header_constant("cotengra_amd/csrc/ctg_lds.h", "LR_WORDS")}
    public = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    assert counts["step"] == int(re.search(r"#define CTG_STEP_WORDS (\d+)", public).group(1)) == STEP_WORDS
    assert counts["stem"] == PW.stem.DESC_WORDS and counts["lds_head"] == ldsrun.LR_HEAD_WORDS and counts["lds_record"] == ldsrun.LR_WORDS
    for name, words in PW.RECORD_TYPES.items():
        assert sorted(words) == list(range(counts[name])), name
        for w, word in words.items():
            assert word.cls in PW.CLASSES and word.name, (name, w)
            if word.cls == PW.TABLE:
                assert word.length is not None and word.reads, (name, w)
    # the free words are the bookkeeping and the reserved ones
    free = {w.name for words in PW.RECORD_TYPES.values() for w in words.values() if w.cls == PW.FREE}
    assert free == {"macs", "elems_rw", "node", "reserved", "lds_bytes", "phases"}


def test_fixtures_hold_every_kind():
    have, lds = set(), set()
    for fx in fixtures().values():
        have |= {step_key(fx, s) for s in range(fx.n_steps)}
        lds |= {lds_form(fx, lds_record(fx, d, i)[1]) for d in lds_components(fx) for i in range(int(fx.T[d + 1]))}
    assert have >= {(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (3, "pair"), (3, "one")}, have
    assert {(0, 0, False), (0, 1, False), (1, -1, False), (1, 2, False)} <= lds and any(f[2] for f in lds), lds
    fx = fixtures()
    assert (fx["project_1"].f["slice_fixed"] >= 0).any() and fx["lattice4x4_sliced"].f["slice_group"].any()
    assert fx["mfma_batched_c64"].recs[0][12] == 3                                    # batch tables of length 3
    assert (fx["vjp_lattice4x4_sliced"].recs[:, 0] == PW.KIND_ACCUM).sum() > 1        # a run of accumulate steps
    assert fx["stem_pair_sliced"].n_sliced > 0
    # (three-step tiles: out of the product library since round 5 -- the probe below is the one the GPU suite uses to skip
    # its triple tests; the middle-stage branch of validate_stem is attacked by no fixture: ADVICE.md)
    assert runtime.load().ctg_stem_triple_instantiated(1, 0, 1, 2, 1, 1, 1, 1, 0) == 0


def test_planner_plans_are_accepted():
    """The accept side: every fixture, and every golden tree in the four dtypes, fused and unfused, with its gradient
    plan -- a validator made too strict fails here, without a GPU."""
    assert sorted(fixtures()) == sorted(FIXTURE_NAMES)
    for case in G.cases("tree"):
        tree = G.tree_of(case)
        for dtype in ("float32", "float64", "complex64", "complex128"):
            for fuse in (None, False):
                runtime.DevicePlan(compile_tree(tree, dtype, fuse=fuse)).close()
            runtime.DevicePlan(compile_vjp(tree, dtype)).close()


def test_stem_and_lds_variant_plans_are_accepted():
    """... and the plans of the variant tables: every stem instantiation's tree and every LDS form's."""
    import lds_variant_cases as LV
    import stem_variant_cases as SV
    from cotengra_amd import stem
    for row in LV.ALL_ROWS:
        for dtype in LV.DTYPES:
            runtime.DevicePlan(compile_tree(row.tree(), dtype)).close()
    with pytest.MonkeyPatch.context() as mp:
        G.fuse_whatever_fits(mp, h2_all=True)
        mp.setattr(stem, "single_seconds", lambda *a, **k: 0.0)
        seen = set()
        for row in SV.ALL_ROWS:
            if row.network not in seen:
                seen.add(row.network)
                runtime.DevicePlan(compile_tree(row.tree(), "complex64", fuse=True, fuse_min_elems=1 << 10, stem_bf16x3=True)).close()


@pytest.mark.parametrize("name", ["lattice4x4_sliced", "lds_mfma"])
def test_records_of_one_phase_may_not_share_a_result_range(name):
    """Records of one phase run between the same two barriers: a record whose result is moved onto another one's result,
    or onto an operand another one reads, is a data race -- refused, with the component and both records named."""
    fx = fixtures()[name]
    tried = 0
    for d in lds_components(fx):
        recs = [lds_record(fx, d, i) for i in range(int(fx.T[d + 1]))]
        for i, (at_i, qi) in enumerate(recs):
            for j, (at_j, qj) in enumerate(recs):
                if i == j or qi[1] != qj[1] or qi[8] != 1:
                    continue
                # record i's result onto record j's result / onto record j's first operand, where it fits the data area
                for w_lds, w_off in ((8, 9), (4, 5)):
                    if qj[w_lds] != 1 or qj[w_off] == qi[9] or qj[w_off] + qi[31] > fx.T[d + 2]:
                        continue
                    rc, msg, _, _ = fx.create((("tables", at_i + 9, int(qj[w_off])),))
                    tried += 1
                    # (the first clash in record order is the one reported: it involves a record of this phase)
                    m = re.search(rf"component \d+: records (\d+) and (\d+) of phase {qi[1]} ", msg)
                    assert rc == E_INVALID and m and {int(m.group(1)), int(m.group(2))} & {i, j}, (d, i, j, rc, msg)
    assert tried >= 2


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_every_hostile_word_is_judged_as_the_contract_says(name):
    """Every classified (word, value) pair of the fixture's chosen records, the contents of every table they read and the
    descriptor's own arrays.  Rejected with CTG_E_INVALID / CTG_E_BOUNDS and a message naming the step or component;
    free words, producer words and absent-legal tables accepted with unchanged ``ctg_plan_nslices`` and workspace."""
    fx = fixtures()[name]
    rows = rows_of(fx)
    assert len(rows) > 100 and {r[2] for r in rows} == {"accept", "reject"}
    wrong = [(row[0], why) for row in rows for why in [judge(fx, row)] if why]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows:\n" + "\n".join(f"  {i}: {w}" for i, w in wrong[:60])
