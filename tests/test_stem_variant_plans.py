"""The plans the device tests of the stem-kernel instantiations rely on (tests/stem_variant_cases.py, run by
tests/test_gpu_stem_variants.py), checked without a device: every row is planned, in the arithmetic it runs in, as
exactly one stem step with the geometry the table records, that geometry takes the dispatch entry the row names by the
header's rules, and the table's rows are the rows of csrc/ctg_stem_impl.h's lists -- a row added to the header without
a case, or a case that drifts to the run-time-count variant when the planner changes, fails here."""
import os
import re

import pytest

from cotengra_amd.plan import KIND_STEM2, compile_tree

import golden_util as G
import stem_variant_cases as V

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cotengra_amd", "csrc", "ctg_stem_impl.h")
# what HipContractor(stem_bf16x3=<arithmetic>) hands to compile_tree: the pairs are priced with fp32 or 16-bit products
PLAN_MODE = {"fp32": False, "bf16x3": True, "fp16x2": True}


@pytest.fixture
def open_model(monkeypatch):
    """Every pair the kernel can run is fused, every capable single step runs on the stem kernel."""
    from cotengra_amd import stem
    G.fuse_whatever_fits(monkeypatch, h2_all=True)
    monkeypatch.setattr(stem, "single_seconds", lambda *a, **k: 0.0)


def stem_record(row, arith):
    plan = compile_tree(row.tree(), "complex64", fuse=True, fuse_min_elems=1 << 10, stem_bf16x3=PLAN_MODE[arith])
    assert plan.nslices == 1 << row.sliced
    steps = [s for s in plan.steps if s.kind == KIND_STEM2]
    assert len(steps) == 1, [s.label for s in plan.steps]
    return steps[0].stem


def assert_planned_as_recorded(row, arith):
    st = stem_record(row, arith)
    got = (st["K1"], st["N1"], st["K2"], st["N2"], st["nr1"], st["items"], st["ng2"], bool(st["vec"]), bool(st.get("one")))
    assert got == row.shape + row.geo[:3] + (bool(row.geo[3]), row.one), (row.id, arith, got)
    # (what the rules derive from the record's other fields is what they derive from the row's)
    rec = row.record()
    assert (st["rows2"], st["ld2"]) == (rec["rows2"], rec["ld2"])
    return st


CASES = [(r, a) for r, a in V.DEVICE_CASES]


@pytest.mark.parametrize("row,arith", CASES, ids=[f"{r.id}-{a}" for r, a in CASES])
def test_rows_are_planned_as_recorded(row, arith, open_model):
    assert_planned_as_recorded(row, arith)


@pytest.mark.parametrize("row", V.DEEP_ROWS, ids=repr)
def test_deep_rows_have_the_tiles_they_say(row, open_model):
    st = assert_planned_as_recorded(row, row.arith)
    assert st["n_tiles"] == row.tiles and row.tiles in (512, 1024)
    assert 1 << row.nq <= 1 << 23
    base = V.by_id(row.base)
    assert (base.args, base.shape, base.geo) == (row.args, row.shape, row.geo)


def test_rows_take_the_entry_they_name():
    """The geometry a row records takes, by the header's rules, the entry the row stands for."""
    for r in V.INST_ROWS:
        assert V.stem_shape(r.record()) == r.args and r.args[5] > 0, r.id
        assert not r.one and V.expected(r, "fp32")[1]["nch"] > 0, r.id
    for r in V.GEO_ROWS:
        assert V.geo_of(V.stem_shape(r.record())) == r.args, r.id
        assert V.has_16bit(r.record()) == r.fits16, r.id   # (the limb planes fit: the row runs on the 16-bit matrix cores)
        assert r.forms == (V.form_of("bf16x3", r.args), V.form_of("fp16x2", r.args)), r.id
    for r in V.ONE_ROWS:
        assert r.one and V.one_key(r.record()) == r.args, r.id
    for r in V.GENERIC_ROWS:
        assert V.generic_key(r.record()) == r.args, r.id
        if not r.env:
            assert not r.one and V.stem_shape(r.record())[5] == 0, r.id   # (items no multiple of the waves)
        else:
            assert r.env == {"CTG_STEM_GENERIC": "1"}, r.id
        assert V.expected(r, "fp32")[1]["nch"] == 0, r.id


def test_forms_of_the_geometries():
    """bf16 x 3: the symmetric form, or the round-4 form with four items per wave; fp16 x 2: specialised waves on the
    27 geometries whose dispatch has them, rerun in the symmetric form under CTG_STEM_FORM=1."""
    for r in V.GEO_ROWS:
        p1, p2, rt1, _, _, it2, _ = r.args
        assert r.forms[0] == (0 if it2 == 4 else 1), r.id
        ws = it2 <= 2 and (p1 or rt1 == 1) and (p2 or it2 < 2)
        assert r.forms[1] == (3 if ws else 0 if it2 == 4 else 1), r.id
    ws_rows = [r for r in V.GEO_ROWS if r.forms[1] == 3]
    assert len(ws_rows) == 27
    assert sorted(r.base for r in V.FORM1_ROWS) == sorted(r.id for r in ws_rows if r.fits16)
    for r in V.FORM1_ROWS:
        kernel, flags = V.expected(r, "fp16x2")
        assert kernel == "stem2h_kernel" and flags["xm"] and not flags["ws"], r.id
        assert V.expected(V.by_id(r.base), "fp16x2")[1]["ws"], r.id


def header_list(macro, letter):
    """The rows of a dispatch list of the header (the full list, behind the development one)."""
    src = open(HEADER, encoding="utf-8").read()
    body = src.split("#define %s(%s)" % (macro, letter))[-1].split("#endif")[0]
    body = body.split("#define ")[0]   # (CTG_STEM_INST is followed by CTG_STEM_GEO inside the same #else)
    conv = {"true": True, "false": False}
    rows = [tuple(conv[a.strip()] if a.strip() in conv else int(a) for a in m.split(","))
            for m in re.findall(r"\b%s\(([^)]*)\)" % letter, body)]
    assert len(set(rows)) == len(rows), (macro, "a row is listed twice")
    return rows


@pytest.mark.parametrize("macro,letter,rows,count", [("CTG_STEM_INST", "X", "INST_ROWS", 47),
                                                     ("CTG_STEM_GEO", "G", "GEO_ROWS", 38),
                                                     ("CTG_STEM_ONE", "X", "ONE_ROWS", 10)])
def test_table_has_the_rows_of_the_header(macro, letter, rows, count):
    listed = header_list(macro, letter)
    table = [r.args for r in getattr(V, rows)]
    assert len(table) == len(set(table)), "a row has two cases"
    assert set(table) == set(listed), (sorted(set(listed) - set(table)), sorted(set(table) - set(listed)))
    assert len(listed) == count


def test_run_time_count_entries_are_all_accounted_for():
    """CTG_STEM_CASE: 16 (P1, P2, RT1, CS1) x the two gathers; CTG_STEM_CASE1: 6 (RT1, CS1) x the two gathers."""
    src = open(HEADER, encoding="utf-8").read()
    pairs = re.findall(r"CTG_STEM_CASE\((true|false), P2, (\d), (\d)\)", src)
    assert len(pairs) == 8
    all_pairs = {(p1 == "true", p2, int(r), int(c), v) for p1, r, c in pairs for p2 in (F_, T_) for v in (F_, T_)}
    (line,) = re.findall(r"((?:CTG_STEM_CASE1\(\d, \d\)\s*)+)#undef CTG_STEM_CASE1", src)
    all_ones = {(int(r), int(c), v) for r, c in re.findall(r"CTG_STEM_CASE1\((\d), (\d)\)", line) for v in (F_, T_)}
    assert len(all_pairs) == 32 and len(all_ones) == 12
    ran = [r.args for r in V.GENERIC_ROWS if r.env]
    assert len(ran) == len(set(ran))
    dead = [e for e, _ in V.UNREACHABLE]
    assert len(dead) == len(set(dead)) and not set(dead) & set(ran)
    assert set(ran) | set(dead) == all_pairs | all_ones
    assert all(isinstance(why, str) and why for _, why in V.UNREACHABLE)
    assert any(not r.env for r in V.GENERIC_ROWS)


F_, T_ = False, True
KS = (16, 32, 64, 128)   # stem.K_OK: the contraction lengths the kernel takes


def test_unreachable_entries_fit_no_lds():
    """The reason UNREACHABLE gives, from stem.geometry's own LDS check: two units per wave with ``cs1`` column groups
    in step 1 is a tile of 2^nr1 rows, nr1 = 5 + log2(16 / cs1); no K1, K2, N2 of the entry's kind fits."""
    from cotengra_amd import stem

    assert KS == stem.K_OK

    def fits(K1, N1, K2, N2, nr1):
        rows2 = (1 << nr1) * N1 // K2
        lds = 2 * rows2 * (K2 + 4) * 4 + stem.b_lds_bytes(K1, N1) + stem.b_lds_bytes(K2, N2) + 8 * N2 + stem.LDS_SLACK
        return rows2 >= 32 and lds <= stem.LDS_BYTES

    def any_fits(p2, cs1):
        nr1 = 5 + {2: 3, 4: 2}[cs1]
        return any(fits(K1, 32 * cs1, K2, N2, nr1) for K1 in KS for K2 in KS for N2 in ((16,) if p2 else (32, 64, 128)))

    for (p1, p2, rt1, cs1, _), _ in V.UNREACHABLE:
        assert not p1 and rt1 == 2 and not any_fits(p2, cs1), (p2, cs1)
    assert any_fits(True, 2)   # (RP_ft22f, RP_ft22t: the one kind that is reached)


def test_geometries_whose_limb_planes_never_fit():
    """``fits16=False``: for every (K2, N2) that gives the geometry its item count the 16-bit kernel's LDS
    (stem2_lds_bytes_bf3) is more than 160 KB, so stem2_bf3 refuses and the instantiation is never launched."""
    never = [r for r in V.GEO_ROWS if not r.fits16]
    assert [r.id for r in never] == ["G16", "G26"]
    for r in V.GEO_ROWS:
        p1, p2, rt1, cs1, nch, it2, vec = r.args
        K1, N1 = 16 * nch, 16 if p1 else 32 * cs1
        nr1 = 5 + (rt1 * V.SW // cs1).bit_length() - 1
        sizes = []
        for N2 in ((16,) if p2 else (32, 64, 128)):
            ng2 = max(1, N2 // 32)
            if (it2 * V.SW) % ng2:
                continue
            rows2 = it2 * V.SW // ng2 * 32
            K2 = (1 << nr1) * N1 // rows2
            if K2 in KS and K2 * rows2 == (1 << nr1) * N1:
                st = dict(K1=K1, N1=N1, K2=K2, N2=N2, rows2=rows2, ld2=K2 + 4, one=0)
                sizes.append(V.lds_bytes_16bit(st))
        assert sizes, r.id
        assert (min(sizes) <= V.LDS) == r.fits16, (r.id, sizes)


@pytest.mark.parametrize("row", V.SLICED_ROWS, ids=repr)
def test_sliced_rows_are_planned_as_recorded(row, open_model):
    assert_planned_as_recorded(row, row.arith)


def test_ids_are_unique():
    ids = [r.id for r in V.ALL_ROWS]
    assert len(set(ids)) == len(ids)
    for r in V.ALL_ROWS:
        assert V.by_id(r.id) is r
        assert 15 <= r.nq - r.sliced <= 18 or r in V.DEEP_ROWS, r.id


def test_sliced_rows_keep_their_shape():
    """One row per kernel family with the first tensor's leading index sliced: the same entry, two slices."""
    kinds = set()
    for r in V.SLICED_ROWS:
        base = V.by_id(r.base)
        assert r.sliced == 1 and (r.args, r.shape, r.geo) == (base.args, base.shape, base.geo), r.id
        kinds.add(r.family)
    assert kinds == {"inst_ri2", "inst_xy", "form3", "form1", "form0", "single"}
    assert len(V.SLICED_ROWS) == 6
