"""Stem kernels on specialised waves, operand rows shared between column groups (csrc/ctg_stem_impl.h: SH1).

With 64 columns in step 1 a 32-row tile of the big operand is multiplied into two 32-column groups.  A producer wave
takes a row tile and BOTH its column groups: one gather and one split per (row tile, chunk), where each of two waves
used to gather and split the same rows for its own group.  The pairs here are the shapes that take this dealing
(``cs1 == 2`` on ``ws``) and the pairs with a 64-column second step on specialised waves, whose consumers hold two
items of one row tile; each in three sizes of the running tensor, so that a workgroup has one tile (the tail of a
two-tile pass alone), two and four (a workgroup's tile count is a power of two: the only odd one is 1).

The dealing changes which wave multiplies which unit, not the order in which an accumulator sees its products: the
result is compared with the complex128 oracle under the single-precision gate.  The symmetric kernel
(``CTG_STEM_FORM=1``) runs step 1 with a two-accumulator real part (X = Xp - Xm) where a producer of the specialised
form flips the sign of Im a, so the two forms round differently and did so before this dealing existed (measured on
the commit before it: all 30 cases differ in bits between the forms); the symmetric form is therefore held to the same
gate, not to the same bits."""
import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd.contractor import HipContractor
from oracle import contract_ref as orc

import golden_util as G

pytestmark = pytest.mark.gpu

# (name, gates of the pair, log2 of the elements of the running tensor one tile takes, what must have run)
#   tile = (256 / column groups of step 1) rows x K1
PAIRS = [
    ("k64n64_k32n32", [(6, 6), (5, 5)], 13, "cs1"),
    ("k64n64_k16n16", [(6, 6), (4, 4)], 13, "cs1"),
    ("k32n64_k64n64", [(5, 6), (6, 6)], 12, "cs1+n64"),
    ("k32n32_k64n64", [(5, 5), (6, 6)], 13, "n64"),
    ("k64n32_k64n64", [(6, 5), (6, 6)], 14, "n64"),
]
# tiles of a slice: 256 (one per workgroup), 512, 1024
TILES_LOG2 = [8, 9, 10]
# Which indices a gate contracts is drawn from the seed, and with it the geometry the planner finds (a sliced index may be
# one a gate contracts).  The first seeds with which the pair takes the shape its name says -- unsliced, two indices sliced:
SEEDS = [(0, 1), (0, 2), (0, 1), (0, 1), (0, 1)]


@pytest.fixture
def fuse_whatever_fits(monkeypatch):
    from cotengra_amd import stem
    monkeypatch.setattr(stem, "gather_rate", lambda run_bytes: 5.4e12)
    for k in ("CTG_STEM_ARITH", "CTG_STEM_BF16X3", "CTG_STEM_H2", "CTG_STEM_FORM"):
        monkeypatch.delenv(k, raising=False)
    # (every capable pair in fp16 x 2, the first one of a stem too: a max-abs pass supplies its scale)
    monkeypatch.setenv("CTG_STEM_H2_ALL", "1")


def _stem_names(fn, arrays):
    return [n for n in fn.setup(*arrays)["exec"].step_kernels() if n.startswith(("stem2_kernel", "stem2h_kernel"))]


def build_case(pair, tiles_log2, sliced):
    """The stem (3, 3) + the pair on a running tensor of tiles x tile elements per slice, and its arrays."""
    name, gates, tile_log2, _ = PAIRS[pair]
    nq = tile_log2 + tiles_log2 + sliced
    tree = G.stem_network(nq, [(3, 3)] + gates, SEEDS[pair][1 if sliced else 0], sliced=sliced)
    arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=pair, dtype="complex64")
    return tree, arrays


def run_case(tree, arrays):
    fn = HipContractor(tree, fuse=True, fuse_min_elems=1 << 10)
    try:
        got = np.asarray(fn(*arrays))
        names = _stem_names(fn, arrays)
    finally:
        fn.close()
    return got, names


@pytest.mark.parametrize("sliced", [0, 2])
@pytest.mark.parametrize("tiles_log2", TILES_LOG2)
@pytest.mark.parametrize("pair", range(len(PAIRS)))
def test_stem_pairs_with_shared_rows(pair, tiles_log2, sliced, fuse_whatever_fits, monkeypatch):
    name, gates, _, what = PAIRS[pair]
    tree, arrays = build_case(pair, tiles_log2, sliced)
    assert tree.nslices == (1 << sliced)
    ref = np.asarray(orc.contract(tree, [a.astype("complex128") for a in arrays]))
    gate = G.single_gate(ref, orc.contract(tree, arrays))
    got, names = run_case(tree, arrays)
    flags = [G.stem_flags(n) for n in names if n.startswith("stem2h_kernel")]
    # (specialised waves, and the first contraction as deep as the case says: 16 per chunk)
    ws = [f for f in flags if f["ws"] and not f["one"] and f["nch"] == (1 << gates[0][0]) // 16]
    print(name, tiles_log2, sliced, names)
    # the kernel this case is about really ran
    if "cs1" in what:
        assert any(f["cs1"] == 2 for f in ws), names
    if "n64" in what:
        # (64 columns in step 2 on specialised waves: 32-column items, one per wave of the symmetric kernel)
        assert any(not f["pack2"] and f["it2"] == 1 for f in ws), names
    if what == "cs1+n64":
        assert any(f["cs1"] == 2 and not f["pack2"] and f["it2"] == 1 for f in ws), names
    err = G.relerr(got, ref)
    print("relerr", err, "gate", gate)
    assert err <= gate, (err, gate)
    # the symmetric kernel of the same pair: the same gate (its bits differ, see the module's docstring)
    monkeypatch.setenv("CTG_STEM_FORM", "1")
    sym, names1 = run_case(tree, arrays)
    assert not any(G.stem_flags(n)["ws"] for n in names1), names1
    err1 = G.relerr(sym, ref)
    print("symmetric relerr", err1, "same bits", bool(np.array_equal(sym, got)))
    assert err1 <= gate, (err1, gate)
