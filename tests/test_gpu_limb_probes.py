"""The 16-bit arithmetics of the stem kernels and of the tiled pair kernels, every limb product probed BIT FOR BIT.

tests/test_gpu_stem_variants.py and tests/test_gpu_pair_variants_c64.py pin each instantiation by name; by value they
hold random data to a gate of 1e-5 -- a limb product of bf16 x 3 left out, paired with the wrong limb or read from the
wrong plane is 2e-6 of ONE product -- and integer data bit for bit -- where every operand fits one limb and the planes
of the second and third limbs hold zeros.  Here the operands are limb probes (tests/limb_probe.py): every limb of
both operands of one stage is populated, every output is a single product, and the device must return the numpy model
of the documented split and product list exactly.  tests/test_limb_probe_host.py proves on the host, row by row, that
the bits are owed (any accumulation order is exact) and that any one missing product changes every output element.

stem rows   every 16-bit (row, arithmetic) of stem_variant_cases.DEVICE_CASES and the deep rows in their arithmetic,
            under the environment of test_gpu_stem_variants: the kernel's name (assert_named), then probe S1 (state
            and B1 carry probe values, B2 is a unit) and S2 (state and B2; B1 a unit) against the chain's model.  The
            three geometries whose limb planes do not fit (G16, G26, O01) run fp32 products in every arithmetic:
            their model is the rounded exact product.  The sliced rows are left out: a sum of two slices rounds.
pairs       P_bf3, P_h2, P_h2_f of pair_variant_cases_c64 (8192 x 64 x 512): A dense probe values, B one per column.
            P_h2_f slices the fastest index of A: each of its three slices is a product of its own.
controls    the same data through fp32 products -- one S1 probe per fp32 stem kernel of DEVICE_CASES and P_fast
            (pair_mfma_fast_kernel) -- against the rounded exact product: a failure there is the data's or the
            model's, not a 16-bit arithmetic's."""
from collections import OrderedDict

import numpy as np
import pytest

import golden_util as G
import limb_probe as L
import pair_variant_cases_c64 as C
import stem_variant_cases as V
from cotengra_amd.contractor import HipContractor
from cotengra_amd.plan import KIND_STEM2
from test_gpu_pair_variants_c64 import assert_variant, set_env as set_pair_env
from test_gpu_stem_valu_paths import stem_env  # noqa: F401  (the fixture: every capable step on the stem kernels)
from test_gpu_stem_variants import assert_exact, assert_named, contractor, set_env, stem_names

pytestmark = pytest.mark.gpu

STEM_CASES = L.stem_cases()
# one fp32 case per kernel name the table expects (rows of one instantiation under another seed run the same kernel)
_seen = set()
FP32_CONTROLS = []
for _r, _a in V.DEVICE_CASES:
    _key = repr(V.expected(_r, _a))
    if _a == "fp32" and _key not in _seen:
        _seen.add(_key)
        FP32_CONTROLS.append(_r)

_DATA = OrderedDict()


def probe_of(row, arith, probe):
    """(tree, complex64 inputs, the model's complex64 result): computed once per network, arithmetic and probe (rows
    of one network follow each other), never modified."""
    ariths = L.stage_ariths(row, arith)
    key = (row.network, tuple(ariths), probe)
    if key not in _DATA:
        tree = row.tree()
        arrays = L.chain_arrays(tree, row.gates, probe, L.VALUES_OF[ariths[-1]], L.probe_seed(row, probe))
        want = L.model_c64(tree, arrays, ariths)
        assert np.all(want.real != 0) and np.all(want.imag != 0)
        arrays = [L.to_c64(a) for a in arrays]
        for x in arrays + [want]:
            x.setflags(write=False)
        _DATA[key] = (tree, arrays, want)
        while len(_DATA) > 4:
            _DATA.popitem(last=False)
    return _DATA[key]


def run_probes(row, arith, probes, monkeypatch, tiles=None):
    set_env(monkeypatch, row)
    tree = row.tree()
    fn = contractor(tree, arith)
    got, names = {}, None
    try:
        for probe in probes:
            _, arrays, _ = probe_of(row, arith, probe)
            got[probe] = np.asarray(fn(*arrays))
            if names is None:
                names = stem_names(fn, arrays)
                if tiles is not None:
                    assert [s.stem["n_tiles"] for s in fn.setup(*arrays)["plan"].steps if s.kind == KIND_STEM2] == [tiles]
            else:
                assert stem_names(fn, arrays) == names
    finally:
        fn.close()
    assert_named(row, arith, names)
    for probe in probes:
        assert_exact(row, f"{arith} {probe}", got[probe], probe_of(row, arith, probe)[2])


@pytest.mark.parametrize("row,arith", STEM_CASES, ids=[f"{r.id}-{a}" for r, a in STEM_CASES])
def test_stem_limb_products(row, arith, stem_env, monkeypatch):
    run_probes(row, arith, L.probes_of(row), monkeypatch, tiles=getattr(row, "tiles", None))


@pytest.mark.parametrize("row", FP32_CONTROLS, ids=repr)
def test_stem_fp32_control(row, stem_env, monkeypatch):
    run_probes(row, "fp32", ("S1",), monkeypatch)


PAIR_ARITH = {"P_bf3": "bf16x3", "P_h2": "fp16x2", "P_h2_f": "fp16x2", "P_fast": "fp32"}
_PAIR = {}


def pair_probe(case, arith):
    """(operands of the case's equation, the model's result per slice)."""
    key = (case.id, arith)
    if key not in _PAIR:
        _PAIR.clear()
        R, _, K, N = case.step
        nsl = case.sizes.get("s", 1)
        rng_seed = case.seed
        parts = [L.pair_arrays(R, K, N, L.VALUES_OF[arith], rng_seed + 7 * i) for i in range(nsl)]
        b = parts[0][1]
        want = [L.to_c64(L.stage(a, b, arith)) for a, _ in parts]
        a = np.stack([a for a, _ in parts], axis=-1) if "s" in case.sizes else parts[0][0]
        assert a.shape == tuple(case.sizes[i] for i in case.ta) and b.shape == tuple(case.sizes[i] for i in case.tb)
        _PAIR[key] = ([L.to_c64(a), L.to_c64(b)], want)
    return _PAIR[key]


@pytest.mark.parametrize("ident", ["P_bf3", "P_h2", "P_h2_f", "P_fast"])
def test_pair_limb_products(ident, monkeypatch):
    case, arith = C.by_id(ident), PAIR_ARITH[ident]
    assert case.eq in ("ak,kn->an", "aks,kn->an")
    arrays, want = pair_probe(case, arith)
    set_pair_env(monkeypatch, case)
    fn = HipContractor(case.tree(sliced=case.sliced))
    try:
        names = [n for n in fn.setup(*arrays)["exec"].step_kernels() if n.startswith("pair_")]
        assert len(names) == 1, names
        print(f"KERNEL {case.id} {names[0]}")
        if case.sliced:
            got = [np.asarray(fn.contract_slice(arrays, i)) for i in range(len(want))]
        else:
            got = [np.asarray(fn(*arrays))]
    finally:
        fn.close()
    assert_variant(G.pair_flags_c64(names[0]), case)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_exact(case, f"{arith} slice {i}", g, w)
