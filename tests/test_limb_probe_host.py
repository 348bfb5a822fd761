"""Why the device owes the limb probes bit for bit (tests/limb_probe.py, run on the device by
tests/test_gpu_limb_probes.py), proved on the host for every row and both probes:

rounding     the emulated round-to-nearest-even agrees with torch.bfloat16 / numpy.float16 conversion, ties included;
split        the emulated split returns the limbs the probe values were built from, and the limbs sum back to the value;
any order    every stage's kept products are multiples of a quantum q with sum |terms| < 2^24 q -- so every partial sum
             in every order is an fp32 number -- and every stage's value is an fp32 number;
scale        an fp16 x 2 stage gives the same value under twice and half the scale (the intermediate's scale is per
             tile on the device, per tensor in the model: all of a probe's values lie within a factor of two);
non-zero     every output of the chain is non-zero;
sensitive    with any one product a stage multiplies left out, the chain's model differs in EVERY output element (the
             stage that multiplies limbs with limbs: all kept products; a unit stage: the products with the unit's one
             limb, where the other limb is not zero), and with a dropped product wrongly included it differs wherever
             that product is more than half a unit in the last place of the value.

The plans of the rows do not depend on the data: tests/test_stem_variant_plans.py pins them (imported, not repeated).
The deep rows (2^21 to 2^23 elements) are modelled in fp32 planes (limb_probe.chain_model32: under the any-order
condition, asserted here on the whole data, an fp32 sum IS the float64 sum; for every other row the two models are
compared directly).  Their float64 model and the sensitivity part run on the elements of the state with the leading
uncontracted indices at 0 (limb_probe.restrict: 2^16 elements, the same gates), after asserting that the restricted
float64 model is that part of the whole fp32-plane one."""
import functools
import itertools

import numpy as np
import pytest

import limb_probe as L
import pair_variant_cases_c64 as C
import stem_variant_cases as V
import test_stem_variant_plans  # noqa: F401  (the rows' plans, pinned there)

STEM_CASES = L.stem_cases()
SMALL = 1 << 16


# ---------------------------------------------------------------------------------------------------------------- #
# rounding and splits
# ---------------------------------------------------------------------------------------------------------------- #
def random_floats_with_ties(bits_kept):
    """A few thousand fp32 numbers: random ones over many binades, and exact ties of a format that keeps
    ``bits_kept`` significant bits (odd and even neighbours)."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4096) * 2.0 ** rng.integers(-12, 13, size=4096)).astype(np.float32)
    m = rng.integers(1 << (bits_kept - 1), 1 << bits_kept, size=2048).astype(np.float64)
    ties = (m + 0.5) * 2.0 ** rng.integers(-10 - bits_kept, 4, size=2048) * rng.choice([-1.0, 1.0], size=2048)
    ties = ties.astype(np.float32)
    return np.concatenate([x, ties, np.float32([0.0, -0.0, 1.0, -1.0])])


def test_rn_bf16_is_torch():
    import torch
    x = random_floats_with_ties(8)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(L.rn_bf16(x).view(np.uint32), want.view(np.uint32))
    # (the ties are ties: both neighbours are equally far, and the even one is taken)
    t = x[4096:4096 + 2048].astype(np.float64)
    r = L.rn_bf16(x[4096:4096 + 2048]).astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.abs(t))) - 7)
    assert np.all(np.abs(r - t) == ulp / 2) and np.all((r / ulp) % 2 == 0)


def test_rn_fp16_is_numpy():
    x = random_floats_with_ties(11)
    x = x[np.abs(x) < 6e4]
    assert np.array_equal(L.rn_fp16(x), x.astype(np.float16).astype(np.float32))
    t = x[(np.abs(x) >= 2.0 ** -10)].astype(np.float64)
    r = L.rn_fp16(t.astype(np.float32)).astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.abs(t))) - 10)
    assert np.all(np.abs(r - t) <= ulp / 2)
    tie = np.abs(r - t) == ulp / 2
    assert tie.sum() > 1000 and np.all((r[tie] / ulp[tie]) % 2 == 0)


@pytest.mark.parametrize("arith", L.ARITHS)
def test_split_returns_the_chosen_limbs(arith):
    rng = np.random.default_rng(3)
    x, limbs = L.probe_values(rng, (100000,), arith, with_limbs=True)
    L.f32(x)
    if arith == "bf16x3":
        got = [L.split_bf16x3(x)]
    else:
        got = [[h / s for h in L.split_fp16x2(x, s)] for s in (1.0, 2.0 ** 12, 2.0 ** 13)]
    for g in got:
        for k, (a, b) in enumerate(zip(g, limbs)):
            assert np.array_equal(a.astype(np.float64), b), (arith, k)
    # every combination of mantissas and signs occurs
    assert len(np.unique(x)) == np.prod([2 * len(m) for m, _ in L.PROBE_LIMBS[arith]])


def test_kept_products_are_the_header_s():
    """KEPT restates bf3_ta / bf3_tb and Fp16x2::t_step."""
    ta = lambda t: 0 if t < 3 else (2 if t == 5 else 1)           # noqa: E731
    tb = lambda t: 1 if t in (1, 4) else (2 if t == 2 else 0)     # noqa: E731
    assert L.KEPT["bf16x3"] == tuple((ta(t), tb(t)) for t in range(6))
    walk, t = [], 0
    while t < 6:
        walk.append(t)
        t += 2 if t == 1 else (3 if t == 3 else 1)
    assert walk == [0, 1, 3] and L.KEPT["fp16x2"] == tuple((ta(t), tb(t)) for t in walk)
    for a in L.ARITHS:
        n = L.LIMBS[a]
        assert set(L.KEPT[a]) | set(L.DROPPED[a]) == set(itertools.product(range(n), range(n)))


def test_any_order_of_the_six_accumulations():
    """All 720 orders of the six fp32 accumulations of a bf16 x 3 product of probe values give the model's bits."""
    rng = np.random.default_rng(9)
    a, b = L.probe_values(rng, (4096,), "bf16x3"), L.probe_values(rng, (4096,), "bf16x3")
    la, lb = L.split_bf16x3(a), L.split_bf16x3(b)
    terms = [la[i] * lb[j] for i, j in L.KEPT["bf16x3"]]   # (fp32 products of bf16 numbers: exact)
    want = sum(t.astype(np.float64) for t in terms)
    for order in itertools.permutations(range(6)):
        acc = np.zeros(4096, dtype=np.float32)
        for t in order:
            acc = acc + terms[t]
        assert np.array_equal(acc.astype(np.float64), want), order


# ---------------------------------------------------------------------------------------------------------------- #
# the conditions, per stage
# ---------------------------------------------------------------------------------------------------------------- #
def assert_any_order_exact(rec, what):
    """Stage record -> the quantum's exponent: every kept product a multiple of q = 2^rec.q (by construction: the
    product of the limbs' lowest bits), sum |terms| < 2^24 q, the value an fp32 number."""
    L.f32(rec.out.real), L.f32(rec.out.imag)
    if rec.q is None:
        return None
    assert rec.total < 2.0 ** (24 + rec.q), (what, rec.q, rec.total)
    return rec.q


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return 2.0 ** (np.floor(np.log2(np.where(x == 0, 1.0, x))) - 23)


@functools.lru_cache(maxsize=None)
def check_chain(network, gates, one, ariths, probe, seed):
    """Every condition of the module's docstring for one chain; returns what it found (shared by the rows of one
    network that run in the same arithmetic)."""
    import golden_util as G
    nq, _, net_seed, sliced = network
    assert sliced == 0
    tree = G.stem_network(nq, [(3, 3)] + list(gates), net_seed)
    ariths = list(ariths)
    karith = ariths[-1]
    values = L.VALUES_OF[karith]
    arrays = L.chain_arrays(tree, gates, probe, values, seed)
    for a in arrays:
        L.f32(a.real), L.f32(a.imag)
    hot = {"S1": 1, "S2": 2}[probe]
    what = (network, karith, probe)

    # the state's limbs are the chosen ones: all non-zero, and they sum back to the value
    if karith != "fp32":
        limbs, scale = L.limbs_of(arrays[0], karith)
        assert all(np.all(x.real != 0) and np.all(x.imag != 0) for x in limbs), what
        assert np.array_equal(sum(limbs) / scale, arrays[0]), what

    large = arrays[0].size > L.LARGE
    if large:
        # (the fp32-plane form of the model: the conditions on the whole data, the float64 model on a part below)
        bounds = []
        model = L.chain_model32(tree, arrays, ariths, bounds)   # (what model_c64 gives the device test)
        quanta = []
        for s, (q, total) in enumerate(bounds):
            assert q is None or total < 2.0 ** (24 + q), (what, s, q, total)
            quanta.append(q)
    else:
        model, recs = L.chain_model(tree, arrays, ariths, details=True)
        assert len(recs) == len(ariths)
        quanta = [assert_any_order_exact(r, what + (s,)) for s, r in enumerate(recs)]
        assert np.array_equal(L.chain_model32(tree, arrays, ariths), L.to_c64(model)), what
        assert np.array_equal(L.model_c64(tree, arrays, ariths), L.to_c64(model)), what
    found = {"quanta": quanta}
    assert np.all(model.real != 0) and np.all(model.imag != 0), what
    if karith == "fp32":
        # the control: the rounded exact product (complex128 holds a product of two 24-bit numbers exactly)
        from oracle import contract_ref as orc
        exact = np.asarray(orc.contract(tree, arrays))
        assert np.array_equal(model, exact.astype(np.complex64).astype(np.complex128)), what
        return found
    # scale and sensitivity, on at most 2^16 elements of the state
    net, sub, index = (tree, arrays, None) if arrays[0].size <= SMALL else L.restrict(tree, arrays, SMALL)
    base, sub_recs = L.chain_model(net, sub, ariths, details=True)
    if index is not None:
        assert sub[0].size == SMALL and np.array_equal(base, model[index]), what
        for s, r in enumerate(sub_recs):
            assert_any_order_exact(r, what + (s, "part"))
    if karith == "fp16x2":
        for s in range(1, len(ariths)):
            for shift in (-1, 1):
                assert np.array_equal(L.chain_model(net, sub, ariths, scale_shift={s: shift}), base), (what, s, shift)

    def differs(other):
        return (other.real != base.real) | (other.imag != base.imag)

    shares = {}
    for s in range(1, len(ariths)):
        for ij in L.KEPT[karith]:
            if s != hot and ij[1] != 0:
                continue   # (a unit has one limb: the product is zero, nothing to leave out)
            kept = tuple(p for p in L.KEPT[karith] if p != ij)
            share = float(differs(L.chain_model(net, sub, ariths, kept={s: kept})).mean())
            shares[(s, ij)] = share
            if s == hot or probe == "S2" or ij == (0, 0):
                # (limbs with limbs; or a unit stage in front of it, fed by the state's chosen limbs)
                assert share == 1.0, f"{what}: without product {ij} of stage {s}, {100 * share:.4f} % of the elements differ"
            else:
                # a unit stage behind the products splits a 24-bit value: its second (third) limb is zero where 11 (8)
                # or more bits of the value happen to be zero -- 2^-8 (2^-7) of the elements at random; 95 % is far off
                assert share >= 0.95, f"{what}: without product {ij} of stage {s}, {100 * share:.4f} % of the elements differ"
    # a dropped product wrongly included: visible wherever it is more than half an ulp of the value
    # (of the stage that multiplies limbs with limbs, in that stage's result)
    rec = sub_recs[hot]
    for ij in L.DROPPED[karith]:
        extra = L.stage(*stage_inputs(net, sub, ariths, hot), karith, kept=(ij,))
        with_it = rec.out + extra
        moved = ((with_it.real.astype(np.float32) != rec.out.real.astype(np.float32))
                 | (with_it.imag.astype(np.float32) != rec.out.imag.astype(np.float32)))
        owed = (np.abs(extra.real) > ulp32(rec.out.real) / 2) | (np.abs(extra.imag) > ulp32(rec.out.imag) / 2)
        shares[("extra", ij)] = (float(moved.mean()), float(owed.mean()))
        assert np.all(moved[owed]), (f"{what}: with the dropped product {ij}, {100 * moved.mean():.2f} % of the elements "
                                     f"differ; it is above half an ulp in {100 * owed.mean():.2f} %")
    found["shares"] = shares
    return found


def stage_inputs(net, arrays, ariths, s):
    """``(a[R, K], b[K, N])`` of stage ``s`` of the chain, the stages in front of it run by the model."""
    cur, x = list(net.inputs[0]), np.asarray(arrays[0])
    for t, (inds, g) in enumerate(zip(net.inputs[1:], arrays[1:])):
        k = sum(1 for ix in inds if ix in cur)
        if t == s:
            keep = [c for c in cur if c not in inds[:k]]
            a = np.transpose(x, [cur.index(c) for c in keep + list(inds[:k])]).reshape(-1, 1 << k)
            return a, np.asarray(g).reshape(1 << k, -1)
        cur, x = L.apply_gate(cur, x, inds, k, g, lambda a, b, t=t: L.stage(a, b, ariths[t]))
    raise AssertionError(s)


@pytest.mark.parametrize("row,arith", STEM_CASES, ids=[f"{r.id}-{a}" for r, a in STEM_CASES])
def test_stem_row_owes_bits(row, arith):
    assert not row.sliced
    for probe in L.probes_of(row):
        found = check_chain(row.network, tuple(row.gates), row.one, tuple(L.stage_ariths(row, arith)), probe,
                            L.probe_seed(row, probe))
        print(row.id, arith, probe, found)


def test_every_16_bit_row_is_probed():
    ids = {(r.id, a) for r, a in STEM_CASES}
    for r, a in V.DEVICE_CASES:
        assert (a == "fp32") != ((r.id, a) in ids)
    for r in V.DEEP_ROWS:
        assert (r.arith == "fp32") != ((r.id, r.arith) in ids)
    # the geometries whose limb planes do not fit run fp32 products in every arithmetic: probed as the control
    fp32 = sorted({r.id for r, a in STEM_CASES if L.kernel_arith(r, a) == "fp32"})
    assert fp32 == ["G16", "G26", "O01"], fp32


# ---------------------------------------------------------------------------------------------------------------- #
# the plain pair of the 16-bit pipe
# ---------------------------------------------------------------------------------------------------------------- #
PAIR_ARITH = {"P_bf3": "bf16x3", "P_h2": "fp16x2", "P_h2_f": "fp16x2", "P_fast": "fp32"}


@pytest.mark.parametrize("ident", sorted(PAIR_ARITH))
def test_pair_row_owes_bits(ident):
    case, arith = C.by_id(ident), PAIR_ARITH[ident]
    R, _, K, N = case.step
    assert (R, K, N) == (8192, 64, 512)
    a, b = L.pair_arrays(R, K, N, L.VALUES_OF[arith], case.seed)
    rec = L.stage(a, b, arith, details=True)
    assert_any_order_exact(rec, ident)
    assert np.all(rec.out.real != 0) and np.all(rec.out.imag != 0)
    if arith == "fp32":
        assert np.array_equal(rec.out, (a @ b).astype(np.complex64).astype(np.complex128))
        return
    for shift in (-1, 1):
        assert np.array_equal(L.stage(a, b, arith, scale_shift=shift), rec.out)
    for ij in L.KEPT[arith]:
        other = L.stage(a, b, arith, kept=tuple(p for p in L.KEPT[arith] if p != ij))
        share = float(((other.real != rec.out.real) | (other.imag != rec.out.imag)).mean())
        assert share == 1.0, f"{ident}: without product {ij}, {100 * share:.4f} % of the elements differ"
