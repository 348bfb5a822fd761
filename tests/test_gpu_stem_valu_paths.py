"""The vector paths of the 16-bit stem kernels (csrc/ctg_stem_impl.h): the split of an operand into limbs and the factors
the stores apply, in both arithmetics (fp16 x 2 and bf16 x 3).

fp16 x 2 splits with v_fma_mixlo_f16 / v_fma_mixhi_f16 (two instructions per value, the pair of a word packed by the
instructions themselves); the stores of both arithmetics multiply by two powers of two, the second one live only where
the total exponent leaves +-126.  Neither may lose a bit:

(a) one pair of every kernel family the headline tree launches -- specialised waves with one and with two column groups
    in step 1, 16 columns in step 1 (PACK1), 16 columns in step 2 (PACK2), a single step, a symmetric pair -- against
    the complex128 oracle under the suite's single-precision gate;
(b) powers of two: inputs scaled by exact powers of two give the scaled result, bit for bit -- with the powers chosen so
    that BOTH store factors are live (see the test's docstring for where the power has to sit);
(c) limb edges: exact fp16 ties of both residual signs, zeros (negative ones in the small operands only: the split's
    operand is always a kernel's result and cannot hold one) and a largest element one ulp below a power of two, against a host emulation of the two-limb product that must give the same bits.

Running tensors of 2^15 elements (four tiles: more than one workgroup), CTG_FUSE_MIN_ELEMS=4096."""
import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd.contractor import HipContractor
from oracle import contract_ref as orc

import golden_util as G

pytestmark = pytest.mark.gpu

NQ = 15
PREFIX = [(3, 3)]   # (the first step of a chain is an ordinary pair step: the stem kernel's big operand is its result)
# family -> (gates of the stem step(s), seed of the network, CTG_STEM_FORM or None, what the fp16 x 2 kernel's name must say)
FAMILIES = {
    "ws_cs1": ([(5, 5), (6, 6)], 0, None, dict(ws=True, cs1=1, pack1=False, pack2=False, one=False)),
    "ws_cs2": ([(6, 6), (5, 5)], 0, None, dict(ws=True, cs1=2, pack1=False, pack2=False, one=False)),
    "pack1": ([(4, 4), (5, 5)], 0, None, dict(pack1=True, one=False)),
    "pack2": ([(5, 5), (4, 4)], 0, None, dict(pack2=True, one=False)),
    "single": ([(5, 5)], 0, None, dict(one=True)),
    "symmetric": ([(5, 5), (6, 6)], 0, "1", dict(ws=False, pack1=False, pack2=False, one=False)),
}
# (b): four inputs share the power of two, so the single step comes behind two small gates
LIVE_FAMILIES = dict(FAMILIES, single=([(3, 3), (5, 5)], 0, None, dict(one=True)))
ARITHS = ["fp16x2", "bf16x3"]


@pytest.fixture
def stem_env(monkeypatch):
    """Every capable step on the stem kernel (single steps too), every capable pair in fp16 x 2 unless the contractor
    says bf16 x 3, the fusion threshold of the module's docstring."""
    from cotengra_amd import stem
    G.fuse_whatever_fits(monkeypatch, h2_all=True)
    monkeypatch.setattr(stem, "single_seconds", lambda *a, **k: 0.0)
    monkeypatch.delenv("CTG_STEM_FORM", raising=False)
    monkeypatch.setenv("CTG_FUSE_MIN_ELEMS", "4096")


def network(family, upto=None, families=None):
    gates, seed, _, _ = (families or FAMILIES)[family]
    return G.stem_network(NQ, (PREFIX + gates)[:upto], seed)


_ORACLE = {}


def oracle_of(family, families=None):
    """(tree, arrays, complex128 reference, numpy's complex64 result): computed once per family, never modified."""
    key = (family, "live" if families is not None else "")
    if key not in _ORACLE:
        tree = network(family, families=families)
        arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=7, dtype="complex64")
        ref = np.asarray(orc.contract(tree, [a.astype("complex128") for a in arrays]))
        for x in arrays:
            x.setflags(write=False)
        _ORACLE[key] = (tree, arrays, ref, np.asarray(orc.contract(tree, arrays)))
    return _ORACLE[key]


def contractor(tree, arith):
    return HipContractor(tree, fuse=True, **({"stem_bf16x3": "bf16x3"} if arith == "bf16x3" else {}))


def run(fn, arrays, **kw):
    out = fn(*arrays, **kw)
    names = [n for n in fn.setup(*arrays)["exec"].step_kernels() if n.startswith(("stem2_kernel", "stem2h_kernel"))]
    return out, names


def assert_family_ran(family, arith, names, families=None):
    """The stem kernel of the family ran, in the arithmetic asked for."""
    assert len(names) == 1, names
    flags = G.stem_flags(names[0])
    assert flags["bf3"], names
    want = dict((families or FAMILIES)[family][3])
    if arith == "fp16x2":
        assert names[0].startswith("stem2h_kernel"), names
    else:
        assert names[0].startswith("stem2_kernel"), names
        # (three limbs: the symmetric form is the only one -- Bf16x3::max_form -- and it deals column groups its own way)
        want.pop("ws", None)
        want.pop("cs1", None)
        assert not flags["ws"], names
    assert {k: flags[k] for k in want} == want, (names, want)


def top_of(x):
    x = np.asarray(x)
    return float(max(np.abs(x.real).max(), np.abs(x.imag).max()))


# ---------------------------------------------------------------------- #
# (a) one pair of every family against the oracle
# ---------------------------------------------------------------------- #


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_pair_families_against_oracle(family, arith, stem_env, monkeypatch):
    tree, arrays, ref, np64 = oracle_of(family)
    if FAMILIES[family][2] is not None:
        monkeypatch.setenv("CTG_STEM_FORM", FAMILIES[family][2])
    fn = contractor(tree, arith)
    try:
        got, names = run(fn, arrays)
    finally:
        fn.close()
    assert_family_ran(family, arith, names)
    err, gate = G.relerr(np.asarray(got), ref), G.single_gate(ref, np64)
    print(family, arith, names, "relerr", err, "gate", gate)
    assert err <= gate, (err, gate)


# ---------------------------------------------------------------------- #
# (b) powers of two
# ---------------------------------------------------------------------- #


def h2_exponent(top):
    """What the fp16 x 2 kernels take out of an operand whose largest |component| is ``top`` (h2_exponent_of,
    Fp16x2::operand_exponent): the power of two that brings it to [2^13, 2^14)."""
    return int(np.floor(np.log2(top))) - 13


@pytest.mark.parametrize("family", list(LIVE_FAMILIES))
def test_fp16x2_second_store_factor_live(family, stem_env, monkeypatch):
    """fp16 x 2 stores x 2^E as two factors, E = (exponents taken out of A, B1, B2) + (exponent of the intermediate
    tile); the second factor is live where E < -126.  E counts the BIG operand too, so inputs whose powers cancel
    (B1, B2 x 2^-70, A x 2^+140) leave E where it was, and the upload takes out of an input whatever leaves
    [2^-32, 2^32): the power that survives is one spread over ALL FOUR inputs, each inside the upload window, that
    brings the RESULT to about 2^-104.  The big operand of the stem step -- the product of the state and the gate(s)
    before the step, a device intermediate the upload never sees -- carries the power of every input before it, the
    small operands their own, and every tile has E <= -127: asserted below from the data (the oracle's intermediates
    of the chain's prefixes; the largest element of the whole intermediate bounds every tile's; one more for the
    rounding of each device tensor).  The scaled run must give the plain run's bits times that power, every one of
    them: every component of the expected result is a normal float or zero (asserted -- below 2^-126 x alpha x alpha2
    rounds twice, which tests/test_gpu_round4.py pins and this data stays clear of), so the power is exact."""
    tree, arrays, ref, _ = oracle_of(family, LIVE_FAMILIES)
    gates, _, form, flags = LIVE_FAMILIES[family]
    if form is not None:
        monkeypatch.setenv("CTG_STEM_FORM", form)
    n = len(arrays)
    assert n == 4
    s = -((104 + int(np.floor(np.log2(top_of(ref)))) + n - 1) // n)
    scaled = [G.scaled_in_window(a, s) for a in arrays]
    a128 = [a.astype("complex128") for a in scaled]
    if flags["one"]:
        # E = exponent of A + exponent of B1
        big = np.asarray(orc.contract(network(family, upto=2, families=LIVE_FAMILIES), a128[:3]))
        e = h2_exponent(top_of(big)) + 1 + h2_exponent(top_of(scaled[3]))
    else:
        # E = e(A) + e(B1) + e(B2) + (exponent of the intermediate in units of 2^(e(A) + e(B1))) = e(A B1) + e(B2)
        mid = np.asarray(orc.contract(network(family, upto=2, families=LIVE_FAMILIES), a128[:3]))
        e = h2_exponent(top_of(mid)) + 2 + h2_exponent(top_of(scaled[3]))
    print(family, "shift per input", s, "E <=", e)
    assert e <= -127, e
    fn = contractor(tree, "fp16x2")
    try:
        plain, names = run(fn, arrays)
        got, names_s = run(fn, scaled)
    finally:
        fn.close()
    assert_family_ran(family, "fp16x2", names, LIVE_FAMILIES)
    assert names_s == names
    plain, got = np.asarray(plain), np.asarray(got)
    want = plain.astype("complex128") * 2.0 ** (n * s)

    def parts(z):
        return np.concatenate([np.asarray(z).real.ravel(), np.asarray(z).imag.ravel()]).astype(np.float64)

    w, g = parts(want), parts(got)
    normal = (np.abs(w) >= 2.0 ** -126) | (w == 0)
    print(family, "largest", float(np.abs(w).max()), "components below 2^-126:", int((~normal).sum()), "of", w.size)
    assert normal.all()
    assert np.array_equal(g, w), float(np.abs(g - w).max())


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bf16x3_powers_of_two(family, stem_env, monkeypatch):
    """bf16 x 3 takes a power of two out of a SMALL operand only where its largest element leaves [2^-64, 2^64), and
    the upload leaves no input outside [2^-32, 2^32): in these chains, whose small operands are inputs, both store
    factors are 1 (a live second factor needs small operands that are themselves products of inputs: not built here).  What is checked is that unscaled path (B1, B2 x 2^-24,
    the state and the first gate x 2^+24: the plain run's bits) and the scaling path with a first factor
    (strip_exponent: every stored intermediate renormalised, the store multiplies by 1 / the operands' factors)
    against the oracle."""
    tree, arrays, ref, np64 = oracle_of(family)
    if FAMILIES[family][2] is not None:
        monkeypatch.setenv("CTG_STEM_FORM", FAMILIES[family][2])
    shifts = [24, 24] + [-24] * (len(arrays) - 2)
    if len(arrays) == 3:
        shifts = [24, 0, -24]
    scaled = [G.scaled_in_window(a, s) for a, s in zip(arrays, shifts)]
    fn = contractor(tree, "bf16x3")
    try:
        plain, names = run(fn, arrays)
        got, _ = run(fn, scaled)
        (m, e), names_x = run(fn, arrays, strip_exponent=True)
    finally:
        fn.close()
    assert_family_ran(family, "bf16x3", names)
    assert_family_ran(family, "bf16x3", names_x)
    assert np.array_equal(np.asarray(got), np.asarray(plain))
    err, gate = G.relerr(np.asarray(m).astype("complex128") * 10.0 ** e, ref), G.single_gate(ref, np64)
    print(family, "strip_exponent relerr", err, "gate", gate)
    assert err <= gate, (err, gate)


# ---------------------------------------------------------------------- #
# (c) limb edges
# ---------------------------------------------------------------------- #


def two_fp16_limbs(x, top):
    """x -> h1 + h2, its two rounded fp16 limbs under the power of two that brings ``top`` to [2^13, 2^14) (the host
    emulation of tools/exp_product_levers.py with the kernels' scale; numpy rounds float64 -> float16 to nearest even,
    once, and the residual is exact in float64)."""
    scale = 2.0 ** h2_exponent(top)

    def limbs(v):
        v = v / scale
        h1 = v.astype(np.float16).astype(np.float64)
        h2 = (v - h1).astype(np.float16).astype(np.float64)
        return (h1 + h2) * scale

    return limbs(x.real) + 1j * limbs(x.imag)


def unit_permutation(rng, shape):
    """A gate tensor that is a permutation matrix of its (contracted, new) halves with entries 1, -1, i, -i -- one
    limb each, one term per output element: the kernel's fp32 sums are exact in any order -- and whose zeros are
    negative zeros in half of the places."""
    k = 1 << (len(shape) // 2)
    assert k * k == int(np.prod(shape))
    m = np.zeros((k, k), dtype="complex64")
    m[np.arange(k), rng.permutation(k)] = rng.choice(np.array([1, -1, 1j, -1j], dtype="complex64"), size=k)
    neg = rng.random((k, k)) < 0.5
    re = np.where((m.real == 0) & neg, np.float32(-0.0), m.real).astype("float32")
    im = np.where((m.imag == 0) & ~neg, np.float32(-0.0), m.imag).astype("float32")
    out = np.empty((k, k), dtype="complex64")
    out.real, out.imag = re, im
    return out.reshape(shape)


def edge_state(rng, shape, generic):
    """The running tensor: a quarter zeros, ties of fp16 rounding -- (2 k + 1) 2^-11 2^j, twelve significant bits,
    j = -10 ... -7, k of both parities (the first limb rounds down and up: residuals of both signs), both signs, real and
    imaginary parts drawn apart -- and, with ``generic``, values of 24 random bits, which two limbs truncate; the largest
    element is 1 - 2^-24, one ulp below a power of two: its first limb rounds UP to the power, the second is -1 ulp."""
    n = int(np.prod(shape))

    def part():
        k = rng.integers(0, 1024, size=n)
        tie = (2048 + 2 * k + 1).astype(np.float64) * 2.0 ** -11 * 2.0 ** rng.integers(-10, -6, size=n)
        v = tie * rng.choice([-1.0, 1.0], size=n)
        if generic:
            g = rng.integers(1 << 23, 1 << 24, size=n).astype(np.float64) * 2.0 ** -24 * 2.0 ** rng.integers(-10, -1, size=n)
            v = np.where(rng.random(n) < 0.5, v, g * rng.choice([-1.0, 1.0], size=n))
        return np.where(rng.random(n) < 0.25, 0.0, v)

    x = (part() + 1j * part()).astype("complex64")
    x[int(rng.integers(n))] = np.complex64(complex(1.0 - 2.0 ** -24, 0.0))
    assert top_of(x) == float(np.float32(1.0 - 2.0 ** -24))
    return x.reshape(shape)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("family,generic", [("single", True), ("ws_cs1", False), ("pack2", False)])
def test_limb_edges_give_the_emulations_bits(family, generic, arith, stem_env):
    """The first gate is the identity, so the stem step's big operand IS the state's values (x 1 + 0 is exact in the
    pair kernel's fp32), and every later gate is a unit permutation: each output element is one element of the state
    times 1, -1, i or -i, whatever the layout, and every sum the kernel forms is exact.  What comes out is therefore
    the state as its limbs carry it: two fp16 limbs under the scale of its largest element (the emulation below; a
    24-bit value loses its last bits there, ties and the largest element do not), three bf16 limbs exactly.  A pair
    splits its intermediate once more, per tile and under the TILE's scale: the pairs take only values that two limbs
    hold under any of these scales (``generic`` off).  Zeros: the state's and the permutations'.  NEGATIVE zeros are in
    the permutations only, small operands staged by store_limbs: the split itself never sees one -- its operand is a
    kernel's result, accumulators start from +0 and (-0) x 1 + 0 is +0 -- so the sign of a zero residual is not covered
    here (mixlo with the addend 0 gives +0 for -0, as the compiler's own form of the product did).  Equality is numeric."""
    tree = network(family)
    rng = np.random.default_rng(11)
    shapes = [tuple(tree.size_dict[ix] for ix in t) for t in tree.inputs]
    state = edge_state(rng, shapes[0], generic)
    eye = np.eye(8, dtype="complex64").reshape(shapes[1])
    arrays = [state, eye] + [unit_permutation(rng, s) for s in shapes[2:]]
    a128 = [a.astype("complex128") for a in arrays]
    exact = np.asarray(orc.contract(tree, a128))
    # the two-limb product: limbs of A times limbs of B, without (second limb) x (second limb); the permutations'
    # second limbs are zero, so it is (h1 + h2)(A) x B, and linear in A
    emulated = np.asarray(orc.contract(tree, [two_fp16_limbs(a128[0], top_of(state))] + a128[1:]))
    if not generic:
        assert np.array_equal(emulated, exact)   # (the pairs' values: two limbs hold them)
    else:
        assert not np.array_equal(emulated, exact)   # (the single step's: they do not)
    want = emulated if arith == "fp16x2" else exact
    assert np.array_equal(want.astype("complex64").astype("complex128"), want)   # (a float result, no rounding in the way)
    fn = contractor(tree, arith)
    try:
        got, names = run(fn, arrays)
    finally:
        fn.close()
    assert_family_ran(family, arith, names)
    got = np.asarray(got)
    bad = int(np.count_nonzero(got != want.astype("complex64")))
    print(family, arith, names, "elements that differ", bad, "of", got.size)
    assert bad == 0
    gate = G.single_gate(exact, np.asarray(orc.contract(tree, arrays)))
    assert G.relerr(got, exact) <= gate
