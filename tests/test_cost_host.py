"""Host suite of the cost statistics (csrc/ctg_cost.hip; no device): the numpy models of
tests/cost_util.py against direct evaluation and against an independent select in exact rationals, the input condition of
every fixture of the GPU suite, the plan function pinned, the refusals of the plan function and of the Python layers, the
symbols and the source lists."""
import ctypes as C
import fractions
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import cost_requests

import cost_util as cu
import spectrum_util as spu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gaussian(n, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "c":
        return rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return rng.standard_normal(n)


def term_sets(L):
    """Ring, complete-graph and 3-body terms over ``L`` qubits, with the identity in front."""
    ring = [(q, (q + 1) % L) for q in range(L)]
    complete = [(a, b) for a in range(L) for b in range(a + 1, L)]
    three = [(q, (q + 2) % L, (q + 5) % L) for q in range(L)]
    return {"ring": [()] + ring, "complete": [()] + complete, "three": [()] + three}


@pytest.mark.parametrize("L", [6, 10])
@pytest.mark.parametrize("kind", ["ring", "complete", "three"])
def test_the_cost_model_is_direct_evaluation_for_integer_coefficients(L, kind):
    terms = term_sets(L)[kind]
    rng = np.random.default_rng(L)
    coeffs = rng.integers(-7, 8, size=len(terms)).astype(np.float64)
    masks = cu.term_masks(L, terms)
    got = cu.cost_model(masks, coeffs, L)
    ref = cu.cost_direct(masks, coeffs, L)
    assert np.array_equal(got, ref) and not np.signbit(got[got == 0.0]).any()
    assert masks == runtime.cost_masks((2,) * L, cu.term_ops(L, terms)).tolist()


@pytest.mark.parametrize("L", [6, 10])
def test_the_cost_model_meets_its_bound_for_gaussian_coefficients(L):
    n = 2 ** L
    terms = term_sets(L)["complete"] + term_sets(L)["three"][1:] + [(0, 1)]          # (one mask twice)
    coeffs = np.random.default_rng(7 + L).standard_normal(len(terms))
    masks = cu.term_masks(L, terms)
    got = cu.cost_model(masks, coeffs, L)
    ref = cu.cost_direct(masks, coeffs, L)
    tol = n * 2.0 ** -53 * float(np.sum(np.abs(coeffs)))
    err = np.abs(got - ref)
    print(f"cost model L={L}: max err {err.max():.2e}, bound {tol:.2e}")
    assert np.all(err <= tol)
    # one wrong sign of a median coefficient is far outside the bound
    j = int(np.argsort(np.abs(coeffs))[len(coeffs) // 2])
    wrong = coeffs.copy()
    wrong[j] = -wrong[j]
    assert np.all(np.abs(cu.cost_direct(masks, wrong, L) - got) > 100 * tol)


def rational_select(C, w, alpha, tail):
    """An independent select: the distinct costs in order, their masses as rationals of W."""
    C = np.asarray(C, dtype=np.float64)
    W = sum(int(v) for v in w)
    classes = {}
    for c, v in zip(C.tolist(), w.tolist()):
        classes[c + 0.0] = classes.get(c + 0.0, 0) + int(v)
    run = fractions.Fraction(0)
    for c in sorted(classes, reverse=tail > 0):
        if run + fractions.Fraction(classes[c], W) >= fractions.Fraction(alpha):
            return dict(t=c, below=int(run * W), at=classes[c])
        run += fractions.Fraction(classes[c], W)
    raise AssertionError("alpha above 1")


def test_the_select_model_is_a_sort_and_cumsum_in_exact_rationals():
    L = 14
    terms, coeffs = cu.ring_terms(L)
    Cv = cu.cost_model(cu.term_masks(L, terms), coeffs, L)
    assert sorted(set(Cv.tolist())) == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0]     # 8 distinct values: heavy ties
    x = cu.scaled(gaussian(2 ** L, "complex64", 5), "complex64")
    S, s, w = cu.weights(x)
    assert 0.7 <= S <= 0.8 and s == 62
    W = int(w.sum(dtype=np.uint64))
    for tail in (-1, 1):
        for alpha in (2.0 ** -10, 0.1, 0.5, 1.0):
            got = cu.select_model(Cv, w, alpha, tail)
            ref = rational_select(Cv, w, alpha, tail)
            assert (got["t"], got["below"], got["at"]) == (ref["t"], ref["below"], ref["at"]), (tail, alpha, got, ref)
            assert got["A"] == -((-fractions.Fraction(alpha) * W) // 1) and 1 <= got["A"] <= W
            assert got["below"] < got["A"] <= got["below"] + got["at"]
    # alpha = 1 reaches the far end of the support, whatever the tail
    assert cu.select_model(Cv, w, 1.0, -1)["t"] == 14.0 and cu.select_model(Cv, w, 1.0, 1)["t"] == 0.0


def test_the_select_model_at_a_level_exactly_on_a_class_boundary():
    # weights 2^60 each on four costs: alpha = 1/2 ends exactly with the second class; one unit more starts the third
    Cv = np.array([3.0, -1.0, 2.0, -1.0, 7.0, 2.0, 3.0, 7.0])
    w = np.full(8, 2 ** 59, dtype=np.uint64)
    got = cu.select_model(Cv, w, 0.5, -1)
    assert got == dict(A=2 ** 61, t=2.0, below=2 ** 60, at=2 ** 60)
    assert cu.select_model(Cv, w, 0.5, 1) == dict(A=2 ** 61, t=3.0, below=2 ** 60, at=2 ** 60)
    assert cu.select_model(Cv, w, 0.5 + 2.0 ** -52, -1)["t"] == 3.0
    assert cu.select_model(Cv, w, 0.25, -1) == dict(A=2 ** 60, t=-1.0, below=0, at=2 ** 60)
    assert rational_select(Cv, w, 0.5, -1) == dict(t=2.0, below=2 ** 60, at=2 ** 60)
    # -0.0 and +0.0 are one class
    z = cu.select_model(np.array([-0.0, 0.0, 1.0]), np.array([1, 1, 2], dtype=np.uint64), 0.5, -1)
    assert z == dict(A=2, t=0.0, below=0, at=2) and not np.signbit(z["t"])
    assert cu.select_model(Cv, np.zeros(8, dtype=np.uint64), 0.5, -1) == dict(A=0, t=0.0, below=0, at=0)


def test_the_histogram_model():
    Cv = np.array([-1.0, 0.0, 0.5, 1.0, 1.0, 2.0, 5.0])
    w = np.arange(1, 8, dtype=np.uint64)
    h = cu.hist_model(Cv, w, [0.0, 1.0, 2.0])
    assert h.tolist() == [1, 2 + 3, 4 + 5, 6 + 7]          # (an edge equal to a cost opens the bin; the last edge too)
    assert int(h.sum()) == int(w.sum())


def gpu_fixtures():
    """Every tensor of tests/test_gpu_cost.py, by the same constructors."""
    import test_gpu_cost as tg

    out = [tg.tensor(L, dt) for L, dt in tg.TENSORS]
    out.append(tg.values_tensor())
    out.append(tg.zero_optimum_tensor())
    return out


def test_the_input_condition_holds_for_every_fixture():
    for x in gpu_fixtures():
        S, s, w = cu.weights(x)
        W = int(w.sum(dtype=np.uint64))
        assert 0.7 <= S <= 0.8 and s == 62, (x.size, x.dtype, S)
        assert W < 2 ** 63 and abs(W * 2.0 ** -s - S) <= x.size * 2.0 ** -54 + x.size * 2.0 ** -(s + 1)


# ---- the plan ------------------------------------------------------------------------------------------------- #


def up256(b):
    return (b + 255) & ~255


def scratch(n, grid, ne):
    """The layout of csrc/ctg_cost.hip by the header's words: the vector, 8 states of 32 bytes, the digit rows and their
    sum, a record of 176 bytes per workgroup, the histogram rows and their sum, the edges, 64 words, a flag."""
    h = [grid * (ne + 1) * 8, (ne + 1) * 8, ne * 8] if ne else []
    return sum(up256(b) for b in [n * 8, 8 * 32, grid * 4096 * 8, 4096 * 8, grid * 176] + h + [64 * 8, 8])


def test_the_plan_is_pinned():
    P = runtime.CostPlan
    d, r, s_, f = "cost_digit_kernel<c64>", "cost_rowsum_kernel", "cost_select_kernel", "cost_finish_kernel"

    def kernels(passes, nl, ne, tag="c64"):
        dg = (f"cost_digit_kernel<{tag}>", r, s_)
        return (("cost_scatter_kernel", "cost_tile_kernel") + ("cost_pass_kernel",) * passes + dg[:2] + (dg[2:] if nl else ())
                + dg * (5 * nl) + (f"cost_final_kernel<{tag},{1 if ne else 0}>",) + ((r,) if ne else ()) + (f,))

    def plan(L, nl=0, ne=0, dtype="complex64"):
        return runtime.cost_plan(dtype, (2,) * L, "terms", nl, ne)

    assert plan(0) == P(0, 1, 0, 0, (), 1, 1, 1, 1, scratch(1, 1, 0), 1, 0, kernels(0, 0, 0))
    assert plan(12, 4) == P(12, 4096, 12, 0, (), 1, 6, 21, 1, scratch(4096, 1, 0), 1, 0, kernels(0, 4, 0))
    assert plan(13, 1, 2) == P(13, 8192, 12, 1, (1,), 2, 6, 6, 2, scratch(8192, 2, 2), 2, 3, kernels(1, 1, 2))
    assert plan(20, 8, 4097) == P(20, 1 << 20, 12, 1, (8,), 256, 6, 41, 256, scratch(1 << 20, 256, 4097), 256, 4098, kernels(1, 8, 4097))
    assert plan(21) == P(21, 1 << 21, 12, 2, (8, 1), 512, 1, 1, 512, scratch(1 << 21, 512, 0), 512, 0, kernels(2, 0, 0))
    assert plan(28, 1) == P(28, 1 << 28, 12, 2, (8, 8), 1 << 16, 6, 6, 512, scratch(1 << 28, 512, 0), 1 << 16, 0, kernels(2, 1, 0))
    assert plan(13, dtype="float64").kernels[3] == "cost_digit_kernel<double>"
    assert plan(13, dtype="float32").kernels[-2] == "cost_final_kernel<float,0>"
    # values: any extents, no transform; 3 * 5 * 7 * 11 elements are one chunk, 3 * 4099 are four
    v = runtime.cost_plan("complex128", (3, 5, 7, 11), "values", 2, 0)
    assert (v.bits, v.n, v.tile_bits, v.passes, v.tiles, v.grid, v.chunks) == (-1, 1155, 0, 0, 0, 1, 1)
    assert v.kernels[0] == "cost_check_kernel" and v.kernels[1] == "cost_digit_kernel<c128>" and v.digit_launches == 11
    assert v.scratch_bytes == scratch(1155, 1, 0)
    assert runtime.cost_plan("float32", (3, 4099), "values").chunks == 4
    # above 512 chunks the workgroups take spans, none of them empty: 513 chunks are 257 spans of 2
    w = runtime.cost_plan("float32", (513, 4096), "values")
    assert (w.chunks, w.grid) == (513, 257)
    # axes of extent 1 carry no bit
    assert runtime.cost_plan("complex64", (2, 1, 2, 2, 1), "terms").bits == 3


def test_the_plan_function_refuses_what_the_call_refuses():
    lib = runtime.load()
    i64p = C.POINTER(C.c_int64)
    words = np.full(runtime.COST_PLAN_WORDS, 7, np.int64)
    ext = np.array([2, 2, 1], np.int64)

    def call(dtype=2, rank=3, e=ext, source=0, nl=0, ne=0, w=words):
        return lib.ctg_cost_plan(dtype, rank, None if e is None else e.ctypes.data_as(i64p), source, nl, ne,
                                 None if w is None else w.ctypes.data_as(i64p))

    bad = [dict(dtype=4), dict(dtype=-1), dict(e=None), dict(w=None), dict(rank=-1), dict(source=2), dict(source=-1),
           dict(e=np.array([2, 3, 1], np.int64)), dict(e=np.array([2, 0, 1], np.int64)), dict(e=np.array([2, 0, 1], np.int64), source=1),
           dict(nl=-1), dict(nl=9), dict(ne=1), dict(ne=-2), dict(ne=4098),
           dict(rank=41, e=np.full(41, 2, np.int64)),                                     # past 2^40 elements
           dict(rank=2, e=np.array([2 ** 40, 2 ** 40], np.int64), source=1)]
    for row in bad:
        assert call(**row) == -1, row
        assert lib.ctg_last_error() and np.all(words == 7)
    assert call() == 0 and words[0] == 2 and words[1] == 4
    assert call(e=np.array([2, 3, 1], np.int64), source=1) == 0 and words[0] == -1 and words[1] == 6
    for kw in (dict(extents=[2, 3]), dict(extents=[2, 2], source="both"), dict(extents=[2, 2], nl=9), dict(extents=[2, 2], ne=1)):
        with pytest.raises(ValueError):
            runtime.cost_plan("complex64", **kw)


# ---- the Python layers ---------------------------------------------------------------------------------------- #


def test_requests_are_refused_before_the_device():
    tree = ca.ContractionTree(["abx", "xcd"], "abcd", dict(a=2, b=2, c=1, d=2, x=3))
    ops, co = cost_requests(tree, [{}, {"a": "Z", "d": "z"}, "IZII"], [1.0, -0.5, 2])
    assert ops.tolist() == [[0, 0, 0, 0], [3, 0, 0, 3], [0, 3, 0, 0]] and co.tolist() == [1.0, -0.5, 2.0]
    assert runtime.cost_masks((2, 2, 1, 2), ops).tolist() == [0, 0b101, 0b010]              # (strides 4, 2, 1, 1)
    assert cost_requests(tree, "ZIII")[1].tolist() == [1.0]
    for terms, coeffs in (("XIII", None), ([{"a": "Y"}], None), ([{"c": "Z"}], None), ([{"e": "Z"}], None), ("ZII", None),
                          (["ZIII", "IZII"], [1.0]), (["ZIII"], [np.inf]), (["ZIII"], [1j]), (["ZIIQ"], None)):
        with pytest.raises(ValueError):
            cost_requests(tree, terms, coeffs)
    wide = ca.ContractionTree(["abx", "xcd"], "abcd", dict(a=2, b=3, c=1, d=2, x=3))
    arrays = [np.zeros((2, 3, 3)), np.zeros((3, 1, 2))]
    with pytest.raises(ValueError):
        cost_requests(wide, "ZIII")
    # every one of these is refused before setup: the arrays never reach a device
    for kw in (dict(terms="ZIII"), dict(), dict(terms="ZIII", values=np.zeros((2, 3, 1, 2))), dict(values=np.zeros((2, 3, 2))),
               dict(values=np.zeros((2, 3, 1, 2), complex)), dict(values=np.full((2, 3, 1, 2), np.nan)),
               dict(values=np.zeros((2, 3, 1, 2)), coeffs=[1.0]), dict(values=np.zeros((2, 3, 1, 2)), levels=[0.0]),
               dict(values=np.zeros((2, 3, 1, 2)), levels=[1.5]), dict(values=np.zeros((2, 3, 1, 2)), levels=[0.5] * 9),
               dict(values=np.zeros((2, 3, 1, 2)), edges=[1.0]), dict(values=np.zeros((2, 3, 1, 2)), edges=[1.0, 1.0]),
               dict(values=np.zeros((2, 3, 1, 2)), edges=[0.0, np.inf]), dict(values=np.zeros((2, 3, 1, 2)), tail="middle")):
        with pytest.raises(ValueError):
            wide.contract_cost(arrays, **kw)
    for bad in (dict(terms=["XII"]), dict(terms=[{3: "Z"}]), dict(terms=[{1: "Z"}], fixed={1: 0}), dict(terms=[{0: "Z"}], qubits=[1]),
                dict(terms=[{0: "Z"}], coeffs=[1.0, 2.0]), dict(terms=[{0: "Z"}], fixed={1: 2}), dict(terms=[{0: "Z"}], qubits=[5])):
        with pytest.raises(ValueError):
            circuits.cost_statistics(3, [], **bad)


def test_maxcut_terms_count_the_cut():
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2), (4, 1)]
    weights = [1.0, 2.0, 0.5, 1.5, 3.0, 0.25]
    L = 5
    terms, coeffs = circuits.maxcut_terms(edges, weights)
    assert terms[0] == {} and coeffs[0] == sum(weights) / 2 and len(terms) == len(edges) + 1
    Cv = cu.cost_model(cu.term_masks(L, [tuple(t) for t in terms]), coeffs, L)
    for z in range(2 ** L):
        bit = lambda q: (z >> (L - 1 - q)) & 1                                            # noqa: E731
        assert Cv[z] == sum(w for (i, j), w in zip(edges, weights) if bit(i) != bit(j)), z
    assert circuits.maxcut_terms([(0, 1)])[1].tolist() == [0.5, -0.5]
    for bad in (dict(edges=[(0, 0)]), dict(edges=[(0, 1, 2)]), dict(edges=[(0, 1)], weights=[1.0, 2.0]), dict(edges=[(-1, 0)]),
                dict(edges=[(0, 1)], weights=[np.nan])):
        with pytest.raises(ValueError):
            circuits.maxcut_terms(**bad)


def test_symbols_sources_and_header():
    import __graft_entry__ as g

    for sym in ("ctg_exec_result_cost", "ctg_cost_plan"):
        assert sym in runtime.SYMBOLS and hasattr(runtime.load(), sym)
    assert "ctg_cost.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "ctg_cost.hip"))
    assert os.path.exists(os.path.join(g.CSRC, "ctg_wht.h"))
    spectrum = open(os.path.join(g.CSRC, "ctg_pauli_spectrum.hip")).read()
    assert '#include "ctg_wht.h"' in spectrum and "void wht_local" not in spectrum
    tool = open(os.path.join(ROOT, "tools", "result_resources.py")).read()
    assert '"ctg_cost.hip"' in tool and '"ctg_pauli_spectrum.hip"' in tool
    header = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", header) and runtime.ABI_VERSION == 10
    for name, value in (("MAX_TERMS", r"\(1 << 20\)"), ("MAX_LEVELS", "8"), ("MAX_EDGES", "4097"), ("WORDS", "64"), ("LEVEL_WORD0", "24"),
                        ("LEVEL_WORDS", "5"), ("PLAN_WORDS", "16"), ("TERMS", "0"), ("VALUES", "1")):
        assert re.search(rf"#define\s+CTG_COST_{name}\s+{value}\s", header), name
    assert (runtime.COST_MAX_TERMS, runtime.COST_MAX_LEVELS, runtime.COST_MAX_EDGES) == (1 << 20, 8, 4097)
    assert (runtime.COST_WORDS, runtime.COST_LEVEL_WORD0, runtime.COST_LEVEL_WORDS, runtime.COST_PLAN_WORDS) == (64, 24, 5, 16)
    assert runtime.Executor.COST_MAX_TERMS == 1 << 20 and runtime.Executor.COST_MAX_LEVELS == 8 and runtime.Executor.COST_MAX_EDGES == 4097
    assert re.search(r"int\s+ctg_exec_result_cost\s*\(\s*ctg_exec\*\s*exec,\s*int64_t rank,\s*const int64_t\*\s*extents,\s*int64_t m,"
                     r"\s*const uint8_t\*\s*ops,\s*const double\*\s*coeffs,\s*const void\*\s*dev_cost,\s*int32_t tail,\s*int64_t nl,"
                     r"\s*const double\*\s*levels,\s*int64_t ne,\s*const double\*\s*edges,\s*int64_t\*\s*out_words,\s*int64_t\*\s*out_hist,"
                     r"\s*void\*\s*dev_cost_out\)", header)
    assert re.search(r"int\s+ctg_cost_plan\s*\(\s*int32_t dtype,\s*int64_t rank,\s*const int64_t\*\s*extents,\s*int32_t source,"
                     r"\s*int64_t nl,\s*int64_t ne,\s*int64_t\*\s*words\)", header)
    assert hasattr(ca, "CostResult") and hasattr(ca.ContractionTree, "contract_cost") and hasattr(circuits, "cost_statistics")


def test_the_spectrum_kernels_keep_their_names():
    p = runtime.pauli_spectrum_plan("complex64", (2,) * 21, spu.flips_of(21, 5))
    assert p.kernels == ("spectrum_tile_kernel<c64>", "spectrum_pass_kernel", "spectrum_pass_kernel")
    src = open(os.path.join(ROOT, "cotengra_amd", "csrc", "ctg_pauli_spectrum.hip")).read()
    assert re.search(r"void spectrum_tile_kernel\(", src) and re.search(r"void spectrum_pass_kernel\(", src)
