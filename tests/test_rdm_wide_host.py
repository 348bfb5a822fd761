"""CPU suite: the host side of reduced density matrices above 64 rows (csrc/ctg_rdm_wide.hip) --
the header, ``ctg_rdm_wide_plan`` against its Python mirror ``runtime.rdm_wide_plan`` word for word, the invariants of
a plan (blocks x splits = grid, every pair a >= b in exactly one block, the splits partition r, the scratch within the
header's bound), the refusals, the kernel names, the validation of ``circuits.entanglement_*`` and a numpy
interpretation of the plan on small-integer data.  No device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime

import rdm_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["float32", "float64", "complex64", "complex128"]
TAG = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}


def bits_request(L, bits):
    """``(shape, keep flags)`` for kept ``bits`` of the flat index of 2^L elements (bit b is axis L - 1 - b)."""
    axes = {L - 1 - b for b in bits}
    return (2,) * L, [1 if a in axes else 0 for a in range(L)]


def table():
    """(shape, keep flags, D, t, route)"""
    rows = []
    for L, bits in [(12, range(5, 12)), (12, range(0, 7)), (14, range(0, 14, 2)),            # D = 128: high, low, interleaved
                    (14, range(1, 14, 2)), (20, range(13, 20)), (20, range(0, 7)),
                    (14, range(6, 14)), (16, range(0, 16, 2)),                                # 256
                    (18, range(9, 18)), (18, range(0, 9)), (18, range(0, 18, 2)),             # 512
                    (20, range(10, 20)), (20, range(0, 20, 2)), (11, range(0, 10)),           # 1024 (the last: n < 4096)
                    (12, range(0, 12)), (13, range(0, 12)), (13, range(1, 13)),               # 4096: t = 1, 2, 2
                    (16, range(4, 16)), (16, range(0, 12)), (25, range(13, 25)),              #       t = 16, 16, 2^13
                    (20, [0, 1, 2, 3, 4, 5, 19]), (17, range(4, 11))]:
        shape, flags = bits_request(L, list(bits))
        d = 2 ** len(list(bits))
        rows.append((shape, flags, d, 2 ** L // d, 0 if L >= 12 else 1))
    for shape, keep in [((4, 8, 1, 2, 16, 8), (0, 1, 3, 5)), ((4, 8, 1, 2, 16, 8), (1, 4)), ((4, 8, 1, 2, 16, 8), (0, 2, 3, 4)),
                        ((2, 64, 4, 128, 2, 4, 2, 2), (1, 5, 6)), ((2, 64, 4, 128, 2, 4, 2, 2), (3,)),
                        ((2, 64, 4, 128, 2, 4, 2, 2), (0, 3, 7))]:
        d = int(np.prod([shape[a] for a in keep]))
        rows.append((shape, [1 if a in keep else 0 for a in range(len(shape))], d, int(np.prod(shape)) // d, 0))
    for shape, keep in [((3,) * 8, range(5)), ((3,) * 8, range(1, 8)), ((3,) * 8, (0, 2, 4, 6, 7)), ((5, 7, 11, 13), (1, 3)),
                        ((5, 7, 11, 13), (2, 3)), ((3, 4096), (1,)), ((2, 3) * 6, (0, 2, 4, 6, 8, 10, 1))]:
        keep = list(keep)
        d = int(np.prod([shape[a] for a in keep]))
        rows.append((shape, [1 if a in keep else 0 for a in range(len(shape))], d, int(np.prod(shape)) // d, 1))
    return rows


def c_plan(dtype, shape, flags):
    ext, kp = np.array(shape, np.int64), np.array(flags, np.int32)
    words = np.full(runtime.RdmWidePlan._fields.__len__(), -7, np.int64)
    rc = runtime.load().ctg_rdm_wide_plan(runtime._DTYPE_CODE[dtype], ext.size, ext.ctypes.data_as(C.POINTER(C.c_int64)),
                                          kp.ctypes.data_as(C.POINTER(C.c_int32)), words.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, words


def test_header_and_public_names():
    text = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+ctg_exec_result_rdm_wide\s*\(\s*ctg_exec\s*\*\s*exec,\s*int64_t rank,\s*const int64_t\s*\*\s*extents,"
                     r"\s*const int32_t\s*\*\s*keep,\s*void\s*\*\s*out,\s*double\s*\*\s*purity\)", code)
    assert re.search(r"int\s+ctg_rdm_wide_plan\s*\(\s*int32_t dtype,\s*int64_t rank,\s*const int64_t\s*\*\s*extents,"
                     r"\s*const int32_t\s*\*\s*keep,\s*int64_t\s*\*\s*words\)", code)
    assert re.search(r"#define\s+CTG_RDM_WIDE_MAX_DIM\s+4096\b", code)
    assert re.search(r"#define\s+CTG_RDM_MAX_DIM\s+64\b", code) and re.search(r"#define\s+CTG_OP_MAX_DIM\s+64\b", code)
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", code) and runtime.ABI_VERSION == 10
    m = re.search(r"#define\s+CTG_RDM_WIDE_PLAN_WORDS\s+(\d+)", code)
    assert m and int(m.group(1)) == len(runtime.RdmWidePlan._fields)
    assert runtime.Executor.RDM_WIDE_MAX_DIM == 4096 and runtime.Executor.RDM_MAX_DIM == 64
    for name in ("rdm_wide_dim", "rdm_wide_plan", "rdm_wide_variant", "rdm_wide_scratch_bound"):
        assert callable(getattr(runtime, name))
    for name in ("rdm_wide_result", "rdm_wide_variant"):
        assert callable(getattr(runtime.Executor, name))
    assert ca.RdmWideResult._fields == ("rho", "dims", "purity", "norm", "exponent")
    assert callable(ca.HipContractor.rdm_wide) and callable(ca.ContractionTree.contract_rdm_wide)
    from cotengra_amd.interface import ContractExpression

    assert callable(ContractExpression.rdm_wide)
    for name in ("entanglement_spectrum", "entanglement_entropy", "entanglement_cut"):
        assert callable(getattr(circuits, name))
    # the header's scratch bound is the binding's
    m = re.search(r"#define\s+CTG_RDM_WIDE_SCRATCH_BYTES\(D\)(.*?)\n[^\\\n]*\n", text, flags=re.S)
    expr = m.group(0).split("(D)", 1)[1].replace("\\\n", " ").replace("ll", "")
    expr = re.sub(r"(.*)\?(.*):(.*)", r"\1 and \2 or \3", expr)
    for d in (65, 128, 2187, 2897, 4096):
        assert eval(expr, {"D": d}) == runtime.rdm_wide_scratch_bound(d)


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_plan_equals_the_library_word_for_word(dtype):
    for shape, flags, d, t, route in table():
        rc, words = c_plan(dtype, shape, flags)
        assert rc == 0, (shape, flags, runtime.load().ctg_last_error())
        plan = runtime.rdm_wide_plan(dtype, shape, flags)
        assert tuple(int(w) for w in words) == tuple(plan), (shape, flags)
        assert (plan.route, plan.dim) == (route, d)
        assert plan.name_code == 4 * route + runtime._DTYPE_CODE[dtype]
        name = f"rdm_wide_kernel<{TAG[dtype]},64>" if route == 0 else f"rdm_wide_general_kernel<{TAG[dtype]}>"
        assert runtime.rdm_wide_variant(dtype, shape, flags) == name


def blocks_of(plan):
    """(bi, bj) of every block, in the plan's numbering"""
    return [(bi, bj) for bi in range(plan.panels) for bj in range(bi + 1)]


@pytest.mark.parametrize("dtype", ["float32", "complex128"])
def test_plan_invariants(dtype):
    for shape, flags, d, t, route in table():
        plan = runtime.rdm_wide_plan(dtype, shape, flags)
        assert plan.blocks * plan.splits == plan.grid
        assert plan.panels * plan.edge == d and plan.blocks == plan.panels * (plan.panels + 1) // 2
        assert plan.edge >= 64 if route == 0 else plan.edge == 1
        # every pair (a >= b) lies in exactly one block
        bl = np.array(blocks_of(plan))
        assert len(bl) == plan.blocks
        number = bl[:, 0] * (bl[:, 0] + 1) // 2 + bl[:, 1]
        assert np.array_equal(number, np.arange(plan.blocks))
        count = np.zeros((plan.panels, plan.panels), np.int64)
        np.add.at(count, (bl[:, 0], bl[:, 1]), 1)
        assert np.array_equal(count, np.tril(np.ones_like(count)))   # (panel pairs: pairs of rows follow, edge by edge)
        a = np.arange(d)
        assert np.array_equal(a // plan.edge * plan.edge + a % plan.edge, a) and a.max() // plan.edge == plan.panels - 1
        # the splits partition r: whole chunks, consecutive, all of them
        assert plan.chunks == -(-t // plan.cols) and plan.chunks % plan.splits == 0
        cps = plan.chunks // plan.splits
        cover = np.zeros(t, np.int64)
        for s in range(plan.splits):
            cover[s * cps * plan.cols:min((s + 1) * cps * plan.cols, t)] += 1
        assert np.all(cover == 1)
        if route == 0:
            assert plan.cols == min(32, t) and (plan.splits == 1 or cps >= 32)
            assert plan.splits == 1 or plan.blocks * plan.splits < 1024
        assert 0 < plan.scratch_bytes <= runtime.rdm_wide_scratch_bound(d), (shape, flags)
        assert plan.scratch_bytes >= d * d * (16 if dtype == "complex128" else 8)
    # the bound holds at the widest matrix of either route
    for shape, flags in [bits_request(24, range(12, 24)), ((4096, 3), [1, 0]), ((4096, 10 ** 6), [1, 0])]:
        plan = runtime.rdm_wide_plan("complex128", shape, flags)
        assert plan.scratch_bytes <= runtime.rdm_wide_scratch_bound(4096) < 400 << 20
    assert runtime.rdm_wide_plan("complex64", *bits_request(20, range(13, 20))).splits > 1
    assert runtime.rdm_wide_plan("complex64", *bits_request(20, range(10, 20))).splits == 1


def test_refusals():
    lib = runtime.load()
    cases = [((64, 128), [1, 0], b"ctg_exec_result_rdm"), ((2,) * 13, [1] * 6 + [0] * 7, b"CTG_RDM_MAX_DIM"),
             ((8192, 2), [1, 0], b"CTG_RDM_WIDE_MAX_DIM"), ((3,) * 9, [1] * 9, b"CTG_RDM_WIDE_MAX_DIM"),
             ((2,) * 12, [0] * 12, b"ctg_exec_result_rdm"),
             ((128, 0), [1, 1], b"extent"), ((128, 64), [2, 0], b"keep"), ((128, 64), [-1, 0], b"keep"),
             ((2 ** 21, 2 ** 21, 128), [0, 0, 1], b"product")]
    for shape, flags, word in cases:
        rc, words = c_plan("complex64", shape, flags)
        assert rc == -1 and word in lib.ctg_last_error(), (shape, flags, lib.ctg_last_error())
        assert np.all(words == -7)
        with pytest.raises(ValueError):
            runtime.rdm_wide_plan("complex64", shape, flags)
        with pytest.raises(ValueError):
            runtime.rdm_wide_variant("complex64", shape, flags)
    for shape, flags, _ in cases[:5]:
        with pytest.raises(ValueError):
            runtime.rdm_wide_dim(shape, flags)
    with pytest.raises(ValueError):
        runtime.rdm_wide_plan("complex64", (128, 64), [1])
    ext, kp = np.array([128, 64], np.int64), np.array([1, 0], np.int32)
    args = (2, ext.ctypes.data_as(C.POINTER(C.c_int64)), kp.ctypes.data_as(C.POINTER(C.c_int32)))
    words = np.zeros(16, np.int64)
    assert lib.ctg_rdm_wide_plan(4, *args, words.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    assert lib.ctg_rdm_wide_plan(-1, *args, words.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    assert lib.ctg_rdm_wide_plan(2, *args, None) == -1
    assert lib.ctg_rdm_wide_plan(2, 2, None, None, words.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    # a null executor is refused before anything else
    assert lib.ctg_exec_result_rdm_wide(None, *args, None, None) == -1
    # the narrow entry points keep their limit
    with pytest.raises(ValueError):
        runtime.rdm_variant("complex64", (128, 64), [1, 0])
    # one request per call
    tree = ca.ContractionTree(["ab"], "ab", {"a": 128, "b": 64})
    from cotengra_amd.contractor import _tree_contractor

    with pytest.raises(ValueError, match="one request"):
        _tree_contractor(tree).rdm_wide(keep=[["a"], ["b"]])
    with pytest.raises(ValueError, match="CTG_RDM_MAX_DIM"):
        _tree_contractor(tree).rdm_wide(keep=["b"])
    with pytest.raises(ValueError):
        _tree_contractor(tree).rdm_wide(keep=["z"])


def test_entanglement_validation():
    side, open_qubits, fixed = circuits.entanglement_cut(14, range(7))
    assert side == list(range(7)) and open_qubits == list(range(14)) and fixed == {}
    side, _, _ = circuits.entanglement_cut(14, range(3, 14))                 # 11 | 3: the complement, ascending
    assert side == [0, 1, 2]
    side, _, _ = circuits.entanglement_cut(14, [13, 2, 5, 7, 9, 11, 0, 1], fixed={3: 1})   # 8 | 5 of 13 open
    assert side == [4, 6, 8, 10, 12]
    side, _, _ = circuits.entanglement_cut(10, [9, 4, 0])                   # the caller's order is kept
    assert side == [9, 4, 0]
    assert circuits.entanglement_cut(24, range(12))[0] == list(range(12))
    assert circuits.entanglement_cut(30, range(20))[0] == list(range(20, 30))
    gates = [("H", 0)]
    with pytest.raises(ValueError, match="13 qubits"):
        circuits.entanglement_cut(26, range(13))
    with pytest.raises(ValueError, match="13 qubits"):
        circuits.entanglement_spectrum(26, gates, range(13))
    with pytest.raises(ValueError, match="13 qubits"):
        circuits.entanglement_entropy(27, gates, range(14), alpha=2)
    for fn in (circuits.entanglement_spectrum, circuits.entanglement_entropy):
        with pytest.raises(ValueError, match="both fixed and kept"):
            fn(8, gates, [0, 1], fixed={1: 0})
        with pytest.raises(ValueError):
            fn(8, gates, [0, 0])
        with pytest.raises(ValueError):
            fn(8, gates, [])
        with pytest.raises(ValueError):
            fn(8, gates, [8])
        with pytest.raises(ValueError):
            fn(8, gates, [0], fixed={3: 2})
    with pytest.raises(ValueError, match="alpha"):
        circuits.entanglement_entropy(8, gates, [0], alpha=0)
    with pytest.raises(ValueError, match="base"):
        circuits.entanglement_entropy(8, gates, [0], base=1)
    # the eigenvalue gate: a clearly negative one is refused, rounding noise is clipped
    with pytest.raises(ValueError, match="positive semidefinite"):
        circuits._cut_spectrum(np.diag([1.0, -1e-9]), 2)
    w = circuits._cut_spectrum(np.diag([0.75, 0.25, -1e-17, 0.0]), 4)
    assert np.array_equal(w, [0.75, 0.25, 0.0, 0.0])
    # reduced_density_matrix itself stays at 6 qubits
    with pytest.raises(ValueError):
        circuits.reduced_density_matrix(8, gates, list(range(7)))


def interpret(plan, X):
    """rho = X X^H as the plan lists the work: block by block, split by split (ascending), the lower blocks only, the
    other half mirrored -- in exact arithmetic on the integers of X."""
    d, t = X.shape
    e, cps = plan.edge, plan.chunks // plan.splits
    rho = np.zeros((d, d), X.dtype)
    for bi, bj in blocks_of(plan):
        A, B = X[bi * e:(bi + 1) * e], X[bj * e:(bj + 1) * e]
        acc = np.zeros((e, e), X.dtype)
        for s in range(plan.splits):
            c0, c1 = s * cps * plan.cols, min((s + 1) * cps * plan.cols, t)
            acc = acc + A[:, c0:c1] @ B[:, c0:c1].conj().T
        rho[bi * e:(bi + 1) * e, bj * e:(bj + 1) * e] = acc
    low = np.tril(rho)
    out = low + np.tril(rho, -1).conj().T
    if out.dtype.kind == "c":
        out[np.diag_indices(d)] = np.diag(low).real
    return out


def test_numpy_interpretation_of_the_plan_is_exact_on_small_integers():
    rng = np.random.default_rng(20)
    cases = [bits_request(15, [0, 2, 3, 5, 8, 13, 14]) + ("complex64",),            # D = 128, t = 256: 3 blocks, 1 split
             bits_request(19, [18, 17, 9, 8, 3, 1, 0]) + ("float32",),              # D = 128, t = 4096: splits > 1
             ((4, 8, 1, 2, 16, 8), [1, 1, 0, 1, 0, 1], "complex128"),               # D = 512, t = 16: less than a chunk
             ((3,) * 8, [1, 1, 1, 1, 1, 0, 0, 0], "complex64"),                     # general, D = 243
             ((5, 3000, 13), [1, 0, 1], "float64")]                                 # general, several chunks of r
    for shape, flags, dtype in cases:
        n = int(np.prod(shape))
        x = rng.integers(-4, 5, n).astype(dtype)
        if np.dtype(dtype).kind == "c":
            x = x + 1j * rng.integers(-4, 5, n).astype(dtype)
        keep = [a for a, f in enumerate(flags) if f]
        X = du.rdm_matrix(x, shape, keep)
        plan = runtime.rdm_wide_plan(dtype, shape, flags)
        assert (plan.splits > 1) == (shape in ((2,) * 19, (5, 3000, 13)))
        got = interpret(plan, X)
        assert np.array_equal(got, du.rdm_reference(x, shape, keep)) and np.array_equal(got, got.conj().T)
