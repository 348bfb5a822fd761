"""Host suite of the Pauli spectrum (csrc/ctg_pauli_spectrum.hip; no device): the numpy model of
tests/spectrum_util.py against ``pauli_util.pauli_reference`` for EVERY ``z``, that the derived bound is met and is sharp
enough to see one wrong sign, the plan function pinned, the refusals of the Python layers, the symbols and the source
lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import spectrum_requests

import pauli_util as pu
import spectrum_util as spu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L6_MASKS = [0, 1, 0b100101, 63]


def gaussian(n, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "c":
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype)
    return rng.standard_normal(n).astype(dtype)


def all_strings(shape, flips):
    n = int(np.prod(shape, dtype=np.int64))
    return np.array([spu.string_of(shape, flips, z) for z in range(n)], dtype=np.uint8)


@pytest.mark.parametrize("dtype", ["complex64", "float32", "complex128", "float64"])
@pytest.mark.parametrize("xm", L6_MASKS)
def test_the_model_is_the_reference_for_every_z(xm, dtype):
    L = 6
    shape = (2,) * L
    flips = spu.flips_of(L, xm)
    assert spu.flip_mask(shape, flips) == xm
    x = gaussian(2 ** L, dtype, seed=60 + xm)
    got = spu.spectrum_model(x, shape, flips).reshape(-1)
    ops = all_strings(shape, flips)
    assert len({tuple(r) for r in ops.tolist()}) == 2 ** L         # (2^L different strings, all with X / Y on flips)
    assert all(m[0] == xm and m[1] == z for z, m in enumerate(runtime.pauli_masks(shape, ops)))
    ref = pu.pauli_reference(x, shape, ops)
    tol = spu.spectrum_tol(x, 2 ** L)
    err = np.abs(got - ref)
    print(f"model xm={xm:#x} {dtype}: max err {err.max():.2e}, bound {tol:.2e}")
    assert np.all(err <= tol)
    if np.dtype(dtype).kind != "c":
        odd = spu.popcount(np.arange(2 ** L) & xm) % 2 == 1
        assert np.all(got[odd].view(np.uint64) == 0) and np.all(ref[odd] == 0.0)


def test_mixed_extents_and_the_layout():
    """Axes of extent 1 carry no bit; entry ``b`` of the array has Z / Y on the axes where ``b`` is 1."""
    shape = (2, 1, 2, 2, 1)
    flips = [0, 0, 1, 0, 0]
    x = gaussian(8, "complex128", seed=3)
    got = spu.spectrum_model(x, shape, flips)
    assert got.shape == shape and spu.flip_mask(shape, flips) == 2
    for b in np.ndindex(*shape):
        row = [(2 if c else 1) if f else (3 if c else 0) for f, c in zip(flips, b)]
        assert abs(got[b] - pu.pauli_reference(x, shape, row)) <= spu.spectrum_tol(x, 8)
    assert abs(spu.spectrum_model(x, shape, [0] * 5)[(0,) * 5] - np.sum(np.abs(x) ** 2)) <= spu.spectrum_tol(x, 8)


@pytest.mark.parametrize("dtype", ["complex64", "float32"])
def test_half_integers_are_exact_in_the_model(dtype):
    L = 10
    shape = (2,) * L
    x = (np.clip(np.round(2 * gaussian(2 ** L, dtype, seed=7)), -4, 4) / 2).astype(dtype)
    for xm in (0, 1, 0b1000000101, 2 ** L - 1):
        flips = spu.flips_of(L, xm)
        got = spu.spectrum_model(x, shape, flips).reshape(-1)
        zs = [0, 1, xm, 2 ** L - 1, 0b0101010101, 0b1100110011]
        ref = pu.pauli_reference(x, shape, [spu.string_of(shape, flips, z) for z in zs])
        assert np.array_equal(got[zs], ref), (xm, got[zs], ref)


@pytest.mark.parametrize("dtype", ["complex64", "float32"])
def test_one_wrong_sign_of_a_median_term_exceeds_the_bound(dtype):
    """The bound is no licence: flipping the sign of one butterfly input of median size moves every value it feeds by
    twice its size, far past the bound."""
    L = 6
    shape = (2,) * L
    x = gaussian(2 ** L, dtype, seed=11)
    flips = [0] * L
    good = spu.spectrum_model(x, shape, flips).reshape(-1)
    u = np.abs(x.astype(np.complex128)) ** 2
    j = int(np.argsort(u)[u.size // 2])
    had = np.array([[(-1) ** bin(a & z).count("1") for a in range(2 ** L)] for z in range(2 ** L)], dtype=np.float64)
    v = u.copy()
    v[j] = -v[j]
    wrong = had @ v
    tol = spu.spectrum_tol(x, 2 ** L)
    assert np.all(np.abs(had @ u - good) <= tol)
    assert np.all(np.abs(wrong - good) > 100 * tol)


# ---- the plan ------------------------------------------------------------------------------------------------- #


def plan(dtype, L, xm):
    return runtime.pauli_spectrum_plan(dtype, (2,) * L, spu.flips_of(L, xm))


def test_the_plan_is_pinned():
    t = "spectrum_tile_kernel<c64>"
    p = "spectrum_pass_kernel"
    P = runtime.PauliSpectrumPlan
    assert plan("complex64", 0, 0) == P(0, 0, 0, 0, 0, (), 1, 256, (t,))
    assert plan("complex64", 12, 0) == P(12, 0, 0, 12, 0, (), 1, 8 << 12, (t,))
    assert plan("complex64", 12, 1) == P(12, 1, 1, 12, 0, (), 1, 8 << 12, (t,))
    assert plan("complex64", 12, 2) == P(12, 2, 2, 12, 0, (), 1, 8 << 12, (t,))
    assert plan("complex64", 13, 4095) == P(13, 4095, 2, 12, 1, (1,), 2, 8 << 13, (t, p))
    assert plan("complex64", 13, 4096) == P(13, 4096, 3, 12, 1, (1,), 2, 8 << 13, (t, p))
    assert plan("complex64", 20, 0) == P(20, 0, 0, 12, 1, (8,), 256, 8 << 20, (t, p))
    assert plan("complex64", 20, 3 << 11) == P(20, 3 << 11, 3, 12, 1, (8,), 256, 8 << 20, (t, p))
    assert plan("complex64", 21, 5) == P(21, 5, 2, 12, 2, (8, 1), 512, 8 << 21, (t, p, p))
    assert plan("complex64", 21, 1 << 20) == P(21, 1 << 20, 3, 12, 2, (8, 1), 512, 8 << 21, (t, p, p))
    assert plan("complex64", 28, 0) == P(28, 0, 0, 12, 2, (8, 8), 1 << 16, 8 << 28, (t, p, p))
    assert plan("complex64", 28, 1 << 27) == P(28, 1 << 27, 3, 12, 2, (8, 8), 1 << 16, 8 << 28, (t, p, p))
    assert plan("complex64", 29, 0).pass_bits == (8, 8, 1) and plan("float32", 40, 0).pass_bits == (8, 8, 8, 4)
    # the partner's place depends on the elements of a 16-byte group: 4 floats, 2 doubles / complex64, 1 complex128
    assert [plan(dt, 12, 2).partner for dt in ("float32", "float64", "complex64", "complex128")] == [1, 2, 2, 2]
    assert [plan(dt, 12, 1).partner for dt in ("float32", "float64", "complex64", "complex128")] == [1, 1, 1, 2]
    assert plan("float64", 12, 0).kernels == ("spectrum_tile_kernel<double>",)
    # axes of extent 1 carry no bit
    q = runtime.pauli_spectrum_plan("complex128", (2, 1, 2, 2, 1), [0, 0, 1, 0, 0])
    assert (q.bits, q.xm, q.partner) == (3, 2, 2)


def test_the_plan_function_refuses_what_the_call_refuses():
    lib = runtime.load()
    i64p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    words = np.full(runtime.PAULI_SPECTRUM_PLAN_WORDS, 7, np.int64)
    ext, fl = np.array([2, 2, 1], np.int64), np.array([1, 0, 0], np.uint8)

    def call(dtype=2, rank=3, e=ext, f=fl, w=words):
        return lib.ctg_pauli_spectrum_plan(dtype, rank, None if e is None else e.ctypes.data_as(i64p),
                                           None if f is None else f.ctypes.data_as(u8p), None if w is None else w.ctypes.data_as(i64p))

    bad = [dict(dtype=4), dict(dtype=-1), dict(e=None), dict(f=None), dict(w=None), dict(rank=-1),
           dict(e=np.array([2, 3, 1], np.int64)), dict(e=np.array([2, 0, 1], np.int64)), dict(f=np.array([2, 0, 0], np.uint8)),
           dict(f=np.array([0, 0, 1], np.uint8)),
           dict(rank=41, e=np.full(41, 2, np.int64), f=np.zeros(41, np.uint8))]            # past 2^40 elements
    for row in bad:
        assert call(**row) == -1, row
        assert lib.ctg_last_error() and np.all(words == 7)
    assert call() == 0 and words[0] == 2 and words[1] == 2
    for bad_ext, bad_fl in (([2, 3], [0, 0]), ([2, 1], [0, 1]), ([2, 2], [0, 2]), ([2, 2], [0]), ([2, 2], [0.5, 0]), ([2, 2], [-1, 0])):
        with pytest.raises(ValueError):
            runtime.pauli_spectrum_plan("complex64", bad_ext, bad_fl)


# ---- the Python layers ---------------------------------------------------------------------------------------- #


def test_requests_are_refused_before_the_device():
    tree = ca.ContractionTree(["abx", "xcd"], "abcd", dict(a=2, b=2, c=1, d=2, x=3))
    flags, several, select = spectrum_requests(tree, ["a", "d"])
    assert flags == [1, 0, 0, 1] and several and select is None
    flags, several, select = spectrum_requests(tree, ("d", "a"), ["XZIY", {"a": "Y", "d": "x"}, [("d", "Y"), ("a", "Y"), ("b", "Z")]])
    assert flags == [1, 0, 0, 1] and several and select.tolist() == [0b011, 0b100, 0b111]   # (strides 4, 2, 1, 1)
    assert spectrum_requests(tree, [], "IZII")[1:] == (False, pytest.approx([2]))
    assert spectrum_requests(tree, "a", "XIII")[0] == [1, 0, 0, 0]
    for flips, paulis in ((["e"], None), (["a", "a"], None), (["c"], None), (["a"], "IIII"), (["a"], "XIIX"), ([], "XIII"),
                          (["a"], ["XIII", "YIIY"]), (["a"], "XIIQ"), (["a"], "XII")):
        with pytest.raises(ValueError):
            spectrum_requests(tree, flips, paulis)
    wide = ca.ContractionTree(["abx", "xcd"], "abcd", dict(a=2, b=3, c=1, d=2, x=3))
    with pytest.raises(ValueError):
        spectrum_requests(wide, [])
    with pytest.raises(ValueError):
        wide.contract_pauli_spectrum([np.zeros((2, 3, 3)), np.zeros((3, 1, 2))])
    # up to 2^24 requests, where expectation takes 4096
    many = ["IZII"] * 5000
    assert spectrum_requests(tree, [], many)[2].shape == (5000,)
    with pytest.raises(ValueError):
        ca.pauli_requests(tree, many)
    for bad in (dict(qubits=[0, 0]), dict(qubits=[3]), dict(qubits=[1], fixed={1: 0}), dict(fixed={1: 2})):
        with pytest.raises(ValueError):
            circuits.z_correlations(3, [], **bad)


def test_symbols_sources_and_header():
    import __graft_entry__ as g

    for sym in ("ctg_exec_result_pauli_spectrum", "ctg_pauli_spectrum_plan"):
        assert sym in runtime.SYMBOLS and hasattr(runtime.load(), sym)
    assert "ctg_pauli_spectrum.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "ctg_pauli_spectrum.hip"))
    tool = open(os.path.join(ROOT, "tools", "result_resources.py")).read()
    assert '"ctg_pauli_spectrum.hip"' in tool
    header = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", header) and runtime.ABI_VERSION == 10
    assert re.search(r"#define\s+CTG_PAULI_SPECTRUM_MAX_SELECT\s+\(1 << 24\)", header)
    assert runtime.Executor.PAULI_SPECTRUM_MAX_SELECT == runtime.PAULI_SPECTRUM_MAX_SELECT == 1 << 24
    m = re.search(r"#define\s+CTG_PAULI_SPECTRUM_PLAN_WORDS\s+(\d+)", header)
    assert m and int(m.group(1)) == runtime.PAULI_SPECTRUM_PLAN_WORDS
    assert re.search(r"int\s+ctg_exec_result_pauli_spectrum\s*\(\s*ctg_exec\*\s*exec,\s*int64_t rank,\s*const int64_t\*\s*extents,"
                     r"\s*const uint8_t\*\s*flips,\s*int64_t m,\s*const int64_t\*\s*select,\s*double\*\s*out,\s*void\*\s*dev_out\)", header)
    assert hasattr(ca, "SpectrumResult") and hasattr(ca.ContractionTree, "contract_pauli_spectrum")
