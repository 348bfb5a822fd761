"""GPU suite: the Pauli spectrum of the result tensor -- all strings of one X / Y pattern by a Walsh-Hadamard transform on
the device (csrc/ctg_pauli_spectrum.hip) -- ``Executor.pauli_spectrum``,
``HipContractor.pauli_spectrum``, ``ContractionTree.contract_pauli_spectrum``, ``ContractExpression.pauli_spectrum``,
``circuits.z_correlations``.

Data reaches the result tensor bit for bit through a one-tensor tree, as in tests/test_gpu_result_reduce.py.  The sharp
test needs no tolerance: tests/spectrum_util.py holds a numpy model of the arithmetic (``u``, then the butterflies over
the bits in ascending order, the sign, the zeros of real plans) and the device must equal it BIT FOR BIT on Gaussian
data.  Against ``pauli_util.pauli_reference`` and against section 16's ``pauli_result`` the derived bound
``spectrum_util.spectrum_tol`` applies; no ``z`` is excluded.

Shapes: the tile pass transforms bits 0 .. 11 of a chunk of 4096 elements, a strided pass up to 8 further bits.  L = 0,
1, 5: below a tile; 12: one tile; 13, 16, 20: a 1-bit, a 4-bit and a full strided pass; 21, 22: a 1-bit and a 2-bit
second strided pass.  Masks: 0 (the partner is the element itself), bit 0 and bit 1 (inside a 16-byte group for the
narrower types), bits 11 | 12 (the chunk boundary: another chunk AND another group), bit L - 1, all bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits, runtime
from cotengra_amd.contractor import _tree_contractor

import pauli_util as pu
import spectrum_util as spu
from test_gpu_pauli import strings_for
from test_gpu_result_reduce import resident
from test_gpu_sample import gaussian, one_tensor_tree, random_circuit, statevector

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "complex64", "complex128"]
TAG = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}
SIZES = [0, 1, 5, 12, 13, 16, 20, 21, 22]
MASKS = ["none", "bit0", "bit1", "bits11_12", "top", "all"]


def mask_of(kind, L):
    """The mask of a case, or None where the tensor does not have its bits."""
    if kind == "none":
        return 0
    if kind == "all":
        return (1 << L) - 1 if L >= 2 else None          # (L = 1: that is bit 0)
    need, xm = {"bit0": (1, 1), "bit1": (2, 2), "bits11_12": (13, 3 << 11), "top": (3, 1 << max(L - 1, 0))}[kind]
    return xm if L >= need else None


@functools.lru_cache(maxsize=2)
def tensor(L, dtype):
    x = gaussian(2 ** L, dtype, seed=100 + L)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=2)
def on_device(L, dtype):
    return resident(tensor(L, dtype))


def expected_plan(L, xm, dtype):
    """(partner, kernels) from the header's rules, not from the plan function."""
    V = 16 // np.dtype(dtype).itemsize
    partner = 0 if xm == 0 else 1 if xm < V else 2 if xm < 4096 else 3
    passes = 0 if L <= 12 else (L - 12 + 7) // 8
    return partner, (f"spectrum_tile_kernel<{TAG[dtype]}>",) + ("spectrum_pass_kernel",) * passes


# (dtype, L, kind) with consecutive cases on one tensor; a mask the tensor has no bits for is no case
CASES = [(dt, L, k) for dt in DTYPES for L in SIZES for k in MASKS if mask_of(k, L) is not None]


@pytest.mark.parametrize("dtype,L,kind", CASES)
def test_bit_for_bit_against_the_model(dtype, L, kind):
    xm = mask_of(kind, L)
    shape = (2,) * L
    flips = spu.flips_of(L, xm)
    x = tensor(L, dtype)
    ex = on_device(L, dtype)
    plan = ex.pauli_spectrum_plan(shape, flips)
    partner, kernels = expected_plan(L, xm, dtype)
    assert (plan.bits, plan.xm, plan.partner, plan.kernels) == (L, xm, partner, kernels), plan
    assert plan.tile_bits == min(L, 12) and sum(plan.pass_bits) == max(L - 12, 0) and plan.tiles == max(1, 2 ** L // 4096)
    got = ex.pauli_spectrum(shape, flips)
    assert got.shape == shape and got.dtype == np.float64
    spu.assert_same_bits(got, spu.spectrum_model(x, shape, flips), f"L={L} xm={xm:#x} {dtype}")
    assert ex.download_result().tobytes() == x.tobytes()


def test_the_partner_modes_are_all_reached():
    seen = {dt: {expected_plan(L, mask_of(k, L), dt)[0] for d, L, k in CASES if d == dt} for dt in DTYPES}
    assert seen["float32"] == seen["float64"] == seen["complex64"] == {0, 1, 2, 3} and seen["complex128"] == {0, 2, 3}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [13, 16])
def test_against_the_string_by_string_entry(L, dtype):
    """Every string of ``strings_for(L)`` (about 35 per L, some 70 in all) read from the spectrum of its own mask, against
    section 16's ``pauli_result`` within the sum of both bounds and against the reference within the spectrum's."""
    shape = (2,) * L
    x = tensor(L, dtype)
    ex = on_device(L, dtype)
    ops = strings_for(L)
    assert len(ops) >= 30
    each = ex.pauli_result(shape, ops)
    ref = pu.pauli_reference(x, shape, ops)
    tol, tol16 = spu.spectrum_tol(x, x.size), pu.pauli_tol(x, x.size)
    masks = runtime.pauli_masks(shape, ops)
    spectra, worst = {}, 0.0
    for s, (xm, zm, ny) in enumerate(masks):
        if xm not in spectra:
            spectra[xm] = ex.pauli_spectrum(shape, spu.flips_of(L, xm)).reshape(-1)
        v = spectra[xm][zm]
        assert spu.string_of(shape, spu.flips_of(L, xm), zm) == ops[s].tolist()
        worst = max(worst, abs(v - ref[s]) / tol)
        assert abs(v - ref[s]) <= tol and abs(v - each[s]) <= tol + tol16, (s, v, ref[s], each[s])
        if np.dtype(dtype).kind != "c" and ny % 2:
            assert v == 0.0 and not np.signbit(v) and each[s] == 0.0
    print(f"spectrum L={L} {dtype}: {len(spectra)} masks, {len(ops)} strings, max err/bound={worst:.3e}")
    assert len(spectra) >= 10


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_integers_are_exact(dtype):
    """``test_gpu_pauli.test_half_integers_are_exact``'s data at 2^20: every product is a multiple of 1/4, every ``u`` at
    most 16 in size and every partial sum of 2^20 of them exact in fp64 -- so the part of ``u`` that does not belong to a
    string cancels exactly and the device must equal the reference bit for bit, whatever the order."""
    L = 20
    x = (np.clip(np.round(2 * gaussian(2 ** L, dtype, seed=7)), -4, 4) / 2).astype(dtype)
    ex = resident(x)
    held = ex.download_result().tobytes()                 # (x up to the sign of its zeros: the copy step adds to +0.0)
    shape = (2,) * L
    ops = strings_for(L)
    ref = pu.pauli_reference(x, shape, ops)
    spectra = {}
    for s, (xm, zm, ny) in enumerate(runtime.pauli_masks(shape, ops)):
        if xm not in spectra:
            spectra[xm] = ex.pauli_spectrum(shape, spu.flips_of(L, xm)).reshape(-1)
        assert spectra[xm][zm] == ref[s], (s, xm, zm, spectra[xm][zm], ref[s])
    assert np.count_nonzero(ref) >= 10
    assert ex.download_result().tobytes() == held


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_real_plans_write_positive_zeros_for_odd_ny(dtype):
    L = 14
    xm = (1 << 13) | (1 << 11) | 5
    shape = (2,) * L
    got = on_device(L, dtype).pauli_spectrum(shape, spu.flips_of(L, xm)).reshape(-1)
    odd = spu.popcount(np.arange(2 ** L) & xm) % 2 == 1
    assert odd.sum() == 2 ** (L - 1)
    assert np.all(got[odd].view(np.uint64) == 0)
    assert np.count_nonzero(got[~odd]) == 2 ** (L - 1)


def device_spectrum(ex, shape, flips, select=None, fill=None):
    """``(what the call returns, dev_out downloaded)`` with a torch buffer as ``dev_out``."""
    import torch

    buf = torch.empty(shape, dtype=torch.float64, device="cuda")
    if fill is not None:
        buf.fill_(fill)
    out = ex.pauli_spectrum(shape, flips, select=select, dev_out=buf.data_ptr())
    torch.cuda.synchronize()
    return out, buf.cpu().numpy()


def test_the_same_bits_whatever_the_route():
    """select, dev_out, a repeated call, calls of other entries in the same scratch between, a fresh executor."""
    L, dtype = 21, "complex64"
    shape = (2,) * L
    xm = (3 << 11) | 1
    flips = spu.flips_of(L, xm)
    x = tensor(L, dtype)
    ex = on_device(L, dtype)
    whole = ex.pauli_spectrum(shape, flips)
    rng = np.random.default_rng(21)
    select = np.concatenate([[0, 2 ** L - 1, xm, 4096, 4095], rng.integers(0, 2 ** L, size=1000)]).astype(np.int64)
    picked = ex.pauli_spectrum(shape, flips, select=select)
    spu.assert_same_bits(picked, whole.reshape(-1)[select], "select")
    none, dev = device_spectrum(ex, shape, flips)
    assert none is None
    spu.assert_same_bits(dev, whole, "dev_out")
    picked2, dev2 = device_spectrum(ex, shape, flips, select=select[:7], fill=3.0)
    spu.assert_same_bits(picked2, picked[:7], "select with dev_out")
    spu.assert_same_bits(dev2, whole, "dev_out with select")
    ex.topk_result(100)
    ex.rdm_result(shape, [1, 1] + [0] * (L - 2))
    spu.assert_same_bits(ex.pauli_spectrum(shape, flips), whole, "after top-k and rdm in the same scratch")
    spu.assert_same_bits(resident(x).pauli_spectrum(shape, flips), whole, "a fresh executor")
    assert ex.pauli_spectrum(shape, flips, select=np.zeros(0, np.int64)).shape == (0,)
    assert ex.download_result().tobytes() == x.tobytes()


def test_the_scratch_is_counted():
    L = 16
    shape = (2,) * L
    x = gaussian(2 ** L, "complex64", seed=5)
    ex = resident(x)
    before = ex.device_bytes()
    device_spectrum(ex, shape, [0] * L)
    assert ex.device_bytes() - before < 8 * 2 ** L        # (dev_out holds the vector: the statistics' blocks at most)
    ex.pauli_spectrum(shape, [0] * L)
    grown = ex.device_bytes()
    assert grown - before >= ex.pauli_spectrum_plan(shape, [0] * L).scratch_bytes == 8 * 2 ** L
    ex.pauli_spectrum(shape, [0] * L, select=np.arange(10))
    assert ex.device_bytes() >= grown + 2 * 256           # (the select table and its values)


def raw_call(ex, rank, ext, flips, m, select, out, dev_out=None, handle="own"):
    i64p, u8p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    return runtime.load().ctg_exec_result_pauli_spectrum(
        ex.handle if handle == "own" else handle, rank, None if ext is None else ext.ctypes.data_as(i64p),
        None if flips is None else flips.ctypes.data_as(u8p), m, None if select is None else select.ctypes.data_as(i64p),
        None if out is None else out.ctypes.data_as(dp), C.c_void_p(dev_out))


def test_refusals_through_the_c_abi():
    import torch

    L = 13
    n = 2 ** L
    x = gaussian(n, "complex64", seed=13)
    ex = resident(x)
    before = ex.device_bytes()
    ext = np.full(L, 2, np.int64)
    fl = np.zeros(L, np.uint8)
    fl[0] = 1
    out = np.full(n, 7.0)
    sel = np.array([0, 5, n - 1], np.int64)
    buf = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    dev = buf.data_ptr()
    res = ex.result_ptr()

    def ext_with(a, v):
        e = ext.copy()
        e[a] = v
        return e

    def fl_with(a, v):
        f = fl.copy()
        f[a] = v
        return f

    wide = np.array([2] * 12 + [1, 2], np.int64)          # (an axis of extent 1)
    bad = [
        dict(handle=None),                                                     # a null exec
        dict(ext=None), dict(flips=None),
        dict(rank=-1), dict(rank=L - 1),                                       # rank < 0; a wrong product
        dict(ext=ext_with(3, 0)), dict(ext=ext_with(3, 1)),
        dict(rank=3, ext=np.array([2 ** 21, 2 ** 21, 2], np.int64), flips=np.zeros(3, np.uint8)),
        dict(rank=2, ext=np.array([4, 2048], np.int64), flips=np.zeros(2, np.uint8)),            # an extent above 2
        dict(flips=fl_with(2, 2)), dict(flips=fl_with(2, 255)),                # a flip code above 1
        dict(rank=14, ext=wide, flips=np.array([0] * 12 + [1, 0], np.uint8)),  # a flip on an axis of extent 1
        dict(out=None, dev_out=None),                                          # no output
        dict(select=sel, m=-1), dict(select=sel, m=2 ** 24 + 1),               # m out of range
        dict(select=np.array([0, n], np.int64), m=2), dict(select=np.array([-1, 0], np.int64), m=2),
        dict(select=sel, m=3, out=None),                                       # a select table with nowhere to go
        dict(dev_out=res), dict(dev_out=res + 8 * n - 8), dict(dev_out=res - 8 * n + 8),         # overlapping the result
        dict(dev_out=dev + 4),                                                 # misaligned
    ]
    for row in bad:
        a = dict(rank=L, ext=ext, flips=fl, m=0, select=None, out=out, dev_out=dev, handle="own")
        a.update(row)
        assert raw_call(ex, a["rank"], a["ext"], a["flips"], a["m"], a["select"], a["out"], a["dev_out"], a["handle"]) == -1, row
        assert runtime.load().ctg_last_error()
        assert np.all(out == 7.0)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    assert ex.device_bytes() == before                    # (nothing was launched, not even the scratch reserved)
    assert ex.download_result().tobytes() == x.tobytes()
    # ... and the binding raises ValueError for them
    for bad_ext, bad_fl in (([2] * 12, fl[:12]), ([4, 2048], [0, 0]), (ext, fl_with(2, 2)), (wide, [0] * 12 + [1, 0]), (ext, fl[:5])):
        with pytest.raises(ValueError):
            ex.pauli_spectrum(bad_ext, bad_fl)
    with pytest.raises(ValueError):
        ex.pauli_spectrum(ext, fl, select=[n])
    # a following valid call is correct, to both outputs
    assert raw_call(ex, L, ext, fl, 0, None, out, dev) == 0
    torch.cuda.synchronize()
    model = spu.spectrum_model(x, (2,) * L, fl.tolist()).reshape(-1)
    spu.assert_same_bits(out, model, "host out")
    spu.assert_same_bits(buf.cpu().numpy(), model, "dev_out")
    # a NaN member: CTG_E_NORM, through every layer
    badx = x.copy()
    badx[4097] = np.nan
    exn = resident(badx)
    out[:] = 7.0
    assert raw_call(exn, L, ext, fl, 0, None, out, None) == -6 and np.all(out == 7.0)
    with pytest.raises(ValueError):
        exn.pauli_spectrum(ext, fl)
    # an all-zero tensor: zeros, no error
    zz = resident(np.zeros(n, "complex64")).pauli_spectrum(ext, fl)
    assert zz.shape == (2,) * L and not zz.any()


def circuit_tree(n, gates, dtype):
    from cotengra_amd.interface import array_contract_tree

    inputs, output, size_dict, arrays = circuits.circuit_to_network(n, gates, "?" * n, simplify=True, dtype=dtype)
    return array_contract_tree(inputs, output, size_dict, optimize="greedy"), arrays


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_through_the_layers_on_a_circuit(dtype):
    n = 10
    gates = random_circuit(n, 5, seed=3)
    psi = statevector(n, gates)
    rel = 1e-10 if dtype == "complex128" else 1e-5        # the library's promise per amplitude
    tree, arrays = circuit_tree(n, gates, dtype)
    out = list(tree.output)
    x = np.asarray(tree.contract(arrays))                 # (what the result tensor holds)
    shape = x.shape
    assert shape == (2,) * n
    flips = [out[2], out[7]]
    flags = [1 if ix in flips else 0 for ix in out]
    r = tree.contract_pauli_spectrum([], flips=flips, reuse=True)                                 # after __call__
    assert isinstance(r, ca.SpectrumResult) and r.values.shape == shape and r.exponent == 0.0
    spu.assert_same_bits(r.values, spu.spectrum_model(x, shape, flags), "reuse after the call")
    assert abs(r.norm - 1) <= 4 * rel
    fresh = tree.contract_pauli_spectrum(arrays, flips=flips)
    spu.assert_same_bits(fresh.values, r.values, "a fresh contraction")
    # every entry against the state vector
    texts = ["IIXIIIIXII", "ZIYIIIIXIZ", "IIYZZIIYII", "ZZXZZZZYZZ"]
    ref = pu.pauli_reference(psi, psi.shape, [pu.codes(t) for t in texts])
    picked = tree.contract_pauli_spectrum([], flips=flips, paulis=texts, reuse=True)
    assert picked.values.shape == (4,) and np.all(np.abs(picked.values - ref) <= 8 * rel)
    for t, v in zip(texts, picked.values):
        z = tuple(1 if c in "YZ" else 0 for c in t)
        assert v == r.values[z]
    # ... and against expectation: the same quantity, other bits
    each = tree.contract_expectation([], texts, reuse=True)
    assert np.all(np.abs(each.values - picked.values) <= spu.spectrum_tol(x, x.size) + pu.pauli_tol(x, x.size))
    one = _tree_contractor(tree).pauli_spectrum(flips=flips, paulis={out[2]: "Y", out[7]: "x", out[0]: "Z"}, reuse=True)
    assert np.ndim(one.values) == 0 and one.values == r.values[(1, 0, 1) + (0,) * 7]
    # a request whose X / Y are not exactly on flips: refused before the device is touched
    for wrong in ("IIXIIIIIII", "XIXIIIIXII", "IIZIIIIXII"):
        with pytest.raises(ValueError):
            tree.contract_pauli_spectrum([], flips=flips, paulis=[texts[0], wrong], reuse=True)
    for wrong in (["nope"], [out[2], out[2]]):
        with pytest.raises(ValueError):
            tree.contract_pauli_spectrum([], flips=wrong, reuse=True)
    assert tree.contract_pauli_spectrum([], flips=flips, paulis=texts[1], reuse=True).values == picked.values[1]
    # sliced, an output index among the sliced ones: the same values within the library's promise
    tree2, arrays2 = circuit_tree(n, gates, dtype)
    big = max((p for p, _, _ in tree2.traverse()), key=tree2.get_size)
    inner = [ix for ix in tree2.get_legs(big) if ix not in tree2.output][:1]
    for ix in [tree2.output[4]] + inner:
        tree2.remove_ind_(ix)
    assert tree2.nslices > 1 and tree2.gathered_shape() == (2,) * n and list(tree2.output) == out
    sliced = tree2.contract_pauli_spectrum(arrays2, flips=flips)
    assert sliced.values.shape == shape and np.all(np.abs(sliced.values - r.values) <= 8 * rel)


def test_torch_inputs_get_a_device_tensor():
    import torch

    n = 8
    tree, arrays = circuit_tree(n, random_circuit(n, 4, seed=5), "complex64")
    host = tree.contract_pauli_spectrum(arrays)
    r = tree.contract_pauli_spectrum([torch.as_tensor(a).cuda() for a in arrays])
    assert torch.is_tensor(r.values) and r.values.is_cuda and r.values.dtype == torch.float64
    spu.assert_same_bits(r.values.cpu().numpy(), host.values, "torch inputs")


def test_expression_pauli_spectrum():
    from cotengra_amd import interface

    rng = np.random.default_rng(71)
    a, b = rng.standard_normal((2, 2, 7)), rng.standard_normal((7, 2, 2))
    interface.clear_expression_cache()
    try:
        expr = ca.einsum_expression("xab,bcy->xacy", a.shape, b.shape, cache_expression=True)
        out = np.asarray(expr(a, b))
        before = expr._bytes
        r = expr.pauli_spectrum(a, b, flips=["x", "y"])
        spu.assert_same_bits(r.values, spu.spectrum_model(out, out.shape, [1, 0, 0, 1]), "expression")
        assert expr._bytes == expr.device_bytes() > before        # (the scratch is counted)
        wide = ca.einsum_expression("xab,bcy->xacy", (2, 3, 7), (7, 2, 2))
        with pytest.raises(ValueError):
            wide.pauli_spectrum(rng.standard_normal((2, 3, 7)), b)    # an output index of extent 3
        wide.close()
    finally:
        interface.clear_expression_cache()


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_z_correlations_against_the_state_vector(dtype):
    n = 10
    gates = random_circuit(n, 5, seed=9)
    psi = statevector(n, gates)
    rel = 1e-10 if dtype == "complex128" else 1e-5
    p = np.abs(psi) ** 2
    sign = lambda q: np.array([1.0, -1.0]).reshape((1,) * q + (2,) + (1,) * (n - q - 1))   # noqa: E731
    z_ref = np.array([np.sum(p * sign(q)) for q in range(n)])
    zz_ref = np.array([[np.sum(p * sign(a) * sign(b)) for b in range(n)] for a in range(n)])
    z, zz, conn, norm = circuits.z_correlations(n, gates, dtype=dtype)
    assert z.shape == (n,) and zz.shape == conn.shape == (n, n) and abs(norm - 1) <= 4 * rel
    assert np.all(np.abs(z - z_ref) <= 8 * rel) and np.all(np.abs(zz - zz_ref) <= 8 * rel)
    assert np.array_equal(zz, zz.T) and np.all(np.diag(zz) == 1.0)
    assert np.all(np.abs(conn - (zz_ref - np.outer(z_ref, z_ref))) <= 32 * rel)
    # a subset in another order, two qubits projected
    fixed = {1: 1, 7: 0}
    sub = np.take(np.take(psi, 1, axis=1), 0, axis=6)
    ps = np.abs(sub) ** 2
    pn = float(ps.sum())
    qs = [9, 0, 4]
    ax = {9: 7, 0: 0, 4: 3}                               # (axes of what is left)
    sg = lambda q: np.array([1.0, -1.0]).reshape((1,) * ax[q] + (2,) + (1,) * (8 - ax[q] - 1))   # noqa: E731
    z, zz, conn, norm = circuits.z_correlations(n, gates, qubits=qs, fixed=fixed, dtype=dtype)
    assert abs(norm - pn) <= 4 * rel * pn
    assert np.all(np.abs(z - np.array([np.sum(ps * sg(q)) / pn for q in qs])) <= 8 * rel)
    assert abs(zz[0, 2] - np.sum(ps * sg(9) * sg(4)) / pn) <= 8 * rel
    for bad in (dict(qubits=[0, 0]), dict(qubits=[10]), dict(qubits=[1], fixed={1: 0}), dict(fixed={1: 2})):
        with pytest.raises(ValueError):
            circuits.z_correlations(n, gates, dtype=dtype, **bad)
