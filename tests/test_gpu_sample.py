"""GPU suite: statistics of, and draws from, the result tensor on the device (csrc/ctg_sample.hip, DESIGN.md
section 10) -- ``HipContractor.sample`` / ``ContractionTree.contract_sample`` / ``circuits.sample_chaotic``.

Data reaches the result tensor bit for bit through a one-tensor tree (a single copy step).  The reference
sampler and the acceptance condition of a draw are in tests/sample_util.py; the condition is derived from the
error of two summation orders, never from what the device returns."""
import math
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits
from cotengra_amd.contractor import _tree_contractor
from oracle import contract_ref as orc

import sample_util as su

pytestmark = pytest.mark.gpu

B = 4096   # kSampleBlock of csrc/ctg_sample.hip
DTYPES = ["float32", "float64", "complex64", "complex128"]
HERE = os.path.dirname(os.path.abspath(__file__))


def one_tensor_tree(n):
    return ca.ContractionTree(["a"], "a", {"a": int(n)})


def gaussian(n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(n)
    return x.astype(dtype)


def draw(x, u, tree=None, **kw):
    tree = one_tensor_tree(x.size) if tree is None else tree
    return tree.contract_sample([x], len(u), uniforms=u, **kw)


def same(a, b):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.coords, b.coords)
    assert a.amplitudes.tobytes() == b.amplitudes.tobytes() and a.p.tobytes() == b.p.tobytes()
    assert (a.norm, a.sum_p2, a.max_p, a.argmax) == (b.norm, b.sum_p2, b.max_p, b.argmax)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17, 2 ** 20 + 3])
def test_draws_meet_the_interval_condition(n, dtype):
    x = gaussian(n, dtype, seed=n)
    u = su.uniforms_257(seed=n + 1)
    res = draw(x, u)
    p, c, t = su.check_draws(x, u, res.indices)
    assert res.amplitudes.dtype == x.dtype and res.amplitudes.tobytes() == x[res.indices].tobytes()
    assert np.array_equal(res.p, p[res.indices])
    assert res.coords.shape == (257, 1) and np.array_equal(res.coords[:, 0], res.indices)
    assert abs(res.norm - c[-1]) <= su.default_tol(p, c)
    assert res.exponent == 0.0


def test_exact_indices_away_from_boundaries():
    """No target within tol of a CDF boundary (asserted): the device's indices ARE numpy's."""
    n = 3 * B + 17
    x = gaussian(n, "complex128", seed=5)
    u = np.random.default_rng(6).random(257)
    p, c, t = su.reference(x, u)
    assert su.boundary_distance(c, t).min() > su.default_tol(p, c)
    res = draw(x, u)
    assert np.array_equal(res.indices, su.reference_indices(c, t))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["first", "last", "block_end", "block_start"])
def test_one_hot_every_draw_returns_it(where, dtype):
    n = 3 * B + 17
    pos = {"first": 0, "last": n - 1, "block_end": B - 1, "block_start": B}[where]
    x = np.zeros(n, dtype)
    x[pos] = -1.5
    res = draw(x, su.uniforms_257(seed=pos))
    assert np.all(res.indices == pos) and np.all(res.amplitudes == x[pos]) and np.all(res.p == 2.25)
    assert (res.norm, res.sum_p2, res.max_p, res.argmax) == (2.25, 2.25 ** 2, 2.25, pos)


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_zero_gap_and_zero_tail(dtype):
    """[0, B + 100) and [3B + 50, 3B + 60) hold data; between them lie zeros with the whole block [2B, 3B), behind
    them a zero tail longer than a block.  Uniforms on both sides of the gap, next to it."""
    n = 5 * B
    x = gaussian(n, dtype, seed=11)
    x[B + 100:3 * B + 50] = 0
    x[3 * B + 60:] = 0
    p = su.probabilities(x)
    c = np.cumsum(p)
    edge = c[B + 99] / c[-1]
    u = np.concatenate([su.uniforms_257(seed=12)[:-1], [edge * (1 - 1e-9), edge * (1 - 1e-15), edge * (1 + 1e-15),
                                                          edge * (1 + 1e-9), np.nextafter(edge, 0), np.nextafter(edge, 1),
                                                          np.nextafter(1.0, 0.0)]])
    res = draw(x, u)
    su.check_draws(x, u, res.indices)
    assert res.indices[256] < B + 100 and res.indices[259] >= 3 * B + 50
    assert res.indices.max() < 3 * B + 60
    assert np.all(p[res.indices] > 0)


def test_all_zero_raises():
    with pytest.raises(ValueError):
        draw(np.zeros(B + 5, "complex64"), np.array([0.25]))


def test_bad_uniforms_raise_and_launch_nothing():
    x = gaussian(B + 5, "complex64", seed=3)
    tree = one_tensor_tree(x.size)
    for bad in (float("nan"), 1.0, -0.25):
        with pytest.raises(ValueError):
            draw(x, np.array([0.5, bad]), tree=tree)
    # the library's own check, before its first launch: the scratch of the kernels does not exist yet
    ex = _tree_contractor(tree).setup(x)["exec"]
    before = ex.device_bytes()
    for bad in (float("nan"), 1.0):
        with pytest.raises(ValueError):
            ex.sample_result(np.array([0.5, bad]))
    assert ex.device_bytes() == before
    idx, _, _ = ex.sample_result(np.zeros(0))
    assert idx.size == 0 and ex.device_bytes() == before
    ex.zero_result()
    ex.run_slices()
    ex.sample_result(np.array([0.5]))
    assert ex.device_bytes() > before


def test_flat_targets_on_boundaries():
    n = 2 ** 13
    u = np.arange(n) / n
    res = draw(np.ones(n, "float64"), u)
    su.check_draws(np.ones(n), u, res.indices)
    assert res.norm == n and res.sum_p2 == n and res.max_p == 1.0 and res.argmax == 0


def test_range_of_36_decades_in_complex64():
    """Moduli log-uniform over 1e-18 ... 1: the squares span 36 decades, the small ones at the edge of what fp32
    holds; in double the sums keep every term."""
    n = 3 * B + 17
    rng = np.random.default_rng(21)
    mod = 10.0 ** rng.uniform(-18, 0, n)
    x = (mod * np.exp(2j * np.pi * rng.random(n))).astype("complex64")
    u = su.uniforms_257(seed=22)
    res = draw(x, u)
    p = su.probabilities(x)
    norm, q = math.fsum(p), math.fsum(p * p)
    assert abs(res.norm - norm) <= n * 2.0 ** -52 * norm
    assert abs(res.sum_p2 - q) <= n * 2.0 ** -52 * q
    su.check_draws(x, u, res.indices)
    assert res.amplitudes.tobytes() == x[res.indices].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_stats_match_numpy(dtype):
    n = 3 * B + 17
    x = gaussian(n, dtype, seed=31)
    p = su.probabilities(x)
    res = draw(x, np.array([0.5]))
    assert res.argmax == int(np.argmax(p)) and res.max_p == p.max()
    # a tie: the same largest value three times, in two blocks -- the lowest index wins
    big = 2 * np.abs(x).max()
    for pos in (5001, 5000, 100):
        x[pos] = big
    res = draw(x, np.array([0.5]))
    p = su.probabilities(x)
    assert res.argmax == 100 and res.max_p == p[100] == p.max()


def test_deterministic_across_runs_and_executors():
    n = 3 * B + 17
    x, y = gaussian(n, "complex64", seed=41), gaussian(n, "complex64", seed=42)
    u = su.uniforms_257(seed=43)
    tree = one_tensor_tree(n)
    first = draw(x, u, tree=tree)
    same(first, draw(x, u, tree=tree))
    other = draw(y, u, tree=tree)
    assert not np.array_equal(other.indices, first.indices)
    same(first, draw(x, u, tree=tree))
    same(first, draw(x, u))


def test_expression_sample_and_cache_bytes():
    """``ContractExpression.sample`` on a cached expression ("ab,bc->ac", a 96 x 80 result over two blocks): the draws
    meet the condition against what the expression itself returns, and the cache's byte count sees the scratch."""
    from cotengra_amd import interface

    rng = np.random.default_rng(71)
    a, b = rng.standard_normal((96, 7)), rng.standard_normal((7, 80))
    interface.clear_expression_cache()
    try:
        expr = ca.einsum_expression("ab,bc->ac", a.shape, b.shape, cache_expression=True)
        assert expr._cached
        out = np.asarray(expr(a, b))
        before = expr._bytes
        assert before == expr.device_bytes() > 0
        u = su.uniforms_257(seed=72)
        res = expr.sample(a, b, n_samples=257, uniforms=u)
        su.check_draws(out, u, res.indices)
        assert res.amplitudes.tobytes() == out.reshape(-1)[res.indices].tobytes()
        assert np.array_equal(np.ravel_multi_index(tuple(res.coords.T), out.shape), res.indices)
        assert expr._bytes == expr.device_bytes() > before
        # an expression built with strip_exponent samples its mantissa
        exs = ca.einsum_expression("ab,bc->ac", a.shape, b.shape, strip_exponent=True)
        mant, E = exs(a, b)
        rs = exs.sample(a, b, n_samples=257, uniforms=u)
        su.check_draws(np.asarray(mant), u, rs.indices)
        assert rs.exponent == E
        exs.close()
    finally:
        interface.clear_expression_cache()


@pytest.mark.parametrize("dtype", ["complex64", "float64"])
def test_torch_inputs_sample_the_torch_owned_result(dtype):
    """ROCm tensors in: torch owns the result tensor and the executor follows torch's current stream -- also a side
    stream.  The same draws as from numpy inputs."""
    import torch

    n = 3 * B + 17
    x = gaussian(n, dtype, seed=81)
    u = su.uniforms_257(seed=82)
    ref = draw(x, u)
    tree = one_tensor_tree(n)
    xt = torch.tensor(x, device="cuda")
    res = tree.contract_sample([xt], 257, uniforms=u)
    same(ref, res)
    su.check_draws(x, u, res.indices)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        same(ref, tree.contract_sample([xt], 257, uniforms=u))
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_golden_batch_m10_open8(dtype):
    tree = ca.tree_from_record(ca.load_network(os.path.join(HERE, "golden", "trees", "sycamore_m10_open8.json")))
    z = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_arrays.npz"))
    golden = np.load(os.path.join(HERE, "golden", "sycamore_m10_open8_expected.npz"))["amplitudes"]
    xs = [z[f"t{i}"].astype(dtype) for i in range(tree.N)]
    assert tree.nslices == 8 and golden.size == 256
    u = np.random.default_rng(51).random(4096)
    amps = np.asarray(tree.contract(xs))
    res = tree.contract_sample(xs, 4096, uniforms=u)
    p, c, t = su.check_draws(amps, u, res.indices)
    assert res.amplitudes.tobytes() == amps.reshape(-1)[res.indices].tobytes()
    assert res.coords.shape == (4096, 8)
    assert np.array_equal(np.ravel_multi_index(tuple(res.coords.T), amps.shape), res.indices)
    if dtype == "complex128":
        ref = float(np.sum(su.probabilities(golden)))
        assert abs(res.norm - ref) <= 1e-10 * ref
    # strip_exponent: draws from the mantissa, the exponent next to it
    mant, E = tree.contract(xs, strip_exponent=True)
    res_s = tree.contract_sample(xs, 4096, uniforms=u, strip_exponent=True)
    su.check_draws(np.asarray(mant), u, res_s.indices)
    assert res_s.exponent == E
    tol = 1e-10
    if dtype == "complex64":
        scale = np.abs(golden).max()
        tol = max(1e-5, 8.0 * np.abs(np.asarray(orc.contract(tree, xs)) - golden).max() / scale)
    assert abs(res_s.norm * 10.0 ** (2 * E) - res.norm) <= tol * res.norm


def random_circuit(n, depth, seed):
    """Sycamore-style layers: a random single-qubit gate on every qubit, then
    fSim gates on a brick pattern of neighbouring pairs."""
    rng = np.random.default_rng(seed)
    gates = []
    for d in range(depth):
        for q in range(n):
            name = ("x_1_2", "y_1_2", "hz_1_2", "rz")[int(rng.integers(0, 4))]
            gates.append((name, (q,), (float(rng.normal()),) if name == "rz" else ()))
        for q in range(d % 2, n - 1, 2):
            gates.append(("fs", (q, q + 1), (float(rng.normal()), float(rng.normal()))))
    return gates


def statevector(n, gates):
    psi = np.zeros([2] * n, complex)
    psi[(0,) * n] = 1
    for name, qs, ps in gates:
        U = circuits.gate_matrix(name, ps)
        if len(qs) == 1:
            psi = np.moveaxis(np.tensordot(U, psi, axes=([1], [qs[0]])), 0, qs[0])
        else:
            psi = np.moveaxis(
                np.tensordot(U.reshape(2, 2, 2, 2), psi, axes=([2, 3], [qs[0], qs[1]])), [0, 1], list(qs))
    return psi


def test_sample_chaotic_end_to_end():
    """12 qubits, 6 layers, 5 marginal qubits, 4 bunches x 64 draws in complex128 on a tree sliced on one output
    and two inner indices, against the dense state vector."""
    n, qs, seed = 12, [1, 3, 5, 6, 9], 61
    gates = random_circuit(n, 6, seed=7)
    psi = statevector(n, gates)
    inputs, output, sd, arrays = circuits.circuit_to_network(n, gates, "0?1?0??10?01", simplify=True, dtype="complex128")
    tree = ca.array_contract_tree(inputs, output, sd)
    big = max((p for p, _, _ in tree.traverse()), key=tree.get_size)
    inner = [ix for ix in tree.get_legs(big) if ix not in tree.output][:2]
    for ix in [tree.output[1]] + inner:
        tree.remove_ind_(ix)
    assert tree.nslices == 8
    tree.contract(arrays)   # (the executor exists from here on)
    fn = _tree_contractor(tree)
    before = sum(st["exec"].device_bytes() for st in fn._execs.values())
    out = circuits.sample_chaotic(n, gates, 256, qs, bunches=4, seed=seed, optimize=tree, dtype="complex128")
    after = sum(st["exec"].device_bytes() for st in fn._execs.values())
    assert after >= before and after > before   # (the issue's bound; and the scratch of the kernels is counted)
    templates, rng = circuits.chaotic_prefixes(n, qs, 4, seed)
    assert out["prefixes"] == templates and len(set(templates)) > 1
    assert len(out["bitstrings"]) == 256 and out["amplitudes"].shape == (256,)
    for b, template in enumerate(templates):
        u = rng.random(64)
        sel = tuple(slice(None) if ch == "?" else int(ch) for ch in template)
        sub = psi[sel].reshape(-1)
        mine = slice(64 * b, 64 * (b + 1))
        assert np.all(out["bunch"][mine] == b)
        strings = out["bitstrings"][mine]
        for s in strings:
            assert len(s) == n and all(s[q] == template[q] for q in range(n) if template[q] != "?")
        idx = np.array([int("".join(s[q] for q in qs), 2) for s in strings], dtype=np.int64)
        norm = float(np.sum(su.probabilities(sub)))
        su.check_draws(sub, u, idx, tol=1e-10 * norm)
        exact = np.array([psi[tuple(int(ch) for ch in s)] for s in strings])
        assert np.abs(out["amplitudes"][mine] - exact).max() <= 1e-11 * np.abs(psi).max()
        assert abs(out["norms"][b] - norm) <= 1e-10 * norm
    xeb = circuits.linear_xeb(len(qs), out["p"] / np.repeat(out["norms"], 64))
    assert np.isfinite(xeb)
