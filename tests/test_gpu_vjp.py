"""GPU suite: gradients of sliced tree contractions (VJP plans, cotengra_amd/vjp.py) and the torch
autograd route through ``HipContractor``."""
import os

import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd.contractor import HipContractor
from cotengra_amd.plan import KIND_ACCUM
from cotengra_amd.vjp import compile_vjp
from oracle.plan_interp import run_plan

import golden_util as G
import vjp_util as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_CASES = [c for c in G.cases("tree")
              if c["name"] not in ("C5_hyper200", "C4_m20_w30_narrow20") and c["stats"]["max_size"] <= 1 << 16]
SINGLE = {"complex64": "complex128", "float32": "float64"}


def _case(name):
    return next(c for c in G.cases("tree") if c["name"] == name)


def _close(tree):
    for fn in tree.contraction_cores.values():
        if isinstance(fn, HipContractor):
            fn.close()


@pytest.mark.parametrize("case", TREE_CASES, ids=[c["name"] for c in TREE_CASES])
def test_vjp_golden_sweep(case):
    for dt in ("complex128", "float64", "complex64", "float32"):
        wide = SINGLE.get(dt, dt)
        tree = G.tree_of(case)
        arrays = G.arrays_of(case, wide, tree)
        h = V.cotangent(tree, wide)
        ref = V.reference_vjp(tree, arrays, h)
        xs, hx = [a.astype(dt) for a in arrays], h.astype(dt)
        got = tree.contract_vjp(xs, hx)
        if dt in SINGLE:
            plan = compile_vjp(tree, dt)
            npy = V.split_grads(plan, run_plan(plan, xs + [hx]), [a.shape for a in xs])
        for i, (g, r) in enumerate(zip(got, ref)):
            assert g.dtype == np.dtype(dt)
            gate = 1e-10 if dt not in SINGLE else max(1e-5, 8 * G.relerr(npy[i], r))
            assert G.relerr(g, r) <= gate, (case["name"], dt, i)
        _close(tree)


@pytest.mark.parametrize("name", ["rand_s42_r2_o1_hi0_ho0", "lattice4x4_sliced",
                                  "rand_s42_r2_o1_hi0_ho0_outsliced", "preproc_s0_a"])
def test_vjp_gradcheck(name):
    import torch

    case = _case(name)
    tree = G.tree_of(case)
    xs = [torch.tensor(a, device="cuda", requires_grad=True) for a in G.arrays_of(case, "complex128", tree)]
    assert torch.autograd.gradcheck(lambda *x: tree.contract(list(x)), xs, fast_mode=True, atol=1e-8, rtol=1e-6)
    _close(tree)


def _m10():
    rec = ca.load_network(os.path.join(ROOT, "tests", "golden", "trees", "sycamore_m10.json"))
    z = np.load(os.path.join(ROOT, "tests", "golden", "sycamore_m10_arrays.npz"))
    tree = ca.tree_from_record(rec)
    return tree, [z[f"t{i}"] for i in range(tree.N)]


def test_vjp_sycamore_m10_backward():
    import torch

    tree, arrays = _m10()
    xs = [torch.tensor(a, device="cuda", requires_grad=True) for a in arrays]
    out = tree.contract(xs)
    (out.abs() ** 2).sum().backward()
    cs = [torch.tensor(a, requires_grad=True) for a in arrays]
    ref = tree.contract(cs, implementation=(torch.einsum, torch.tensordot))
    (ref.abs() ** 2).sum().backward()
    for x, c in zip(xs, cs):
        assert G.relerr(x.grad.cpu().numpy(), c.grad.numpy()) <= 1e-10
    _close(tree)


def test_vjp_forward_value_unchanged():
    import torch

    tree, arrays = _m10()
    plain = tree.contract([torch.tensor(a.astype("complex64"), device="cuda") for a in arrays])
    xs = [torch.tensor(a.astype("complex64"), device="cuda", requires_grad=True) for a in arrays]
    with_grad = tree.contract(xs)
    assert with_grad.grad_fn is not None
    assert torch.equal(plain, with_grad.detach())
    _close(tree)


def test_vjp_partial_gradients():
    import torch

    case = _case("lattice4x4_sliced")
    tree = G.tree_of(case)
    arrays = G.arrays_of(case, "complex128", tree)
    arrays[1] = arrays[1].real.copy()          # a real leaf in a complex network
    xs = [torch.tensor(a, device="cuda", requires_grad=i in (1, 2)) for i, a in enumerate(arrays)]
    xs[3] = arrays[3]                          # a numpy constant
    out = tree.contract(xs)
    (out.abs() ** 2).sum().backward()
    assert xs[0].grad is None and xs[4].grad is None
    assert xs[1].grad.dtype == torch.float64 and xs[2].grad.dtype == torch.complex128
    cs = [torch.tensor(a, requires_grad=i in (1, 2)) for i, a in enumerate(arrays)]
    ref = tree.contract([c.to(torch.complex128) for c in cs], implementation=(torch.einsum, torch.tensordot))
    (ref.abs() ** 2).sum().backward()
    for i in (1, 2):
        assert G.relerr(xs[i].grad.cpu().numpy(), cs[i].grad.numpy()) <= 1e-10
    _close(tree)


def test_vjp_upload_scale_per_leaf():
    case = _case("lattice4x4_sliced")
    tree = G.tree_of(case)
    arrays = G.arrays_of(case, "complex128", tree)
    arrays[0] = arrays[0] * 2.0 ** 40
    arrays[5] = arrays[5] * 2.0 ** -40
    h = V.cotangent(tree, "complex128")
    ref = V.reference_vjp(tree, arrays, h)
    xs, hx = [a.astype("complex64") for a in arrays], h.astype("complex64")
    got = tree.contract_vjp(xs, hx)
    plan = compile_vjp(tree, "complex64")
    npy = V.split_grads(plan, run_plan(plan, xs + [hx]), [a.shape for a in xs])
    for i, (g, r) in enumerate(zip(got, ref)):
        assert G.relerr(g, r) <= max(1e-5, 8 * G.relerr(npy[i], r)), i
    _close(tree)


def test_vjp_repeated_calls():
    case = _case("rand_s42_r3_o2_hi2_ho2_sliced")
    tree = G.tree_of(case)
    fn = HipContractor(tree)
    for seed in (1, 2):
        arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=seed, dtype="complex128")
        h = V.cotangent(tree, "complex128", seed=seed)
        got = fn.vjp(*arrays, cotangent=h)
        for g, r in zip(got, V.reference_vjp(tree, arrays, h)):
            assert G.relerr(g, r) <= 1e-10, seed
    fn.close()


def test_vjp_repeated_calls_single_precision():
    """complex64: two different uploads on one contractor -- the second with every leaf and the cotangent scaled by
    powers of two inside the upload window [2^-32, 2^32), so that the kernels see them -- against the reference under
    this file's gate, and the same bits as a contractor that only ever saw that upload."""
    case = _case("rand_s42_r3_o2_hi2_ho2_sliced")
    tree = G.tree_of(case)
    plan = compile_vjp(tree, "complex64")
    fn = HipContractor(tree)
    for seed, shifts in ((1, None), (2, (-20, 5, 5)), (1, None)):
        arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=seed, dtype="complex128")
        h = V.cotangent(tree, "complex128", seed=seed)
        if shifts is not None:
            arrays = [G.scaled_in_window(a, shifts[i % 3]) for i, a in enumerate(arrays)]
            h = G.scaled_in_window(h, -12)
        ref = V.reference_vjp(tree, arrays, h)
        xs, hx = [a.astype("complex64") for a in arrays], h.astype("complex64")
        for x in xs + [hx]:
            G.assert_in_upload_window(x)
        got = fn.vjp(*xs, cotangent=hx)
        npy = V.split_grads(plan, run_plan(plan, xs + [hx]), [a.shape for a in xs])
        fresh_fn = HipContractor(tree)
        fresh = fresh_fn.vjp(*xs, cotangent=hx)
        fresh_fn.close()
        for i, (g, r) in enumerate(zip(got, ref)):
            assert G.relerr(g, r) <= max(1e-5, 8 * G.relerr(npy[i], r)), (seed, i)
            assert np.array_equal(g, fresh[i]), (seed, i)
    fn.close()


def test_vjp_slice_batching_bit_identical(monkeypatch):
    case = _case("lattice8x8_sliced")
    outs = []
    for cap in ("1", None):
        if cap is None:
            monkeypatch.delenv("CTG_SLICE_BATCH", raising=False)
        else:
            monkeypatch.setenv("CTG_SLICE_BATCH", cap)
        tree = G.tree_of(case)
        arrays = G.arrays_of(case, "complex64", tree)
        fn = HipContractor(tree)
        outs.append(fn.vjp(*arrays, cotangent=V.cotangent(tree, "complex64")))
        fn.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_vjp_grouped_accumulate_launch():
    case = _case("C2_lattice8x8_d4")
    tree = G.tree_of(case)
    arrays = G.arrays_of(case, "complex64", tree)
    fn = HipContractor(tree)
    fn.vjp(*arrays, cotangent=V.cotangent(tree, "complex64"))
    st = next(v for k, v in fn._execs.items() if "vjp" in k)
    plan, ex = st["plan"], st["exec"]
    names = ex.step_kernels()
    acc = [i for i, s in enumerate(plan.steps) if s.kind == KIND_ACCUM]
    assert len(acc) == 64 and all(names[i] == "accum_group_kernel" for i in acc)
    ns, nl = ex.launch_count()
    ex_f = fn.setup(*arrays)["exec"]
    assert ns - nl >= 63
    fwd = ex_f.step_kernels()
    assert [n for n, s in zip(fwd, ex_f.plan.steps) if s.kind == KIND_ACCUM] == ["accum_kernel"]
    fn.close()


def test_conjugate_view_inputs():
    import torch

    case = _case("lattice4x4_sliced")
    tree = G.tree_of(case)
    xs = [torch.tensor(a, device="cuda") for a in G.arrays_of(case, "complex64", tree)]
    a = tree.contract([xs[0].conj()] + xs[1:])
    b = tree.contract([xs[0].conj().resolve_conj()] + xs[1:])
    assert torch.equal(a, b)
    _close(tree)
