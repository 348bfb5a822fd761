"""CPU suite: gradients of sliced tree contractions (cotengra_amd/vjp.py).

* every golden tree case, in complex128: the VJP plan run through the numpy plan interpreter (the
  kernels' addressing semantics) equals torch autograd through the per-op plug-in;
* ``wrt`` subsets drop pair steps and keep the gradients of the leaves that remain;
* ``ctg_plan_create`` rejects a plan whose consecutive accumulate steps write overlapping ranges
  (they would race inside one grouped launch).
"""
import numpy as np
import pytest

from cotengra_amd.plan import KIND_ACCUM, KIND_PAIR
from cotengra_amd.vjp import compile_vjp
from oracle.plan_interp import run_plan

import golden_util as G
import vjp_util as V

TREE_CASES = G.cases("tree")
SLOW = {"C5_hyper200", "C4_m20_w30_narrow20"}


def _vjp_on_cpu(tree, arrays, h, wrt=None, ids=None):
    plan = compile_vjp(tree, "complex128", wrt=wrt)
    flat = run_plan(plan, list(arrays) + [h], slice_ids=ids)
    return plan, V.split_grads(plan, flat, [a.shape for a in arrays])


@pytest.mark.parametrize("case", TREE_CASES, ids=[c["name"] for c in TREE_CASES])
def test_vjp_plan_matches_autograd(case):
    if case["name"] in SLOW or case["stats"]["max_size"] > 1 << 16:
        pytest.skip("plan interpreter is for small cases")
    tree = G.tree_of(case)
    arrays = G.arrays_of(case, "complex128", tree)
    h = V.cotangent(tree, "complex128")
    ids = V.slice_ids_of(tree, case["slice_ids"])
    plan, got = _vjp_on_cpu(tree, arrays, h, ids=ids)
    ref = V.reference_vjp(tree, arrays, h, ids=ids)
    assert sum(s.kind == KIND_ACCUM for s in plan.steps) == tree.N
    for i, (g, r) in enumerate(zip(got, ref)):
        assert G.relerr(g, r) <= 1e-10, (case["name"], i)


def test_vjp_plan_float64():
    case = next(c for c in TREE_CASES if c["name"] == "rand_s42_r3_o2_hi2_ho2_sliced")
    tree = G.tree_of(case)
    arrays = G.arrays_of(case, "float64", tree)
    h = V.cotangent(tree, "float64")
    plan = compile_vjp(tree, "float64")
    got = V.split_grads(plan, run_plan(plan, list(arrays) + [h]), [a.shape for a in arrays])
    for g, r in zip(got, V.reference_vjp(tree, arrays, h)):
        assert G.relerr(g, r) <= 1e-10


@pytest.mark.parametrize("name", ["lattice4x4_sliced", "rand_s666_r3_o2_hi1_ho0_outsliced", "preproc_s1_ac"])
def test_vjp_wrt_subset(name):
    case = next(c for c in TREE_CASES if c["name"] == name)
    tree = G.tree_of(case)
    arrays = G.arrays_of(case, "complex128", tree)
    h = V.cotangent(tree, "complex128")
    full, g_full = _vjp_on_cpu(tree, arrays, h)
    wrt = [0, tree.N - 1]
    part, g_part = _vjp_on_cpu(tree, arrays, h, wrt=wrt)
    n_pairs = lambda p: sum(s.kind == KIND_PAIR for s in p.steps)  # noqa: E731
    assert n_pairs(part) < n_pairs(full)
    assert sum(s.kind == KIND_ACCUM for s in part.steps) == len(wrt)
    assert part.result_elems < full.result_elems
    for i in range(tree.N):
        if i in wrt:
            assert G.relerr(g_part[i], g_full[i]) <= 1e-12
        else:
            assert g_part[i] is None


def test_vjp_size_limit_and_arena():
    case = next(c for c in TREE_CASES if c["name"] == "lattice8x8_sliced")
    tree = G.tree_of(case)
    plan = compile_vjp(tree, "complex64")
    # every per-slice intermediate the backward reads is retained: more than the forward's arena
    from cotengra_amd.plan import compile_tree

    assert plan.arena_elems >= compile_tree(tree, "complex64", fuse=False).arena_elems
    assert plan.input_sizes[-1] == int(np.prod(tree.gathered_shape()))
    with pytest.raises(ValueError):
        compile_vjp(tree, "complex64", wrt=[])


def test_vjp_plan_rejects_overlapping_accumulates():
    from cotengra_amd import runtime

    case = next(c for c in TREE_CASES if c["name"] == "lattice4x4")
    tree = G.tree_of(case)
    plan = compile_vjp(tree, "complex128")
    runtime.DevicePlan(plan).close()   # (the plan as compiled is accepted)
    acc = [s for s in plan.steps if s.kind == KIND_ACCUM]
    acc[1].c.offset = acc[0].c.offset + 1   # the second gradient now overlaps the first
    with pytest.raises(ValueError, match="overlapping"):
        runtime.DevicePlan(plan)
