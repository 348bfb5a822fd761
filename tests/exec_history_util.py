"""The trees of tests/test_gpu_exec_history.py, what their plans must look like (checked without a device in
tests/test_exec_history_plans.py and again on the device), and the references the results are compared with."""
import numpy as np

import cotengra_amd as ca
from cotengra_amd.plan import KERNEL_MFMA, KIND_PAIR, KIND_STEM2, SPACE_INPUTS
from oracle import contract_ref as orc

import golden_util as G

STEM_OPTS = dict(fuse=True, fuse_min_elems=1 << 10)


def default_arithmetic(monkeypatch):
    """Nothing in the environment names an arithmetic, a batch size, a graph or groups (the variables the library
    reads for them: one list, with G.fuse_whatever_fits)."""
    for k in G.ARITH_ENV:
        monkeypatch.delenv(k, raising=False)


def leaves_below(plan, step):
    """The input tensors under plan step ``step``: what its operands read of the inputs space, and what its producers
    read."""
    s, out = plan.steps[step], set()
    for ref, prod in ((s.a, s.a_prod), (s.b, s.b_prod), (s.b2, s.b2_prod)):
        if ref is None:
            continue
        if ref.space == SPACE_INPUTS:
            out.add(plan.input_offsets.index(ref.offset))
        elif prod >= 0:
            out |= leaves_below(plan, prod)
    return out


# ---- A: an unsliced chain of two long tiled steps ---------------------------------------------------------------

CHAIN = (16384, 256, 256, 256)


def chain_plan_checks(plan):
    s0, s1 = plan.steps[0], plan.steps[1]
    assert plan.nslices == 1
    assert (s0.kind, s0.kernel, s1.kind, s1.kernel) == (KIND_PAIR, KERNEL_MFMA, KIND_PAIR, KERNEL_MFMA)
    assert s1.a_prod == 0 and not (s0.invariant or s0.group or s1.invariant or s1.group)


# ---- B: an unsliced stem under the default rule -------------------------------------------------------------------

STEM_B_FIRST_LEAVES = {0, 1, 2, 3}


def stem_b():
    return G.stem_network(*G.STEM_CASES[10], 1000)


def stem_b_plan_checks(plan):
    stems = [i for i, s in enumerate(plan.steps) if s.kind == KIND_STEM2]
    assert plan.nslices == 1 and len(stems) >= 2
    for prev, i in zip(stems, stems[1:]):
        assert plan.steps[i].a_prod == prev
    assert not any(plan.steps[i].invariant or plan.steps[i].group for i in stems)
    # (the state and gates 0-2 lie under the first, recording stem launch: what case B scales)
    assert leaves_below(plan, stems[0]) == STEM_B_FIRST_LEAVES
    return stems


# ---- C: a sliced tree whose first long tiled step does not depend on the slice ------------------------------------

def sliced_chain():
    tree = ca.ContractionTree.from_path([("a", "b"), ("b", "c"), ("s", "c", "d")], ("a", "d"),
                                        dict(a=16384, b=256, c=256, d=256, s=4), path=[(0, 1), (0, 1)])
    tree.remove_ind_("s")
    return tree


def sliced_chain_plan_checks(plan):
    s0, s1 = plan.steps[0], plan.steps[1]
    assert plan.nslices == 4
    assert (s0.kind, s0.kernel, s1.kind, s1.kernel) == (KIND_PAIR, KERNEL_MFMA, KIND_PAIR, KERNEL_MFMA)
    assert s0.invariant and not s0.group
    assert s1.a_prod == 0 and not s1.invariant and not s1.group


# ---- D: a sliced stem -- slice-invariant stem step -> step a slice group shares -> per-slice step -----------------

STEM_D_GATES = [(3, 3), (5, 5), (5, 5), (5, 7), (5, 5), (5, 7), (5, 5)]
STEM_D_KEY, STEM_D_GROUP = ("g3_5", "g3_6"), ("g5_5", "g5_6")


STEM_D_INVARIANT_LEAVES = {0, 1, 2, 3}


def stem_d(seed):
    """Gate 3 carries the two sliced indices that select the slice GROUP (the key), gate 5 the two in which the
    slices of a group differ.  (Call with the pairing model and the group thresholds patched: G.fuse_whatever_fits,
    G.groups_everywhere.)"""
    tree = G.stem_network(17, STEM_D_GATES, seed)
    for ix in STEM_D_KEY + STEM_D_GROUP:
        tree.remove_ind_(ix)
    return tree


def stem_d_plan_checks(plan):
    assert plan.nslices == 16 and plan.group_size == 4 and set(plan.group_inds) == set(STEM_D_GROUP)
    s1, s2, s3 = plan.steps[1], plan.steps[2], plan.steps[3]
    assert s1.kind == s2.kind == s3.kind == KIND_STEM2
    assert s1.invariant and not s1.group
    assert s2.group and not s2.invariant and s2.a_prod == 1
    assert not s3.group and not s3.invariant and s3.a_prod == 2
    # (the state and gates 0-2 lie under the slice-invariant stem step: what D1 scales; gate 3, with the key indices,
    # under the shared one: what D2 scales block by block)
    assert leaves_below(plan, 1) == STEM_D_INVARIANT_LEAVES
    assert leaves_below(plan, 2) - leaves_below(plan, 1) == {4, 5}


def stem_d_key_blocks(tree, arrays, log2_of_key):
    """The gate-3 tensor with its block at key indices (v5, v6) scaled by 2^log2_of_key[(v5, v6)]: what the slices of a
    group share then differs by those powers from group to group, and the leaf's largest element stays where the
    largest block has it."""
    leaf = next(i for i, t in enumerate(tree.inputs) if all(ix in t for ix in STEM_D_KEY))
    ax = [tree.inputs[leaf].index(ix) for ix in STEM_D_KEY]
    x = arrays[leaf].copy()
    for (v5, v6), lg in log2_of_key.items():
        sel = [slice(None)] * x.ndim
        sel[ax[0]], sel[ax[1]] = v5, v6
        x[tuple(sel)] *= np.float32(2.0 ** lg)
    G.assert_in_upload_window(x)
    out = list(arrays)
    out[leaf] = x
    return out


# ---- references ----------------------------------------------------------------------------------------------------

def chunk_index(tree, i):
    """Where slice ``i`` lands in the gathered result: sliced output indices fixed at the slice's values."""
    key = orc.slice_key(tree, i)
    return tuple((0 if tree.sliced_inds[ix].project is not None else key[ix]) if ix in tree.sliced_inds else slice(None)
                 for ix in tree.output)


def slices_ref(tree, arrays, ids):
    """The slices ``ids`` gathered by the oracle in the arrays' own precision: every slice added at its place in a
    result of the gathered shape (what ``zero_result(); run_slice_list(ids); download_result()`` holds)."""
    out = np.zeros(tuple(tree.gathered_shape()), dtype=np.result_type(*[a.dtype for a in arrays]))
    for i in ids:
        out[chunk_index(tree, i)] += np.asarray(orc.contract_slice(tree, arrays, int(i)))
    return out


def slices_ref_stripped(tree, arrays, ids):
    """... under strip_exponent: ``(mantissa, exponent)`` with the largest exponent of the slices (core.py:125-172)."""
    pairs = [orc.contract_slice(tree, arrays, int(i), strip_exponent=True) for i in ids]
    emax = max(e for _, e in pairs)
    out = np.zeros(tuple(tree.gathered_shape()), dtype=np.result_type(*[a.dtype for a in arrays]))
    for i, (m, e) in zip(ids, pairs):
        out[chunk_index(tree, i)] += np.asarray(m) * 10.0 ** (e - emax)
    return out, emax


def wide(arrays):
    return [a.astype("complex128" if np.iscomplexobj(a) else "float64") for a in arrays]
