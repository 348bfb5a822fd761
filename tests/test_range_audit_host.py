"""Host half of the range audit: what ``rangeaudit.summarise`` reads from a row, how operands
are joined to rows, the ``"auto"`` option's argument check and what the header declares.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from cotengra_amd import plan as P
from cotengra_amd import rangeaudit as RA
from cotengra_amd import runtime

import range_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _summary(x):
    row, sumsq = U.reference_row(np.asarray(x, dtype=np.float32))
    return RA.summarise(row, sumsq)


def test_one_hot_tensor():
    x = np.zeros(1024, dtype=np.float32)
    x[17] = 3.0                               # bin 128: [2, 4)
    s = _summary(x)
    assert (s.n, s.zeros, s.nonfinite, s.top) == (1024, 1023, 0, 128)
    assert s.rms == math.sqrt(9.0 / 1024)
    assert s.crest_up == 4.0 / s.rms          # the upper edge of the top binade over the rms
    true_crest = 3.0 / s.rms
    assert true_crest <= s.crest_up < 2 * true_crest
    assert s.eps_h2 == 2.0 ** -24 * s.crest_up
    assert s.below(0) == 0.0 and s.below(14) == 0.0   # its one non-zero component IS the top


def test_all_in_one_bin():
    x = np.full(4096, 1.5, dtype=np.float32)
    x[::2] = -1.25
    s = _summary(x)
    assert (s.n, s.zeros, s.nonfinite, s.top) == (4096, 0, 0, 127)
    assert 1.0 < s.crest_up < 2.0
    assert s.below(0) == 0.0
    assert s.eps_h2 < 2.0 ** -23


def test_one_component_far_above_the_rest():
    x = np.ones(1 << 12, dtype=np.float32)
    x[5] = 2.0 ** 20
    s = _summary(x)
    assert s.top == 127 + 20
    assert s.below(19) == (x.size - 1) / x.size and s.below(20) == 0.0
    rms = math.sqrt((2.0 ** 40 + x.size - 1) / x.size)
    assert s.rms == rms and s.crest_up == 2.0 ** 21 / rms
    assert s.crest_up > 64.0   # one scale for this tensor costs six bits of every other component


def test_all_zeros_is_inf_not_an_exception():
    s = _summary(np.zeros(100, dtype=np.float32))
    assert (s.n, s.zeros, s.nonfinite) == (100, 100, 0)
    assert s.rms == 0.0 and s.crest_up == float("inf") and s.eps_h2 == float("inf")
    assert s.below(14) == 0.0


def test_tensor_with_inf():
    x = np.array([1.0, -2.0, np.inf, np.nan, 0.0, -0.0], dtype=np.float32)
    s = _summary(x)
    assert (s.n, s.zeros, s.nonfinite, s.top) == (6, 2, 2, 128)
    assert s.sumsq == 5.0 and math.isfinite(s.crest_up)


def test_row_that_was_not_materialised():
    assert RA.summarise(np.zeros(RA.RANGE_WORDS, dtype=np.int64), 0.0) is None
    with pytest.raises(ValueError):
        RA.summarise(np.zeros(10, dtype=np.int64), 0.0)


def test_worst_of_two_slices():
    a = _summary(np.array([1.0, 1.0, 1.0, 1.0], dtype=np.float32))
    b = _summary(np.array([16.0, 2.0 ** -20, 0.0, 1.0], dtype=np.float32))
    w = RA.RangeSummary.worst([a, None, b])
    assert w.crest_up == max(a.crest_up, b.crest_up) and w.zeros == 1 and w.top == b.top
    assert w.below(14) == max(a.below(14), b.below(14)) == 1.0 / 3.0


def _ref(space, offset, leaf=-1, size=8):
    return P.TensorRef(space, offset, leaf, ("i",), (1,), size)


class _Plan:
    input_sizes = [8, 8, 8]


def test_operand_join_on_a_three_step_plan():
    """leaf 2 is preprocessed into the arena (step 0); step 1 is a pair of leaf 0 and that; step 2 a fused pair of
    step 1's result with leaves 1 and 2's preprocessed copy; then the accumulate step."""
    pre = P.Step(kind=P.KIND_SINGLE, a=_ref(P.SPACE_INPUTS, 16, 2), c=_ref(P.SPACE_ARENA, 64))
    pair = P.Step(kind=P.KIND_PAIR, a=_ref(P.SPACE_INPUTS, 0, 0), b=_ref(P.SPACE_ARENA, 64), c=_ref(P.SPACE_ARENA, 128))
    fused = P.Step(kind=P.KIND_STEM2, a=_ref(P.SPACE_ARENA, 128), b=_ref(P.SPACE_INPUTS, 8, 1), b2=_ref(P.SPACE_ARENA, 64),
                   c=_ref(P.SPACE_ARENA, 0), a_prod=1)
    acc = P.Step(kind=P.KIND_ACCUM, a=_ref(P.SPACE_ARENA, 0), c=_ref(P.SPACE_RESULT, 0))
    plan = _Plan()
    plan.steps = [pre, pair, fused, acc]
    j = RA.join_operands(plan)
    assert j[0] == {"a": 2, "b": None, "b2": None, "c": 3}
    assert j[1] == {"a": 0, "b": 3, "b2": None, "c": 4}
    assert j[2] == {"a": 4, "b": 1, "b2": 3, "c": 5}
    assert j[3]["a"] == 5 and j[3]["c"] == 6

    # records: every leaf and result all ones of 8 components, but step 1's result (row 4): one large component
    rows = np.zeros((7, RA.RANGE_WORDS), dtype=np.int64)
    sumsq = np.zeros(7)
    for t in range(6):
        x = np.ones(8, dtype=np.float32)
        if t == 4:
            x[0] = 2.0 ** 12
        rows[t], sumsq[t] = U.reference_row(x)
    names = ["single_kernel", "pair_valu_kernel", "stem2h_kernel<5,5,5,5,true,1,false>", "accum_kernel"]
    recs = RA.step_records(plan, names, [(rows, sumsq)])
    assert [r["scaled"] for r in recs] == [(), (), ("a", "b", "b2"), ()]
    assert recs[2]["a"].top == 139 and recs[2]["b"].top == 127 and recs[2]["c"].top == 127
    assert recs[3]["c"] is None and recs[3]["kappa"] is None
    assert recs[1]["kappa"] == math.sqrt(8.0) * math.sqrt(8.0) / math.sqrt(2.0 ** 24 + 7)
    big = recs[2]["a"].crest_up
    assert RA.auto_choice(names, recs, 2 * big) == "fp16x2"
    assert RA.auto_choice(names, recs, big / 2) == "bf16x3"
    assert RA.auto_choice(["single_kernel", "pair_valu_kernel", "stem2_kernel<5,5,5,5,true>", "accum_kernel"], recs, 1.0) == "fp16x2"
    assert RA.scaled_operands("pair_mfma_h2_kernel<128,64,16>,VEC") == ("a", "b")


def test_auto_needs_a_crest_limit():
    import cotengra_amd as ca
    from cotengra_amd.contractor import HipContractor

    tree = ca.ContractionTree.from_path([("a", "b"), ("b", "c")], ("a", "c"), dict(a=4, b=4, c=4), path=[(0, 1)])
    with pytest.raises(ValueError):
        HipContractor(tree, stem_bf16x3="auto")
    with pytest.raises(ValueError):
        HipContractor(tree, stem_bf16x3="fp16x2", crest_limit=8.0)
    fn = HipContractor(tree, stem_bf16x3="auto", crest_limit=64)
    assert fn.auto_arith and fn.crest_limit == 64.0 and fn.last_audit is None and fn.arithmetic_chosen is None
    assert hasattr(ca.ContractionTree, "contract_audit") and hasattr(runtime.Executor, "range_audit")


def test_header_declares_the_audit_and_abi_10():
    text = open(os.path.join(ROOT, "include", "ctg_hip.h")).read()
    assert re.search(r"#define\s+CTG_ABI_VERSION\s+10\b", text)
    assert re.search(r"#define\s+CTG_RANGE_WORDS\s+260\b", text)
    assert re.search(r"int\s+ctg_exec_range_audit\s*\(\s*ctg_exec\s*\*\s*\w*\s*,\s*int64_t\s+slice_id\s*,\s*int64_t\s*\*\s*rows\s*,"
                     r"\s*double\s*\*\s*sumsq\s*\)", text)
    assert runtime.ABI_VERSION == 10 and "ctg_exec_range_audit" in runtime.SYMBOLS
    assert runtime.Executor.RANGE_WORDS == RA.RANGE_WORDS == U.RANGE_WORDS == 260
