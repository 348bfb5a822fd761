"""The plans that tests/test_gpu_exec_history.py relies on, checked without a device: which step of each case is
slice-invariant, which one a slice group shares, which one runs per slice, and who produces whose big operand."""
import pytest

from cotengra_amd.plan import compile_tree

import exec_history_util as H
import golden_util as G


def test_unsliced_chain_plan():
    H.chain_plan_checks(compile_tree(G.chain_tree(*H.CHAIN), "complex64"))


def test_unsliced_stem_plan(monkeypatch):
    G.fuse_whatever_fits(monkeypatch, h2_all=False)
    stems = H.stem_b_plan_checks(compile_tree(H.stem_b(), "complex64", **H.STEM_OPTS))
    assert len(stems) == 3


def test_sliced_chain_plan():
    H.sliced_chain_plan_checks(compile_tree(H.sliced_chain(), "complex64"))


@pytest.mark.parametrize("seed", range(9))
def test_sliced_stem_plan(seed, monkeypatch):
    G.fuse_whatever_fits(monkeypatch, h2_all=False)
    G.groups_everywhere(monkeypatch)
    tree = H.stem_d(seed)
    H.stem_d_plan_checks(compile_tree(tree, "complex64", **H.STEM_OPTS))
    if seed in (6, 8):   # (the key indices stay open in the output: every group writes its own chunk of the result)
        assert all(ix in tree.output for ix in H.STEM_D_KEY)


def test_window_helper_refuses_a_scale_the_upload_would_take_out():
    import numpy as np

    x = np.ones(4, dtype="complex64")
    assert G.scaled_in_window(x, -31).real.max() == np.float32(2.0 ** -31)
    with pytest.raises(AssertionError):
        G.scaled_in_window(x, -40)
    with pytest.raises(AssertionError):
        G.scaled_in_window(x, 32)
