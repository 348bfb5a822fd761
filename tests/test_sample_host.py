"""CPU suite: the host side of sampling (cotengra_amd/circuits.py: sample_chaotic, chaotic_prefixes, linear_xeb;
the argument checks of HipContractor.sample) and the reference sampler of tests/sample_util.py."""
import numpy as np
import pytest

import cotengra_amd as ca
from cotengra_amd import circuits
from cotengra_amd.plan import compile_tree
from oracle import contract_ref as orc

import sample_util as su

QSIM = """4
0 hz_1_2 0
0 x_1_2 1
0 y_1_2 2
0 x_1_2 3
1 rz 0 0.3
1 fs 0 1 1.5157741664069029 0.5567125777723744
2 y_1_2 0
2 hz_1_2 1
2 x_1_2 2
3 rz 2 0.7
3 fs 1 2 1.2 -0.4
3 fs 0 3 0.9 0.2
4 x_1_2 0
4 y_1_2 3
"""


def test_linear_xeb_of_a_porter_thomas_vector():
    """p_k = the quantiles of N exp(-N p): draws from it score N sum p^2 - 1 = 1 - O(1/N); uniform ones 0."""
    nq = 12
    N = 2 ** nq
    p = -np.log(1.0 - (np.arange(N) + 0.5) / N) / N
    p /= p.sum()
    assert circuits.linear_xeb(nq, np.full(100, 1.0 / N)) == 0.0
    vals = np.array([3.0, 1.0, 2.0]) / N
    assert circuits.linear_xeb(nq, vals) == 2.0 ** nq * vals.mean() - 1.0
    expected = N * float(np.sum(p * p)) - 1.0
    assert abs(expected - 1.0) < 0.01
    c = np.cumsum(p)
    draws = su.reference_indices(c, np.random.default_rng(1).random(200000) * c[-1])
    assert abs(circuits.linear_xeb(nq, p[draws]) - expected) < 0.02
    with pytest.raises(ValueError):
        circuits.linear_xeb(nq, [])


def test_reference_sampler_and_condition():
    x = np.array([0.0, 1.0, 0.0, 2.0, 0.0])
    u = np.array([0.0, 0.19, 0.21, np.nextafter(1.0, 0.0)])
    p, c, t = su.reference(x, u)
    idx = su.reference_indices(c, t)
    assert list(idx) == [1, 1, 3, 3]
    su.check_draws(x, u, idx)
    with pytest.raises(AssertionError):
        su.check_draws(x, u, np.array([1, 1, 3, 4]))    # p = 0
    with pytest.raises(AssertionError):
        su.check_draws(x, u, np.array([1, 3, 3, 3]))    # outside its interval
    assert su.boundary_distance(c, t)[0] == 0.0


def test_prefixes_and_arrays_are_deterministic_and_independent_of_simplify():
    n, gates = circuits.parse_qsim(QSIM)
    a, _ = circuits.chaotic_prefixes(n, [1, 2], bunches=5, seed=9)
    b, rng = circuits.chaotic_prefixes(n, (2, 1), bunches=5, seed=9)
    assert a == b and len(a) == 5 and all(t[1] == t[2] == "?" and set(t[0] + t[3]) <= set("01") for t in a)
    assert len(set(a)) > 1
    _, rng2 = circuits.chaotic_prefixes(n, [1, 2], bunches=5, seed=9)
    assert np.array_equal(rng.random(7), rng2.random(7))
    assert circuits.chaotic_prefixes(n, [1, 2], bunches=5, seed=10)[0] != a
    batches = {}
    for simplify in (False, True):
        for template in a[:3]:
            net1 = circuits.circuit_to_network(n, gates, template, simplify=simplify)
            net2 = circuits.circuit_to_network(n, gates, template, simplify=simplify)
            assert net1[:3] == net2[:3]
            assert all(x.tobytes() == y.tobytes() for x, y in zip(net1[3], net2[3]))
            tree = ca.array_contract_tree(*net1[:3])
            batches[simplify, template] = np.asarray(orc.contract(tree, net1[3]))
    for template in a[:3]:
        assert np.allclose(batches[False, template], batches[True, template], atol=1e-13)


@pytest.mark.parametrize("simplify", [False, True])
def test_network_structure_does_not_depend_on_the_prefix(simplify):
    n, gates = circuits.parse_qsim(QSIM)
    nets = [circuits.circuit_to_network(n, gates, t, simplify=simplify, dtype="complex64")
            for t in ("0??1", "1??0", "0??0", "1??1")]
    plans = []
    for inputs, output, sd, arrays in nets:
        assert (inputs, output, sd) == nets[0][:3]
        assert [x.shape for x in arrays] == [x.shape for x in nets[0][3]]
        tree = ca.array_contract_tree(inputs, output, sd)
        plans.append(compile_tree(tree, "complex64").serialise())
    for s in plans[1:]:
        assert sorted(s) == sorted(plans[0])
        for key, val in s.items():
            assert np.array_equal(np.asarray(val), np.asarray(plans[0][key])), key
    assert any(x.tobytes() != y.tobytes() for x, y in zip(nets[0][3], nets[1][3]))


def test_argument_validation():
    n, gates = circuits.parse_qsim(QSIM)
    with pytest.raises(ValueError):
        circuits.sample_chaotic(n, gates, -1, [1, 2])
    for bad in ([4], [-1, 2], [1, 1], []):
        with pytest.raises(ValueError):
            circuits.sample_chaotic(n, gates, 8, bad)
    with pytest.raises(ValueError):
        circuits.sample_chaotic(n, gates, 8, [1, 2], bunches=0)
    tree = ca.ContractionTree(["a"], "a", {"a": 8})
    x = np.ones(8)
    with pytest.raises(ValueError):
        tree.contract_sample([x], -1)
    with pytest.raises(ValueError):
        tree.contract_sample([x], 2, uniforms=[0.5, 1.0])
    with pytest.raises(ValueError):
        tree.contract_sample([x], 2, uniforms=[0.5, float("nan")])
    with pytest.raises(ValueError):
        tree.contract_sample([x], 3, uniforms=[0.5, 0.25])
