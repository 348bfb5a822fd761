"""qsim circuit -> amplitude tensor network (the data format on the caller's
side of the contraction path).

The reference ships Sycamore circuits only as qsim gate lists
(``examples/circuit_n53_m*_s0_e0_pABCDCDAB.qsim``) and relies on quimb (absent
here) to turn them into networks.  This module does that step: parse the gate
list, build the network of ``<b| U_T ... U_1 |0>``, and absorb every rank-1 and
rank-2 tensor into a neighbour -- the simplification that leaves the Sycamore
networks with only rank-3/4 tensors (the reference's own m20 benchmark JSON has
365 rank-4 + 16 rank-3 tensors).

Gate set of the Sycamore supremacy circuits (qsim names):
``x_1_2`` = sqrt(X), ``y_1_2`` = sqrt(Y), ``hz_1_2`` = sqrt(W) with
W = (X+Y)/sqrt(2), ``rz(theta)``, ``fs(theta, phi)`` (fSim).
"""

from __future__ import annotations

import numpy as np

from .utils import get_symbol


def parse_qsim(text):
    """Return ``(n_qubits, [(name, qubits, params), ...])`` in file order."""
    lines = [ln.split() for ln in text.strip().splitlines() if ln.strip()]
    n = int(lines[0][0])
    gates = []
    for tok in lines[1:]:
        name = tok[1]
        nq = 2 if name in ("fs", "cz", "is") else 1
        qubits = tuple(int(q) for q in tok[2 : 2 + nq])
        params = tuple(float(x) for x in tok[2 + nq :])
        gates.append((name, qubits, params))
    return n, gates


def gate_matrix(name, params=()):
    """Unitary of a gate, 2x2 or 4x4 (row = output basis state)."""
    s = 1.0 / np.sqrt(2.0)
    if name == "x_1_2":
        return s * np.array([[1, -1j], [-1j, 1]])
    if name == "y_1_2":
        return s * np.array([[1, -1], [1, 1]], dtype=complex)
    if name == "hz_1_2":
        return s * np.array([[1, -np.exp(0.25j * np.pi)], [np.exp(-0.25j * np.pi), 1]])
    if name == "rz":
        (theta,) = params
        return np.diag([np.exp(-0.5j * theta), np.exp(0.5j * theta)])
    if name == "fs":
        theta, phi = params
        c, sn = np.cos(theta), np.sin(theta)
        return np.array(
            [[1, 0, 0, 0], [0, c, -1j * sn, 0], [0, -1j * sn, c, 0], [0, 0, 0, np.exp(-1j * phi)]]
        )
    if name == "cz":
        return np.diag([1, 1, 1, -1]).astype(complex)
    raise ValueError(f"unknown gate {name!r}")


def circuit_to_network(n, gates, bitstring=None, simplify=True, dtype="complex128"):
    """Amplitude network ``<bitstring| circuit |0...0>``.

    ``bitstring`` holds one character per qubit: ``'0'`` / ``'1'`` project the
    qubit, any other character (e.g. ``'?'``) leaves it *open* -- the network
    then has one output index per open qubit (in qubit order) and contracts to
    the batch of ``2**n_open`` amplitudes, which gives the pairwise steps a real
    N dimension.

    Returns ``(inputs, output, size_dict, arrays)`` with single-character index
    labels (``utils.get_symbol``), all of size 2.
    """
    if bitstring is None:
        bitstring = "0" * n
    counter = [0]

    def new_ix():
        ix = get_symbol(counter[0])
        counter[0] += 1
        return ix

    tensors = []  # [inds(list), array]
    cur = []
    zero, one = np.array([1.0, 0.0], dtype=complex), np.array([0.0, 1.0], dtype=complex)
    for q in range(n):
        ix = new_ix()
        cur.append(ix)
        tensors.append([[ix], zero.copy()])
    for name, qubits, params in gates:
        U = gate_matrix(name, params)
        if len(qubits) == 1:
            (q,) = qubits
            out = new_ix()
            tensors.append([[out, cur[q]], U.astype(complex)])
            cur[q] = out
        else:
            q0, q1 = qubits
            o0, o1 = new_ix(), new_ix()
            tensors.append([[o0, o1, cur[q0], cur[q1]], U.reshape(2, 2, 2, 2).astype(complex)])
            cur[q0], cur[q1] = o0, o1
    open_inds = []
    for q in range(n):
        if bitstring[q] in "01":
            tensors.append([[cur[q]], (one if bitstring[q] == "1" else zero).copy()])
        else:
            open_inds.append(cur[q])

    if simplify:
        tensors = absorb_low_rank(tensors, keep=set(open_inds))

    # relabel compactly in order of appearance
    relabel = {}
    inputs, arrays = [], []
    for inds, arr in tensors:
        term = []
        for ix in inds:
            if ix not in relabel:
                relabel[ix] = get_symbol(len(relabel))
            term.append(relabel[ix])
        inputs.append(tuple(term))
        arrays.append(np.ascontiguousarray(arr.astype(dtype)))
    size_dict = {ix: 2 for ix in relabel.values()}
    return inputs, tuple(relabel[ix] for ix in open_inds), size_dict, arrays


def absorb_low_rank(tensors, keep=()):
    """Contract every tensor of rank <= 2 into a neighbour (never raising the
    neighbour's rank), until none is left.  Indices in ``keep`` (open outputs)
    are never summed."""
    keep = set(keep)
    tensors = [[list(i), a] for i, a in tensors]
    where = {}
    for t, (inds, _) in enumerate(tensors):
        for ix in inds:
            where.setdefault(ix, set()).add(t)
    alive = set(range(len(tensors)))
    changed = True
    while changed:
        changed = False
        for t in sorted(alive):
            if t not in alive:
                continue
            inds, arr = tensors[t]
            if len(inds) > 2 or len(alive) == 1:
                continue
            # neighbour sharing an index, highest rank first
            nbrs = {u for ix in inds if ix not in keep for u in where[ix] if u != t and u in alive}
            if not nbrs:
                continue
            u = max(nbrs, key=lambda v: (len(tensors[v][0]), -v))
            uinds, uarr = tensors[u]
            shared = [ix for ix in inds if ix in uinds and ix not in keep]
            keep_t = [ix for ix in inds if ix not in shared]
            if len(keep_t) > 1:
                continue   # (open index + dangling index: leave the tensor alone)
            # result keeps u's index order with shared slots replaced by t's free index
            letters = {ix: chr(ord("a") + k) for k, ix in enumerate(dict.fromkeys(uinds + inds))}
            out = []
            replaced = False
            for ix in uinds:
                if ix in shared:
                    if keep_t and not replaced:
                        out.append(keep_t[0])
                        replaced = True
                else:
                    out.append(ix)
            if keep_t and not replaced:
                out.append(keep_t[0])
            eq = (
                "".join(letters[i] for i in uinds) + "," + "".join(letters[i] for i in inds)
                + "->" + "".join(letters[i] for i in out)
            )
            new = np.einsum(eq, uarr, arr)
            for ix in inds:
                where[ix].discard(t)
            for ix in shared:
                where[ix].discard(u)
            for ix in out:
                where.setdefault(ix, set()).add(u)
            tensors[u] = [out, new]
            alive.discard(t)
            changed = True
    return [tensors[t] for t in sorted(alive)]


# ---------------------------------------------------------------------------------------------------- #
# sampling: fix most qubits at random, leave a few open, draw from the conditional distribution
# ---------------------------------------------------------------------------------------------------- #
#
# What quimb offers as ``Circuit.sample_chaotic`` on top of the reference: for a chaotic circuit the
# marginal of a random assignment of the fixed qubits is as good as a draw from it, so a bunch of
# samples costs ONE contraction with the ``marginal_qubits`` open -- a batch of 2^k amplitudes that
# stays on the device, where ``HipContractor.sample`` draws from it.


def _check_marginal(n, marginal_qubits):
    qs = sorted(int(q) for q in marginal_qubits)
    if not qs:
        raise ValueError("marginal_qubits is empty: leave at least one qubit open.")
    if len(set(qs)) != len(qs):
        raise ValueError(f"marginal_qubits {list(marginal_qubits)} repeats a qubit.")
    if qs[0] < 0 or qs[-1] >= n:
        raise ValueError(f"marginal_qubits {list(marginal_qubits)} outside the {n} qubits.")
    return qs


def chaotic_prefixes(n, marginal_qubits, bunches=1, seed=None):
    """The bitstring templates of ``sample_chaotic``'s bunches (``'?'`` at the marginal qubits, a random bit
    at every other one) and the generator that drew them, which goes on to draw the uniforms -- a pure
    function of ``seed``."""
    qs = set(_check_marginal(n, marginal_qubits))
    bunches = int(bunches)
    if bunches < 1:
        raise ValueError(f"bunches = {bunches}: need at least one.")
    rng = np.random.default_rng(seed)
    templates = []
    for _ in range(bunches):
        bits = rng.integers(0, 2, size=n)
        templates.append("".join("?" if q in qs else str(int(bits[q])) for q in range(n)))
    return templates, rng


def sample_chaotic(n, gates, n_samples, marginal_qubits, bunches=1, seed=None, optimize="greedy",
                   dtype="complex64", target_size=None):
    """Bitstrings of the ``n``-qubit circuit ``gates`` by the fix-and-marginalise scheme: ``bunches`` times,
    fix every qubit outside ``marginal_qubits`` to a random bit, contract the batch of ``2^k`` amplitudes of
    the open ones on the device and draw ``n_samples // bunches`` of its members from ``|amplitude|^2``
    there (``HipContractor.sample``) -- only indices, the drawn amplitudes and the norm come back.

    The network is built and its tree found once (``optimize``: as for ``array_contract_tree``, e.g. a
    ``ContractionTree`` over the network of any template; ``target_size`` slices the tree found); a bunch
    only rebuilds and uploads the arrays, the structure of the network not depending on the bit values.

    Returns a dict: ``bitstrings`` (one ``'0'/'1'`` string of ``n`` characters per draw, bunch after
    bunch), ``amplitudes`` (of those bitstrings), ``p`` (their ``|amplitude|^2``), ``bunch`` (which bunch
    each draw belongs to), and per bunch ``prefixes`` (its template, ``'?'`` at the marginal qubits),
    ``norms`` (``sum |amplitude|^2`` of its batch: the marginal probability of its fixed bits) and
    ``sum_p2``."""
    from .interface import array_contract_tree

    n_samples = int(n_samples)
    if n_samples < 0:
        raise ValueError(f"n_samples = {n_samples} is negative.")
    qs = _check_marginal(n, marginal_qubits)
    templates, rng = chaotic_prefixes(n, qs, bunches, seed)
    per = n_samples // len(templates)
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, templates[0], simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    out = {"bitstrings": [], "amplitudes": [], "p": [], "bunch": [], "prefixes": templates, "norms": [], "sum_p2": []}
    for b, template in enumerate(templates):
        if b:
            inputs_b, output_b, _, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
            assert inputs_b == inputs and output_b == output, "the network's structure depends on the bit values"
        res = tree.contract_sample(arrays, per, uniforms=rng.random(per))
        for coords in res.coords:
            bits = list(template)
            for q, c in zip(qs, coords):
                bits[q] = str(int(c))
            out["bitstrings"].append("".join(bits))
        out["amplitudes"].append(res.amplitudes)
        out["p"].append(res.p)
        out["bunch"].append(np.full(per, b, dtype=np.int64))
        out["norms"].append(res.norm)
        out["sum_p2"].append(res.sum_p2)
    for key in ("amplitudes", "p", "bunch"):
        out[key] = np.concatenate(out[key])
    out["norms"] = np.asarray(out["norms"])
    out["sum_p2"] = np.asarray(out["sum_p2"])
    return out


def top_chaotic(n, gates, marginal_qubits, bunches=1, top=1, seed=None, optimize="greedy", dtype="complex64",
                target_size=None):
    """The post-selection companion of :func:`sample_chaotic`: the same bunches (``chaotic_prefixes``: every qubit
    outside ``marginal_qubits`` fixed to a random bit), the same single tree and executor, but of every bunch's
    batch of ``2^k`` amplitudes the ``top`` heaviest members, selected on the device (``HipContractor.topk``) --
    ``|amplitude|^2`` descending, the lower bitstring first among equals.

    Returns a dict: ``bitstrings`` (``top`` per bunch, bunch after bunch, heaviest first), ``amplitudes``, ``p``
    (their ``|amplitude|^2``), ``bunch``, and per bunch ``prefixes``, ``norms`` (``sum |amplitude|^2`` of its
    batch) and ``sum_p2``."""
    from .interface import array_contract_tree

    top = int(top)
    qs = _check_marginal(n, marginal_qubits)
    if top < 1 or top > 2 ** len(qs):
        raise ValueError(f"top = {top}: a bunch has {2 ** len(qs)} members.")
    templates, _ = chaotic_prefixes(n, qs, bunches, seed)
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, templates[0], simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    out = {"bitstrings": [], "amplitudes": [], "p": [], "bunch": [], "prefixes": templates, "norms": [], "sum_p2": []}
    for b, template in enumerate(templates):
        if b:
            inputs_b, output_b, _, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
            assert inputs_b == inputs and output_b == output, "the network's structure depends on the bit values"
        res = tree.contract_topk(arrays, top)
        for coords in res.coords:
            bits = list(template)
            for q, c in zip(qs, coords):
                bits[q] = str(int(c))
            out["bitstrings"].append("".join(bits))
        out["amplitudes"].append(res.amplitudes)
        out["p"].append(res.p)
        out["bunch"].append(np.full(top, b, dtype=np.int64))
        out["norms"].append(res.norm)
        out["sum_p2"].append(res.sum_p2)
    for key in ("amplitudes", "p", "bunch"):
        out[key] = np.concatenate(out[key])
    out["norms"] = np.asarray(out["norms"])
    out["sum_p2"] = np.asarray(out["sum_p2"])
    return out


def amplitudes_of(n, gates, bitstrings, optimize="greedy", dtype="complex64", target_size=None, chain=False):
    """Ideal amplitudes of given bitstrings -- measured or spoofed ones to be scored -- of the ``n``-qubit circuit
    ``gates``: the qubits on which all ``bitstrings`` agree are projected, the others left open, and of that one
    network's batch of ``2^k`` amplitudes only the requested members are contracted
    (``ContractionTree.contract_pick``: a sparse root step, the batch itself never exists).  One network, one
    tree (``optimize``: as for ``array_contract_tree``; ``target_size`` slices inner indices of the tree found),
    one call.

    ``chain`` (``True``, or an ``int``: at most that many levels below the root): the requests are carried
    down the tree -- a node below the root whose output legs the table addresses at few distinct projections
    (``plan.pick_chain_nodes``: ``PICK_CHAIN_GAIN * M_c <= O_c``, its parent sparse too) is stored as ``M_c`` rows
    of its other legs and computed by one row-sparse step, so cost and memory follow the
    table, not ``2^k``.  Which nodes are sparse depends on the table through that rule: a request's bits are
    therefore independent of the table's order and of duplicates, but not of which other requests are present.

    Returns a dict: ``bitstrings`` (as given), ``amplitudes`` (one per bitstring, in that order), ``p`` (their
    ``|amplitude|^2``, float64) and ``open_qubits`` (the qubits left open, ascending).

    >>> out = amplitudes_of(n, gates, measured)
    >>> fidelity = linear_xeb(n, out["p"])
    """
    from .interface import array_contract_tree

    bitstrings = [str(b) for b in bitstrings]
    if not bitstrings:
        raise ValueError("amplitudes_of: no bitstrings.")
    for b in bitstrings:
        if len(b) != n or set(b) - {"0", "1"}:
            raise ValueError(f"amplitudes_of: {b!r} is not a string of {n} characters '0' / '1'.")
    bits = np.array([[int(c) for c in b] for b in bitstrings], dtype=np.int64)
    open_qubits = [q for q in range(n) if bits[:, q].min() != bits[:, q].max()]
    template = "".join("?" if q in open_qubits else bitstrings[0][q] for q in range(n))
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size, allow_outer=False)
    amps = np.asarray(tree.contract_pick(arrays, coords=bits[:, open_qubits], chain=chain))
    return {"bitstrings": bitstrings, "amplitudes": amps, "p": np.abs(amps).astype(np.float64) ** 2,
            "open_qubits": open_qubits}


def linear_xeb(n_qubits, probabilities):
    """Linear cross-entropy benchmark fidelity of sampled bitstrings with ideal probabilities
    ``probabilities``: ``2^n mean(p) - 1`` (1 for draws from a Porter-Thomas distribution, 0 for uniform
    ones)."""
    p = np.asarray(probabilities, dtype=np.float64)
    if p.size == 0:
        raise ValueError("linear_xeb of no samples.")
    return float(2.0 ** int(n_qubits) * p.mean() - 1.0)


# ---------------------------------------------------------------------------------------------------- #
# reduced density matrices of a (conditional) state: entanglement entropy, purity, correlators
# ---------------------------------------------------------------------------------------------------- #


def reduced_density_matrix(n, gates, qubits, fixed=None, optimize="greedy", dtype="complex64", target_size=None):
    """The reduced density matrix of ``qubits`` in the output state of the ``n``-qubit circuit ``gates``: every
    qubit not in ``fixed`` (a dict ``{qubit: 0 | 1}``: qubits projected onto that bit) stays open, so the result
    tensor is the -- conditional, for a non-empty ``fixed`` -- state, and the partial trace over the open qubits
    outside ``qubits`` is taken on the device (``ContractionTree.contract_rdm``); only the
    ``2^k x 2^k`` matrix comes back.  At most 6 qubits.

    Returns ``(rho, norm)``: ``rho`` of trace 1, rows and columns row-major over ``qubits`` in the order given, and
    ``norm`` = ``sum |amplitude|^2`` of the open qubits (the probability of the fixed bits; 1 without any).
    ``ValueError`` for an empty, repeated or out-of-range qubit list (as for ``sample_chaotic``'s marginal qubits),
    a fixed qubit among ``qubits``, a fixed value other than 0 / 1, and a state of norm zero."""
    from .interface import array_contract_tree

    qs = [int(q) for q in qubits]
    _check_marginal(n, qs)
    fixed = {int(q): int(b) for q, b in (fixed or {}).items()}
    for q, b in fixed.items():
        if q < 0 or q >= n:
            raise ValueError(f"fixed: qubit {q} outside the {n} qubits.")
        if b not in (0, 1):
            raise ValueError(f"fixed: qubit {q} is projected onto {b}; 0 or 1 is expected.")
        if q in qs:
            raise ValueError(f"qubit {q} is both fixed and kept.")
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    open_qubits = [q for q in range(n) if q not in fixed]
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    res = tree.contract_rdm(arrays, [label[q] for q in qs])
    if not res.norm > 0:
        raise ValueError("reduced_density_matrix: the state has norm zero.")
    return res.rho / res.norm, res.norm


ENTANGLEMENT_MAX_QUBITS = 12   # the smaller side of a cut: D = 4096 rows (Executor.RDM_WIDE_MAX_DIM)


def entanglement_cut(n, qubits, fixed=None):
    """The side of the cut ``qubits | the other open qubits`` whose reduced density matrix ``entanglement_spectrum``
    computes -- host only: ``(side, open_qubits, fixed)``.  The two sides of a pure state share their non-zero
    spectrum, so the SMALLER one is taken (``qubits`` itself on a tie), in ascending order when it is the
    complement.  ``ValueError`` for what ``reduced_density_matrix`` refuses of ``qubits`` and ``fixed``, and for a
    smaller side above ``ENTANGLEMENT_MAX_QUBITS`` qubits."""
    n = int(n)
    qs = [int(q) for q in qubits]
    _check_marginal(n, qs)
    fixed = {int(q): int(b) for q, b in (fixed or {}).items()}
    for q, b in fixed.items():
        if q < 0 or q >= n:
            raise ValueError(f"fixed: qubit {q} outside the {n} qubits.")
        if b not in (0, 1):
            raise ValueError(f"fixed: qubit {q} is projected onto {b}; 0 or 1 is expected.")
        if q in qs:
            raise ValueError(f"qubit {q} is both fixed and kept.")
    open_qubits = [q for q in range(n) if q not in fixed]
    rest = [q for q in open_qubits if q not in qs]
    side = rest if len(rest) < len(qs) else qs
    if len(side) > ENTANGLEMENT_MAX_QUBITS:
        raise ValueError(f"the smaller side of the cut has {len(side)} qubits; at most {ENTANGLEMENT_MAX_QUBITS} "
                         f"(a matrix of {1 << ENTANGLEMENT_MAX_QUBITS} rows).")
    return side, open_qubits, fixed


def _cut_result(n, gates, qubits, fixed, optimize, dtype, target_size, matrix):
    """The (wide) reduced density matrix result of the smaller side of the cut, and the number of its rows."""
    from .interface import array_contract_tree
    from .runtime import Executor

    side, open_qubits, fixed = entanglement_cut(n, qubits, fixed)
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    keep = [label[q] for q in side]
    d = 1 << len(side)
    if d <= Executor.RDM_MAX_DIM:
        res = tree.contract_rdm(arrays, keep)
    else:
        res = tree.contract_rdm_wide(arrays, keep, matrix=matrix)
    if not res.norm > 0:
        raise ValueError("the state has norm zero.")
    return res, d


def _cut_spectrum(rho, d):
    """The eigenvalues of the Hermitian ``rho`` descending, scaled to sum 1: ``ValueError`` for one below
    ``-D 2^-52 max``, the rest clipped at 0."""
    w = np.linalg.eigvalsh(rho)[::-1]
    top = float(w[0])
    if float(w[-1]) < -d * 2.0 ** -52 * top:
        raise ValueError(f"the reduced density matrix has the eigenvalue {float(w[-1])!r} (largest: {top!r}): it is "
                         "not positive semidefinite within rounding.")
    w = np.clip(w, 0.0, None)
    return w / w.sum()


def entanglement_spectrum(n, gates, qubits, fixed=None, optimize="greedy", dtype="complex64", target_size=None):
    """The entanglement spectrum of the cut ``qubits | the other open qubits`` of the output state of the
    ``n``-qubit circuit ``gates`` (``fixed``: as for :func:`reduced_density_matrix`): the eigenvalues of the reduced
    density matrix of the smaller side (:func:`entanglement_cut`), which is formed on the device --
    ``ContractionTree.contract_rdm`` up to 6 qubits, ``contract_rdm_wide`` up to 12 -- and
    diagonalised on the host by ``numpy.linalg.eigvalsh``.

    Returns ``(eigenvalues, norm)``: the ``2^k`` eigenvalues descending, summing to 1, and ``norm`` = ``sum
    |amplitude|^2`` of the open qubits.  ``ValueError`` for what :func:`entanglement_cut` refuses, a state of norm
    zero and an eigenvalue below ``-D 2^-52 max``."""
    res, d = _cut_result(n, gates, qubits, fixed, optimize, dtype, target_size, True)
    return _cut_spectrum(res.rho, d), res.norm


def entanglement_entropy(n, gates, qubits, fixed=None, alpha=1, base=2, optimize="greedy", dtype="complex64",
                         target_size=None):
    """The entanglement entropy across the cut ``qubits | the other open qubits``: von Neumann, ``-sum l log l``, for
    ``alpha = 1``; Renyi, ``log(sum l^alpha) / (1 - alpha)``, otherwise; logarithms to ``base``.  ``alpha = 2``
    needs no eigenvalues: ``-log(purity / norm^2)`` with the purity ``sum |rho[a, b]|^2`` summed on the device -- above
    6 qubits on the smaller side the matrix is not downloaded at all (``contract_rdm_wide(matrix=False)``).

    Returns ``(entropy, norm)``.  ``ValueError`` for ``alpha <= 0``, ``base <= 1`` and what
    :func:`entanglement_spectrum` refuses."""
    alpha, base = float(alpha), float(base)
    if not alpha > 0:
        raise ValueError(f"alpha = {alpha}: a positive order is expected.")
    if not base > 1:
        raise ValueError(f"base = {base}: a base above 1 is expected.")
    res, d = _cut_result(n, gates, qubits, fixed, optimize, dtype, target_size, alpha != 2.0)
    if alpha == 2.0:
        purity = res.purity if hasattr(res, "purity") else float(np.sum(np.abs(res.rho) ** 2))
        return float(-np.log(purity / res.norm ** 2) / np.log(base)), res.norm
    w = _cut_spectrum(res.rho, d)
    if alpha == 1.0:
        nz = w[w > 0]
        return float(-np.sum(nz * np.log(nz)) / np.log(base)), res.norm
    return float(np.log(np.sum(w ** alpha)) / (1.0 - alpha) / np.log(base)), res.norm


def _circuit_pauli_requests(who, n, paulis, fixed, coeffs):
    """The validation ``pauli_expectation`` and ``energy_gradient`` share -- host only: ``(n, fixed, several?,
    [{qubit: letter}, ...] without identities, coeffs as float64 or None)``."""
    n = int(n)
    fixed = {int(q): int(b) for q, b in (fixed or {}).items()}
    for q, b in fixed.items():
        if q < 0 or q >= n:
            raise ValueError(f"fixed: qubit {q} outside the {n} qubits.")
        if b not in (0, 1):
            raise ValueError(f"fixed: qubit {q} is projected onto {b}; 0 or 1 is expected.")
    several = not isinstance(paulis, (str, dict))
    if several and not isinstance(paulis, (list, tuple)):
        raise ValueError(f"{who}: paulis = {paulis!r}; a string, a dict or a list of those is expected.")
    reqs = list(paulis) if several else [paulis]
    if len(reqs) > 4096:
        raise ValueError(f"{who}: {len(reqs)} requests; at most 4096 are taken by one call.")
    letters = []
    for req in reqs:
        if isinstance(req, str):
            if len(req) != n:
                raise ValueError(f"{who}: {req!r} is not a string of {n} letters.")
            named = dict(enumerate(req))
        elif isinstance(req, dict):
            named = {}
            for q, c in req.items():
                if isinstance(q, bool) or int(q) != q or not 0 <= int(q) < n:
                    raise ValueError(f"{who}: qubit {q!r} outside the {n} qubits.")
                named[int(q)] = c
        else:
            raise ValueError(f"{who}: the request {req!r} is neither a string nor a dict {{qubit: letter}}.")
        row = {}
        for q, c in named.items():
            if not isinstance(c, str) or c.upper() not in ("I", "X", "Y", "Z"):
                raise ValueError(f"{who}: {c!r} is none of the letters I, X, Y, Z.")
            if c.upper() != "I":
                if q in fixed:
                    raise ValueError(f"{who}: qubit {q} is fixed and carries {c!r}; a fixed qubit must be I.")
                row[q] = c.upper()
        letters.append(row)
    if coeffs is not None:
        coeffs = np.asarray(coeffs, dtype=np.float64).reshape(-1)
        if coeffs.size != len(reqs):
            raise ValueError(f"{who}: {coeffs.size} coefficients for {len(reqs)} requests.")
    return n, fixed, several, letters, coeffs


def pauli_expectation(n, gates, paulis, fixed=None, coeffs=None, optimize="greedy", dtype="complex64", target_size=None):
    """Expectation values of Pauli strings in the output state of the ``n``-qubit circuit ``gates``: energy terms of
    a Hamiltonian, QAOA / MaxCut cost functions, stabiliser checks, correlators.  ``paulis``: a list of requests (or
    one request), each a ``str`` of ``n`` letters over ``IXYZ`` (any case), qubit 0 first, or a dict ``{qubit:
    letter}`` (qubits not named are I).  Every qubit not in ``fixed`` (a dict ``{qubit: 0 | 1}``, as for
    :func:`reduced_density_matrix`) stays open, so the result tensor is the -- conditional, for a non-empty ``fixed``
    -- state, and every ``<psi| P |psi>`` is taken on the device (``ContractionTree.contract_expectation``, DESIGN.md
    section 16): strings that share their X / Y positions share one read of the state.  A fixed qubit must be I.

    Returns ``(values, norm)``: ``values`` = ``<psi| P |psi> / norm`` per request (a float64 array; a 0-d float for
    one request) and ``norm`` = ``sum |amplitude|^2`` of the open qubits (the probability of the fixed bits; 1 without
    any).  With ``coeffs`` (one real per request) also the scalar ``sum_k coeffs[k] values[k]`` as a third item.
    ``ValueError`` -- before any device work -- for a string of the wrong length, a letter outside ``IXYZ``, a qubit
    outside the circuit, a fixed value other than 0 / 1, a letter other than I on a fixed qubit, ``coeffs`` of
    another length than ``paulis`` and more than 4096 requests; and for a state of norm zero."""
    from .interface import array_contract_tree

    n, fixed, several, letters, coeffs = _circuit_pauli_requests("pauli_expectation", n, paulis, fixed, coeffs)
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    open_qubits = [q for q in range(n) if q not in fixed]
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    res = tree.contract_expectation(arrays, [{label[q]: c for q, c in row.items()} for row in letters])
    if not res.norm > 0:
        raise ValueError("pauli_expectation: the state has norm zero.")
    values = np.asarray(res.values, dtype=np.float64) / res.norm
    out = (values if several else np.float64(values[0]), res.norm)
    if coeffs is not None:
        out += (float(np.dot(coeffs, values)),)
    return out


def z_correlations(n, gates, qubits=None, fixed=None, optimize="greedy", dtype="complex64", target_size=None):
    """``<Z_i>``, ``<Z_i Z_j>`` and the connected correlations of the output state of the ``n``-qubit circuit
    ``gates`` over ``qubits`` (default: every qubit not in ``fixed``), normalised: the cost function of a QAOA / Ising
    problem with dense couplings, from ONE transform of the state on the device
    (``ContractionTree.contract_pauli_spectrum`` with the ``k + k (k - 1) / 2`` strings selected; DESIGN.md section
    21).  ``fixed``: a dict ``{qubit: 0 | 1}`` as for :func:`pauli_expectation`; a fixed qubit cannot be in ``qubits``.

    Returns ``(z, zz, connected, norm)``: ``z[a] = <Z_qa>``, ``zz[a, b] = <Z_qa Z_qb>`` (symmetric, ones on the
    diagonal), ``connected = zz - outer(z, z)``, all float64 and divided by ``norm`` = ``sum |amplitude|^2`` of the open
    qubits.  ``ValueError`` -- before any device work -- for a qubit outside the circuit, repeated or fixed and for a
    fixed value other than 0 / 1; and for a state of norm zero."""
    from .interface import array_contract_tree

    n, fixed, _, _, _ = _circuit_pauli_requests("z_correlations", n, [], fixed, None)
    open_qubits = [q for q in range(n) if q not in fixed]
    qs = open_qubits if qubits is None else [int(q) for q in qubits]
    for q in qs:
        if q < 0 or q >= n:
            raise ValueError(f"z_correlations: qubit {q} outside the {n} qubits.")
        if q in fixed:
            raise ValueError(f"z_correlations: qubit {q} is fixed.")
    if len(set(qs)) != len(qs):
        raise ValueError("z_correlations: a qubit is named twice.")
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    k = len(qs)
    pairs = [(a, b) for a in range(k) for b in range(a + 1, k)]
    reqs = [{label[qs[a]]: "Z"} for a in range(k)] + [{label[qs[a]]: "Z", label[qs[b]]: "Z"} for a, b in pairs]
    res = tree.contract_pauli_spectrum(arrays, flips=(), paulis=reqs)
    if not res.norm > 0:
        raise ValueError("z_correlations: the state has norm zero.")
    values = np.asarray(res.values, dtype=np.float64) / res.norm
    z = values[:k].copy()
    zz = np.eye(k, dtype=np.float64)
    for (a, b), v in zip(pairs, values[k:].tolist()):
        zz[a, b] = zz[b, a] = v
    return z, zz, zz - np.outer(z, z), res.norm


def maxcut_terms(edges, weights=None):
    """The Z-type terms of the MaxCut cost ``sum over edges (i, j) of w_ij (1 - Z_i Z_j) / 2`` -- the weight of the cut a
    bitstring makes -- as ``(terms, coeffs)`` for :func:`cost_statistics`: per edge the dict ``{i: "Z", j: "Z"}`` with
    coefficient ``-w_ij / 2``, and the constant ``sum w_ij / 2`` as the identity string ``{}`` in front.  ``weights``:
    one real per edge (default: ones).  ``ValueError`` for an edge that is no pair of two different non-negative
    qubits and for ``weights`` of another length or not finite."""
    pairs = []
    for e in edges:
        if len(e) != 2 or int(e[0]) == int(e[1]) or int(e[0]) < 0 or int(e[1]) < 0:
            raise ValueError(f"maxcut_terms: the edge {e!r} is no pair of two different qubits.")
        pairs.append((int(e[0]), int(e[1])))
    w = np.ones(len(pairs), dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != len(pairs):
        raise ValueError(f"maxcut_terms: {w.size} weights for {len(pairs)} edges.")
    if not np.all(np.isfinite(w)):
        raise ValueError("maxcut_terms: a weight is not finite.")
    terms = [{}] + [{i: "Z", j: "Z"} for i, j in pairs]
    return terms, np.concatenate([[0.5 * float(np.sum(w))], -0.5 * w])


def cost_statistics(n, gates, terms, coeffs=None, qubits=None, fixed=None, levels=(), tail="lower", edges=None, optimize="greedy",
                    dtype="complex64", target_size=None):
    """The distribution of the classical cost ``C = sum_k coeffs[k] Z-string_k`` in the output state of the ``n``-qubit
    circuit ``gates``: mean, variance, ``CVaR_alpha`` and quantiles at ``levels``, a histogram over ``edges``, the
    optimum over all bitstrings of the open qubits and the probability of sampling it -- the QAOA objectives, taken on
    the device from one contraction (``ContractionTree.contract_cost``).  ``terms``: requests as
    for :func:`pauli_expectation` with letters I and Z only (a dict ``{qubit: "Z"}``, ``{}`` for a constant; or a
    string of ``n`` letters); :func:`maxcut_terms` builds them for a graph.  ``qubits`` (default: every qubit not in
    ``fixed``): the qubits a term may name; ``fixed``: a dict ``{qubit: 0 | 1}`` as for :func:`pauli_expectation`.
    Returns the ``CostResult``; its ``argmin`` / ``argmax`` are bit tuples over the open qubits in qubit order.
    ``ValueError`` -- before any device work -- for what :func:`pauli_expectation` refuses of the requests, a letter X
    or Y, a term on a qubit outside ``qubits``; and for a state of norm zero."""
    from .interface import array_contract_tree

    n, fixed, several, letters, coeffs = _circuit_pauli_requests("cost_statistics", n, terms, fixed, coeffs)
    open_qubits = [q for q in range(n) if q not in fixed]
    qs = set(open_qubits if qubits is None else (int(q) for q in qubits))
    for q in qs:
        if q < 0 or q >= n or q in fixed:
            raise ValueError(f"cost_statistics: qubit {q} is outside the circuit or fixed.")
    for row in letters:
        for q, c in row.items():
            if c not in "IZ":
                raise ValueError(f"cost_statistics: the letter {c!r} on qubit {q}; a classical cost has I and Z only.")
            if c == "Z" and q not in qs:
                raise ValueError(f"cost_statistics: a term names qubit {q}, which is not among qubits = {sorted(qs)}.")
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    reqs = [{label[q]: c for q, c in row.items() if c == "Z"} for row in letters]
    res = tree.contract_cost(arrays, terms=reqs, coeffs=coeffs, levels=levels, tail=tail, edges=edges)
    if not res.norm > 0:
        raise ValueError("cost_statistics: the state has norm zero.")
    return res


def gate_derivatives(name, params=()):
    """``[dU / d params[0], ...]`` of :func:`gate_matrix`, analytic: one matrix for ``rz``, two for ``fs``, none for a
    gate without parameters."""
    if name == "rz":
        (theta,) = params
        return [np.diag([-0.5j * np.exp(-0.5j * theta), 0.5j * np.exp(0.5j * theta)])]
    if name == "fs":
        theta, phi = params
        c, sn = np.cos(theta), np.sin(theta)
        d_theta = np.array([[0, 0, 0, 0], [0, -sn, -1j * c, 0], [0, -1j * c, -sn, 0], [0, 0, 0, 0]], dtype=complex)
        d_phi = np.zeros((4, 4), dtype=complex)
        d_phi[3, 3] = -1j * np.exp(-1j * phi)
        return [d_theta, d_phi]
    gate_matrix(name, params)   # (ValueError for an unknown gate)
    return []


def energy_gradient(n, gates, paulis, coeffs, fixed=None, optimize="greedy", dtype="complex64", target_size=None,
                    normalize=True):
    """Energy ``sum_k coeffs[k] <psi| P_k |psi>`` of the output state of the ``n``-qubit circuit ``gates`` and its
    derivative by every gate parameter, in one step on the device: a VQE / QAOA iteration.  ``paulis``, ``fixed``:
    as for :func:`pauli_expectation`; ``coeffs``: one real per request.  The network is built unsimplified, so leaf
    ``n + k`` of the tree is gate ``k``; ``ContractionTree.contract_energy`` gives the energy
    and its gradient by every gate tensor, and the chain rule with the analytic ``dU / d theta``
    (:func:`gate_derivatives`) the derivative by every parameter.  ``normalize`` (default): the energy is divided by
    ``norm`` = ``sum |amplitude|^2`` of the open qubits and that quotient is differentiated.

    Returns ``(energy, norm, dparams)``: ``dparams[k]`` a float64 array with one entry per parameter of gate ``k``
    (one for ``rz``, two for ``fs``, empty otherwise).  ``ValueError`` -- before any device work -- for what
    :func:`pauli_expectation` refuses and for coefficients that are not finite; and for a state of norm zero under
    ``normalize``."""
    from .interface import array_contract_tree

    if coeffs is None:
        raise ValueError("energy_gradient: coeffs is None; one real coefficient per request is expected.")
    n, fixed, several, letters, coeffs = _circuit_pauli_requests("energy_gradient", n, paulis, fixed, coeffs)
    if not np.all(np.isfinite(coeffs)):
        raise ValueError("energy_gradient: a coefficient is not finite.")
    gates = list(gates)
    derivs = [gate_derivatives(name, params) for name, _, params in gates]
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    open_qubits = [q for q in range(n) if q not in fixed]
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=False, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    wrt = [n + k for k, d in enumerate(derivs) if d]
    res = tree.contract_energy(arrays, [{label[q]: c for q, c in row.items()} for row in letters], coeffs=coeffs,
                               wrt=wrt, normalize=normalize)
    dparams = []
    for k, ds in enumerate(derivs):
        g = None if not ds else np.asarray(res.grads[n + k], dtype=np.complex128).reshape(-1)
        # dE = Re sum conj(dE / d Re U + i dE / d Im U) dU
        dparams.append(np.array([float(np.real(np.vdot(g, d.reshape(-1)))) for d in ds], dtype=np.float64))
    return float(res.energy), res.norm, dparams


def _circuit_operator_requests(who, n, operators, fixed):
    """The validation ``operator_expectation`` and ``operator_energy_gradient`` share -- host only: ``(n, fixed,
    several?, [(qubits, complex128 (2^k, 2^k) matrix), ...])``."""
    n = int(n)
    fixed = {int(q): int(b) for q, b in (fixed or {}).items()}
    for q, b in fixed.items():
        if q < 0 or q >= n:
            raise ValueError(f"fixed: qubit {q} outside the {n} qubits.")
        if b not in (0, 1):
            raise ValueError(f"fixed: qubit {q} is projected onto {b}; 0 or 1 is expected.")

    def is_request(p):
        if not (isinstance(p, (tuple, list)) and len(p) == 2):
            return False
        try:
            arr = np.asarray(p[1])
        except ValueError:
            return False
        return arr.dtype.kind in "iufbc" and arr.ndim >= 2

    if is_request(operators):
        several, reqs = False, [operators]
    elif isinstance(operators, (list, tuple)):
        several, reqs = True, list(operators)
    else:
        raise ValueError(f"{who}: operators = {operators!r}; a (qubits, matrix) pair or a list of those is expected.")
    if len(reqs) > 4096:
        raise ValueError(f"{who}: {len(reqs)} requests; at most 4096 are taken by one call.")
    out = []
    for req in reqs:
        if not is_request(req):
            raise ValueError(f"{who}: the request {req!r} is no (qubits, matrix) pair with a numeric matrix.")
        qs = [req[0]] if not hasattr(req[0], "__iter__") else list(req[0])
        if not qs:
            raise ValueError(f"{who}: a request names no qubit.")
        for q in qs:
            if isinstance(q, bool) or int(q) != q or not 0 <= int(q) < n:
                raise ValueError(f"{who}: qubit {q!r} outside the {n} qubits.")
            if int(q) in fixed:
                raise ValueError(f"{who}: qubit {q} is fixed; an operator acts on open qubits only.")
        qs = [int(q) for q in qs]
        if len(set(qs)) != len(qs):
            raise ValueError(f"{who}: the qubits {qs} repeat.")
        if len(qs) > 6:
            raise ValueError(f"{who}: an operator on {len(qs)} qubits; at most 6.")
        mat = np.asarray(req[1], dtype=np.complex128)
        d = 1 << len(qs)
        if mat.shape != (d, d) and mat.shape != (2,) * (2 * len(qs)):
            raise ValueError(f"{who}: a matrix of shape {mat.shape} on the qubits {qs}; ({d}, {d}) is expected.")
        if not np.all(np.isfinite(mat)):
            raise ValueError(f"{who}: the matrix on the qubits {qs} has an entry that is not finite.")
        out.append((qs, mat.reshape(d, d)))
    return n, fixed, several, out


def operator_expectation(n, gates, operators, fixed=None, optimize="greedy", dtype="complex64", target_size=None):
    """Expectation values of dense few-qubit operators in the output state of the ``n``-qubit circuit ``gates``:
    projectors, number operators, hopping terms, any observable on up to 6 qubits -- without an expansion into Pauli
    strings.  ``operators``: a list of ``(qubits, matrix)`` pairs (or one pair); ``matrix`` is ``2^k x 2^k``, rows and
    columns row-major over ``qubits`` in the order given.  ``fixed``: as for :func:`pauli_expectation`; a fixed qubit
    may not be named.  The values come from reduced density matrices formed on the device
    (``ContractionTree.contract_operator_expectation``).

    Returns ``(values, norm)``: ``values`` = ``<psi| O |psi> / norm`` per request (a complex128 array; a 0-d complex
    for one request) and ``norm`` = ``sum |amplitude|^2`` of the open qubits.  ``ValueError`` -- before any device
    work -- for a qubit outside the circuit, repeated or fixed, more than 6 qubits, a matrix of the wrong shape or
    with an entry that is not finite, a fixed value other than 0 / 1 and more than 4096 requests; and for a state of
    norm zero."""
    from .interface import array_contract_tree

    n, fixed, several, reqs = _circuit_operator_requests("operator_expectation", n, operators, fixed)
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    open_qubits = [q for q in range(n) if q not in fixed]
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=True, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    res = tree.contract_operator_expectation(arrays, [([label[q] for q in qs], mat) for qs, mat in reqs])
    if not res.norm > 0:
        raise ValueError("operator_expectation: the state has norm zero.")
    values = np.asarray(res.values, dtype=np.complex128) / res.norm
    return (values if several else np.complex128(values[0]), res.norm)


def operator_energy_gradient(n, gates, operators, fixed=None, optimize="greedy", dtype="complex64", target_size=None,
                             normalize=True):
    """Energy ``sum_k <psi| O_k |psi>`` of Hermitian dense few-qubit operators in the output state of the ``n``-qubit
    circuit ``gates`` and its derivative by every gate parameter, in one step on the device: :func:`energy_gradient`
    for a Hamiltonian given as matrices.  ``operators``, ``fixed``: as for :func:`operator_expectation`.  Goes through
    ``ContractionTree.contract_operator_energy``; ``normalize`` as for
    :func:`energy_gradient`.

    Returns ``(energy, norm, dparams)`` exactly as :func:`energy_gradient` does.  ``ValueError`` -- before any device
    work -- for what :func:`operator_expectation` refuses and for a matrix that is not Hermitian; and for a state of
    norm zero under ``normalize``."""
    from .interface import array_contract_tree

    n, fixed, several, reqs = _circuit_operator_requests("operator_energy_gradient", n, operators, fixed)
    for qs, mat in reqs:
        if np.abs(mat - mat.conj().T).max() > 1e-12 * np.abs(mat).max():
            raise ValueError(f"operator_energy_gradient: the matrix on the qubits {qs} is not Hermitian.")
    gates = list(gates)
    derivs = [gate_derivatives(name, params) for name, _, params in gates]
    template = "".join(str(fixed[q]) if q in fixed else "?" for q in range(n))
    open_qubits = [q for q in range(n) if q not in fixed]
    inputs, output, size_dict, arrays = circuit_to_network(n, gates, template, simplify=False, dtype=dtype)
    tree = array_contract_tree(inputs, output, size_dict, optimize=optimize)
    if [tuple(t) for t in tree.inputs] != [tuple(t) for t in inputs] or tuple(tree.output) != tuple(output):
        raise ValueError("optimize: the tree is not over this circuit's network.")
    if target_size is not None:
        tree = tree.slice(target_size=target_size)
    label = dict(zip(open_qubits, output))   # (one output index per open qubit, in qubit order)
    wrt = [n + k for k, d in enumerate(derivs) if d]
    res = tree.contract_operator_energy(arrays, [([label[q] for q in qs], mat) for qs, mat in reqs], wrt=wrt,
                                        normalize=normalize)
    dparams = []
    for k, ds in enumerate(derivs):
        g = None if not ds else np.asarray(res.grads[n + k], dtype=np.complex128).reshape(-1)
        # dE = Re sum conj(dE / d Re U + i dE / d Im U) dU
        dparams.append(np.array([float(np.real(np.vdot(g, d.reshape(-1)))) for d in ds], dtype=np.float64))
    return float(res.energy), res.norm, dparams


def _spectrum(rho):
    """Eigenvalues of the trace-normalised Hermitian matrix ``rho``, those below 0 from rounding clipped."""
    rho = np.asarray(rho)
    if rho.ndim != 2 or rho.shape[0] != rho.shape[1]:
        raise ValueError(f"rho of shape {rho.shape}; a square matrix is expected.")
    tr = float(np.trace(rho).real)
    if not tr > 0:
        raise ValueError("rho has no positive trace.")
    return np.clip(np.linalg.eigvalsh(rho / tr), 0.0, None)


def purity(rho):
    """``trace(rho^2)`` of the trace-normalised ``rho``: 1 for a pure state, ``1 / D`` for the maximally mixed one."""
    w = _spectrum(rho)
    return float(np.sum(w * w))


def von_neumann_entropy(rho, base=2):
    """``-trace(rho log rho)`` of the trace-normalised ``rho`` in units of ``log(base)`` (bits by default)."""
    w = _spectrum(rho)
    w = w[w > 0]
    return float(-np.sum(w * np.log(w)) / np.log(base))
