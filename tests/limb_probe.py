"""Limb probes: data whose every limb is populated and whose results the 16-bit arithmetics still owe BIT FOR BIT.

The 16-bit arithmetics of the stem kernels (csrc/ctg_stem_impl.h: Bf16x3, Fp16x2) and of the tiled pair kernels
(csrc/ctg_pair_mfma.hip: pair_mfma_bf3_kernel, pair_mfma_h2_kernel) multiply fp32 values as sums of 16-bit limbs:

    bf16 x 3   l1 = rn_bf16(x), l2 = rn_bf16(x - l1), l3 = x - l1 - l2 (kept as its upper 16 bits);
               the products (0,0) (0,1) (0,2) (1,0) (1,1) (2,0) of (limb of a, limb of b)      -- bf3_ta / bf3_tb
    fp16 x 2   h1 = rn_fp16(x s), h2 = rn_fp16(x s - h1), s a power of two that brings the operand's largest
               |component| to [2^13, 2^14); the products (0,0) (0,1) (1,0)                      -- Fp16x2::t_step

accumulated in fp32 by the matrix cores.  This module emulates exactly that in numpy -- a MODEL of the arithmetic, not
the exact product -- on data built so that the model's value is owed by the device bit for bit:

*   a probe value is l1 + l2 (+ l3) with short limbs of independent sign (PROBE_LIMBS): the split returns the chosen
    limbs, every kept product is a multiple of a quantum q and their absolute sum stays below 2^24 q, so the sum and
    every partial sum in every order is an fp32 number;
*   a small operand has ONE non-zero per column, purely real or purely imaginary: every real component of an output is
    a single real product of two values, the zeros contribute exact zeros;
*   in a chain, one stage at a time multiplies probe values with probe values; the other small operands are unit
    one-per-column matrices (entries +-1, +-i) that pass a value through -- as the arithmetic passes it: bf16 x 3 gives
    the value back, fp16 x 2 gives it back rounded to two fp16 limbs.

Nothing here touches a device.  tests/test_limb_probe_host.py asserts the conditions above for every row the device
test (tests/test_gpu_limb_probes.py) runs."""
import numpy as np

# (limb of a, limb of b) of the products an arithmetic keeps, in the kernels' order: bf3_ta(t), bf3_tb(t) for
# t = 0..5, and t = 0, 1, 3 of them (Fp16x2::t_step)
KEPT = {
    "bf16x3": ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)),
    "fp16x2": ((0, 0), (0, 1), (1, 0)),
}
# ... and the products of existing limbs that it leaves out
DROPPED = {
    "bf16x3": ((1, 2), (2, 1), (2, 2)),
    "fp16x2": ((1, 1),),
}
LIMBS = {"bf16x3": 3, "fp16x2": 2}
ARITHS = ("bf16x3", "fp16x2")

# limb k of a probe value is +- one of the mantissas times 2^exponent.  1.0 is left out of the first two limbs: with
# a limb of the opposite sign below it the value drops into the lower binade and the rounded split returns other limbs.
PROBE_LIMBS = {
    "bf16x3": (((1.25, 1.5, 1.75), 0), ((1.25, 1.5, 1.75), -9), ((1.0, 1.5), -18)),
    "fp16x2": (((1.25, 1.5, 1.75), 0), ((1.25, 1.5, 1.75), -12)),
}
# the fp32 kernels are probed with the three-limb values: 24 significant bits, a product is one rounding
VALUES_OF = {"fp32": "bf16x3", "bf16x3": "bf16x3", "fp16x2": "fp16x2"}


# ---------------------------------------------------------------------------------------------------------------- #
# round to nearest even, the splits
# ---------------------------------------------------------------------------------------------------------------- #
def f32(x):
    x = np.asarray(x)
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64)), "not an fp32 number"
    return y


def rn_bf16(x):
    """fp32 -> the nearest bfloat16 (ties to even), as an fp32 number: v_cvt_pk_bf16_f32 on finite values."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def trunc_bf16(x):
    """The upper 16 bits of an fp32 number (how the third limb is kept)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def rn_fp16(x):
    """fp32 -> the nearest fp16 (ties to even), as an fp32 number."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def split_bf16x3(x):
    """Bf16x3::split / store_limbs (and put3x2 of the pair kernel): three fp32 arrays."""
    x = np.asarray(x, dtype=np.float32)
    l1 = rn_bf16(x)
    r1 = x - l1
    l2 = rn_bf16(r1)
    return [l1, l2, trunc_bf16(r1 - l2)]


def h2_exponent(top):
    """h2_exponent_of / Fp16x2::operand_exponent: the exponent to REMOVE, the largest |component| goes to [2^13, 2^14)."""
    top = float(top)
    if top == 0.0 or not np.isfinite(top):
        return 0
    return int(np.floor(np.log2(top))) - 13


def split_fp16x2(x, scale):
    """Fp16x2::split / store_limbs (put2x2 of the pair kernel): the two limbs of x * scale, in scaled units."""
    xs = np.asarray(x, dtype=np.float32) * np.float32(scale)
    h1 = rn_fp16(xs)
    return [h1, rn_fp16(xs - h1)]


def top_of(x):
    x = np.asarray(x)
    return float(max(np.abs(x.real).max(), np.abs(x.imag).max())) if x.size else 0.0


def limbs_of(x, arith, scale_shift=0):
    """``(limbs, scale)``: the limbs of a complex array of fp32 components as complex128 arrays, and the power of two
    they are scaled by (1 for bf16 x 3; fp16 x 2: from the array's largest |component|, ``scale_shift`` more powers
    for the tests that show the result does not depend on it)."""
    x = np.asarray(x)
    re, im = f32(x.real), f32(x.imag)
    if arith == "bf16x3":
        scale = 1.0
        lr, li = split_bf16x3(re), split_bf16x3(im)
    else:
        scale = 2.0 ** (scale_shift - h2_exponent(top_of(x)))
        lr, li = split_fp16x2(re, scale), split_fp16x2(im, scale)
    return [a.astype(np.float64) + 1j * b.astype(np.float64) for a, b in zip(lr, li)], scale


# ---------------------------------------------------------------------------------------------------------------- #
# probe values and one-per-column operands
# ---------------------------------------------------------------------------------------------------------------- #
def probe_values(rng, shape, values, with_limbs=False):
    """Real probe values of ``values`` ("bf16x3" | "fp16x2") as float64 (every one an fp32 number)."""
    limbs = []
    for mant, ex in PROBE_LIMBS[values]:
        m = rng.choice(np.asarray(mant), size=shape) * rng.choice(np.asarray([-1.0, 1.0]), size=shape)
        limbs.append(m * 2.0 ** ex)
    x = sum(limbs)
    return (x, limbs) if with_limbs else x


def probe_complex(rng, shape, values):
    return probe_values(rng, shape, values) + 1j * probe_values(rng, shape, values)


def one_per_column(rng, K, N, values=None):
    """A (K, N) operand with one non-zero per column, in a random row, purely real or purely imaginary: a probe value
    of ``values``, or a unit +-1 / +-i (``values`` None)."""
    rows = rng.integers(0, K, size=N)
    mag = probe_values(rng, (N,), values) if values else rng.choice(np.asarray([-1.0, 1.0]), size=N)
    val = np.where(rng.integers(0, 2, size=N) == 1, 1j, 1.0) * mag
    b = np.zeros((K, N), dtype=np.complex128)
    b[rows, np.arange(N)] = val
    return b


def column_entries(b):
    """``(rows, values)`` of a one-per-column (K, N) operand."""
    b = np.asarray(b)
    assert b.ndim == 2 and np.all(np.count_nonzero(b, axis=0) == 1), "one non-zero per column"
    rows = np.argmax(b != 0, axis=0)
    vals = b[rows, np.arange(b.shape[1])]
    assert np.all((vals.real == 0) != (vals.imag == 0)), "purely real or purely imaginary"
    return rows, vals


# ---------------------------------------------------------------------------------------------------------------- #
# one stage: a[R, K] b[K, N] with b one-per-column
# ---------------------------------------------------------------------------------------------------------------- #
def low_bit_exponent(x):
    """The exponent of the lowest set bit over the non-zero entries of a real array (None: all zero)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    x = x[x != 0]
    if not x.size:
        return None
    m, e = np.frexp(x)
    i = np.abs(m * 2.0 ** 53).astype(np.int64)
    return int((e - 53 + np.log2((i & -i).astype(np.float64)).astype(np.int64)).min())


class Stage:
    """What the model computed for one stage: ``out`` (complex128, shape (R, N)) and, for the exactness assertions of
    a 16-bit stage (``details``), in the units of the accumulators: ``q``, the exponent of a quantum every kept
    product is a multiple of (the lowest bit of limb i of a's components times the lowest bit of limb j of b's, the
    least over the kept (i, j)), and ``total``, a bound on the sum of |products| of any component: the largest sum of
    |limbs| of a component of a times the largest sum of |limbs| of an entry of b."""

    def __init__(self, out, q=None, total=None):
        self.out, self.q, self.total = out, q, total


def stage(a, b, arith, kept=None, scale_shift=0, details=False):
    """The model of ``a @ b`` for a one-per-column ``b``: out[r, n] = a[r, k(n)] b[k(n), n] as the arithmetic computes
    it -- the float64 sum of the kept limb products (exact: the products are of 11 bits or fewer each and the host test
    asserts from ``q`` and ``total`` that the sum has no more than 24); "fp32": the product rounded once.
    ``kept``: another list of products (the sensitivity tests).

    A column's non-zero is m or i m with m real, so the components of an output are single real products:
    (x + i y) m = x m + i y m and (x + i y) i m = -y m + i x m.  The sum over the kept (i, j) is taken limb of a by
    limb of a, sum_i a_i (sum_j b_j): a float64 product of 8 or 11 bits with at most 24, exact."""
    a, b = np.asarray(a), np.asarray(b)
    rows, vals = column_entries(b)
    is_im = vals.imag != 0
    mag = np.where(is_im, vals.imag, vals.real)
    if arith == "fp32":
        g = np.take(a, rows, axis=1)
        # (float64 holds a product of two 24-bit numbers exactly: rounded once, as an fp32 multiplication is)
        p, q = f32r(g.real * mag[None, :]), f32r(g.imag * mag[None, :])
        out = np.where(is_im[None, :], -q, p) + 1j * np.where(is_im[None, :], p, q)
        return Stage(out) if details else out
    kept = KEPT[arith] if kept is None else tuple(kept)
    re, im = f32(a.real), f32(a.imag)
    if arith == "bf16x3":
        sa = sb = 1.0
        lr, li, lb = split_bf16x3(re), split_bf16x3(im), split_bf16x3(f32(mag))
    else:
        sa = 2.0 ** (scale_shift - h2_exponent(top_of(a)))
        sb = 2.0 ** -h2_exponent(np.abs(mag).max())
        lr, li, lb = split_fp16x2(re, sa), split_fp16x2(im, sa), split_fp16x2(f32(mag), sb)
    lb = [x.astype(np.float64) for x in lb]
    p = np.zeros((a.shape[0], len(rows)))
    q = np.zeros_like(p)
    for i in range(LIMBS[arith]):
        js = [j for (i_, j) in kept if i_ == i]
        if not js:
            continue
        bi = sum(lb[j] for j in js)[None, :]
        p += np.take(lr[i], rows, axis=1) * bi
        q += np.take(li[i], rows, axis=1) * bi
    unit = 1.0 / (sa * sb)
    p *= unit
    q *= unit
    out = np.where(is_im[None, :], -q, p) + 1j * np.where(is_im[None, :], p, q)
    if not details:
        return out
    return Stage(out, *limb_bounds([np.concatenate([r, i], axis=1) for r, i in zip(lr, li)], lb, kept))


def limb_bounds(la, lb, kept):
    """``(q, total)`` of a Stage from the limbs of its operands (real arrays, one per limb)."""
    low_a, low_b = [low_bit_exponent(x) for x in la], [low_bit_exponent(x) for x in lb]
    qexp = min(low_a[i] + low_b[j] for i, j in kept if low_a[i] is not None and low_b[j] is not None)
    top_a = float(sum(np.abs(x.astype(np.float64)) for x in la).max())
    return qexp, top_a * float(sum(np.abs(np.asarray(x, dtype=np.float64)) for x in lb).max())


def stage32(re, im, b, arith, bounds=None):
    """``stage`` in fp32 arithmetic on separate planes, for the large rows: every limb product is exact in fp32 (8 x 8
    or 11 x 11 bits) and, under the any-order condition the host test asserts for the row, so is every partial sum --
    the float64 model's bits at a quarter of the memory traffic (asserted equal on the host).  Returns (re, im);
    ``bounds``: a list that receives the stage's (q, total) as limb_bounds gives them."""
    rows, vals = column_entries(np.asarray(b))
    K = re.shape[1]
    is_im = vals.imag != 0
    mag = np.where(is_im, vals.imag, vals.real)
    a2 = np.concatenate([re, im], axis=1)
    idx_p, idx_q = np.where(is_im, K + rows, rows), np.where(is_im, rows, K + rows)
    sgn_p = np.where(is_im, -1.0, 1.0).astype(np.float32)
    if arith == "fp32":
        m = mag[None, :]
        p = (np.take(a2, idx_p, axis=1).astype(np.float64) * (sgn_p * m)).astype(np.float32)
        q = (np.take(a2, idx_q, axis=1).astype(np.float64) * m).astype(np.float32)
        if bounds is not None:
            bounds.append((None, None))
        return p, q
    if arith == "bf16x3":
        sa = sb = 1.0
        la, lb = split_bf16x3(a2), split_bf16x3(f32(mag))
    else:
        sa = 2.0 ** -h2_exponent(np.abs(a2).max())
        sb = 2.0 ** -h2_exponent(np.abs(mag).max())
        la, lb = split_fp16x2(a2, sa), split_fp16x2(f32(mag), sb)
    if bounds is not None:
        bounds.append(limb_bounds(la, lb, KEPT[arith]))
    p = np.zeros((re.shape[0], len(rows)), dtype=np.float32)
    q = np.zeros_like(p)
    for i in range(LIMBS[arith]):
        gp, gq = np.take(la[i], idx_p, axis=1), np.take(la[i], idx_q, axis=1)
        for j in [j for (i_, j) in KEPT[arith] if i_ == i]:
            p += gp * (sgn_p * lb[j])[None, :]
            q += gq * lb[j][None, :]
    unit = np.float32(1.0 / (sa * sb))
    p *= unit
    q *= unit
    return p, q


def chain_model32(tree, arrays, ariths, bounds=None):
    """``chain_model`` through stage32: the result as complex64 (``bounds``: receives every stage's (q, total))."""
    assert tree.nslices == 1 and len(ariths) == len(arrays) - 1
    cur, x = list(tree.inputs[0]), np.asarray(arrays[0])
    x = (f32(x.real), f32(x.imag))
    for s, (inds, g) in enumerate(zip(tree.inputs[1:], arrays[1:])):
        k = sum(1 for ix in inds if ix in cur)
        con, new = list(inds[:k]), list(inds[k:])
        keep = [c for c in cur if c not in con]
        perm = [cur.index(c) for c in keep + con]
        re, im = (np.transpose(c, perm).reshape(-1, 1 << k) for c in x)
        x = stage32(re, im, np.asarray(g).reshape(1 << k, -1), ariths[s], bounds)
        cur = keep + new
        x = tuple(c.reshape((2,) * len(cur)) for c in x)
    perm = [cur.index(c) for c in tree.output]
    out = np.empty((2,) * len(cur), dtype=np.complex64)
    out.real, out.imag = np.transpose(x[0], perm), np.transpose(x[1], perm)
    return out


def f32r(x):
    """float64 -> the nearest fp32 number (ties to even), as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- #
# chains: a row of tests/stem_variant_cases.py
# ---------------------------------------------------------------------------------------------------------------- #
def gate_matrix(rng, k, n, values=None):
    """A gate tensor of shape (2,) * k + (2,) * n -- contracted indices first -- as its (2^k, 2^n) matrix."""
    return one_per_column(rng, 1 << k, 1 << n, values)


def chain_arrays(tree, gates, probe, values, seed):
    """The inputs of a stem ``[(3, 3)] + gates`` (tests/golden_util.py: stem_network) for a probe, as complex128:
    the state is dense probe values, the (3, 3) gate a unit, and of the stem step's small operands the one the probe
    names carries probe values -- "S1": B1, "S2": B2 -- the other is a unit."""
    assert probe in ("S1", "S2") and len(gates) in (1, 2) and not (probe == "S2" and len(gates) == 1)
    rng = np.random.default_rng(seed)
    shapes = [tuple(tree.size_dict[ix] for ix in t) for t in tree.inputs]
    out = [probe_complex(rng, shapes[0], values)]
    hot = {"S1": 2, "S2": 3}[probe]
    for i, (k, n) in enumerate([(3, 3)] + list(gates), start=1):
        assert shapes[i] == (2,) * (k + n)
        out.append(gate_matrix(rng, k, n, values if i == hot else None).reshape(shapes[i]))
    return out


def apply_gate(cur, x, gate_inds, k, g, fn):
    """The running tensor ``x`` with labels ``cur`` through one gate: ``fn(a[R, K], b[K, N]) -> [R, N]``.  Returns the
    new labels and tensor -- kept labels in their order, then the gate's new ones, as stem_network orders them."""
    con, new = list(gate_inds[:k]), list(gate_inds[k:])
    keep = [c for c in cur if c not in con]
    a = np.transpose(x, [cur.index(c) for c in keep + con]).reshape(-1, 1 << k)
    out = fn(a, np.asarray(g).reshape(1 << k, -1))
    return keep + new, out.reshape((2,) * (len(keep) + len(new)))


def chain_model(tree, arrays, ariths, kept=None, scale_shift=None, details=False):
    """The composition of the per-stage models along a stem: ``ariths[s]`` is the arithmetic of stage s (stage 0 is
    the (3, 3) gate, outside the stem kernel: "fp32").  ``kept``: {stage: products}; ``scale_shift``: {stage: powers
    of two on the fp16 x 2 scale of that stage's big operand}.  Returns the result in the tree's output order as
    complex128 (``details``: and the Stage records)."""
    assert tree.nslices == 1 and len(ariths) == len(arrays) - 1
    cur, x, recs = list(tree.inputs[0]), np.asarray(arrays[0]), []
    for s, (inds, g) in enumerate(zip(tree.inputs[1:], arrays[1:])):
        k = sum(1 for ix in inds if ix in cur)
        assert all(ix in cur for ix in inds[:k]) and not any(ix in cur for ix in inds[k:])

        def fn(a, b, s=s):
            st = stage(a, b, ariths[s], (kept or {}).get(s), (scale_shift or {}).get(s, 0), details=True)
            recs.append(st)
            return st.out

        cur, x = apply_gate(cur, x, inds, k, g, fn)
    out = np.transpose(x, [cur.index(c) for c in tree.output])
    return (out, recs) if details else out


def stem_cases():
    """(row, arithmetic asked for) of the probes: every 16-bit case of stem_variant_cases.DEVICE_CASES and the deep
    rows in their 16-bit arithmetic."""
    import stem_variant_cases as V
    return ([(r, a) for r, a in V.DEVICE_CASES if a in ARITHS] + [(r, r.arith) for r in V.DEEP_ROWS if r.arith in ARITHS])


def kernel_arith(row, arith):
    """The arithmetic the row's stem kernel multiplies in: the one asked for, or -- where the limb planes of the
    geometry do not fit the LDS and the step runs its fp32 instantiation (stem_variant_cases.has_16bit) -- "fp32"."""
    import stem_variant_cases as V
    return arith if V.expected(row, arith)[1]["bf3"] else "fp32"


def probes_of(row):
    return ("S1",) if row.one else ("S1", "S2")


def stage_ariths(row, arith):
    """The arithmetic of every stage of the row's chain: the (3, 3) gate in fp32, the stem step(s) in the kernel's."""
    return ["fp32"] + [kernel_arith(row, arith)] * len(row.gates)


# a chain whose state is larger than this is modelled in fp32 planes (chain_model32) on the device test
LARGE = 1 << 18


def model_c64(tree, arrays, ariths):
    """The chain's model as complex64: the float64 model, or its fp32-plane form for the large rows."""
    if np.asarray(arrays[0]).size > LARGE:
        return chain_model32(tree, arrays, ariths)
    return to_c64(chain_model(tree, arrays, ariths))


def probe_seed(row, probe):
    return 1000 * row.seed + 17 * row.nq + (1 if probe == "S1" else 2)


class Net:
    """The part of a tree chain_model reads."""

    def __init__(self, inputs, output):
        self.inputs, self.output, self.nslices = [tuple(t) for t in inputs], tuple(output), 1


def restrict(tree, arrays, max_elems):
    """``(net, arrays, index)``: the chain with indices of the state that no gate contracts fixed at 0 until the state
    has at most ``max_elems`` elements -- the same gates on fewer rows; ``result[index]`` of the whole chain's result
    is the restricted chain's result (a row of a stage depends on no other row)."""
    state = tree.inputs[0]
    free = [ix for ix in state if ix in tree.output]
    fixed = set(free[: max(0, len(state) - int(np.log2(max_elems)))])
    net = Net([tuple(ix for ix in state if ix not in fixed)] + list(tree.inputs[1:]),
              [ix for ix in tree.output if ix not in fixed])
    a0 = np.asarray(arrays[0])[tuple(0 if ix in fixed else slice(None) for ix in state)]
    index = tuple(0 if ix in fixed else slice(None) for ix in tree.output)
    return net, [a0] + list(arrays[1:]), index


def to_c64(x):
    """complex128 holding fp32 components -> complex64 (asserted exact)."""
    x = np.asarray(x)
    y = x.astype(np.complex64)
    assert np.array_equal(y.astype(np.complex128), x), "not fp32 numbers"
    return y


# ---------------------------------------------------------------------------------------------------------------- #
# a plain pair R x K x N
# ---------------------------------------------------------------------------------------------------------------- #
def pair_arrays(R, K, N, values, seed):
    """``(a[R, K], b[K, N])``: dense probe values, one-per-column probe values."""
    rng = np.random.default_rng(seed)
    return probe_complex(rng, (R, K), values), one_per_column(rng, K, N, values)
