"""The instantiations of the fused stem kernel (csrc/ctg_stem_impl.h: launch_stem), one row each.
tests/test_stem_variant_plans.py checks on the host that the planner gives every row the stem step this table records and
that the table names the very rows of the header's lists; tests/test_gpu_stem_variants.py runs the rows in the
arithmetic(s) they exist in, asserts the kernel the executor names (tests/golden_util.py: stem_flags) and compares the
numbers with the complex128 oracle -- random data under the suite's gate, integer data bit for bit.

A row is a small stem ``G.stem_network(nq, [(3, 3)] + gates, seed)`` -- the smallest ``nq`` of 15..18 and then the
smallest seed of 0..40 with which the planner, its pairing model opened up (G.fuse_whatever_fits, single steps for
free, ``fuse_min_elems = 1 << 10``), takes the shape --, the stem step's ``(K1, N1, K2, N2)``, the rest of its
geometry ``(nr1, items, ng2, vec)`` and the entry of the dispatch list the step must take, spelled as in the header:

    INST_ROWS     CTG_STEM_INST   (P1, P2, RT1, CS1, NCH, IT2, BR1, K2Q, VEC, RI2)   fp32 products
    GEO_ROWS      CTG_STEM_GEO    (P1, P2, RT1, CS1, NCH, IT2, VEC)                  bf16 x 3 and fp16 x 2
    ONE_ROWS      CTG_STEM_ONE    (RT1, CS1, NCH, VEC)                               the three arithmetics
    GENERIC_ROWS  CTG_STEM_CASE   (P1, P2, RT1, CS1, VEC),  CTG_STEM_CASE1 (RT1, CS1, VEC):  run-time counts

What a row's kernel must be called is worked out below from the header's rules, restated: ``stem_shape``
(stem2_shape), ``has_16bit`` (stem2_bf3), ``form_of`` (stem2_bf3_form) and ``expected`` (stem_kernel_name,
stem_step_h2).  Nothing here was read off a device; profiles/stem_variants.txt holds what one reported."""

T, F = True, False
SW, LDS = 8, 160 * 1024      # waves of a workgroup, bytes of LDS a kernel may ask for
BR1_CHUNKS = 2               # 16-bit kernels: B1's fragments in registers up to this many chunks
ARITHS = ("fp32", "bf16x3", "fp16x2")
MAX_FORM = {"bf16x3": 1, "fp16x2": 3}   # Bf16x3::max_form, Fp16x2::max_form


class Row:
    """``gates``: (contracted, new) index counts of the stem step(s) behind the (3, 3) gate; ``shape``: (K1, N1, K2, N2),
    zeros for a single step; ``geo``: (nr1, items, ng2, vec); ``args``: the dispatch entry; ``env``: what the environment
    must say at launch; ``sliced``: leading indices of the first tensor to slice."""

    def __init__(self, ident, nq, gates, seed, shape, geo, args, env=None, sliced=0):
        self.id, self.nq, self.gates, self.seed = ident, nq, [tuple(g) for g in gates], seed
        self.shape, self.geo, self.args = tuple(shape), tuple(geo), tuple(args)
        self.env, self.sliced = dict(env or {}), sliced

    def __repr__(self):
        return self.id

    @property
    def one(self):
        return self.shape[2] == 0

    @property
    def network(self):
        """What identifies the row's tree and data."""
        return (self.nq, tuple(self.gates), self.seed, self.sliced)

    def tree(self, upto=None):
        import golden_util as G
        return G.stem_network(self.nq, ([(3, 3)] + self.gates)[:upto], self.seed, sliced=self.sliced)

    def record(self):
        """The fields of the plan's ``stem`` record the kernel's rules read."""
        K1, N1, K2, N2 = self.shape
        nr1, items, ng2, vec = self.geo
        rows2 = 0 if self.one else ((1 << nr1) * N1) // K2
        return dict(K1=K1, N1=N1, K2=K2, N2=N2, nr1=nr1, items=items, ng2=ng2, vec=int(vec), one=int(self.one),
                    rows2=rows2, ld2=0 if self.one else K2 + 4)

    def like(self, ident, **kw):
        d = dict(nq=self.nq, gates=self.gates, seed=self.seed, shape=self.shape, geo=self.geo, args=self.args,
                 env=self.env, sliced=self.sliced)
        d.update(kw)
        return Row(ident, **d)


# ---------------------------------------------------------------------------------------------------------------- #
# The header's rules, restated
# ---------------------------------------------------------------------------------------------------------------- #
def lds_bytes_ri2(st, b2_in_regs):
    b1 = (3 if st["N1"] == 16 else 2) * st["N1"] * (st["K1"] + 4)
    b2 = 2 * st["N2"] * (st["K2"] + 4)
    mid = 3 * st["rows2"] * st["ld2"]
    return 4 * (b1 + (max(mid, b2) if b2_in_regs else b2 + mid)) + 8 * st["N2"]


def lds_bytes_16bit(st):
    """stem2_lds_bytes_bf3 / stem2_lds_bytes_one(p, true): the small operands as limb planes."""
    q1 = (3 if st["N1"] == 16 else 2) * st["N1"] * ((st["K1"] >> 4) * 48 + 8)
    if st["one"]:
        return 2 * q1 + 8 * st["N1"] + 64
    q2 = (3 if st["N2"] == 16 else 2) * st["N2"] * ((st["K2"] >> 3) * 24 + 8)
    return 2 * (q1 + q2) + 8 * st["rows2"] * st["ld2"] + 8 * st["N2"] + 64


def one_key(st):
    """(RT1, CS1, NCH, VEC) of a single step."""
    cs1 = st["N1"] // 32
    return ((1 << (st["nr1"] - 5)) * cs1 // SW, cs1, st["K1"] // 16, bool(st["vec"]))


def stem_shape(st):
    """stem2_shape of a pair with fp32 products: (P1, P2, RT1, CS1, NCH, IT2, BR1, K2Q, VEC, RI2)."""
    p1, p2 = st["N1"] == 16, st["N2"] == 16
    cs1 = max(1, st["N1"] // 32)
    rt1 = (1 << (st["nr1"] - 5)) * cs1 // SW
    nch = st["K1"] // 16
    it2 = st["items"] // SW if st["items"] % SW == 0 else 0
    vec, ng2 = bool(st["vec"]), st["ng2"]
    if not p2 and it2 > 0 and 1 <= ng2 <= SW and SW % ng2 == 0:
        fixed = rt1 * (16 if p1 else 32) + (64 if it2 > 1 else 32) + 32 + 40
        r1 = st["K1"] if st["K1"] <= 64 else 0
        r2 = st["K2"] if st["K2"] <= 64 else 0
        if fixed + r1 + r2 > 256:
            r2 = 0
        if fixed + r1 > 256:
            r1 = 0
        if lds_bytes_ri2(st, r2 != 0) <= LDS:
            return (p1, p2, rt1, cs1, nch, it2, bool(r1), st["K2"] // 4 if r2 else 0, vec, True)
    r1 = st["K1"] if st["K1"] <= 64 else 0
    r2 = 0
    if (p2 and st["K2"] <= 64) or (not p2 and it2 == 1 and st["K2"] <= 32):
        r2 = st["K2"] if p2 else 2 * st["K2"]
    if r1 and r2 and r1 + r2 > 96:
        r2 = 0
    return (p1, p2, rt1, cs1, nch, it2, bool(r1), st["K2"] // 4 if r2 else 0, vec, False)


def geo_of(shape10):
    """(P1, P2, RT1, CS1, NCH, IT2, VEC) of a stem_shape."""
    return shape10[:6] + (shape10[8],)


def generic_key(st):
    """The entry of the run-time-count dispatch a step would take."""
    if st["one"]:
        k = one_key(st)
        return (k[0], k[1], k[3])
    s = stem_shape(st)
    return (s[0], s[1], s[2], s[3], s[8])


def has_16bit(st, generic=False):
    """stem2_bf3 with a 16-bit arithmetic asked for: a static instantiation of the geometry, and room for the planes."""
    if generic:
        return False
    if st["one"]:
        return one_key(st) in ONE_ARGS and lds_bytes_16bit(st) <= LDS
    s = stem_shape(st)
    return s[5] > 0 and geo_of(s) in GEO_ARGS and st["K2"] % 8 == 0 and lds_bytes_16bit(st) <= LDS


def form_of(arith, geo7, form_env=None):
    """stem2_bf3_form, in terms of the geometry (items = IT2 x 8, units = RT1 x 8): 3, specialised waves -- at most two
    items per wave, one unit per wave unless step 1 has 16 columns, and not two items of 32 columns --; 0, the form with
    sign flips on limbs, for four items per wave; else 1, the symmetric form."""
    p1, p2, rt1, _, _, it2, _ = geo7
    form = MAX_FORM[arith]
    if form_env is not None:
        form = min(form, int(form_env))
    if form < 1 or form == 2:
        form = 1
    if form == 3 and not (it2 <= 2 and (p1 or rt1 == 1)):
        form = 1
    if form == 3 and it2 == 2 and not p2:
        form = 1
    if it2 >= 4:
        form = 0
    return form


def _flags(p1, p2, rt1, cs1, nch, it2, br1, k2q, vec, bf3, ri2, one, xm=False, ws=False):
    return {"pack1": p1, "pack2": p2, "rt1": rt1, "cs1": cs1, "nch": nch, "it2": it2, "br1": br1, "k2q": k2q, "vec": vec,
            "bf3": bf3, "ri2": ri2, "one": one, "itm": 0, "packm": False, "xm": xm, "lm": False, "ws": ws}


def expected(row, arith, env=None):
    """(kernel, flags as G.stem_flags spells them) of ``row`` run in ``arith`` with ``env`` in the environment
    (stem_kernel_name; the fp16 x 2 object, stem2h_kernel, holds 16-bit instantiations only: stem_step_h2)."""
    env = dict(row.env, **(env or {}))
    st = row.record()
    generic = env.get("CTG_STEM_GENERIC") not in (None, "", "0")
    b16 = arith != "fp32" and has_16bit(st, generic)
    kernel = "stem2h_kernel" if (b16 and arith == "fp16x2") else "stem2_kernel"
    if st["one"]:
        rt1, cs1, nch, vec = one_key(st)
        static = not generic and (rt1, cs1, nch, vec) in ONE_ARGS
        if static and b16:
            return kernel, _flags(F, F, rt1, cs1, nch, 0, nch <= BR1_CHUNKS, 0, vec, T, F, T, xm=T)
        return kernel, _flags(F, F, rt1, cs1, nch if static else 0, 0, static and st["K1"] <= 64, 0, vec, F, F, T)
    s = stem_shape(st)
    p1, p2, rt1, cs1, nch, it2, br1, k2q, vec, ri2 = s
    if b16:
        form = form_of(arith, geo_of(s), env.get("CTG_STEM_FORM"))
        if form == 0:
            return kernel, _flags(p1, p2, rt1, cs1, nch, it2, nch <= BR1_CHUNKS, 0, vec, T, F, F)
        b = ((2 if cs1 == 2 else 1) * nch <= BR1_CHUNKS) if form == 3 else nch <= BR1_CHUNKS   # (stem_br1_ws)
        return kernel, _flags(p1, p2, rt1, cs1, nch, it2, b, 0, vec, T, F, F, xm=T, ws=form == 3)
    if not generic and it2 > 0 and s in INST_ARGS:
        return kernel, _flags(p1, p2, rt1, cs1, nch, it2, br1, k2q, vec, F, ri2, F)
    return kernel, _flags(p1, p2, rt1, cs1, 0, 0, F, 0, vec, F, F, F)


# ---------------------------------------------------------------------------------------------------------------- #
# The rows.  Columns: id, nq, gates, seed, (K1, N1, K2, N2), (nr1, items, ng2, vec), the dispatch entry.
# ---------------------------------------------------------------------------------------------------------------- #
_GENERIC = {"CTG_STEM_GENERIC": "1"}


def _geo(ident, nq, gates, seed, shape, geo, args, forms, fits16=True):
    """A geometry: ``forms``, the form of the 16-bit pair in (bf16 x 3, fp16 x 2); ``fits16`` False: the limb planes of
    this geometry fit the LDS with no K2, N2 (tests/test_stem_variant_plans.py enumerates them), so stem2_bf3 says no
    and the step runs the fp32 instantiation of the same shape in every arithmetic -- the 16-bit one is never launched."""
    r = Row(ident, nq, gates, seed, shape, geo, args)
    r.forms, r.fits16 = tuple(forms), fits16
    return r


# CTG_STEM_INST, in the header's order: run with fp32 products
INST_ROWS = [
    Row("I01", 15, [(5, 5), (5, 5)], 0, (32, 32, 32, 32), (8, 8, 1, 0), (F, F, 1, 1, 2, 1, T, 8, F, T)),   # k32 n32 | k32 n32
    Row("I02", 15, [(5, 5), (4, 4)], 0, (32, 32, 16, 16), (8, 16, 1, 0), (F, T, 1, 1, 2, 2, T, 4, F, F)),   # k32 n32 | k16 n16
    Row("I03", 15, [(6, 6), (5, 5)], 0, (64, 64, 32, 32), (7, 8, 1, 0), (F, F, 1, 2, 4, 1, T, 8, F, T)),   # k64 n64 | k32 n32
    Row("I04", 15, [(5, 5), (6, 6)], 0, (32, 32, 64, 64), (8, 8, 2, 0), (F, F, 1, 1, 2, 1, T, 16, F, T)),   # k32 n32 | k64 n64
    Row("I05", 15, [(4, 4), (4, 4)], 0, (16, 16, 16, 16), (9, 16, 1, 0), (T, T, 2, 1, 1, 2, T, 4, F, F)),   # k16 n16 | k16 n16
    Row("I06", 15, [(5, 5), (4, 4)], 2, (32, 32, 16, 16), (8, 16, 1, 1), (F, T, 1, 1, 2, 2, T, 4, T, F)),   # k32 n32 | k16 n16
    Row("I07", 15, [(4, 4), (5, 5)], 0, (16, 16, 32, 32), (9, 8, 1, 0), (T, F, 2, 1, 1, 1, T, 8, F, T)),   # k16 n16 | k32 n32
    Row("I08", 15, [(5, 6), (5, 5)], 0, (32, 64, 32, 32), (7, 8, 1, 0), (F, F, 1, 2, 2, 1, T, 8, F, T)),   # k32 n64 | k32 n32
    Row("I09", 15, [(6, 6), (5, 5)], 7, (64, 64, 32, 32), (7, 8, 1, 1), (F, F, 1, 2, 4, 1, T, 8, T, T)),   # k64 n64 | k32 n32
    Row("I10", 15, [(7, 5), (5, 5)], 0, (128, 32, 32, 32), (8, 8, 1, 0), (F, F, 1, 1, 8, 1, F, 8, F, T)),   # k128 n32 | k32 n32
    Row("I11", 15, [(4, 4), (4, 4)], 7, (16, 16, 16, 16), (9, 16, 1, 1), (T, T, 2, 1, 1, 2, T, 4, T, F)),   # k16 n16 | k16 n16
    Row("I12", 15, [(4, 4), (5, 5)], 7, (16, 16, 32, 32), (9, 8, 1, 1), (T, F, 2, 1, 1, 1, T, 8, T, T)),   # k16 n16 | k32 n32
    Row("I13", 15, [(6, 6), (6, 6)], 0, (64, 64, 64, 64), (7, 8, 2, 0), (F, F, 1, 2, 4, 1, T, 0, F, F)),   # k64 n64 | k64 n64
    Row("I14", 15, [(5, 5), (5, 6)], 0, (32, 32, 32, 64), (8, 16, 2, 0), (F, F, 1, 1, 2, 2, T, 8, F, T)),   # k32 n32 | k32 n64
    Row("I15", 15, [(4, 5), (4, 4)], 0, (16, 32, 16, 16), (8, 16, 1, 0), (F, T, 1, 1, 1, 2, T, 4, F, F)),   # k16 n32 | k16 n16
    Row("I16", 15, [(5, 6), (6, 6)], 0, (32, 64, 64, 64), (7, 8, 2, 0), (F, F, 1, 2, 2, 1, T, 16, F, T)),   # k32 n64 | k64 n64
    Row("I17", 15, [(5, 6), (4, 4)], 0, (32, 64, 16, 16), (7, 16, 1, 0), (F, T, 1, 2, 2, 2, T, 4, F, F)),   # k32 n64 | k16 n16
    Row("I18", 15, [(4, 4), (5, 6)], 7, (16, 16, 32, 64), (9, 16, 2, 1), (T, F, 2, 1, 1, 2, T, 8, T, T)),   # k16 n16 | k32 n64
    Row("I19", 15, [(6, 6), (4, 4)], 0, (64, 64, 16, 16), (7, 16, 1, 0), (F, T, 1, 2, 4, 2, T, 4, F, F)),   # k64 n64 | k16 n16
    Row("I20", 15, [(6, 6), (5, 6)], 0, (64, 64, 32, 64), (7, 16, 2, 0), (F, F, 1, 2, 4, 2, T, 0, F, F)),   # k64 n64 | k32 n64
    Row("I21", 15, [(6, 5), (5, 5)], 7, (64, 32, 32, 32), (8, 8, 1, 1), (F, F, 1, 1, 4, 1, T, 8, T, T)),   # k64 n32 | k32 n32
    Row("I22", 15, [(4, 6), (5, 5)], 0, (16, 64, 32, 32), (7, 8, 1, 0), (F, F, 1, 2, 1, 1, T, 8, F, T)),   # k16 n64 | k32 n32
    Row("I23", 15, [(7, 5), (5, 6)], 0, (128, 32, 32, 64), (8, 16, 2, 0), (F, F, 1, 1, 8, 2, F, 8, F, T)),   # k128 n32 | k32 n64
    Row("I24", 15, [(4, 4), (5, 6)], 0, (16, 16, 32, 64), (9, 16, 2, 0), (T, F, 2, 1, 1, 2, T, 8, F, T)),   # k16 n16 | k32 n64
    Row("I25", 15, [(5, 6), (4, 6)], 2, (32, 64, 16, 64), (7, 32, 2, 1), (F, F, 1, 2, 2, 4, T, 4, T, T)),   # k32 n64 | k16 n64
    Row("I26", 15, [(5, 5), (5, 5)], 2, (32, 32, 32, 32), (8, 8, 1, 1), (F, F, 1, 1, 2, 1, T, 8, T, T)),   # k32 n32 | k32 n32
    Row("I27", 15, [(5, 5), (6, 7)], 0, (32, 32, 64, 128), (8, 16, 4, 0), (F, F, 1, 1, 2, 2, T, 0, F, F)),   # k32 n32 | k64 n128
    Row("I28", 15, [(4, 4), (6, 7)], 0, (16, 16, 64, 128), (9, 16, 4, 0), (T, F, 2, 1, 1, 2, T, 16, F, T)),   # k16 n16 | k64 n128
    Row("I29", 15, [(4, 5), (5, 5)], 0, (16, 32, 32, 32), (9, 16, 1, 0), (F, F, 2, 1, 1, 2, T, 0, F, F)),   # k16 n32 | k32 n32
    Row("I30", 15, [(4, 5), (5, 6)], 0, (16, 32, 32, 64), (8, 16, 2, 0), (F, F, 1, 1, 1, 2, T, 8, F, T)),   # k16 n32 | k32 n64
    Row("I31", 15, [(6, 5), (6, 6)], 0, (64, 32, 64, 64), (8, 8, 2, 0), (F, F, 1, 1, 4, 1, T, 0, F, T)),   # k64 n32 | k64 n64
    Row("I32", 15, [(5, 6), (5, 4)], 0, (32, 64, 32, 16), (7, 8, 1, 0), (F, T, 1, 2, 2, 1, T, 8, F, F)),   # k32 n64 | k32 n16
    Row("I33", 15, [(5, 5), (5, 4)], 0, (32, 32, 32, 16), (8, 8, 1, 0), (F, T, 1, 1, 2, 1, T, 8, F, F)),   # k32 n32 | k32 n16
    Row("I34", 15, [(6, 7), (4, 4)], 7, (64, 128, 16, 16), (6, 16, 1, 1), (F, T, 1, 4, 4, 2, T, 4, T, F)),   # k64 n128 | k16 n16
    Row("I35", 15, [(7, 5), (4, 4)], 3, (128, 32, 16, 16), (8, 16, 1, 1), (F, T, 1, 1, 8, 2, F, 4, T, F)),   # k128 n32 | k16 n16
    Row("I36", 15, [(5, 4), (5, 5)], 0, (32, 16, 32, 32), (9, 8, 1, 0), (T, F, 2, 1, 2, 1, T, 8, F, T)),   # k32 n16 | k32 n32
    Row("I37", 15, [(4, 4), (4, 5)], 0, (16, 16, 16, 32), (9, 16, 1, 0), (T, F, 2, 1, 1, 2, T, 4, F, T)),   # k16 n16 | k16 n32
    Row("I38", 15, [(4, 4), (6, 6)], 0, (16, 16, 64, 64), (9, 8, 2, 0), (T, F, 2, 1, 1, 1, T, 16, F, T)),   # k16 n16 | k64 n64
    Row("I39", 15, [(7, 5), (4, 4)], 0, (128, 32, 16, 16), (8, 16, 1, 0), (F, T, 1, 1, 8, 2, F, 4, F, F)),   # k128 n32 | k16 n16
    Row("I40", 15, [(5, 5), (4, 6)], 0, (32, 32, 16, 64), (8, 32, 2, 0), (F, F, 1, 1, 2, 4, T, 4, F, T)),   # k32 n32 | k16 n64
    Row("I41", 15, [(5, 5), (5, 7)], 0, (32, 32, 32, 128), (8, 32, 4, 0), (F, F, 1, 1, 2, 4, T, 8, F, T)),   # k32 n32 | k32 n128
    Row("I42", 15, [(5, 5), (4, 5)], 0, (32, 32, 16, 32), (8, 16, 1, 0), (F, F, 1, 1, 2, 2, T, 4, F, T)),   # k32 n32 | k16 n32
    Row("I43", 15, [(6, 4), (5, 4)], 0, (64, 16, 32, 16), (9, 8, 1, 0), (T, T, 2, 1, 4, 1, T, 8, F, F)),   # k64 n16 | k32 n16
    Row("I44", 15, [(5, 6), (5, 6)], 2, (32, 64, 32, 64), (7, 16, 2, 1), (F, F, 1, 2, 2, 2, T, 8, T, T)),   # k32 n64 | k32 n64
    Row("I45", 15, [(4, 6), (4, 4)], 0, (16, 64, 16, 16), (7, 16, 1, 0), (F, T, 1, 2, 1, 2, T, 4, F, F)),   # k16 n64 | k16 n16
    Row("I46", 15, [(6, 4), (5, 5)], 0, (64, 16, 32, 32), (9, 8, 1, 0), (T, F, 2, 1, 4, 1, T, 8, F, T)),   # k64 n16 | k32 n32
    Row("I47", 15, [(5, 6), (4, 6)], 0, (32, 64, 16, 64), (7, 32, 2, 0), (F, F, 1, 2, 2, 4, T, 4, F, T)),   # k32 n64 | k16 n64
]

# CTG_STEM_GEO, in the header's order: run in bf16 x 3 and in fp16 x 2; the last column is the form in each
GEO_ROWS = [
    _geo("G01", 15, [(4, 5), (4, 5)], 0, (16, 32, 16, 32), (8, 16, 1, 0), (F, F, 1, 1, 1, 2, F), (1, 1)),   # k16 n32 | k16 n32
    _geo("G02", 15, [(5, 5), (5, 5)], 0, (32, 32, 32, 32), (8, 8, 1, 0), (F, F, 1, 1, 2, 1, F), (1, 3)),   # k32 n32 | k32 n32
    _geo("G03", 15, [(5, 5), (5, 5)], 2, (32, 32, 32, 32), (8, 8, 1, 1), (F, F, 1, 1, 2, 1, T), (1, 3)),   # k32 n32 | k32 n32
    _geo("G04", 15, [(5, 5), (4, 5)], 0, (32, 32, 16, 32), (8, 16, 1, 0), (F, F, 1, 1, 2, 2, F), (1, 1)),   # k32 n32 | k16 n32
    _geo("G05", 15, [(5, 5), (4, 6)], 0, (32, 32, 16, 64), (8, 32, 2, 0), (F, F, 1, 1, 2, 4, F), (0, 0)),   # k32 n32 | k16 n64
    _geo("G06", 15, [(6, 5), (5, 5)], 0, (64, 32, 32, 32), (8, 8, 1, 0), (F, F, 1, 1, 4, 1, F), (1, 3)),   # k64 n32 | k32 n32
    _geo("G07", 16, [(6, 5), (5, 5)], 1, (64, 32, 32, 32), (8, 8, 1, 1), (F, F, 1, 1, 4, 1, T), (1, 3)),   # k64 n32 | k32 n32
    _geo("G08", 15, [(7, 5), (5, 5)], 0, (128, 32, 32, 32), (8, 8, 1, 0), (F, F, 1, 1, 8, 1, F), (1, 3)),   # k128 n32 | k32 n32
    _geo("G09", 15, [(7, 5), (4, 5)], 0, (128, 32, 16, 32), (8, 16, 1, 0), (F, F, 1, 1, 8, 2, F), (1, 1)),   # k128 n32 | k16 n32
    _geo("G10", 15, [(4, 6), (5, 5)], 0, (16, 64, 32, 32), (7, 8, 1, 0), (F, F, 1, 2, 1, 1, F), (1, 3)),   # k16 n64 | k32 n32
    _geo("G11", 15, [(5, 6), (5, 5)], 0, (32, 64, 32, 32), (7, 8, 1, 0), (F, F, 1, 2, 2, 1, F), (1, 3)),   # k32 n64 | k32 n32
    _geo("G12", 15, [(5, 6), (4, 6)], 2, (32, 64, 16, 64), (7, 32, 2, 1), (F, F, 1, 2, 2, 4, T), (0, 0)),   # k32 n64 | k16 n64
    _geo("G13", 15, [(6, 6), (5, 5)], 0, (64, 64, 32, 32), (7, 8, 1, 0), (F, F, 1, 2, 4, 1, F), (1, 3)),   # k64 n64 | k32 n32
    _geo("G14", 16, [(6, 6), (5, 5)], 1, (64, 64, 32, 32), (7, 8, 1, 1), (F, F, 1, 2, 4, 1, T), (1, 3)),   # k64 n64 | k32 n32
    _geo("G15", 15, [(6, 6), (4, 5)], 0, (64, 64, 16, 32), (7, 16, 1, 0), (F, F, 1, 2, 4, 2, F), (1, 1)),   # k64 n64 | k16 n32
    _geo("G16", 15, [(4, 5), (5, 5)], 0, (16, 32, 32, 32), (9, 16, 1, 0), (F, F, 2, 1, 1, 2, F), (1, 1), fits16=F),   # k16 n32 | k32 n32
    _geo("G17", 15, [(4, 5), (4, 4)], 0, (16, 32, 16, 16), (8, 16, 1, 0), (F, T, 1, 1, 1, 2, F), (1, 3)),   # k16 n32 | k16 n16
    _geo("G18", 15, [(5, 5), (5, 4)], 0, (32, 32, 32, 16), (8, 8, 1, 0), (F, T, 1, 1, 2, 1, F), (1, 3)),   # k32 n32 | k32 n16
    _geo("G19", 15, [(5, 5), (4, 4)], 0, (32, 32, 16, 16), (8, 16, 1, 0), (F, T, 1, 1, 2, 2, F), (1, 3)),   # k32 n32 | k16 n16
    _geo("G20", 15, [(5, 5), (4, 4)], 2, (32, 32, 16, 16), (8, 16, 1, 1), (F, T, 1, 1, 2, 2, T), (1, 3)),   # k32 n32 | k16 n16
    _geo("G21", 15, [(7, 5), (4, 4)], 0, (128, 32, 16, 16), (8, 16, 1, 0), (F, T, 1, 1, 8, 2, F), (1, 3)),   # k128 n32 | k16 n16
    _geo("G22", 15, [(7, 5), (4, 4)], 3, (128, 32, 16, 16), (8, 16, 1, 1), (F, T, 1, 1, 8, 2, T), (1, 3)),   # k128 n32 | k16 n16
    _geo("G23", 15, [(5, 6), (5, 4)], 0, (32, 64, 32, 16), (7, 8, 1, 0), (F, T, 1, 2, 2, 1, F), (1, 3)),   # k32 n64 | k32 n16
    _geo("G24", 15, [(5, 6), (4, 4)], 0, (32, 64, 16, 16), (7, 16, 1, 0), (F, T, 1, 2, 2, 2, F), (1, 3)),   # k32 n64 | k16 n16
    _geo("G25", 15, [(6, 6), (4, 4)], 0, (64, 64, 16, 16), (7, 16, 1, 0), (F, T, 1, 2, 4, 2, F), (1, 3)),   # k64 n64 | k16 n16
    _geo("G26", 15, [(6, 7), (4, 4)], 7, (64, 128, 16, 16), (6, 16, 1, 1), (F, T, 1, 4, 4, 2, T), (1, 3), fits16=F),   # k64 n128 | k16 n16
    _geo("G27", 15, [(4, 4), (5, 5)], 0, (16, 16, 32, 32), (9, 8, 1, 0), (T, F, 2, 1, 1, 1, F), (1, 3)),   # k16 n16 | k32 n32
    _geo("G28", 18, [(4, 4), (5, 5)], 2, (16, 16, 32, 32), (9, 8, 1, 1), (T, F, 2, 1, 1, 1, T), (1, 3)),   # k16 n16 | k32 n32
    _geo("G29", 15, [(4, 4), (4, 5)], 0, (16, 16, 16, 32), (9, 16, 1, 0), (T, F, 2, 1, 1, 2, F), (1, 1)),   # k16 n16 | k16 n32
    _geo("G30", 18, [(4, 4), (4, 5)], 2, (16, 16, 16, 32), (9, 16, 1, 1), (T, F, 2, 1, 1, 2, T), (1, 1)),   # k16 n16 | k16 n32
    _geo("G31", 15, [(5, 4), (5, 5)], 0, (32, 16, 32, 32), (9, 8, 1, 0), (T, F, 2, 1, 2, 1, F), (1, 3)),   # k32 n16 | k32 n32
    _geo("G32", 15, [(4, 4), (4, 4)], 0, (16, 16, 16, 16), (9, 16, 1, 0), (T, T, 2, 1, 1, 2, F), (1, 3)),   # k16 n16 | k16 n16
    _geo("G33", 18, [(4, 4), (4, 4)], 2, (16, 16, 16, 16), (9, 16, 1, 1), (T, T, 2, 1, 1, 2, T), (1, 3)),   # k16 n16 | k16 n16
    _geo("G34", 15, [(6, 4), (5, 4)], 0, (64, 16, 32, 16), (9, 8, 1, 0), (T, T, 2, 1, 4, 1, F), (1, 3)),   # k64 n16 | k32 n16
    _geo("G35", 15, [(5, 6), (4, 5)], 2, (32, 64, 16, 32), (7, 16, 1, 1), (F, F, 1, 2, 2, 2, T), (1, 1)),   # k32 n64 | k16 n32
    _geo("G36", 15, [(4, 6), (4, 4)], 0, (16, 64, 16, 16), (7, 16, 1, 0), (F, T, 1, 2, 1, 2, F), (1, 3)),   # k16 n64 | k16 n16
    _geo("G37", 15, [(6, 4), (5, 5)], 0, (64, 16, 32, 32), (9, 8, 1, 0), (T, F, 2, 1, 4, 1, F), (1, 3)),   # k64 n16 | k32 n32
    _geo("G38", 15, [(5, 6), (4, 6)], 0, (32, 64, 16, 64), (7, 32, 2, 0), (F, F, 1, 2, 2, 4, F), (0, 0)),   # k32 n64 | k16 n64
]

# CTG_STEM_ONE, in the header's order: run in the three arithmetics.  By the kernel's rules O01 (K = N = 128: no room
# for B1's limb planes, stem2_lds_bytes_one) runs its static fp32 instantiation in all three.
ONE_ROWS = [
    Row("O01", 15, [(7, 7)], 0, (128, 128, 0, 0), (6, 0, 0, 0), (1, 4, 8, F)),   # k128 n128
    Row("O02", 15, [(5, 5)], 0, (32, 32, 0, 0), (8, 0, 0, 0), (1, 1, 2, F)),   # k32 n32
    Row("O03", 15, [(6, 6)], 0, (64, 64, 0, 0), (7, 0, 0, 0), (1, 2, 4, F)),   # k64 n64
    Row("O04", 15, [(7, 5)], 0, (128, 32, 0, 0), (8, 0, 0, 0), (1, 1, 8, F)),   # k128 n32
    Row("O05", 15, [(6, 5)], 0, (64, 32, 0, 0), (8, 0, 0, 0), (1, 1, 4, F)),   # k64 n32
    Row("O06", 15, [(6, 7)], 0, (64, 128, 0, 0), (6, 0, 0, 0), (1, 4, 4, F)),   # k64 n128
    Row("O07", 15, [(5, 5)], 2, (32, 32, 0, 0), (8, 0, 0, 1), (1, 1, 2, T)),   # k32 n32
    Row("O08", 15, [(5, 6)], 2, (32, 64, 0, 0), (7, 0, 0, 1), (1, 2, 2, T)),   # k32 n64
    Row("O09", 15, [(4, 5)], 0, (16, 32, 0, 0), (9, 0, 0, 0), (2, 1, 1, F)),   # k16 n32
    Row("O10", 15, [(7, 6)], 0, (128, 64, 0, 0), (7, 0, 0, 0), (1, 2, 8, F)),   # k128 n64
]

# The run-time-count variants, fp32 products.  RP_*: a pair under CTG_STEM_GENERIC=1, entry (P1, P2, RT1, CS1, VEC);
# RO_*: a single step under it, entry (RT1, CS1, VEC); RZ_*: pairs that take the variant by themselves -- four items
# of step 2, no multiple of the eight waves.
GENERIC_ROWS = [
    Row("RP_ff11f", 15, [(4, 5), (4, 5)], 0, (16, 32, 16, 32), (8, 16, 1, 0), (F, F, 1, 1, F), env=_GENERIC),   # k16 n32 | k16 n32
    Row("RP_ff11t", 15, [(5, 5), (4, 5)], 2, (32, 32, 16, 32), (8, 16, 1, 1), (F, F, 1, 1, T), env=_GENERIC),   # k32 n32 | k16 n32
    Row("RP_ff12f", 15, [(4, 6), (4, 5)], 0, (16, 64, 16, 32), (7, 16, 1, 0), (F, F, 1, 2, F), env=_GENERIC),   # k16 n64 | k16 n32
    Row("RP_ff12t", 15, [(5, 6), (4, 5)], 2, (32, 64, 16, 32), (7, 16, 1, 1), (F, F, 1, 2, T), env=_GENERIC),   # k32 n64 | k16 n32
    Row("RP_ff14f", 15, [(4, 7), (4, 5)], 0, (16, 128, 16, 32), (6, 16, 1, 0), (F, F, 1, 4, F), env=_GENERIC),   # k16 n128 | k16 n32
    Row("RP_ff14t", 15, [(5, 7), (4, 5)], 2, (32, 128, 16, 32), (6, 16, 1, 1), (F, F, 1, 4, T), env=_GENERIC),   # k32 n128 | k16 n32
    Row("RP_ff21f", 15, [(4, 5), (5, 5)], 0, (16, 32, 32, 32), (9, 16, 1, 0), (F, F, 2, 1, F), env=_GENERIC),   # k16 n32 | k32 n32
    Row("RP_ff21t", 15, [(4, 5), (5, 5)], 7, (16, 32, 32, 32), (9, 16, 1, 1), (F, F, 2, 1, T), env=_GENERIC),   # k16 n32 | k32 n32
    Row("RP_ft11f", 15, [(4, 5), (4, 4)], 0, (16, 32, 16, 16), (8, 16, 1, 0), (F, T, 1, 1, F), env=_GENERIC),   # k16 n32 | k16 n16
    Row("RP_ft11t", 15, [(5, 5), (4, 4)], 2, (32, 32, 16, 16), (8, 16, 1, 1), (F, T, 1, 1, T), env=_GENERIC),   # k32 n32 | k16 n16
    Row("RP_ft12f", 15, [(4, 6), (4, 4)], 0, (16, 64, 16, 16), (7, 16, 1, 0), (F, T, 1, 2, F), env=_GENERIC),   # k16 n64 | k16 n16
    Row("RP_ft12t", 15, [(5, 6), (4, 4)], 2, (32, 64, 16, 16), (7, 16, 1, 1), (F, T, 1, 2, T), env=_GENERIC),   # k32 n64 | k16 n16
    Row("RP_ft14f", 15, [(4, 7), (4, 4)], 0, (16, 128, 16, 16), (6, 16, 1, 0), (F, T, 1, 4, F), env=_GENERIC),   # k16 n128 | k16 n16
    Row("RP_ft14t", 15, [(5, 7), (4, 4)], 2, (32, 128, 16, 16), (6, 16, 1, 1), (F, T, 1, 4, T), env=_GENERIC),   # k32 n128 | k16 n16
    Row("RP_ft21f", 15, [(4, 5), (5, 4)], 0, (16, 32, 32, 16), (9, 16, 1, 0), (F, T, 2, 1, F), env=_GENERIC),   # k16 n32 | k32 n16
    Row("RP_ft21t", 15, [(5, 5), (6, 4)], 2, (32, 32, 64, 16), (9, 8, 1, 1), (F, T, 2, 1, T), env=_GENERIC),   # k32 n32 | k64 n16
    Row("RP_ft22f", 15, [(4, 6), (6, 4)], 0, (16, 64, 64, 16), (8, 8, 1, 0), (F, T, 2, 2, F), env=_GENERIC),   # k16 n64 | k64 n16
    Row("RP_ft22t", 15, [(4, 6), (6, 4)], 7, (16, 64, 64, 16), (8, 8, 1, 1), (F, T, 2, 2, T), env=_GENERIC),   # k16 n64 | k64 n16
    Row("RP_tf11f", 15, [(5, 4), (4, 5)], 0, (32, 16, 16, 32), (8, 8, 1, 0), (T, F, 1, 1, F), env=_GENERIC),   # k32 n16 | k16 n32
    Row("RP_tf11t", 15, [(5, 4), (4, 5)], 2, (32, 16, 16, 32), (8, 8, 1, 1), (T, F, 1, 1, T), env=_GENERIC),   # k32 n16 | k16 n32
    Row("RP_tf21f", 15, [(4, 4), (4, 5)], 0, (16, 16, 16, 32), (9, 16, 1, 0), (T, F, 2, 1, F), env=_GENERIC),   # k16 n16 | k16 n32
    Row("RP_tf21t", 15, [(5, 4), (5, 5)], 2, (32, 16, 32, 32), (9, 8, 1, 1), (T, F, 2, 1, T), env=_GENERIC),   # k32 n16 | k32 n32
    Row("RP_tt11f", 15, [(5, 4), (4, 4)], 0, (32, 16, 16, 16), (8, 8, 1, 0), (T, T, 1, 1, F), env=_GENERIC),   # k32 n16 | k16 n16
    Row("RP_tt11t", 15, [(5, 4), (4, 4)], 2, (32, 16, 16, 16), (8, 8, 1, 1), (T, T, 1, 1, T), env=_GENERIC),   # k32 n16 | k16 n16
    Row("RP_tt21f", 15, [(4, 4), (4, 4)], 0, (16, 16, 16, 16), (9, 16, 1, 0), (T, T, 2, 1, F), env=_GENERIC),   # k16 n16 | k16 n16
    Row("RP_tt21t", 15, [(5, 4), (5, 4)], 2, (32, 16, 32, 16), (9, 8, 1, 1), (T, T, 2, 1, T), env=_GENERIC),   # k32 n16 | k32 n16
    Row("RO_11f", 15, [(5, 5)], 0, (32, 32, 0, 0), (8, 0, 0, 0), (1, 1, F), env=_GENERIC),   # k32 n32
    Row("RO_11t", 15, [(5, 5)], 2, (32, 32, 0, 0), (8, 0, 0, 1), (1, 1, T), env=_GENERIC),   # k32 n32
    Row("RO_12f", 15, [(5, 6)], 0, (32, 64, 0, 0), (7, 0, 0, 0), (1, 2, F), env=_GENERIC),   # k32 n64
    Row("RO_12t", 15, [(5, 6)], 2, (32, 64, 0, 0), (7, 0, 0, 1), (1, 2, T), env=_GENERIC),   # k32 n64
    Row("RO_14f", 15, [(5, 7)], 0, (32, 128, 0, 0), (6, 0, 0, 0), (1, 4, F), env=_GENERIC),   # k32 n128
    Row("RO_14t", 15, [(5, 7)], 2, (32, 128, 0, 0), (6, 0, 0, 1), (1, 4, T), env=_GENERIC),   # k32 n128
    Row("RO_21f", 15, [(4, 5)], 0, (16, 32, 0, 0), (9, 0, 0, 0), (2, 1, F), env=_GENERIC),   # k16 n32
    Row("RO_21t", 15, [(4, 5)], 7, (16, 32, 0, 0), (9, 0, 0, 1), (2, 1, T), env=_GENERIC),   # k16 n32
    Row("RO_22f", 15, [(4, 6)], 0, (16, 64, 0, 0), (8, 0, 0, 0), (2, 2, F), env=_GENERIC),   # k16 n64
    Row("RO_22t", 15, [(4, 6)], 7, (16, 64, 0, 0), (8, 0, 0, 1), (2, 2, T), env=_GENERIC),   # k16 n64
    Row("RO_24f", 15, [(4, 7)], 0, (16, 128, 0, 0), (7, 0, 0, 0), (2, 4, F), env=_GENERIC),   # k16 n128
    Row("RO_24t", 15, [(4, 7)], 7, (16, 128, 0, 0), (7, 0, 0, 1), (2, 4, T), env=_GENERIC),   # k16 n128
    Row("RZ_ft11f", 15, [(6, 5), (6, 4)], 0, (64, 32, 64, 16), (8, 4, 1, 0), (F, T, 1, 1, F)),   # k64 n32 | k64 n16: 4 items
    Row("RZ_tf11t", 15, [(7, 4), (5, 5)], 3, (128, 16, 32, 32), (8, 4, 1, 1), (T, F, 1, 1, T)),   # k128 n16 | k32 n32: 4 items
    Row("RZ_tt21f", 15, [(4, 4), (6, 4)], 0, (16, 16, 64, 16), (9, 4, 1, 0), (T, T, 2, 1, F)),   # k16 n16 | k64 n16: 4 items
    Row("RZ_ft14t", 15, [(5, 7), (6, 4)], 2, (32, 128, 64, 16), (6, 4, 1, 1), (F, T, 1, 4, T)),   # k32 n128 | k64 n16: 4 items
]

# Entries of the run-time-count dispatch that no planned stem takes (stems of seeds 0..40 searched: 26 of the 32 pair
# entries and all 12 single-step entries are reached).  Two units per wave (RT1 = 2) with more than one column group in
# step 1 is a tile of 2^14 intermediate elements -- 256 rows x 64 columns, or 128 rows x 128 columns.  stem.geometry
# takes it only where the smaller tile gives step 2 fewer items, and then checks the LDS: two planes of the
# intermediate (at least 132 KB with their padding), B1 and B2 must fit 160 KB.  They do for K1 = 16, N1 = 64, K2 = 64,
# N2 = 16 alone (RP_ft22f, RP_ft22t); with 32 or more columns in step 2, or with 128 columns in step 1, no K1, K2, N2
# fits (tests/test_stem_variant_plans.py enumerates them with stem.geometry's own formula).
_NO_LDS = "stem.geometry: the 2^14-element intermediate, B1 and B2 exceed the 160 KB of LDS for every K1, K2, N2"
UNREACHABLE = [((F, p2, 2, cs1, vec), _NO_LDS) for p2, cs1 in ((F, 2), (F, 4), (T, 4)) for vec in (F, T)]

# The 26 specialised-wave geometries that run in 16 bits, again in the symmetric form (fp16 x 2 under CTG_STEM_FORM=1)
FORM1_ROWS = [r.like(r.id + "_sym", env={"CTG_STEM_FORM": "1"}) for r in GEO_ROWS if r.forms[1] == 3 and r.fits16]
for _r in FORM1_ROWS:
    _r.base = _r.id[:-4]


def _variant(base, ident, arith, **kw):
    r = base.like(ident, **kw)
    r.base, r.arith = base.id, arith
    return r


def _by(rows, ident):
    return next(r for r in rows if r.id == ident)


# One index of the first tensor sliced (nq + 1: a slice has the row's size), one row per kernel family; the seed is the
# first with which the sliced stem keeps the shape
SLICED_ROWS = [
    _variant(_by(INST_ROWS, "I01"), "I01_z", "fp32", nq=16, seed=1, sliced=1),      # fp32, step 2 row-interleaved
    _variant(_by(INST_ROWS, "I02"), "I02_z", "fp32", nq=16, seed=1, sliced=1),      # fp32, X / Y form
    _variant(_by(GEO_ROWS, "G02"), "G02_z", "fp16x2", nq=16, seed=1, sliced=1),     # form 3
    _variant(_by(GEO_ROWS, "G04"), "G04_z", "bf16x3", nq=16, seed=1, sliced=1),     # form 1
    _variant(_by(GEO_ROWS, "G05"), "G05_z", "fp16x2", nq=16, seed=1, sliced=1),     # form 0
    _variant(_by(ONE_ROWS, "O02"), "O02_z", "fp16x2", nq=16, seed=1, sliced=1),     # a single step
]
for _r, _f in zip(SLICED_ROWS, ("inst_ri2", "inst_xy", "form3", "form1", "form0", "single")):
    _r.family = _f


# More than one tile per workgroup (a launch has min(tiles, 256) workgroups): 512 and 1024 tiles, the loop structures
# that tests/test_gpu_stem_mempath.py (specialised waves with one and two column groups, PACK1, PACK2, a static
# single step) and tests/test_gpu_stem_shared_rows.py (specialised waves and the symmetric fp16 x 2 form under
# CTG_STEM_FORM=1, up to 1024 tiles) do not run.  In each class the row with the smallest tile: the running tensor
# stays at or below 2^23 elements -- which leaves the pairs with NCH = 8 out (a tile of 2^15 elements: 512 tiles
# are 2^24), so B1 from LDS runs on the single steps O01 (fp32, K = N = 128) and O10 (16 bits, 512 tiles only).
def _deep(base, what, arith, per_tiles, **kw):
    out = []
    for tiles, (nq, seed) in per_tiles.items():
        r = _variant(base, f"D_{what}_{arith}_{tiles}", arith, nq=nq, seed=seed, **kw)
        r.tiles = tiles
        out.append(r)
    return out


DEEP_ROWS = (
    # form 0 (four items per wave) in both 16-bit arithmetics
    _deep(_by(GEO_ROWS, "G38"), "form0", "bf16x3", {512: (21, 0), 1024: (22, 0)})
    + _deep(_by(GEO_ROWS, "G38"), "form0", "fp16x2", {512: (21, 0), 1024: (22, 0)})
    # run-time counts: a pair and a single step
    + _deep(_by(GENERIC_ROWS, "RP_ff12f"), "generic_pair", "fp32", {512: (20, 0), 1024: (21, 0)})
    + _deep(_by(GENERIC_ROWS, "RO_14f"), "generic_one", "fp32", {512: (20, 0), 1024: (21, 0)})
    # NCH = 8: B1's fragments from LDS
    + _deep(_by(ONE_ROWS, "O01"), "nch8", "fp32", {512: (22, 0), 1024: (23, 0)})
    + _deep(_by(ONE_ROWS, "O10"), "nch8", "fp16x2", {512: (23, 0)})
    # 16-byte gathers in 16 bits (the symmetric form: two items of 32 columns per wave)
    + _deep(_by(GEO_ROWS, "G35"), "vec", "bf16x3", {512: (21, 2), 1024: (22, 2)})
    + _deep(_by(GEO_ROWS, "G35"), "vec", "fp16x2", {512: (21, 2), 1024: (22, 2)})
    # four column groups in step 1 (fp32 products: the 16-bit instantiation of this geometry never fits, G26)
    + _deep(_by(INST_ROWS, "I34"), "cs4", "fp32", {512: (21, 1), 1024: (22, 7)})
)

INST_ARGS = {r.args for r in INST_ROWS}
GEO_ARGS = {r.args for r in GEO_ROWS}
ONE_ARGS = {r.args for r in ONE_ROWS}

ALL_ROWS = INST_ROWS + GEO_ROWS + FORM1_ROWS + ONE_ROWS + GENERIC_ROWS + SLICED_ROWS + DEEP_ROWS

# (row, arithmetic) of the per-row device test; rows of one network follow each other (their data is computed once)
DEVICE_CASES = sorted(
    [(r, "fp32") for r in INST_ROWS + GENERIC_ROWS]
    + [(r, a) for r in GEO_ROWS for a in ("bf16x3", "fp16x2")]
    + [(r, "fp16x2") for r in FORM1_ROWS]
    + [(r, a) for r in ONE_ROWS for a in ARITHS],
    key=lambda ra: ra[0].network)


def by_id(ident):
    return _by(ALL_ROWS, ident)
