"""Range audit: what the exponent histograms of ``Executor.range_audit`` say about a contraction's tensors.

Pure numpy -- nothing here touches the device.  The fp16 x 2 arithmetic rounds an operand
to two fp16 limbs under ONE power of two per tensor: its absolute error is at most 2^-24 of the tensor's largest
element, so relative to the tensor's norm it is ``2^-24 * max / rms`` -- fp32's own 2^-24 times the crest factor.
:func:`summarise` turns one row of the audit into that figure, :func:`join_operands` says which rows are the
operands of which plan step, :func:`step_records` puts both together and :func:`auto_choice` is the rule of
``HipContractor(stem_bf16x3="auto", crest_limit=L)``.
"""

from __future__ import annotations

import math

import numpy as np

RANGE_WORDS = 260
SPACE_INPUTS, SPACE_ARENA = 0, 1

# kernels that multiply under one power of two per operand tensor, and the operands they scale that way
SCALED_OPERANDS = (("stem2h_kernel", ("a", "b", "b2")), ("pair_mfma_h2_kernel", ("a", "b")))


class RangeSummary:
    """One tensor's row (or, from :meth:`worst`, the same tensor in several slices: the worst value per field).

    ``n`` components, ``zeros`` equal to +-0, ``nonfinite`` inf or NaN; ``top`` the highest non-empty exponent
    bin below 255 (-1: none; 0 for a tensor of zeros); ``rms = sqrt(sumsq / n)``; ``crest_up = 2^(top - 126) / rms``, the upper edge of
    the top binade over the rms -- at least the crest factor ``max / rms`` and less than twice it, and the
    quantity fp16 x 2 works with, its scale being a power of two (``inf`` for a tensor without a finite non-zero
    component); ``eps_h2 = 2^-24 crest_up``, the norm-wise representation error of the tensor under one scale
    (fp32 itself: 2^-24); ``below(g)`` the fraction of the non-zero finite components more than ``g`` binades
    under ``top``."""

    def __init__(self, row, sumsq):
        row = np.asarray(row, dtype=np.int64).reshape(-1)
        if row.size != RANGE_WORDS:
            raise ValueError(f"a range row has {RANGE_WORDS} words, got {row.size}")
        self.n = int(row[1])
        self.zeros = int(row[2])
        self.hist = row[4:].copy()
        self.nonfinite = int(self.hist[255])
        self.sumsq = float(sumsq)
        filled = np.flatnonzero(self.hist[:255])
        self.top = int(filled[-1]) if filled.size else -1
        self.rms = math.sqrt(self.sumsq / self.n) if self.n > 0 and self.sumsq >= 0.0 else float("nan")
        if self.top >= 0 and self.rms > 0.0 and math.isfinite(self.rms):
            self.crest_up = math.ldexp(1.0, self.top - 126) / self.rms
        else:
            self.crest_up = float("inf")
        self.eps_h2 = math.ldexp(self.crest_up, -24)
        self._parts = (self,)

    def _below_one(self, g):
        nonzero = self.n - self.zeros - self.nonfinite
        if nonzero <= 0 or self.top < 0:
            return 0.0
        cut = self.top - int(g)   # bins below `cut` are more than g binades under top
        if cut <= 0:
            return 0.0
        return float(int(self.hist[:cut].sum()) - self.zeros) / nonzero

    def below(self, g):
        return max(p._below_one(g) for p in self._parts)

    @classmethod
    def worst(cls, parts):
        """The same tensor in several slices: per field the value that speaks most against one scale."""
        parts = [p for p in parts if p is not None]
        if not parts:
            return None
        if len(parts) == 1:
            return parts[0]
        out = cls.__new__(cls)
        out._parts = tuple(q for p in parts for q in p._parts)
        out.n = max(p.n for p in parts)
        out.zeros = max(p.zeros for p in parts)
        out.nonfinite = max(p.nonfinite for p in parts)
        out.top = max(p.top for p in parts)
        out.sumsq = min(p.sumsq for p in parts)
        rms = [p.rms for p in parts]
        out.rms = float("nan") if any(math.isnan(r) for r in rms) else min(rms)
        out.crest_up = max(p.crest_up for p in parts)
        out.eps_h2 = max(p.eps_h2 for p in parts)
        out.hist = np.max([p.hist for p in parts], axis=0)
        return out

    def as_dict(self, g=14):
        return {"n": self.n, "zeros": self.zeros, "nonfinite": self.nonfinite, "top": self.top, "rms": self.rms,
                "crest_up": self.crest_up, "eps_h2": self.eps_h2, f"below({g})": self.below(g)}

    def __repr__(self):
        return (f"RangeSummary(n={self.n}, zeros={self.zeros}, nonfinite={self.nonfinite}, top={self.top}, "
                f"rms={self.rms:.3e}, crest_up={self.crest_up:.3e})")


def summarise(row, sumsq):
    """:class:`RangeSummary` of one audited row (status word 1); ``None`` for a row that was not materialised."""
    row = np.asarray(row).reshape(-1)
    if row.size != RANGE_WORDS:
        raise ValueError(f"a range row has {RANGE_WORDS} words, got {row.size}")
    if int(row[0]) != 1:
        return None
    return RangeSummary(row, sumsq)


def join_operands(plan):
    """Per plan step ``{"a": row, "b": row, "b2": row, "c": row}``: the rows of ``Executor.range_audit`` that
    describe the step's operands and its result (``None``: no such operand).  An operand in the inputs space is
    the leaf's row; one in the arena is the row of its producer -- ``Step.a_prod`` / ``b_prod`` / ``b2_prod``,
    or, for the result of a preprocessing step (which those do not name), the last earlier step that wrote the
    operand's arena offset."""
    n_in = len(plan.input_sizes)
    steps = list(plan.steps)

    def row_of(s, ref, prod):
        if ref is None:
            return None
        if prod is not None and prod >= 0:
            return n_in + int(prod)
        if ref.space == SPACE_INPUTS:
            return int(ref.leaf) if ref.leaf is not None and ref.leaf >= 0 else None
        if ref.space == SPACE_ARENA:
            for t in range(s - 1, -1, -1):
                c = steps[t].c
                if c is not None and c.space == SPACE_ARENA and c.offset == ref.offset:
                    return n_in + t
        return None

    out = []
    for s, st in enumerate(steps):
        out.append({
            "a": row_of(s, st.a, getattr(st, "a_prod", -1)),
            "b": row_of(s, st.b, getattr(st, "b_prod", -1)),
            "b2": row_of(s, getattr(st, "b2", None), getattr(st, "b2_prod", -1)),
            "c": n_in + s,
        })
    return out


def scaled_operands(kernel_name):
    """Which operands of a step named ``kernel_name`` (``Executor.step_kernels``) run under a per-tensor scale."""
    for prefix, ops in SCALED_OPERANDS:
        if kernel_name.startswith(prefix):
            return ops
    return ()


def step_records(plan, names, audits):
    """One record per plan step from ``names`` (``step_kernels()``) and ``audits``, a list of ``(rows, sumsq)``
    -- one per audited slice: ``{"step", "kernel", "a", "b", "b2", "c", "operands", "scaled", "kappa"}`` with a
    :class:`RangeSummary` (or ``None``) per tensor, ``scaled`` the operands that run under a per-tensor scale
    and ``kappa = |A| |B| (|B2|) / |C|`` in Frobenius norms: at least 1, how far the step cancels and so how far
    it amplifies its operands' norm-wise errors (``None`` where a tensor was not audited, ``inf`` for a zero
    result).  With several slices every tensor and ``kappa`` take the worst value per field."""
    joins = join_operands(plan)
    records = []
    for s, j in enumerate(joins):
        rec = {"step": s, "kernel": names[s] if s < len(names) else "", "kappa": None}
        per_slice = {k: [] for k in ("a", "b", "b2", "c")}
        kappas = []
        for rows, sumsq in audits:
            rows = np.asarray(rows).reshape(-1, RANGE_WORDS)
            here = {}
            for k in ("a", "b", "b2", "c"):
                t = j[k]
                here[k] = summarise(rows[t], sumsq[t]) if t is not None else None
                per_slice[k].append(here[k])
            ops = [here[k] for k in ("a", "b", "b2") if j[k] is not None]
            if here["c"] is not None and ops and all(o is not None for o in ops):
                num = math.prod(math.sqrt(o.sumsq) for o in ops)
                den = math.sqrt(here["c"].sumsq)
                kappas.append(num / den if den > 0.0 else float("inf"))
        for k in ("a", "b", "b2", "c"):
            rec[k] = RangeSummary.worst(per_slice[k])
        rec["operands"] = tuple(k for k in ("a", "b", "b2") if j[k] is not None)
        rec["scaled"] = tuple(k for k in scaled_operands(rec["kernel"]) if j[k] is not None)
        if kappas:
            rec["kappa"] = max(kappas)
        records.append(rec)
    return records


def auto_choice(h2_names, records, crest_limit):
    """The rule of ``stem_bf16x3="auto"``: ``"fp16x2"`` if every tensor that fp16 x 2 would scale per tensor --
    the operands named by :func:`scaled_operands` of the step names ``h2_names`` read under ``"fp16x2"`` -- has
    ``crest_up <= crest_limit`` and no non-finite component; else ``"bf16x3"``.  A scaled operand that was not
    audited (a member of an LDS-resident subtree) speaks against: nothing is known about it."""
    for s, name in enumerate(h2_names):
        for k in scaled_operands(name):
            if k not in records[s]["operands"]:
                continue   # (a step without a second small operand)
            t = records[s].get(k)
            if t is None:
                return "bf16x3"
            if t.nonfinite or not t.crest_up <= crest_limit:
                return "bf16x3"
    return "fp16x2"


def format_table(records, g=14):
    """The per-step table ``tools/range_audit.py`` prints."""
    lines = [f"{'step':>4}  {'kernel':<44} {'scaled':<7} {'crest_up A':>10} {'B':>9} {'B2':>9} {'C':>9} "
             f"{'below' + str(g) + ' A':>9} {'kappa':>9}"]

    def f(t, attr="crest_up"):
        return f"{getattr(t, attr):9.3g}" if t is not None else f"{'-':>9}"

    for r in records:
        b14 = f"{r['a'].below(g):9.2e}" if r["a"] is not None else f"{'-':>9}"
        kap = f"{r['kappa']:9.3g}" if r["kappa"] is not None else f"{'-':>9}"
        lines.append(f"{r['step']:>4}  {r['kernel'][:44]:<44} {','.join(r['scaled']):<7} {f(r['a']):>10} {f(r['b'])} "
                     f"{f(r['b2'])} {f(r['c'])} {b14} {kap}")
    return "\n".join(lines)
