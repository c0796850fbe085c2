"""The fp32 gather family (acm_gather_device.h) over the chooser's table: the operators, the table layouts, the cases -- each with
the form it was built to reach written next to it --, the two references and the runners (tests/test_gather_forms_cpu.py asks the
real acm_gather_form for every case on fabricated addresses; tests/test_gpu_gather_forms.py runs every case through
acm_conv_bwd_spmm or acm_spmm_ex).  Importable without a GPU; every runner takes the device it works on.

The references.  EXACT: operator values and tables are integers in [-8, 8], scales are powers of two, so every partial sum of a
row (the longest has 1398 entries) stays below 1400 * 64 < 2^24 and every fp32 operation is exact in any order: the output must be
bit-equal to the integer result.  BOUNDED: N(0, 1) tables against float64 under the a-priori bound of fp32 summation in any
order.  A row of L stored entries is a sum of L products through at most L roundings (each fmaf rounds once; the adds of a
lane-group reduction, of the LDS meeting and of a fix-up replace adds of the serial chain), and the epilogue adds at most four
(self_scale * s_high, the subtraction, s_struc * inv_deg, its subtraction; row_scale * sum, sub_scale * sub and the subtraction
for acm_spmm_ex), so with u = 2^-24 and n = L + 4
    |got - ref| <= n u / (1 - n u) * (sum |a g| + |self term|)            element by element
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Derived, not measured."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import scipy.sparse as sp
import torch

import bf16_ref as R
import launch_forms as LF

U = 2.0 ** -24
NARROW_WIDTHS = tuple(range(1, 9))
ROUNDING_WIDTHS = (9, 32, 33, 34, 50, 62, 64, 65, 66, 128, 129, 130, 192, 193, 196, 256)
MULTIPLES_OF_4 = tuple(range(12, 257, 4))
EVEN_PAIR_WIDTHS = tuple(range(34, 65, 2))
K4_OPTIONS = ((1, 1, 1), (0, 0, 0), (0, 1, 0), (1, 0, 1))          # (masks, self_scale, inv_deg)


# ---- the operators ----
def dense_operator():
    """190 x 200 at density 0.9 with chunk 64: more than 160 entries per row and per column (32 lanes per item for the operator
    and its transpose), every non-empty row a long row of three pieces; rows 5 and 100 are empty, columns 0 and 199 are never
    referenced."""
    n, m = LF.GATHER_DENSE_SHAPE
    rng = np.random.default_rng(7)
    mask = rng.random((n, m)) < 0.9
    mask[:, [0, m - 1]] = False
    mask[[5, 100], :] = False
    pat = sp.csr_matrix(mask)
    pat.sort_indices()
    op = R.Operator("dense", pat.indptr, pat.indices, R._random_values(rng, pat.nnz), m, 64)
    assert set(op.dead) == {0, m - 1} and (op.lengths == 0).sum() == 2
    return op


def big_operator(name, mean):
    """300 x 16 500 with chunk 64: row lengths 1 .. 2 mean - 1, one row of 1100 entries, rows 3 and 299 empty; columns 0, 7777 and
    16 499 are never referenced."""
    n, m = LF.GATHER_BIG_ROWS, LF.GATHER_BIG_COLS
    rng = np.random.default_rng(8 + mean)
    lens = rng.integers(1, 2 * mean, n)
    lens[[3, n - 1]] = 0
    lens[17] = 1100
    live = np.setdiff1d(np.arange(m), [0, 7777, m - 1])
    indices = np.concatenate([np.sort(rng.choice(live, int(k), replace=False)) for k in lens])
    op = R.Operator(name, np.concatenate([[0], np.cumsum(lens)]), indices, R._random_values(rng, len(indices)), m, 64)
    assert set(op.dead) >= {0, 7777, m - 1}
    return op


def two_more_rows(op):
    """``op`` with two empty rows appended: empty rows for the operator, two table rows nobody references for its transpose."""
    return R.Operator(op.name, np.concatenate([op.indptr, op.indptr[-1:], op.indptr[-1:]]), op.indices, op.vals, op.n_cols, op.chunk)


_OPS = {}


def operators():
    """name -> Operator: bf16_ref's ladder and hub with two empty rows appended, the dense operator and the two large ones, each
    with explicit and with pattern-only values, itself and transposed; and ladder-whole."""
    if not _OPS:
        _OPS["ladder-whole"] = two_more_rows(R.ladder_operator(256, "ladder-whole"))
        for base in (two_more_rows(R.ladder_operator()), two_more_rows(R.hub_operator()), dense_operator(),
                     big_operator("big48", LF.GATHER_BIG_MEANS[0]), big_operator("big20", LF.GATHER_BIG_MEANS[1])):
            for op in (base, base.unit()):
                _OPS[op.name] = op
                t = op.transposed()
                _OPS[t.name] = t
    return _OPS


def _four(base):
    return (base, base + "-unit", base + "-T", base + "-unit-T")


# What the cases expect of an operator, WRITTEN here and checked against the operator in test_gather_forms_cpu.py: lanes per work
# item of the narrow gather, the fix-up after a narrow gather and after a wide one, whether the mean row length reaches 16 (the
# vector form's bar with one gathered channel; every operator that runs a wide family reaches the 4 of several channels).
OPERATOR_FORMS = {}
for _nm in _four("ladder"):
    OPERATOR_FORMS[_nm] = (8, "narrow", "wide", False)
OPERATOR_FORMS["ladder-whole"] = (8, "none", "none", False)                # chunk 256: no long row
for _nm in _four("hub"):
    OPERATOR_FORMS[_nm] = (16, "windows", "wide", True)                     # the hub row takes three windows
for _nm in _four("dense"):
    OPERATOR_FORMS[_nm] = (32, "narrow", "wide", True)
for _nm in ("big48", "big48-unit", "big20", "big20-unit"):
    OPERATOR_FORMS[_nm] = (16, "none", "wide", True)                        # long rows of one window each: the gather finishes them
for _nm in ("big48-T", "big48-unit-T", "big20-T", "big20-unit-T"):
    OPERATOR_FORMS[_nm] = (8, "none", "none", False)                        # 16 500 short rows
SMALL_OPS = _four("ladder") + ("ladder-whole",) + _four("hub") + _four("dense")
BIG_OPS = ("big48", "big48-unit", "big20", "big20-unit")
BIG_T_OPS = ("big48-T", "big20-unit-T")


def n_multi(op):
    """Rows that take several windows of pieces (acm_items.h, build_items): more than sixteen pieces and more than 64 x chunk."""
    deg = op.lengths.astype(np.int64)
    return int(((deg > 16 * op.chunk) & ((deg + 15) // 16 > 4 * op.chunk)).sum())


def n_long(op):
    return int((op.lengths > op.chunk).sum())


def int_twin(op):
    """The same pattern with values in +-{1 .. 8} (a pattern-only operator is its own twin: its values are ones)."""
    if op.vals is None:
        return op
    rng = np.random.default_rng(zlib.crc32(op.name.encode()))
    v = rng.integers(1, 9, len(op.indices)) * rng.choice([-1, 1], len(op.indices))
    return R.Operator(op.name + "-int", op.indptr, op.indices, v.astype(np.float32), op.n_cols, op.chunk)


_HANDLES = {}


def handle_of(op, dev):
    key = (op.name, str(dev))
    if key not in _HANDLES:
        g = op.handle(dev)
        op.check_shape(g)
        _HANDLES[key] = g
    return _HANDLES[key]


# ---- table layouts ----
class Layout:
    """Where the gathered channels lie: ``bufs`` = [(floats in front of the first row, pitch)] -- one allocation each --,
    ``chan`` = [(buffer, first column)] per channel."""

    def __init__(self, name, bufs, chan):
        self.name, self.bufs, self.chan = name, list(bufs), list(chan)

    def pitch(self, c):
        return self.bufs[self.chan[c][0]][1]

    def offset(self, c):
        """floats between the allocation's start and channel c of table row 0"""
        b, col = self.chan[c]
        return self.bufs[b][0] + col


def sep(name, ng, ld, off=0):
    """every channel in a table of its own, pitch ``ld``, ``off`` floats into its buffer"""
    return Layout(name, [(off, ld)] * ng, [(c, 0) for c in range(ng)])


def each(name, specs):
    """a table of its own per channel: [(off, ld)]"""
    return Layout(name, specs, [(c, 0) for c in range(len(specs))])


def adj(name, ng, w, ld, off=0, third=None, gap=0):
    """channels 0 and 1 in one table at columns 0 and w + gap; channel 2 in its own ``third`` = (off, ld)"""
    lay = Layout(name, [(off, ld)], [(0, 0), (0, w + gap)])
    if ng == 3:
        lay.bufs.append(third)
        lay.chan.append((1, 0))
    return lay


# ---- the cases ----
class Case:
    """One call.  ``api``: "k4" (acm_conv_bwd_spmm: ng = 2, or 3 with the structure channel) or "spmm" (acm_spmm_ex: ng = 1).
    ``opts``: K4's (masks, self_scale, inv_deg), or for spmm 1 = row_scale + sub + sub_scale + relu.  ``tune``: wide_form /
    bwd_split.  ``expect``: the form the case was built to reach -- kind, f_arg, and for NARROW vecmask and merged; ``split``:
    None (K4 keeps all channels in one pass) or the reason it splits ("auto" / "forced"), and then ``expect`` describes every
    single-channel pass."""

    def __init__(self, family, f, ng, layout, expect, tune=None, opts=0, split=None, why=""):
        self.family, self.f, self.ng, self.layout, self.expect = family, f, ng, layout, dict(expect)
        self.tune, self.opts, self.split, self.why = dict(tune or {}), opts, split, why
        self.api = "spmm" if ng == 1 else "k4"
        assert len(layout.chan) == ng

    @property
    def id(self):
        t = "".join(f"-{k[0]}{v}" for k, v in sorted(self.tune.items()))
        return f"{self.api}-F{self.f}-ng{self.ng}-{self.layout.name}{t}-o{self.opts}"


def fp_of(f):
    return 2 if f <= 2 else (4 if f <= 4 else 8)


def _narrow_cases():
    """F = 1 .. 8.  The padded row is FP = 2 / 4 / 8 columns; a channel takes the vector fetch (its vecmask bit) when its rows
    are 8-byte (FP = 2) or 16-byte aligned and its pitch is at least FP."""
    out, k = [], 0
    for f in NARROW_WIDTHS:
        fp = fp_of(f)
        for ng in (1, 2, 3):
            full = (1 << ng) - 1
            lays = [(sep("aligned", ng, fp), full, 0, "pitch padded to FP, aligned base"),
                    (sep("pad2", ng, 2 * fp), full, 0, "a wider pitch, still a multiple of the block"),
                    (sep("odd", ng, fp + 1), 0, 0, "odd pitch: no channel's rows are aligned"),
                    (sep("off4", ng, fp, off=1), 0, 0, "a base 4 bytes in"),
                    (sep("off8", ng, fp, off=2), full if fp == 2 else 0, 0, "a base 8 bytes in: aligned for FP = 2 alone")]
            if f < fp:
                lays.append((sep("tight", ng, f), 0, 0, "F < FP at pitch F: the block fetch would run into the next row"))
            if ng >= 2:
                third = (0, fp)
                mixed = [(0, fp), (1, fp), (0, fp)][:ng]
                lays += [(each("mixed", mixed), 0b101 & full, 0, "channel 1 alone 4 bytes in"),
                         (adj("merged", ng, fp, 2 * fp, third=third), full, 1, "[c0 | c1] adjacent, block-aligned: one fetch"),
                         (adj("merged-pad", ng, fp, 4 * fp, third=(1, fp)), 0b011, 1, "the same at twice the pitch; channel 2 unaligned"),
                         (adj("apart", ng, fp, 4 * fp, third=third, gap=fp), full, 0, "one table, but a gap between the channels"),
                         (adj("adj-off8", ng, fp, 2 * fp, off=2, third=third), (0b111 if fp == 2 else 0b100) & full, 0,
                          "adjacent, 8 bytes in: not block-aligned")]
            for lay, vecmask, merged, why in lays:
                out.append(Case("narrow", f, ng, lay, dict(kind="NARROW", f_arg=fp, vecmask=vecmask, merged=merged),
                                tune=dict(bwd_split=(0, 1, -1)[k % 3]), opts=K4_OPTIONS[k % 4] if ng > 1 else k % 2, why=why))
                k += 1
    return out


PAIR3 = Layout("pair3", [(0, 8)], [(0, 0), (0, 2), (0, 4)])
PAIR3_OFF16 = Layout("pair3-off16", [(4, 8)], [(0, 0), (0, 2), (0, 4)])


def _pair3_cases():
    """F = 2 with the structure channel in packed 32-byte rows [c0 c0 c1 c1 | c2 c2 - -]: the pair-lane kernel with sixteen lanes
    per item; the merged narrow kernel with 8 or 32 lanes, and with the rows 16 bytes off the 32-byte grid."""
    out = []
    for k, opts in enumerate(K4_OPTIONS):
        out.append(Case("pair3", 2, 3, PAIR3, dict(kind="PAIR3", f_arg=2, vecmask=7, merged=0, kind_other_lanes="NARROW", merged_other_lanes=1),
                        tune=dict(bwd_split=(0, 1, -1)[k % 3]), opts=opts, why="packed rows"))
    out.append(Case("pair3", 2, 3, PAIR3_OFF16, dict(kind="NARROW", f_arg=2, vecmask=7, merged=1), opts=K4_OPTIONS[0],
                    why="packed rows 16 bytes in: off the 32-byte grid of the pair-lane kernel; [c0 | c1] is still a 16-byte block"))
    return out


def _wide_layouts(f, ng, quantum):
    """aligned layouts of a wide table, rotated by the caller: contiguous, pitch padded by ``quantum`` floats, base ``quantum``
    floats in, [c0 | c1] adjacent in one table"""
    lays = [sep("contig", ng, f), sep(f"pad{quantum}", ng, f + quantum), sep(f"off{4 * quantum}", ng, f + quantum, off=quantum)]
    if ng >= 2:
        lays.append(adj("adjacent", ng, f, 2 * f + quantum, third=(0, f)))
    return lays


def _vec_cases(widths=tuple(f for f in MULTIPLES_OF_4 if f <= 128), family="vec"):
    """wide_form = 2, every multiple of 4 from 12 to 256 (family "vec" up to 128 columns, "vec-hi" beyond): spmm_vec_kernel<NG,
    NB = 1 .. 4> on 16-byte aligned rows."""
    out, k = [], 0
    for f in widths:
        for ng in (1, 2, 3):
            lays = _wide_layouts(f, ng, 4)
            lay = lays[k % len(lays)]
            split = (0, 1, 0, -1)[k % 4] if ng > 1 else -1
            out.append(Case(family, f, ng, lay, dict(kind="VEC", f_arg=(f + 63) // 64), tune=dict(wide_form=2, bwd_split=split),
                            opts=K4_OPTIONS[k % 4] if ng > 1 else k % 2, split="forced" if split == 1 else None))
            k += 1
    return out


def _wide_cases():
    """wide_form = 1: spmm_wide_kernel<NREG = 1 / 2 / 4> -- except on even 34 .. 64 columns with 8-byte aligned rows, where the
    pair form stays (family "pair"); those widths come here with rows that are not."""
    out, k = [], 0
    widths = sorted(set(ROUNDING_WIDTHS) | {10, 12, 16, 31, 35, 63, 127, 191, 255})
    for f in widths:
        pairable = 32 < f <= 64 and f % 2 == 0
        for ng in (1, 2, 3):
            lays = [sep("odd", ng, f + 1 + f % 2), sep("off4", ng, f + 2, off=1)]
            if not pairable:
                lays += [sep("contig", ng, f), sep("off8", ng, f + 4, off=2)] + ([adj("adjacent", ng, f, 2 * f, third=(0, f))] if ng > 1 else [])
            lay = lays[k % len(lays)]
            split = (0, 1, 0, -1)[k % 4] if ng > 1 else -1
            out.append(Case("wide", f, ng, lay, dict(kind="WIDE", f_arg=1 if f <= 64 else (2 if f <= 128 else 4)),
                            tune=dict(wide_form=1, bwd_split=split), opts=K4_OPTIONS[k % 4] if ng > 1 else k % 2,
                            split="forced" if split == 1 else None))
            k += 1
    return out


def _pair_cases():
    """Every even width 34 .. 64 with the vector form off (wide_form = 1), and the multiples of 4 among them with the pair form
    kept (3): spmm_pair_kernel<NG, Epi, false> on 8-byte aligned rows."""
    out, k = [], 0
    for f in EVEN_PAIR_WIDTHS:
        for ng in (1, 2, 3):
            for form in (1, 3) if f % 4 == 0 else (1,):
                lays = _wide_layouts(f, ng, 2)
                lay = lays[k % len(lays)]
                split = (0, 1, 0, -1)[k % 4] if ng > 1 else -1
                out.append(Case("pair", f, ng, lay, dict(kind="PAIR_F32", f_arg=0), tune=dict(wide_form=form, bwd_split=split),
                                opts=K4_OPTIONS[k % 4] if ng > 1 else k % 2, split="forced" if split == 1 else None))
                k += 1
    return out


def _default_cases():
    """wide_form = 0, bwd_split = -1 on the small operators (their tables fit the L2 at every width), the form the documented
    rule gives, per class of operator (mean row length below 16: ladder; 16 and more: hub, dense):
      VEC        F % 4 == 0 on 16-byte aligned rows with a pitch of 4 k -- with one channel only from a mean row length of 16
      PAIR_F32   else even 32 < F <= 64 on 8-byte aligned rows with an even pitch
      WIDE       else.
    ``expect`` holds the kind for rows of 16 and more (kind) and for shorter rows (kind_short)."""
    out, k = [], 0
    for f in ROUNDING_WIDTHS:
        pairable = 32 < f <= 64 and f % 2 == 0
        nreg = 1 if f <= 64 else (2 if f <= 128 else 4)
        nb = (f + 63) // 64
        for ng in (1, 2, 3):
            lays = [("contig", sep("contig", ng, f), f % 4 == 0, pairable),
                    ("odd", sep("odd", ng, f + 1 + f % 2), False, False),
                    ("off4", sep("off4", ng, f + 4 - f % 4, off=1), False, False),
                    ("off8", sep("off8", ng, f + 4 - f % 4, off=2), False, pairable)]
            for _, lay, vec, pair in lays:
                long_rows = "VEC" if vec else ("PAIR_F32" if pair else "WIDE")
                short_rows = long_rows if ng > 1 or not vec else ("PAIR_F32" if pair else "WIDE")
                f_arg = {"VEC": nb, "PAIR_F32": 0, "WIDE": nreg}
                out.append(Case("default", f, ng, lay, dict(kind=long_rows, f_arg=f_arg[long_rows], kind_short=short_rows,
                                                            f_arg_short=f_arg[short_rows]),
                                tune=dict(wide_form=0, bwd_split=-1), opts=K4_OPTIONS[k % 4] if ng > 1 else k % 2))
                k += 1
    return out


def _big_cases():
    """The operators with 16 500 table rows.  ``only``: the operators a case is for (big48: mean row length 48; big20: 20)."""
    c = []

    def add(f, ng, lay, expect, tune, opts, split=None, only=None, why=""):
        case = Case("big", f, ng, lay, expect, tune=tune, opts=opts, split=split, why=why)
        case.only = only
        c.append(case)

    dflt = dict(wide_form=0, bwd_split=-1)
    add(64, 2, adj("adjacent", 2, 64, 128), dict(kind="WIDE", f_arg=1), dflt, K4_OPTIONS[0],
        why="two channels of 64 columns exceed 8 MiB: neither the vector nor the pair form, by the table size alone")
    add(64, 3, sep("contig", 3, 64), dict(kind="WIDE", f_arg=1), dflt, K4_OPTIONS[3], why="three channels of 64 columns")
    add(32, 2, adj("adjacent", 2, 32, 64), dict(kind="VEC", f_arg=1), dflt, K4_OPTIONS[1], why="two channels of 32 columns fit")
    add(64, 1, sep("contig", 1, 64), dict(kind="VEC", f_arg=1), dflt, 1, why="one channel of 64 columns stays resident")
    add(50, 1, sep("contig", 1, 50), dict(kind="PAIR_F32", f_arg=0), dflt, 0, why="one channel of 50 columns: the pair form")
    add(128, 2, adj("adjacent", 2, 128, 256), dict(kind="VEC", f_arg=2), dflt, K4_OPTIONS[0], split="auto", only="big48",
        why="a channel of 128 columns exceeds 8 MiB at a mean row length of 32 and more: one channel per pass")
    add(128, 3, sep("contig", 3, 128), dict(kind="VEC", f_arg=2), dflt, K4_OPTIONS[2], split="auto", only="big48",
        why="the same with the structure channel")
    add(128, 2, adj("adjacent", 2, 128, 256), dict(kind="WIDE", f_arg=2), dflt, K4_OPTIONS[0], only="big20",
        why="the same tables at a mean row length below 32: one pass, beyond the L2")
    add(128, 2, sep("contig", 2, 128), dict(kind="VEC", f_arg=2), dict(wide_form=0, bwd_split=1), K4_OPTIONS[3], split="forced",
        only="big20", why="forced on")
    add(128, 2, sep("contig", 2, 128), dict(kind="WIDE", f_arg=2), dict(wide_form=0, bwd_split=0), K4_OPTIONS[1], only="big48",
        why="forced off")
    add(130, 2, sep("contig", 2, 130), dict(kind="WIDE", f_arg=4), dflt, K4_OPTIONS[2], split="auto", only="big48",
        why="automatic split, a width the vector form does not take")
    add(64, 2, sep("contig", 2, 64), dict(kind="VEC", f_arg=1), dict(wide_form=2, bwd_split=-1), K4_OPTIONS[3],
        why="wide_form = 2 forces the vector form beyond the L2")
    add(64, 2, sep("contig", 2, 64), dict(kind="WIDE", f_arg=1), dict(wide_form=3, bwd_split=-1), K4_OPTIONS[0],
        why="wide_form = 3 keeps the pair form only where the tables fit")
    for f, ng in ((2, 2), (4, 3), (7, 2), (8, 1)):
        fp = fp_of(f)
        lay = adj("merged", ng, fp, 2 * fp, third=(0, fp)) if ng > 1 else sep("aligned", 1, fp)
        add(f, ng, lay, dict(kind="NARROW", f_arg=fp, vecmask=(1 << ng) - 1, merged=int(ng > 1)), dflt, K4_OPTIONS[f % 4] if ng > 1 else 1)
    add(2, 3, PAIR3, dict(kind="PAIR3", f_arg=2, vecmask=7, merged=0), dflt, K4_OPTIONS[0])
    return c


_CASES = {}


def cases(family):
    if not _CASES:
        for fam, make in (("narrow", _narrow_cases), ("pair3", _pair3_cases), ("vec", _vec_cases), ("wide", _wide_cases),
                          ("pair", _pair_cases), ("default", _default_cases), ("big", _big_cases)):
            _CASES[fam] = make()
        _CASES["vec-hi"] = _vec_cases(tuple(f for f in MULTIPLES_OF_4 if f > 128), "vec-hi")
    return _CASES[family]


FAMILIES = ("narrow", "pair3", "vec", "vec-hi", "wide", "pair", "default", "big")
# (operator, family) pairs the GPU file runs
PAIRS = ([(nm, fam) for fam in FAMILIES[:-1] for nm in SMALL_OPS] + [(nm, "big") for nm in BIG_OPS] +
         [(nm, "narrow") for nm in BIG_T_OPS])


def cases_for(name, family):
    return [c for c in cases(family) if getattr(c, "only", None) in (None, name.split("-")[0])]


def expected(case, name):
    """The answer acm_gather_form must give for ``case`` on operator ``name``: (form of the whole call or, where K4 splits, of
    every single-channel pass; k4_split)."""
    lanes, fix_narrow, fix_wide, rows16 = OPERATOR_FORMS[name]
    e = case.expect
    short = not rows16
    kind = e["kind_short"] if short and "kind_short" in e else e["kind"]
    f_arg = e["f_arg_short"] if short and "f_arg_short" in e else e["f_arg"]
    merged = e.get("merged", 0)
    if lanes != 16 and "kind_other_lanes" in e:
        kind, merged = e["kind_other_lanes"], e["merged_other_lanes"]
    want = dict(kind=kind, f_arg=f_arg, fixup=fix_narrow if case.f <= 8 else fix_wide)
    if case.f <= 8:
        want.update(lanes=lanes, vecmask=e["vecmask"], merged=merged)
    return want, int(case.split is not None)


# ---- the query ----
FAKE_BASE = 0x7F0000000000          # fabricated allocations: 4 GiB apart, aligned far beyond any predicate


def query(op, case, bases, ng=None, chan=None, bf16=0, fused_head=0):
    """acm_gather_query_t of ``case`` over ``op`` with buffer b at address bases[b]; ``chan``: the single channel of a pass."""
    from acm_gnn_amd import _lib
    q = _lib.GatherQuery()
    q.n_rows, q.n_cols, q.nnz = op.n_rows, op.n_cols, len(op.indices)
    q.n_long, q.n_multi = n_long(op), n_multi(op)
    q.has_long_index = int(q.n_long > 0)
    q.n_gathered, q.width, q.bf16, q.fused_head = (case.ng if chan is None else 1), case.f, bf16, fused_head
    for i, c in enumerate(range(case.ng) if chan is None else [chan]):
        q.table[i] = bases[case.layout.chan[c][0]] + 4 * case.layout.offset(c)
        q.ld[i] = case.layout.pitch(c)
    return q


def ask(q):
    """dict of the library's answer (kind and fixup by name)"""
    from acm_gnn_amd import _lib
    a = _lib.GatherFormAnswer()
    _lib.check(_lib.load().acm_gather_form(C.byref(q), C.byref(a)), "acm_gather_form")
    return dict(kind=_lib.GATHER_KINDS[a.kind], lanes=a.lanes, vecmask=a.vecmask, merged=a.merged, f_arg=a.f_arg,
                fixup=_lib.GATHER_FIXUPS[a.fixup], k4_split=a.k4_split)


def check_forms(op, name, case, bases):
    """The query's answers for ``case`` (the whole call, or every pass of a split K4) are what the table lists.  Returns the
    forms reached as tuples."""
    want, split = expected(case, name)
    whole = ask(query(op, case, bases))
    assert whole["k4_split"] == (split if case.api == "k4" else whole["k4_split"]), (name, case.id, whole, "split", split)
    answers = [ask(query(op, case, bases, chan=c)) for c in range(case.ng)] if split else [whole]
    reached = []
    for a in answers:
        got = {k: a[k] for k in want}
        assert got == want, (name, case.id, case.why, "got", got, "want", want)
        reached.append((a["kind"], a["lanes"] if case.f <= 8 else 0, a["f_arg"], 1 if split else case.ng,
                        a["vecmask"] if case.f <= 8 else 0, a["merged"], a["fixup"]))
    return reached


# ---- tables on the device ----
def _fill(total):
    return np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), total)


def build_tables(case, op, values, dev):
    """The gathered tables of ``case`` on the device: values[c] ([n_cols, F] float32) at channel c's place; every other float of
    every allocation -- pad columns, the floats in front of the first row, the rows no stored entry references -- holds NaN or
    +-inf.  An allocation ends where its last table row ends: after the last channel's F columns for F > 8, after the pitch for
    F <= 8 (the narrow vector fetch reads the padded block: acm_hip.h asks for n_cols x ld floats).  Returns
    (addresses per channel, pitches per channel, the tensors)."""
    f, lay = case.f, case.layout
    tensors, ptrs, lds = [], [None] * case.ng, [None] * case.ng
    for b, (off, ld) in enumerate(lay.bufs):
        chans = [c for c in range(case.ng) if lay.chan[c][0] == b]
        tail = ld if f <= 8 else max(lay.chan[c][1] for c in chans) + f
        assert tail <= ld, (case.id, tail, ld)
        total = off + (op.n_cols - 1) * ld + tail
        host = _fill(total)
        rows = np.lib.stride_tricks.as_strided(host[off:], shape=(op.n_cols, tail), strides=(4 * ld, 4))
        for c in chans:
            col = lay.chan[c][1]
            rows[:, col:col + f] = values[c]
        for i, r in enumerate(op.dead):
            rows[int(r), :] = R.NONFINITE[i % 3]
        t = torch.from_numpy(host).to(dev)
        assert t.data_ptr() % 256 == 0
        tensors.append(t)
        for c in chans:
            ptrs[c], lds[c] = t.data_ptr() + 4 * (off + lay.chan[c][1]), ld
    return ptrs, lds, tensors


def _zero_dead(values, op):
    v = values.astype(np.float64)
    v[np.asarray(op.dead, dtype=np.int64)] = 0.0
    return v


class Outputs:
    """``n`` outputs of [n_rows, F] as views of ONE NaN-filled buffer: output i starts at column 1 + i (F + 2) of rows of pitch
    n (F + 2) + 1.  Afterwards every [row, :F] must be finite and every other float still NaN."""

    def __init__(self, n_rows, f, n, dev):
        self.f, self.n, self.ld = f, n, n * (f + 2) + 1
        self.buf = torch.full((n_rows, self.ld), float("nan"), device=dev)

    def ptr(self, i):
        return self.buf.data_ptr() + 4 * (1 + i * (self.f + 2))

    def read(self, who):
        host = self.buf.cpu()
        keep = torch.zeros(self.ld, dtype=torch.bool)
        outs = []
        for i in range(self.n):
            lo = 1 + i * (self.f + 2)
            keep[lo:lo + self.f] = True
            outs.append(host[:, lo:lo + self.f].contiguous())
            assert bool(torch.isfinite(outs[-1]).all()), (who, "output", i, "is not finite everywhere")
        assert bool(torch.isnan(host[:, ~keep]).all()), (who, "a pad column of the outputs was written")
        return outs, host


def _pow2(rng, n):
    return (2.0 ** rng.integers(-2, 3, n)).astype(np.float32)


def _inputs(case, op, exact, seed):
    """Host inputs of one call: tables (integers in [-8, 8] or N(0, 1)) and the row-local terms."""
    rng = np.random.default_rng(seed)
    n, f = op.n_rows, case.f
    if exact:
        tabs = [rng.integers(-8, 9, (op.n_cols, f)).astype(np.float32) for _ in range(case.ng)]
        local = lambda: rng.integers(-8, 9, (n, f)).astype(np.float32)
        scale = lambda: _pow2(rng, n)
    else:
        tabs = [rng.standard_normal((op.n_cols, f)).astype(np.float32) for _ in range(case.ng)]
        local = lambda: rng.standard_normal((n, f)).astype(np.float32)
        scale = lambda: rng.uniform(0.25, 2.0, n).astype(np.float32)
    host = dict(s_high=local(), s_struc=local(), self_scale=scale(), inv_deg=scale(), sub=local(), row_scale=scale(), sub_scale=scale())
    for k in ("mask_low", "mask_high"):
        host[k] = (rng.uniform(0.1, 1.0, (n, f)) * rng.choice([-1.0, 1.0], (n, f))).astype(np.float32)
    return tabs, host


def reference(case, op, tabs, host):
    """float64 outputs and, per output, sum |a g| + |self term| (the bound's factor).  Exact for the integer inputs."""
    a = op.matrix()
    aa = abs(a)
    t64 = [_zero_dead(t, op) for t in tabs]
    h = {k: v.astype(np.float64) for k, v in host.items()}
    prod = [a @ t for t in t64]
    mag = [aa @ np.abs(t) for t in t64]
    if case.api == "spmm":
        if case.opts:
            ref = h["row_scale"][:, None] * prod[0] - h["sub_scale"][:, None] * h["sub"]
            m = h["row_scale"][:, None] * mag[0] + np.abs(h["sub_scale"][:, None] * h["sub"])
            keep = ref > 0
            return [np.where(keep, ref, 0.0)], [m]                      # (relu is 1-Lipschitz: the bound carries over)
        return [prod[0]], [mag[0]]
    masks, self_scale, inv_deg = case.opts
    sh = (h["self_scale"][:, None] if self_scale else 1.0) * h["s_high"]
    dl, dh = prod[0], sh - prod[1]
    ml, mh = mag[0], mag[1] + np.abs(sh)
    if masks:
        dl, dh = np.where(h["mask_low"] > 0, dl, 0.0), np.where(h["mask_high"] > 0, dh, 0.0)
    refs, mags = [dl, dh], [ml, mh]
    if case.ng == 3:
        ss = h["s_struc"] * (h["inv_deg"][:, None] if inv_deg else 1.0)
        refs.append(prod[2] - ss)
        mags.append(mag[2] + np.abs(ss))
    return refs, mags


def launch(case, g, ptrs, lds, host, dev):
    """One call of the case's entry point into fresh NaN-filled outputs.  Returns (the outputs, the whole output buffer)."""
    from acm_gnn_amd import _lib
    f, n = case.f, g.n_rows
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    out = Outputs(n, f, case.ng, dev)
    ws = g.workspace(case.ng * f)
    lib = _lib.load()
    if case.api == "spmm":
        o = _lib.SpmmOpts()
        if case.opts:
            o.row_scale, o.sub, o.ld_sub, o.sub_scale, o.relu = d["row_scale"].data_ptr(), d["sub"].data_ptr(), f, d["sub_scale"].data_ptr(), 1
        st = lib.acm_spmm_ex(g.handle, ptrs[0], lds[0], f, out.ptr(0), out.ld, C.byref(o), ws.data_ptr(), ws.numel() * 4, R._stream())
        _lib.check(st, "acm_spmm_ex")
    else:
        masks, self_scale, inv_deg = case.opts
        r = _lib.ConvBwdSpmm()
        r.f_out, r.row_offset, r.gather_bf16 = f, 0, 0
        r.g_low, r.ld_g_low, r.g_high, r.ld_g_high = ptrs[0], lds[0], ptrs[1], lds[1]
        r.s_high, r.ld_s_high = d["s_high"].data_ptr(), f
        r.dz_low, r.ld_dz_low, r.dz_high, r.ld_dz_high = out.ptr(0), out.ld, out.ptr(1), out.ld
        if case.ng == 3:
            r.g_struc, r.ld_g_struc = ptrs[2], lds[2]
            r.s_struc, r.ld_s_struc = d["s_struc"].data_ptr(), f
            r.d_struc, r.ld_d_struc = out.ptr(2), out.ld
            if inv_deg:
                r.inv_deg = d["inv_deg"].data_ptr()
        if self_scale:
            r.self_scale = d["self_scale"].data_ptr()
        if masks:
            r.mask_low, r.ld_mask_low, r.mask_high, r.ld_mask_high = d["mask_low"].data_ptr(), f, d["mask_high"].data_ptr(), f
        st = lib.acm_conv_bwd_spmm(g.handle, C.byref(r), ws.data_ptr(), ws.numel() * 4, R._stream())
        _lib.check(st, "acm_conv_bwd_spmm")
    return out.read((g, case.id))


def run_case(name, case, dev, seed=0):
    """``case`` on operator ``name``: the query with the real addresses, then the exact and the bounded comparison, each call
    made twice (bit-identical).  Returns (the forms reached, the worst error / bound)."""
    base_op = operators()[name]
    worst, reached = 0.0, []
    for exact in (True, False):
        op = int_twin(base_op) if exact else base_op
        g = handle_of(op, dev)
        assert (g.n_long_rows, g.nnz) == (n_long(op), len(op.indices))
        tabs, host = _inputs(case, op, exact, seed + 2 * case.f + int(exact))
        ptrs, lds, keep = build_tables(case, op, tabs, dev)
        bases = [t.data_ptr() for t in keep]
        reached = check_forms(op, name, case, bases)
        refs, mags = reference(case, op, tabs, host)
        first, raw1 = launch(case, g, ptrs, lds, host, dev)
        _, raw2 = launch(case, g, ptrs, lds, host, dev)
        assert torch.equal(raw1.view(torch.int32), raw2.view(torch.int32)), (name, case.id, "two runs differ")
        for i, (got, ref, mag) in enumerate(zip(first, refs, mags)):
            got = got.numpy().astype(np.float64)
            if exact:
                bad = np.argwhere(got != ref)
                assert bad.size == 0, (name, case.id, reached, "output", i, "differs from the integer result at", bad[:8].tolist(),
                                       got[tuple(bad[0])], ref[tuple(bad[0])])
            else:
                nn = (op.lengths.astype(np.float64) + 4.0)[:, None] * U
                bound = nn / (1.0 - nn) * mag
                err = np.abs(got - ref)
                over = np.argwhere(err > bound)
                assert over.size == 0, (name, case.id, reached, "output", i, "beyond the bound at", over[:8].tolist(),
                                        err[tuple(over[0])], bound[tuple(over[0])])
                pos = bound > 0
                if pos.any():
                    worst = max(worst, float((err[pos] / bound[pos]).max()))
    return reached, worst


def dump_evidence(forms):
    """Worst error / bound per form (R.RATIOS, keys "gather ...") and the forms reached, as gather_forms.json where
    ACM_EVIDENCE_DIR says; without it nothing is written."""
    out_dir = os.environ.get("ACM_EVIDENCE_DIR")
    if not out_dir:
        return
    os.makedirs(out_dir, exist_ok=True)
    ratios = {k: v for k, v in R.RATIOS.items() if k.startswith("gather ")}
    with open(os.path.join(out_dir, "gather_forms.json"), "w") as fh:
        json.dump({"worst_error_over_bound": ratios, "forms_reached": sorted(forms)}, fh, indent=1, sort_keys=True)
