"""The table of tests/gather_forms.py against the real chooser: acm_gather_form (host code, no device) is asked for every case on
fabricated addresses with the case's alignment and must answer the form written in the table; the table must reach every form of
the fp32 gather family, and every alignment predicate must be the sole reason for at least one case's form."""
import ctypes as C

import pytest

import gather_forms as G
import launch_forms as LF

BASES = [G.FAKE_BASE + (b << 32) for b in range(3)]


def _all_pairs():
    """the GPU file's (operator, family) pairs and, for the operator table's sake, every other operator on one small family"""
    extra = [(nm, "pair3") for nm in G.OPERATOR_FORMS if nm not in G.SMALL_OPS + G.BIG_OPS + G.BIG_T_OPS]
    return G.PAIRS + extra


_REACHED = {}


def _reached(tune):
    """(kind, lanes, f_arg, NG, vecmask, merged, fixup, split) -> a case that reaches it, over every pair of the GPU file"""
    if not _REACHED:
        for name, family in _all_pairs():
            op = G.operators()[name]
            for case in G.cases_for(name, family):
                tune(**case.tune)
                for form in G.check_forms(op, name, case, BASES):
                    _REACHED.setdefault(form + (case.split,), (name, case.id))
    return _REACHED


def test_symbol_answers_without_a_device():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    assert "acm_gather_form" in _lib.EXPORTED_SYMBOLS and lib.acm_version() == 29 == _lib.ABI_VERSION
    a = _lib.GatherFormAnswer()
    assert lib.acm_gather_form(None, C.byref(a)) == 1                       # ACM_EINVAL
    q = _lib.GatherQuery()
    q.n_rows, q.n_cols, q.nnz, q.n_gathered, q.width = 10, 10, 50, 4, 8
    assert lib.acm_gather_form(C.byref(q), C.byref(a)) == 2                 # ACM_ESHAPE: four gathered tables
    q.n_gathered, q.width = 1, 257
    assert lib.acm_gather_form(C.byref(q), C.byref(a)) == 4                 # ACM_EUNSUPPORTED: one column block is 256 wide
    q.width, q.bf16 = 33, 1
    assert lib.acm_gather_form(C.byref(q), C.byref(a)) == 4


@pytest.mark.parametrize("name", sorted(G.OPERATOR_FORMS))
def test_operators_are_what_the_table_says(name):
    """Lanes, long rows, rows of several windows and the mean row length of every operator; each has empty rows and at least two
    table rows nobody references."""
    op = G.operators()[name]
    lanes, fix_narrow, fix_wide, rows16 = G.OPERATOR_FORMS[name]
    mean = len(op.indices) / op.n_rows
    t = LF.T
    assert lanes == (8 if mean <= t["NARROW_8_LANES_UP_TO"] else (16 if mean <= t["NARROW_16_LANES_UP_TO"] else 32)), (name, mean)
    narrow_only = name.startswith("big") and name.endswith("-T")           # (they run the narrow family alone)
    assert rows16 == (mean >= t["VEC_MIN_ROW_ONE"]) and (mean >= t["VEC_MIN_ROW_MANY"] or narrow_only), (name, mean)
    assert not t["VEC_MIN_ROW_ONE"] <= mean < t["VEC_MIN_ROW_ONE"] + 1 and not t["VEC_MIN_ROW_MANY"] <= mean < t["VEC_MIN_ROW_MANY"] + 1
    assert fix_wide == ("wide" if G.n_long(op) else "none"), (name, G.n_long(op))
    want_narrow = ("windows" if G.n_multi(op) else "none") if lanes == 16 else fix_wide.replace("wide", "narrow")
    assert fix_narrow == want_narrow, (name, G.n_long(op), G.n_multi(op))
    assert len(op.dead) >= 2 and int((op.lengths == 0).sum()) >= 1, (name, op.dead, int((op.lengths == 0).sum()))
    assert int(op.lengths.max()) * 64 + 64 < 2 ** 24                        # the exact reference: no partial sum leaves the integers
    if name.startswith("big") and not name.endswith("-T"):
        split = name.startswith("big48")
        assert (mean >= t["K4_SPLIT_MIN_ROW"]) == split and op.n_cols == LF.GATHER_BIG_COLS, (name, mean)
    assert (op.vals is None) == ("unit" in name)


def test_every_case_gets_the_form_the_table_lists(tune):
    reached = _reached(tune)
    assert sum(len(G.cases(f)) for f in G.FAMILIES) > 500 and len(reached) > 150


def test_the_table_reaches_every_form(tune):
    reached = _reached(tune)
    keys = list(reached)

    def have(**kw):
        names = ("kind", "lanes", "f_arg", "ng", "vecmask", "merged", "fixup", "split")
        return [k for k in keys if all(k[names.index(n)] == v for n, v in kw.items())]

    for lanes in (8, 16, 32):
        for fp in (2, 4, 8):
            for ng in (1, 2, 3):
                full = (1 << ng) - 1
                assert have(kind="NARROW", lanes=lanes, f_arg=fp, ng=ng, vecmask=full), (lanes, fp, ng, "vecmask all set")
                assert have(kind="NARROW", lanes=lanes, f_arg=fp, ng=ng, vecmask=0, merged=0), (lanes, fp, ng, "vecmask all clear")
                if ng >= 2:
                    assert have(kind="NARROW", lanes=lanes, f_arg=fp, ng=ng, merged=1), (lanes, fp, ng, "merged")
                    assert have(kind="NARROW", lanes=lanes, f_arg=fp, ng=ng, merged=0, vecmask=full), (lanes, fp, ng, "separate")
                    assert [k for k in have(kind="NARROW", lanes=lanes, f_arg=fp, ng=ng, merged=0) if 0 < k[4] < full], (lanes, fp, ng, "mixed")
    # F < FP with and without the vector fetch: by the cases' own widths
    for f in (1, 3, 5, 6, 7):
        got = {c.expect["vecmask"] != 0 for c in G.cases("narrow") if c.f == f and c.ng == 1}
        assert got == {True, False}, f
    assert have(kind="PAIR3", lanes=16, ng=3)
    assert have(kind="PAIR3", fixup="windows") and have(kind="PAIR3", fixup="none")
    for ng in (1, 2, 3):
        assert have(kind="PAIR_F32", ng=ng), ng
        for nb in (1, 2, 3, 4):
            assert have(kind="VEC", f_arg=nb, ng=ng), (nb, ng)
        for nreg in (1, 2, 4):
            assert have(kind="WIDE", f_arg=nreg, ng=ng), (nreg, ng)
    for ng in (1, 2, 3):                            # the pair form below 64 columns and at 64
        widths = {c.f for fam in ("pair", "default", "big") for c in G.cases(fam) if c.ng == ng and c.expect["kind"] == "PAIR_F32"}
        assert 64 in widths and min(widths) < 64, (ng, widths)
    for fix in ("narrow", "windows", "wide", "none"):
        assert have(fixup=fix), fix
    assert have(kind="NARROW", fixup="none", lanes=8) and have(kind="NARROW", fixup="none", lanes=16) and have(kind="WIDE", fixup="none")
    assert have(split="auto") and have(split="forced")
    big = {c.why: c for c in G.cases("big")}
    assert any(c.expect["kind"] == "WIDE" and "by the table size alone" in w for w, c in big.items())
    assert any(c.split is None and c.tune.get("bwd_split") == 0 and getattr(c, "only", None) == "big48" for c in big.values())   # forced off


def _ask(op, case, bases=BASES, **edit):
    q = G.query(op, case, bases)
    for k, v in edit.items():
        if k in ("table", "ld"):
            for c, delta in v.items():
                getattr(q, k)[c] += delta
        else:
            setattr(q, k, v)
    return G.ask(q)


def _case(family, **kw):
    found = [c for c in G.cases(family) if all(getattr(c, k) == v or (k == "layout" and c.layout.name == v) for k, v in kw.items())]
    assert found, (family, kw)
    return found[0]


def test_every_alignment_predicate_alone_changes_a_form(tune):
    """One property flipped in a case that has the form: the answer changes, in the field that property decides."""
    ops = G.operators()
    hub, ladder, big = ops["hub"], ops["ladder"], ops["big20"]
    tune(wide_form=0, bwd_split=-1)
    # narrow, one channel: base alignment, pitch alignment, pitch at least FP
    c = _case("narrow", f=4, ng=1, layout="aligned")
    assert _ask(hub, c)["vecmask"] == 1
    assert _ask(hub, c, table={0: 4})["vecmask"] == 0 and _ask(hub, c, table={0: 8})["vecmask"] == 0
    assert _ask(hub, c, ld={0: 1})["vecmask"] == 0 and _ask(hub, c, ld={0: 4})["vecmask"] == 1
    c = _case("narrow", f=2, ng=1, layout="aligned")
    assert _ask(hub, c, table={0: 8})["vecmask"] == 1 and _ask(hub, c, table={0: 4})["vecmask"] == 0      # FP = 2: 8-byte rows
    c = _case("narrow", f=5, ng=1, layout="aligned")                              # FP = 8, pitch 8
    assert _ask(hub, c)["vecmask"] == 1 and _ask(hub, c, ld={0: -4})["vecmask"] == 0                      # pitch 4: aligned, but < FP
    # merged: adjacency, equal pitches, the block alignment of base and pitch
    c = _case("narrow", f=4, ng=2, layout="merged")
    base = _ask(hub, c)
    assert base["merged"] == 1 and base["vecmask"] == 3
    for edit in (dict(table={1: 16}), dict(ld={1: 8}), dict(table={0: 16, 1: 16}), dict(ld={0: 4, 1: 4})):
        got = _ask(hub, c, **edit)
        assert got["merged"] == 0 and got["vecmask"] == 3 and got["kind"] == "NARROW", (edit, got)
    # the packed rows: every clause of the pair-lane kernel's condition
    c = _case("pair3", layout="pair3")
    assert _ask(hub, c)["kind"] == "PAIR3"
    for edit in (dict(table={0: 32, 1: 32, 2: 32}), dict(fused_head=1)):
        assert _ask(hub, c, **edit)["kind"] == "PAIR3", edit
    for edit in (dict(table={0: 16, 1: 16, 2: 16}), dict(table={2: 8}), dict(table={1: 8}), dict(ld={0: 8, 1: 8, 2: 8}), dict(ld={2: 8}),
                 dict(has_long_index=0), dict(nnz=12 * hub.n_rows), dict(nnz=161 * hub.n_rows)):
        assert _ask(hub, c, **edit)["kind"] == "NARROW", edit
    # the pair form: 8-byte base, even pitch; the vector form: 16-byte base, pitch 4 k
    c = _case("default", f=50, ng=1, layout="contig")
    assert _ask(hub, c)["kind"] == "PAIR_F32"
    assert _ask(hub, c, table={0: 4})["kind"] == "WIDE" and _ask(hub, c, ld={0: 1})["kind"] == "WIDE"
    assert _ask(hub, c, table={0: 8})["kind"] == "PAIR_F32" and _ask(hub, c, ld={0: 2})["kind"] == "PAIR_F32"
    c = _case("default", f=64, ng=2, layout="contig")
    assert _ask(ladder, c)["kind"] == "VEC"
    for edit in (dict(table={1: 8}), dict(ld={1: 2}), dict(table={0: 8})):
        assert _ask(ladder, c, **edit)["kind"] == "PAIR_F32", edit
    for edit in (dict(table={1: 4}), dict(ld={0: 1})):
        assert _ask(ladder, c, **edit)["kind"] == "WIDE", edit
    c = _case("default", f=128, ng=3, layout="contig")
    assert _ask(hub, c)["kind"] == "VEC" and _ask(hub, c, table={2: 8})["kind"] == "WIDE" and _ask(hub, c, ld={2: 2})["kind"] == "WIDE"


def test_every_size_condition_alone_changes_a_form(tune):
    """The 8 MiB bound, the mean row lengths 16 and 4 of the vector form and K4's 32, each at its edge."""
    ops = G.operators()
    big, hub = ops["big48"], ops["hub"]
    tune(wide_form=0, bwd_split=-1)
    l2 = LF.T["GATHER_L2_MIB"] << 20
    c = [c for c in G.cases("big") if "by the table size alone" in c.why][0]
    assert _ask(big, c)["kind"] == "WIDE"
    assert _ask(big, c, n_cols=l2 // (64 * 2 * 4))["kind"] == "VEC" and _ask(big, c, n_cols=l2 // (64 * 2 * 4) + 1)["kind"] == "WIDE"
    tune(wide_form=3)
    assert _ask(big, c, n_cols=l2 // (64 * 2 * 4))["kind"] == "PAIR_F32" and _ask(big, c, n_cols=l2 // (64 * 2 * 4) + 1)["kind"] == "WIDE"
    tune(wide_form=0)
    c = _case("default", f=64, ng=1, layout="contig")
    n = hub.n_rows
    assert _ask(hub, c, nnz=LF.T["VEC_MIN_ROW_ONE"] * n)["kind"] == "VEC" and _ask(hub, c, nnz=LF.T["VEC_MIN_ROW_ONE"] * n - 1)["kind"] == "PAIR_F32"
    c = _case("default", f=128, ng=2, layout="contig")
    assert _ask(hub, c, nnz=LF.T["VEC_MIN_ROW_MANY"] * n)["kind"] == "VEC" and _ask(hub, c, nnz=LF.T["VEC_MIN_ROW_MANY"] * n - 1)["kind"] == "WIDE"
    c = [c for c in G.cases("big") if c.split == "auto" and c.ng == 2 and c.f == 128][0]
    n = big.n_rows
    assert _ask(big, c)["k4_split"] == 1
    assert _ask(big, c, nnz=LF.T["K4_SPLIT_MIN_ROW"] * n)["k4_split"] == 1 and _ask(big, c, nnz=LF.T["K4_SPLIT_MIN_ROW"] * n - 1)["k4_split"] == 0
    assert _ask(big, c, n_cols=l2 // (128 * 4))["k4_split"] == 0 and _ask(big, c, n_cols=l2 // (128 * 4) + 1)["k4_split"] == 1
    assert _ask(big, c, bf16=1, width=64, n_cols=10 ** 6)["k4_split"] == 0
    for forced in (0, 1):
        tune(bwd_split=forced)
        assert _ask(big, c)["k4_split"] == forced and _ask(hub, c)["k4_split"] == forced
        assert _ask(hub, _case("narrow", f=8, ng=2, layout="merged"))["k4_split"] == 0          # narrow layers never split
    # the long rows decide the fix-up, the lanes which one
    tune(bwd_split=-1)
    c = _case("narrow", f=4, ng=2, layout="merged")
    assert _ask(hub, c)["fixup"] == "windows" and _ask(hub, c, n_multi=0)["fixup"] == "none"
    assert _ask(hub, c, nnz=12 * hub.n_rows)["fixup"] == "narrow" and _ask(hub, c, nnz=12 * hub.n_rows, n_long=0, has_long_index=0)["fixup"] == "none"
    c = _case("default", f=64, ng=2, layout="contig")
    assert _ask(hub, c)["fixup"] == "wide" and _ask(hub, c, n_long=0)["fixup"] == "none"
