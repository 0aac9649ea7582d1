"""Host-side checks of the layout-attribution feature: the span reference and its bound against a numpy model of the kernel's arithmetic
(tests/span_ref.py), the planted defects, the host span / box helpers, and the C ABI's declarations of the two new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import span_ref as SP
from plangen_amd import _lib
from plangen_amd.textproc import TagWordCodec, box_cells, layout_spans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_SETS = [(100, 1), (0, SP.FRAME), (100, 70)]        # (q_col0, n_q): one query in the middle of a tile, every column, a run across tiles


@pytest.fixture(scope="module")
def cases():
    out = {}
    for fam in SP.FAMILIES:
        for q_col0, n_q in QUERY_SETS:
            c = SP.make_case(fam, q_col0, n_q, 16)
            out[(fam, q_col0, n_q)] = (c,) + SP.span_mass_ref(c)
    return out


def test_bound_is_tight_enough(cases):
    for key, (_, _, bound) in cases.items():
        assert 0 < bound.max() <= SP.BOUND_CAP, key


def test_reference_properties(cases):
    c, A, _ = cases[("peaked", 0, SP.FRAME)]
    assert A.min() >= 0 and A.max() <= 1 + 1e-12
    for r in range(len(c["length"])):
        p = int(c["pad"][r])
        assert (A[r, :p] == 0).all()                                   # pad queries
        assert np.allclose(A[r, p:, 9], 1.0, atol=1e-12)               # span 9 is the whole frame
        assert (A[r, :, 1] == 0).all() and (A[r, :, 8] == 0).all()     # the two empty spans
    # a partition of the frame sums to one on every real query
    cp = SP.make_case("peaked", 0, SP.FRAME, 16, partition=True)
    Ap, _ = SP.span_mass_ref(cp)
    for r in range(len(cp["length"])):
        p = int(cp["pad"][r])
        assert np.allclose(Ap[r, p:].sum(-1), 1.0, atol=1e-12) and (Ap[r, :p] == 0).all()


def test_emulated_arithmetic_stays_inside_the_bound(cases):
    for key, (c, A, bound) in cases.items():
        err, frac, exact = SP.worst(SP.span_mass_emulated(c), A, bound)
        print(f"{key}: max |emulated - ref| = {err:.3e}, error / bound = {frac:.3f}")
        assert frac <= 1.0 and exact, key


@pytest.mark.parametrize("defect", SP.DEFECTS)
def test_planted_defect_leaves_the_bound(cases, defect):
    worst_frac = {}
    for key, (c, A, bound) in cases.items():
        _, frac, exact = SP.worst(SP.span_mass_emulated(c, defect), A, bound)
        worst_frac[key] = frac if exact else float("inf")
    print(f"{defect}: largest error / bound per case: { {k: round(v, 1) for k, v in worst_frac.items()} }")
    assert max(worst_frac.values()) >= 10.0, worst_frac


def test_large_family_raises_the_running_maximum(cases):
    """Without the rescale of the span sum the large-magnitude family is off by far more than on the others: it is the family that shows it."""
    c, A, bound = cases[("large", 0, SP.FRAME)]
    _, frac, _ = SP.worst(SP.span_mass_emulated(c, "no_rescale"), A, bound)
    assert frac >= 100.0


# ------------------------------------------------------------------------------------------------ layout_spans / box_cells
def _enc(codec, text):
    return codec.encode(text)


def _tags(codec):
    return {t: codec.token_id(t) for t in ("<ref>", "</ref>", "<box>", "</box>")}


def _item(i):
    return f"<ref>thing {'x' * (i + 1)}</ref><box>[{10 * i},{20 + i},{500 + i},{600 + i}]</box>"


@pytest.mark.parametrize("n", [0, 1, 17])
def test_layout_spans_counts_and_contents(n):
    codec = TagWordCodec(512)
    text = "a caption <grounding>" + "".join(_item(i) for i in range(n)) + "</grounding>"
    ids = _enc(codec, text)
    tags = _tags(codec)
    ent, phr, box = (layout_spans(ids, tags, k) for k in ("entity", "phrase", "box"))
    assert len(ent) == len(phr) == len(box) == n
    for i in range(n):
        assert codec.decode(ids[ent[i][0]:ent[i][1]]) == _item(i)
        assert codec.decode(ids[phr[i][0]:phr[i][1]]) == f"thing {'x' * (i + 1)}"
        assert codec.decode(ids[box[i][0]:box[i][1]]) == f"[{10 * i},{20 + i},{500 + i},{600 + i}]"
        assert ent[i][0] == phr[i][0] - 1 and ent[i][1] == box[i][1] + 1
    assert all(a[1] <= b[0] for a, b in zip(ent, ent[1:]))


def test_layout_spans_malformed():
    codec = TagWordCodec(512)
    tags = _tags(codec)
    good = "<ref>a cat</ref><box>[1,2,3,4]</box>"
    # nested <ref>: the inner one is the item; unclosed / truncated tails and out-of-place tags yield nothing
    ids = _enc(codec, "<ref>outer <ref>a cat</ref><box>[1,2,3,4]</box>")
    (lo, hi), = layout_spans(ids, tags, "entity")
    assert codec.decode(ids[lo:hi]) == good
    for bad in ("<ref>a cat</ref><box>[1,2,3", "<ref>a cat</ref>", "<ref>a cat", "<box>[1,2,3,4]</box>", "</ref><box>[1,2,3,4]</box>",
                "<ref>a cat</ref> and <box>[1,2,3,4]</box>", "<ref>a cat<box>[1,2,3,4]</box>", "<ref>a</ref><box>[1,2<box>3,4]</box>"):
        ids = _enc(codec, good + bad)
        spans = layout_spans(ids, tags, "entity")
        assert len(spans) == 1 and codec.decode(ids[spans[0][0]:spans[0][1]]) == good, bad
    with pytest.raises(ValueError):
        layout_spans([1, 2], tags, "word")


def test_box_cells():
    m = box_cells("[0,0,500,250]", 8)
    assert m.dtype == bool and m.shape == (8, 8)
    want = np.zeros((8, 8), dtype=bool); want[:2, :4] = True            # centres at 62.5 + 125 i: x <= 500 -> 4 columns, y <= 250 -> 2 rows
    assert (m == want).all()
    assert (box_cells("0,0,500,250", 8) == want).all()                   # brackets optional
    assert box_cells("[0,0,1000,1000]", 24).all()
    # cx, cy, h, w: centre (250, 125), height 250, width 500 -> the same box
    assert (box_cells("[250,125,250,500]", 8, use_centerhw=True) == want).all()
    assert (box_cells("[250,125,250,500]", 8) != want).any()
    # degenerate: a box between two cell centres, an inverted one, and text that is no box
    for t in ("[70,70,100,100]", "[500,500,100,100]", "[1,2,3]", "[a,b,c,d]", ""):
        assert not box_cells(t, 8).any(), t
    one = box_cells("[60,60,65,65]", 8)                                   # holds exactly the first centre (62.5, 62.5)
    assert one.sum() == 1 and one[0, 0]


# ------------------------------------------------------------------------------------------------ the C ABI's two new symbols
def test_new_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int pg_request_attn_spans\(pg_handle h, const pg_attn_spans\* req\s*\);", code)
    assert m, "pg_request_attn_spans(pg_handle, const pg_attn_spans*) not declared"
    op = re.search(r"int pg_op_attn_span_mass\((.*?)\);", code, flags=re.S)
    assert op and len(op.group(1).split(",")) == 17
    st = re.search(r"typedef struct pg_attn_spans \{(.*?)\} pg_attn_spans;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", st)
    assert fields == ["span_lo_host", "span_hi_host", "rows", "n_spans", "q_col0", "n_q", "layer_mask", "out_dev", "capacity_floats"]
    assert [n for n, _ in _lib.pg_attn_spans._fields_] == fields
    assert C.sizeof(_lib.pg_attn_spans) == 56 and _lib.pg_attn_spans.layer_mask.offset == 32 and _lib.pg_attn_spans.out_dev.offset == 40
    mp = open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    sym = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in ("pg_request_attn_spans", "pg_op_attn_span_mass"):
        assert re.search(rf"\b{name};", mp) and name in sym
    assert sym["pg_request_attn_spans"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.pg_attn_spans)])
    r, a = sym["pg_op_attn_span_mass"]
    assert r is C.c_int and len(a) == 17 and a[:8] == [C.c_void_p] * 8 and a[8:14] == [C.c_int] * 6 and a[14] is C.c_float and a[15:] == [C.c_void_p] * 2
