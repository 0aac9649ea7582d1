"""CPU: the host model of the planned sampler step (tests/plan_ref.py) and the plan builders of plangen_amd/guidance.py.  The model's power is shown with
planted mutants: each wrong reading of the definition must be caught by the comparison the GPU tests make (the mixed row bit for bit, every decided draw,
every greedy token) on the families those tests use; and the model alone, with draw_ref.E_G_CPU, must leave at most draw_ref.UNDECIDED_CAP of each
family's draws undecided.  Also the ABI surface: header, version script and the ctypes table name the entry point."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import draw_ref as D
import plan_ref as P
from plangen_amd import _lib, guidance as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _family(V, S):
    """[(case, step, model outputs)] of one parametrisation, computed once and shared."""
    if (V, S) not in _CACHE:
        out = []
        for c in P.plan_cases(V, S):
            cond, unc = P.cond_uncond(c)
            for step in c["steps"]:
                out.append((c, step, cond, unc, P.step_model(cond, unc, c["plan"], c["b_off"], step, c["seed"])))
        _CACHE[(V, S)] = out
    return _CACHE[(V, S)]


@pytest.mark.parametrize("S", P.PLAN_S)
@pytest.mark.parametrize("V", P.PLAN_V)
def test_model_alone_stays_inside_the_undecided_cap(V, S):
    n = open_ = 0
    greedy = sampled = flt = 0
    for c, step, cond, unc, (mixed, tok, gap, scale, ru, smp) in _family(V, S):
        assert (mixed == mixed.astype(np.float32)).all()                 # the dyadic slabs: the fp32 row is the fp64 row
        dec = D.decided(gap, scale, D.E_G_CPU)
        n += int(smp.sum()); open_ += int((smp & ~dec).sum())
        greedy += int((~smp).sum()); sampled += int(smp.sum()); flt += int(P.filtered(c["plan"]))
    print(f"plan V={V} S={S}: {open_} of {n} sampled draws open; {greedy} greedy")
    assert greedy > 0 and sampled > 0                                     # both kinds share calls
    assert (flt > 0) == (V >= 1000)
    assert open_ <= D.UNDECIDED_CAP * n, (open_, n)


def _caught(V, S, mutant):
    for c, step, cond, unc, (mixed, tok, gap, scale, ru, smp) in _family(V, S):
        m_mixed, m_tok, *_ = P.step_model(cond, unc, c["plan"], c["b_off"], step, c["seed"], mutant)
        if not np.array_equal(m_mixed, mixed):
            return True
        binding = ~smp | D.decided(gap, scale, D.E_G_CPU)
        if (binding & (m_tok != tok)).any():
            return True
    return False


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_every_planted_mutant_is_caught(mutant):
    """On every family where the mutant can show at all.  The weight mutants: everywhere.  The draw mutants (temperature, key, greedy): wherever a row
    has more than one token, V >= 17 -- at V = 1 every draw is token 0 whatever the noise.  The shifted filter: where the family has a filtered
    image, V >= 1000 (plan_cases keeps the filters off below that: top_k = 50 of 17 tokens keeps everything)."""
    first = {"w_local_b": 1, "w_step_major": 1, "filter_shifted": 1000}.get(mutant, 17)
    for V in P.PLAN_V:
        for S in P.PLAN_S:
            if V >= first:
                assert _caught(V, S, mutant), (mutant, V, S)


def test_plan_offsets_reach_both_ends_of_the_weight_array():
    assert P.PLAN_T == 576 and set(D.IMG_CASE_STEPS) >= {0, 575}
    offs = {(c["b_off"], c["B_total"]) for c in P.plan_cases(17, 1)}
    assert any(b == 0 for b, _ in offs) and any(b + P.PLAN_B == n for b, n in offs) and any(b > 0 for b, _ in offs)


# ------------------------------------------------------------------------------------------------------------------------------- guidance.py
def test_schedule_endpoints_monotone_and_one_hand_value():
    T = 576
    for kind in G.KINDS:
        w = G.schedule(kind, 7.0, 3.0, T)
        assert w.dtype == np.float32 and w.shape == (T,) and w[0] == np.float32(7.0)
        if kind == "constant":
            assert (w == np.float32(7.0)).all()
        else:
            assert w[-1] == np.float32(3.0) and (np.diff(w.astype(np.float64)) <= 0).all() and (np.diff(w.astype(np.float64)) < 0).any()
        up = G.schedule(kind, 1.0, 9.0, T)
        assert (np.diff(up.astype(np.float64)) >= 0).all()
    # cosine at a quarter of the way, T = 5 -> s = 1/4: 3 + 4 (1 + cos(pi / 4)) / 2 = 5 + sqrt(2) = 6.414213562...
    assert G.schedule("cosine", 7.0, 3.0, 5)[1] == np.float32(5.0 + math.sqrt(2.0))
    assert G.schedule("linear", 7.0, 3.0, 5).tolist() == [7.0, 6.0, 5.0, 4.0, 3.0]
    assert G.schedule("cosine", 7.0, 3.0, 5)[2] == np.float32(5.0)
    assert G.schedule("linear", 2.0, 4.0, 1).tolist() == [2.0]
    with pytest.raises(ValueError):
        G.schedule("ramp", 1, 2, 4)


def test_box_weights_union_and_empty_box():
    g = 24
    w = G.box_weights(["[0,0,500,500]", "[500,500,1000,1000]"], g, 7.0, 3.0)
    m = w.reshape(g, g)
    assert w.dtype == np.float32 and w.shape == (g * g,)
    assert (m[:12, :12] == 7.0).all() and (m[12:, 12:] == 7.0).all() and (m[:12, 12:] == 3.0).all() and (m[12:, :12] == 3.0).all()
    # a box between two cell centres (centres sit at 20.83 + 41.67 k) holds none: all outside; so does a malformed text, and no box at all
    assert (G.box_weights(["[22,22,60,60]"], g, 7.0, 3.0) == 3.0).all()
    assert (G.box_weights(["[a,b]"], g, 7.0, 3.0) == 3.0).all() and (G.box_weights([], g, 7.0, 3.0) == 3.0).all()
    # centre / height / width form: the same region
    assert np.array_equal(G.box_weights(["[250,250,500,500]"], g, 1.0, 0.0, use_centerhw=True), G.box_weights(["[0,0,500,500]"], g, 1.0, 0.0))


def test_replicate_layout_and_plan_validation():
    per = G.SamplePlan(cfg_weight=np.array([[1, 2], [3, 4], [5, 6]], dtype=np.float32), temperature=[0.0, 0.7, 1.3], image_key=[10, 11, 12])
    r = G.replicate(per, 2, 3)
    assert r.B == 6
    for t in range(2):
        for i in range(3):
            assert r.cfg_weight[t * 3 + i].tolist() == per.cfg_weight[i].tolist()
            assert r.temperature[t * 3 + i] == per.temperature[i] and r.image_key[t * 3 + i] == per.image_key[i]
    assert r.top_k is None and r.top_p is None
    w, t, k, p, key = r.arrays(2)
    assert w.dtype == np.float32 and w.shape == (6, 2) and key.dtype == np.int32 and k is None
    assert G.SamplePlan(cfg_weight=[1.0, 5.0]).arrays(4)[0].tolist() == [[1.0] * 4, [5.0] * 4]          # [B] broadcast over the steps
    with pytest.raises(ValueError):
        r.arrays(3)                                                                                         # T differs
    with pytest.raises(ValueError):
        G.replicate(per, 2, 4)
    for bad in (dict(), dict(cfg_weight=[1.0, float("nan")]), dict(temperature=[float("inf")]), dict(top_k=[-1]), dict(top_p=[0.0]), dict(top_p=[1.5]),
                dict(top_p=[float("nan")]), dict(image_key=[-1]), dict(image_key=[2 ** 31 - 1]), dict(temperature=[1.0, 1.0], top_k=[1]),
                dict(top_k=[1.5]), dict(image_key=[float("nan")]), dict(top_k=[True])):
        with pytest.raises(ValueError):
            G.SamplePlan(**bad)


# ------------------------------------------------------------------------------------------------------------------------------- ABI surface
def test_entry_point_in_header_map_and_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    assert re.search(r"int\s+pg_request_sample_plan\s*\(\s*pg_handle h,\s*const pg_sample_plan\*\s*plan[^;]*pg_stream s\s*\)\s*;", hdr)
    body = re.search(r"typedef struct pg_sample_plan \{(.*?)\} pg_sample_plan;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:,\s*(\w+)\s*)?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    flat = [n for pair in names for n in pair if n]
    assert flat == [f for f, _ in _lib.pg_sample_plan._fields_], flat
    assert "pg_request_sample_plan;" in open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    sym = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert sym["pg_request_sample_plan"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.pg_sample_plan), C.c_void_p])
    assert "pg_diag_op_cfg_sample_plan" in open(os.path.join(ROOT, "plangen_amd", "csrc", "diag_ops.hip")).read()
