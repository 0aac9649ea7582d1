"""CPU: the fp64 reference of the per-token uncertainty outputs (stats_ref.py) against torch in fp64, its comparison against planted
errors, the derived entropy bound against an fp32 restatement of the two passes, and the binding of the two new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import logprob_ref as LR
import stats_ref as SR
from plangen_amd import _lib
from plangen_amd._lib import pg_token_stats  # noqa: F401  (without the feature: the import fails)
from plangen_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (5, 3), (1025, 3), (4099, 2)]


@pytest.mark.parametrize("V,B", SHAPES)
@pytest.mark.parametrize("temp", [0.0, 0.7])
def test_reference_agrees_with_torch_fp64(V, B, temp):
    for name, (y, tok) in SR.families(V, B, V + 1).items():
        if name not in SR.FINITE_FAMILIES:
            continue
        ref = SR.token_stats_ref(y, tok, temp, min(8, V))
        x = torch.from_numpy(np.stack([LR.scaled_row(r, temp) for r in y]))
        ls = torch.log_softmax(x, -1)
        assert np.allclose(ref["logprob"], ls[torch.arange(B), torch.from_numpy(tok).long()].numpy(), rtol=0, atol=1e-11), name
        assert np.allclose(ref["entropy"], torch.distributions.Categorical(logits=x).entropy().numpy(), rtol=0, atol=1e-11), name
        srt = torch.sort(x, dim=-1, descending=True, stable=True)            # stable: the lowest index first among equals
        k = min(8, V)
        assert np.array_equal(ref["alt_tok"], srt.indices[:, :k].numpy()), name
        assert np.allclose(ref["alt_logprob"], torch.gather(ls, 1, srt.indices[:, :k]).numpy(), rtol=0, atol=1e-11), name
        assert np.array_equal(ref["rank"], (x > x[torch.arange(B), torch.from_numpy(tok).long()][:, None]).sum(1).numpy()), name
    assert abs(SR.token_stats_ref(np.full((1, V), 1.5, np.float32), [0], temp)["entropy"][0] - np.log(V)) < 1e-12


def test_special_cases():
    inf = np.inf
    r = SR.token_stats_ref(np.array([[-inf, -inf, -inf]], np.float32), [1], 0.7, 8)
    assert r["entropy"][0] == 0 and r["rank"][0] == 3 and r["logprob"][0] == -inf and (r["alt_tok"] == -1).all() and np.isneginf(r["alt_logprob"]).all()
    r = SR.token_stats_ref(np.array([[inf, 2, inf, -1]], np.float32), [2], 0.0, 3)
    assert r["entropy"][0] == np.log(2) and r["rank"][0] == 0 and r["logprob"][0] == -np.log(2)
    assert r["alt_tok"].tolist() == [[0, 2, 1]] and r["alt_logprob"][0, 0] == -np.log(2) and r["alt_logprob"][0, 2] == -inf
    r = SR.token_stats_ref(np.array([[1, -inf, np.nan, 1]], np.float32), [1], 0.0, 4)
    assert r["rank"][0] == 4 and r["alt_tok"].tolist() == [[0, 3, -1, -1]] and abs(r["entropy"][0] - np.log(2)) < 1e-15
    assert SR.token_stats_ref(np.array([[1, 2, 3]], np.float32), [7], 0.0, 0)["rank"][0] == 3
    fin = SR.text_stats_ref(np.zeros((3, 1, 4), np.float32), np.array([[2, 9, 9]]), eos=9, n_alt=2)
    assert fin["logprob"][0, 2] == 0 and fin["entropy"][0, 2] == 0 and fin["rank"][0, 2] == 0 and (fin["alt_tok"][0, 2] == -1).all() \
        and (fin["alt_logprob"][0, 2] == 0).all() and fin["entropy"][0, 1] > 1 and fin["alt_tok"][0, 1].tolist() == [0, 1]


MUTANTS = {"bits": ("entropy", ("normal", "ties", "holes")), "ge": ("rank", ("normal", "ties", "flat")),
           "ascending": ("alt_tok", ("normal", "ties", "holes", "peaked")), "ties_high": ("alt_tok", ("ties", "flat")),
           "nan_on_holes": ("entropy", ("holes", "tok_on_neginf"))}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_comparison_rejects_planted_errors(mutant):
    V, B = 1025, 3
    fam = SR.families(V, B, 5)
    output, where = MUTANTS[mutant]
    for name in where:
        y, tok = fam[name]
        ref = SR.token_stats_ref(y, tok, 0.7, 8)
        assert SR.mismatches(ref, ref, V) == []
        wrong = SR.token_stats_ref(y, tok, 0.7, 8, **{mutant: True})
        assert output in SR.mismatches(wrong, ref, V), (mutant, name)


def test_derived_entropy_bound_holds_for_an_fp32_restatement():
    worst = 0.0
    for V in (5, 1025, 16384, 102400):
        for name, (y, tok) in SR.families(V, 2, V).items():
            for temp in (0.0, 0.7):
                for r in y:
                    err = abs(SR.two_pass_fp32(r, temp) - SR._entropy_of_x(LR.scaled_row(r, temp)))
                    worst = max(worst, err / SR.ent_tol(V))
                    assert err <= SR.ent_tol(V), (V, name, temp, err)
    print(f"fp32 two-pass entropy (sums of the kernel's shape): largest error / ent_tol(V) = {worst:.3f}")


def test_binding_matches_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plangen_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+pg_request_token_stats\s*\(\s*pg_handle h,\s*const pg_token_stats\*\s*req\s*\)\s*;", hdr)
    assert re.search(r"int\s+pg_op_token_stats\s*\(([^;]*)\)\s*;", hdr)
    m = re.search(r"typedef struct pg_token_stats \{(.*?)\} pg_token_stats;", hdr, flags=re.S)
    fields = re.findall(r"(float\*|int32_t\*|int32_t|int64_t)\s+([a-z_]+);", m.group(1))
    ctype = {"float*": C.c_void_p, "int32_t*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.pg_token_stats._fields_)
    sym = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert sym["pg_request_token_stats"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.pg_token_stats)])
    assert sym["pg_op_token_stats"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.POINTER(_lib.pg_token_stats), C.c_void_p])
    assert callable(Engine.token_stats)


def test_system_summaries():
    from plangen_amd.system import System
    ent = torch.tensor([[1.0, 3.0, 2.0, 0.0], [0.5, 0.5, 0.5, 0.5]])
    rank = torch.tensor([[0, 4, 7, 0], [0, 0, 1, 9]], dtype=torch.int32)
    forced = torch.tensor([[True, True, True, False], [False, False, False, False]])
    s = System.image_token_stats_summary(dict(entropy=ent, rank=rank), forced)
    assert s["mean_entropy"] == [1.5, 0.5] and s["mean_rank"] == [2.75, 2.5] and s["rank0_share"] == [0.5, 0.5]
    assert s["top1"] == [pytest.approx(1 / 3), None] and s["top5"] == [pytest.approx(2 / 3), None]
    assert set(System.image_token_stats_summary(dict(entropy=ent, rank=rank))) == {"mean_entropy", "mean_rank", "rank0_share"}
    toks = torch.tensor([[5, 9, 9, 9], [5, 6, 7, 8]])                         # eos = 9: row 0 owns two tokens, row 1 all four
    alt = torch.arange(2 * 4 * 2, dtype=torch.int32).view(2, 4, 2)
    t = System.text_token_stats_summary(toks, dict(entropy=ent, alt_tok=alt), 9)
    assert t["n_tokens"] == [2, 4] and t["mean_entropy"] == [2.0, 0.5] and t["alt_tok"][0] == [[0, 1], [2, 3]] and len(t["alt_tok"][1]) == 4
