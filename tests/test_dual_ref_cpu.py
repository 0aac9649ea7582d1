"""CPU: the host model of the dual-guidance sampler step (tests/dual_ref.py).  Its power is shown with planted mutants: each wrong reading of the
definition must be caught by the comparison tests/test_gpu_dual_ops.py makes (the mixed row bit for bit, every decided draw, every greedy token) on the
families that test uses; and the model alone, with draw_ref.E_G_CPU, must leave at most draw_ref.UNDECIDED_CAP of each family's sampled draws undecided.
Also the three-row oracle loop against the oracle's own pair loop in the degenerate cases, and the ABI surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import draw_ref as D
import dual_ref as U
from oracle import ref_cpu as O
from plangen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _family(V, S):
    """[(case, step, model outputs)] of one parametrisation, computed once and shared."""
    if (V, S) not in _CACHE:
        _CACHE[(V, S)] = [(c, step, U.case_model(c, step)) for c in U.dual_cases(V, S) for step in c["steps"]]
    return _CACHE[(V, S)]


@pytest.mark.parametrize("S", U.DUAL_S)
@pytest.mark.parametrize("V", U.DUAL_V)
def test_model_alone_stays_inside_the_undecided_cap(V, S):
    n = open_ = greedy = flt = 0
    for c, step, (mixed, tok, gap, scale, ru, keep) in _family(V, S):
        assert (mixed == mixed.astype(np.float32)).all()                 # dyadic slabs and weights: the fp32 row is the fp64 row
        if c["T"] <= 0:
            greedy += len(tok)
            continue
        dec = D.decided(gap, scale, D.E_G_CPU)
        n += dec.size; open_ += int((~dec).sum()); flt += int(keep is not None)
    print(f"dual V={V} S={S}: {open_} of {n} sampled draws open; {greedy} greedy")
    assert greedy > 0 and n > 0
    assert (flt > 0) == (V >= 1000)
    assert open_ <= D.UNDECIDED_CAP * n, (open_, n)


def _caught(V, S, mutant):
    for c, step, (mixed, tok, gap, scale, ru, keep) in _family(V, S):
        m_mixed, m_tok, *_ = U.case_model(c, step, mutant)
        if not np.array_equal(m_mixed, mixed):
            return True
        binding = D.decided(gap, scale, D.E_G_CPU) if c["T"] > 0 else np.ones(len(tok), dtype=bool)
        if (binding & (m_tok != tok)).any():
            return True
    return False


@pytest.mark.parametrize("mutant", U.MUTANTS)
def test_every_planted_mutant_is_caught(mutant):
    """Every mutant changes the mixed row itself, so it shows on every family, V = 1 included."""
    for V in U.DUAL_V:
        for S in U.DUAL_S:
            assert _caught(V, S, mutant), (mutant, V, S)


def test_families_cover_what_the_operator_test_names():
    assert U.DUAL_T == 576 and set(D.IMG_CASE_STEPS) >= {0, 1, 2, 3, 574, 575}
    assert all(wc != wl for wc, wl in U.DUAL_W)
    offs = {(c["b_off"], c["B_total"]) for c in U.dual_cases(17, 1)}
    assert any(b > 0 and n > b + U.DUAL_B for b, n in offs) and any(b == 0 for b, _ in offs)
    assert 16384 % (4 * 256 * U.CHUNKS) == 0 and 1000 % U.CHUNKS != 0 and 17 % U.CHUNKS != 0      # full passes, and ragged last chunks


def test_degenerate_cases_are_the_pair_mix():
    rng = np.random.default_rng(5)
    f, p, u = (rng.standard_normal((3, 40)) for _ in range(3))
    assert np.array_equal(U.mix(f, f, u, 5.0, 9.0), D.cfg_mix(f, u, 5.0))          # p == f: the pair result at w_caption
    assert np.array_equal(U.mix(f, u, u, 5.0, 9.0), D.cfg_mix(f, u, 9.0))          # p == u: the pair result at w_layout
    assert np.allclose(U.mix(f, p, u, 3.0, 3.0), D.cfg_mix(f, u, 3.0), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- the oracle loop
def _tiny():
    cfg = O.OracleCfg()
    return cfg, O.make_weights(cfg, seed=0)


def test_oracle_loop_degenerates_to_the_pair_loop():
    """Caption rows equal to the full rows: the three-row loop at (w_caption, anything) emits what oracle.ref_cpu.sample_image emits at w_caption, with
    forcing and with the edit region."""
    cfg, W = _tiny()
    g = torch.Generator().manual_seed(3)
    B, T = 2, 5
    full = [torch.randint(3, cfg.vocab, (n,), generator=g).tolist() for n in (7, 4)]
    neg = torch.randint(3, cfg.vocab, (3,), generator=g).tolist()
    ids2, mask2 = O.t2i_infer_collate_batch(full, neg, 0, T)
    ids3, mask3 = U.collate_triples(full, full, neg, 0, T)
    assert ids3.shape == (3 * B, ids2.shape[1]) and torch.equal(ids3[0::3], ids2[0::2]) and torch.equal(ids3[1::3], ids2[0::2]) and torch.equal(ids3[2::3], ids2[1::2])
    assert torch.equal(mask3[0::3], mask2[0::2]) and torch.equal(mask3[2::3], mask2[1::2])
    e2, e3 = O.embed_tokens(W, ids2), O.embed_tokens(W, ids3)
    force = torch.randint(0, cfg.img_vocab, (B, T), generator=g, dtype=torch.int32)
    region = torch.tensor([[1, 0, 1, 0, 1], [0, 0, 1, 1, 1]])
    for kw in (dict(), dict(force_tokens=force), dict(edit_region=region, gt_labels=force)):
        t2, l2 = O.sample_image(W, cfg, e2, mask2, 5.0, T, return_logits=True, **kw)
        t3, l3 = U.sample_image_dual(W, cfg, e3, mask3, 5.0, 2.0, T, return_logits=True, **kw)
        # six rows against four: the host BLAS sums in another order; 2e-3 is the project's bound for fp32 reassociation (test_gpu_path.LOGIT_TOL_F32)
        assert torch.equal(t2, t3) and torch.allclose(l2, l3, rtol=0, atol=2e-3)
    t3 = U.sample_image_dual(W, cfg, e3, mask3, 5.0, 2.0, T, edit_region=region, gt_labels=force)
    assert torch.equal(t3[region == 0], force[region == 0])


# ---------------------------------------------------------------------------------------------------------------- ABI surface
def test_entry_point_in_header_map_and_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    assert re.search(r"int\s+pg_decode_image_tokens_dual\s*\(\s*pg_handle h,\s*int T,\s*float w_caption,\s*float w_layout,\s*float temperature,\s*int32_t top_k,"
                     r"\s*float top_p,\s*uint64_t seed,\s*const int32_t\*\s*force_tok_dev,\s*const uint8_t\*\s*force_mask_dev,\s*int32_t\*\s*out_tok_dev,"
                     r"\s*float\*\s*logits_out_dev,\s*pg_stream s\s*\)\s*;", hdr)
    assert "pg_decode_image_tokens_dual;" in open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    sym = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    P = C.c_void_p
    assert sym["pg_decode_image_tokens_dual"] == (C.c_int, [P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_uint64, P, P, P, P, P])
    assert "pg_diag_op_cfg3_sample" in open(os.path.join(ROOT, "plangen_amd", "csrc", "diag_ops.hip")).read()
