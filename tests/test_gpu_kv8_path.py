"""GPU: the engine with the opt-in FP8 KV cache (Engine(..., kv_dtype="fp8")): cache contents, logits against the fp32 fixture with the
reference's own bf16 error plus the quantisation's own fp32 effect as the yardstick, equalities inside the mode, rejections, footprint."""
import json

import numpy as np
import pytest
import torch

import bf16ref
import kv8_ref
from conftest import get_engine, load_golden
from fullwidth_cfg import FULLW
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

SLOTS = 96 + 64          # get_engine: max_prompt 96 + the tiny config's 64 image tokens
ROWS = 8


def _golden():
    g = load_golden("sample_image_tiny.npz")
    return g, torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])


def _pad(mask, L):
    return (L - mask[:, :L].sum(-1)).tolist()


def _e8(tiny_cfg, tiny_weights):
    return get_engine(tiny_cfg, tiny_weights, "bf16", kv_dtype="fp8")


_REFQ = {}


def _image_loop_ref(tiny_weights, ocfg):
    """(sel, vsel, ref32, E_ref, D_q, lgq) of the tiny image fixture: E_ref as bf16ref.check_image_loop computes it, D_q from the fp32 oracle
    with the quantised cache, both at the fixture's selected steps and columns."""
    if not _REFQ:
        g, ids, mask = _golden()
        gref, _ = bf16ref.load("sample_image_tiny")
        G = torch.from_numpy(g["logits"])
        _, lgq = kv8_ref.sample_image_kv8(tiny_weights, ocfg, R.embed_tokens(tiny_weights, ids), mask, 5.0,
                                          force_tokens=torch.from_numpy(g["tokens"]), return_logits=True)
        sel, vsel = torch.from_numpy(gref["sel_steps"]).long(), torch.from_numpy(gref["vsel"]).long()
        ref32 = G[sel][:, :, vsel]
        _REFQ["v"] = (sel, vsel, ref32, (bf16ref.bf16_bits(gref["ref_bf16_sel_logits"]) - ref32).abs(), (lgq[sel][:, :, vsel] - ref32).abs())
    return _REFQ["v"]


def test_prefill_cache_is_the_quantised_bf16_cache(tiny_cfg, tiny_weights):
    g, ids, mask = _golden()
    L = ids.shape[1]
    pad = _pad(mask, L)
    eb, e8 = get_engine(tiny_cfg, tiny_weights, "bf16"), _e8(tiny_cfg, tiny_weights)
    hb = eb.prefill(ids, pad, position_mode=0, return_hidden=True)
    h8 = e8.prefill(ids, pad, position_mode=0, return_hidden=True)
    assert torch.equal(hb.view(torch.int32), h8.view(torch.int32)), "prefill attention stays exactly bf16"
    nh = tiny_cfg.n_heads
    n_el = ROWS * nh * SLOTS * 128
    for share in (0, 1):
        for e in (eb, e8):
            e.set_option("share_uncond", share)
            e.prefill(ids, pad, position_mode=0)
        for layer in range(tiny_cfg.n_layers):
            for nm, sn in (("kcache", "kscale"), ("vcache", "vscale")):
                ref = eb.debug_read(nm, layer, n_el, torch.bfloat16).cpu().view(ROWS, nh, SLOTS, 128)
                codes = e8.debug_read(nm, layer, n_el, torch.uint8).cpu().view(ROWS, nh, SLOTS, 128)
                scale = e8.debug_read(sn, layer, n_el // 128, torch.float32).cpu().view(ROWS, nh, SLOTS)
                for r in range(ids.shape[0]):
                    if share and r % 2 == 1 and r != 1:
                        continue                                     # aliases row 1's prompt: neither written nor converted
                    n = L - pad[r]
                    rc, rs = kv8_ref.quantize(ref[r, :, :n])
                    assert torch.equal(codes[r, :, :n], rc), (nm, layer, r, share)
                    assert torch.equal(scale[r, :, :n].view(torch.int32), rs.view(torch.int32)), (sn, layer, r, share)
    for e in (eb, e8):
        e.set_option("share_uncond", 1)


def test_teacher_forced_logits_within_reference_bf16_plus_quantisation(tiny_cfg, tiny_weights, ocfg):
    """E_hip8 = |engine(fp8 cache) - G| <= k (E_ref + D_q), statistic by statistic (tests/bf16ref.py: k = K on quantiles and the mean, K_MAX on
    the maximum): E_ref = the reference's own bf16 error on this fixture, D_q = what the quantised cache alone does to the fp32 oracle
    (kv8_ref.sample_image_kv8).  The sum is the triangle inequality over the two error sources: exact for the maximum and the mean,
    conservative for quantiles.  Nothing here was measured on this build."""
    g, ids, mask = _golden()
    pad = _pad(mask, ids.shape[1])
    gold_tok = torch.from_numpy(g["tokens"])
    G = torch.from_numpy(g["logits"])                                # [T, B, V] fp32
    e8, eb = _e8(tiny_cfg, tiny_weights), get_engine(tiny_cfg, tiny_weights, "bf16")
    e8.prefill(ids, pad, position_mode=0)
    toks8, lg8 = e8.decode_image_tokens(cfg_weight=5.0, temperature=0.0, force_tokens=gold_tok, return_logits=True)
    eb.prefill(ids, pad, position_mode=0)
    _, lgb = eb.decode_image_tokens(cfg_weight=5.0, temperature=0.0, force_tokens=gold_tok, return_logits=True)
    toks8, lg8, lgb = toks8.cpu(), lg8.cpu(), lgb.cpu()
    sel, vsel, ref32, E_ref, D_q = _image_loop_ref(tiny_weights, ocfg)
    E_hip8 = (lg8[sel][:, :, vsel] - ref32).abs()
    assert float(D_q.max()) > 0 and not torch.equal(lg8, lgb), "the mode is live"
    sh, sr, sq = bf16ref.err_stats(E_hip8), bf16ref.err_stats(E_ref), bf16ref.err_stats(D_q)
    ratios = {k: sh[k] / (sr[k] + sq[k]) for k in bf16ref.STATS}
    print("tiny fp8-KV teacher-forced:", json.dumps({"E_hip8": sh, "E_ref": sr, "D_q": sq, "E_hip8_over_(E_ref+D_q)": {k: round(v, 3) for k, v in ratios.items()},
                                                     "E_hip_bf16_cache": bf16ref.err_stats((lgb[sel][:, :, vsel] - ref32).abs())}))
    bad = {k: v for k, v in ratios.items() if v > (bf16ref.K_MAX if k == "max" else bf16ref.K)}
    assert not bad, bad
    top2 = G.topk(2, dim=-1).values
    decisive = (top2[..., 0] - top2[..., 1]) > 2 * bf16ref.K_MAX * (sr["max"] + sq["max"])        # [T, B]
    assert torch.equal(toks8.t()[decisive], gold_tok.t()[decisive])
    print(f"decisive steps {int(decisive.sum())} / {decisive.numel()}, agreement overall {(toks8 == gold_tok).float().mean():.3f}")


def test_equalities_inside_the_mode(tiny_cfg, tiny_weights):
    from plangen_amd.system import System
    g, ids, mask = _golden()
    pad = _pad(mask, ids.shape[1])
    e = _e8(tiny_cfg, tiny_weights)

    def run(**kw):
        e.prefill(ids, pad, position_mode=0)
        return e.decode_image_tokens(cfg_weight=5.0, **kw).cpu()
    try:
        base = run(temperature=0.0)
        e.set_option("use_graph", 1)
        assert torch.equal(run(temperature=0.0), base), "use_graph 1 == 0"
        samp_g = run(temperature=1.0, seed=11, top_k=20, top_p=0.9)
        e.set_option("use_graph", 0)
        samp = run(temperature=1.0, seed=11, top_k=20, top_p=0.9)
        assert torch.equal(samp, samp_g) and torch.equal(run(temperature=1.0, seed=11, top_k=20, top_p=0.9), samp), "filtered sampling is reproducible"
        assert not torch.equal(run(temperature=1.0, seed=12, top_k=20, top_p=0.9), samp)
        e.set_option("share_uncond", 0)
        assert torch.equal(run(temperature=0.0), base), "share_uncond 0 == 1"
    finally:
        e.set_option("share_uncond", 1)
        e.set_option("use_graph", 0)
    # forcing with an edit mask: masked-out positions are fed (and reported) from the forced tokens
    gen = torch.Generator().manual_seed(5)
    B, T = ids.shape[0] // 2, 16
    ft = torch.randint(0, tiny_cfg.img_vocab, (B, T), generator=gen).int()
    fm = (torch.rand(B, T, generator=gen) > 0.5).to(torch.uint8)
    e.prefill(ids, pad, position_mode=0)
    a = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=0.0, force_tokens=ft, force_mask=fm).cpu()
    e.prefill(ids, pad, position_mode=0)
    b = e.decode_image_tokens(T=T, cfg_weight=5.0, temperature=0.0, force_tokens=ft, force_mask=fm).cpu()
    assert torch.equal(a, b)
    # the stepwise facade loop (pg_prefill_embeds + pg_step + pg_gen_head) == the fused loop
    sysm = System(tiny_cfg, e)
    emb = sysm.vl_gpt.language_model.get_input_embeddings()(ids.to(e.device))
    step_toks = sysm.sample_image_stepwise(emb, mask.to(e.device), 5.0, n_tokens=12).cpu()
    assert torch.equal(step_toks.int(), base[:, :12].int())


def test_text_greedy_runs_and_agrees_where_the_oracle_is_decisive(tiny_cfg, tiny_weights, ocfg):
    """pg_generate_text_greedy over the fp8 cache: the ids equal the bf16-cache engine's at every step both engines
    reached on the same prefix and where the fp32 oracle's top-1 margin exceeds 2 K_MAX (E_ref.max + D_q.max), the image-loop test's bound."""
    from plangen_amd.system import System
    g = load_golden("generate_tiny.npz")
    ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
    n = 12
    outs = {}
    for name, e in (("bf16", get_engine(tiny_cfg, tiny_weights, "bf16")), ("fp8", _e8(tiny_cfg, tiny_weights))):
        sysm = System(tiny_cfg, e)
        emb = sysm.vl_gpt.language_model.get_input_embeddings()(ids.to(e.device))
        outs[name] = sysm.vl_gpt.language_model.generate(inputs_embeds=emb, attention_mask=mask.to(e.device), eos_token_id=tiny_cfg.eos_id,
                                                         max_new_tokens=n, min_new_tokens=n).cpu()
    assert outs["fp8"].shape == (ids.shape[0], n)
    emb = R.embed_tokens(tiny_weights, ids)
    _, lg = R.generate_text_greedy(tiny_weights, ocfg, emb, mask, n, tiny_cfg.eos_id, min_new_tokens=n, force_tokens=outs["bf16"], return_logits=True)
    lg = lg.permute(1, 0, 2).clone()
    lg[:, :, tiny_cfg.eos_id] = float("-inf")
    top2 = lg.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]                             # [B, n]
    _, _, _, E_ref, D_q = _image_loop_ref(tiny_weights, ocfg)
    bound = 2 * bf16ref.K_MAX * (float(E_ref.max()) + float(D_q.max()))
    same_prefix = torch.cumprod((outs["fp8"] == outs["bf16"]).long(), dim=1)
    prefix_ok = torch.cat([torch.ones_like(same_prefix[:, :1]), same_prefix[:, :-1]], 1).bool()   # step i saw identical inputs
    decisive = (margin > bound) & prefix_ok
    print(f"fp8-KV text greedy: agreement {(outs['fp8'] == outs['bf16']).float().mean():.3f}, decisive {int(decisive.sum())}/{decisive.numel()}, bound {bound:.4f}")
    assert torch.equal(outs["fp8"][decisive], outs["bf16"][decisive])


def test_rejections(tiny_cfg, tiny_weights):
    from plangen_amd.engine import Engine, PlanGenError
    with pytest.raises(PlanGenError):
        Engine(tiny_cfg, dtype="f32", max_rows=4, max_prompt=32, kv_dtype="fp8")
    with pytest.raises(PlanGenError):
        Engine(tiny_cfg, dtype="bf16", max_rows=4, max_prompt=32, kv_dtype="int4")
    g, ids, mask = _golden()
    e = _e8(tiny_cfg, tiny_weights)
    e.set_option("lanes", 2)
    try:
        e.prefill(ids, _pad(mask, ids.shape[1]), position_mode=0)
        with pytest.raises(PlanGenError, match="lanes"):
            e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0)
    finally:
        e.set_option("lanes", -1)
    e.prefill(ids, _pad(mask, ids.shape[1]), position_mode=0)
    assert e.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0).shape == (ids.shape[0] // 2, 4)


def test_footprint_full_width():
    """From the allocation list (engine_core.hip): the bf16 cache's n_layers * 2 * E * 2 bytes become n_layers * 2 * E codes plus
    n_layers * 2 * rows * heads * slots fp32 scales plus the 2 * E * 2-byte one-layer prefill scratch."""
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    cfg = PlanGenConfig(**dict(FULLW, n_layers=8))
    rows, prompt, new = 8, 64, 32
    kw = dict(dtype="bf16", max_rows=rows, max_prompt=prompt, max_new=new, max_images=2)
    eb, e8 = Engine(cfg, **kw), Engine(cfg, kv_dtype="fp8", **kw)
    try:
        slots = prompt + new
        E = rows * cfg.n_heads * slots * 128
        saved = eb.device_bytes() - e8.device_bytes()
        need = cfg.n_layers * 2 * E * (2 - 1) - 2 * E * 2 - 2 * cfg.n_layers * rows * cfg.n_heads * slots * 4 - (1 << 20)
        print(f"full-width 8 layers: bf16 cache engine {eb.device_bytes()} B, fp8 {e8.device_bytes()} B, saved {saved} >= {need}")
        assert need > 0 and saved >= need
    finally:
        eb.close(); e8.close()
