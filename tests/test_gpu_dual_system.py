"""GPU: dual guidance at the System level (cfg key cfg_weight_layout, System.t2i_dual) at the tiny config, PG_F32 greedy: uni_generate builds the triples,
prefills without the shared negative prompt, runs the three-row loop and VQ-decodes; the tokens are the engine's on the same triples and the oracle loop's; the
per-batch JSON carries the two weights; with the key unset the pair path gives the golden tokens as before."""
import json
import os

import numpy as np
import pytest
import torch

import dual_ref as U
from conftest import get_engine, load_golden
from oracle import ref_cpu as R
from plangen_amd.engine import PlanGenError

pytestmark = pytest.mark.gpu


def _system(cfg, weights, **keys):
    from plangen_amd.system import System
    s = System(cfg, get_engine(cfg, weights, "f32"))
    s.args.temperature = 0.0
    for k, v in keys.items():
        setattr(s.args, k, v)
    return s


def _batch(cfg, seed=3, n=2):
    from plangen_amd.system import pad_input_ids
    g = torch.Generator().manual_seed(seed)
    cond = [torch.randint(8, cfg.vocab, (k,), generator=g).tolist() for k in (9, 6)[:n]]
    caps = [c[:k] for c, k in zip(cond, (4, 5))]
    neg = torch.randint(8, cfg.vocab, (4,), generator=g).tolist()
    ids, mask = pad_input_ids(cond, cfg.pad_id)
    mask = torch.cat([mask, torch.ones((n, cfg.img_tokens), dtype=mask.dtype)], -1)
    return dict(uni_inputs_ids=ids, uni_attention_mask=mask, neg_inputs_ids=neg, caption_inputs_ids=caps), cond, caps, neg


def test_uni_generate_dual_end_to_end(tmp_path, tiny_cfg, tiny_weights, ocfg):
    batch, cond, caps, neg = _batch(tiny_cfg)
    s = _system(tiny_cfg, tiny_weights, cfg_weight=5.0, cfg_weight_layout=2.0)
    out = s.uni_generate(batch, gen_path=str(tmp_path), batch_idx=0, pred_layout=False, save_local=True)
    toks = out["pr_tokens"].cpu()
    T, S = tiny_cfg.img_tokens, tiny_cfg.img_size
    assert toks.shape == (2, T) and out["pr_image"].shape == (2, 3, S, S) and bool(torch.isfinite(out["pr_image"]).all())
    assert out["dual_guidance"] == dict(w_caption=5.0, w_layout=2.0) == s.last_dual_guidance
    rec = json.load(open(os.path.join(str(tmp_path), "0_layout.json")))
    assert rec["dual_guidance"] == dict(w_caption=5.0, w_layout=2.0) and "sample_plan" not in rec
    # the oracle loop on the same triples
    ids3, mask3 = U.collate_triples(cond, caps, neg, tiny_cfg.pad_id, T)
    want = U.sample_image_dual(tiny_weights, ocfg, R.embed_tokens(tiny_weights, ids3), mask3, 5.0, 2.0, n_tokens=16)
    assert torch.equal(toks[:, :16].int(), want)
    # the image is the VQ decode of those tokens
    dec = s.vl_gpt.gen_vision_model.decode_code(out["pr_tokens"].to(torch.int), shape=[2, tiny_cfg.img_dim, tiny_cfg.grid, tiny_cfg.grid])
    assert torch.equal(dec.float().cpu(), out["pr_image"].cpu())
    # the layout weight steers: another w_layout, other tokens; t2i_dual's arguments override the keys
    s.t2i_dual(ids3, mask3, w_layout=9.0)
    assert not torch.equal(s.last_generated_tokens.cpu(), toks) and s.last_dual_guidance["w_layout"] == 9.0
    s.t2i_dual(ids3, mask3, return_logprobs=True)
    assert torch.equal(s.last_generated_tokens.cpu(), toks) and s.last_logprobs.shape == (2, T) and bool((s.last_logprobs <= 0).all())
    s.t2i_dual(ids3, mask3)
    assert s.last_logprobs is None


def test_parallel_size_replicates_the_triples_and_forcing_holds(tiny_cfg, tiny_weights):
    batch, cond, caps, neg = _batch(tiny_cfg, n=1)
    g = torch.Generator().manual_seed(9)
    batch["image"] = torch.rand(1, 3, tiny_cfg.img_size, tiny_cfg.img_size, generator=g) * 2 - 1
    batch["edit_region"] = (torch.rand(1, tiny_cfg.img_tokens, generator=g) > 0.5).int()
    s = _system(tiny_cfg, tiny_weights, cfg_weight=5.0, cfg_weight_layout=2.0, parallel_size=2, use_teacher_forcing=True)
    out = s.uni_generate(batch, pred_layout=False)
    toks = out["pr_tokens"].cpu().int()
    assert toks.shape == (2, tiny_cfg.img_tokens) and out["pr_image"].shape[0] == 2 and out["edit_mask"] is not None
    labels = get_engine(tiny_cfg, tiny_weights, "f32").vq_encode(batch["image"]).reshape(1, -1).cpu().int()
    keep = batch["edit_region"][0] == 0
    assert torch.equal(toks[0][keep], labels[0][keep])                      # the first replica is forced where the region is 0 ...
    s1 = _system(tiny_cfg, tiny_weights, cfg_weight=5.0, cfg_weight_layout=2.0, parallel_size=2)
    free = s1.uni_generate({k: v for k, v in batch.items() if k not in ("image", "edit_region")}, pred_layout=False)["pr_tokens"].cpu().int()
    assert torch.equal(toks[1], free[1])                                     # ... and the second runs free: greedy, the unforced image of the same batch shape
    assert not torch.equal(toks[0], free[0])


def test_key_unset_takes_the_pair_path(tiny_cfg, tiny_weights):
    g = load_golden("sample_image_tiny.npz")
    ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
    for keys in (dict(), dict(cfg_weight_layout=None)):
        s = _system(tiny_cfg, tiny_weights, cfg_weight=5.0, **keys)
        s.t2i(ids, mask)
        assert np.array_equal(s.last_generated_tokens.cpu().numpy(), g["tokens"])
        L = ids.shape[1]
        cond = [ids[r][mask[r, :L].bool()].tolist() for r in range(0, ids.shape[0], 2)]
        from plangen_amd.system import pad_input_ids
        ci, cm = pad_input_ids(cond, tiny_cfg.pad_id)
        cm = torch.cat([cm, torch.ones((len(cond), tiny_cfg.img_tokens), dtype=cm.dtype)], -1)
        out = s.uni_generate(dict(uni_inputs_ids=ci, uni_attention_mask=cm, neg_inputs_ids=ids[1][mask[1, :L].bool()].tolist()), pred_layout=False)
        assert np.array_equal(out["pr_tokens"].cpu().numpy(), g["tokens"]) and "dual_guidance" not in out and s.last_dual_guidance is None


@pytest.mark.parametrize("key,value,extra", [("share_replicas", 1, {"parallel_size": 2}), ("cfg_weight_end", 1.0, {"cfg_schedule": "linear"}),
                                             ("prefill_forced_prefix", True, {}), ("select_best", True, {"parallel_size": 2}), ("token_stats", True, {}),
                                             ("score_gt_image", True, {})])
def test_refusals_by_key_leave_the_engine_usable(tiny_cfg, tiny_weights, key, value, extra):
    batch, *_ = _batch(tiny_cfg)
    s = _system(tiny_cfg, tiny_weights, cfg_weight_layout=2.0, **{key: value}, **extra)
    with pytest.raises(PlanGenError, match=key):
        s.uni_generate(batch, pred_layout=False)
    s = _system(tiny_cfg, tiny_weights, cfg_weight_layout=2.0, parallel_size=2)
    with pytest.raises(PlanGenError, match="max_rows"):                     # 3 x 2 x 2 = 12 rows > 8
        s.uni_generate(batch, pred_layout=False)
    s = _system(tiny_cfg, tiny_weights, cfg_weight_layout=2.0)
    assert s.uni_generate(batch, pred_layout=False)["pr_tokens"].shape == (2, tiny_cfg.img_tokens)
