"""GPU: the System-level users of pg_prefill_extend / pg_rewind at the tiny config, PG_F32 greedy.

* ``prefill_forced_prefix=True`` against False on a tiny edit batch: identical tokens, positions < t0 are the ground-truth codes,
  ``forced_prefix`` in the per-batch JSON; the key combinations it refuses.
* ``mmu_ask`` with two questions against two independent ``mmu`` runs: identical ids."""
import json
import os

import pytest
import torch

from conftest import get_engine
from plangen_amd.engine import PlanGenError

pytestmark = pytest.mark.gpu


def _edit_batch(cfg, seed=3, first=(21, 30)):
    """Two prompts, a ground-truth image and edit regions whose first edited cells are ``first`` (t0 = their minimum)."""
    from plangen_amd.system import pad_input_ids
    g = torch.Generator().manual_seed(seed)
    cond = [torch.randint(8, cfg.vocab, (n,), generator=g).tolist() for n in (6, 9)]
    neg = torch.randint(8, cfg.vocab, (4,), generator=g).tolist()
    gt = torch.rand(2, 3, cfg.img_size, cfg.img_size, generator=g) * 2 - 1
    region = torch.zeros(2, cfg.img_tokens, dtype=torch.int32)
    for b, f in enumerate(first):
        region[b, f:] = (torch.rand(cfg.img_tokens - f, generator=g) > 0.4).int()
        region[b, f] = 1
    ids, mask = pad_input_ids(cond, cfg.pad_id)
    mask = torch.cat([mask, torch.ones((2, cfg.img_tokens), dtype=mask.dtype)], -1)
    return dict(uni_inputs_ids=ids, uni_attention_mask=mask, neg_inputs_ids=neg, image=gt, edit_region=region, base_caption=["a", "b"])


def _system(cfg, weights, **keys):
    from plangen_amd.system import System
    s = System(cfg, get_engine(cfg, weights, "f32"))
    s.args.use_teacher_forcing, s.args.temperature = True, 0.0
    for k, v in keys.items():
        setattr(s.args, k, v)
    return s


def test_forced_prefix_gives_the_unaccelerated_tokens(tmp_path, tiny_cfg, tiny_weights):
    batch = _edit_batch(tiny_cfg)
    outs = {}
    for on in (False, True):
        s = _system(tiny_cfg, tiny_weights, prefill_forced_prefix=on)
        out = s.uni_generate(batch, gen_path=str(tmp_path / str(on)), batch_idx=0, pred_layout=False, save_local=True)
        outs[on] = out["pr_tokens"].cpu()
        rec = json.load(open(os.path.join(str(tmp_path / str(on)), "0_layout.json")))
        if on:
            assert out["forced_prefix"] == 21 == s.last_forced_prefix and rec["forced_prefix"] == 21
        else:
            assert "forced_prefix" not in out and "forced_prefix" not in rec
    assert torch.equal(outs[True], outs[False])
    labels = get_engine(tiny_cfg, tiny_weights, "f32").vq_encode(batch["image"]).reshape(2, -1).cpu().int()
    assert torch.equal(outs[True][:, :21].int(), labels[:, :21])
    keep = batch["edit_region"] == 0
    assert torch.equal(outs[True].int()[keep], labels[keep])


def test_forced_prefix_edges(tiny_cfg, tiny_weights):
    """A region that starts at cell 0 leaves nothing to prefill (t0 = 0: the plain loop); an all-zero region keeps one step in the loop."""
    T = tiny_cfg.img_tokens
    for first, want in (((0, 30), 0), ((T, T), T - 1)):
        batch = _edit_batch(tiny_cfg, seed=4, first=(min(first[0], T - 1), min(first[1], T - 1)))
        if first[0] == T:
            batch["edit_region"].zero_()
        toks = {}
        for on in (False, True):
            s = _system(tiny_cfg, tiny_weights, prefill_forced_prefix=on)
            s.uni_generate(batch, pred_layout=False)
            toks[on] = s.last_generated_tokens.cpu()
        assert s.last_forced_prefix == want
        assert torch.equal(toks[True], toks[False])


@pytest.mark.parametrize("key,value", [("select_best", True), ("token_stats", True), ("return_logprobs", True), ("cfg_weight_end", 1.0), ("share_replicas", 1)])
def test_forced_prefix_refuses_what_it_cannot_serve(tiny_cfg, tiny_weights, key, value):
    extra = {"parallel_size": 2} if key in ("select_best", "share_replicas") else {}
    if key == "cfg_weight_end":
        extra["cfg_schedule"] = "linear"
    s = _system(tiny_cfg, tiny_weights, prefill_forced_prefix=True, **{key: value}, **extra)
    with pytest.raises(PlanGenError, match="prefill_forced_prefix cannot be combined"):
        s.uni_generate(_edit_batch(tiny_cfg), pred_layout=False)
    # ... and is ignored, as documented, without teacher forcing
    s.args.use_teacher_forcing = False
    setattr(s.args, key, False if value is True else (None if key == "cfg_weight_end" else 0))
    s.args.cfg_schedule = "constant"
    s.args.parallel_size = 1
    s.uni_generate(_edit_batch(tiny_cfg), pred_layout=False)
    assert s.last_forced_prefix is None


def _mmu_batch(cfg, tails, seed=3):
    """Rows [bos, <image slots>, tail...] left-padded, as the mmu collate builds them; rows 0 / 1 have different tails per question."""
    P = cfg.vit_tokens
    g = torch.Generator().manual_seed(seed)
    px = torch.rand(2, 1, 3, cfg.vit_img, cfg.vit_img, generator=g) * 2 - 1
    rows = [[1] + [0] * P + t for t in tails]
    Lp = max(len(r) for r in rows)
    ids = torch.full((2, Lp), cfg.pad_id, dtype=torch.long)
    seq = torch.zeros((2, Lp), dtype=torch.bool)
    attn = torch.zeros((2, Lp), dtype=torch.int32)
    for i, row in enumerate(rows):
        o = Lp - len(row)
        ids[i, o:] = torch.tensor(row)
        seq[i, o + 1:o + 1 + P] = True
        attn[i, o:] = 1
    return dict(input_ids=ids, pixel_values=px, images_seq_mask=seq, images_emb_mask=torch.ones((2, 1, P), dtype=torch.bool), attention_mask=attn)


def test_mmu_ask_equals_independent_mmu_runs(tiny_cfg, tiny_weights):
    from plangen_amd.system import System
    s = System(tiny_cfg, get_engine(tiny_cfg, tiny_weights, "f32"))
    qs = [_mmu_batch(tiny_cfg, t) for t in ([[20, 21, 22], [23]], [[30], [31, 32, 33, 34, 35]])]
    want = [s.uni_generate(dict(prepare_inputs_infer=q), pred_image=False, is_mmu=True, max_new_tokens=10)["pr_text_ids"].cpu() for q in qs]
    answers = s.mmu_ask(dict(prepare_inputs_infer=qs[0]), qs, max_new_tokens=10)
    assert len(answers) == 2 and all(len(a) == 2 for a in answers)
    for got, ref in zip(s.last_ask_ids, want):
        assert torch.equal(got.cpu(), ref)
    # a question whose rows disagree with question 0 in front of the image block's end is refused
    bad = dict(qs[1]); bad["input_ids"] = qs[1]["input_ids"].clone()
    o = int((bad["attention_mask"][0] == 0).sum())
    bad["input_ids"][0, o] = 2
    with pytest.raises(PlanGenError, match="differs from question 0"):
        s.mmu_ask(dict(prepare_inputs_infer=qs[0]), [qs[0], bad], max_new_tokens=4)
