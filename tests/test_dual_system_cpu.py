"""CPU: the host side of dual guidance in System -- the collate of triples, the caption-only prompt through the offline tokenizer, and the cfg
keys the dual path refuses by name before anything reaches the engine (a stub engine stands in: nothing here launches)."""
from types import SimpleNamespace

import pytest
import torch

from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import PlanGenError
from plangen_amd.system import System, t2i_dual_collate_batch, t2i_infer_collate_batch
from plangen_amd.textproc import TagWordCodec


def _system(codec=None, **keys):
    cfg = PlanGenConfig.tiny()
    eng = SimpleNamespace(device="cpu", max_rows=8, dtype="f32", cfg=cfg)
    s = System(cfg, eng, codec=codec)
    for k, v in keys.items():
        setattr(s.args, k, v)
    return s


def test_collate_of_triples_row_order_and_mask():
    cond = [[11, 12, 13, 14, 15], [21, 22]]
    caps = [[11, 12], [21, 22, 23, 24, 25, 26]]
    neg = [91, 92, 93]
    ids, mask = t2i_dual_collate_batch(cond, caps, neg, 3, 4)
    assert ids.shape == (6, 6) and mask.shape == (6, 10) and ids.dtype == torch.int32
    want = [cond[0], caps[0], neg, cond[1], caps[1], neg]
    for r, row in enumerate(want):
        n = len(row)
        assert ids[r, 6 - n:].tolist() == row and (ids[r, :6 - n] == 3).all()                       # left-padded to the longest row of all
        assert mask[r].tolist() == [0] * (6 - n) + [1] * n + [1] * 4                                  # image part all ones
    # one negative prompt per sample; the f and u rows are the pair collate's rows
    ids2, mask2 = t2i_dual_collate_batch(cond, caps, [[91], [92, 93]], 3, 4)
    assert ids2[2, -1:].tolist() == [91] and ids2[5, -2:].tolist() == [92, 93]
    pi, pm = t2i_infer_collate_batch(cond, neg, 3, 4)
    wide = t2i_dual_collate_batch(cond, [c[:2] for c in caps], neg, 3, 4)
    assert torch.equal(wide[0][0::3], pi[0::2]) and torch.equal(wide[0][2::3], pi[1::2]) and torch.equal(wide[1][0::3], pm[0::2])
    with pytest.raises(PlanGenError):
        t2i_dual_collate_batch(cond, caps[:1], neg, 3, 4)
    with pytest.raises(PlanGenError):
        t2i_dual_collate_batch(cond, caps, [[91]], 3, 4)


def _batch(s, captions, layouts):
    from plangen_amd.system import pad_input_ids
    rows = [s.wrap_uni_prompt(c, g)[1].tolist() for c, g in zip(captions, layouts)]
    ids, mask = pad_input_ids(rows, s.cfg.pad_id)
    mask = torch.cat([mask, torch.ones((len(rows), s.cfg.img_tokens), dtype=mask.dtype)], -1)
    return dict(uni_inputs_ids=ids, uni_attention_mask=mask, base_caption=list(captions)), rows


def test_caption_only_prompt_is_the_absent_layout_form():
    codec = TagWordCodec(512, eos_id=7, pad_id=3)
    s = _system(codec, cfg_weight_layout=2.0, neg_prompt="blurry")
    captions = ["a cat on a mat", "two dogs"]
    layouts = ["<ref>a cat</ref><box>[12,40,500,620]</box>", "<ref>dogs</ref><box>[1,2,3,4]</box>"]
    batch, rows = _batch(s, captions, layouts)
    ids3, mask3 = s._cfg_prompt_dual(batch)
    L = ids3.shape[1]
    unpad = lambda r: ids3[r][mask3[r, :L].bool()].tolist()
    neg = s.wrap_uni_prompt("blurry", "")[1].tolist()
    for i in range(2):
        cap = s.wrap_uni_prompt(captions[i], "")[1].tolist()
        assert unpad(3 * i) == rows[i] and unpad(3 * i + 1) == cap and unpad(3 * i + 2) == neg
        text = s.decode_text(cap)
        assert captions[i] in text and "<box>" not in text and "<box>" in s.decode_text(rows[i])
        assert len(cap) < len(rows[i])
    assert mask3.shape == (6, L + s.cfg.img_tokens) and bool((mask3[:, L:] == 1).all())
    # ids override the tokenizer, and without either the key is refused by name
    over = dict(batch, caption_inputs_ids=[[40, 41], torch.tensor([42])])
    ids4, mask4 = s._cfg_prompt_dual(over)
    assert ids4[1, -2:].tolist() == [40, 41] and ids4[4, -1:].tolist() == [42]
    s2 = _system(None, cfg_weight_layout=2.0)
    b2 = {k: v for k, v in batch.items() if k != "base_caption"}
    b2["neg_inputs_ids"] = neg
    with pytest.raises(PlanGenError, match="cfg_weight_layout"):
        s2._cfg_prompt_dual(b2)
    with pytest.raises(PlanGenError, match="cfg_weight_layout"):
        s._cfg_prompt_dual(dict(batch, caption_inputs_ids=[[40]]))


def test_key_off_by_default_and_by_none():
    assert _system().dual_weight_layout() is None and _system(cfg_weight_layout=None).dual_weight_layout() is None
    assert _system(cfg_weight_layout=0).dual_weight_layout() == 0.0 and _system(cfg_weight_layout="2.5").dual_weight_layout() == 2.5


@pytest.mark.parametrize("key,value,extra", [("share_replicas", 1, {"parallel_size": 2}), ("cfg_weight_end", 1.0, {"cfg_schedule": "linear"}), ("same_noise", True, {}),
                                             ("temperatures", [1.0], {}), ("prefill_forced_prefix", True, {}), ("select_best", True, {"parallel_size": 2}),
                                             ("token_stats", True, {}), ("token_stats", 2, {}), ("score_gt_image", True, {})])
def test_refused_keys_are_named_before_anything_runs(key, value, extra):
    s = _system(None, cfg_weight_layout=2.0, **{key: value}, **extra)
    ids = torch.zeros((3, 4), dtype=torch.int32)
    mask = torch.ones((3, 4 + s.cfg.img_tokens), dtype=torch.int32)
    with pytest.raises(PlanGenError, match=key):                           # the stub engine has no prefill: reaching it would be an AttributeError
        s.t2i_dual(ids, mask)
    with pytest.raises(PlanGenError, match="cfg_weight_layout"):
        s.uni_generate(dict(uni_inputs_ids=ids[:1], uni_attention_mask=mask[:1], neg_inputs_ids=[5], caption_inputs_ids=[[6]]), pred_layout=False)


def test_too_many_rows_and_broken_triples_are_refused():
    s = _system(None, cfg_weight_layout=2.0)
    T = s.cfg.img_tokens
    with pytest.raises(PlanGenError, match="max_rows"):
        s.t2i_dual(torch.zeros((9, 4), dtype=torch.int32), torch.ones((9, 4 + T), dtype=torch.int32))
    with pytest.raises(PlanGenError, match="max_rows"):
        s.t2i_dual(torch.zeros((6, 4), dtype=torch.int32), torch.ones((6, 4 + T), dtype=torch.int32), parallel_size=2)
    with pytest.raises(PlanGenError, match="triples"):
        s.t2i_dual(torch.zeros((4, 4), dtype=torch.int32), torch.ones((4, 4 + T), dtype=torch.int32))
    s.args.cfg_weight_layout = None
    with pytest.raises(PlanGenError, match="w_layout"):
        s.t2i_dual(torch.zeros((3, 4), dtype=torch.int32), torch.ones((3, 4 + T), dtype=torch.int32))
