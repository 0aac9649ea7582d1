"""GPU: the text paths on the real codec path -- an ``HFCodec`` over tokenizer files shaped like a checkpoint's, extended the way the
reference extends its tokenizer (plangen_base.py:110-127).  The constrained decode under the automaton compiled from that codec, the
stage-1 -> stage-2 hand-off's prompt ids, and the embedding rows of the added ids.  Ids, masks and states are integers and the
embedding rows are copies: every comparison is exact, against a tokenizer prepared by tok_fixtures.reference_prepared and the numpy
restatement of the constrained step (text_dfa_ref.py)."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import get_engine, load_golden
from oracle import ref_cpu as R
from test_gpu_text_sampling import _prefill
from text_dfa_ref import accepts_layout, allowed_mask, greedy_step, n_items
from tok_fixtures import SPECIAL_ORDER, plain_hf_tokenizer_dir, reference_prepared

pytestmark = pytest.mark.gpu

MAX_NEW = 48
BOS_TAG, EOS_TAG = "<｜begin▁of▁sentence｜>", "<｜end▁of▁sentence｜>"


@pytest.fixture(scope="module")
def hf(tmp_path_factory, tiny_cfg):
    """(extended HFCodec, the reference-prepared tokenizer, the layout automaton over the codec's vocabulary)"""
    from plangen_amd.grammar import layout_token_dfa
    from plangen_amd.textproc import HFCodec
    d = plain_hf_tokenizer_dir(tmp_path_factory.mktemp("plain"))
    codec, oracle = HFCodec(d, special_tokens=True), reference_prepared(d, True, False)
    assert len(codec) == len(oracle) <= tiny_cfg.vocab
    return codec, oracle, layout_token_dfa(codec, tiny_cfg.vocab)


def _walk(dfa, ids, state=None):
    st = dfa.start_state if state is None else state
    for t in ids:
        st = int(dfa.next_state[st, dfa.token_class[t]])
        assert st >= 0, t
    return st


# ----------------------------------------------------------------------------------------------------------------- 1
def test_constrained_decode_writes_layouts_with_the_added_tokens(hf, tiny_cfg, tiny_weights):
    from plangen_amd.textproc import GROUNDING_OPEN, cut_plan_text, trans_gr_to_creati
    codec, oracle, dfa = hf
    e, g = get_engine(tiny_cfg, tiny_weights, "f32"), load_golden("generate_tiny.npz")
    e.set_text_dfa(dfa)
    eos = codec.eos_token_id
    tag_id = {t: oracle.convert_tokens_to_ids(t) for t in SPECIAL_ORDER}
    rows4 = [i % g["ids"].shape[0] for i in range(4)]
    items = 0
    for kw in (dict(), dict(temperature=1.5, seed=17), dict(temperature=1.5, seed=18), dict(temperature=1.5, seed=19)):
        _prefill(e, g, rows4)
        out = e.generate_text_constrained(MAX_NEW, eos, **kw).cpu()
        assert out.shape[0] == 4 and out.shape[1] <= MAX_NEW
        for row in out.tolist():
            assert eos in row and max(row) < len(codec), row
            body = row[:row.index(eos)]
            text = codec.decode(body)
            assert accepts_layout(text), text                              # the regular-expression acceptor of the layout language
            assert dfa.dist[_walk(dfa, body + [eos])] == 0
            assert cut_plan_text(codec.decode(row)) == GROUNDING_OPEN + text
            boxes, descs = trans_gr_to_creati(GROUNDING_OPEN + text)
            assert len(boxes) == len(descs) == n_items(text)
            for t, i in tag_id.items():                                    # every tag in the text is ONE id, the reference tokenizer's
                assert body.count(i) == text.count(t), (t, text)
            items += len(boxes)
    assert items > 0                                                       # the sampled runs do write items: the tag checks saw tags


def test_constrained_step_on_the_hf_tables_equals_the_restatement(hf, tiny_cfg, tiny_weights):
    """pg_op_text_constrain on the tables compiled from the HFCodec at three places of a layout: just after ``<box>``, inside a number,
    and where the budget leaves only the shortest way out (remaining == dist)."""
    codec, oracle, dfa = hf
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    e.set_text_dfa(dfa)
    eos, V = codec.eos_token_id, tiny_cfg.vocab
    ids = oracle.encode("<ref>a cat</ref><box>[12")[1:]
    k = ids.index(oracle.convert_tokens_to_ids("<box>"))
    s_box, s_num = _walk(dfa, ids[:k + 1]), _walk(dfa, ids)
    assert ids.count(oracle.convert_tokens_to_ids("<box>")) == 1 and len(ids) > k + 2
    x = torch.randn(3, V, generator=torch.Generator().manual_seed(406)) * 2.4
    cases = [(0, s_box, MAX_NEW), (1, s_num, MAX_NEW), (2, s_num, int(dfa.dist[s_num]))]
    kept = {}
    for extra in (dict(), dict(temperature=1.5, seed=7, step=3)):
        for b, s, remaining in cases:
            keep, tok, nxt = (t.cpu().numpy() for t in e.text_constrain(x[b:b + 1], [s], remaining, eos, **extra))
            ok, rt, rs = greedy_step(x[b].numpy(), dfa.token_class, dfa.next_state, dfa.dist, s, remaining, eos)
            assert np.array_equal(keep[0], ok) and ok.any(), (b, extra)
            assert np.array_equal(ok, allowed_mask(dfa.token_class, dfa.next_state, dfa.dist, s, remaining, V))
            if not extra:
                assert (int(tok[0]), int(nxt[0])) == (rt, rs), (b, tok, rt)
            else:
                assert ok[tok[0]] and int(nxt[0]) == int(dfa.next_state[s, dfa.token_class[tok[0]]])
            kept[b] = np.nonzero(ok)[0]
    strings = codec.token_strings(V)
    assert all(strings[i].startswith("[") for i in kept[0]) and len(kept[0]) >= 1                   # after <box>: only "[" ...
    assert all(strings[i][0] in "0123456789," for i in kept[1]) and len(kept[1]) > len(kept[2])     # inside the number: digits or the comma
    assert set(kept[2]) < set(kept[1])                                                               # the budget rule cut the set down
    assert all(dfa.dist[dfa.next_state[s_num, dfa.token_class[i]]] == dfa.dist[s_num] - 1 for i in kept[2])


# ----------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("pred_image", [True, False], ids=["uni_2stage", "plan"])
def test_stage2_prompt_ids_equal_the_reference_tokenizers(hf, tiny_cfg, tiny_weights, pred_image):
    """uni_generate's stage-1 -> stage-2 route with the layouts forced: what reaches Engine.prefill for the image stage is, id for id, the
    reference tokenizer's encoding of the reference's prompt (plangen_base.py:232-261) around the decoded layout (:296-306)."""
    from plangen_amd.system import System
    codec, oracle, _ = hf
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    cfg = dataclasses.replace(tiny_cfg, eos_id=codec.eos_token_id, pad_id=codec.pad_id)      # what the CLI System does with an HFCodec
    captions = ["a red cat on the table", "two dogs <ref> playing"]
    layouts = ["<ref>a cat</ref><box>[12,40,500,620]</box><ref>the table</ref><box>[0, 7, 999, 1000]</box></grounding>",
               "<ref>two dogs</ref><box>[1,2,300,400]</box></grounding> junk after the end"]
    eos = oracle.eos_token_id
    forced = [oracle.encode(t)[1:] + [eos] for t in layouts]
    forced = torch.tensor([r + [eos] * (max(map(len, forced)) - len(r)) for r in forced])
    s = System(cfg, e, SimpleNamespace(seed=3, parallel_size=1, cfg_weight=5.0, temperature=0.0, use_teacher_forcing=False, debug_max_seq_len=None,
                                       janus_hw=cfg.img_size, neg_prompt="", use_neg_box=False), codec=codec)
    ids1, mask1 = s.pad_input_ids([s.wrap_uni_prompt(c, "<grounding>", in_stage1=True)[1].tolist() for c in captions])
    for c, row in zip(captions, ids1.tolist()):
        want = oracle.encode(f"<|User|>: {c}\n\n<|Assistant|>: <grounding>{EOS_TAG}")[:-1]
        assert row[len(row) - len(want):] == want and set(row[:len(row) - len(want)]) <= {cfg.pad_id}
    s.x2t = lambda emb, mask, **kw: forced.to(e.device)                   # stage 1's decode, forced
    seen = []
    orig = e.prefill
    e.prefill = lambda ids, pad_len, **kw: (seen.append((ids.cpu().tolist(), [int(p) for p in pad_len])), orig(ids, pad_len, **kw))[1]
    try:
        out = s.uni_generate(dict(base_caption=captions, uni_stage1_inputs_ids=ids1, uni_stage1_attention_mask=mask1),
                             pred_layout=True, pred_image=pred_image, max_new_tokens=MAX_NEW)
    finally:
        del e.prefill
    grounding = []
    for t in layouts:                                                      # decode_plan_text_batch, plangen_base.py:296-306
        text = "<grounding>" + oracle.decode(oracle.encode(t)[1:] + [eos], skip_special_tokens=False)
        grounding.append(text[:text.find("</grounding>") + len("</grounding>")])
    assert out["pr_grounding"] == grounding and all(g.endswith("</box></grounding>") for g in grounding)
    if not pred_image:
        assert seen == []                                                  # plan: the layout text is the result
        return
    assert len(seen) == 1 and out["pr_image"].shape[0] == 2
    rows, pad = seen[0]
    neg = oracle.encode("<|User|>:<|Assistant|>:<begin_of_image>")         # neg_prompt '' with grounding '': two empty turns (conversation.py:80-91)
    assert neg == s.wrap_uni_prompt("", "")[1].tolist()
    for i, (c, g) in enumerate(zip(captions, grounding)):
        want = oracle.encode(f"<|User|>: {c}\n\n<|Assistant|>: {g}{EOS_TAG}<begin_of_image>")
        assert rows[2 * i][pad[2 * i]:] == want, (i, oracle.convert_ids_to_tokens(rows[2 * i][pad[2 * i]:]))
        assert set(rows[2 * i][:pad[2 * i]]) <= {cfg.pad_id} and len(rows[2 * i]) - pad[2 * i] == len(want)
        assert rows[2 * i + 1][pad[2 * i + 1]:] == neg
        for t in SPECIAL_ORDER:
            assert want.count(oracle.convert_tokens_to_ids(t)) == (c + g).count(t)
    assert max(max(r) for r in rows) < len(codec) <= cfg.vocab


# ----------------------------------------------------------------------------------------------------------------- 3
def test_added_ids_reach_their_own_embedding_rows(hf, tiny_cfg, tiny_weights):
    """pg_embed_tokens clamps an id past the table to the last row (load_ref.embed_gather_ref): a tokenizer longer than the table would
    pass silently.  The six added ids get THEIR rows, bit for bit, and none of those is the clamp's row."""
    from load_ref import embed_gather_ref
    codec, oracle, _ = hf
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids = torch.tensor(oracle.convert_tokens_to_ids(SPECIAL_ORDER))
    assert ids.tolist() == [codec.token_id(t) for t in SPECIAL_ORDER] == list(range(len(codec) - 6, len(codec))) and int(ids.max()) < tiny_cfg.vocab
    table = tiny_weights["language_model.model.embed_tokens.weight"]
    got = e.embed_tokens(ids.to(torch.int32)).cpu()
    assert torch.equal(got, table[ids]) and torch.equal(got, R.embed_tokens(tiny_weights, ids))
    assert torch.equal(got, embed_gather_ref(table, ids, None))          # the clamp is the identity on these ids
    assert not any(torch.equal(r, table[-1]) for r in got) and len(set(map(tuple, got.tolist()))) == 6
