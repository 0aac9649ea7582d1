"""CPU: the text plumbing either side of the hot path: chat template vs the fixture generated
by the reference's own conversation.py, the layout / answer post-processing rules vs the oracle restatement
(plangen_base.py:296-325, :460-473), the offline codec, and the CLI driver's error behaviour."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN
from oracle import ref_cpu as R
from plangen_amd import textproc as T


def test_chat_template_matches_reference_conversation_py():
    cases = json.load(open(os.path.join(GOLDEN, "text_golden.json")))
    assert len(cases) >= 5
    for c in cases:
        if "mmu_question" in c:
            continue
        assert T.wrap_uni_prompt_text(c["caption"], c["grounding"], c["in_stage1"]) == c["prompt"], c
    assert T.wrap_t2i_prompt_text("two dogs playing") == "<|User|>: two dogs playing\n\n<|Assistant|>:<begin_of_image>"


@pytest.mark.parametrize("text", [
    "<ref>a cat</ref><box>[12,40,500,620]</box></grounding> trailing <ref>x</ref>",
    "</grounding></grounding>", "no closing tag at all", "", "<ref>a</ref><box>[1,2,3,4]</box><ref>b c</ref><box>[10,20,30,40]</box></grounding>",
])
def test_plan_text_rules_match_oracle(text):
    assert T.cut_plan_text(text) == R.decode_plan_text(text)
    full = T.cut_plan_text(text)
    assert T.trans_gr_to_creati(full) == R.trans_gr_to_creati(full)
    assert T.get_pr_grounding_part("junk " + full).startswith("<grounding>")


def test_box_regex_values():
    boxes, names = T.trans_gr_to_creati("<grounding><ref>a red car</ref><box>[120,400,530,880]</box><ref>tree</ref><box>[0,0,1000,1000]</box></grounding>")
    assert names == ["a red car", "tree"] and boxes == [[0.12, 0.4, 0.53, 0.88], [0.0, 0.0, 1.0, 1.0]]
    assert T.trans_gr_to_creati("<grounding></grounding>") == ([], [])
    with pytest.raises(ValueError):
        T.trans_gr_to_creati("<ref>a</ref><box>[1,2,3]</box>")          # the reference's map(int, ...) unpack fails the same way


def test_cut_at_eos_matches_oracle():
    for ids in ([5, 9, 7, 4, 7], [7], [1, 2, 3], []):
        assert T.cut_at_eos(ids, 7) == R.cut_mmu_ids(ids, 7)


def test_tagword_codec_round_trip_and_stage1_drop():
    c = T.TagWordCodec(512)
    gr = "<grounding><ref>a small red cat</ref><box>[12,40,500,620]</box></grounding>"
    prompt, ids = T.wrap_uni_prompt_ids(c, "a cat on the table", gr)
    assert c.decode(ids) == prompt and ids[0] == c.bos_token_id and max(ids) < 512
    p1, ids1 = T.wrap_uni_prompt_ids(c, "a cat on the table", "<grounding>", in_stage1=True)
    assert p1.endswith("<grounding><｜end▁of▁sentence｜>") and c.decode(ids1).endswith("<grounding>")      # last token (EOS tag) dropped
    # ids of a layout survive decode -> cut -> parse
    layout_ids = c.encode("<ref>a dog</ref><box>[1,2,3,4]</box></grounding> and more")[1:]
    text = T.cut_plan_text(c.decode(layout_ids))
    assert T.trans_gr_to_creati(text) == ([[0.001, 0.002, 0.003, 0.004]], ["a dog"])
    with pytest.raises(ValueError):
        small = T.TagWordCodec(40)
        small.encode("many different words exceed this tiny vocabulary quickly indeed")


def _cli(**over):
    import train
    from conftest import ROOT
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1"] + [f"{k}={v!r}" for k, v in over.items()]
    return train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])


def test_cli_rejects_unknown_task_before_touching_the_gpu():
    from plangen_amd.engine import PlanGenError
    from project.plangen.plangen_base import System
    a = _cli()
    a.test_data = dict(a.test_data, task_type="segmentation")
    with pytest.raises(PlanGenError, match="task_type"):
        System(a, None)


def test_cli_resume_errors_are_loud(tmp_path):
    """a missing explicit resume path / a missing janus_path must not fall back to random weights."""
    from project.plangen.plangen_base import System
    s = object.__new__(System)
    s.engine = None
    s.synthetic = False
    s.cli = SimpleNamespace(out_path=str(tmp_path), resume=str(tmp_path / "checkpoint-9"), janus_path=str(tmp_path / "nope"))
    with pytest.raises(FileNotFoundError, match="resume"):
        s.resume()
    s.cli.resume = None
    with pytest.raises(FileNotFoundError, match="janus_path"):
        s.resume()


def test_mmu_chat_template_matches_reference_conversation_py():
    """wrap_mmu_prompt's text (plangen_base.py:263-279) as VLChatProcessor renders it -- the reference's conversation.py under the
    processor's own system prompt (fixture: oracle/make_golden.py::golden_text); ADVICE r2: mmu prompts were bare caption tokens."""
    cases = [c for c in json.load(open(os.path.join(GOLDEN, "text_golden.json"))) if "mmu_question" in c]
    assert len(cases) >= 3
    for c in cases:
        assert T.wrap_mmu_prompt_text(c["mmu_question"], c["mmu_answer"]) == c["prompt"], c
    assert cases[0]["prompt"].startswith("You are a helpful language and vision assistant.") and cases[0]["prompt"].endswith("<|Assistant|>:")
    assert "<|User|>: <image_placeholder>\nDescribe the layout of the image.\n\n<|Assistant|>:" in cases[0]["prompt"]


def test_image_placeholder_expansion_like_add_image_token():
    """processing_vlm.py:243-248 (add_special_token=False): the placeholder id is replaced by boi + P slots + eoi."""
    assert T.expand_image_tokens([1, 5, 9, 6], image_id=9, image_start_id=20, image_end_id=21, num_image_tokens=3) == [1, 5, 20, 9, 9, 9, 21, 6]
    assert T.expand_image_tokens([9, 9], 9, 20, 21, 1) == [20, 9, 21, 20, 9, 21]
    c = T.TagWordCodec(512)
    prompt, ids, slots = T.wrap_mmu_prompt_ids(c, "what is there?", 4)
    img, boi, eoi = c.token_id(T.IMAGE_TAG), c.token_id(T.IMAGE_START_TAG), c.token_id(T.IMAGE_END_TAG)
    k = ids.index(boi)
    assert ids[k:k + 6] == [boi, img, img, img, img, eoi] and sum(slots) == 4 and slots[k + 1:k + 5] == [True] * 4
    assert c.decode(ids[:k]).endswith("<|User|>: ") and c.decode(ids[k + 6:]).startswith("\nwhat is there?")


def test_cli_shards_whole_batches_so_file_names_cannot_collide(monkeypatch):
    """64 rows over 3 ranks with test_batch_size 8 -- every rank starts on a batch boundary, the global batch indices
    partition 0..7, and the names {gidx*bs+i} of all ranks are exactly 0..63."""
    from project.plangen import plangen_base as P
    names = []
    for rank in range(3):
        s = object.__new__(P.System)
        s.cli = SimpleNamespace(test_batch_size=8)
        s._rows = lambda: [{"k": i} for i in range(64)]
        s.collate = lambda rows: rows
        monkeypatch.setattr(P, "world", lambda r=rank: (r, 3))
        dl = s.setup_data()
        assert s.row_offset == s.batch_offset * 8
        for idx, b in enumerate(dl):
            names += [(s.batch_offset + idx) * 8 + i for i in range(len(b))]
            assert [r["k"] for r in b] == list(range((s.batch_offset + idx) * 8, (s.batch_offset + idx) * 8 + len(b)))
    assert sorted(names) == list(range(64)) and len(set(names)) == 64


def test_cli_integer_resume_maps_to_checkpoint_dir(tmp_path):
    """base_system.py:132-134: resume=<int> -> out_path/checkpoint-<int>."""
    from project.plangen.plangen_base import System
    s = object.__new__(System)
    s.engine = None
    s.synthetic = False
    s.cli = SimpleNamespace(out_path=str(tmp_path), resume=7, janus_path=str(tmp_path / "nope"))
    with pytest.raises(FileNotFoundError, match="checkpoint-7"):
        s.resume()
    os.makedirs(tmp_path / "checkpoint-7")
    with pytest.raises(FileNotFoundError, match="janus_path"):          # the overlay resolves; the base weights are what is missing now
        s.resume()


def _tiny_hf_tokenizer_dir(tmp_path):
    """A small byte-level BPE tokenizer saved in the HF layout (tokenizer.json + tokenizer_config.json + special_tokens_map.json) with the
    Janus special tokens -- what VLChatProcessor.from_pretrained(janus_path).tokenizer loads, minus the real vocabulary (no network here)."""
    from tokenizers import AddedToken, Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    from transformers import PreTrainedTokenizerFast
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    specials = ["<｜begin▁of▁sentence｜>", T.SEP2, T.PAD_TAG, T.IMAGE_TAG, T.IMAGE_START_TAG, T.IMAGE_END_TAG, "<|User|>", "<|Assistant|>",
                "<grounding>", "</grounding>", "<ref>", "</ref>", "<box>", "</box>"]
    corpus = ["a red cat on the table", "two dogs playing in a field", "what is on the table?", "0 1 2 3 4 5 6 7 8 9 , [ ] : \n\n",
              T.MMU_SYSTEM_PROMPT, "Describe the layout of the image."]
    tok.train_from_iterator(corpus * 4, trainers.BpeTrainer(vocab_size=400, special_tokens=specials, initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    bos = tok.token_to_id(specials[0])
    tok.post_processor = processors.TemplateProcessing(single=f"{specials[0]} $A", special_tokens=[(specials[0], bos)])
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, bos_token=specials[0], eos_token=T.SEP2, pad_token=T.PAD_TAG,
                                   additional_special_tokens=[AddedToken(s, special=True) for s in specials[3:]])
    d = tmp_path / "janus_tok"
    fast.save_pretrained(str(d))
    return str(d)


def test_hf_codec_on_tokenizer_files(tmp_path):
    """HFCodec (the path real Janus-Pro tokenizer files take): BOS prepended like tokenizer.encode, special tags are single ids,
    pad / eos ids come from the files, decode keeps specials (plangen_base.py:294), and the mmu prompt expands its placeholder."""
    d = _tiny_hf_tokenizer_dir(tmp_path)
    assert os.path.exists(os.path.join(d, "tokenizer.json"))
    c = T.HFCodec(d)
    assert c.eos_token_id == c.token_id(T.SEP2) and c.pad_id == c.token_id(T.PAD_TAG)
    prompt, ids = T.wrap_uni_prompt_ids(c, "a red cat on the table", "<grounding><ref>a cat</ref><box>[1,2,300,400]</box></grounding>")
    assert ids[0] == c.bos_token_id and ids[-1] == c.token_id(T.IMAGE_START_TAG)
    assert ids.count(c.token_id("<ref>")) == 1 and ids.count(c.token_id("<|User|>")) == 1 and ids.count(c.eos_token_id) == 1
    assert c.decode(ids[1:]) == prompt
    p1, ids1 = T.wrap_uni_prompt_ids(c, "two dogs", "<grounding>", in_stage1=True)
    assert p1.endswith("<grounding>" + T.SEP2) and ids1[-1] == c.token_id("<grounding>")            # trailing EOS-tag token dropped (:259-260)
    _, mids, slots = T.wrap_mmu_prompt_ids(c, "what is on the table?", 5)
    k = mids.index(c.token_id(T.IMAGE_START_TAG))
    assert mids[k + 1:k + 6] == [c.token_id(T.IMAGE_TAG)] * 5 and mids[k + 6] == c.token_id(T.IMAGE_END_TAG) and sum(slots) == 5
    assert c.decode(mids[1:k]).startswith(T.MMU_SYSTEM_PROMPT) and c.decode(mids[k + 7:]).endswith("<|Assistant|>:")
    with pytest.raises(KeyError):
        c.token_id("<no_such_tag>")
    # answers cut at the first EOS and parsed (decode_mmu_text_batch / trans_gr_to_creati on real tokenizer output)
    ans = c.encode("<ref>a cat</ref><box>[12,40,500,620]</box>")[1:] + [c.eos_token_id] + c.encode("junk")[1:]
    text = c.decode(T.cut_at_eos(ans, c.eos_token_id))
    assert T.trans_gr_to_creati(text) == ([[0.012, 0.04, 0.5, 0.62]], ["a cat"])


# ------------------------------------------------------------------------------------------ the reference's tokenizer extension
# System.__init__ (plangen_base.py:110-127) adds the six layout tags -- and with use_numhw_tokens 200 size tokens -- to the tokenizer before
# anything is encoded.  The directory of _tiny_hf_tokenizer_dir above already holds the tags (somebody extended it: the idempotence case);
# the one of tok_fixtures.plain_hf_tokenizer_dir does not, like the files of a checkpoint.  Every comparison below is integer equality with
# a tokenizer prepared by tok_fixtures.reference_prepared.
import re

from tok_fixtures import NUMHW_ORDER, SPECIAL_ORDER
from tok_fixtures import plain_hf_tokenizer_dir as _plain_hf_tokenizer_dir
from tok_fixtures import reference_prepared as _reference_prepared

GROUNDING = "<grounding><ref>a cat</ref><box>[12,40,500,620]</box><ref>a red dog</ref><box>[0, 7, 999, 1000]</box></grounding>"
ANSWER = "<ref>a cat</ref><box>[12,40,500,620]</box><ref>the table</ref><box>[1,2,300,400]</box>"
CAPTIONS = ["a red cat on the table",
            "look at <ref>the cat</ref> here",                          # a tag directly after a space
            "line one\n<box>[1,2,3,4]</box>\n</grounding>tail",         # ... after a newline
            "room 5<ref>x</ref>7</box>8",                               # ... after a digit
            "<ref></ref><box></box><grounding></grounding>",            # tags back to back
            "a <reflex> and </boxes> and <refs> stay text, <ref >too",  # a tag's prefix is not the tag
            "sizes <h3><w12><h99> and <h100>"]                          # numhw tokens, and one past the last


@pytest.fixture(scope="module")
def plain_dir(tmp_path_factory):
    return _plain_hf_tokenizer_dir(tmp_path_factory.mktemp("plain"))


def _prompts(codec):
    """(prompt, ids as the project builds them, how the reference gets them from ITS tokenizer's encode(prompt))"""
    out = []
    for cap in CAPTIONS:
        p, ids = T.wrap_uni_prompt_ids(codec, cap, GROUNDING)
        out.append((p, ids, lambda e: e))
        p, ids = T.wrap_uni_prompt_ids(codec, cap, "<grounding>", in_stage1=True)
        out.append((p, ids, lambda e: e[:-1]))                                     # plangen_base.py:259-260
    img = codec.token_id(T.IMAGE_TAG)
    slots = [codec.token_id(T.IMAGE_START_TAG)] + [img] * 5 + [codec.token_id(T.IMAGE_END_TAG)]
    for q, a in (("what is on the table?", ""), (CAPTIONS[1], ANSWER)):
        p, ids, mask = T.wrap_mmu_prompt_ids(codec, q, 5, a)
        assert sum(mask) == 5
        out.append((p, ids, lambda e, s=slots, i=img: [t for v in e for t in (s if v == i else [v])]))      # add_image_token, processing_vlm.py:243-248
    for text in (ANSWER, GROUNDING, ANSWER + "</grounding>"):
        out.append((text, codec.encode(text), lambda e: e))
    return out


@pytest.mark.parametrize("numhw", [False, True])
def test_hf_codec_adds_the_tags_at_the_reference_ids(plain_dir, numhw):
    n = len(_reference_prepared(plain_dir, False, False))
    o = _reference_prepared(plain_dir, True, numhw)
    c = T.HFCodec(plain_dir, special_tokens=True, numhw_tokens=numhw)
    assert [c.token_id(t) for t in SPECIAL_ORDER] == list(range(n, n + 6)) == o.convert_tokens_to_ids(SPECIAL_ORDER)
    assert len(c.tok) == len(c) == len(o) == n + 6 + 200 * numhw and c.n_added == 6 + 200 * numhw
    if numhw:
        assert [c.token_id(t) for t in NUMHW_ORDER] == list(range(n + 6, n + 206)) == o.convert_tokens_to_ids(NUMHW_ORDER)
        assert (c.token_id("<h0>"), c.token_id("<w0>"), c.token_id("<h1>"), c.token_id("<w99>")) == (n + 6, n + 7, n + 8, n + 205)
    else:
        with pytest.raises(KeyError):
            c.token_id("<h0>")
    assert (c.eos_token_id, c.bos_token_id, c.pad_id) == (o.eos_token_id, o.bos_token_id, o.convert_tokens_to_ids(T.PAD_TAG))
    assert c.eos_token_id == c.token_id(T.SEP2) < n and c.pad_id == c.token_id(T.PAD_TAG) < n
    only = T.HFCodec(plain_dir, numhw_tokens=True)                                   # the second switch alone: the same 200 names right after the files' ids
    assert [only.token_id(t) for t in NUMHW_ORDER] == list(range(n, n + 200)) and only.n_added == 200
    assert only.encode(GROUNDING) == _reference_prepared(plain_dir, False, True).encode(GROUNDING)


@pytest.mark.parametrize("numhw", [False, True])
def test_hf_codec_prompt_ids_equal_the_reference_tokenizers(plain_dir, numhw):
    o = _reference_prepared(plain_dir, True, numhw)
    c = T.HFCodec(plain_dir, special_tokens=True, numhw_tokens=numhw)
    tags = SPECIAL_ORDER + (NUMHW_ORDER if numhw else [])
    seen = 0
    for prompt, ids, ref in _prompts(c):
        assert list(ids) == ref(o.encode(prompt)), prompt
        for t in tags:
            assert list(ids).count(c.token_id(t)) == prompt.count(t), (prompt, t)              # one id per occurrence, none for <reflex> / </boxes>
            seen += prompt.count(t)
    assert seen > 100
    body = c.encode(CAPTIONS[5])[1:]
    assert not set(body) & set(c.token_id(t) for t in tags) and c.decode(body) == CAPTIONS[5]
    assert c.encode(CAPTIONS[6]).count(o.convert_tokens_to_ids("<h3>") if numhw else -1) == int(numhw)


def test_hf_codec_round_trip_through_the_added_tokens(plain_dir):
    c = T.HFCodec(plain_dir, special_tokens=True)
    for cap in CAPTIONS:
        p, ids = T.wrap_uni_prompt_ids(c, cap, GROUNDING)
        assert ids[0] == c.bos_token_id and c.decode(ids[1:]) == p, cap
        p, ids = T.wrap_uni_prompt_ids(c, cap, "<grounding>", in_stage1=True)
        assert p.endswith("<grounding>" + T.SEP2) and c.decode(ids[1:]) == p[:-len(T.SEP2)], cap           # stage 1: the EOS tag was dropped
    for text in (ANSWER, GROUNDING, T.wrap_mmu_prompt_text(CAPTIONS[1], ANSWER)):
        assert c.decode(c.encode(text)[1:]) == text
    ans = c.encode(ANSWER)[1:] + [c.eos_token_id] + c.encode("junk <ref>x</ref>")[1:]
    text = c.decode(T.cut_at_eos(ans, c.eos_token_id))
    assert text == ANSWER and T.trans_gr_to_creati(text) == ([[0.012, 0.04, 0.5, 0.62], [0.001, 0.002, 0.3, 0.4]], ["a cat", "the table"])
    lay = c.encode(ANSWER + "</grounding> and more")[1:]
    assert T.cut_plan_text(c.decode(lay)) == "<grounding>" + ANSWER + "</grounding>"


def test_hf_codec_extension_is_idempotent_on_extended_files(tmp_path):
    d = _tiny_hf_tokenizer_dir(tmp_path)
    before, c = T.HFCodec(d), T.HFCodec(d, special_tokens=True)
    n = len(before.tok)
    assert c.n_added == 0 and len(c.tok) == n == len(_reference_prepared(d, True, False))
    assert c.tok.convert_ids_to_tokens(list(range(n))) == before.tok.convert_ids_to_tokens(list(range(n)))
    assert [c.token_id(t) for t in SPECIAL_ORDER] == [before.token_id(t) for t in SPECIAL_ORDER] and max(c.token_id(t) for t in SPECIAL_ORDER) < n
    o = _reference_prepared(d, True, False)
    for prompt, ids, ref in _prompts(c):
        assert list(ids) == ref(before.encode(prompt)) == ref(o.encode(prompt)), prompt
    both = T.HFCodec(d, special_tokens=True, numhw_tokens=True)                      # the tags stay where they were, the size tokens follow the files' ids
    assert both.n_added == 200 and [both.token_id(t) for t in NUMHW_ORDER] == list(range(n, n + 200))
    assert [both.token_id(t) for t in SPECIAL_ORDER] == [before.token_id(t) for t in SPECIAL_ORDER]


def test_hf_codec_switches_off_is_the_tokenizer_of_the_files(plain_dir):
    """The reference with use_special_tokens=False (cfg/base.py:69): nothing is added, the tags are ordinary text."""
    o = _reference_prepared(plain_dir, False, False)
    for c in (T.HFCodec(plain_dir), T.HFCodec(plain_dir, special_tokens=False, numhw_tokens=False)):
        assert c.n_added == 0 and len(c.tok) == len(o)
        for t in SPECIAL_ORDER + ["<h0>"]:
            with pytest.raises(KeyError):
                c.token_id(t)
            assert len(c.encode(t)) > 2                                               # BOS + several pieces
        for cap in CAPTIONS:
            p, ids = T.wrap_uni_prompt_ids(c, cap, GROUNDING)
            assert ids == o.encode(p) and c.decode(ids[1:]) == p
        assert len(c.encode(GROUNDING)) > len(T.HFCodec(plain_dir, special_tokens=True).encode(GROUNDING)) + 10


def _symbols(text):
    from plangen_amd import grammar as G
    return re.findall("|".join(re.escape(t) for t in G.TAGS) + "|.", text, re.S)


def test_layout_grammar_over_the_extended_hf_codec(plain_dir):
    from plangen_amd import grammar as G
    from text_dfa_ref import accepts_layout
    vocab = 512
    o, plain = _reference_prepared(plain_dir, True, False), _reference_prepared(plain_dir, False, False)
    c = T.HFCodec(plain_dir, special_tokens=True)
    dfa = G.compile_token_dfa(G.layout_char_dfa(), c.token_strings(vocab), c.eos_token_id)
    assert dfa.token_class.shape == (vocab,) and (dfa.token_class[len(c):] == 0).all()
    for tag in G.TAGS:                                                    # every tag: a class of its own that holds this one token
        k = dfa.token_class[o.convert_tokens_to_ids(tag)]
        assert k != 0 and (dfa.token_class == k).sum() == 1, tag
    assert dfa.token_class[c.token_id("<grounding>")] == 0               # the prompt carries it; the layout never repeats it
    chars = G.layout_char_dfa()
    for text in (ANSWER + "</grounding>", "</grounding>", GROUNDING[len("<grounding>"):]):
        assert accepts_layout(text)
        st = dfa.start_state
        for t in o.encode(text)[1:] + [o.eos_token_id]:
            st = dfa.step(st, t)
            assert st >= 0, (text, t)
        assert dfa.dist[st] == 0                                          # the accepting state
        # the files' own tokenizer spells the tags in pieces: the same string, judged by the character-level rules
        split = plain.encode(text)[1:]
        assert len(split) > len(o.encode(text)[1:]) and plain.decode(split) == text
        assert chars.accepts(_symbols(plain.decode(split)) + [G.EOS])
        assert not chars.accepts(_symbols(plain.decode(split)[:-1]) + [G.EOS])
    assert G.layout_token_dfa(c, vocab) is G.layout_token_dfa(c, vocab)


def test_layout_grammar_refuses_a_vocabulary_without_the_tags(plain_dir):
    """A tag that is not a single token: an error that names it, not an automaton that can only write the empty layout."""
    from plangen_amd import grammar as G
    plain = T.HFCodec(plain_dir)
    with pytest.raises(ValueError, match=re.escape("<ref>")) as ei:
        G.layout_token_dfa(plain, 512)
    assert all(t in str(ei.value) for t in G.TAGS)
    c = T.HFCodec(plain_dir, special_tokens=True)
    strings = c.token_strings(512)
    for tag in G.TAGS:
        with pytest.raises(ValueError, match=re.escape(tag)) as ei:
            G.compile_token_dfa(G.layout_char_dfa(), [None if s == tag else s for s in strings], c.eos_token_id)
        assert [t for t in G.TAGS if t in str(ei.value)] == [tag]
    with pytest.raises(ValueError, match=re.escape("</box>")):             # the tag's characters in one token's string do not make it the tag
        G.compile_token_dfa(G.layout_char_dfa(), [s + " " if s == "</box>" else s for s in strings], c.eos_token_id)


def test_tokenizer_longer_than_the_embedding_table_is_refused(plain_dir, tiny_cfg):
    from plangen_amd.engine import PlanGenError
    from plangen_amd.system import System, check_codec_capacity
    from project.plangen.plangen_base import System as CliSystem
    fits, over = T.HFCodec(plain_dir, special_tokens=True), T.HFCodec(plain_dir, special_tokens=True, numhw_tokens=True)
    assert len(fits) <= tiny_cfg.vocab < len(over)
    check_codec_capacity(fits, tiny_cfg.vocab)
    check_codec_capacity(fits, len(fits))                                   # the largest id is len - 1: a table of exactly len rows holds it
    with pytest.raises(PlanGenError, match=f"{len(fits)}.*vocab={len(fits) - 1}"):
        check_codec_capacity(fits, len(fits) - 1)
    with pytest.raises(PlanGenError, match=f"{len(over)}.*vocab={tiny_cfg.vocab}"):
        System(tiny_cfg, None, codec=over)                                  # refused before the engine is touched
    a = _cli(janus_path=plain_dir, use_numhw_tokens=True)
    assert a.use_special_tokens is True                                     # the README configuration's key (h_text_ump+oimsam.py:11)
    with pytest.raises(PlanGenError, match=f"{len(over)}.*vocab={tiny_cfg.vocab}"):
        CliSystem(a, None)                                                  # ... and before one is created
