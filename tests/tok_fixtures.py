"""Tokenizer fixtures for the tokenizer-extension tests: a directory shaped like the tokenizer files of a checkpoint (the layout tags are
NOT in it), and the same files prepared the way the reference's ``System.__init__`` prepares its tokenizer (plangen_base.py:110-127) --
the oracle of every id comparison.  Built with the ``tokenizers`` / ``transformers`` packages; nothing is downloaded."""
from plangen_amd import textproc as T

BOS_TAG = "<｜begin▁of▁sentence｜>"
PLAIN_SPECIALS = [BOS_TAG, T.SEP2, T.PAD_TAG, T.IMAGE_TAG, T.IMAGE_START_TAG, T.IMAGE_END_TAG, "<|User|>", "<|Assistant|>"]
# plangen_base.py:111-118 and :122-126, written out: the order is what fixes the ids
SPECIAL_ORDER = ["<grounding>", "</grounding>", "<box>", "</box>", "<ref>", "</ref>"]
NUMHW_ORDER = [f"<{a}{i}>" for i in range(100) for a in ("h", "w")]
MAX_FIXTURE_VOCAB = 400                 # + 6 tags < the tiny model's 512 rows; + 200 more (numhw) > 512: the capacity case
CORPUS = ["a red cat on the table", "two dogs playing in a field", "what is on the table?", "0 1 2 3 4 5 6 7 8 9 , [ ] : \n\n",
          T.MMU_SYSTEM_PROMPT, "Describe the layout of the image.",
          # layout text as data_hico.py:get_grounding writes it: BPE learns merges over the characters of the tags ('ref', 'box', '</', '><' ...),
          # so that without add_tokens a tag still encodes -- silently, into several ordinary pieces
          "<grounding><ref>a cat</ref><box>[12,40,500,620]</box><ref>a red dog</ref><box>[0, 7, 999, 1000]</box></grounding>",
          "<ref>a cat</ref><box>[12,40,500,620]</box>", "<ref>the table</ref><box>[100,200,300,400]</box></grounding>"]


def plain_hf_tokenizer_dir(tmp_path):
    """A byte-level BPE tokenizer saved in the HF layout (tokenizer.json + tokenizer_config.json + special_tokens_map.json) whose special
    tokens are BOS, the EOS tag, the pad tag, the three image tags and the two role tags -- and none of the six layout tags."""
    from tokenizers import AddedToken, Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    from transformers import PreTrainedTokenizerFast
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    tok.train_from_iterator(CORPUS * 4, trainers.BpeTrainer(vocab_size=MAX_FIXTURE_VOCAB, special_tokens=PLAIN_SPECIALS,
                                                            initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    bos = tok.token_to_id(BOS_TAG)
    tok.post_processor = processors.TemplateProcessing(single=f"{BOS_TAG} $A", special_tokens=[(BOS_TAG, bos)])
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, bos_token=BOS_TAG, eos_token=T.SEP2, pad_token=T.PAD_TAG,
                                   additional_special_tokens=[AddedToken(s, special=True) for s in PLAIN_SPECIALS[3:]])
    d = tmp_path / "janus_tok_plain"
    fast.save_pretrained(str(d))
    # the properties the tests lean on, asserted on the files themselves
    from transformers import AutoTokenizer
    back = AutoTokenizer.from_pretrained(str(d))
    assert 256 + len(PLAIN_SPECIALS) < len(back) <= MAX_FIXTURE_VOCAB, len(back)
    vocab = back.get_vocab()
    assert not any(t in vocab for t in SPECIAL_ORDER + NUMHW_ORDER)
    for tag in SPECIAL_ORDER:
        pieces = back.encode(tag)[1:]
        assert len(pieces) > 1 and back.decode(pieces) == tag, (tag, pieces)        # split, and silently: it still round-trips
    assert len(back.encode("<ref>")[1:]) < len("<ref>")                              # through learned merges, not byte by byte
    return str(d)


def reference_prepared(path, special, numhw):
    """The tokenizer as the reference holds it when it encodes (plangen_base.py:93, :110-127)."""
    from tokenizers import AddedToken
    from transformers import AutoTokenizer
    tokenizer = AutoTokenizer.from_pretrained(path)
    if special:
        tokenizer.add_tokens([AddedToken(t, special=True) for t in SPECIAL_ORDER])
    if numhw:
        tokenizer.add_tokens([AddedToken(t, special=True) for t in NUMHW_ORDER])
    return tokenizer
