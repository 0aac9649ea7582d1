"""CPU: plangen_amd/grammar.py -- the layout language's character automaton compiled over a vocabulary into the token automaton of
pg_set_text_dfa.  Checked against a regular-expression acceptor (text_dfa_ref.py) and the project's own readers of the layout string
(cut_plan_text, trans_gr_to_creati); ``dist`` against a brute-force shortest path."""
import numpy as np
import pytest

from text_dfa_ref import DIST_INF, accepts_layout, brute_dist, n_items
from plangen_amd import grammar as G
from plangen_amd.textproc import GROUNDING_OPEN, TagWordCodec, cut_plan_text, trans_gr_to_creati

TINY_VOCAB = 512


def get_grounding(items, sep=", "):
    """data_hico.py:get_grounding with use_textual, after the ``<grounding>`` the stage-1 prompt ends with."""
    return "".join(f"<ref>{d}</ref><box>[{sep.join(str(x) for x in box)}]</box>" for d, box in items) + "</grounding>"


class PieceCodec:
    """A hand-made 64-entry vocabulary with multi-character pieces, encoded by longest match."""
    PIECES = ["<eos>", "<ref>", "</ref>", "<box>", "</box>", "</grounding>", "<grounding>", ", ", ",", " ", " [", "[", "]", "12", "100", "999",
              "0", "1", "2", "3", "4", "5", "6", "7", "8", "9", "a", "b", "c", "d", "e", "g", "o", "t", "cat", "dog", " a", "a ", "at", "\n", "<", ">",
              "], ", "9]", "[1", "</box> <ref>", ".", ":", "-", "red", " red", "x<", "box"]
    eos_token_id = 0

    def __init__(self):
        assert len(self.PIECES) <= 64 and len(set(self.PIECES)) == len(self.PIECES)
        self.by_len = sorted(range(len(self.PIECES)), key=lambda i: -len(self.PIECES[i]))

    def token_strings(self, vocab):
        return [self.PIECES[i] if i < len(self.PIECES) else None for i in range(vocab)]

    def encode(self, text):
        out, pos = [], 0
        while pos < len(text):
            i = next(i for i in self.by_len if i != 0 and text.startswith(self.PIECES[i], pos))
            out.append(i)
            pos += len(self.PIECES[i])
        return out

    def decode(self, ids):
        return "".join(self.PIECES[i] for i in ids if i != 0)


def _run(dfa, ids):
    """-> (final state, index of the first token the automaton refuses or None)"""
    st = dfa.start_state
    for k, t in enumerate(ids):
        nx = dfa.step(st, t)
        if nx < 0:
            return st, k
        st = nx
    return st, None


def _tagword():
    c = TagWordCodec(TINY_VOCAB)
    for w in ("cat", "dog", "a", "red", "bike", "on", "the", "left"):
        c.token_id(w)
    return c, lambda text: c.encode(text)[1:]                         # encode() prepends BOS


def _piece():
    c = PieceCodec()
    return c, c.encode


LAYOUTS = [
    [],
    [("cat", (1, 2, 3, 4))],
    [("a red cat", (12, 100, 999, 1000)), ("dog", (0, 0, 9, 9))],
    [("cat " * 16, (1234, 5, 67, 890))],                              # 64 characters of text
    [(f"dog {i}", (i, 10 * i, 100 * i, 999)) for i in range(10)],     # 10 items
]


# ----------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("make", [_tagword, _piece])
def test_accepts_valid_layouts(make):
    codec, enc = make()
    vocab = TINY_VOCAB if make is _tagword else 64
    dfa = G.layout_token_dfa(codec, vocab) if make is _tagword else G.compile_token_dfa(G.layout_char_dfa(), codec.token_strings(vocab), 0)
    assert dfa.token_class.shape == (vocab,) and dfa.token_class.dtype == np.int16 and dfa.next_state.dtype == np.int16
    assert dfa.next_state.shape == (dfa.n_states, dfa.n_classes) and dfa.dist.shape == (dfa.n_states,) and dfa.dist.dtype == np.int32
    assert dfa.n_states <= G.MAX_STATES and dfa.n_classes <= G.MAX_CLASSES and (dfa.dist < DIST_INF).all()      # pruned
    for items in LAYOUTS:
        for sep in (", ", ","):
            text = get_grounding(items, sep)
            assert accepts_layout(text)
            ids = enc(text) + [codec.eos_token_id]
            st, bad = _run(dfa, ids)
            assert bad is None and dfa.dist[st] == 0, (text, bad)
            assert _run(dfa, ids[:-1])[1] is None and dfa.dist[_run(dfa, ids[:-1])[0]] == 1          # before the EOS: one token to go
    if make is _piece:                                                # the multi-character pieces are really in use
        ids = enc(get_grounding([("cat a", (12, 100, 999, 12))]))
        for p in (", ", "12", "100", "999", "cat", " a"):
            assert PieceCodec.PIECES.index(p) in ids, p
        tc = dfa.token_class
        P = PieceCodec.PIECES.index
        assert tc[P(" [")] != tc[P("[")] and tc[P("], ")] != 0 and tc[P("9]")] != 0 and tc[P("[1")] != 0
        assert tc[P("</box> <ref>")] == 0 and tc[P("<")] == 0 and tc[P("\n")] == 0 and tc[P("<grounding>")] == 0     # a tag is a symbol only as a whole token
        assert (tc[len(PieceCodec.PIECES):] == 0).all()              # unknown ids: allowed nowhere
        assert (dfa.next_state[:, 0] == -1).all()


def test_layout_token_dfa_is_cached_and_follows_a_growing_vocabulary():
    codec, enc = _tagword()
    a = G.layout_token_dfa(codec, TINY_VOCAB)
    assert G.layout_token_dfa(codec, TINY_VOCAB) is a
    new = codec.token_id("zebra")
    assert a.token_class[new] == 0
    b = G.layout_token_dfa(codec, TINY_VOCAB)
    assert b is not a and b.token_class[new] != 0
    assert codec.token_strings(TINY_VOCAB)[new] == "zebra" and codec.token_strings(TINY_VOCAB)[TINY_VOCAB - 1] is None
    assert b.token_class[codec.bos_token_id] == 0                     # an empty string spells nothing


# ----------------------------------------------------------------------------------------------------------------- (b)
def test_rejects_corrupted_layouts_at_the_first_offending_token():
    codec, enc = _tagword()
    dfa = G.layout_token_dfa(codec, TINY_VOCAB)
    eos = codec.eos_token_id
    tid = codec.token_id
    good = "<ref>cat</ref><box>[1,2,3,4]</box>"

    def first_bad(ids):
        return _run(dfa, ids)[1]
    ids = enc("<ref>cat<box>[1,2,3,4]</box></grounding>")             # missing </ref>
    assert first_bad(ids) == ids.index(tid("<box>"))
    ids = enc("<ref>cat</ref><box>[1,2,3,4,5]</box></grounding>")     # five coordinates
    commas = [k for k, t in enumerate(ids) if t == tid(",")]
    assert first_bad(ids) == commas[3]
    ids = enc("<ref>cat</ref><box>[12345,2,3,4]</box></grounding>")   # a five-digit number
    assert first_bad(ids) == ids.index(tid("5"))
    ids = enc("<box>[1,2,3,4]</box><ref>cat</ref></grounding>")       # <box> before <ref>
    assert first_bad(ids) == 0
    ids = enc(good) + [eos]                                           # EOS before </grounding>
    assert first_bad(ids) == len(ids) - 1
    assert first_bad([eos]) == 0
    for text in ("<ref></ref><box>[1,2,3,4]</box></grounding>", "<ref>" + "a " * 33 + "</ref><box>[1,2,3,4]</box></grounding>",
                 "<ref>cat</ref><box>[1,,2,3,4]</box></grounding>", "<ref>cat</ref><box>[1,  2,3,4]</box></grounding>",
                 "<ref>cat</ref><box>[1,2,3]</box></grounding>", "<ref>cat</ref><box>[1,2,3,4]</box>\n</grounding>"):
        assert not accepts_layout(text) and first_bad(enc(text)) is not None, text
    assert first_bad(enc(good + "</grounding>") + [eos, eos]) is not None          # nothing after the EOS


# ----------------------------------------------------------------------------------------------------------------- (c)
def test_random_walks_end_in_time_and_parse():
    codec, _ = _tagword()
    dfa = G.layout_token_dfa(codec, TINY_VOCAB)
    eos = codec.eos_token_id
    rng = np.random.default_rng(2024)
    d0 = int(dfa.dist[dfa.start_state])
    assert d0 == 2                                                    # </grounding> EOS
    cache = {}
    lengths, items = [], 0
    for w in range(2000):
        max_new = (d0, 24, 40)[w % 3]
        st, ids = dfa.start_state, []
        for step in range(max_new):
            rem = max_new - step
            if (st, rem) not in cache:
                cache[st, rem] = np.nonzero(dfa.allowed(st, rem))[0]
            ok = cache[st, rem]
            assert len(ok) > 0, (w, step, st)
            tok = int(rng.choice(ok))
            ids.append(tok)
            st = dfa.step(st, tok)
            assert st >= 0 and dfa.dist[st] <= rem - 1
            if tok == eos:
                break
        assert ids[-1] == eos and len(ids) <= max_new and eos not in ids[:-1], (w, ids)
        text = codec.decode(ids[:-1])
        assert accepts_layout(text), text
        assert cut_plan_text(codec.decode(ids)) == GROUNDING_OPEN + text            # kept whole, EOS text cut off
        boxes, descs = trans_gr_to_creati(GROUNDING_OPEN + text)
        assert len(boxes) == len(descs) == n_items(text)
        lengths.append(len(ids))
        items += len(boxes)
    assert max(lengths) == 40 and items > 50                          # the walks do reach the budget and do hold items


# ----------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("make", [_tagword, _piece])
def test_dist_is_the_shortest_path(make):
    codec, _ = make()
    vocab = TINY_VOCAB if make is _tagword else 64
    dfa = G.compile_token_dfa(G.layout_char_dfa(), codec.token_strings(vocab), codec.eos_token_id)
    col = dfa.next_state[:, dfa.token_class[codec.eos_token_id]]
    accept = sorted(set(int(s) for s in col if s >= 0))
    assert len(accept) == 1
    assert np.array_equal(dfa.dist, brute_dist(dfa.token_class, dfa.next_state, accept))
    assert dfa.dist[dfa.start_state] == 2 and (dfa.dist == 0).sum() == 1


# ----------------------------------------------------------------------------------------------------------------- (e)
def test_builder_raises():
    codec = PieceCodec()
    strings = codec.token_strings(64)
    with pytest.raises(ValueError):                                   # no </grounding> token: the start state cannot finish
        G.compile_token_dfa(G.layout_char_dfa(), [None if s == "</grounding>" else s for s in strings], 0)
    with pytest.raises(ValueError):                                   # the EOS id is not in the vocabulary
        G.compile_token_dfa(G.layout_char_dfa(), strings[1:], 999)
    n = G.MAX_STATES + 1                                              # a^n EOS: n + 2 live states
    chain = G.CharDFA(n + 2, 0, [n + 1], [G.EOS])
    for s in range(n):
        chain.add(s, "a", s + 1)
    chain.add(n, G.EOS, n + 1)
    with pytest.raises(ValueError):
        G.compile_token_dfa(chain, ["a", "<eos>"], 1)
    n = G.MAX_CLASSES + 1                                             # a different character at every step: n + 2 classes
    wide = G.CharDFA(n + 2, 0, [n + 1], [G.EOS])
    chars = [chr(0x4E00 + i) for i in range(n)]
    for s, ch in enumerate(chars):
        wide.add(s, ch, s + 1)
    wide.add(n, G.EOS, n + 1)
    with pytest.raises(ValueError):
        G.compile_token_dfa(wide, chars + ["<eos>"], n)
    ok = G.CharDFA(5, 0, [4], [G.EOS])                                # the same shapes inside the limits compile
    for s in range(3):
        ok.add(s, "a", s + 1)
    ok.add(3, G.EOS, 4)
    d = G.compile_token_dfa(ok, ["a", "<eos>", None], 1)
    assert d.n_states == 5 and d.n_classes == 3 and d.dist.tolist() == [4, 3, 2, 1, 0] and d.token_class.tolist() == [1, 2, 0]
