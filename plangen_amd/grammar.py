"""Grammar-constrained layout decoding, host side: a character-level automaton for the layout string stage 1 of
``uni_2stage`` / the ``plan`` task writes, compiled over a tokenizer's vocabulary into the token automaton the text
sampler masks its logits with (``pg_set_text_dfa`` / ``pg_generate_text_constrained``, include/plangen_hip.h).

The language is what ``data_hico.py:get_grounding`` emits with ``use_textual`` (minus the ``<grounding>`` the prompt already
carries), as ``cut_plan_text`` / ``trans_gr_to_creati`` read it back::

    layout := item* "</grounding>" EOS
    item   := "<ref>" text "</ref>" "<box>" "[" int ("," " "? int){3} "]" "</box>"
    text   := 1..64 characters, none of "<" ">" or newline
    int    := 1..4 digits

Tags and EOS are atomic symbols: a token spells a tag only if its string IS the tag, and a vocabulary in which some tag is no single
token (tokenizer files the reference's ``add_tokens`` was never applied to: ``HFCodec(special_tokens=True)``) is refused by name.
Pure numpy; no GPU.

Known limit: the automaton reads each token's OWN string (``codec.token_strings``).  A byte-level piece that is not valid UTF-8 alone
has no string of its own (HFCodec maps it to None: allowed nowhere), so descriptions that need such pieces (characters split over
several byte tokens) cannot be generated under the constraint; and a tokenizer whose decode of joined ids differs from the joined
decodes of the ids (space merging) is outside what the per-token check can promise.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

MAX_STATES, MAX_CLASSES = 4096, 1024            # the limits of pg_set_text_dfa
DIST_INF = 1 << 30                              # dist >= DIST_INF: the row cannot finish from this state
TEXT_MAX, INT_DIGITS = 64, 4
EOS = "\x00<eos>"                               # the EOS symbol (never a token's string)
TAGS = ("<ref>", "</ref>", "<box>", "</box>", "</grounding>")


class CharDFA:
    """A deterministic automaton over symbols = single characters + atomic tags + EOS.  ``table[sym, state]`` is the next state;
    state ``n_states`` is the dead state (every symbol keeps it there).  ``accept``: the states a finished row is in."""

    def __init__(self, n_states: int, start: int, accept: Sequence[int], atoms: Sequence[str]):
        self.n_states, self.start, self.accept = n_states, start, tuple(accept)
        self.atoms = {a: i for i, a in enumerate(atoms)}                  # tag / EOS -> symbol
        self._chars: Dict[str, int] = {}                                  # character -> symbol
        self._rows: List[np.ndarray] = [np.full(n_states + 1, n_states, np.int32) for _ in atoms]
        self._other: Optional[int] = None

    def _sym(self, s: str) -> int:
        if s in self.atoms:
            return self.atoms[s]
        if s not in self._chars:
            self._chars[s] = len(self._rows)
            self._rows.append(np.full(self.n_states + 1, self.n_states, np.int32))
        return self._chars[s]

    def add(self, src: int, sym: str, dst: int) -> None:
        self._rows[self._sym(sym)][src] = dst

    def add_other(self, src: int, dst: int) -> None:
        """Every character without a row of its own (see ``forbid``) moves src -> dst."""
        if self._other is None:
            self._other = len(self._rows)
            self._rows.append(np.full(self.n_states + 1, self.n_states, np.int32))
        self._rows[self._other][src] = dst

    def forbid(self, ch: str) -> None:
        self._sym(ch)                                                      # an all-dead row of its own

    @property
    def table(self) -> np.ndarray:
        return np.stack(self._rows)

    def symbols(self, s: Optional[str]) -> Optional[List[int]]:
        """The symbols a token's string spells, or None when it spells nothing the automaton can read."""
        if not s:
            return None
        if s in self.atoms:
            return [self.atoms[s]]
        out = []
        for ch in s:
            i = self._chars.get(ch, self._other)
            if i is None:
                return None
            out.append(i)
        return out

    def accepts(self, symbols: Sequence[str]) -> bool:
        """Run a sequence of symbols (characters, tags, EOS) from the start state."""
        st, t = self.start, self.table
        for s in symbols:
            sy = self.symbols(s)
            if sy is None:
                return False
            for i in sy:
                st = int(t[i, st])
        return st in self.accept


def layout_char_dfa() -> CharDFA:
    ids: Dict[object, int] = {}

    def S(*k):
        return ids.setdefault(k, len(ids))
    names = [("item",)] + [("text", n) for n in range(TEXT_MAX + 1)] + [("ref_done",), ("box_open",)]
    names += [("int", k, d) for k in range(4) for d in range(INT_DIGITS + 1)]
    names += [("comma", k) for k in range(3)] + [("space", k) for k in range(3)] + [("box_close",), ("end",), ("accept",)]
    for n in names:
        S(*n)
    d = CharDFA(len(ids), S("item"), [S("accept")], list(TAGS) + [EOS])
    for ch in "<>\n":
        d.forbid(ch)
    digits = "0123456789"
    special = digits + ", []"
    d.add(S("item"), "<ref>", S("text", 0))
    d.add(S("item"), "</grounding>", S("end"))
    d.add(S("end"), EOS, S("accept"))
    for n in range(TEXT_MAX):
        for ch in special:
            d.add(S("text", n), ch, S("text", n + 1))
        d.add_other(S("text", n), S("text", n + 1))
    for n in range(1, TEXT_MAX + 1):
        d.add(S("text", n), "</ref>", S("ref_done"))
    d.add(S("ref_done"), "<box>", S("box_open"))
    d.add(S("box_open"), "[", S("int", 0, 0))
    for k in range(4):
        for n in range(INT_DIGITS):
            for ch in digits:
                d.add(S("int", k, n), ch, S("int", k, n + 1))
        for n in range(1, INT_DIGITS + 1):
            if k < 3:
                d.add(S("int", k, n), ",", S("comma", k))
            else:
                d.add(S("int", k, n), "]", S("box_close"))
    for k in range(3):
        d.add(S("comma", k), " ", S("space", k))
        for ch in digits:
            d.add(S("comma", k), ch, S("int", k + 1, 1))
            d.add(S("space", k), ch, S("int", k + 1, 1))
    d.add(S("box_close"), "</box>", S("item"))
    return d


@dataclass
class TokenDFA:
    """The tables of ``pg_text_dfa``: ``token_class`` int16 [vocab], ``next_state`` int16 [n_states, n_classes] (-1: not allowed),
    ``dist`` int32 [n_states] = fewest further tokens (EOS included) until the row can finish."""
    token_class: np.ndarray
    next_state: np.ndarray
    dist: np.ndarray
    start_state: int

    @property
    def n_states(self) -> int:
        return int(self.next_state.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.next_state.shape[1])

    def allowed_classes(self, state: int, remaining: int) -> np.ndarray:
        """bool [n_classes]: the transition exists and the row can still finish within the budget after it."""
        nx = self.next_state[state].astype(np.int64)
        return (nx >= 0) & (self.dist[np.maximum(nx, 0)] <= remaining - 1)

    def allowed(self, state: int, remaining: int) -> np.ndarray:
        return self.allowed_classes(state, remaining)[self.token_class]

    def step(self, state: int, token: int) -> int:
        return int(self.next_state[state, self.token_class[token]])


def token_dist(next_state: np.ndarray, accept: Sequence[int], used: np.ndarray) -> np.ndarray:
    """Breadth-first search backwards from the accepting states over the classes that hold at least one token."""
    n = next_state.shape[0]
    dist = np.full(n, DIST_INF, np.int64)
    dist[list(accept)] = 0
    nx = next_state[:, used] if used.any() else np.zeros((n, 0), np.int64)
    for d in range(1, n + 1):
        reach = ((nx >= 0) & (dist[np.maximum(nx, 0)] == d - 1)).any(axis=1) & (dist == DIST_INF)
        if not reach.any():
            break
        dist[reach] = d
    return dist


def compile_token_dfa(char_dfa: CharDFA, token_strings: Sequence[Optional[str]], eos_id: int) -> TokenDFA:
    """Run every token's string through ``char_dfa`` from every state; tokens with the same transition column share a class."""
    n, table = char_dfa.n_states, char_dfa.table
    # a tag is a symbol only as a whole token: over a vocabulary that spells one in pieces (a tokenizer the tags were never added to) every
    # state behind it is unreachable, and what would come out is an automaton that can never write or close an item
    have = set(s for i, s in enumerate(token_strings) if i != eos_id)
    missing = [a for a in char_dfa.atoms if a != EOS and a not in have]
    if missing:
        raise ValueError(f"compile_token_dfa: no single token of this vocabulary spells {', '.join(missing)}: add the tags to the tokenizer "
                         "(HFCodec(special_tokens=True), cfg key use_special_tokens)")
    ident = np.arange(n + 1, dtype=np.int32)
    dead_col = np.full(n + 1, n, np.int32)
    by_string: Dict[Optional[str], bytes] = {}
    cols: Dict[bytes, int] = {dead_col.tobytes(): 0}                      # class 0: allowed nowhere
    cls = np.zeros(len(token_strings), np.int64)
    for i, s in enumerate(token_strings):
        key = EOS if i == eos_id else s
        if key not in by_string:
            syms = [char_dfa.atoms[EOS]] if i == eos_id else char_dfa.symbols(s)
            col = dead_col
            if syms is not None:
                col = ident
                for sy in syms:
                    col = table[sy][col]
                    if (col == n).all():
                        break
            by_string[key] = col.tobytes()
        cls[i] = cols.setdefault(by_string[key], len(cols))
    nxt = np.stack([np.frombuffer(c, np.int32) for c in cols]).T[:n].astype(np.int64)      # [state, class], dead = n
    nxt[nxt == n] = -1
    used = np.bincount(cls, minlength=nxt.shape[1]) > 0
    used[0] = False
    dist = token_dist(nxt, char_dfa.accept, used)
    if dist[char_dfa.start] >= DIST_INF:
        raise ValueError("compile_token_dfa: no token sequence of this vocabulary finishes from the start state")
    # prune the states that cannot finish, then merge the classes whose columns became equal
    live = dist < DIST_INF
    remap = np.full(n + 1, -1, np.int64)
    remap[:n][live] = np.arange(int(live.sum()))
    nxt = remap[nxt[live]]                                                # remap[-1] is the dead slot
    uniq, first, inv = np.unique(nxt.T, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first)                                             # keep class 0 first and the numbering stable
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    nxt, cls = uniq[order].T, rank[inv][cls]
    if nxt.shape[0] > MAX_STATES or nxt.shape[1] > MAX_CLASSES:
        raise ValueError(f"compile_token_dfa: {nxt.shape[0]} states x {nxt.shape[1]} classes exceed the limits {MAX_STATES} x {MAX_CLASSES}")
    return TokenDFA(np.ascontiguousarray(cls, dtype=np.int16), np.ascontiguousarray(nxt, dtype=np.int16),
                    np.ascontiguousarray(dist[live], dtype=np.int32), int(remap[char_dfa.start]))


def layout_token_dfa(codec, vocab: int) -> TokenDFA:
    """The layout automaton over ``codec``'s vocabulary, cached on the codec (rebuilt when a growing vocabulary has grown)."""
    version = getattr(codec, "token_table_version", lambda: 0)()
    cache = codec.__dict__.setdefault("_layout_dfa_cache", {})
    key = (int(vocab), version)
    if key not in cache:
        cache.clear()
        cache[key] = compile_token_dfa(layout_char_dfa(), codec.token_strings(vocab), codec.eos_token_id)
    return cache[key]
