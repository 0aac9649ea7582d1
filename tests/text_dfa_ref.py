"""numpy restatement of the grammar-constrained text step (include/plangen_hip.h, pg_generate_text_constrained): the allowed set with the
budget rule, the masked greedy token, the next state, a loop simulator, a brute-force ``dist`` and random automata for the operator tests;
and an acceptor for the layout language written as a regular expression, so that it shares no code with plangen_amd/grammar.py."""
import re

import numpy as np

DIST_INF = 1 << 30
LAYOUT_RE = re.compile(r"^(<ref>[^<>\n]{1,64}</ref><box>\[\d{1,4}(, ?\d{1,4}){3}\]</box>)*</grounding>$")
ITEM_RE = re.compile(r"<ref>[^<>\n]{1,64}</ref><box>\[\d{1,4}(?:, ?\d{1,4}){3}\]</box>")


def accepts_layout(text: str) -> bool:
    """``text``: the decoded new tokens up to (excluding) the EOS."""
    return LAYOUT_RE.match(text) is not None


def n_items(text: str) -> int:
    return len(ITEM_RE.findall(text))


def allowed_mask(token_class, next_state, dist, state: int, remaining: int, V=None) -> np.ndarray:
    """bool [V]: v is allowed in ``state`` iff nx = next_state[state][token_class[v]] >= 0 and dist[nx] <= remaining - 1."""
    token_class = np.asarray(token_class)[:V].astype(np.int64)
    if not 0 <= state < next_state.shape[0]:
        return np.zeros(token_class.shape[0], bool)
    nx = np.asarray(next_state)[state].astype(np.int64)[token_class]
    return (nx >= 0) & (np.asarray(dist).astype(np.int64)[np.maximum(nx, 0)] <= remaining - 1)


def masked_row(logits, allowed) -> np.ndarray:
    return np.where(allowed, np.asarray(logits, dtype=np.float32), np.float32(-np.inf))


def greedy_step(logits, token_class, next_state, dist, state: int, remaining: int, eos: int):
    """-> (allowed mask, token, next state): the masked argmax, lowest index on ties; nothing above -inf: eos, state kept."""
    V = len(logits)
    ok = allowed_mask(token_class, next_state, dist, state, remaining, V)
    row = masked_row(logits, ok)
    row = np.where(np.isnan(row), np.float32(-np.inf), row)
    if not (row > -np.inf).any():
        return ok, int(eos), int(state)
    tok = int(np.argmax(row))                                  # first maximum
    return ok, tok, int(next_state[state][token_class[tok]])


def simulate_greedy(logits_fn, token_class, next_state, dist, start: int, max_new: int, eos: int):
    """One row of the loop: logits_fn(step, prefix) -> fp32 [V].  -> (tokens incl. the EOS padding, final state)."""
    state, out, done = start, [], False
    for step in range(max_new):
        if done:
            out.append(eos)
            continue
        _, tok, state = greedy_step(logits_fn(step, out), token_class, next_state, dist, state, max_new - step, eos)
        out.append(tok)
        done = tok == eos
    return out, state


def brute_dist(token_class, next_state, accept) -> np.ndarray:
    """Shortest number of tokens to an accepting state, by relaxation over every (state, token-bearing class) edge (Bellman-Ford)."""
    ns, nc = next_state.shape
    used = np.zeros(nc, bool)
    used[np.unique(np.asarray(token_class))] = True
    d = [DIST_INF] * ns
    for a in accept:
        d[a] = 0
    for _ in range(ns):
        changed = False
        for s in range(ns):
            for c in range(nc):
                nx = int(next_state[s, c])
                if used[c] and nx >= 0 and d[nx] + 1 < d[s]:
                    d[s], changed = d[nx] + 1, True
        if not changed:
            break
    return np.asarray(d, np.int32)


class RandomDFA:
    """A seeded automaton for the operator tests: ``ns`` states (the last one accepting, no way out of it), ``nc`` classes, a random class
    map over ``vocab`` ids, about half of the transitions -1, ``dist`` by brute force."""

    def __init__(self, vocab: int, ns: int = 5, nc: int = 7, seed: int = 0):
        rng = np.random.default_rng(seed)
        self.token_class = rng.integers(0, nc, vocab).astype(np.int16)
        self.token_class[:nc] = np.arange(nc)                  # every class holds a token, also in the short operator rows
        nxt = rng.integers(0, ns, (ns, nc))
        nxt[rng.random((ns, nc)) < 0.5] = -1
        nxt[ns - 1] = -1
        for s in range(ns - 1):                                # every live state keeps a way on, and state 0 reaches the accepting one
            nxt[s, s % nc] = s + 1
        self.next_state = nxt.astype(np.int16)
        self.dist = brute_dist(self.token_class, self.next_state, [ns - 1])
        self.start_state = 0
        assert self.dist[0] < DIST_INF


class FreeDFA:
    """Everything is allowed: one live state on which every token loops, EOS moves to the accepting state; dist = (1, 0)."""

    def __init__(self, vocab: int, eos: int):
        self.token_class = np.zeros(vocab, np.int16)
        self.token_class[eos] = 1
        self.next_state = np.array([[0, 1], [-1, -1]], np.int16)
        self.dist = np.array([1, 0], np.int32)
        self.start_state = 0
