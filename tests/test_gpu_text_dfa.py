"""GPU: grammar-constrained text decode (pg_set_text_dfa, pg_generate_text_constrained, pg_op_text_constrain).  Masks, tokens and states are
integers and -inf patterns: every comparison against the numpy restatement (text_dfa_ref.py) is exact."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, get_engine, load_golden
from test_gpu_text_sampling import _full, _prefill
from text_dfa_ref import DIST_INF, FreeDFA, RandomDFA, accepts_layout, allowed_mask, greedy_step

pytestmark = pytest.mark.gpu

V_FULL = 102400
NEG_INF = float("-inf")


def _tiny(tiny_cfg, tiny_weights):
    return get_engine(tiny_cfg, tiny_weights, "f32"), load_golden("generate_tiny.npz")


def _rows(g, n):
    return [i % g["ids"].shape[0] for i in range(n)]


def _constrained(e, g, n, eos, rows=None, **kw):
    _prefill(e, g, rows)
    out = e.generate_text_constrained(n, eos, **kw)
    return tuple(t.cpu() for t in out) if isinstance(out, tuple) else out.cpu()


def _follow(dfa, out, lg, state_out, eos, max_new, greedy):
    """Track every row's state on the host from the emitted tokens; at every step the tap's -inf set is the reference mask, the token is
    allowed (greedy: it is the first maximum of the tap row), finished rows emit eos; the final states are the tracked ones."""
    out, lg = out.numpy(), lg.numpy()
    B, L = out.shape
    V = lg.shape[-1]
    st = [dfa.start_state] * B
    unf = [True] * B
    for t in range(L):
        for b in range(B):
            ok = allowed_mask(dfa.token_class, dfa.next_state, dfa.dist, st[b], max_new - t, V)
            row = lg[t, b]
            assert np.isfinite(row[ok]).all() and np.array_equal(np.isneginf(row), ~ok), (t, b)
            tok = int(out[b, t])
            if not unf[b]:
                assert tok == eos
                continue
            if not ok.any():
                assert tok == eos                                        # nothing kept: eos, the state stays
            else:
                assert ok[tok], (t, b, tok)
                if greedy:
                    assert tok == int(np.argmax(row)), (t, b)
                st[b] = int(dfa.next_state[st[b], dfa.token_class[tok]])
            unf[b] = tok != eos
    assert state_out.tolist() == st
    return st, unf


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("V", [37, 4100, V_FULL])
def test_operator_equals_the_restatement(V):
    e, _ = _full("f32")
    dfa = RandomDFA(V_FULL, ns=5, nc=7, seed=3)
    e.set_text_dfa(dfa)
    eos, states = 5, [0, 2, 3]
    gen = torch.Generator().manual_seed(V)
    for remaining in (1, 2, 50):
        x = torch.randn(3, V, generator=gen) * 2.4
        for b, s in enumerate(states):                                   # equal maxima: a disallowed one first, then two allowed ones
            ok = allowed_mask(dfa.token_class, dfa.next_state, dfa.dist, s, remaining, V)
            if ok.any() and not ok.all():
                x[b, int(np.nonzero(~ok)[0][0])] = 50.0
                x[b, torch.from_numpy(np.nonzero(ok)[0][-2:].copy())] = 50.0
        keep, tok, nxt = (t.cpu().numpy() for t in e.text_constrain(x, states, remaining, eos))
        some = 0
        for b, s in enumerate(states):
            ok, rt, rs = greedy_step(x[b].numpy(), dfa.token_class, dfa.next_state, dfa.dist, s, remaining, eos)
            assert np.array_equal(keep[b], ok), (V, remaining, b)
            assert (int(tok[b]), int(nxt[b])) == (rt, rs), (V, remaining, b, tok[b], rt)
            some += int(ok.any())
            if ok.any() and not ok.all() and ok.sum() >= 2:
                assert rt == int(np.nonzero(ok)[0][-2])                  # the lower of the two allowed maxima, not the disallowed one
        assert some > 0 or remaining == 1
    # every allowed logit -inf (NaN counts as -inf): eos, the state stays; a state outside the table allows nothing
    x = torch.randn(3, V, generator=gen)
    for b, s in enumerate(states):
        ok = torch.from_numpy(allowed_mask(dfa.token_class, dfa.next_state, dfa.dist, s, 50, V))
        x[b, ok] = NEG_INF if b != 1 else float("nan")
    keep, tok, nxt = e.text_constrain(x, states, 50, eos)
    assert not keep.any() and tok.cpu().tolist() == [eos] * 3 and nxt.cpu().tolist() == states
    for extra in (dict(temperature=1.5, seed=7), dict(temperature=1.5, top_k=20, seed=7), dict(temperature=1.5, top_p=0.9, seed=7)):
        keep, tok, nxt = e.text_constrain(x, states, 50, eos, **extra)                           # the same rule in the sampled and filtered forms
        assert not keep.any() and tok.cpu().tolist() == [eos] * 3 and nxt.cpu().tolist() == states, extra
    keep, tok, nxt = e.text_constrain(torch.zeros(2, V), [-1, 5], 50, eos)
    assert not keep.any() and tok.cpu().tolist() == [eos] * 2 and nxt.cpu().tolist() == [-1, 5]
    # the sampled forms draw inside the mask, and the filtered kept set lies inside it
    x = torch.randn(3, V, generator=gen) * 2.4
    for k, p in ((0, 1.0), (20, 1.0), (0, 0.9)):
        keep, tok, nxt = (t.cpu().numpy() for t in e.text_constrain(x, states, 50, eos, temperature=1.5, top_k=k, top_p=p, seed=7, step=3))
        for b, s in enumerate(states):
            ok = allowed_mask(dfa.token_class, dfa.next_state, dfa.dist, s, 50, V)
            assert not (keep[b] & ~ok).any() and keep[b].any() == ok.any()
            if ok.any():
                assert keep[b][tok[b]] and nxt[b] == dfa.next_state[s, dfa.token_class[tok[b]]]
                if k == 0 and p == 1.0:
                    assert np.array_equal(keep[b], ok)
                    free = e.text_sample(torch.where(torch.from_numpy(ok), x[b], torch.tensor(NEG_INF))[None], 1.5, 0, 1.0, seed=7, row_offset=b, step=3)[1]
                    assert int(free.cpu()[0]) == int(tok[b])             # the draw of the unconstrained sampler over the masked row


# ----------------------------------------------------------------------------------------------------------------- 2
def test_loop_equals_operator_equals_model(tiny_cfg, tiny_weights):
    e, g = _tiny(tiny_cfg, tiny_weights)
    eos, n = int(g["eos"]), 10
    dfa = RandomDFA(tiny_cfg.vocab, ns=5, nc=7, seed=11)
    e.set_text_dfa(dfa)
    out, lg, st = _constrained(e, g, n, eos, return_logits=True, return_state=True)
    B = out.shape[0]
    assert lg.shape == (out.shape[1], B, tiny_cfg.vocab)
    _follow(dfa, out, lg, st, eos, n, greedy=True)
    # the operator on the tapped rows gives the loop's tokens
    states = [dfa.start_state] * B
    _, tok, nxt = e.text_constrain(lg[0], states, n, eos)
    assert torch.equal(tok.cpu().long(), out[:, 0])
    # step 0: the finite entries are the unconstrained loop's logits, bit for bit
    _prefill(e, g)
    _, free = e.generate_text(n, eos, temperature=0.0, return_logits=True)
    fin = torch.isfinite(lg[0])
    assert fin.any() and torch.equal(lg[0][fin], free[0].cpu()[fin])


# ----------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("k,p", [(0, 1.0), (20, 1.0), (0, 0.9)])
def test_every_row_is_a_whole_layout_inside_the_budget(tiny_cfg, tiny_weights, k, p):
    from plangen_amd.grammar import layout_token_dfa
    from plangen_amd.textproc import GROUNDING_OPEN, TagWordCodec, cut_plan_text
    e, g = _tiny(tiny_cfg, tiny_weights)
    codec = TagWordCodec(tiny_cfg.vocab, eos_id=tiny_cfg.eos_id, pad_id=tiny_cfg.pad_id)
    dfa = layout_token_dfa(codec, tiny_cfg.vocab)
    e.set_text_dfa(dfa)
    eos = tiny_cfg.eos_id
    longest = 0
    for max_new in (int(dfa.dist[dfa.start_state]), 24, 40):
        out = _constrained(e, g, max_new, eos, rows=_rows(g, 4), temperature=1.5, top_k=k, top_p=p, seed=17 + max_new)
        assert out.shape[0] == 4 and out.shape[1] <= max_new
        for row in out.tolist():
            assert eos in row, row                                       # every row ends in EOS
            body = row[:row.index(eos)]
            assert all(t == eos for t in row[len(body):])
            text = codec.decode(body)
            assert accepts_layout(text), text
            assert cut_plan_text(codec.decode(row)) == GROUNDING_OPEN + text
            longest = max(longest, len(body) + 1)
    assert longest > 2                                                   # not only the empty layout


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=1.0, seed=5), dict(temperature=1.0, top_k=30, top_p=0.9, seed=6)])
def test_an_automaton_that_allows_everything_changes_nothing(tiny_cfg, tiny_weights, kw):
    e, g = _tiny(tiny_cfg, tiny_weights)
    eos, n = int(g["eos"]), 10
    e.set_text_dfa(FreeDFA(tiny_cfg.vocab, eos))
    got = _constrained(e, g, n, eos, **kw)
    _prefill(e, g)
    ref = e.generate_text(n, eos, min_new_tokens=0, **kw).cpu()
    pad = lambda t: torch.cat([t, torch.full((t.shape[0], n - t.shape[1]), eos, dtype=t.dtype)], 1)
    got, ref = pad(got), pad(ref)
    assert torch.equal(got[:, :n - 1], ref[:, :n - 1])
    running = (ref[:, :n - 1] != eos).all(1)
    assert running.any() or not kw["temperature"] > 0
    assert (got[running, n - 1] == eos).all()                            # the budget forces the EOS in the last column
    assert torch.equal(got[~running, n - 1], ref[~running, n - 1])


# ----------------------------------------------------------------------------------------------------------------- 5
def test_execution_forms(tiny_cfg, tiny_weights):
    e, g = _tiny(tiny_cfg, tiny_weights)
    eos, n = int(g["eos"]), 12
    d1, d2 = RandomDFA(tiny_cfg.vocab, seed=21), RandomDFA(tiny_cfg.vocab, ns=6, nc=9, seed=22)
    kw = dict(temperature=1.2, top_k=40, top_p=0.95, seed=31)
    runs = {}
    for name, d in (("d1", d1), ("d2", d2)):
        e.set_text_dfa(d)
        runs[name] = _constrained(e, g, n, eos, return_logits=True, return_state=True, **kw)
        runs[name + "g"] = _constrained(e, g, n, eos, return_logits=True, return_state=True)
        _follow(d, *runs[name], eos, n, greedy=False)
        _follow(d, *runs[name + "g"], eos, n, greedy=True)
    assert not torch.equal(runs["d1"][0], runs["d2"][0])
    e.set_option("use_graph", 1)
    try:
        # one mode, no tap (the tap's address is part of the graph key), three calls in a row: the step graph the first call captures under
        # d1 is the one the next two replay, under d2's tables and then d1's again (same handle, same addresses, new contents)
        for key, extra in (("", kw), ("g", {})):
            for name, d in (("d1", d1), ("d2", d2), ("d1", d1)):
                e.set_text_dfa(d)
                out, st = _constrained(e, g, n, eos, return_state=True, **extra)
                assert torch.equal(out, runs[name + key][0]) and torch.equal(st, runs[name + key][2]), (name, key)
        # with the tap (re-captured per call): eager == graph, logits included
        e.set_text_dfa(d2)
        for key, extra in (("d2", kw), ("d2g", {})):
            got = _constrained(e, g, n, eos, return_logits=True, return_state=True, **extra)
            assert all(torch.equal(a, b) for a, b in zip(got, runs[key])), key
    finally:
        e.set_option("use_graph", 0)
    # a row's tokens do not depend on its neighbours: 4 rows == 2 + 2 with rng_image_offset
    e.set_text_dfa(d2)
    rows = _rows(g, 4)
    whole = _constrained(e, g, n, eos, rows=rows, **kw)
    pad = lambda t: torch.cat([t, torch.full((t.shape[0], n - t.shape[1]), eos, dtype=t.dtype)], 1)
    head = _constrained(e, g, n, eos, rows=rows[:2], **kw)
    e.set_option("rng_image_offset", 2)
    try:
        tail = _constrained(e, g, n, eos, rows=rows[2:], **kw)
    finally:
        e.set_option("rng_image_offset", 0)
    assert torch.equal(pad(whole), torch.cat([pad(head), pad(tail)]))


# ----------------------------------------------------------------------------------------------------------------- 6
def test_full_vocabulary_bf16():
    e, s = _full("bf16")
    g, eos, n = s["g"], s["cfg"].eos_id, 8
    dfa = RandomDFA(V_FULL, ns=8, nc=12, seed=41)
    e.set_text_dfa(dfa)
    kw = dict(temperature=1.0, top_k=50, top_p=0.9, seed=5)
    a = _constrained(e, g, n, eos, rows=slice(0, 3), return_logits=True, return_state=True, **kw)
    b = _constrained(e, g, n, eos, rows=slice(0, 3), return_logits=True, return_state=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].shape[0] == 3
    _follow(dfa, *a, eos, n, greedy=False)
    _follow(dfa, *_constrained(e, g, n, eos, rows=slice(0, 3), return_logits=True, return_state=True), eos, n, greedy=True)


# ----------------------------------------------------------------------------------------------------------------- 7
def test_errors_leave_the_handle_usable(tiny_cfg, tiny_weights):
    from types import SimpleNamespace
    from plangen_amd.engine import PlanGenError
    e, g = _tiny(tiny_cfg, tiny_weights)
    eos, V = int(g["eos"]), tiny_cfg.vocab
    good = RandomDFA(V, seed=51)

    def raises(status, fn):
        with pytest.raises(PlanGenError) as ei:
            fn()
        assert status in str(ei.value), ei.value

    e.set_text_dfa(None)
    _prefill(e, g)
    raises("PG_ERR_STATE", lambda: e.generate_text_constrained(8, eos))
    raises("PG_ERR_STATE", lambda: e.text_constrain(torch.zeros(1, 8), [0], 4, eos))
    wide = SimpleNamespace(token_class=np.zeros(V, np.int16), next_state=np.zeros((2, 1025), np.int16), dist=np.array([1, 0], np.int32), start_state=0)
    raises("PG_ERR_ARG", lambda: e.set_text_dfa(wide))
    cls = good.token_class.copy(); cls[V - 1] = good.next_state.shape[1]
    raises("PG_ERR_ARG", lambda: e.set_text_dfa(SimpleNamespace(token_class=cls, next_state=good.next_state, dist=good.dist, start_state=0)))
    nxt = good.next_state.copy(); nxt[1, 2] = good.next_state.shape[0]
    raises("PG_ERR_ARG", lambda: e.set_text_dfa(SimpleNamespace(token_class=good.token_class, next_state=nxt, dist=good.dist, start_state=0)))
    raises("PG_ERR_ARG", lambda: e.set_text_dfa(SimpleNamespace(token_class=good.token_class, next_state=good.next_state, dist=good.dist, start_state=5)))
    assert 1 < good.dist[0] < DIST_INF
    dist = good.dist.copy(); dist[0] -= 1                                # a promise the tables do not keep: nothing leads from state 0 to dist - 2
    raises("PG_ERR_ARG", lambda: e.set_text_dfa(SimpleNamespace(token_class=good.token_class, next_state=good.next_state, dist=dist, start_state=0)))
    raises("PG_ERR_STATE", lambda: e.generate_text_constrained(8, eos))                          # a refused upload sets nothing
    e.set_text_dfa(good)
    raises("PG_ERR_ARG", lambda: e.generate_text_constrained(int(good.dist[0]) - 1, eos))        # dist[start] > max_new
    raises("PG_ERR_ARG", lambda: e.generate_text_constrained(8, eos, temperature=1.0, top_k=-1))
    raises("PG_ERR_ARG", lambda: e.generate_text_constrained(8, eos, temperature=1.0, top_p=0.0))
    assert e.generate_text_constrained(int(good.dist[0]), eos).shape[0] == g["ids"].shape[0]     # the same prefill is still good
    _prefill(e, g)
    assert np.array_equal(e.generate_text_greedy(10, eos).cpu().numpy(), g["out"])


# ----------------------------------------------------------------------------------------------------------------- 8
def test_through_uni_generate(tiny_cfg, tiny_weights):
    from types import SimpleNamespace
    from plangen_amd.system import System
    from plangen_amd.textproc import GROUNDING_OPEN, TagWordCodec, trans_gr_to_creati
    from text_dfa_ref import n_items
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    codec = TagWordCodec(tiny_cfg.vocab, eos_id=tiny_cfg.eos_id, pad_id=tiny_cfg.pad_id)
    base = dict(seed=3, parallel_size=1, cfg_weight=5.0, temperature=0.0, use_teacher_forcing=False, debug_max_seq_len=None,
                janus_hw=tiny_cfg.img_size, neg_prompt="", use_neg_box=False, text_temperature=1.5)
    captions = ["a red cat on the left", "two dogs", "a bike"]

    def run(**extra):
        s = System(tiny_cfg, e, SimpleNamespace(**base, **extra), codec=codec)
        ids1, mask1 = s.pad_input_ids([s.wrap_uni_prompt(c, GROUNDING_OPEN, in_stage1=True)[1].tolist() for c in captions])
        seen = []
        wrap = s.wrap_uni_prompt
        s.wrap_uni_prompt = lambda c, gr=None, in_stage1=False: (seen.append((c, gr)), wrap(c, gr, in_stage1))[1]
        batch = dict(base_caption=captions, uni_stage1_inputs_ids=ids1, uni_stage1_attention_mask=mask1)
        return s.uni_generate(batch, pred_layout=True, pred_image=True, max_new_tokens=24), seen

    out, seen = run(layout_grammar=True)
    eos = tiny_cfg.eos_id
    assert len(out["pr_grounding"]) == 3
    for row, gr in zip(out["pr_layout_ids"].cpu().tolist(), out["pr_grounding"]):
        assert eos in row and codec.decode(row[:row.index(eos)]).endswith("</grounding>")       # closed by the model, not by the fallback
        assert gr and gr.startswith(GROUNDING_OPEN) and accepts_layout(gr[len(GROUNDING_OPEN):]), gr
        assert len(trans_gr_to_creati(gr)[0]) == n_items(gr)
    assert seen[:3] == list(zip(captions, out["pr_grounding"]))              # the stage-2 prompts carry these layouts
    assert out["pr_image"].shape[0] == 3
    free, _ = run()                                                      # key absent: the unconstrained sampler, which does not keep the format
    assert not all(accepts_layout(gr[len(GROUNDING_OPEN):]) and eos in row
                   for row, gr in zip(free["pr_layout_ids"].cpu().tolist(), free["pr_grounding"]))


@pytest.mark.parametrize("task", ["uni_2stage", "plan"])
def test_through_the_cli(tmp_path, task):
    import json
    import train
    from project.plangen.plangen_base import System as CliSystem
    from plangen_amd.textproc import GROUNDING_OPEN
    opts = ["test=True", "tiny=True", "test_batch_size=2", "max_test_len=1", "dtype='f32'", "temperature=0.0", f"out_path={str(tmp_path / 'a')!r}",
            f"test_data.task_type={task!r}", "max_new_tokens=24", "max_prompt=160", "layout_grammar=True", "text_temperature=1.5"]
    a = train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", *opts])
    assert a.layout_grammar is True
    m = CliSystem(a, None)
    calls = []
    orig = m.engine.generate_text_constrained
    m.engine.generate_text_constrained = lambda *args, **kw: (calls.append(kw), orig(*args, **kw))[1]
    m.setup_data(None)
    m.resume(None)
    m.validation(0)
    m.engine.close()
    assert len(calls) == 1 and calls[0]["temperature"] == 1.5
    base = os.path.join(str(tmp_path / "a"), "test", f"synthetic_{task}_1")
    lay = json.load(open(os.path.join(base, "0_batch", "0_layout.json")))
    assert len(lay["pr_grounding"]) == 2
    for gr in lay["pr_grounding"]:
        assert gr.startswith(GROUNDING_OPEN) and accepts_layout(gr[len(GROUNDING_OPEN):]), gr
    assert len(os.listdir(os.path.join(base, "0", "pr_image"))) == (2 if task == "uni_2stage" else 0)
