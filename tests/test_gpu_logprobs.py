"""GPU: token log-probabilities (pg_request_token_logprobs, pg_op_token_logprob) against the fp64 reference of logprob_ref.py, with the
comparison |lp - lp64| <= 1e-4 + 1e-6 |lp64| (derivation: logprob_ref.py); infinities must agree exactly.  The loops are checked on their
own tapped logits and emitted tokens, and a scored call must return the tokens and logits of the unscored call bit for bit."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import get_engine, load_golden
import logprob_ref as LR
from test_gpu_sampling_filters import _prompt
from test_gpu_text_sampling import _prefill
from text_dfa_ref import RandomDFA

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
T_IMG = 12


def _assert_close(lp, ref, what):
    lp, ref = np.asarray(lp, np.float64), np.asarray(ref, np.float64)
    print(f"{what}: max |lp - lp64| = {LR.max_excess(lp, ref):.3e} over {np.isfinite(ref).sum()} finite, {np.isinf(ref).sum()} -inf entries")
    ok = LR.close(lp, ref)
    assert ok.all(), (what, np.argwhere(~ok)[:8].tolist(), lp[~ok][:8], ref[~ok][:8])


# ----------------------------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [1, 5, 1000, 1023, 16384, 102400])
def test_operator_against_fp64(tiny_cfg, tiny_weights, V, B):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = torch.Generator().manual_seed(V * 7 + B)
    base = torch.randn(B, V, generator=g) * 2.4
    rows = {"plain": base, "x40": base * 40.0}                           # x40: exp overflows without the max-subtraction
    sp = base.clone()
    sp[:, 0] = NEG_INF
    if V > 4:
        sp[:, V // 2] = float("nan"); sp[0, V - 2] = NEG_INF
    rows["holes"] = sp
    pinf = base.clone()
    pinf[:, V - 1] = float("inf")
    if V > 4:
        pinf[0, 1] = float("inf")
    rows["plus_inf"] = pinf
    rows["empty"] = torch.full((B, V), NEG_INF)
    rnd = torch.randint(0, V, (B,), generator=g).int()
    toks = {"first": torch.zeros(B, dtype=torch.int32), "last": torch.full((B,), V - 1, dtype=torch.int32), "random": rnd,
            "outside": torch.tensor(([V, -1, V + 5] * B)[:B], dtype=torch.int32)}
    for name, x in rows.items():
        for temp in (0.0, 0.5, 3.0):
            for tname, tok in toks.items():
                lp = e.token_logprob(x, tok, temp).cpu().numpy()
                ref = LR.token_logprob_ref(x.numpy(), tok.numpy(), temp)
                _assert_close(lp, ref, f"V={V} B={B} {name} T={temp} tok={tname}")
                if name == "holes" and tname == "first" or name == "empty" or tname == "outside":
                    assert np.isneginf(lp).all()                         # token on a -inf entry / no finite entry / out of range


# ----------------------------------------------------------------------------------------------------------------- image loop
IMAGE_MODES = {
    "greedy": dict(temperature=0.0),
    "sampled": dict(temperature=0.8, seed=5),
    "filtered": dict(temperature=0.8, seed=5, top_k=9, top_p=0.8),
}


def _image_modes(cfg, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    force = torch.randint(0, cfg.img_vocab, (B, T_IMG), generator=g, dtype=torch.int32)
    part = (torch.rand(B, T_IMG, generator=g) < 0.5).to(torch.uint8)
    modes = dict(IMAGE_MODES)
    modes["scoring"] = dict(temperature=0.8, seed=5, force_tokens=force, force_mask=torch.zeros(B, T_IMG, dtype=torch.uint8))
    modes["forced_part"] = dict(temperature=0.8, seed=5, force_tokens=force, force_mask=part)
    modes["forced_no_mask"] = dict(temperature=0.0, force_tokens=force)
    return modes


def _image_pair(e, prefill, kw):
    """(tokens, logits) of the unscored call and (tokens, logits, logprobs) of the scored one, same prefill, same arguments"""
    prefill()
    plain = e.decode_image_tokens(T=T_IMG, cfg_weight=5.0, return_logits=True, **kw)
    prefill()
    scored = e.decode_image_tokens(T=T_IMG, cfg_weight=5.0, return_logits=True, return_logprobs=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu() for t in plain], [t.cpu() for t in scored]


def _check_image(plain, scored, kw, what):
    assert torch.equal(plain[0], scored[0]), what                        # tokens: bit-equal to the unscored call
    assert torch.equal(plain[1], scored[1]), what                        # logits_out too
    toks, lg, lp = scored
    assert lp.shape == toks.shape and lp.dtype == torch.float32
    _assert_close(lp.numpy(), LR.image_logprobs_ref(lg.numpy(), toks.numpy(), kw["temperature"]), what)
    return lp


def test_image_loop_modes(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 3, 91)
    results = {}
    for name, kw in _image_modes(tiny_cfg, 3).items():
        plain, scored = _image_pair(e, lambda: e.prefill(ids, pad), kw)
        results[name] = _check_image(plain, scored, kw, name)
        if name == "scoring":                                            # the emitted tokens are the given ones: their log-likelihood
            assert torch.equal(scored[0], kw["force_tokens"])
        if name == "forced_no_mask":                                     # the emitted token is the model's own, and so is the score
            assert not torch.equal(scored[0], kw["force_tokens"])
    # top-k / top-p do not renormalise: where the filtered and the unfiltered call drew the same token from the same context, same score
    assert torch.isfinite(results["filtered"]).all()


def test_image_loop_under_graph_replicas_and_fp8(tiny_cfg, tiny_weights):
    kw = IMAGE_MODES["sampled"]
    # use_graph = 1: the scored step is captured (a scored call after an unscored one re-captures) and equals the eager result
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 92)
    eager_plain, eager = _image_pair(e, lambda: e.prefill(ids, pad), kw)
    e.set_option("use_graph", 1)
    try:
        plain, scored = _image_pair(e, lambda: e.prefill(ids, pad), kw)
        _check_image(plain, scored, kw, "graph")
        assert all(torch.equal(a, b) for a, b in zip(scored, eager))
    finally:
        e.set_option("use_graph", 0)
    # after pg_prefill_replicated (2 replicas, aliased prompts)
    er = get_engine(tiny_cfg, tiny_weights, "f32", max_rows=12, max_prompt=192)
    plain, scored = _image_pair(er, lambda: er.prefill_replicated(ids, pad, 2, alias=True), kw)
    lp = _check_image(plain, scored, kw, "replicated")
    assert lp.shape[0] == 4 and not torch.equal(scored[0][:2], scored[0][2:])        # replicas draw different images
    # FP8 KV cache
    e8 = get_engine(tiny_cfg, tiny_weights, "bf16", kv_dtype="fp8")
    plain, scored = _image_pair(e8, lambda: e8.prefill(ids, pad), kw)
    _check_image(plain, scored, kw, "fp8-kv")


# ----------------------------------------------------------------------------------------------------------------- text loop
def _text_pair(e, g, gen, n, kw):
    _prefill(e, g)
    plain = gen(n, return_logits=True, **kw)
    _prefill(e, g)
    scored = gen(n, return_logits=True, return_logprobs=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu() for t in plain], [t.cpu() for t in scored]


def _check_text(plain, scored, eos, temperature, what):
    assert len(scored) == len(plain) + 1
    for a, b in zip(plain, scored):
        assert torch.equal(a, b), what                                   # tokens, logits (and states): bit-equal to the unscored call
    toks, lg, lp = scored[0], scored[1], scored[-1]
    assert lp.shape == toks.shape and lp.dtype == torch.float32
    ref = LR.text_logprobs_ref(lg.numpy(), toks.numpy(), eos, temperature)
    _assert_close(lp.numpy(), ref, what)
    done = (toks == eos).int().cumsum(1) - (toks == eos).int() > 0       # columns after a row's first EOS
    assert (lp[done] == 0).all()
    return toks, lg, lp, done


@pytest.mark.parametrize("name,kw", [("greedy", dict(temperature=0.0)), ("sampled", dict(temperature=1.2, seed=4)),
                                     ("filtered_min_new", dict(temperature=1.2, seed=4, top_k=30, top_p=0.9, min_new_tokens=2))])
def test_text_loop_modes(tiny_cfg, tiny_weights, name, kw):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    eos, n = int(g["eos"]), 10
    gen = lambda n_, **k: e.generate_text(n_, eos, **k)
    plain, scored = _text_pair(e, g, gen, n, kw)
    toks, lg, lp, done = _check_text(plain, scored, eos, kw["temperature"], name)
    if name == "greedy":
        assert np.array_equal(toks.numpy(), g["out"])
        assert toks[1, 0] == eos and done[1, 1:].all() and lp[1, 0] < 0  # row 1 finishes at once: its EOS is scored, the rest is 0.0
        assert (lp[0] < 0).all() and (lp[2] < 0).all()
    if name == "filtered_min_new":
        # the EOS ban renormalises: the banned entry is -inf in the tap, and row 1 (which wants EOS at once) pays for its second choice
        assert torch.isneginf(lg[:2, :, eos]).all() and (toks[:, :2] != eos).all() and torch.isfinite(lp[:, :2]).all()


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=1.2, seed=8), dict(temperature=1.2, seed=8, top_k=20, top_p=0.9)],
                         ids=["greedy", "sampled", "filtered"])
def test_text_loop_constrained(tiny_cfg, tiny_weights, kw):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    eos, n = int(g["eos"]), 10
    e.set_text_dfa(RandomDFA(tiny_cfg.vocab, ns=5, nc=7, seed=11))
    gen = lambda n_, **k: e.generate_text_constrained(n_, eos, return_state=True, **k)
    plain, scored = _text_pair(e, g, gen, n, kw)
    toks, lg, lp, done = _check_text(plain, scored, eos, kw["temperature"], f"constrained {kw}")
    assert torch.isneginf(lg).any()                                      # the mask is in the rows the scores are normalised over
    # an emitted token is an allowed one; -inf only for the "nothing kept" emission of eos from a state that allows nothing finite
    empty = ~torch.isfinite(lg).any(-1).T                                # [B, n]
    assert torch.equal(torch.isneginf(lp), empty & ~done) and (toks[torch.isneginf(lp)] == eos).all()


def test_text_columns_past_out_len_stay_untouched(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    eos, n = int(g["eos"]), 12
    _prefill(e, g, rows=[1, 1, 1])                                       # three copies of the row that emits EOS at once
    lp = torch.full((3, n), 123.0, dtype=torch.float32, device=e.device)
    e._check(e.lib.pg_request_token_logprobs(e.h, e._p(lp), lp.numel()), "pg_request_token_logprobs")
    out = e.generate_text(n, eos, temperature=0.0)
    torch.cuda.synchronize()
    assert out.shape[1] < n and (out.cpu()[:, 0] == eos).all()
    lp = lp.cpu()
    assert (lp[:, out.shape[1]:] == 123.0).all() and (lp[:, 0] < 0).all() and (lp[:, 1:out.shape[1]] == 0).all()


# ----------------------------------------------------------------------------------------------------------------- one-shot
def test_one_shot_semantics(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 93)
    B, T = 2, T_IMG
    SENT = 77.0

    def request(buf, cap=None):
        return e.lib.pg_request_token_logprobs(e.h, e._p(buf), buf.numel() if cap is None else cap)

    def fresh():
        return torch.full((B, T), SENT, dtype=torch.float32, device=e.device)

    def untouched(buf):
        torch.cuda.synchronize()
        return bool((buf == SENT).all())

    # a failing call consumes the request too
    e.prefill(ids, pad)
    buf = fresh()
    assert request(buf) == 0
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.decode_image_tokens(T=T, temperature=1.0, top_k=-1)
    ref = e.decode_image_tokens(T=T, temperature=0.0).cpu()              # the same prefill is still good, and nothing is scored
    assert untouched(buf)
    # a scored call, then a second decode without a new request: nothing goes to the old pointer
    e.prefill(ids, pad)
    assert request(buf) == 0
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref)
    torch.cuda.synchronize()
    assert bool((buf < 0).all())
    buf.fill_(SENT)
    e.prefill(ids, pad)
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(buf)
    # too small a capacity: PG_ERR_ARG at the consuming call, nothing launched, the handle (and the prefill) stay usable
    e.prefill(ids, pad)
    assert request(buf, B * T - 1) == 0
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.decode_image_tokens(T=T, temperature=0.0)
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(buf)
    assert request(buf, 0) == -1                                         # capacity_floats < 1 is refused at once
    # NULL cancels
    e.prefill(ids, pad)
    assert request(buf) == 0 and e.lib.pg_request_token_logprobs(e.h, None, 0) == 0
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(buf)
    # lanes = 2 with a request: PG_ERR_ARG at decode time
    e.set_option("lanes", 2)
    try:
        e.prefill(ids, pad)
        assert request(buf) == 0
        with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
            e.decode_image_tokens(T=T, temperature=0.0)
    finally:
        e.set_option("lanes", 1)
    assert untouched(buf)
    # the library-owned score buffer is counted
    assert e.lib.pg_device_bytes(e.h) > 0


# ----------------------------------------------------------------------------------------------------------------- System
def _args(cfg, **kw):
    base = dict(seed=13, parallel_size=2, cfg_weight=5.0, temperature=1.0, top_k=0, top_p=1.0, use_teacher_forcing=False,
                debug_max_seq_len=None, janus_hw=cfg.img_size, neg_prompt="", use_neg_box=False)
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("share", [0, 1])
def test_t2i_select_best_keeps_the_higher_scoring_replica(tiny_cfg, tiny_weights, share):
    from plangen_amd.system import System
    e = get_engine(tiny_cfg, tiny_weights, "f32", max_rows=12, max_prompt=192)
    ids, pad, _ = _prompt(tiny_cfg, 2, 94)
    from test_gpu_sampling_filters import _MASKS
    mask = _MASKS[id(ids)]
    B0, p, T = 2, 2, tiny_cfg.img_tokens
    # the plain parallel_size = 2 run: all 4 images' tokens, and the logits they were drawn from
    s = System(tiny_cfg, e, _args(tiny_cfg, share_replicas=share))
    rep_mask = torch.cat([mask] * p)
    toks, lg = s.sample_image(ids if share else torch.cat([ids] * p), rep_mask, 5.0, 1.0, 13, return_logits=True, replicas=p if share else 1)
    toks, lg = toks.cpu(), lg.cpu()
    score = LR.image_logprobs_ref(lg.numpy(), toks.numpy(), 1.0).mean(1).reshape(p, B0)      # row t * B0 + i
    margin = np.abs(score[0] - score[1])
    print("replica scores", score.tolist())
    assert (margin > 1e-3).all(), margin                                 # far above the tolerance of a mean of T scores: the choice is not a coin flip
    best = score.argmax(0)
    want = e.vq_decode(toks[torch.from_numpy(best) * B0 + torch.arange(B0)]).cpu()
    # select_best
    s2 = System(tiny_cfg, e, _args(tiny_cfg, share_replicas=share, select_best=True))
    dec, _ = s2.t2i(ids, mask)
    assert dec.shape[0] == B0 and torch.equal(dec.cpu(), want)
    assert s2.last_selection["replica"].cpu().tolist() == best.tolist()
    assert torch.equal(s2.last_generated_tokens.cpu(), toks[torch.from_numpy(best) * B0 + torch.arange(B0)])
    _assert_close(s2.last_selection["scores"].cpu().numpy(), score, "select_best scores")


def test_uni_generate_layout_best_of(tiny_cfg, tiny_weights):
    from plangen_amd.system import System
    from plangen_amd.textproc import GROUNDING_OPEN, TagWordCodec
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    codec = TagWordCodec(tiny_cfg.vocab, eos_id=tiny_cfg.eos_id, pad_id=tiny_cfg.pad_id)
    captions = ["a red cat on the left", "two dogs", "a bike"]
    N, B, eos = 2, 3, tiny_cfg.eos_id
    base = dict(parallel_size=1, temperature=0.0, seed=3, text_temperature=1.5, layout_grammar=True)

    def batch_of(s, caps):
        ids1, mask1 = s.pad_input_ids([s.wrap_uni_prompt(c, GROUNDING_OPEN, in_stage1=True)[1].tolist() for c in caps])
        return dict(base_caption=caps, uni_stage1_inputs_ids=ids1, uni_stage1_attention_mask=mask1)

    # the plain replicated batch (row t * B + i = draw t of caption i), with its scores from the engine's own log-probs
    s = System(tiny_cfg, e, _args(tiny_cfg, **base), codec=codec)
    from plangen_amd.grammar import layout_token_dfa
    b = batch_of(s, captions * N)
    emb = s.vl_gpt.language_model.get_input_embeddings()(b["uni_stage1_inputs_ids"].to(e.device))
    toks, lp = s.x2t(emb, b["uni_stage1_attention_mask"].to(e.device), max_new_tokens=24, dfa=layout_token_dfa(codec, tiny_cfg.vocab),
                     return_logprobs=True)
    toks, lp = toks.cpu(), lp.cpu().double()
    assert not torch.equal(toks[:B], toks[B:])                           # the two draws differ
    count = torch.tensor([row.index(eos) + 1 if eos in row else len(row) for row in toks.tolist()])
    score = (lp.sum(1) / count).view(N, B)
    print("layout scores", score.tolist())
    same = torch.tensor([toks[i].tolist() == toks[B + i].tolist() for i in range(B)])
    # two different layouts of a caption score far apart (no coin flip); the same layout drawn twice is a tie, which goes to the first draw
    assert (((score[0] - score[1]).abs() > 1e-4) | same).all() and not same.all()
    best = torch.where(same, torch.zeros(B, dtype=torch.long), score.argmax(0))
    # layout_best_of = 2 on the un-replicated batch
    s2 = System(tiny_cfg, e, _args(tiny_cfg, layout_best_of=N, **base), codec=codec)
    out = s2.uni_generate(batch_of(s2, captions), pred_layout=True, pred_image=False, max_new_tokens=24)
    assert out["pr_layout_replica"].cpu().tolist() == best.tolist()
    assert torch.equal(out["pr_layout_ids"].cpu(), toks[best * B + torch.arange(B)])
    assert np.allclose(out["pr_layout_score"].cpu().numpy(), score.gather(0, best.view(1, B))[0].numpy(), atol=1e-5)
    assert len(out["pr_grounding"]) == B
