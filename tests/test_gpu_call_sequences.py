"""GPU: no call on a pg_engine handle depends on the calls before it.

Every result a call returns, and every KV-cache slot it writes, must be bit for bit what a FRESH handle (same config, weights and options)
returns for that call alone -- whatever the first handle did before.  The engine is deterministic by design (no atomics in reductions,
split-K slabs folded in a fixed order), so there is no tolerance: the only oracle here is a fresh handle.  The state that could leak is
listed in DESIGN.md ("Per-handle state that survives a call"): the instantiated decode graphs and their keys, the double-buffered pinned
staging of pg_prefill, the row-set geometry of the last prefill, the one-shot hint and requests, the lane rebasing of decode_image, the
lazily allocated buffers, the installed text automaton, the step counters, and the previous batch's keys (and FP8 scales) in the cache.

The handles are private to this file (call_sequences.make_engine) and closed when the module ends: options set here cannot reach other
tests, and other tests cannot pre-age the veteran.  Each group keeps one veteran handle per parametrisation; each checked step builds a
fresh handle, runs that step alone on it and closes it."""
import pytest
import torch

import call_sequences as cs
from call_sequences import Step, batch, chain_call, codes, image_call, prefill_hidden, prefill_only, rejected, run_sequence, score_image_call, \
    score_text_call, text_call

pytestmark = pytest.mark.gpu

ENGINES = {"f32": ("f32", "bf16"), "bf16": ("bf16", "bf16"), "bf16-fp8": ("bf16", "fp8")}
GRAPH = dict(use_graph=1)


@pytest.fixture(scope="module", autouse=True)
def _close_private_handles():
    yield
    cs.close_all()


def _maker(tiny_cfg, tiny_weights, eng, diag=False):
    dtype, kv = ENGINES[eng]
    return lambda: cs.make_engine(tiny_cfg, tiny_weights, dtype, kv_dtype=kv, diag=diag)


def _force(cfg, B, T, seed, masked):
    """Forced tokens [B, T], and with ``masked`` a mask that lets about half of the positions sample freely."""
    g = torch.Generator().manual_seed(seed)
    kw = dict(force_tokens=codes(cfg, B, T, seed))
    if masked:
        kw["force_mask"] = (torch.rand(B, T, generator=g) > 0.5).to(torch.uint8)
    return kw


# ----------------------------------------------------------------------------------------------------------------- control
@pytest.mark.parametrize("eng", list(ENGINES))
def test_control_two_fresh_handles_agree(tiny_cfg, tiny_weights, eng):
    """The premise of every test below: one call on two fresh handles gives the same bits (tokens, logits, log-probs, stats, cache)."""
    make = _maker(tiny_cfg, tiny_weights, eng)
    b = batch(tiny_cfg, (9, 5, 30, 5), seed=100, shared_neg=True)
    for opts in ({}, GRAPH):
        call = image_call(b, 8, opts, temperature=1.0, top_k=20, top_p=0.9, seed=4, return_logits=True, return_logprobs=True, return_stats=3)
        bad = cs.differences(cs.fresh_result(make, call), cs.fresh_result(make, call))
        assert not bad, f"control ({opts}): two fresh handles disagree -- " + "; ".join(bad)


# ----------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("eng", ["f32", "bf16"])
def test_a_graph_replay_across_different_batches(tiny_cfg, tiny_weights, eng):
    """use_graph = 1 throughout.  The instantiated step graph is replayed while its key holds and re-captured when it changes; everything
    outside the key reaches the kernels through device memory the next prefill rewrites.  Steps 0-3 keep every key field but shared_len
    equal (R = 4, no logits_out, log-probs requested, unfiltered), so only shared_len tells a shared negative prompt from per-sample ones;
    the later steps vary ids, L, padding, R, share_uncond, tune_epoch, the sampler and the outputs."""
    cfg = tiny_cfg
    shared = lambda seed, lens=(9, 5, 30, 5), L=None: batch(cfg, lens, seed, L, shared_neg=True)
    own = lambda seed, lens=(12, 4, 7, 9), L=None: batch(cfg, lens, seed, L)
    lp = dict(return_logprobs=True)
    off = dict(use_graph=1, share_uncond=0)
    steps = [
        Step("shared negative, greedy", image_call(shared(1), 8, GRAPH, temperature=0.0, **lp)),
        Step("per-sample negatives, same key but shared_len", image_call(own(2, L=14), 8, GRAPH, temperature=1.0, seed=3, **lp)),
        Step("shared negative of another length, device ids", image_call(shared(3, (6, 11, 21, 11)), 10, GRAPH, on_device=True, temperature=0.0, **lp)),
        Step("per-sample negatives again", image_call(own(4, (3, 8, 8, 2)), 6, GRAPH, temperature=1.0, seed=9, **lp)),
        Step("70-token prompt in row 0, top-k / top-p", image_call(shared(5, (70, 6, 3, 6)), 6, GRAPH, temperature=1.0, top_k=20, top_p=0.9, seed=5)),
        Step("1-token prompt in row 0, forced, logits", image_call(own(6, (1, 2, 17, 1)), 12, GRAPH, temperature=0.0, return_logits=True,
                                                                 **_force(cfg, 2, 12, 60, False))),
        Step("shared, forced under a mask", image_call(shared(7, (4, 9, 19, 9), L=20), 7, GRAPH, temperature=1.0, seed=2, **_force(cfg, 2, 7, 61, True))),
        Step("tune_epoch moves", cs.bump_tune_epoch, False),
        Step("per-sample, forced without a mask, after the epoch moved", image_call(own(8), 9, GRAPH, temperature=0.0, return_logits=True,
                                                                                        **_force(cfg, 2, 9, 62, False))),
        Step("R = 8, shared", image_call(shared(9, (9, 5, 30, 5, 2, 5, 14, 5)), 8, GRAPH, temperature=1.0, seed=7, **lp)),
        Step("R = 8, per-sample", image_call(own(10, (3, 9, 1, 4, 22, 6, 5, 5)), 8, GRAPH, temperature=1.0, seed=7, **lp)),
        Step("R = 2", image_call(batch(cfg, (13, 4), 11), 8, GRAPH, temperature=0.0, return_logits=True)),
        Step("R = 4 again, shared", image_call(shared(12), 8, GRAPH, temperature=0.0, **lp)),
        Step("share_uncond off, shared ids", image_call(shared(13), 8, off, temperature=0.0, **lp)),
        Step("share_uncond off, per-sample", image_call(own(14), 8, off, temperature=1.0, seed=1, **lp)),
        Step("share_uncond on again, shared ids", image_call(shared(15), 8, GRAPH, temperature=1.0, seed=1, **lp)),
        Step("eager after all the graphs", image_call(own(16), 8, {}, temperature=0.0, **lp)),
    ]
    run_sequence(_maker(cfg, tiny_weights, eng), steps)


# ----------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("eng", ["f32", "bf16"])
def test_b_one_shot_requests_do_not_outlive_their_call(tiny_cfg, tiny_weights, eng, use_graph):
    """plain, log-probs, plain, stats (n_alt 0 and 3), both, plain; then requests left armed in front of calls that are rejected (T beyond
    max_new; a capacity below B * T), each followed by a plain call.  A request does not change tokens, logits or K/V, so the first
    rejected call arms buffers the test keeps (large enough for the next call): they must still hold their NaN / -2 fill after the plain
    call that follows.  cfg_mix, d_logprob and d_stats are allocated mid-session."""
    cfg, o = tiny_cfg, dict(use_graph=use_graph)
    b = lambda seed: batch(cfg, (9, 5, 17, 5), seed, shared_neg=True)
    plain = lambda seed: image_call(b(seed), 8, o, temperature=1.0, seed=seed)

    kept = {}

    def armed_then_too_long(e):
        cs.apply_opts(e, o)
        e.prefill(b(27).ids, b(27).pad)
        kept["lp"] = e._request_logprobs((2, cfg.img_tokens + 2))
        kept["st"] = e._request_stats((2, cfg.img_tokens + 2), 2)
        e.decode_image_tokens(T=cfg.img_tokens + 2, temperature=0.0)

    def kept_buffers_untouched(e):
        torch.cuda.synchronize()
        assert torch.isnan(kept["lp"]).all(), "the log-prob request outlived the call that was rejected"
        for k, v in kept["st"].items():
            assert (torch.isnan(v) if v.is_floating_point() else v == -2).all(), f"the stats request outlived the call that was rejected ({k})"
        return {}

    def too_small(e):
        e.prefill(b(29).ids, b(29).pad)
        e._request_logprobs((1, 1))
        e._request_stats((1, 1), 2)
        e.decode_image_tokens(T=8, temperature=0.0)
    steps = [
        Step("plain", plain(20)),
        Step("log-probs", image_call(b(21), 8, o, temperature=1.0, seed=21, return_logprobs=True)),
        Step("plain after log-probs", plain(22)),
        Step("stats, n_alt 0", image_call(b(23), 8, o, temperature=1.0, seed=23, return_stats=True)),
        Step("stats, n_alt 3", image_call(b(24), 8, o, temperature=0.0, return_stats=3)),
        Step("log-probs and stats", image_call(b(25), 8, o, temperature=1.0, top_k=30, seed=25, return_logprobs=True, return_stats=3)),
        Step("plain after both", plain(26)),
        Step("rejected: T beyond max_new, both requests armed",
             rejected(armed_then_too_long, r"PG_ERR_CAPACITY\): T=\d+ exceeds max_new"), False),
        Step("plain after the rejected call", plain(28)),
        Step("the rejected call's buffers were never written", kept_buffers_untouched, False),
        Step("rejected: request capacity below B * T", rejected(too_small, r"PG_ERR_ARG\): token log-probs: capacity 1 floats is below"), False),
        Step("plain, greedy, logits", image_call(b(30), 8, o, temperature=0.0, return_logits=True)),
    ]
    run_sequence(_maker(cfg, tiny_weights, eng), steps)


# ----------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("eng", ["bf16", "bf16-fp8"])
def test_c_replica_geometry_is_reset_by_every_prefill(tiny_cfg, tiny_weights, eng):
    """alias = 1 replicas, a plain prefill at the same R, alias = 0, a plain prefill at a smaller R, alias = 1 with other lengths; a decode
    after each.  Steps 0 and 1 keep every graph-key field but group_rows equal (R = 8, the same shared_len)."""
    cfg = tiny_cfg
    lp = dict(return_logprobs=True)
    r4 = batch(cfg, (9, 5, 30, 5), 40, shared_neg=True)
    steps = [
        Step("replicas = 2, alias = 1", image_call(r4, 8, GRAPH, kind="replicated", replicas=2, alias=True, temperature=1.0, seed=1, **lp)),
        Step("plain prefill, R = 8, same key but group_rows", image_call(batch(cfg, (7, 5, 12, 5, 3, 5, 18, 5), 41, shared_neg=True), 8, GRAPH,
                                                                         temperature=1.0, seed=2, **lp)),
        Step("replicas = 2, alias = 0, per-sample negatives", image_call(batch(cfg, (11, 4, 6, 8), 42), 8, GRAPH, kind="replicated", replicas=2,
                                                                         alias=False, temperature=0.0, return_logits=True)),
        Step("plain prefill, R = 4", image_call(batch(cfg, (5, 6, 21, 6), 43, shared_neg=True), 10, {}, temperature=1.0, top_p=0.8, seed=3)),
        Step("replicas = 4 of R0 = 2, alias = 1, other lengths", image_call(batch(cfg, (33, 7), 44), 6, {}, kind="replicated", replicas=4, alias=True,
                                                                            temperature=1.0, seed=4, **lp)),
        Step("replicas = 2, alias = 1, longer prompts, graph", image_call(batch(cfg, (64, 9, 2, 9), 45, shared_neg=True), 8, GRAPH, kind="replicated",
                                                                          replicas=2, alias=True, temperature=0.0, **lp)),
        Step("replicas = 2, alias = 0, shared negative", image_call(r4, 8, GRAPH, kind="replicated", replicas=2, alias=False, temperature=0.0, **lp)),
        Step("plain prefill, R = 8, per-sample", image_call(batch(cfg, (3, 9, 1, 4, 22, 6, 5, 5), 46), 8, GRAPH, temperature=0.0, **lp)),
    ]
    run_sequence(_maker(cfg, tiny_weights, eng), steps)


# ----------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("eng,fused", [("f32", 1), ("bf16", 1), ("bf16-fp8", 1), ("f32", 0), ("bf16", 0)],
                         ids=["f32", "bf16", "bf16-fp8", "f32-unfused", "bf16-unfused"])
def test_d_stale_keys_past_the_new_lengths_are_never_read(tiny_cfg, tiny_weights, eng, fused):
    """Eight max_prompt-long prompts decoded for all img_tokens steps make every slot of every row (and every FP8 scale) live; the short
    ragged batch that follows must not see them.  fuse_rope = 0 (libplangen_diag.so's A/B switch) takes the un-fused decode attention,
    which the FP8 cache does not have."""
    cfg = tiny_cfg
    o = {} if fused else dict(fuse_rope=0)
    full = batch(cfg, (cs.MAX_PROMPT,) * 8, 50)
    steps = [
        Step("every slot live", image_call(full, cfg.img_tokens, o, temperature=0.0)),
        Step("short ragged prompts", image_call(batch(cfg, (1, 2, 17, 1, 2, 17, 1, 2), 51), 6, o, temperature=0.0, return_logits=True)),
        Step("every slot live, graph", image_call(full, cfg.img_tokens, {**o, **GRAPH}, temperature=1.0, seed=5), False),
        Step("short, shared negative, graph", image_call(batch(cfg, (1, 2, 17, 2), 52, shared_neg=True), 7, {**o, **GRAPH}, temperature=1.0, seed=6,
                                                         return_logprobs=True)),
    ]
    run_sequence(_maker(cfg, tiny_weights, eng, diag=not fused), steps)


# ----------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("eng", ["f32", "bf16"])
def test_e_back_to_back_prefills_and_the_one_shot_hint(tiny_cfg, tiny_weights, eng):
    """Three prefills and a decode with no host synchronisation from the first prefill to the end of the decode (chain_call: inputs staged
    on the device beforehand, the sharing answer passed in, torch's sync debug mode on "error"): the result is that of the third prefill
    alone.  pg_prefill does not wait for the stream, so the third call meets the pinned staging buffer of the first with nothing but the
    buffer's own event guard in between.  The same with pg_prefill_embeds + hidden_out in the middle.  Then the caller's
    uncond_shared hint: honoured, and consumed by a call that is rejected -- the pg_prefill that follows without a hint of its own
    (issued as a C caller would, no option sent) probes the device and must not share per-sample negatives."""
    cfg = tiny_cfg
    a, b2, c = batch(cfg, (40, 9, 12, 9), 60, shared_neg=True), batch(cfg, (3, 12, 5, 2), 61), batch(cfg, (8, 5, 27, 5), 62, L=30, shared_neg=True)
    d = batch(cfg, (6, 7, 9, 7), 63)                           # odd rows of one length and different ids: only the ids say "not shared"
    nine = batch(cfg, (4, 5) * 5, 64, shared_neg=True)          # 10 rows > max_rows
    steps = [
        Step("prefill A, B, C + decode, unsynchronised", chain_call([a, b2, c], 8, temperature=1.0, seed=1, return_logprobs=True),
             fresh=chain_call([c], 8, temperature=1.0, seed=1, return_logprobs=True)),
        Step("prefill C, prefill_embeds B with hidden_out, D + decode, unsynchronised", chain_call([c, b2, d], 8, embeds_at=1, temperature=0.0, return_logits=True),
             fresh=chain_call([d], 8, temperature=0.0, return_logits=True)),
        Step("five prefills + decode, unsynchronised", chain_call([d, a, c, b2, a], 6, temperature=0.0, return_logprobs=True),
             fresh=chain_call([a], 6, temperature=0.0, return_logprobs=True)),
        Step("prefill_embeds with hidden_out, checked", prefill_hidden(a, position_mode=1)),
        Step("embeds prefill + decode", image_call(b2, 6, {}, kind="embeds", temperature=0.0)),
        Step("hinted: shared", image_call(a, 8, {}, uncond_shared=True, on_device=True, temperature=0.0, return_logprobs=True)),
        Step("hinted: not shared", image_call(c, 8, {}, uncond_shared=False, on_device=True, temperature=0.0, return_logprobs=True)),
        Step("hinted call rejected (rows > max_rows)", rejected(prefill_only(nine, uncond_shared=True), r"PG_ERR_CAPACITY\): rows 10 > max_rows 8"), False),
        Step("un-hinted pg_prefill, per-sample negatives", image_call(d, 8, {}, kind="raw", temperature=0.0, return_logprobs=True)),
        Step("un-hinted pg_prefill, shared negative", image_call(a, 8, {}, kind="raw", temperature=0.0, return_logprobs=True)),
    ]
    run_sequence(_maker(cfg, tiny_weights, eng), steps)


# ----------------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("eng,use_graph", [("f32", 1), ("bf16", 0), ("bf16", 1)])
def test_f_mixed_modes_on_one_handle(tiny_cfg, tiny_weights, eng, use_graph):
    """Image decode, text (greedy, sampled), constrained text under the layout automaton, text again once the automaton is forgotten (the
    fresh handle never saw one), score_text, score_image, image decode again; and a decode right after each scoring call, where the
    veteran and a fresh handle given the same two calls must answer alike -- the same tokens or the same refusal."""
    from plangen_amd.grammar import layout_token_dfa
    from plangen_amd.textproc import TagWordCodec
    cfg, o = tiny_cfg, dict(use_graph=use_graph)
    dfa = layout_token_dfa(TagWordCodec(cfg.vocab, eos_id=cfg.eos_id, pad_id=cfg.pad_id), cfg.vocab)
    img = batch(cfg, (9, 5, 30, 5), 70, shared_neg=True)
    txt = lambda seed: batch(cfg, (9, 5, 7), seed)
    sc = batch(cfg, (14, 9, 20, 11), 75)
    steps = [
        Step("image decode", image_call(img, 8, o, temperature=1.0, seed=1, return_logprobs=True)),
        Step("text, greedy", text_call(txt(71), 10, o, temperature=0.0, return_logits=True)),
        Step("text, sampled", text_call(txt(72), 10, o, temperature=1.0, top_k=30, top_p=0.9, seed=2, min_new_tokens=4, return_logprobs=True)),
        Step("constrained text", text_call(txt(73), 24, o, dfa=dfa, temperature=1.5, seed=3, return_logprobs=True, return_stats=2)),
        Step("the automaton is forgotten", cs.forget_dfa, False),
        Step("text after the automaton, greedy", text_call(txt(74), 10, o, temperature=0.0, return_logprobs=True)),
        Step("text after the automaton, sampled", text_call(txt(71), 10, o, temperature=1.0, seed=4, min_new_tokens=10, return_stats=True)),
        Step("score_text", score_text_call(sc, [p + 3 for p in sc.pad], o)),
        Step("score_image", score_image_call(img, codes(cfg, 2, 10, 76), o)),
        Step("image decode again", image_call(batch(cfg, (4, 7, 12, 7), 77, shared_neg=True), 8, o, temperature=1.0, seed=1, return_logprobs=True)),
        Step("score_text, then decode", score_text_call(sc, [p + 1 for p in sc.pad], o, then_decode=6, temperature=0.7)),
        Step("score_image, then decode", score_image_call(batch(cfg, (6, 3, 11, 8), 78), codes(cfg, 2, 7, 79), o, then_decode=6)),
        Step("image decode, eager", image_call(img, 8, {}, temperature=0.0, return_logits=True)),
    ]
    run_sequence(_maker(cfg, tiny_weights, eng), steps)


# ----------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("eng", ["f32", "bf16"])
def test_g_lanes_restore_every_rebased_member(tiny_cfg, tiny_weights, eng):
    """lanes = 2 at R = 8, lanes = 1 at R = 8 and R = 4, lanes = 2 at R = 4 (two lanes of one CFG pair each), eager and graph; in between, the
    combinations decode_image refuses with lanes = 2 (aliasing replicas, log-probs, stats), each asserted, each followed by a call that
    must not notice."""
    cfg = tiny_cfg
    l1, l2 = dict(lanes=1), dict(lanes=2)
    r8 = lambda seed: batch(cfg, (9, 5, 30, 5, 2, 5, 14, 5), seed, shared_neg=True)
    r4 = lambda seed, sh=True: batch(cfg, (7, 6, 19, 6), seed, shared_neg=sh)
    steps = [
        Step("lanes = 2, R = 8", image_call(r8(80), 8, l2, temperature=1.0, seed=1, return_logits=True)),
        Step("lanes = 1, R = 8", image_call(r8(81), 8, l1, temperature=1.0, seed=2, return_logprobs=True)),
        Step("lanes = 1, R = 4", image_call(r4(82), 8, l1, temperature=0.0, return_stats=2)),
        Step("lanes = 2, R = 4", image_call(r4(83), 8, l2, temperature=1.0, top_k=40, seed=3)),
        Step("lanes = 2 refuses log-probs", rejected(image_call(r4(84), 8, l2, temperature=0.0, return_logprobs=True), r"PG_ERR_ARG\): token log-probs do not support lanes = 2"), False),
        Step("lanes = 1 after the refusal", image_call(r4(84), 8, l1, temperature=0.0, return_logprobs=True)),
        Step("lanes = 2 refuses stats", rejected(image_call(r4(85), 8, l2, temperature=0.0, return_stats=True), r"PG_ERR_ARG\): token stats do not support lanes = 2"), False),
        Step("lanes = 2 refuses aliasing replicas", rejected(image_call(r4(86), 8, l2, kind="replicated", replicas=2, alias=True, temperature=0.0),
                                                             r"PG_ERR_ARG\): replicas that alias .*alias = 1\) do not support lanes = 2"), False),
        Step("lanes = 2, R = 8, graph, per-sample", image_call(batch(cfg, (3, 9, 1, 4, 22, 6, 5, 5), 87), 8, {**l2, **GRAPH}, temperature=0.0)),
        Step("lanes = 1, R = 8, graph", image_call(r8(88), 8, {**l1, **GRAPH}, temperature=0.0, return_logprobs=True)),
        Step("lanes = 2, R = 4, graph", image_call(r4(89, False), 8, {**l2, **GRAPH}, temperature=1.0, seed=4, return_logits=True)),
        Step("lanes = 2, copied replicas", image_call(r4(90), 8, l2, kind="replicated", replicas=2, alias=False, temperature=0.0)),
        Step("default lanes, R = 4", image_call(r4(91), 8, {}, temperature=0.0, return_logprobs=True, return_stats=1)),
    ]
    run_sequence(_maker(cfg, tiny_weights, eng), steps)


def test_g_fp8_cache_refuses_two_lanes(tiny_cfg, tiny_weights):
    """The FP8 KV cache has no two-lane form: refused, and the lanes = 1 call that follows equals a fresh handle's."""
    cfg = tiny_cfg
    b = batch(cfg, (7, 6, 19, 6), 92, shared_neg=True)
    steps = [
        Step("lanes = 2 refused", rejected(image_call(b, 8, dict(lanes=2), temperature=0.0), r"PG_ERR_ARG\): the FP8 KV cache does not support lanes = 2"), False),
        Step("lanes = 1", image_call(b, 8, dict(lanes=1), temperature=1.0, seed=1, return_logprobs=True)),
    ]
    run_sequence(_maker(cfg, tiny_weights, "bf16-fp8"), steps)


# ----------------------------------------------------------------------------------------------------------------- (h)
@pytest.mark.parametrize("two_streams", [False, True], ids=["one-stream", "two-streams"])
def test_h_two_handles_interleaved(tiny_cfg, tiny_weights, two_streams):
    """An f32 and a bf16 veteran take turns, on the caller's one stream or each on a stream of its own; a round's results are fetched only
    after both of its calls were issued (the calls' own uploads of host inputs still wait for the stream they run on): each handle's
    results equal its own fresh reference."""
    cfg = tiny_cfg
    makers = [_maker(cfg, tiny_weights, "f32"), _maker(cfg, tiny_weights, "bf16")]
    sh = lambda seed, lens=(9, 5, 30, 5): batch(cfg, lens, seed, shared_neg=True)
    rounds = [
        (image_call(sh(110), 8, GRAPH, temperature=1.0, seed=1, return_logprobs=True), image_call(batch(cfg, (12, 4, 7, 9), 111), 8, {}, temperature=0.0,
                                                                                                 return_logits=True)),
        (image_call(batch(cfg, (3, 8, 8, 2, 6, 6, 1, 9), 112), 6, {}, temperature=0.0, return_stats=2), image_call(sh(113), 10, GRAPH, temperature=1.0, top_k=20,
                                                                                                                  seed=2)),
        (image_call(sh(114), 8, GRAPH, kind="replicated", replicas=2, temperature=0.0, return_logprobs=True), image_call(sh(115, (2, 7, 21, 7)), 8, dict(lanes=2),
                                                                                                                          temperature=1.0, seed=3)),
        (image_call(batch(cfg, (1, 2, 17, 1), 116), 12, GRAPH, temperature=1.0, seed=4, return_logprobs=True), image_call(sh(117), 8, GRAPH, temperature=0.0,
                                                                                                                         return_logprobs=True)),
    ]
    vets = [m() for m in makers]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()] if two_streams else [torch.cuda.current_stream()] * 2
    try:
        for i, calls in enumerate(rounds):
            torch.cuda.synchronize()
            got = []
            for e, s, call in zip(vets, streams, calls):
                with torch.cuda.stream(s):
                    got.append(call(e))
            got = [cs.to_host(g) for g in got]
            for name, g, m, call in zip(("f32", "bf16"), got, makers, calls):
                cs.assert_same(g, cs.fresh_result(m, call), f"round {i}, {name} handle")
    finally:
        torch.cuda.synchronize()
        for e in vets:
            e.close()
            cs._OPEN.remove(e)
