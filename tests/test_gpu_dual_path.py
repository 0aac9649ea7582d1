"""GPU: the dual-guidance decode loop through the C ABI (pg_decode_image_tokens_dual) on the tiny fixture: max_rows = 8, so B = 2 images and 6 rows.  Against
the three-row oracle loop of tests/dual_ref.py (f32: tokens equal, logits within the project's LOGIT_TOL_F32; bf16: teacher-forced, within LOGIT_TOL_BF16), the
caption rows given the full rows' ids (w_layout then multiplies an exact zero), graph replay, the one-shot requests, the FP8 cache, the refusals, and the pair
call left as it was."""
import numpy as np
import pytest
import torch

import dual_ref as U
from conftest import get_engine, load_golden
from oracle import ref_cpu as R
from plangen_amd.engine import PlanGenError
from plangen_amd.guidance import SamplePlan
from test_gpu_path import LOGIT_TOL_BF16, LOGIT_TOL_F32

pytestmark = pytest.mark.gpu
B, T = 2, 16
WC, WL = 5.0, 2.0
_S = {}


def _golden():
    g = load_golden("sample_image_tiny.npz")
    return g, torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])


def _pad(mask, L):
    return (L - mask[:, :L].sum(-1)).tolist()


def _triples(tiny_cfg, caption="other"):
    """(ids [6, L], mask [6, L + img_tokens], pad) from the golden pair batch: full = its cond rows 0 and 2, negative = its row 1, caption = other prompts of
    other lengths (its cond row 4 without its tail, its row 0 without its head), or the full rows themselves (caption="full")."""
    g, ids, mask = _golden()
    L = ids.shape[1]
    pad = _pad(mask, L)
    row = lambda r: ids[r, pad[r]:].tolist()
    full = [row(0), row(2)]
    cap = full if caption == "full" else [row(4)[:-2], row(0)[3:]]
    ids3, mask3 = U.collate_triples(full, cap, row(1), 0, tiny_cfg.img_tokens)
    return ids3, mask3, _pad(mask3, ids3.shape[1])


def _oracle(tiny_cfg, tiny_weights, ocfg):
    if "oracle" not in _S:
        ids3, mask3, _ = _triples(tiny_cfg)
        _S["oracle"] = U.sample_image_dual(tiny_weights, ocfg, R.embed_tokens(tiny_weights, ids3), mask3, WC, WL, n_tokens=T, return_logits=True)
    return _S["oracle"]


def _prefill(e, tiny_cfg, caption="other"):
    ids3, _, pad = _triples(tiny_cfg, caption)
    e.prefill(ids3, pad, position_mode=0, uncond_shared=False)


def test_f32_engine_equals_the_oracle_loop(tiny_cfg, tiny_weights, ocfg):
    ref_tok, ref_logits = _oracle(tiny_cfg, tiny_weights, ocfg)
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    _prefill(e, tiny_cfg)
    toks, logits = e.decode_image_tokens_dual(T, WC, WL, return_logits=True)
    err = (logits.cpu() - ref_logits).abs().max().item()
    print(f"dual f32: max |logit err| {err:.2e} (bound {LOGIT_TOL_F32})")
    assert toks.shape == (B, T) and logits.shape == (T, B, tiny_cfg.img_vocab)
    assert torch.equal(toks.cpu(), ref_tok) and err < LOGIT_TOL_F32
    # the weights matter on this fixture: swapped, the logits move by far more than the bound
    _prefill(e, tiny_cfg)
    swapped = e.decode_image_tokens_dual(T, WL, WC, force_tokens=ref_tok, return_logits=True)[1]
    assert (swapped.cpu() - ref_logits).abs().max() > 10 * LOGIT_TOL_F32
    # the edit region: where it is 0 the label is emitted and fed back
    gen = torch.Generator().manual_seed(5)
    gt = torch.randint(0, tiny_cfg.img_vocab, (B, T), generator=gen).int()
    region = (torch.rand(B, T, generator=gen) > 0.5).int()
    ids3, mask3, _ = _triples(tiny_cfg)
    want = U.sample_image_dual(tiny_weights, ocfg, R.embed_tokens(tiny_weights, ids3), mask3, WC, WL, n_tokens=T, edit_region=region, gt_labels=gt)
    _prefill(e, tiny_cfg)
    got = e.decode_image_tokens_dual(T, WC, WL, force_tokens=gt, force_mask=region.to(torch.uint8))
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("n", [1, 3])
def test_f32_engine_equals_the_oracle_loop_at_other_image_counts(tiny_cfg, tiny_weights, ocfg, n):
    """R = 3 (one image, on the shared engine) and R = 9 (three images, an engine of its own with max_rows = 9): odd row counts through the prefill,
    forward_decode and the loop."""
    g, ids, mask = _golden()
    pad = _pad(mask, ids.shape[1])
    row = lambda r: ids[r, pad[r]:].tolist()
    full = [row(0), row(2), row(4)][:n]
    cap = [row(4)[:-2], row(0)[3:], row(2)[:-1]][:n]
    ids3, mask3 = U.collate_triples(full, cap, row(1), 0, tiny_cfg.img_tokens)
    ref_tok, ref_logits = U.sample_image_dual(tiny_weights, ocfg, R.embed_tokens(tiny_weights, ids3), mask3, WC, WL, n_tokens=T, return_logits=True)
    if n == 1:
        e = get_engine(tiny_cfg, tiny_weights, "f32")
    else:
        from plangen_amd.engine import Engine
        e = Engine(tiny_cfg, dtype="f32", max_rows=9, max_prompt=32, max_new=tiny_cfg.img_tokens, max_images=3)
        e.load_state_dict(tiny_weights)
    try:
        e.prefill(ids3, _pad(mask3, ids3.shape[1]), position_mode=0, uncond_shared=False)
        toks, logits = e.decode_image_tokens_dual(T, WC, WL, return_logits=True)
        err = (logits.cpu() - ref_logits).abs().max().item()
        print(f"dual f32, {n} image(s): max |logit err| {err:.2e} (bound {LOGIT_TOL_F32})")
        assert toks.shape == (n, T) and torch.equal(toks.cpu(), ref_tok) and err < LOGIT_TOL_F32
    finally:
        if n != 1:
            e.close()


def test_bf16_engine_teacher_forced(tiny_cfg, tiny_weights, ocfg):
    ref_tok, ref_logits = _oracle(tiny_cfg, tiny_weights, ocfg)
    e = get_engine(tiny_cfg, tiny_weights, "bf16")
    _prefill(e, tiny_cfg)
    toks, logits = e.decode_image_tokens_dual(T, WC, WL, force_tokens=ref_tok, return_logits=True)
    err = (logits.cpu() - ref_logits).abs().max().item()
    print(f"dual bf16 teacher-forced: max |logit err| {err:.4f} (bound {LOGIT_TOL_BF16:.4f})")
    assert err < LOGIT_TOL_BF16, err
    top2 = ref_logits.topk(2, dim=-1).values
    decisive = (top2[..., 0] - top2[..., 1]) > 2 * LOGIT_TOL_BF16          # [T, B]
    assert torch.equal(toks.cpu().t()[decisive], ref_tok.t()[decisive])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_caption_rows_equal_to_full_rows_ignore_w_layout(tiny_cfg, tiny_weights, dtype):
    """f - p is an exact zero when rows 3b and 3b + 1 carry the same ids and identical rows of one launch get identical bits."""
    e = get_engine(tiny_cfg, tiny_weights, dtype)
    outs = []
    for wl in (1.0, 9.0):
        _prefill(e, tiny_cfg, "full")
        outs.append(e.decode_image_tokens_dual(T, WC, wl, return_logits=True))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_graph_replay_equals_eager_and_follows_new_weights(tiny_cfg, tiny_weights):
    """Every call writes the SAME token and tap buffers through the raw entry point, so the graph key (which holds the tap's address) is the same in all of
    them: the first graphed call captures the step, the second (other weights) and the third (the first weights again) replay that capture.  Their tokens and
    tapped logits equal the eager calls' bit for bit -- weights baked into the captured arguments would give the second call the first call's logits."""
    weights = ((WC, WL), (1.5, 7.0), (WC, WL))
    for dtype in ("f32", "bf16"):
        e = get_engine(tiny_cfg, tiny_weights, dtype)
        out = torch.zeros((B, T), dtype=torch.int32, device=e.device)
        lg = torch.zeros((T, B, tiny_cfg.img_vocab), dtype=torch.float32, device=e.device)
        res = {}
        for use_graph in (1, 0):
            e.set_option("use_graph", use_graph)
            for i, (wc, wl) in enumerate(weights):
                _prefill(e, tiny_cfg)
                out.fill_(-1); lg.fill_(float("nan"))
                e._check(e.lib.pg_decode_image_tokens_dual(e.h, T, wc, wl, 0.0, 0, 1.0, 0, None, None, out.data_ptr(), lg.data_ptr(), e.stream), "dual")
                torch.cuda.synchronize()
                res[(use_graph, i)] = (out.cpu().clone(), lg.cpu().clone())
        e.set_option("use_graph", 0)
        for i in range(3):
            assert torch.equal(res[(1, i)][0], res[(0, i)][0]) and torch.equal(res[(1, i)][1], res[(0, i)][1]), (dtype, i)
        assert torch.equal(res[(1, 2)][1], res[(1, 0)][1]) and not torch.equal(res[(1, 1)][1], res[(1, 0)][1]), dtype
        # and without a tap (address 0 in the key): the tokens of the replayed calls are the eager calls'
        for use_graph in (1, 0):
            e.set_option("use_graph", use_graph)
            for i, (wc, wl) in enumerate(weights):
                _prefill(e, tiny_cfg)
                assert torch.equal(e.decode_image_tokens_dual(T, wc, wl).cpu(), res[(0, i)][0]), (dtype, use_graph, i)
        e.set_option("use_graph", 0)
    # seeded sampling repeats, another seed does not
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    draws = []
    for seed in (11, 11, 12):
        _prefill(e, tiny_cfg)
        draws.append(e.decode_image_tokens_dual(T, WC, WL, temperature=1.0, seed=seed, top_k=50, top_p=0.9).cpu())
    assert torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], draws[2])


def test_requests_are_honoured_and_one_shot(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    for kw in (dict(temperature=0.0), dict(temperature=0.8, seed=3), dict(temperature=0.8, seed=3, top_k=9, top_p=0.8)):
        _prefill(e, tiny_cfg)
        toks, logits, lp, st = e.decode_image_tokens_dual(T, WC, WL, return_logits=True, return_logprobs=True, return_stats=2, **kw)
        want = e.token_logprob(logits.transpose(0, 1).reshape(B * T, -1), toks.reshape(-1), kw["temperature"]).view(B, T)
        assert torch.equal(lp, want), kw
        assert torch.equal(st["logprob"], lp) and bool(torch.isfinite(st["entropy"]).all()) and bool((st["rank"] >= 0).all())
        assert st["alt_tok"].shape == (B, T, 2) and bool((st["alt_tok"] >= 0).all())
        _prefill(e, tiny_cfg)
        plain = e.decode_image_tokens_dual(T, WC, WL, **kw)
        assert torch.equal(plain, toks)                                    # the requests change no token
    lp2 = e._request_logprobs((B, T))
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):                  # a refused call consumes the request
        e.decode_image_tokens_dual(T, WC, WL, top_p=0.0)
    _prefill(e, tiny_cfg)
    e.decode_image_tokens_dual(T, WC, WL)
    torch.cuda.synchronize()
    assert bool(torch.isnan(lp2).all())


def test_fp8_cache_runs_and_agrees_where_bf16_is_decisive(tiny_cfg, tiny_weights):
    eb, e8 = get_engine(tiny_cfg, tiny_weights, "bf16"), get_engine(tiny_cfg, tiny_weights, "bf16", kv_dtype="fp8")
    _prefill(eb, tiny_cfg)
    tb, lb = eb.decode_image_tokens_dual(T, WC, WL, return_logits=True)
    _prefill(e8, tiny_cfg)
    t8 = e8.decode_image_tokens_dual(T, WC, WL, force_tokens=tb)
    top2 = lb.cpu().topk(2, dim=-1).values
    decisive = (top2[..., 0] - top2[..., 1]) > 2 * LOGIT_TOL_BF16
    assert torch.equal(t8.cpu().t()[decisive], tb.cpu().t()[decisive])


def _guarded_call(e, **kw):
    """decode_image_tokens_dual through the raw entry point on guarded outputs: (PlanGenError or None, outputs untouched)."""
    out = torch.full((B + 2, T), -99, dtype=torch.int32, device=e.device)
    lg = torch.full((T + 2, B, e.cfg.img_vocab), 77.0, dtype=torch.float32, device=e.device)
    a = dict(T=T, wc=WC, wl=WL, temperature=0.0, top_k=0, top_p=1.0)
    a.update(kw)
    rc = e.lib.pg_decode_image_tokens_dual(e.h, a["T"], a["wc"], a["wl"], a["temperature"], a["top_k"], a["top_p"], 0, None, None, out[1].data_ptr(),
                                           lg[1].data_ptr(), e.stream)
    torch.cuda.synchronize()
    return rc, e.lib.pg_last_error(e.h).decode(), bool((out == -99).all()) and bool((lg == 77.0).all())


def test_refusals_launch_nothing_and_leave_the_handle_usable(tiny_cfg, tiny_weights):
    g, ids, mask = _golden()
    pad = _pad(mask, ids.shape[1])
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    e.prefill(ids, pad, position_mode=0)
    before = e.decode_image_tokens(T, cfg_weight=5.0, temperature=0.0).cpu()
    ARG, STATE = -1, -3
    # R % 3 != 0: two pairs
    e.prefill(ids[:4], pad[:4], position_mode=0, uncond_shared=False)
    rc, msg, clean = _guarded_call(e)
    assert rc == ARG and "three" in msg and clean
    # a shared negative prompt: six rows whose odd rows carry one prompt
    six = torch.cat([ids[:2]] * 3)
    e.prefill(six, pad[:2] * 3, position_mode=0)
    rc, msg, clean = _guarded_call(e)
    assert rc == STATE and "uncond_shared=False" in msg and "uncond_shared_hint" in msg and clean
    # replicated prompts
    e.prefill_replicated(ids[:2], pad[:2], 3, alias=True, uncond_shared=False)
    rc, msg, clean = _guarded_call(e)
    assert rc == STATE and "replicas" in msg and clean
    # lanes = 2
    _prefill(e, tiny_cfg)
    e.set_option("lanes", 2)
    rc, msg, clean = _guarded_call(e)
    e.set_option("lanes", -1)
    assert rc == ARG and "lanes" in msg and clean
    # a pending sample plan: consumed and refused; the next call runs without it
    e._request_sample_plan(SamplePlan(temperature=[1.0] * B), T)
    rc, msg, clean = _guarded_call(e)
    assert rc == ARG and "plan" in msg and clean
    rc, msg, clean = _guarded_call(e)
    assert rc == 0 and not clean
    # ranges, and a call before a fresh prefill
    rc, msg, clean = _guarded_call(e)
    assert rc == STATE and "fresh prefill" in msg and clean
    _prefill(e, tiny_cfg)
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(wc=float("nan")), dict(wl=float("inf"))):
        rc, msg, clean = _guarded_call(e, **kw)
        assert rc == ARG and clean, kw
    rc, msg, clean = _guarded_call(e, T=tiny_cfg.img_tokens + 2)
    assert rc == -5 and clean
    # the handle is usable: the dual call runs, and the pair call gives the tokens it gave before
    ref = e.decode_image_tokens_dual(T, WC, WL).cpu()
    _prefill(e, tiny_cfg)
    assert torch.equal(e.decode_image_tokens_dual(T, WC, WL).cpu(), ref)
    e.prefill(ids, pad, position_mode=0)
    assert torch.equal(e.decode_image_tokens(T, cfg_weight=5.0, temperature=0.0).cpu(), before)


def test_filtering_refused_beyond_the_selects_vocabulary(tiny_cfg):
    """An engine of its own with img_vocab = 16 640 > SEL_MAXV = 16 384 (synthetic weights, one triple): a filtered call is refused with PG_ERR_CAPACITY, its
    message names the limit, nothing is written; greedy and unfiltered sampled calls (and a greedy call that carries filter values, which greedy ignores)
    run on the same handle before and after."""
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    V = 16640
    cfg = PlanGenConfig(**dict(tiny_cfg.model_dict(), img_vocab=V))
    e = Engine(cfg, dtype="f32", max_rows=3, max_prompt=16, max_new=T, max_images=1)
    try:
        e.init_synthetic(seed=3)
        g = torch.Generator().manual_seed(41)
        ids = torch.randint(8, cfg.vocab, (3, 6), generator=g).int()
        pf = lambda: e.prefill(ids, [0, 2, 3], position_mode=0, uncond_shared=False)

        def call(**kw):
            out = torch.full((1 + 2, T), -99, dtype=torch.int32, device=e.device)
            lg = torch.full((T + 2, 1, V), 77.0, dtype=torch.float32, device=e.device)
            a = dict(temperature=0.0, top_k=0, top_p=1.0)
            a.update(kw)
            rc = e.lib.pg_decode_image_tokens_dual(e.h, T, WC, WL, a["temperature"], a["top_k"], a["top_p"], 5, None, None, out[1].data_ptr(), lg[1].data_ptr(),
                                                   e.stream)
            torch.cuda.synchronize()
            clean = bool((out == -99).all()) and bool((lg == 77.0).all())
            guards = bool((out[0] == -99).all()) and bool((out[2] == -99).all()) and bool((lg[0] == 77.0).all()) and bool((lg[-1] == 77.0).all())
            return rc, e.lib.pg_last_error(e.h).decode(), clean, guards, out[1].cpu()

        pf()
        rc, msg, clean, guards, greedy = call()
        assert rc == 0 and guards and not clean and bool(((greedy >= 0) & (greedy < V)).all())
        pf()
        for kw in (dict(temperature=1.0, top_k=5), dict(temperature=1.0, top_p=0.9), dict(temperature=0.7, top_k=50, top_p=0.5)):
            rc, msg, clean, guards, _ = call(**kw)
            assert rc == -5 and "16384" in msg and str(V) in msg and "top-k / top-p" in msg and clean, (kw, rc, msg)
        # nothing was launched: the prefill is still fresh and the handle runs what the select kernel is not needed for
        rc, msg, clean, guards, again = call(top_k=5, top_p=0.9)           # greedy ignores the filter values
        assert rc == 0 and guards and torch.equal(again, greedy)
        pf()
        rc, msg, clean, guards, sampled = call(temperature=1.0)
        assert rc == 0 and guards and not clean and bool(((sampled >= 0) & (sampled < V)).all())
    finally:
        e.close()


def test_pair_call_unchanged_after_dual_calls(tiny_cfg, tiny_weights):
    g, ids, mask = _golden()
    for dtype in ("f32", "bf16"):
        e = get_engine(tiny_cfg, tiny_weights, dtype)
        for use_graph in (1, 0):
            e.set_option("use_graph", use_graph)
            _prefill(e, tiny_cfg)
            e.decode_image_tokens_dual(T, WC, WL, temperature=1.0, top_k=9)
            e.prefill(ids, _pad(mask, ids.shape[1]), position_mode=0)
            toks = e.decode_image_tokens(cfg_weight=5.0, temperature=0.0)
            if dtype == "f32":
                assert np.array_equal(toks.cpu().numpy(), g["tokens"]), use_graph
            else:
                _S.setdefault("pair_bf16", toks.cpu())
                assert torch.equal(toks.cpu(), _S["pair_bf16"])
        e.set_option("use_graph", 0)


def test_graph_alternation_between_the_pair_and_dual_loops(tiny_cfg, tiny_weights):
    """One f32 handle, use_graph on, T = 4 (a graph needs T > 2), the six rows of _triples read as three pairs or two triples: pair, dual, pair, dual,
    each after its own prefill, each with its own seed, all four through the raw entry points into the SAME token and tap buffers.  Both loops keep their
    step graph in one slot under one key, and with these calls every field of that key but the rows per image is equal (R = 6, the tap's address, no shared
    prompt, unfiltered), so a key that did not tell pairs from triples would replay the other loop's step.  Tokens and tapped logits of each call equal,
    bit for bit, the same call alone on a fresh handle."""
    import call_sequences as cs
    T4, V = 4, tiny_cfg.img_vocab
    ids3, _, pad3 = _triples(tiny_cfg)

    def call(e, bufs, form, seed):
        out, lg = bufs
        nb = 3 if form == "pair" else 2
        e.set_option("use_graph", 1)
        e.prefill(ids3, pad3, position_mode=0, uncond_shared=False)
        out.fill_(-1); lg.fill_(float("nan"))
        if form == "pair":
            rc = e.lib.pg_decode_image_tokens(e.h, T4, WC, 1.0, seed, None, None, out.data_ptr(), lg.data_ptr(), e.stream)
        else:
            rc = e.lib.pg_decode_image_tokens_dual(e.h, T4, WC, WL, 1.0, 0, 1.0, seed, None, None, out.data_ptr(), lg.data_ptr(), e.stream)
        e._check(rc, form)
        torch.cuda.synchronize()
        return out[:nb * T4].cpu().clone(), lg[:T4 * nb * V].cpu().clone()

    def bufs(e):
        return torch.zeros(3 * T4, dtype=torch.int32, device=e.device), torch.zeros(T4 * 3 * V, dtype=torch.float32, device=e.device)

    calls = (("pair", 21), ("dual", 22), ("pair", 23), ("dual", 24))
    try:
        vet = cs.make_engine(tiny_cfg, tiny_weights, "f32")
        vb = bufs(vet)
        got = [call(vet, vb, form, seed) for form, seed in calls]
        for (form, seed), (tok, lg) in zip(calls, got):
            fresh = cs.make_engine(tiny_cfg, tiny_weights, "f32")
            ftok, flg = call(fresh, bufs(fresh), form, seed)
            fresh.close(); cs._OPEN.remove(fresh)
            assert bool((tok >= 0).all()) and bool(torch.isfinite(lg).all()), (form, seed)
            assert torch.equal(tok, ftok) and torch.equal(lg.view(torch.int32), flg.view(torch.int32)), (form, seed)
    finally:
        cs.close_all()
