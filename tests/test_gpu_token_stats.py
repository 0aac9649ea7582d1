"""GPU: per-token uncertainty (pg_request_token_stats, pg_op_token_stats) against the fp64 reference of stats_ref.py.  rank and alt_tok are
exact; logprob is bit-equal to pg_op_token_logprob / pg_request_token_logprobs; alt_logprob within logprob_ref's bound and entropy within
stats_ref.ent_tol(V) (both derived there).  The loops are checked on their own tapped logits and emitted tokens, and a call with the
request must return the tokens and logits of the call without it bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import get_engine, load_golden
import logprob_ref as LR
import stats_ref as SR
from plangen_amd._lib import pg_token_stats
from test_gpu_sampling_filters import _prompt
from test_gpu_text_sampling import _prefill
from text_dfa_ref import RandomDFA

pytestmark = pytest.mark.gpu

PAD, F_CANARY, I_CANARY = 16, 1234.5, -77
KEYS = ("logprob", "entropy", "rank", "alt_tok", "alt_logprob")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _assert_stats(got, ref, V, what, keys=KEYS):
    got = {k: np.asarray(v) for k, v in got.items()}
    n_alt = got["alt_tok"].shape[-1] if "alt_tok" in got else 0
    ref = dict(ref, alt_tok=ref["alt_tok"][..., :n_alt], alt_logprob=ref["alt_logprob"][..., :n_alt])     # the first n_alt of the 8 best
    print(f"{what}: max |H - H64| = {SR.max_entropy_error(got['entropy'], ref['entropy']):.3e} (bound {SR.ent_tol(V):.3e}), "
          f"max |alt_lp - alt_lp64| = {LR.max_excess(got.get('alt_logprob', []), ref['alt_logprob'] if n_alt else []):.3e}")
    bad = SR.mismatches(got, ref, V, keys)
    assert not bad, (what, bad, {k: (got[k], ref[k]) for k in bad if ":" not in k})


# ----------------------------------------------------------------------------------------------------------------- operator
def _raw_op(e, y, tok, temp, n_alt, off, lp_too=True):
    """pg_op_token_stats on rows that start ``off`` floats past a 16-byte boundary, every output between canaries; also
    pg_op_token_logprob on the very same rows (same addresses: the order of the sum depends on a row's alignment)."""
    B, V = y.shape
    buf = torch.zeros(B * V + 8, dtype=torch.float32, device=e.device)
    assert buf.data_ptr() % 16 == 0
    x = buf[off:off + B * V]
    x.copy_(torch.from_numpy(y).reshape(-1))
    t = torch.from_numpy(tok).to(e.device)
    n = max(n_alt, 1)
    f = lambda k: torch.full((PAD + B * k + PAD,), F_CANARY, dtype=torch.float32, device=e.device)
    i = lambda k: torch.full((PAD + B * k + PAD,), I_CANARY, dtype=torch.int32, device=e.device)
    arr = dict(logprob=f(1), entropy=f(1), rank=i(1), alt_tok=i(n), alt_logprob=f(n))
    ptr = {k: v.data_ptr() + PAD * 4 for k, v in arr.items()}
    req = pg_token_stats(ptr["logprob"], ptr["entropy"], ptr["rank"], ptr["alt_tok"] if n_alt else None, ptr["alt_logprob"] if n_alt else None, n_alt, B)
    e._check(e.lib.pg_op_token_stats(e.h, x.data_ptr(), B, V, e._p(t), C.c_float(temp), C.byref(req), e.stream), "pg_op_token_stats")
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=e.device)
    if lp_too:
        e._check(e.lib.pg_op_token_logprob(e.h, x.data_ptr(), B, V, e._p(t), C.c_float(temp), e._p(lp), e.stream), "pg_op_token_logprob")
    torch.cuda.synchronize()
    out = {}
    for k, v in arr.items():
        v = v.cpu()
        width = (n_alt if k.startswith("alt") else 1) * B
        canary = F_CANARY if v.dtype == torch.float32 else I_CANARY
        assert (v[:PAD] == canary).all() and (v[PAD + width:] == canary).all(), f"{k}: canary overwritten"
        if k.startswith("alt"):
            if n_alt:
                out[k] = v[PAD:PAD + width].view(B, n_alt).numpy()
        else:
            out[k] = v[PAD:PAD + B].numpy()
    return out, lp.cpu().numpy(), (x, t)


@pytest.mark.parametrize("V", [1, 3, 5, 1023, 1024, 1025, 4099, 16384, 102400])
def test_operator_against_fp64(tiny_cfg, tiny_weights, V):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    B = 3
    for name, (y, tok) in SR.families(V, B, 1000 + V).items():
        for temp in (0.0, 0.7):
            ref = SR.token_stats_ref(y, tok, temp, 8)                        # once per (family, temperature): n_alt < 8 is its prefix
            for n_alt, off in ((0, 0), (1, 1), (8, 0), (8, 1), (8, 2), (8, 3)):
                got, lp, (x, t) = _raw_op(e, y, tok, temp, n_alt, off)
                what = f"V={V} {name} T={temp} n_alt={n_alt} off={off}"
                _assert_stats(got, ref, V, what)
                assert np.array_equal(got["logprob"].view(np.int32), lp.view(np.int32)), what       # the bits of pg_op_token_logprob
                if n_alt:
                    # alt_logprob[0] is what pg_op_token_logprob gives the best token (a row without one: alt_tok -1, both -inf)
                    top = torch.from_numpy(got["alt_tok"][:, 0].copy()).to(e.device)
                    lp0 = torch.full((B,), float("nan"), dtype=torch.float32, device=e.device)
                    e._check(e.lib.pg_op_token_logprob(e.h, x.data_ptr(), B, V, e._p(top), C.c_float(temp), e._p(lp0), e.stream), "pg_op_token_logprob")
                    assert np.array_equal(got["alt_logprob"][:, 0].view(np.int32), lp0.cpu().numpy().view(np.int32)), what
            if name == "flat":
                assert (got["rank"] == 0).all() and got["alt_tok"][0].tolist() == list(range(min(8, V))) + [-1] * (8 - min(8, V))
            if name in ("empty", "tok_on_neginf", "tok_outside"):
                assert (got["rank"] == V).all() and np.isneginf(got["logprob"]).all()
            if name == "empty":
                assert (got["entropy"] == 0).all() and (got["alt_tok"] == -1).all() and np.isneginf(got["alt_logprob"]).all()


def test_engine_wrapper_and_row_independence(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    for V in (1025, 4099):
        y, tok = SR.families(V, 3, 77)["normal"]
        d = _np(e.token_stats(torch.from_numpy(y), torch.from_numpy(tok), 0.7, n_alt=8))
        _assert_stats(d, SR.token_stats_ref(y, tok, 0.7, 8), V, f"wrapper V={V}")
        assert np.array_equal(d["logprob"], e.token_logprob(torch.from_numpy(y), torch.from_numpy(tok), 0.7).cpu().numpy())
        assert set(e.token_stats(torch.from_numpy(y), torch.from_numpy(tok))) == {"logprob", "entropy", "rank"}
        # the same row alone and as slot 2 of 3, at the same address alignment (the head / vector / tail split follows the address): same bits
        three, _, _ = _raw_op(e, y, tok, 0.7, 8, 0, lp_too=False)
        one, _, _ = _raw_op(e, y[2:3], tok[2:3], 0.7, 8, (2 * V) % 4, lp_too=False)
        for k in KEYS:
            assert np.array_equal(three[k][2:3].view(np.int32), one[k].view(np.int32)), (V, k)


# ----------------------------------------------------------------------------------------------------------------- image loop
T_IMG, N_ALT = 8, 8


def _image_modes(cfg, B):
    g = torch.Generator().manual_seed(3)
    force = torch.randint(0, cfg.img_vocab, (B, T_IMG), generator=g, dtype=torch.int32)
    return {"greedy": dict(temperature=0.0), "sampled": dict(temperature=1.0, seed=5),
            "filtered": dict(temperature=1.0, seed=5, top_k=9, top_p=0.8),
            "teacher_forced": dict(temperature=1.0, seed=5, force_tokens=force, force_mask=torch.zeros(B, T_IMG, dtype=torch.uint8))}


@pytest.mark.parametrize("mode", ["greedy", "sampled", "filtered", "teacher_forced"])
def test_image_loop(tiny_cfg, tiny_weights, mode):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 3, 191)
    kw = _image_modes(tiny_cfg, 3)[mode]
    e.prefill(ids, pad)
    plain = e.decode_image_tokens(T=T_IMG, cfg_weight=5.0, return_logits=True, **kw)
    e.prefill(ids, pad)
    toks, lg, lp, st = e.decode_image_tokens(T=T_IMG, cfg_weight=5.0, return_logits=True, return_logprobs=True, return_stats=N_ALT, **kw)
    e.prefill(ids, pad)
    toks1, st1 = e.decode_image_tokens(T=T_IMG, cfg_weight=5.0, return_stats=True, **kw)      # the stats request alone, n_alt = 0
    torch.cuda.synchronize()
    assert torch.equal(plain[0], toks) and torch.equal(plain[1], lg) and torch.equal(toks1, toks)    # the request changes nothing else
    st, st1 = _np(st), _np(st1)
    assert st["entropy"].shape == (3, T_IMG) and st["alt_tok"].shape == (3, T_IMG, N_ALT) and set(st1) == {"logprob", "entropy", "rank"}
    ref = SR.image_stats_ref(lg.cpu().numpy(), toks.cpu().numpy(), kw["temperature"], N_ALT)
    _assert_stats(st, ref, tiny_cfg.img_vocab, mode)
    assert np.array_equal(st["logprob"].view(np.int32), lp.cpu().numpy().view(np.int32))      # both requests pending: the same bits
    for k in ("logprob", "entropy", "rank"):
        assert np.array_equal(st1[k].view(np.int32), st[k].view(np.int32)), k               # and n_alt does not move them
    if mode == "greedy":
        assert (st["rank"] == 0).all() and np.array_equal(st["alt_tok"][..., 0], toks.cpu().numpy())
    if mode == "teacher_forced":
        assert torch.equal(toks.cpu(), kw["force_tokens"]) and (st["rank"] > 0).any()


# ----------------------------------------------------------------------------------------------------------------- text loop
def _text_case(e, g, gen, n, kw, eos, what, V):
    _prefill(e, g)
    plain = [t.cpu() for t in gen(n, return_logits=True, **kw)]
    _prefill(e, g)
    scored = gen(n, return_logits=True, return_logprobs=True, return_stats=N_ALT, **kw)
    torch.cuda.synchronize()
    st, lp = _np(scored[-1]), scored[-2].cpu()
    for a, b in zip(plain, scored):
        assert torch.equal(a, b.cpu()), what
    toks, lg = scored[0].cpu(), scored[1].cpu()
    assert st["entropy"].shape == tuple(toks.shape) and st["alt_tok"].shape == tuple(toks.shape) + (N_ALT,)
    ref = SR.text_stats_ref(lg.numpy(), toks.numpy(), eos, kw["temperature"], N_ALT)
    _assert_stats(st, ref, V, what)
    assert np.array_equal(st["logprob"].view(np.int32), lp.numpy().view(np.int32))
    return toks, lg, st


@pytest.mark.parametrize("name,kw", [("greedy", dict(temperature=0.0)), ("sampled", dict(temperature=1.2, seed=4)),
                                     ("filtered", dict(temperature=1.2, seed=4, top_k=30, top_p=0.9))])
def test_text_loop(tiny_cfg, tiny_weights, name, kw):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    eos, n = int(g["eos"]), 8
    toks, lg, st = _text_case(e, g, lambda n_, **k: e.generate_text(n_, eos, **k), n, kw, eos, name, tiny_cfg.vocab)
    if name == "greedy":                                                     # row 1 emits EOS at once: finished from step 1 on
        assert toks.shape[0] == 3 and toks[1, 0] == eos and toks.shape[1] > 1
        assert (st["logprob"][1, 1:] == 0).all() and (st["entropy"][1, 1:] == 0).all() and (st["rank"][1, 1:] == 0).all()
        assert (st["alt_tok"][1, 1:] == -1).all() and (st["alt_logprob"][1, 1:] == 0).all()
        assert st["entropy"][1, 0] > 0 and st["rank"][1, 0] == 0 and st["alt_tok"][1, 0, 0] == eos


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=1.2, seed=8)], ids=["greedy", "sampled"])
def test_text_loop_constrained(tiny_cfg, tiny_weights, kw):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    eos, n = int(g["eos"]), 8
    e.set_text_dfa(RandomDFA(tiny_cfg.vocab, ns=5, nc=7, seed=11))
    toks, lg, st = _text_case(e, g, lambda n_, **k: e.generate_text_constrained(n_, eos, **k), n, kw, eos, f"constrained {kw}", tiny_cfg.vocab)
    masked = torch.isneginf(lg).permute(1, 0, 2).numpy()                     # [B, n, V]: what the automaton (and nothing else) removed
    assert masked.any()
    alt = st["alt_tok"]
    b, t, k = np.nonzero(alt >= 0)
    assert len(b) and not masked[b, t, alt[b, t, k]].any()                   # a masked entry is never an alternative


def test_text_columns_past_out_len_stay_untouched(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    g = load_golden("generate_tiny.npz")
    eos, n = int(g["eos"]), 8
    _prefill(e, g, rows=[1, 1, 1])                                           # three copies of the row that emits EOS at once
    d, req = e._stats_buffers((3, n), 2)
    for v in d.values():
        v.fill_(-55)
    e._check(e.lib.pg_request_token_stats(e.h, C.byref(req)), "pg_request_token_stats")
    out = e.generate_text(n, eos, temperature=0.0)
    torch.cuda.synchronize()
    w = out.shape[1]
    assert w < n and (out.cpu()[:, 0] == eos).all()
    for k, v in d.items():
        v = v.cpu()
        assert (v[:, w:] == -55).all(), k
        assert (v[:, :w] != -55).all(), k


# ----------------------------------------------------------------------------------------------------------------- request semantics
def test_request_semantics(tiny_cfg, tiny_weights):
    from plangen_amd.engine import PlanGenError
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 193)
    B, T, SENT = 2, T_IMG, -55

    def fresh(n_alt=2):
        d, req = e._stats_buffers((B, T), n_alt)
        for v in d.values():
            v.fill_(SENT)
        return d, req

    def untouched(d):
        torch.cuda.synchronize()
        return all(bool((v == SENT).all()) for v in d.values())

    request = lambda req: e.lib.pg_request_token_stats(e.h, C.byref(req))
    e.prefill(ids, pad)
    ref = e.decode_image_tokens(T=T, temperature=0.0).cpu()
    # a failing call consumes the request too
    e.prefill(ids, pad)
    d, req = fresh()
    assert request(req) == 0
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.decode_image_tokens(T=T, temperature=1.0, top_k=-1)
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(d)
    # one-shot: the call after the consuming one writes nothing
    e.prefill(ids, pad)
    assert request(req) == 0
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref)
    torch.cuda.synchronize()
    assert all(bool((v != SENT).all()) for v in d.values())
    for v in d.values():
        v.fill_(SENT)
    e.prefill(ids, pad)
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(d)
    # NULL cancels
    e.prefill(ids, pad)
    assert request(req) == 0 and e.lib.pg_request_token_stats(e.h, None) == 0
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(d)
    # refused at once: n_alt outside 0..8, capacity < 1, one alt pointer without the other, nothing asked for
    P = {k: e._p(v) for k, v in d.items()}
    for bad in (pg_token_stats(P["logprob"], P["entropy"], P["rank"], P["alt_tok"], P["alt_logprob"], 9, B * T),
                pg_token_stats(P["logprob"], P["entropy"], P["rank"], P["alt_tok"], P["alt_logprob"], -1, B * T),
                pg_token_stats(P["logprob"], P["entropy"], P["rank"], P["alt_tok"], P["alt_logprob"], 2, 0),
                pg_token_stats(P["logprob"], P["entropy"], P["rank"], P["alt_tok"], None, 2, B * T),
                pg_token_stats(P["logprob"], P["entropy"], P["rank"], None, P["alt_logprob"], 2, B * T),
                pg_token_stats(None, None, None, None, None, 0, B * T)):
        assert request(bad) == -1
        assert e.lib.pg_op_token_stats(e.h, e._p(torch.zeros(B * T, 4, device=e.device)), B * T, 4,
                                       e._p(torch.zeros(B * T, dtype=torch.int32, device=e.device)), C.c_float(0.0), C.byref(bad), e.stream) == -1
    e.prefill(ids, pad)
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(d)      # nothing is pending after a refusal
    # refused at the consuming call: capacity below B * T; lanes = 2.  Nothing launched, the handle and the prefill stay usable
    e.prefill(ids, pad)
    small = pg_token_stats(P["logprob"], P["entropy"], P["rank"], P["alt_tok"], P["alt_logprob"], 2, B * T - 1)
    assert request(small) == 0
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        e.decode_image_tokens(T=T, temperature=0.0)
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref) and untouched(d)
    e.set_option("lanes", 2)
    try:
        e.prefill(ids, pad)
        assert request(req) == 0
        with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
            e.decode_image_tokens(T=T, temperature=0.0)
    finally:
        e.set_option("lanes", 1)
    assert untouched(d)
    # a partial request (entropy alone) writes only that
    e.prefill(ids, pad)
    assert request(pg_token_stats(None, P["entropy"], None, None, None, 0, B * T)) == 0
    assert torch.equal(e.decode_image_tokens(T=T, temperature=0.0).cpu(), ref)
    torch.cuda.synchronize()
    assert bool((d["entropy"] != SENT).all()) and all(bool((d[k] == SENT).all()) for k in d if k != "entropy")
    assert e.lib.pg_device_bytes(e.h) > 0


def test_graph_with_and_without_the_request(tiny_cfg, tiny_weights):
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    ids, pad, _ = _prompt(tiny_cfg, 2, 194)
    kw = dict(T=T_IMG, cfg_weight=5.0, temperature=1.0, seed=7)
    e.prefill(ids, pad)
    eager, st_eager = e.decode_image_tokens(return_stats=N_ALT, **kw)
    e.set_option("use_graph", 1)
    try:
        e.prefill(ids, pad)
        plain = e.decode_image_tokens(**kw)
        e.prefill(ids, pad)
        toks, st = e.decode_image_tokens(return_stats=N_ALT, **kw)           # re-captured: the step holds the reducer now
        e.prefill(ids, pad)
        again = e.decode_image_tokens(**kw)                                  # and back
        torch.cuda.synchronize()
    finally:
        e.set_option("use_graph", 0)
    assert torch.equal(plain, eager) and torch.equal(toks, eager) and torch.equal(again, eager)
    for k in st:
        assert torch.equal(st[k], st_eager[k]), k


# ----------------------------------------------------------------------------------------------------------------- System
def test_system_uni_writes_image_token_stats(tmp_path, tiny_cfg, tiny_weights):
    from plangen_amd import textproc as TP
    from plangen_amd.system import System, pad_input_ids
    e = get_engine(tiny_cfg, tiny_weights, "f32")
    codec = TP.TagWordCodec(tiny_cfg.vocab, eos_id=tiny_cfg.eos_id, pad_id=tiny_cfg.pad_id)
    caps, grs = ["a red cat", "two dogs on a field"], ["<grounding><ref>cat</ref><box>[1,2,300,400]</box></grounding>", "<grounding></grounding>"]
    outs = {}
    for key in (False, True):
        s = System(tiny_cfg, e, codec=codec)
        s.args.temperature, s.args.seed = 1.0, 3
        if key:
            s.args.token_stats = True
        ids, m = pad_input_ids([s.wrap_uni_prompt(c, g)[1].tolist() for c, g in zip(caps, grs)], tiny_cfg.pad_id)
        batch = dict(base_caption=caps, gt_grounding=grs, uni_inputs_ids=ids,
                     uni_attention_mask=torch.cat([m, torch.ones((2, tiny_cfg.img_tokens), dtype=m.dtype)], -1))
        path = str(tmp_path / f"k{int(key)}")
        outs[key] = s.uni_generate(batch, pred_layout=False, gen_path=path, batch_idx="0", save_local=True)
        rec = json.load(open(os.path.join(path, "0_layout.json")))
        if not key:
            assert "image_token_stats" not in rec and "image_token_stats" not in outs[key] and not os.path.exists(os.path.join(path, "0_entropy.npy"))
            continue
        its = rec["image_token_stats"]
        assert set(its) == {"mean_entropy", "mean_rank", "rank0_share"} and all(len(v) == 2 for v in its.values())
        ent = np.load(os.path.join(path, "0_entropy.npy"))
        assert ent.shape == (2, tiny_cfg.grid, tiny_cfg.grid) and ent.dtype == np.float32 and (ent >= -1e-4).all()
        assert np.allclose(ent.reshape(2, -1).mean(1), its["mean_entropy"], atol=1e-5)
        assert all(0 <= v <= 1 for v in its["rank0_share"])
    assert torch.equal(outs[False]["pr_tokens"], outs[True]["pr_tokens"])     # the key changes nothing that was there
