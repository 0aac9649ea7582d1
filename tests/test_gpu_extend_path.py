"""GPU: pg_prefill_extend / pg_rewind through the C ABI at the tiny config.

* PG_F32: prefill(P) + extend(gen_embed(golden tokens[:k])) + a greedy decode of T - k tokens gives tokens k .. T - 1 of sample_image_tiny.
* Anchored bound: on the same embeddings E_step = |hidden of S x pg_step - one-shot prefill_embeds(P + S)| is what the parent's own way of
  growing a cache costs; |extend - one-shot| <= K_MAX (1.25, tests/bf16ref.py: two roundings of one computation) x E_step, max and mean.
* Rewind, text continuation, split extensions, every refusal, and "no call depends on the calls before it" against a second handle."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16ref
from conftest import load_golden
from plangen_amd.engine import Engine, PlanGenError

pytestmark = pytest.mark.gpu

MAX_PROMPT, MAX_NEW, MAX_ROWS = 96, 80, 8
_ENG = {}


def _engine(tiny_cfg, tiny_weights, dtype, which="a", kv_dtype="bf16"):
    """Handles of this file's own (max_new 80: S = 70 single steps must fit).  "a" is the veteran every test reuses, "b" the handle that
    has not seen the calls under test."""
    key = (dtype, which, kv_dtype)
    if key not in _ENG:
        e = Engine(tiny_cfg, dtype=dtype, max_rows=MAX_ROWS, max_prompt=MAX_PROMPT, max_new=MAX_NEW, max_images=4, with_lm_head=True, kv_dtype=kv_dtype)
        e.load_state_dict({k: v for k, v in tiny_weights.items()
                           if not k.startswith(("vision_model.", "aligner.", "gen_vision_model.encoder", "gen_vision_model.quant_conv"))})
        _ENG[key] = e
    return _ENG[key]


def _golden():
    g = load_golden("sample_image_tiny.npz")
    ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
    L = ids.shape[1]
    return g, ids, (L - mask[:, :L].sum(-1)).tolist()


def _pair_embeds(e, tok):
    """prepare_gen_img_embeds(tok [B, k]) for both rows of every CFG pair: [2B, k, hidden]."""
    B, k = tok.shape
    return e.gen_embed(tok.repeat_interleave(2, 0)).view(2 * B, k, -1)


def _kv(e, cfg, lens):
    """Every layer's K and V slots below the rows' lengths."""
    slots = MAX_PROMPT + MAX_NEW
    out = []
    dt = torch.float32 if e.dtype == "f32" else torch.bfloat16
    for layer in range(cfg.n_layers):
        for name in ("kcache", "vcache"):
            buf = e.debug_read(name, layer, MAX_ROWS * cfg.n_heads * slots * 128, dt).view(MAX_ROWS, cfg.n_heads, slots, 128).cpu()
            out += [buf[r, :, :n].clone() for r, n in enumerate(lens)]
    return out


def _code(fn):
    with pytest.raises(PlanGenError) as ei:
        fn()
    return str(ei.value)


@pytest.mark.parametrize("k", [1, 17, 40])
def test_f32_extend_then_decode_equals_golden_tokens(tiny_cfg, tiny_weights, k):
    g, ids, pad = _golden()
    gold = torch.from_numpy(g["tokens"]).to(torch.int32)
    T = gold.shape[1]
    e = _engine(tiny_cfg, tiny_weights, "f32")
    e.prefill(ids, pad, uncond_shared=False)
    assert e.cached_len() == [ids.shape[1] - p for p in pad]
    e.extend(embeds=_pair_embeds(e, gold[:, :k].to(e.device)))
    assert e.cached_len() == [ids.shape[1] - p + k for p in pad]
    toks = e.decode_image_tokens(T=T - k, cfg_weight=5.0, temperature=0.0)
    assert np.array_equal(toks.cpu().numpy(), g["tokens"][:, k:])
    assert e.cached_len() == [ids.shape[1] - p + T - 1 for p in pad]          # the last emitted token was never fed back


def _grow_three_ways(e, X, pad, Lp, S, pmode, n_new):
    """Hidden states of the S new tokens: one-shot prefill of everything, S single steps, one extension (ragged by n_new)."""
    one = e.prefill_embeds(X, pad, position_mode=pmode, return_hidden=True)[:, Lp:].clone()
    e.prefill_embeds(X[:, :Lp], pad, position_mode=pmode)
    step = torch.stack([e.step(X[:, Lp + i]) for i in range(S)], dim=1)
    e.prefill_embeds(X[:, :Lp], pad, position_mode=pmode)
    ext = e.extend(embeds=X[:, Lp:], n_new=n_new, return_hidden=True)
    return one.float().cpu(), step.float().cpu(), ext.float().cpu()


def _anchored(tag, ext, step, one, valid):
    e_step, e_ext = (step - one).abs()[valid], (ext - one).abs()[valid]
    ratio = lambda x, y: float(x / y) if float(y) > 0 else (0.0 if float(x) == 0 else float("inf"))      # a zero anchor admits a zero error only
    rmax, rmean = ratio(e_ext.max(), e_step.max()), ratio(e_ext.mean(), e_step.mean())
    print(f"{tag}: E_step max {float(e_step.max()):.3g} mean {float(e_step.mean()):.3g}; extend / E_step: max {rmax:.3f} mean {rmean:.3f}")
    assert e_ext.max() <= bf16ref.K_MAX * e_step.max(), f"{tag}: max error {rmax:.3f} x E_step"
    assert e_ext.mean() <= bf16ref.K_MAX * e_step.mean(), f"{tag}: mean error {rmean:.3f} x E_step"


@pytest.mark.parametrize("pmode", [0, 1])
@pytest.mark.parametrize("S", [1, 5, 70])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_extend_hidden_within_the_step_loops_own_error(tiny_cfg, tiny_weights, dtype, S, pmode):
    e = _engine(tiny_cfg, tiny_weights, dtype)
    R, Lp = 4, 24
    gen = torch.Generator().manual_seed(100 + S + pmode)
    X = e.embed_tokens(torch.randint(8, tiny_cfg.vocab, (R, Lp + S), generator=gen))
    pad = [0, 5, 11, 23]                                                      # left padding: rows of 24, 19, 13 and 1 prompt tokens
    n_new = [S, max(1, S - 2), max(1, S // 2), 1]                             # ragged
    one, step, ext = _grow_three_ways(e, X, pad, Lp, S, pmode, n_new)
    valid = torch.zeros(R, S, dtype=torch.bool)
    for r, n in enumerate(n_new):
        valid[r, :n] = True
    assert float(ext[~valid].abs().max() if (~valid).any() else 0.0) == 0.0    # unused columns are zero
    _anchored(f"{dtype} S={S} pmode={pmode}", ext, step, one, valid)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rewind_then_extend_equals_a_handle_that_never_extended(tiny_cfg, tiny_weights, dtype):
    g, ids, pad = _golden()
    gen = torch.Generator().manual_seed(7)
    a, b = _engine(tiny_cfg, tiny_weights, dtype, "a"), _engine(tiny_cfg, tiny_weights, dtype, "b")
    R = ids.shape[0]
    A_ = torch.randint(0, tiny_cfg.img_vocab, (R // 2, 9), generator=gen, dtype=torch.int32)
    B_ = torch.randint(0, tiny_cfg.img_vocab, (R // 2, 6), generator=gen, dtype=torch.int32)
    n_b = [6, 6, 3, 3] + [6] * (R - 4)
    plen = [ids.shape[1] - p for p in pad]
    a.prefill(ids, pad, uncond_shared=False)
    a.extend(embeds=_pair_embeds(a, A_.to(a.device)))
    a.rewind(plen)
    assert a.cached_len() == plen
    ha = a.extend(embeds=_pair_embeds(a, B_.to(a.device)), n_new=n_b, return_hidden=True).cpu()
    b.prefill(ids, pad, uncond_shared=False)
    hb = b.extend(embeds=_pair_embeds(b, B_.to(b.device)), n_new=n_b, return_hidden=True).cpu()
    assert torch.equal(ha, hb)
    lens = [p + n for p, n in zip(plen, n_b)]
    assert a.cached_len() == lens == b.cached_len()
    for x, y in zip(_kv(a, tiny_cfg, lens), _kv(b, tiny_cfg, lens)):
        assert torch.equal(x, y)
    ta = a.decode_image_tokens(T=5, cfg_weight=5.0, temperature=0.0).cpu()
    tb = b.decode_image_tokens(T=5, cfg_weight=5.0, temperature=0.0).cpu()
    assert torch.equal(ta, tb)


def test_f32_second_question_after_rewind_equals_a_fresh_prefill(tiny_cfg, tiny_weights):
    """prefill, greedy text, rewind to the prompt, extend(question 2), greedy text == a fresh handle prefilled with [prompt | question 2]."""
    gen = torch.Generator().manual_seed(31)
    a, b = _engine(tiny_cfg, tiny_weights, "f32", "a"), _engine(tiny_cfg, tiny_weights, "f32", "b")
    R, L, nq = 3, 20, 6
    pad = [0, 4, 13]
    ids = torch.randint(8, tiny_cfg.vocab, (R, L), generator=gen, dtype=torch.int32)
    q2 = torch.randint(8, tiny_cfg.vocab, (R, nq), generator=gen, dtype=torch.int32)
    n_q = [6, 4, 5]
    a.prefill(ids, pad, position_mode=1)
    first = a.generate_text(12, tiny_cfg.eos_id)
    assert first.shape[1] >= 1
    a.rewind([L - p for p in pad])
    a.extend(ids=q2, n_new=n_q)
    got = a.generate_text(10, tiny_cfg.eos_id).cpu()
    Lf = L + nq
    full = torch.full((R, Lf), tiny_cfg.pad_id, dtype=torch.int32)
    pad_f = []
    for r in range(R):
        row = torch.cat([ids[r, pad[r]:], q2[r, :n_q[r]]])
        full[r, Lf - len(row):] = row
        pad_f.append(Lf - len(row))
    b.prefill(full, pad_f, position_mode=1)
    want = b.generate_text(10, tiny_cfg.eos_id).cpu()
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_split_extension(tiny_cfg, tiny_weights, dtype):
    """extend(S) against extend(S1) then extend(S2): under the anchored bound; PG_F32 greedy tokens afterwards are equal."""
    g, ids, pad = _golden()
    e = _engine(tiny_cfg, tiny_weights, dtype)
    R, S, S1 = ids.shape[0], 12, 5
    tok = torch.from_numpy(g["tokens"]).to(torch.int32)[:, :S].to(e.device)
    X = _pair_embeds(e, tok)
    e.prefill(ids, pad, uncond_shared=False)
    step = torch.stack([e.step(X[:, i]) for i in range(S)], dim=1).float().cpu()
    e.prefill(ids, pad, uncond_shared=False)
    whole = e.extend(embeds=X, return_hidden=True).float().cpu()
    t_whole = e.decode_image_tokens(T=8, cfg_weight=5.0, temperature=0.0).cpu()
    e.prefill(ids, pad, uncond_shared=False)
    h1 = e.extend(embeds=X[:, :S1].contiguous(), return_hidden=True)
    h2 = e.extend(embeds=X[:, S1:].contiguous(), return_hidden=True)
    split = torch.cat([h1, h2], dim=1).float().cpu()
    t_split = e.decode_image_tokens(T=8, cfg_weight=5.0, temperature=0.0).cpu()
    # the anchor: the parent's own two ways of computing these hidden states differ by E = |steps - whole|
    _anchored(f"{dtype} split {S1}+{S - S1}", split, step, whole, torch.ones(R, S, dtype=torch.bool))
    if dtype == "f32":
        assert torch.equal(t_whole, t_split)


def test_refusals_launch_nothing_and_leave_the_handle_usable(tiny_cfg, tiny_weights):
    g, ids, pad = _golden()
    R, L = ids.shape
    plen = [L - p for p in pad]
    b = _engine(tiny_cfg, tiny_weights, "bf16", "b")
    b.prefill(ids, pad, uncond_shared=False)
    want = b.decode_image_tokens(T=6, cfg_weight=5.0, temperature=0.0).cpu()
    want_kv = _kv(b, tiny_cfg, plen)

    def usable(e):
        """after a refusal: a normal prefill + decode gives the other handle's bits"""
        e.prefill(ids, pad, uncond_shared=False)
        got = e.decode_image_tokens(T=6, cfg_weight=5.0, temperature=0.0).cpu()
        assert torch.equal(got, want)
        for x, y in zip(_kv(e, tiny_cfg, plen), want_kv):
            assert torch.equal(x, y)

    # before a prefill (a handle of its own: "never prefilled" cannot be restored)
    n = Engine(tiny_cfg, dtype="bf16", max_rows=MAX_ROWS, max_prompt=MAX_PROMPT, max_new=MAX_NEW, max_images=4, with_lm_head=True)
    n.load_state_dict({k: v for k, v in tiny_weights.items()
                       if not k.startswith(("vision_model.", "aligner.", "gen_vision_model.encoder", "gen_vision_model.quant_conv"))})
    n.R = R
    x1 = torch.zeros(R, 2, tiny_cfg.hidden, device=n.device)
    assert "PG_ERR_STATE" in _code(lambda: n.extend(embeds=x1))
    assert "PG_ERR_STATE" in _code(lambda: n.rewind([1] * R))
    usable(n)
    n.close()

    a = _engine(tiny_cfg, tiny_weights, "bf16", "a")
    x = torch.zeros(R, 4, tiny_cfg.hidden, device=a.device)
    # replicated prompts
    a.prefill_replicated(ids[:2], pad[:2], 2, uncond_shared=False)
    assert "PG_ERR_STATE" in _code(lambda: a.extend(embeds=x[:4]))
    assert "PG_ERR_STATE" in _code(lambda: a.rewind([1] * 4))
    usable(a)
    # shared negative prompt: the message names the way out
    a.prefill(ids, pad, uncond_shared=True)
    msg = _code(lambda: a.extend(embeds=x))
    assert "PG_ERR_STATE" in msg and "uncond_shared_hint" in msg
    assert "PG_ERR_STATE" in _code(lambda: a.rewind(plen))
    usable(a)
    # arguments
    a.prefill(ids, pad, uncond_shared=False)
    i32 = torch.zeros(R, 4, dtype=torch.int32, device=a.device)
    for bad in ([0] + [4] * (R - 1), [5] + [4] * (R - 1)):
        assert "PG_ERR_ARG" in _code(lambda: a.extend(embeds=x, n_new=bad))
    nn = (C.c_int32 * R)(*[4] * R)
    call = lambda i, m, dt, hd=0: a.lib.pg_prefill_extend(a.h, i, m, dt, nn, 4, None, hd, a.stream)
    assert call(i32.data_ptr(), x.data_ptr(), 0) == -1                       # both inputs
    assert call(None, None, 0) == -1                                          # neither
    assert call(None, x.data_ptr(), 2) == -1                                  # PG_I32 embeddings
    assert "PG_ERR_ARG" in _code(lambda: a.rewind([0] + plen[1:]))
    assert "PG_ERR_ARG" in _code(lambda: a.rewind([plen[0] + 1] + plen[1:]))
    usable(a)
    # a pending span request is consumed and refused; the next extension goes through
    lo = torch.zeros(R, 1, dtype=torch.int32); hi = torch.ones(R, 1, dtype=torch.int32)
    mass = a._request_attn_spans((lo, hi, 0, 1, None), R)
    assert "PG_ERR_ARG" in _code(lambda: a.extend(embeds=x))
    a.extend(embeds=x)
    assert bool(torch.isnan(mass).all())
    usable(a)
    # a bare rewind leaves no hidden state to sample from: both loops refuse until an extension follows (pg_step brings its own input)
    a.prefill(ids, pad, uncond_shared=False)
    a.rewind(plen)
    assert "PG_ERR_STATE" in _code(lambda: a.decode_image_tokens(T=4, cfg_weight=5.0, temperature=0.0))
    assert "PG_ERR_STATE" in _code(lambda: a.generate_text(4, tiny_cfg.eos_id))
    usable(a)
    # capacity: the KV slots ...
    slots = MAX_PROMPT + MAX_NEW
    big = torch.zeros(R, slots, tiny_cfg.hidden, device=a.device)
    a.prefill(ids, pad, uncond_shared=False)
    assert "PG_ERR_CAPACITY" in _code(lambda: a.extend(embeds=big, n_new=[slots - plen[0] + 1] + [1] * (R - 1)))
    # ... the RoPE table (2 * max_prompt + max_new + 64 positions; position_mode 0 counts the 245 pad columns) ...
    wide = torch.randint(8, tiny_cfg.vocab, (MAX_ROWS, 250), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    big8 = torch.zeros(MAX_ROWS, 100, tiny_cfg.hidden, device=a.device)
    a.prefill(wide, [245] * MAX_ROWS, uncond_shared=False)
    msg = _code(lambda: a.extend(embeds=big8, n_new=[90] * MAX_ROWS))
    assert "PG_ERR_CAPACITY" in msg and "RoPE" in msg
    # ... and the packed tokens (max_rows * max_prompt = 768 < 8 x 100)
    a.prefill(wide, [245] * MAX_ROWS, position_mode=1)
    msg = _code(lambda: a.extend(embeds=big8))
    assert "PG_ERR_CAPACITY" in msg and "packed" in msg
    usable(a)
    # the decode entry points after an extension: rows longer than max_prompt must not leave the KV slots ...
    a.prefill(ids, pad, uncond_shared=False)
    a.extend(embeds=big[:, :slots - 20].contiguous(), n_new=[slots - 20 - plen[0]] + [1] * (R - 1))      # row 0 holds slots - 20 tokens
    msg = _code(lambda: a.decode_image_tokens(T=22, cfg_weight=5.0, temperature=0.0))
    assert "PG_ERR_CAPACITY" in msg and "KV slots" in msg
    a.decode_image_tokens(T=21, cfg_weight=5.0, temperature=0.0)                                 # 20 appended slots: fits
    assert "PG_ERR_CAPACITY" in _code(lambda: a.step(torch.zeros(R, tiny_cfg.hidden, device=a.device)))
    a.prefill(ids, pad, position_mode=1)
    a.extend(embeds=big[:, :slots - 20].contiguous(), n_new=[slots - 20 - plen[0]] + [1] * (R - 1))
    msg = _code(lambda: a.generate_text(22, tiny_cfg.eos_id))
    assert "PG_ERR_CAPACITY" in msg and "KV slots" in msg
    usable(a)
    # ... nor the RoPE table: 245 pad columns + 5 prompt + 86 new tokens end at position 336 of 336, so no further step has a position
    a.prefill(wide, [245] * MAX_ROWS, uncond_shared=False)
    a.extend(embeds=big8[:, :86].contiguous())
    msg = _code(lambda: a.decode_image_tokens(T=2, cfg_weight=5.0, temperature=0.0))
    assert "PG_ERR_CAPACITY" in msg and "RoPE" in msg
    assert "RoPE" in _code(lambda: a.step(torch.zeros(MAX_ROWS, tiny_cfg.hidden, device=a.device)))
    a.decode_image_tokens(T=1, cfg_weight=5.0, temperature=0.0)                                  # one draw, nothing fed back: allowed
    a.prefill(wide, [245] * MAX_ROWS, uncond_shared=False)
    a.extend(embeds=big8[:, :80].contiguous())                                                   # ends at 330: T - 1 = 6 more positions
    assert "RoPE" in _code(lambda: a.decode_image_tokens(T=8, cfg_weight=5.0, temperature=0.0))
    a.decode_image_tokens(T=7, cfg_weight=5.0, temperature=0.0)
    usable(a)
    # an FP8 handle
    f = _engine(tiny_cfg, tiny_weights, "bf16", "a", kv_dtype="fp8")
    f.prefill(ids, pad, uncond_shared=False)
    assert "PG_ERR_ARG" in _code(lambda: f.extend(embeds=x))
    assert "PG_ERR_ARG" in _code(lambda: f.rewind(plen))
    f.prefill(ids, pad, uncond_shared=False)          # the FP8 handle stays usable: twice the same bits (its cache differs from b's by design)
    t1 = f.decode_image_tokens(T=6, cfg_weight=5.0, temperature=0.0).cpu()
    assert "PG_ERR_ARG" in _code(lambda: f.extend(embeds=x))
    f.prefill(ids, pad, uncond_shared=False)
    assert torch.equal(f.decode_image_tokens(T=6, cfg_weight=5.0, temperature=0.0).cpu(), t1)
    # ... and a plain prefill after extend / rewind owes nothing to them
    a.prefill(ids, pad, uncond_shared=False)
    a.extend(embeds=x)
    a.rewind(plen)
    usable(a)
