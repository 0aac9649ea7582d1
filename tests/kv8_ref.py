"""CPU reference of the FP8 KV cache (format: include/plangen_hip.h) and of the engine's rule for using it.

Format: every 128-element K / V row is stored as OCP e4m3fn codes and one power-of-two scale 2^e, e the smallest integer with
amax * 2^-e <= 448, clamped to [-100, 100] (amax == 0: e = 0); code = e4m3_rne(x * 2^-e).  torch's CPU ``float8_e4m3fn`` cast rounds to
nearest even and is the reference of the device's v_cvt_pk_fp8_f32.

Rule: what a forward call APPENDS to the cache is dequantize(quantize(.)) of its new K / V, while the attention of that same call uses the
new K / V unquantised -- prefill attention is exact and a decode step's own key is exact (``llama_forward_kv8``)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R

E_MIN, E_MAX, FP8_MAX = -100, 100, 448.0


def exponent(amax):
    """e per row (int32) for amax >= 0 (float32)."""
    m, ex = torch.frexp(amax)                                   # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = ex - 9 + (m > 0.875).to(ex.dtype)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    return e.clamp(E_MIN, E_MAX)


def quantize(x):
    """x [..., 128] (any float dtype; the values as they are) -> (codes uint8 [..., 128], scale float32 [...])."""
    xf = x.to(torch.float32)
    e = exponent(xf.abs().amax(-1))
    scaled = torch.ldexp(xf, -e[..., None])                     # exact: a power-of-two factor
    codes = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, torch.ldexp(torch.ones_like(xf[..., 0]), e)


def dequantize(codes, scale):
    return codes.view(torch.float8_e4m3fn).to(torch.float32) * scale[..., None].to(torch.float32)


def qdq(x):
    return dequantize(*quantize(x))


def llama_forward_kv8(W, cfg, inputs_embeds, key_mask, positions, cache=None, quant=qdq):
    """oracle.ref_cpu.llama_forward with ONE change: the cache keeps quant(new K / V); this call's attention sees them unquantised."""
    Rr, q, H = inputs_embeds.shape
    nh, d = cfg.n_heads, cfg.head_dim
    if cache is None:
        cache = R.KVCache([None] * cfg.n_layers, [None] * cfg.n_layers)
    past = cache.length()
    c = past + q
    km = key_mask[:, :c].to(torch.bool)
    qi = torch.arange(past, c)[:, None]
    kj = torch.arange(c)[None, :]
    allowed = (kj <= qi)[None] & km[:, None, :]
    allowed = allowed | (kj == qi)[None]
    bias = torch.zeros(Rr, 1, q, c).masked_fill(~allowed[:, None], float("-inf"))
    cos, sin = R.rope_cos_sin(positions, d, cfg.rope_theta)
    x = inputs_embeds.to(torch.float32)
    for i in range(cfg.n_layers):
        p = f"{R.LM}layers.{i}."
        xn = R.rms_norm(x, W[p + "input_layernorm.weight"], cfg.rms_eps)
        qh = F.linear(xn, W[p + "self_attn.q_proj.weight"]).view(Rr, q, nh, d).transpose(1, 2)
        kh = F.linear(xn, W[p + "self_attn.k_proj.weight"]).view(Rr, q, nh, d).transpose(1, 2)
        vh = F.linear(xn, W[p + "self_attn.v_proj.weight"]).view(Rr, q, nh, d).transpose(1, 2)
        qh = R.apply_rope(qh, cos, sin)
        kh = R.apply_rope(kh, cos, sin)
        kq, vq = quant(kh), quant(vh)                           # what later calls will read
        if cache.k[i] is not None:
            kh = torch.cat([cache.k[i], kh], dim=2)
            vh = torch.cat([cache.v[i], vh], dim=2)
            kq = torch.cat([cache.k[i], kq], dim=2)
            vq = torch.cat([cache.v[i], vq], dim=2)
        cache.k[i], cache.v[i] = kq, vq
        s = torch.matmul(qh, kh.transpose(2, 3)) * (d ** -0.5) + bias
        pattn = torch.softmax(s, dim=-1, dtype=torch.float32)
        o = torch.matmul(pattn, vh).transpose(1, 2).reshape(Rr, q, nh * d)
        x = x + F.linear(o, W[p + "self_attn.o_proj.weight"])
        xn = R.rms_norm(x, W[p + "post_attention_layernorm.weight"], cfg.rms_eps)
        hmid = F.silu(F.linear(xn, W[p + "mlp.gate_proj.weight"])) * F.linear(xn, W[p + "mlp.up_proj.weight"])
        x = x + F.linear(hmid, W[p + "mlp.down_proj.weight"])
    return R.rms_norm(x, W[R.LM + "norm.weight"], cfg.rms_eps), cache


def sample_image_kv8(W, cfg, inputs_embeds, mask, cfg_weight=5.0, n_tokens=None, force_tokens=None, return_logits=False, quant=qdq):
    """oracle.ref_cpu.sample_image (greedy parity mode) over llama_forward_kv8."""
    Rr = inputs_embeds.shape[0]
    B = Rr // 2
    T = cfg.img_tokens if n_tokens is None else n_tokens
    tokens = torch.zeros((B, T), dtype=torch.int32)
    all_logits = []
    cache = None
    x = inputs_embeds
    for i in range(T):
        past = 0 if cache is None else cache.length()
        q = x.shape[1]
        pos = torch.arange(past, past + q)[None].expand(Rr, q)
        hidden, cache = llama_forward_kv8(W, cfg, x, mask, pos, cache, quant)
        logits = R.gen_head(W, hidden[:, -1, :])
        mixed = logits[1::2] + cfg_weight * (logits[0::2] - logits[1::2])
        nxt = torch.argmax(mixed, dim=-1).to(torch.int32)
        if return_logits:
            all_logits.append(mixed)
        tokens[:, i] = nxt
        feed = nxt if force_tokens is None else force_tokens[:, i].to(torch.int32)
        x = R.prepare_gen_img_embeds(W, torch.stack([feed, feed], dim=1).view(-1))[:, None, :]
    return (tokens, torch.stack(all_logits)) if return_logits else tokens


def row_families(seed=0, n_random=256):
    """bf16 rows [n, 128] the quantiser tests run on: random rows with amax from 2^-20 to 2^20, an all-zero row, rows whose amax is exactly
    448 * 2^k (the edge of an exponent step) and one just above it, and rows with a wide spread inside (elements down to 2^-14 amax)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-20, 21, (n_random, 1), generator=g)
    rows = [torch.ldexp(torch.randn(n_random, 128, generator=g), k)]
    rows.append(torch.zeros(1, 128))
    for kk in (-12, -1, 0, 3, 11):
        r = torch.ldexp(torch.rand(2, 128, generator=g) * 2 - 1, torch.tensor(kk + 8))
        r[0, 5] = -448.0 * 2.0 ** kk                            # amax exactly 448 * 2^k: e = k
        r[1, 7] = 450.0 * 2.0 ** kk                             # the next bf16 above it: e = k + 1
        rows.append(r)
    spread = torch.ldexp(torch.randn(16, 128, generator=g), torch.randint(-14, 1, (16, 128), generator=g))
    rows.append(spread)
    return torch.cat(rows).to(torch.bfloat16)
