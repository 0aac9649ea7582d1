"""Host models of weight loading for tests/test_gpu_load_ops.py, tests/test_gpu_load_path.py and tests/test_load_ref_cpu.py: what pg_load_tensor and
pg_finalize_weights leave in device memory, and what the row movers of every prefill / step / score call do.  Plain torch on the CPU; nothing imports the package.

Almost everything here is EXACT, so the comparator is bit equality (``same_bits``; a NaN is compared with isnan because the hardware bf16 conversion may change a
NaN's payload):

* conversion        fp32 -> bf16 rounds to nearest even (``f32_to_bf16_bits``, integer arithmetic on the bit pattern; torch's own conversion is the second,
                    independent model and the CPU test holds them against each other), bf16 -> fp32 appends 16 zero bits, same type = a copy.
* layouts           (llm_kernels.hip, gemm.hip; K_* = pg_engine's SlotKind)
    K_T / K_F32     row-major as in the checkpoint, converted to the compute type / fp32.
    K_CONV          checkpoint [Cout][Cin][kh][kw] -> [Cout][tap = kh kw][Cin]: dst (co kk + tap) Cin + ci = src (co Cin + ci) kk + tap.
    K_IL16_G / _U   gate row r -> row (r / 8) 16 + r % 8, up row r -> row (r / 8) 16 + 8 + r % 8 of ONE [2 I][H] buffer.
    wqkv            q | k | v as thirds of [3 HD][H].
    tiled           tile_weights_kernel: 16-byte vector v of the copy = W[n][k .. k + 8) with lane = v % 64, i = (v / 64) % 4, tile = v / 256,
                    chunk = tile % (K / 128), ntile = tile / (K / 128), n = 16 ntile + lane % 16, k = 128 chunk + 32 i + 8 (lane / 16).
    wqkv_p          interleave_qk_kernel: row 16 t + p of a q or k head = row 8 t + p (p < 8) or 64 + 8 t + (p - 8) of that head; v rows stay.
* row movers        gather / scatter by an index vector; embed_gather clamps ids to [0, vocab - 1].

Three derived tables carry a tolerance, each derived from the arithmetic, none fitted to a run (u = 2^-24):

* gen_table = W2 gelu(W0 e + b0) + b2, two fp32 GEMMs.  The first is within ``vq_ref.gemm_bound`` (act = 1) = e1 of its fp64 value; the second sees that
  error through |W2| and adds its own gemm_bound: |e1| |W2|^T + gemm_bound(ref, bracket + |e1| |W2|^T, K = H).
* pq_table = Wpq normalize(c) + bpq.  The normalised row is within ``vision_ref.l2_bound`` = e0; e0 |Wpq|^T + gemm_bound(...); the bf16 handle rounds the fp32
  result once more: + 2^-8 (|ref| + bound).
* RoPE tables.  inv = 1.0f / powf(theta, 2j / 128) and f = (float)p * inv on the host: the exponent 2j / 128 is exact in fp32; powf is documented at 1 ulp
  (relative 2 u), the division and the product are correctly rounded (u each): the phase f is within 4 u phi (1 + 3 u) of phi = p theta^(-2j/128).  cos and sin
  have slope <= 1, so the table moves by at most that, and cosf / sinf are documented at 1 ulp of a result <= 1: 2 u.  ``ROPE_PHASE_ULPS`` u phi +
  ``ROPE_FN_ULPS`` u, with a factor 1 + 2^-20 for the second-order terms."""
from __future__ import annotations

import math

import torch

import vision_ref as VI
import vq_ref as V

F64 = torch.float64
BF = torch.bfloat16
U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
SK_BK = 128                                                 # gemm_skinny.h
K_T, K_F32, K_IL16_G, K_IL16_U, K_CONV, K_DERIVED = 0, 1, 2, 3, 4, 100
SENTINEL = {"bf16": 0x7FA5, "f32": 0x7FA5A5A5}             # NaN payloads no converter produces (tests/prefill_ref.py uses the same)
INT32_MAX = 2 ** 31 - 1
ROPE_PHASE_ULPS, ROPE_FN_ULPS = 4, 2                        # see the module docstring


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------------ bits
def bits(t):
    """The raw bit pattern of a bf16 (-> int16) or fp32 (-> int32) tensor."""
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def from_bits(b, kind):
    """int64 bit patterns -> bf16 / fp32 tensor."""
    if kind == "bf16":
        return ((b & 0xFFFF) - ((b & 0x8000) << 1)).to(torch.int16).view(BF)
    return ((b & 0xFFFFFFFF) - ((b & 0x80000000) << 1)).to(torch.int32).view(torch.float32)


def f32_to_bf16_bits(x):
    """Round to nearest even on the bit pattern (int64 [..] of 16-bit patterns); a NaN gives the quiet NaN 0x7FC0 | sign."""
    u = bits(x.float()).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, (u >> 16) | 0x40, r)


def kind_of(t):
    return "bf16" if t.dtype == BF else "f32"


def tdtype(kind):
    return BF if kind == "bf16" else torch.float32


def convert_ref(src, dst_kind):
    """What every converter stores for a source value: torch's conversion (round to nearest even); ``f32_to_bf16_bits`` is the independent statement of it."""
    return src.to(tdtype(dst_kind))


def sentinel_like(shape, kind, device="cpu"):
    return torch.full(tuple(shape), SENTINEL[kind], dtype=torch.int32 if kind == "f32" else torch.int16, device=device).view(tdtype(kind))


def is_sentinel(t):
    return bits(t) == (SENTINEL[kind_of(t)] if kind_of(t) == "f32" else SENTINEL["bf16"])


def same_bits(got, want):
    """The bit-for-bit comparator: dict(ok, n_bad, first).  Where ``want`` is a NaN ``got`` must be a NaN (any payload); everywhere else the bits are equal.
    A sentinel left in ``got`` is a NaN where a number was expected, so an element that was never written fails."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return dict(ok=False, n_bad=-1, first=("shape / type", tuple(got.shape), got.dtype, tuple(want.shape), want.dtype))
    got, want = got.cpu(), want.cpu()
    wn = torch.isnan(want)
    bad = torch.where(wn, ~torch.isnan(got), bits(got) != bits(want))
    n_bad = int(bad.sum())
    first = None
    if n_bad:
        i = int(bad.reshape(-1).nonzero()[0])
        first = (i, hex(int(bits(got).reshape(-1)[i]) & 0xFFFFFFFF), hex(int(bits(want).reshape(-1)[i]) & 0xFFFFFFFF))
    return dict(ok=n_bad == 0, n_bad=n_bad, first=first)


# ------------------------------------------------------------------------------------------------------------------------------ values
# fp32 bit patterns every convert case carries: +-0, +-inf, the largest finite fp32 (rounds to bf16 inf), the largest fp32 that stays finite in bf16 and the
# smallest that does not (0x7F7F8000, a tie that rounds to even = up to inf), fp32 denormals (smallest, a tie to even down, a tie to even up, the largest: rounds
# up to the smallest normal), ties to even on both sides in both directions with their neighbours one fp32 ulp away, and one NaN (last).
EDGE_F32 = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0xFF7F8000, 0x00000001, 0x80000001, 0x00008000,
            0x00018000, 0x80018000, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF,
            0x3F818001, 0xBF807FFF, 0xBF808001, 0x3F7FFFFF, 0x7FC00001]
# the bf16 source's: +-0, +-inf, the largest finite, denormals, the smallest normal, plain values, one NaN (last)
EDGE_BF16 = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x3F80, 0xBF81, 0x4049, 0x7FC1]


def edge_block(kind):
    return from_bits(torch.tensor(EDGE_BF16 if kind == "bf16" else EDGE_F32, dtype=torch.int64), kind)


def values(n, kind, seed):
    """n values of the source type from a seed: normal values over ~12 binades -- fp32 ones with all 24 significand bits in use, so the rounding to bf16 is
    exercised everywhere -- with the edge block at the front (as much of it as fits) and, when there is room, once more at the end."""
    g = _gen(seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 7, (n,), generator=g).float())
    x = x.to(tdtype(kind))
    e = edge_block(kind)
    m = min(n, e.numel())
    x[:m] = e[:m]
    if n >= e.numel():                                     # spread a second copy through the tensor: the tail and the far side of a grid wrap see the edges too
        x[n - e.numel():] = e
    return x


# ------------------------------------------------------------------------------------------------------------------------------ layouts
def conv_ref(w, dst_kind):
    """K_CONV: checkpoint [Cout, Cin, kh, kw] (or [Cout, Cin, kk]) -> [Cout, kk, Cin]."""
    co, ci = w.shape[:2]
    return convert_ref(w.reshape(co, ci, -1).permute(0, 2, 1).contiguous(), dst_kind)


def il16_rows(I, which):
    """Destination row of source row r of the gate (which = 0) or up (1) matrix."""
    r = torch.arange(I)
    return (r // 8) * 16 + which * 8 + r % 8


def il16_ref(gate, up, dst_kind, fill=None):
    """K_IL16: one [2 I, H] buffer.  gate / up may be None (that half keeps ``fill``, a tensor of the buffer's shape)."""
    src = gate if gate is not None else up
    I, H = src.shape
    out = torch.zeros(2 * I, H, dtype=tdtype(dst_kind)) if fill is None else fill.clone()
    if gate is not None:
        out[il16_rows(I, 0)] = convert_ref(gate, dst_kind)
    if up is not None:
        out[il16_rows(I, 1)] = convert_ref(up, dst_kind)
    return out


def qkv_ref(q, k, v, dst_kind):
    return convert_ref(torch.cat([q, k, v]), dst_kind)


def tile_index(N, K):
    """idx [N K / 8] of 8-element vectors: vector v of the tiled copy = vector idx[v] of the row-major matrix (tile_weights_kernel)."""
    assert N % 16 == 0 and K % SK_BK == 0
    v = torch.arange(N * K // 8)
    lane, i, t = v % 64, (v // 64) % 4, v // 256
    nch = K // SK_BK
    chunk, ntile = t % nch, t // nch
    n = ntile * 16 + lane % 16
    k = chunk * SK_BK + i * 32 + (lane // 16) * 8
    return (n * K + k) // 8


def tile_ref(W):
    N, K = W.shape
    return W.reshape(-1, 8)[tile_index(N, K)].reshape(-1)


def can_tile(N, K):
    return N % 16 == 0 and K % SK_BK == 0                   # pg_engine::tile_one


def interleave_qk_index(nh):
    """idx [3 nh 128]: row n of the copy = row idx[n] of wqkv (interleave_qk_kernel)."""
    n = torch.arange(3 * nh * 128)
    HD = nh * 128
    sec, hc = n // HD, n % HD
    head, c = hc // 128, hc % 128
    t, p = c // 16, c % 16
    so = torch.where(p < 8, 8 * t + p, 64 + 8 * t + p - 8)
    so = torch.where(sec < 2, so, c)
    return sec * HD + head * 128 + so


def interleave_qk_ref(W, nh):
    return W[interleave_qk_index(nh)]


def can_fuse(max_rows, max_prompt, HD):
    """pg_engine::finalize: the handle's capacity reaches the fused prefill epilogue (>= 200 tiles of 256 x 256)."""
    return -(-(max_rows * max_prompt) // 256) * -(-(3 * HD) // 256) >= 200


# ------------------------------------------------------------------------------------------------------------------------------ slots of a state dict
def expected_kind(name, shape):
    """SlotKind of a state-dict name of the reference model (pg_engine::create / build_vq / build_vision)."""
    if name.endswith(("mlp.gate_proj.weight", "mlp.up_proj.weight")):
        return K_IL16_G if "gate_proj" in name else K_IL16_U
    if name.startswith("language_model."):
        return K_F32 if name.endswith("embed_tokens.weight") else K_T
    if name.startswith("gen_head."):
        return K_F32 if name.endswith(".bias") else K_T
    if name.startswith(("gen_embed.", "gen_aligner.", "gen_vision_model.quantize.", "gen_vision_model.post_quant_conv.")) or name.endswith(".bias"):
        return K_F32
    if name.endswith(("pos_embed", "gen_vision_model.encoder.conv_in.weight")) or ".norm" in name:
        return K_F32
    if name.startswith("gen_vision_model.") and len(shape) == 4 and shape[2] * shape[3] > 1:
        return K_CONV
    return K_T


def slot_ref(W, name, engine_kind):
    """The device buffer pg_diag_read_weight returns for a state-dict name after W was loaded into an engine of ``engine_kind``: (tensor, SlotKind)."""
    t = W[name]
    k = expected_kind(name, tuple(t.shape))
    if k == K_F32:
        return convert_ref(t, "f32").reshape(-1), k
    if k == K_CONV:
        return conv_ref(t, engine_kind).reshape(-1), k
    if k in (K_IL16_G, K_IL16_U):
        g = name.replace("up_proj", "gate_proj")
        return il16_ref(W[g], W[g.replace("gate_proj", "up_proj")], engine_kind).reshape(-1), k
    return convert_ref(t, engine_kind).reshape(-1), k


def layer_matrices(W, cfg, i):
    """bf16 row-major (wqkv, wo, wgu, wd) of layer i as the engine holds them."""
    p = f"language_model.model.layers.{i}."
    wqkv = qkv_ref(W[p + "self_attn.q_proj.weight"], W[p + "self_attn.k_proj.weight"], W[p + "self_attn.v_proj.weight"], "bf16")
    wgu = il16_ref(W[p + "mlp.gate_proj.weight"], W[p + "mlp.up_proj.weight"], "bf16")
    return dict(wqkv=wqkv, wo=convert_ref(W[p + "self_attn.o_proj.weight"], "bf16"), wgu=wgu, wd=convert_ref(W[p + "mlp.down_proj.weight"], "bf16"))


def derived_refs(W, cfg, with_lm_head=True):
    """name -> bf16 [.] of every decode-tiled copy pg_finalize_weights builds on a bf16 handle (None: tile_one skips the shape)."""
    out = {}
    for i in range(cfg.n_layers):
        for k, m in layer_matrices(W, cfg, i).items():
            out[f"layers.{i}.{k}_t"] = tile_ref(m) if can_tile(*m.shape) else None
    heads = [("gh_w1_t", "gen_head.output_mlp_projector.weight"), ("gh_w2_t", "gen_head.vision_head.weight")]
    if with_lm_head:
        heads.append(("lm_head_t", "language_model.lm_head.weight"))
    for k, nm in heads:
        m = convert_ref(W[nm], "bf16")
        out[k] = tile_ref(m) if can_tile(*m.shape) else None
    return out


# ------------------------------------------------------------------------------------------------------------------------------ row movers
def clamp_ids(ids, vocab):
    return ids.to(torch.int64).clamp(0, vocab - 1)


def embed_gather_ref(table, ids, src_idx, vocab=None):
    """dst[t] = table[clamp(ids[src_idx[t]] or ids[t], 0, vocab - 1)]."""
    vocab = table.shape[0] if vocab is None else vocab
    sel = ids if src_idx is None else ids[src_idx.long()]
    return table[clamp_ids(sel, vocab)]


def copy_rows_ref(src, src_idx, dst, dst_idx, n):
    """dst[dst_idx[t] or t] = src[src_idx[t] or t] for t < n; the rest of dst is untouched."""
    out = dst.clone()
    s = torch.arange(n) if src_idx is None else src_idx.long()[:n]
    d = torch.arange(n) if dst_idx is None else dst_idx.long()[:n]
    out[d] = src[s]
    return out


def rows_to_f32_ref(src, src_idx, n):
    s = torch.arange(n) if src_idx is None else src_idx.long()[:n]
    return src[s].float()


def t_to_rows_ref(src, dst, dst_idx, n):
    out = dst.clone()
    d = torch.arange(n) if dst_idx is None else dst_idx.long()[:n]
    out[d] = convert_ref(src[:n], kind_of(dst))
    return out


def rows_differ_ref(ids, first, stride, ref, n, frm):
    rows = ids[first:first + (n - 1) * stride + 1:stride]
    return int(bool((rows[:, frm:] != ids[ref, frm:]).any()))


def index_vectors(n, rows, seed):
    """name -> int32 [n] into [0, rows): identity, a permutation (needs rows >= n; also valid as a scatter), repeats (gather only)."""
    g = _gen(seed)
    out = {"identity": torch.arange(n, dtype=torch.int32)}
    if rows >= n:
        out["permutation"] = torch.randperm(rows, generator=g)[:n].to(torch.int32)
    out["repeats"] = torch.randint(0, max(1, min(rows, (n + 1) // 2)), (n,), generator=g).to(torch.int32)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ derived tables (fp64)
def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x * 2.0 ** -0.5))


def gen_table_ref(W):
    """(ref, bound) float64 [img_vocab, H]: gen_aligner(gen_embed) (oracle.ref_cpu.mlp_gelu_projector's arithmetic) on the fp32 values the engine holds."""
    e, w0, b0 = W["gen_embed.weight"].float(), W["gen_aligner.layers.0.weight"].float(), W["gen_aligner.layers.0.bias"].float()
    w2, b2 = W["gen_aligner.layers.2.weight"].float(), W["gen_aligner.layers.2.bias"].float()
    h, mag1 = V.gemm_ref(e[None], w0[None], bias_n=b0, act=1)
    e1 = V.gemm_bound(h[0], mag1[0], e.shape[1], "f32", act=1)
    ref, mag2 = V.gemm_ref(h, w2[None], bias_n=b2)
    carried = e1 @ w2.to(F64).abs().t()
    return ref[0], carried + V.gemm_bound(ref[0], mag2[0] + carried, w2.shape[1], "f32")


def pq_table_ref(W, engine_kind):
    """(ref, bound) float64 [img_vocab, vq_z]: post_quant_conv (1 x 1) of the L2-normalised codebook; the bf16 handle stores it rounded to bf16."""
    cb = W["gen_vision_model.quantize.embedding.weight"].float()
    w = W["gen_vision_model.post_quant_conv.weight"].float().reshape(-1, cb.shape[1])
    b = W["gen_vision_model.post_quant_conv.bias"].float()
    cn, e0 = VI.l2_ref(cb), VI.l2_bound(cb)
    ref = cn @ w.to(F64).t() + b.to(F64)
    mag = cn.abs() @ w.to(F64).abs().t() + b.to(F64).abs()
    carried = e0 @ w.to(F64).abs().t()
    bound = carried + V.gemm_bound(ref, mag + carried, cb.shape[1], "f32")
    if engine_kind == "bf16":
        bound = bound + U_BF16 * (ref.abs() + bound)
    return ref, bound


def rope_ref(max_pos, theta):
    """(cos, sin, bound) float64 [max_pos, 64]: phi = p theta^(-2j/128)."""
    j = torch.arange(64, dtype=F64)
    phi = torch.arange(max_pos, dtype=F64)[:, None] * torch.pow(torch.tensor(float(theta), dtype=F64), -2.0 * j / 128.0)[None, :]
    bound = (ROPE_PHASE_ULPS * U_F32 * phi + ROPE_FN_ULPS * U_F32) * (1 + 2.0 ** -20)
    return torch.cos(phi), torch.sin(phi), bound


def rope_host_emul(max_pos, theta):
    """The host loop of pg_finalize_weights in numpy fp32 (another libm than the engine's: the CPU test uses it to see that the bound has room)."""
    import numpy as np
    j = np.arange(64, dtype=np.float32)
    inv = np.float32(1.0) / np.power(np.float32(theta), (2 * j) / np.float32(128.0), dtype=np.float32)
    f = np.arange(max_pos, dtype=np.float32)[:, None] * inv[None, :]
    return torch.from_numpy(np.cos(f, dtype=np.float32)), torch.from_numpy(np.sin(f, dtype=np.float32))


def within(got, ref, bound):
    """max |got - ref| / bound over the tensor (inf where got is not finite); <= 1 passes."""
    g = got.to(F64).cpu()
    r = (g - ref).abs() / bound
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    return float(r.max()), float((g - ref).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------ planted defects
def defect_conv_swapped(w, dst_kind):
    """tap and channel exchanged: the checkpoint order [Cout][Cin][kk] kept."""
    co, ci = w.shape[:2]
    return convert_ref(w.reshape(co, ci, -1), dst_kind).reshape(co, -1, ci)


def defect_il16_halves(gate, up, dst_kind):
    return il16_ref(up, gate, dst_kind)


def defect_row_dropped(t, row):
    out = t.clone()
    out[row] = from_bits(torch.tensor(SENTINEL[kind_of(t)], dtype=torch.int64), kind_of(t))
    return out


def defect_element_moved(t, i, j):
    out = t.clone().reshape(-1)
    out[i], out[j] = t.reshape(-1)[j], t.reshape(-1)[i]
    return out.reshape(t.shape)
