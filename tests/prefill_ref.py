"""fp64 references, bounds, mutants and case generators of the prefill operator tests (tests/test_gpu_prefill_ops.py, tests/test_prefill_ref_cpu.py).

Everything here runs in plain torch (float64); nothing imports the package.  The operations under test are

* "Q|K|V projection -> RoPE -> cache write under a token map": ``xn [M, K] . Wqkv [3 nh 128, K]^T``, then for packed token m with
  ``row = tok_row[m]``, ``slot = tok_j[m]``, ``pos = min(pos_off[row] + slot, max_pos - 1)``: q and k of every head rotated (rotate_half form:
  ``out[j] = x[j] cos - x[j + 64] sin``, ``out[j + 64] = x[j + 64] cos + x[j] sin``, fp32 tables of ``attn_ref.rope_tables``), q -> ``qbuf[m]``,
  k and v (v unchanged) -> caches ``[R][nh][slots][128]`` at ``(row, head, slot)``.  A token with ``slot >= slots`` owns NOTHING, its qbuf row
  included (both kernels return before the q store).  Kernel forms: the 256 x 256 GEMM's ``act == 3`` epilogue on the [8 | 8]-interleaved
  weight copy (gemm256.hip), or any GEMM followed by ``rope_kv_kernel``.  The reference does not care which.
* ``rope_kv_kernel`` alone: the same on an fp32 ``[S][M][3 nh 128]`` slab tensor summed over S (decode map: token m = row m, slot
  ``len[m] + n_dec``; or the prefill token map).
* the ``act == 2`` SwiGLU epilogue: ``h = silu(g) u`` over ``[8 gate | 8 up]`` column blocks of ``xn . Wgu^T``.
* the two weight interleavers: pure index permutations.

Bounds are per element and derived from the arithmetic, never fitted to a GPU run (u_T = ``attn_ref.U``: 2^-8 bf16, 2^-24 f32):

* RoPE outputs.  The kernel holds fp32 accumulators x~ = x + dx with ``|dx| <= K u_f32 a``, a = the abs-GEMM ``|xn| . |W|^T`` of that
  column (the classical bound of a K-term fp32 dot product in any order, first order in u).  ``out = x0 c -+ x1 s`` therefore carries
  ``K u_f32 (a0 |c| + a1 |s|)`` of accumulation error, plus at most three fp32 roundings of the rotation itself (two products and the sum, or
  a product and a fused multiply-add: ``3 u_f32 (|x0 c| + |x1 s|) <= 3 u_f32 (a0 |c| + a1 |s|)``), then ONE rounding to the storage type
  of the fp32 result: ``u_T |ref| + (1 + 2 u_T) (K + 3) u_f32 (a0 |c| + a1 |s|)``.  v: ``u_T |ref| + (1 + 2 u_T) K u_f32 a``.
  For ``rope_kv_kernel`` alone the slab values are multiples of 2^-12 whose fp32 sum is exact (``attn_ref.make_slabs``): K = 0, a = |x|.
* SwiGLU.  ``h = silu(g) u``: dg and du as above move h by ``|silu'(g)| |u| dg + |silu(g)| du`` (first order; ``silu'(g) = s (1 + g (1 - s))``,
  s = sigmoid(g)); ``(g / (1 + expf(-g))) u`` itself is expf (1 ulp = 2 u), an add, a correctly rounded division and a product: at most 5 u
  relative, taken as ``8 u_f32 |ref|``; then one bf16 rounding.
* floor: ``EPS_ABS u_T max|ref|`` over the tensor -- 2^-12 of one rounding of the largest value.  It never decides a case; it keeps the bound
  positive where the reference is exactly zero.

A kernel result is checked on the elements the token map OWNS; every other qbuf row, cache slot and guard row must still hold the sentinel
bit pattern the buffers were pre-filled with (compared as raw bits)."""
from __future__ import annotations

import torch

import attn_ref as A
import decode_ref as D

F64 = torch.float64
HD = 128
SENTINEL = {"bf16": 0x7FA5, "f32": 0x7FA5A5A5}             # NaN payloads no kernel produces
INT_T = {"bf16": torch.int16, "f32": torch.int32}
GUARD = 3                                                   # guard rows (qbuf, h) / guard cache rows behind the last valid one
OPTS256 = (1, 4, 5, 6, 12, 13, 14)                          # gemm256: auto | 256 / 224 / 192 rows pinned | + 8 = four phases per K tile
LEN_POOL = (1, 63, 64, 65, 255, 256, 257)

# (nh, M, K) of the fused QKV cases and (M, I, K) of the SwiGLU cases: the smallest shapes gemm256_try takes (see gemm256_accepts)
QKV_CASES = [(2, 17000, 128), (2, 16897, 320), (16, 2100, 128), (16, 2305, 192)]
SWIGLU_CASES = [(17000, 384, 128), (17000, 360, 128), (4700, 1408, 192)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------------ tile arithmetic
def tile_counts(M, N):
    """(m-tiles, n-tiles, tiles) of 256 x 256, as gemm256_try counts them whatever tile height it then launches."""
    ntm, ntn = (M + 255) // 256, (N + 255) // 256
    return ntm, ntn, ntm * ntn


def gemm256_accepts(M, N, K):
    """gemm256_try's shape screen for an unbatched launch: K tiles of 64 (at least two), at most 25 % padding, at least 200 tiles."""
    ntm, ntn, tiles = tile_counts(M, N)
    return K % 64 == 0 and K >= 128 and ntm * 256 * ntn * 256 <= M * N * 5 // 4 and tiles >= 200


def last_tile_rows(M, height):
    """Rows of the last m-tile at a tile height (256, 224 or 192); == height: the last tile is full."""
    return M - (M - 1) // height * height


# ------------------------------------------------------------------------------------------------------------------------------ interleavers
def interleave_qk_index(nh):
    """idx [3 nh 128]: row n of launch_interleave_qk's copy = row idx[n] of Wqkv.  Row 16 t + p of a q / k head = row 8 t + p (p < 8) or
    64 + 8 t + p - 8 of that head; v rows stay."""
    c = torch.arange(HD)
    t, p = c // 16, c % 16
    within = torch.where(p < 8, 8 * t + p, 64 + 8 * t + p - 8)
    idx = torch.arange(3 * nh * HD).view(3, nh, HD).clone()
    idx[:2] = idx[:2] - c + within
    return idx.reshape(-1)


def interleave_qk_ref(W, nh):
    return W[interleave_qk_index(nh)]


def deinterleave_qk_ref(Wp, nh):
    out = torch.empty_like(Wp)
    out[interleave_qk_index(nh)] = Wp
    return out


def gate_up_index(I):
    """idx [2 I] into cat(gate, up): row 16 b + p of the interleaved copy = gate row 8 b + p (p < 8) or up row 8 b + p - 8."""
    n = torch.arange(2 * I)
    b, p = n // 16, n % 16
    return torch.where(p < 8, 8 * b + p, I + 8 * b + p - 8)


def interleave16_ref(wg, wu):
    return torch.cat([wg, wu])[gate_up_index(wg.shape[0])]


def deinterleave16_ref(W):
    I = W.shape[0] // 2
    out = torch.empty_like(W)
    out[gate_up_index(I)] = W
    return out[:I], out[I:]


# ------------------------------------------------------------------------------------------------------------------------------ token maps
def make_token_map(seed, M, pool=LEN_POOL, slots=None):
    """Packed prefill token map over M tokens.  Rows of ragged lengths cycled from ``pool`` until M tokens are placed (the last row takes the
    remainder); one more row, in the middle, owns no token.  Rows are packed in a shuffled order and every third row's slots run backwards
    (tok_row / tok_j not monotone); odd rows carry a non-zero pos_off; the longest row's last five positions cross max_pos; two tokens in rows
    other than the last one carry tok_j >= slots (over capacity: they own nothing, and the slot they left is owned by nobody)."""
    g = _gen(seed)
    lens, n, i = [], 0, 0
    while n < M:
        L = min(pool[i % len(pool)], M - n)
        lens.append(L)
        n += L
        i += 1
    empty = len(lens) // 2
    lens.insert(empty, 0)
    R = len(lens)
    assert R >= 4 and lens[R - 1] > 0, "the generator wants a few rows and a last row with tokens"
    slots = slots or max(lens) + 3
    max_pos = max(lens) + 48
    pos_off = [(7 * r) % 41 if r & 1 else 0 for r in range(R)]
    longest = max(range(R), key=lambda r: lens[r])
    pos_off[longest] = max(0, max_pos - lens[longest] + min(5, lens[longest] - 1))
    order = torch.randperm(R, generator=g).tolist()
    tok_row, tok_j = [], []
    for r in order:
        js = list(range(lens[r]))
        if r % 3 == 2:
            js.reverse()
        tok_row += [r] * lens[r]
        tok_j += js
    # two over-capacity tokens: the middle token of the first two packed rows of length >= 2 that are not the last row
    over, m = [], 0
    for r in order:
        if lens[r] >= 2 and r != R - 1 and len(over) < 2:
            over.append(m + lens[r] // 2)
        m += lens[r]
    assert len(over) == 2
    tok_j[over[0]] = slots + 1
    tok_j[over[1]] = 2 * slots - 1
    return {"tok_row": tok_row, "tok_j": tok_j, "pos_off": pos_off, "lens": lens, "R": R, "slots": slots, "max_pos": max_pos, "M": M,
            "over": over, "empty_row": empty, "clamped_row": longest}


def make_decode_map(seed, M, slots=40):
    """Decode token map (rope_kv_kernel mode 0): token m = row m at slot len[m] + n_dec; R = M + 2 rows (the last two own nothing); two rows
    over capacity; some positions past max_pos."""
    g = _gen(seed)
    n_dec = 3
    ln = torch.randint(0, slots - n_dec, (M,), generator=g).tolist()
    over = [M // 3, (2 * M) // 3]
    ln[over[0]] = slots - n_dec + 1
    ln[over[1]] = 2 * slots - 1 - n_dec
    R = M + 2
    max_pos = slots + 16
    pos_off = torch.randint(0, 28, (R,), generator=g).tolist()
    return {"tok_row": list(range(M)), "tok_j": [l + n_dec for l in ln], "len": ln, "n_dec": n_dec, "pos_off": pos_off, "R": R, "slots": slots,
            "max_pos": max_pos, "M": M, "over": over}


def owned_masks(tm):
    """(q_owned [M] bool, cache_owned [R, slots] bool): a token with slot >= slots owns nothing."""
    row, slot = torch.tensor(tm["tok_row"]), torch.tensor(tm["tok_j"])
    q_owned = slot < tm["slots"]
    c = torch.zeros(tm["R"], tm["slots"], dtype=torch.bool)
    c[row[q_owned], slot[q_owned]] = True
    return q_owned, c


def token_map_ok(tm):
    """The host screen of the diag entry points, restated: what a test may hand to a kernel."""
    R, slots = tm["R"], tm["slots"]
    seen = set()
    for r, j in zip(tm["tok_row"], tm["tok_j"]):
        if not (0 <= r < R) or j < 0:
            return False
        if j >= slots:
            if r == R - 1 or j >= 2 * slots:
                return False
            continue
        if (r, j) in seen:
            return False
        seen.add((r, j))
    return all(0 <= p < tm["max_pos"] for p in tm["pos_off"])


# ------------------------------------------------------------------------------------------------------------------------------ cases
def make_qkv_case(seed, nh, M, K, pool=LEN_POOL):
    """xn bf16 [M, K] with a per-column scale, Wqkv bf16 [3 nh 128, K] with a per-(section, head, dim) scale (a transposed, head-swapped or
    section-swapped layout is off by far more than any bound), the token map and the RoPE tables."""
    g = _gen(seed)
    tm = make_token_map(seed + 1, M, pool)
    xn = (torch.randn(M, K, generator=g) * torch.linspace(0.5, 1.5, K)).to(torch.bfloat16)
    ws = 0.3 + 1.4 * torch.rand(3 * nh * HD, 1, generator=g)
    W = (torch.randn(3 * nh * HD, K, generator=g) * ws / K ** 0.5).to(torch.bfloat16)
    cos_t, sin_t = A.rope_tables(tm["max_pos"])
    return {"xn": xn, "W": W, "tm": tm, "cos": cos_t, "sin": sin_t, "nh": nh, "M": M, "K": K}


def make_rope_case(seed, mode, nh, S, M):
    """rope_kv_kernel alone: fp32 slabs [S, M, 3 nh 128] whose sum is exact (attn_ref.make_slabs), a decode (mode 0) or prefill (mode 1) map."""
    g = _gen(seed)
    tm = make_decode_map(seed + 1, M) if mode == 0 else make_token_map(seed + 1, M, pool=(1, 63, 64, 65))
    cos_t, sin_t = A.rope_tables(tm["max_pos"])
    return {"qkv": A.make_slabs(g, S, M, nh), "tm": tm, "cos": cos_t, "sin": sin_t, "nh": nh, "M": M, "S": S, "mode": mode}


def make_swiglu_case(seed, M, I, K):
    """xn bf16 [M, K]; gate and up weights on different scales (swapped halves show), up rows scaled by linspace(0.5, 2); Wgu interleaved."""
    g = _gen(seed)
    xn = (torch.randn(M, K, generator=g) * torch.linspace(0.5, 1.5, K)).to(torch.bfloat16)
    wg = (torch.randn(I, K, generator=g) * (0.3 + 1.4 * torch.rand(I, 1, generator=g)) * 1.5 / K ** 0.5).to(torch.bfloat16)
    wu = (torch.randn(I, K, generator=g) * torch.linspace(0.5, 2.0, I)[:, None] * 0.7 / K ** 0.5).to(torch.bfloat16)
    return {"xn": xn, "wg": wg, "wu": wu, "W": D.interleave_gate_up(wg, wu), "M": M, "I": I, "K": K}


# ------------------------------------------------------------------------------------------------------------------------------ RoPE reference
ROPE_MUTANTS = [("sin_sign",), ("swap_lo_hi",), ("partner32",), ("cols_plain_on_interleaved",), ("cols_interleaved_on_plain",), ("pos", 1), ("pos", -1),
                ("pos_off_row",), ("no_clamp",), ("v_rot",), ("k_slot", 1), ("k_slot", -1), ("head_xor",), ("ragged_meta",)]


def _rope_ref(y, ay, kacc, tm, nh, cos_t, sin_t, dtype, mut=None):
    """y [M, 3 nh 128] float64 projection (or slab sum), ay its abs-GEMM, kacc the K of the accumulation term.  Returns token-space
    expectations q / k / v [M, nh, 128] (render_rope scatters them into the expected qbuf and caches), their bounds bq / bk / bv, where token m's
    k and v go (row, slot; k_slot differs from slot in one mutant only), the owned masks over qbuf rows (q_owned [M]) and cache slots (c_owned
    [R, slots]) and the abs-GEMM the bounds were built from (abs).  ``mut``: a mutant of the operation (ROPE_MUTANTS), for the checker-power tests only."""
    mut = mut or (None,)
    M, R, slots, max_pos = tm["M"], tm["R"], tm["slots"], tm["max_pos"]
    row, slot = torch.tensor(tm["tok_row"]), torch.tensor(tm["tok_j"])
    pos_off = torch.tensor(tm["pos_off"])
    meta = torch.arange(M)
    if mut[0] == "ragged_meta":                                 # every token of a ragged last 256-row tile takes the metadata of token M - 1
        t0 = (M - 1) // 256 * 256
        meta = torch.where(meta >= t0, torch.tensor(M - 1), meta)
    mrow, mslot = row[meta], slot[meta]
    prow = (mrow + 1) % R if mut[0] == "pos_off_row" else mrow
    pos = pos_off[prow] + mslot + (mut[1] if mut[0] == "pos" else 0)
    if mut[0] == "no_clamp":
        cos_t, sin_t = A.rope_tables(int(pos.max()) + 1)
    pos = pos.clamp(0, cos_t.shape[0] - 1)
    c, s = cos_t[pos].to(F64)[:, None], sin_t[pos].to(F64)[:, None]               # [M, 1, 64]
    if mut[0] == "sin_sign":
        s = -s
    if mut[0] == "cols_plain_on_interleaved":                   # the GEMM ran on the interleaved copy, the epilogue assumed the plain order
        idx = interleave_qk_index(nh)
        y, ay = y[:, idx], ay[:, idx]
    if mut[0] == "cols_interleaved_on_plain":                   # the reverse
        inv = torch.empty(3 * nh * HD, dtype=torch.long)
        inv[interleave_qk_index(nh)] = torch.arange(3 * nh * HD)
        y, ay = y[:, inv], ay[:, inv]
    sec = lambda t, i: t[:, i * nh * HD:(i + 1) * nh * HD].reshape(M, nh, HD)
    u_t, u32 = A.U[dtype], A.U["f32"]

    def rot(x, a):
        x0, x1 = x[..., :64], x[..., 64:]
        if mut[0] == "partner32":
            x1 = x[..., 32:96]
        lo, hi = x0 * c - x1 * s, x1 * c + x0 * s
        out = torch.cat([hi, lo], -1) if mut[0] == "swap_lo_hi" else torch.cat([lo, hi], -1)
        w = a[..., :64] * c.abs() + a[..., 64:] * s.abs(), a[..., 64:] * c.abs() + a[..., :64] * s.abs()
        return out, (kacc + 3) * u32 * torch.cat(w, -1)

    def bound(ref, arith):
        return u_t * ref.abs() + (1 + 2 * u_t) * arith + A.EPS_ABS * u_t * ref.abs().max()

    q, eq = rot(sec(y, 0), sec(ay, 0))
    k, ek = rot(sec(y, 1), sec(ay, 1))
    v, ev = sec(y, 2), kacc * u32 * sec(ay, 2)
    if mut[0] == "v_rot":
        v, _ = rot(v, sec(ay, 2))
    if mut[0] == "head_xor":
        assert nh % 2 == 0
        swap = torch.arange(nh) ^ 1
        q, k, v = q[:, swap], k[:, swap], v[:, swap]
    k_slot = mslot + (mut[1] if mut[0] == "k_slot" else 0)
    q_owned = mslot < slots
    if mut[0] == "k_slot":
        k_slot = torch.where(q_owned, k_slot.clamp(0, slots - 1), k_slot)
    c_owned = torch.zeros(R, slots, dtype=torch.bool)
    c_owned[mrow[q_owned], mslot[q_owned]] = True
    return {"q": q, "k": k, "v": v, "bq": bound(q, eq), "bk": bound(k, ek), "bv": bound(v, ev), "row": mrow, "slot": mslot, "k_slot": k_slot,
            "q_owned": q_owned, "c_owned": c_owned, "abs": ay, "R": R, "slots": slots, "nh": nh, "M": M}


def project(xn, W):
    """(xn . W^T, |xn| . |W|^T) in float64 from the bf16 values."""
    x, w = xn.to(F64), W.to(F64)
    return x @ w.t(), x.abs() @ w.abs().t()


def qkv_rope_ref(case, mut=None, proj=None):
    """Reference of "Q|K|V projection -> RoPE -> cache write under a token map" (bf16 storage).  proj: the cached result of project()."""
    y, ay = proj or project(case["xn"], case["W"])
    return _rope_ref(y, ay, case["K"], case["tm"], case["nh"], case["cos"], case["sin"], "bf16", mut)


def rope_kv_ref(case, dtype, mut=None):
    """Reference of rope_kv_kernel alone: the slab sum in float64 (exact by construction of the slabs), no accumulation term."""
    mut = mut or (None,)
    sl = case["qkv"].to(F64)
    if mut[0] == "drop_slab":
        sl = torch.cat([sl[:mut[1]], sl[mut[1] + 1:]])
        mut = (None,)
    y = sl.sum(0)
    return _rope_ref(y, y.abs(), 0, case["tm"], case["nh"], case["cos"], case["sin"], dtype, mut)


# ------------------------------------------------------------------------------------------------------------------------------ buffers and checker
def sentinel_like(shape, dtype, device="cpu"):
    return torch.full(shape, SENTINEL[dtype], dtype=INT_T[dtype], device=device).view(A.TORCH_T[dtype])


def bits(t):
    return t.view(INT_T["bf16" if t.dtype == torch.bfloat16 else "f32"])


def is_sentinel(t):
    dtype = "bf16" if t.dtype == torch.bfloat16 else "f32"
    return bits(t) == SENTINEL[dtype]


def rope_buffers(ref, dtype, device="cpu"):
    """Sentinel-filled (qbuf [M + GUARD, nh 128], kc, vc [R + 1, nh, slots, 128]): guard rows behind qbuf, one guard cache row behind each cache."""
    nh = ref["nh"]
    return (sentinel_like((ref["M"] + GUARD, nh * HD), dtype, device), sentinel_like((ref["R"] + 1, nh, ref["slots"], HD), dtype, device),
            sentinel_like((ref["R"] + 1, nh, ref["slots"], HD), dtype, device))


def render_rope(ref, dtype, values=None):
    """What a kernel computing exactly ``ref`` (or ``values`` = (q, k, v) [M, nh, 128] in any float type) leaves in sentinel-filled buffers."""
    q, k, v = values or (ref["q"], ref["k"], ref["v"])
    T = A.TORCH_T[dtype]
    qb, kc, vc = rope_buffers(ref, dtype)
    o = ref["q_owned"]
    qb[:ref["M"]][o] = q.to(T).reshape(ref["M"], -1)[o]
    kc[ref["row"][o], :, ref["k_slot"][o]] = k.to(T)[o]
    vc[ref["row"][o], :, ref["slot"][o]] = v.to(T)[o]
    return qb, kc, vc


def check_rope(qb, kc, vc, ref):
    """The whole screen of one result against the reference: returns dict(ratio = {q, k, v: max |err| / bound over the OWNED elements},
    sentinel = every un-owned qbuf row, un-owned cache slot and guard row still holds the sentinel, ok).  Works on any device."""
    dev = qb.device
    M, nh = ref["M"], ref["nh"]
    o = ref["q_owned"].to(dev)
    row, slot = ref["row"].to(dev)[o], ref["slot"].to(dev)[o]
    got = {"q": qb[:M].view(M, nh, HD)[o], "k": kc[row, :, slot], "v": vc[row, :, slot]}
    ratio = {}
    for n in ("q", "k", "v"):
        ok, mx, _ = A.check(got[n], ref[n].to(dev)[o], ref["b" + n].to(dev)[o])
        ratio[n] = mx
    cown = ref["c_owned"].to(dev)
    sent = bool(is_sentinel(qb[:M][~o]).all() and is_sentinel(qb[M:]).all())
    for cache in (kc, vc):
        body = cache[:ref["R"]].permute(0, 2, 1, 3)                      # [R, slots, nh, 128]
        sent = sent and bool(is_sentinel(body[~cown]).all() and is_sentinel(cache[ref["R"]:]).all())
        sent = sent and not bool(is_sentinel(body[cown]).any())           # and every owned slot was written in full
    return {"ratio": ratio, "sentinel": sent, "ok": sent and max(ratio.values()) <= 1.0}


def emulate_rope_f32(y32, tm, nh, cos_t, sin_t):
    """Plain fp32 torch emulation of the kernels' arithmetic on fp32 accumulators y32 [M, 3 nh 128]: separate products and sum (one of the
    evaluation orders of attn_ref.rope_variants).  Returns fp32 (q, k, v) [M, nh, 128]."""
    M = y32.shape[0]
    pos = (torch.tensor(tm["pos_off"])[torch.tensor(tm["tok_row"])] + torch.tensor(tm["tok_j"])).clamp(max=tm["max_pos"] - 1)
    c, s = cos_t[pos][:, None], sin_t[pos][:, None]
    sec = lambda i: y32[:, i * nh * HD:(i + 1) * nh * HD].reshape(M, nh, HD)
    rot = lambda x: torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., 64:] * c + x[..., :64] * s], -1)
    return rot(sec(0)), rot(sec(1)), sec(2)


# ------------------------------------------------------------------------------------------------------------------------------ SwiGLU
SWIGLU_MUTANTS = [("swap",), ("block16",), ("col_off4",), ("silu_u",)]


def _silu(g):
    return g * torch.sigmoid(g)


def swiglu256_ref(case, mut=None, proj=None):
    """h = silu(g) u [M, I] in float64 from the [8 gate | 8 up] interleaved projection, and its bound."""
    mut = mut or (None,)
    y, ay = proj or project(case["xn"], case["W"])
    M, I, K = case["M"], case["I"], case["K"]
    blk = 16 if mut[0] == "block16" else 8
    assert I % blk == 0
    split = lambda t: (t.view(M, I // blk, 2, blk)[:, :, 0].reshape(M, I), t.view(M, I // blk, 2, blk)[:, :, 1].reshape(M, I))
    (g, u), (ag, au) = split(y), split(ay)
    if mut[0] == "swap":
        g, u = u, g
    h = _silu(u) * g if mut[0] == "silu_u" else _silu(g) * u
    if mut[0] == "col_off4":
        h = h.roll(4, dims=1)
    sg = torch.sigmoid(g)
    dsilu = (sg * (1 + g * (1 - sg))).abs()
    u_t, u32 = A.U["bf16"], A.U["f32"]
    arith = K * u32 * (dsilu * u.abs() * ag + _silu(g).abs() * au) + 8 * u32 * h.abs()
    return {"h": h, "bound": u_t * h.abs() + (1 + 2 * u_t) * arith + A.EPS_ABS * u_t * h.abs().max()}


def emulate_swiglu_f32(y32, I):
    """fp32 torch emulation: (g / (1 + exp(-g))) * u from fp32 accumulators y32 [M, 2 I]."""
    M = y32.shape[0]
    t = y32.view(M, I // 8, 2, 8)
    g, u = t[:, :, 0].reshape(M, I), t[:, :, 1].reshape(M, I)
    return (g / (1 + torch.exp(-g))) * u


def check_swiglu(hbuf, ref):
    """hbuf bf16 [M + GUARD, I]: (max |err| / bound, guard rows still sentinel)."""
    M = ref["h"].shape[0]
    dev = hbuf.device
    ok, mx, _ = A.check(hbuf[:M], ref["h"].to(dev), ref["bound"].to(dev))
    return mx, bool(is_sentinel(hbuf[M:]).all())
