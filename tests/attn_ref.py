"""fp64 references of the attention kernels, the input families of the attention operator tests and the checker they use.

Everything here runs on the CPU (torch float64).  The kernels under test are

* decode: ``attn_decode_fused_kernel`` (and the unfused pair ``rope_kv_kernel`` + ``attn_kernel`` mode 0): RoPE of q and of the new k summed
  from S fp32 split-K slabs, K/V append at slot ``len + n_dec``, attention over the cached keys ``[0, nprev)`` (odd rows read
  ``[0, kstart)`` from ``shared_row`` when ``shared_len > 0``) plus the new key;
* prefill: ``attn_prefill_flash2_kernel`` / ``attn_prefill_flash_kernel`` / ``attn_kernel`` mode 1: causal attention of every packed token
  over slots ``[0, j]`` of its row;
* SigLIP: ``attn_vit_resident_kernel`` / ``attn_vit_flash_kernel``: non-causal attention over P tokens, heads of 64.

Bounds (``*_bound``) are derived from the kernels' rounding points, never fitted to a GPU run:

* every kernel rounds its fp32 result to the storage type T once: ``u_T * |ref|`` with u_T = 2^-8 (bf16) / 2^-24 (f32), the unit roundoff;
* the flash kernels multiply P (the unnormalised probabilities, fp32) into V after rounding them to bf16 while the denominator sums the
  fp32 values: ``|sum_i (bf16(p_i) - p_i) v_i| / l <= u * sum_i pi_i |v_i|`` (``pv_abs``);
* the prefill flash kernels round ``q * scale`` to bf16 before the QK^T MFMA; that rounding is known exactly, so its effect is the fp64
  difference between the reference with the rounded and the exact scaled query (``qterm``);
* the fused decode kernel computes RoPE as ``q0 * c - q1 * s`` and leaves the fp32 contraction to the compiler; the three possible
  evaluation orders can round differently in the last place, which T-rounding can carry into one element of q or k.  The reference is
  evaluated for all three and their spread is part of the bound (``spread``);
* fp32 accumulation (<= 2 * 864 terms, relative error ~1e-4 at worst) and the approximate exponentials: ``2^-12 * max|v|`` per (row, head).
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64
HD_LLM = 128
U = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24}
EPS_ABS = 2.0 ** -12
TORCH_T = {"bf16": torch.bfloat16, "f32": torch.float32}

# decode geometry of attn_decode_fused_kernel: KPI keys per wave load (64 lanes / lanes per key), KPW = KPI * UN keys per wave iteration,
# chunk = NW * KPW keys per block iteration; big form: UN 6, NW 4; small form: UN 5, NW 8
KPI = {"bf16": 4, "f32": 2}
FORM_UN_NW = {4: (6, 4), 8: (5, 8)}


def decode_geometry(dtype, form):
    un, nw = FORM_UN_NW[form]
    kpw = KPI[dtype] * un
    return KPI[dtype], kpw, nw * kpw


def round_t(x, dtype):
    """Round to the storage type (round to nearest even), returned in float64."""
    return x.to(TORCH_T[dtype]).to(F64)


def f32(x):
    return x.to(torch.float32).to(F64)


def rope_tables(max_pos, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, 64, dtype=F64) / 64.0))
    ang = torch.arange(max_pos, dtype=F64)[:, None] * inv[None, :]
    return torch.cos(ang).float(), torch.sin(ang).float()


def rope_variants(x0, x1, c, s):
    """The fp32 evaluations of (x0 c - x1 s, x1 c + x0 s) a compiler may emit (inputs fp32 values held in float64): fused multiply-add on the
    first product (rope_lo / rope_hi of common.h), on the second, or none.  Products of two fp32 values are exact in float64."""
    a, b = x0 * c, x1 * s
    d, e = x1 * c, x0 * s
    return [
        (f32(a - f32(b)), f32(d + f32(e))),
        (f32(f32(a) - b), f32(f32(d) + e)),
        (f32(f32(a) - f32(b)), f32(f32(d) + f32(e))),
    ]


def _softmax_out(q, k, v):
    """q [h, d], k [h, n, d], v [h, n, d] (float64): o [h, d], pi [h, n] (o is NaN over no key at all)."""
    if k.shape[1] == 0:
        return torch.full_like(q, float("nan")), torch.zeros(q.shape[0], 0, dtype=q.dtype)
    s = torch.einsum("hd,hnd->hn", q, k)
    pi = torch.softmax(s, dim=-1)
    return torch.einsum("hn,hnd->hd", pi, v), pi


# ------------------------------------------------------------------------------------------------------------------------------- decode
def decode_positions(lens, n_dec, shared_len, row_abs):
    """Per local row: (slot of the new key = nprev, kstart = first private key) as the fused kernel computes them."""
    out = []
    for r, L in enumerate(lens):
        nprev = L + n_dec
        sh = shared_len > 0 and (row_abs[r] & 1) == 1
        out.append((nprev, min(shared_len, nprev) if sh else 0))
    return out


def decode_qkv_new(qkv, cos_t, sin_t, r, nh, pos, dtype, drop_slab=None):
    """RoPE'd q, k and v of local row r: lists over the three evaluation orders of (q_T, k_T); v_T.  Shapes [nh, 128]."""
    HD = nh * HD_LLM
    sl = qkv[:, r].to(F64)
    if drop_slab is not None:
        sl = torch.cat([sl[:drop_slab], sl[drop_slab + 1:]])
    a = sl.sum(0)                                          # exact: slab values are multiples of 2^-12 of small magnitude
    q, k, v = a[:HD].view(nh, HD_LLM), a[HD:2 * HD].view(nh, HD_LLM), a[2 * HD:].view(nh, HD_LLM)
    c, s = cos_t[pos].to(F64)[None], sin_t[pos].to(F64)[None]
    qs = [torch.cat([round_t(lo, dtype), round_t(hi, dtype)], 1) for lo, hi in rope_variants(q[:, :64], q[:, 64:], c, s)]
    ks = [torch.cat([round_t(lo, dtype), round_t(hi, dtype)], 1) for lo, hi in rope_variants(k[:, :64], k[:, 64:], c, s)]
    return qs, ks, round_t(v, dtype)


def decode_keys(kc, vc, row_abs, shared_row_abs, nprev, kstart):
    """Cached keys [0, nprev) of one row in slot order: [nh, nprev, 128] K and V (float64)."""
    k = torch.cat([kc[shared_row_abs, :, :kstart], kc[row_abs, :, kstart:nprev]], 1).to(F64)
    v = torch.cat([vc[shared_row_abs, :, :kstart], vc[row_abs, :, kstart:nprev]], 1).to(F64)
    return k, v


def decode_ref(d, dtype, mut=None):
    """Reference of one decode launch.  ``d``: dict of the launch (see make_decode_case).  ``mut`` (checker power tests only): a mutant of
    the reference -- ("drop_key", pos), ("no_new_key",), ("share_shift", +-1), ("rope_pos", +-1), ("drop_slab", s), ("v_head", +1).
    Returns dict: out [M, nh, 128], k_new / v_new [M, nh, 128] (T values), spread / pv_abs [M, nh, 128], vmax [M, nh]."""
    mut = mut or (None,)
    qkv, kc, vc = d["qkv"], d["kc"], d["vc"]
    M, nh, r0 = d["M"], d["nh"], d["r0"]
    scale = torch.tensor(d["scale"], dtype=torch.float32).item()
    row_abs = [r0 + r for r in range(M)]
    outs = torch.zeros(M, nh, HD_LLM, dtype=F64)
    spread, pv_abs = torch.zeros_like(outs), torch.zeros_like(outs)
    k_new, v_new = torch.zeros_like(outs), torch.zeros_like(outs)
    vmax = torch.zeros(M, nh, dtype=F64)
    pos_list = decode_positions(d["len"], d["n_dec"], d["shared_len"], row_abs)
    for r in range(M):
        nprev, kstart = pos_list[r]
        pos = min(d["pos_off"][r] + nprev + (mut[1] if mut[0] == "rope_pos" else 0), d["max_pos"] - 1)
        qs, ks, v_t = decode_qkv_new(qkv, d["cos"], d["sin"], r, nh, pos, dtype, mut[1] if mut[0] == "drop_slab" else None)
        k_new[r], v_new[r] = ks[0], v_t
        if mut[0] == "share_shift" and kstart > 0:
            kstart = max(0, min(nprev, kstart + mut[1]))
        K, V = decode_keys(kc, vc, row_abs[r], d["shared_row_abs"], nprev, kstart)
        if mut[0] == "v_head":
            _, V = decode_keys(kc, vc.roll(-mut[1], dims=1), row_abs[r], d["shared_row_abs"], nprev, kstart)
        if mut[0] == "drop_key" and mut[1] < nprev:
            keep = [i for i in range(nprev) if i != mut[1]]
            K, V = K[:, keep], V[:, keep]
        res = []
        for qv, kv in zip(qs, ks):
            qsc = f32(qv * scale)                              # the kernels scale the T-rounded q in fp32
            if mut[0] == "no_new_key":
                Kf, Vf = K, V
            else:
                Kf, Vf = torch.cat([K, kv[:, None]], 1), torch.cat([V, v_t[:, None]], 1)
            o, pi = _softmax_out(qsc, Kf, Vf)
            res.append((o, pi, Vf))
        o, pi, Vf = res[0]
        outs[r] = o
        spread[r] = torch.stack([(x[0] - o).abs() for x in res]).amax(0)
        pv_abs[r] = torch.einsum("hn,hnd->hd", pi, Vf.abs())
        vmax[r] = Vf.abs().amax(dim=(1, 2)) if Vf.shape[1] else 0.0
    return {"out": outs, "k_new": k_new, "v_new": v_new, "spread": spread, "pv_abs": pv_abs, "vmax": vmax}


def decode_bound(ref, dtype):
    """fp32 attention on exactly the T-rounded inputs: one output rounding, the RoPE evaluation-order spread and the fp32 slack."""
    u = U[dtype]
    return u * ref["out"].abs() + (1 + 2 * u) * ref["spread"] + EPS_ABS * ref["vmax"][..., None]


# ------------------------------------------------------------------------------------------------------------------------------ prefill
def prefill_ref(p, dtype, flash, mut=None):
    """Reference of one packed prefill launch (see make_prefill_case).  flash: the kernel rounds q * scale to bf16 (qterm).  mut:
    ("causal", +-1) shifts the causal mask, ("drop_key", pos), ("v_head", +1).  Returns out [Ntok, nh, 128], pv_abs, qterm, vmax [Ntok, nh]."""
    mut = mut or (None,)
    q, kc, vc = p["q"].to(F64), p["kc"], p["vc"]
    Ntok, nh = q.shape[0], p["nh"]
    scale = torch.tensor(p["scale"], dtype=torch.float32).item()
    out = torch.zeros(Ntok, nh, HD_LLM, dtype=F64)
    pv_abs, qterm = torch.zeros_like(out), torch.zeros_like(out)
    vmax = torch.zeros(Ntok, nh, dtype=F64)
    for r, (off, L) in enumerate(zip(p["row_off"], p["len"])):
        if off < 0:
            continue
        sh = mut[1] if mut[0] == "causal" else 0
        n = min(L + max(sh, 0), kc.shape[2])
        K = kc[r, :, :n].to(F64)
        V = (vc.roll(-mut[1], dims=1) if mut[0] == "v_head" else vc)[r, :, :n].to(F64)
        qr = q[off:off + L].transpose(0, 1)                          # [nh, L, 128]
        j = torch.arange(L)[:, None]
        t = torch.arange(n)[None, :]
        mask = t <= j + sh
        if mut[0] == "drop_key":
            mask = mask & (t != mut[1])
        vm = V.abs().amax(dim=(1, 2))

        def attn(qq):
            s = torch.einsum("hld,hnd->hln", qq, K).masked_fill(~mask, float("-inf"))
            pi = torch.softmax(s, dim=-1)
            return torch.einsum("hln,hnd->hld", pi, V), pi
        qs = f32(qr * scale)
        o, pi = attn(qs)
        out[off:off + L] = o.transpose(0, 1)
        pv_abs[off:off + L] = torch.einsum("hln,hnd->hld", pi, V.abs()).transpose(0, 1)
        if flash:
            o2, _ = attn(round_t(qs, "bf16"))
            qterm[off:off + L] = (o2 - o).abs().transpose(0, 1)
        vmax[off:off + L] = vm[None, :]
    return {"out": out, "pv_abs": pv_abs, "qterm": qterm, "vmax": vmax}


def prefill_bound(ref, dtype, flash):
    """attn_kernel mode 1: fp32 on the T inputs (one output rounding + fp32 slack).  Flash kernels: + bf16 P in the PV product and the
    exactly known effect of the bf16 q * scale."""
    u = U[dtype]
    extra = (u * ref["pv_abs"] + ref["qterm"]) if flash else 0.0
    return u * ref["out"].abs() + (1 + 2 * u) * extra + EPS_ABS * ref["vmax"][..., None]


# ------------------------------------------------------------------------------------------------------------------------------ SigLIP
def vit_ref(qk, vt, B, P, C, NH, scale, mut=None):
    """qk [B*P, 2C] (q | k), vt [B, C, P] (bf16 values): out [B*P, C], pv_abs [B*P, C], vmax [B*P, NH]."""
    mut = mut or (None,)
    x = qk.to(F64).view(B, P, 2, NH, 64)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)          # [B, NH, P, 64]
    v = vt.to(F64).view(B, NH, 64, P).transpose(2, 3)                               # [B, NH, P, 64]
    if mut[0] == "v_head":
        v = v.roll(-mut[1], dims=1)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if mut[0] == "drop_key":
        s[..., mut[1]] = float("-inf")
    pi = torch.softmax(s, dim=-1)
    o = torch.einsum("bhqk,bhkd->bhqd", pi, v)
    pa = torch.einsum("bhqk,bhkd->bhqd", pi, v.abs())
    vm = v.abs().amax(dim=(2, 3))                                                   # [B, NH]
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * P, C)
    return {"out": flat(o), "pv_abs": flat(pa), "vmax": vm[:, None, :].expand(B, P, NH).reshape(B * P, NH)}


def vit_bound(ref):
    """Scores in fp32 from exact bf16 inputs (the scale is applied after the MFMA, in fp32); bf16 P in the PV product; bf16 output."""
    u = U["bf16"]
    vmax = ref["vmax"].repeat_interleave(64, dim=1)
    return u * ref["out"].abs() + (1 + 2 * u) * u * ref["pv_abs"] + EPS_ABS * vmax


# ------------------------------------------------------------------------------------------------------------------------------ checker
def check(got, ref_out, bound):
    """(ok, max |err| / bound, flat index of the worst element).  got: kernel output (any float dtype), same shape as ref_out."""
    err = (got.to(F64).reshape(ref_out.shape) - ref_out).abs()
    ratio = err / bound
    bad = ~torch.isfinite(ratio)
    ratio = torch.where(bad, torch.full_like(ratio, float("inf")), ratio)
    worst = int(ratio.argmax())
    mx = float(ratio.reshape(-1)[worst])
    return mx <= 1.0, mx, worst


def ulp_distance(a, b):
    """Element-wise distance in units in the last place between two tensors of the same float dtype (bf16 or f32)."""
    it = {torch.bfloat16: torch.int16, torch.float32: torch.int32}[a.dtype]
    def key(t):
        i = t.view(it).to(torch.int64)
        mask = (1 << (16 if it == torch.int16 else 32)) - 1
        i = i & mask
        sign = 1 << (15 if it == torch.int16 else 31)
        return torch.where(i & sign != 0, -(i & (sign - 1)), i)
    return (key(a) - key(b)).abs()


# ------------------------------------------------------------------------------------------------------------------------------ inputs
POISON_V = 64.0          # distinctive V of every slot a kernel must not read
POISON_SCORE = 60.0      # score of a poisoned key against the query of its (row, head): dominates every legitimate key
NEEDLE_SCORE = 40.0      # decode needle; legitimate random scores stay within a few units


def _scales(g, shape, lo, hi):
    return lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)


def make_slabs(g, S, M, nh):
    """fp32 split-K slabs [S, M, 3 * nh * 128]: multiples of 2^-12 with a range that differs per (part, head, dim), |value| < 1, so the
    fp32 sum over S <= 8 slabs is exact in any order and V = round_T(sum) is predictable bit for bit."""
    HD = nh * HD_LLM
    R = torch.randint(800, 4000, (3 * HD,), generator=g)
    x = (torch.rand(S, M, 3 * HD, generator=g, dtype=F64) * 2 - 1) * R
    return (x.round() / 4096.0).float()


def make_kv_cache(g, rows, nh, slots, dtype):
    """Random K / V [rows, nh, slots, 128] in T with per-(head, dim) scales and a per-(head, dim) mean in V (transposed layouts fail)."""
    ks = _scales(g, (1, nh, 1, HD_LLM), 0.3, 1.7)
    vs = _scales(g, (1, nh, 1, HD_LLM), 0.2, 1.0)
    vm = _scales(g, (1, nh, 1, HD_LLM), -1.0, 1.0)
    K = torch.randn(rows, nh, slots, HD_LLM, generator=g, dtype=torch.float32) * ks.float()
    V = torch.randn(rows, nh, slots, HD_LLM, generator=g, dtype=torch.float32) * vs.float() + vm.float()
    return K.to(TORCH_T[dtype]), V.to(TORCH_T[dtype])


def _dominant_key(qdir, score, scale, dtype):
    """A T-valued key k = g * sign(qdir) whose score (qdir * scale) . k is about ``score``.  qdir [nh, 128]."""
    den = (qdir.abs().sum(-1, keepdim=True) * scale).clamp_min(1e-6)
    return (torch.sign(qdir) * (score / den)).to(TORCH_T[dtype])


def make_decode_case(seed, dtype, nh, nprevs, S, n_dec=0, shared_len=0, r0=0, row_order="none", needle=False,
                     slots=None, pos_jitter=40, geometry=None):
    """One decode launch.  Local rows r = 0 .. M-1 (absolute cache row r0 + r) carry nprevs[r] cached keys (len = nprev - n_dec).  With
    shared_len > 0 every odd row is an uncond row of prompt length shared_len whose keys [0, shared_len) live in absolute row 1 (local
    row 1 - r0: the two-lane form passes a negative shared_row).  Slots a kernel must not read are poisoned.  needle: every (row, head)
    has one dominant key at a position that sweeps the chunk boundaries (``geometry`` = list of (KPI, KPW, chunk) of the forms that run)."""
    g = torch.Generator().manual_seed(seed)
    M = len(nprevs)
    lens = [n - n_dec for n in nprevs]
    assert min(lens) >= 0
    if shared_len > 0:
        for r in range(M):
            if (r0 + r) & 1:
                assert lens[r] == shared_len, "uncond rows carry the shared prompt"
    if slots is None:
        slots = max(nprevs) + 1 + 32                                   # the engine's max_prompt + max_new: every append slot exists
    rows = r0 + M
    qkv = make_slabs(g, S, M, nh)
    pos_off = torch.randint(0, pos_jitter + 1, (M,), generator=g).tolist()
    max_pos = max(p + n for p, n in zip(pos_off, nprevs)) + 1 + 16
    cos_t, sin_t = rope_tables(max_pos)
    kc, vc = make_kv_cache(g, rows, nh, slots, dtype)
    scale = 1.0 / math.sqrt(HD_LLM)
    row_abs = [r0 + r for r in range(M)]
    pos_list = decode_positions(lens, n_dec, shared_len, row_abs)
    # the queries (reference RoPE) steer the poison / needle keys
    qdirs = []
    for r in range(M):
        pos = min(pos_off[r] + pos_list[r][0], max_pos - 1)
        qs, _, _ = decode_qkv_new(qkv, cos_t, sin_t, r, nh, pos, dtype)
        qdirs.append(qs[0])
    shared_abs = 1 if shared_len > 0 else -1
    read = torch.zeros(rows, slots, dtype=torch.bool)                  # slots some (row, head) of this launch reads
    for r in range(M):
        nprev, kstart = pos_list[r]
        if kstart > 0:
            read[shared_abs, :kstart] = True
        read[row_abs[r], kstart:nprev] = True
    # poison: every slot nobody reads (append slots, private prefix of aliased rows, rows outside the launch, the tail of the cache)
    for a in range(rows):
        pr = [r for r in range(M) if row_abs[r] == a]
        qd = qdirs[pr[0]] if pr else qdirs[0]
        kp = _dominant_key(qd, POISON_SCORE, scale, dtype)
        idx = ~read[a]
        kc[a][:, idx] = kp[:, None]
        vc[a][:, idx] = (POISON_V + torch.arange(HD_LLM, dtype=torch.float32) / 8).to(vc.dtype)
    needles = {}
    if needle:
        marks = set()
        for kpi, kpw, ch in geometry or []:
            for b in (kpi, kpw, ch, 2 * ch):
                marks.update({b - 1, b, b + 1})
        shared_taken = set()
        for r in range(M):
            nprev, kstart = pos_list[r]
            cands = sorted({m for m in marks if 0 <= m < nprev} | {0, nprev - 1, nprev, kstart - 1, kstart})
            cands = [c for c in cands if 0 <= c <= nprev]
            for h in range(nh):
                i = r * nh + h
                p = cands[i % len(cands)] if i < 4 * len(cands) else (i * 97 + 13) % (nprev + 1)
                in_shared = p < kstart
                if in_shared and (h in shared_taken or row_abs[r] == shared_abs):
                    p = kstart if kstart < nprev else nprev
                    in_shared = False
                if p == nprev and kstart > 0:
                    p = nprev - 1 if nprev - 1 >= kstart else nprev
                if in_shared:
                    shared_taken.add(h)
                src = shared_abs if in_shared else row_abs[r]
                if p < nprev:
                    kc[src, h, p] = _dominant_key(qdirs[r][h:h + 1], NEEDLE_SCORE, scale, dtype)[0]
                else:                                                    # needle = the new key: every cached key of this row is pushed far down
                    kc[row_abs[r], h, kstart:nprev] = _dominant_key(qdirs[r][h:h + 1], -NEEDLE_SCORE, scale, dtype)[0]
                needles[(r, h)] = p
    if row_order == "none":
        order = None
    elif row_order == "lpt":                                           # the engine's order: longest private key stream first (stable)
        order = sorted(range(M), key=lambda r: -(pos_list[r][0] - pos_list[r][1]))
    else:
        order = torch.randperm(M, generator=g).tolist()
    return {"qkv": qkv, "kc": kc, "vc": vc, "cos": cos_t, "sin": sin_t, "len": lens, "pos_off": pos_off, "n_dec": n_dec,
            "shared_len": shared_len, "shared_row_abs": shared_abs if shared_len > 0 else 1, "r0": r0, "M": M, "nh": nh, "S": S,
            "slots": slots, "max_pos": max_pos, "scale": scale, "row_order": order, "needles": needles, "dtype": dtype}


PREFILL_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 288]


def make_prefill_case(seed, dtype, nh, lens=None, aliased_row=3, needle=False):
    """One packed prefill launch.  Row ``aliased_row`` has row_off = -1 (no packed token: the shared uncond prompt of the engine).  Slots
    >= len of every row, and every slot of the aliased row, are poisoned; obuf rows past the packed tokens are checked untouched by the
    caller.  needle: q_j = h_j and k_{j+1} = 3 h_j (h_j a random +-1 vector) so the first key in every query's future dominates."""
    g = torch.Generator().manual_seed(seed)
    lens = list(lens or PREFILL_LENS)
    lens.insert(aliased_row, 50)
    R = len(lens)
    max_len = max(lens)
    slots = max_len + 1 + 31
    row_off, tok_row, tok_j, n = [], [], [], 0
    for r, L in enumerate(lens):
        if r == aliased_row:
            row_off.append(-1)
            continue
        row_off.append(n)
        tok_row += [r] * L
        tok_j += list(range(L))
        n += L
    Ntok = n
    kc, vc = make_kv_cache(g, R, nh, slots, dtype)
    qs = _scales(g, (1, nh, HD_LLM), 0.3, 1.7).float()
    q = (torch.randn(Ntok, nh, HD_LLM, generator=g) * qs).to(TORCH_T[dtype])
    scale = 1.0 / math.sqrt(HD_LLM)
    if needle:
        for r, (off, L) in enumerate(zip(row_off, lens)):
            if off < 0:
                continue
            h = torch.randint(0, 2, (L + 1, nh, HD_LLM), generator=g).float() * 2 - 1
            q[off:off + L] = h[:L].to(TORCH_T[dtype])
            kc[r, :, 1:L + 1] = (3 * h[:L]).transpose(0, 1).to(TORCH_T[dtype])
    for r, (off, L) in enumerate(zip(row_off, lens)):
        lo = 0 if off < 0 else L
        qd = q[off + L - 1].to(F64) if off >= 0 else q[0].to(F64)
        kc[r, :, lo:] = _dominant_key(qd, POISON_SCORE, scale, dtype)[:, None]
        vc[r, :, lo:] = POISON_V + torch.arange(HD_LLM, dtype=torch.float32)[None, None] / 8
    return {"q": q, "kc": kc, "vc": vc, "row_off": row_off, "len": lens, "tok_row": tok_row, "tok_j": tok_j, "R": R, "max_len": max_len,
            "Ntok": Ntok, "nh": nh, "slots": slots, "scale": scale, "dtype": dtype}


def make_vit_case(seed, B, P, C, NH, needle=False):
    """qk [B*P, 2C], vt [B, C, P] bf16.  needle: query i of every (image, head) carries h_i, key sigma(i) carries 3 h_i."""
    g = torch.Generator().manual_seed(seed)
    qs = _scales(g, (1, 2 * C), 0.3, 1.7).float()
    qk = (torch.randn(B * P, 2 * C, generator=g) * qs)
    vs = _scales(g, (1, C, 1), 0.2, 1.0).float()
    vm = _scales(g, (1, C, 1), -1.0, 1.0).float()
    vt = torch.randn(B, C, P, generator=g) * vs + vm
    if needle:
        x = qk.view(B, P, 2, NH, 64)
        for b in range(B):
            sigma = torch.randperm(P, generator=g)
            h = torch.randint(0, 2, (P, NH, 64), generator=g).float() * 2 - 1
            x[b, :, 0] = h
            x[b, sigma, 1] = 3 * h
    return {"qk": qk.to(torch.bfloat16), "vt": vt.to(torch.bfloat16), "B": B, "P": P, "C": C, "NH": NH, "scale": 1.0 / math.sqrt(64)}


# ------------------------------------------------------------------------------------------------------------------------------ decode shapes
def decode_counts(dtype):
    """Cached-key counts of the ragged decode launch: 0, 1, KPI +- 1, KPW +- 1 and chunk +- 1 of BOTH forms (one input set serves both),
    2 chunk + 1, and the bench shapes 256 + 575 / 288 + 575."""
    c = {0, 1, 831, 863}
    for form in (4, 8):
        kpi, kpw, ch = decode_geometry(dtype, form)
        c |= {kpi - 1, kpi + 1, kpw - 1, kpw + 1, ch - 1, ch + 1, 2 * ch + 1}
    return sorted(c)


def decode_counts_case(dtype, nh, S, order="none", needle=False, seed=0):
    geo = [decode_geometry(dtype, f) for f in (4, 8)]
    counts = decode_counts(dtype)
    counts = counts[1::2] + counts[0::2]                  # interleave long and short rows
    return make_decode_case(1000 + seed + 7 * S + 3 * nh + (dtype == "bf16"), dtype, nh, counts, S, n_dec=0, row_order=order,
                            needle=needle, geometry=geo, pos_jitter=40 if S % 2 else 0)


def decode_shared_case(dtype, nh, shared_len, n_dec, S, r0=0, needle=False, order="none", seed=0):
    """Uncond rows (odd absolute rows) of prompt length shared_len aliasing absolute row 1; even rows of other lengths.  r0 > 0 (even):
    the second lane of the two-lane decode, whose caches start r0 rows in and whose shared_row is 1 - r0 < 0."""
    geo = [decode_geometry(dtype, f) for f in (4, 8)]
    evens = [shared_len + 37, 1, 290, 2 * shared_len + 3]
    lens = []
    for r in range(6):
        lens.append(shared_len if (r0 + r) & 1 else evens[(r // 2) % len(evens)])
    return make_decode_case(2000 + seed + shared_len + 5 * n_dec + S + r0, dtype, nh, [L + n_dec for L in lens], S, n_dec=n_dec,
                            shared_len=shared_len, r0=r0, row_order=order, needle=needle, geometry=geo)
