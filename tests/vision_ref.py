"""References, input families, emulations, mutants and bounds of the operator tests of the understanding path's input-side kernels
(tests/test_gpu_vision_ops.py, tests/test_vision_ref_cpu.py): SigLIP's LayerNorm (both kernels), patchify, add_pos, the VQ encoder's conv_in, the nearest-code
search (both kernels), l2norm_rows, the two-level batched GEMM of SigLIP's scores and P . V, and pg_engine::lin()'s in-place residual / GELU forms.

Everything here runs on the CPU in plain torch.  Notation as tests/vq_ref.py: u = 2^-24 (fp32), ub = 2^-8 (bf16), ``ref`` the float64 result on the SAME (already
rounded) inputs.  Every bound is a function of the reference and the inputs only, first order in u, one rounding wide; none is fitted to a GPU run.

LayerNorm (``ln_bound``)     mean: an fp32 sum of C values in some order, then one division: dm = C u E|x| + u |m|.
                             variance, two-pass: d_i = fl(x_i - m^) carries u |d_i|; sum (x_i - m^)^2 = sum (x_i - m)^2 + C (m - m^)^2 exactly (the cross term sums
                             to zero); C fmaf roundings of the accumulation: dvar = (C + 5) u var + dm^2.
                             rstd = rsqrtf(q / C + eps): division, sum and rsqrtf (2 ulp) = 4 u: rstd lies in
                             [(var + dvar + eps)^-1/2 (1 - 4 u), (max(var - dvar, 0) + eps)^-1/2 (1 + 4 u)]; dr = the farther end's distance from the float64 rstd.
                             y = fl(fl(fl(x - m^) r^) g) + b: t = (x - m) r g; |g| (|x - m| dr + (r + dr) dm) + 4 u |t| + u |b|; a bf16 store adds ub |ref|.
                             A row whose values all equal one power of two is summed exactly in any order (every partial sum is a representable multiple):
                             dm = dvar = 0 there, so y = beta to one rounding -- the constant row of the cases.
patchify, add_pos            index maps (add_pos: one fp32 addition per element): bit exact.
conv_in (``conv_in_bound``)  acc = bias, then 27 fmaf in the order (ci, row, col): 27 roundings of partial results no larger than the bracket
                             sum|x w| + |bias|: 27 u bracket; a bf16 store adds ub |ref|.
nearest code                 float64 distances d_v = |zn|^2 + |e_v|^2 - 2 zn . e_v of the fp32 inputs, zn = z / max(|z|, 1e-12).  The kernel: ss by D fmaf, sqrtf,
                             division: every zn_d carries ez = (D / 2 + 2) u; zz by D fmaf of those: (2 ez + D u) zz; ee: D u ee; dot: (ez + D u) S with
                             S = sum|zn_d e_d|; zz + ee: u (zz + ee); the last fmaf: u (zz + ee + 2 S).  Together
                             err_v = u ((2 D + 6) zz + (D + 2) ee_v + (3 D + 6) S_v)  (``argmin_err``).
                             The kernel returns i with d^_i <= d^_j for all j, so d_i - err_i <= d_min + err_min: index i is ACCEPTED when
                             d_i <= d_min + err_i + err_min.  No case is excluded.  Planted rows (needles, duplicate codes, the zero vector) have a float64 margin
                             of more than twice that and must match the index exactly; among exact duplicates the lower index must win (the distance is the
                             same expression on the same bits in both kernels).
l2norm_rows                  ss: D products and D - 1 sums, sqrtf, division: (D / 2 + 2) u |ref|.
GEMMs                        vq_ref.gemm_bound (imported, not copied)."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from vq_ref import BF, F64, TINY, U_BF16, U_F32, gemm_bound, gemm_ref, rnd, u_of, worst      # noqa: F401  (re-exported for the tests)

LN_EPS = float(torch.tensor(1e-6, dtype=torch.float32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ============================================================================================================================== LayerNorm
# (form, C, M).  form 0 = layernorm_kernel: C < 256 leaves idle threads, 1000 is no multiple of 256, 1152 = 4.5 strides; form 1 = layernorm_wave_kernel<T, 4>:
# four rows per block, so M = 1, 3, 6, 9 end in a partly filled block (M % 4 rows in it) and M = 4 does not.
LN_CASES = [(0, C, M) for C in (64, 128, 1000, 1024, 1152) for M in (1, 5)] + [(1, 1024, M) for M in (1, 3, 4, 6, 9)]
LN_CONST_ROW, LN_CONST_VALUE = 2, 2.0


def ln_form_of(C, ln_wave):
    """Which kernel launch_layernorm picks: 1 = the wave kernel."""
    return 1 if (C == 1024 and ln_wave) else 0


def ln_rows_in_last_block(M):
    return M % 4 or 4


@functools.lru_cache(maxsize=None)
def ln_inputs(M, C):
    """x fp32 [M, C], gamma, beta.  Row r: sigma 0.5 + 0.25 r, its own mean; r % 4 == 1: mean = 100 sigma (alternating sign); row 2: constant 2.0."""
    g = _gen(M * 131 + C)
    x = torch.randn(M, C, generator=g)
    for r in range(M):
        sig = 0.5 + 0.25 * r
        mu = 0.3 * r - 0.5
        if r % 4 == 1:
            mu = 100.0 * sig * (1 if r % 8 == 1 else -1)
        x[r] = x[r] * sig + mu
        if r == LN_CONST_ROW:
            x[r] = LN_CONST_VALUE
    gamma = 1 + 0.3 * torch.randn(C, generator=g) + torch.linspace(-0.2, 0.2, C)
    beta = 0.5 * torch.randn(C, generator=g) + torch.linspace(0.3, -0.3, C)
    return x, gamma, beta


def ln_ref(x, gamma, beta, eps=LN_EPS, mutant=None):
    """float64 LayerNorm with the biased variance.  mutant: None | "unbiased" | "no_eps" | "pad256" (mean over C rounded up to 256) | "swap_gb" | "row_xor1"
    (row m normalised with row m ^ 1's statistics)."""
    x64, g64, b64 = x.to(F64), gamma.to(F64), beta.to(F64)
    M, C = x64.shape
    m = x64.sum(-1, keepdim=True) / (-(-C // 256) * 256 if mutant == "pad256" else C)
    var = ((x64 - m) ** 2).sum(-1, keepdim=True) / (C - 1 if mutant == "unbiased" else C)
    if mutant == "row_xor1":
        perm = torch.tensor([r ^ 1 if (r ^ 1) < M else r for r in range(M)])
        m, var = m[perm], var[perm]
    r = 1.0 / torch.sqrt(var + (0.0 if mutant == "no_eps" else eps))
    if mutant == "swap_gb":
        g64, b64 = b64, g64
    return (x64 - m) * r * g64 + b64


def ln_bound(x, gamma, beta, out_kind, eps=LN_EPS):
    x64, g64, b64 = x.to(F64), gamma.to(F64), beta.to(F64)
    C = x64.shape[1]
    m = x64.mean(-1, keepdim=True)
    var = ((x64 - m) ** 2).mean(-1, keepdim=True)
    dm = C * U_F32 * x64.abs().mean(-1, keepdim=True) + U_F32 * m.abs()
    lo, hi = x64.amin(-1, keepdim=True), x64.amax(-1, keepdim=True)
    exact = (lo == hi) & (torch.frexp(hi.abs())[0] == 0.5) & (hi.abs() * C < 2.0 ** 24)
    dm = torch.where(exact, torch.zeros_like(dm), dm)
    dvar = torch.where(exact, torch.zeros_like(dm), (C + 5) * U_F32 * var + dm * dm)
    r = 1.0 / torch.sqrt(var + eps)
    r_lo = (1.0 / torch.sqrt(var + dvar + eps)) * (1 - 4 * U_F32)
    r_hi = (1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + eps)) * (1 + 4 * U_F32)
    dr = torch.maximum(r_hi - r, r - r_lo)
    t = (x64 - m) * r * g64
    ref = t + b64
    return g64.abs() * ((x64 - m).abs() * dr + (r + dr) * dm) + 4 * U_F32 * t.abs() + U_F32 * b64.abs() + u_of(out_kind) * ref.abs() + TINY


def _tree64(v):
    """wave_sum's butterfly on the last dimension (64 lanes): lane 0's value (all lanes hold the same one)."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block_sum(per_thread):
    """[M, 256] fp32 per-thread partials -> block_sum<4>: four wave butterflies, then red[0] + red[1] + red[2] + red[3] from 0."""
    w = _tree64(per_thread.reshape(-1, 4, 64))
    t = torch.zeros(w.shape[0], dtype=torch.float32)
    for i in range(4):
        t = t + w[:, i]
    return t


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product is exact in double, one rounding to fp32."""
    return (a.double() * b.double() + c.double()).float()


def ln_emul(x, gamma, beta, form, out_kind, eps=LN_EPS):
    """The two kernels' arithmetic in fp32, in their order.  form 0: thread t sums columns t, t + 256, ..; form 1: lane l holds columns j 256 + 4 l .. + 3."""
    M, C = x.shape
    x = x.float()
    if form == 0:
        pad = -(-C // 256) * 256
        xp = torch.zeros(M, pad)
        xp[:, :C] = x
        xs = xp.reshape(M, pad // 256, 256)
        valid = (torch.arange(pad) < C).reshape(pad // 256, 256)
        s = torch.zeros(M, 256)
        for k in range(pad // 256):
            s = s + xs[:, k]
        mean = _block_sum(s) / torch.tensor(float(C))
        q = torch.zeros(M, 256)
        for k in range(pad // 256):
            d = xs[:, k] - mean[:, None]
            q = torch.where(valid[k], _fma32(d, d, q), q)
        rstd = torch.rsqrt(_block_sum(q) / torch.tensor(float(C)) + torch.tensor(eps))
    else:
        v = x.reshape(M, 4, 64, 4)
        s1 = torch.zeros(M, 64)
        for j in range(4):
            s1 = s1 + ((v[:, j, :, 0] + v[:, j, :, 1]) + (v[:, j, :, 2] + v[:, j, :, 3]))
        mean = _tree64(s1) / torch.tensor(float(C))
        q = torch.zeros(M, 64)
        for j in range(4):
            for e in range(4):
                d = v[:, j, :, e] - mean[:, None]
                q = _fma32(d, d, q)
        rstd = torch.rsqrt(_tree64(q) / torch.tensor(float(C)) + torch.tensor(eps))
    return rnd((x - mean[:, None]) * rstd[:, None] * gamma + beta, out_kind)


# ============================================================================================================================== patchify / add_pos
PATCH_CASES = [(S, ps, B) for (S, ps) in ((64, 8), (48, 16), (32, 16)) for B in (1, 3)]       # K = 3 ps^2 = 192 / 768: one and three 256-thread strides
PATCH_TYPES = [(i, o) for i in ("f32", "bf16") for o in ("f32", "bf16")]
ADD_POS_CASES = [(1, 4, 64), (3, 9, 1000)]


def distinct_values(n, exact_bf16):
    """n distinct values.  exact_bf16: every one a NORMAL bf16 number (bit patterns 0x0080.. and 0x8080.., no NaN / inf / denormal), so the values stay distinct
    through any bf16 side; else fp32 values with mantissa bits a bf16 rounding would lose (an fp32 -> fp32 copy that rounded would show)."""
    if not exact_bf16:
        return torch.arange(n, dtype=torch.float32) * 1.0009765625 + 0.3
    assert n <= 2 * 32512
    i = torch.arange(n, dtype=torch.int32)
    bits = torch.where(i < 32512, 0x0080 + i, 0x8080 + (i - 32512))
    return (bits << 16).view(torch.float32).clone()


def patch_image(S, B, in_kind, out_kind):
    n = B * 3 * S * S
    return distinct_values(n, in_kind == "bf16" or out_kind == "bf16")[torch.randperm(n, generator=_gen(S + B))].reshape(B, 3, S, S)


def patchify_ref(img, ps, mutant=None):
    """[B, 3, S, S] -> [B g g, 3 ps ps], row = (b, gy, gx), k = (c, py, px).  mutant: "yx" ((py, px) transposed) | "channel_last" (k = (py, px, c))."""
    B, _, S, _ = img.shape
    g = S // ps
    v = img.reshape(B, 3, g, ps, g, ps)                      # b c gy py gx px
    order = {None: (0, 2, 4, 1, 3, 5), "yx": (0, 2, 4, 1, 5, 3), "channel_last": (0, 2, 4, 3, 5, 1)}[mutant]
    return v.permute(*order).reshape(B * g * g, 3 * ps * ps)


def add_pos_inputs(B, P, C):
    g = _gen(B * 100 + P * 10 + C)
    return torch.randn(B * P, C, generator=g) * 3, torch.randn(P, C, generator=g) + torch.linspace(-1, 1, P)[:, None]


def add_pos_ref(x, pos, B, mutant=None):
    """fp32: x[b P + p] + pos[p].  mutant "row_div_b": p = row / B."""
    P = pos.shape[0]
    rows = torch.arange(x.shape[0])
    p = rows // B if mutant == "row_div_b" else rows % P
    return x + pos[p]


# ============================================================================================================================== conv_in
# (B, H, W, Cout): every W of {1, 63, 64, 65, 130} (strips of 1, 63, 64, 64 + 1, 64 + 64 + 2 pixels), H of {1, 2, 5}, Cout of {32 (96 idle threads), 128,
# 160 (the co += 128 loop: 32 threads walk the strip twice)}, B of {1, 2}.
CONV_IN_CASES = [(1, 1, 1, 32), (2, 2, 63, 128), (1, 5, 64, 160), (2, 1, 65, 32), (1, 2, 130, 160), (2, 5, 130, 128), (1, 5, 65, 128)]
CONV_IN_TYPES = [(i, o) for i in ("f32", "bf16") for o in ("f32", "bf16")]


def conv_in_strips(W):
    """(number of 64-pixel strips, pixels in the last one)."""
    n = (W + 63) // 64
    return n, W - 64 * (n - 1)


@functools.lru_cache(maxsize=None)
def conv_in_inputs(B, H, W, Cout, in_kind):
    """x NCHW [B, 3, H, W] (values of in_kind), w fp32 [Cout, 3, 3, 3], bias.  Asymmetric: a ramp along x and along y on the image, a per-tap ramp on the kernel."""
    g = _gen(B * 1000 + H * 100 + W * 7 + Cout)
    x = torch.randn(B, 3, H, W, generator=g) + torch.linspace(-1, 1, W) + torch.linspace(0.5, -0.5, H)[:, None] + torch.tensor([0.3, -0.2, 0.1])[:, None, None]
    w = torch.randn(Cout, 3, 3, 3, generator=g) / math.sqrt(27) * torch.linspace(0.5, 1.5, 9).reshape(3, 3) * torch.linspace(0.6, 1.4, Cout)[:, None, None, None]
    bias = torch.linspace(-2.0, 2.0, Cout) + 0.01
    return rnd(x, in_kind), w, bias


def _flat_neighbour_pad(x):
    """x padded by one like F.pad, but the left / right pad columns hold what a kernel WITHOUT the sx bounds test reads: the flat neighbours x[.. - 1] / x[.. + 1]."""
    B, C, H, W = x.shape
    flat = F.pad(x.reshape(-1), (1, 1))
    idx = torch.arange(B * C * H * W).reshape(B, C, H, W)
    left, right = flat[idx[..., 0]], flat[idx[..., W - 1] + 2]                  # flat[i + 1] is x[i]
    return left, right


def conv_in_ref(x, w, bias, mutant=None):
    """(ref, bracket) float64 NHWC [B, H, W, Cout].  mutant: "tap_t" (kernel taps transposed) | "no_left_pad" | "no_right_pad" (the flat neighbour in place of the zero)
    | "drop_last" (the last pixel of a row's last strip is not written: NaN)."""
    x64, w64, b64 = x.to(F64), w.to(F64), bias.to(F64)
    if mutant == "tap_t":
        w64 = w64.transpose(-1, -2)
    xp = F.pad(x64, (1, 1, 1, 1))
    if mutant in ("no_left_pad", "no_right_pad"):
        left, right = _flat_neighbour_pad(x64)
        if mutant == "no_left_pad":
            xp[:, :, 1:-1, 0] = left
        else:
            xp[:, :, 1:-1, -1] = right
    ref = F.conv2d(xp, w64, b64).permute(0, 2, 3, 1).contiguous()
    mag = F.conv2d(F.pad(x64.abs(), (1, 1, 1, 1)), w64.abs(), b64.abs()).permute(0, 2, 3, 1).contiguous()
    if mutant == "drop_last":
        ref[:, :, -1, :] = float("nan")
    return ref, mag


def conv_in_bound(ref, mag, out_kind):
    return 27 * U_F32 * mag + u_of(out_kind) * ref.abs() + TINY


def conv_in_emul(x, w, bias, out_kind):
    """acc = bias; 27 fmaf in the kernel's order (ci, row, col); store."""
    B, _, H, W = x.shape
    xp = F.pad(x.float(), (1, 1, 1, 1))
    acc = bias.float().reshape(1, 1, 1, -1).expand(B, H, W, -1)
    for ci in range(3):
        for r in range(3):
            for c in range(3):
                acc = _fma32(xp[:, ci, r:r + H, c:c + W, None], w[:, ci, r, c].float(), acc)
    return rnd(acc, out_kind)


# ============================================================================================================================== nearest code
# (form, D, V, n).  form 0 = vq_argmin_kernel (a block per vector), form 1 = vq_argmin_multi_kernel<8> (D = 8, n >= 64: eight vectors per block; n = 65 / 71 leave
# 7 / 1 slots of the last block clamped to row n - 1, n = 64 / 72 none).  V = 100 < 256 threads, 256 = one stride exactly, 1000 = 3.9 strides, 16384 = production.
ARGMIN_V = (100, 256, 1000, 16384)
ARGMIN_CASES = ([(0, D, V, n) for D in (8, 4) for V in ARGMIN_V for n in (1, 63)] + [(1, 8, V, n) for V in ARGMIN_V for n in (64, 65, 71, 72)])
ARGMIN_SHARED = [(8, V, n) for V in ARGMIN_V for n in (64, 65, 71, 72)]       # form 0 also runs these: its indices must equal form 1's bit for bit
SHORT_CODE, SHORT_SCALE = 7, 0.9                                            # one code of norm 0.9: the zero vector's nearest (dist = |e|^2), and what a missing z normalisation moves


def argmin_multi_taken(D, n, multi=1):
    return bool(D == 8 and multi and n >= 64)


def argmin_clamped_slots(n):
    """Slots of the eight-vector kernel's last block that are clamped to row n - 1."""
    return (8 - n % 8) % 8


def dup_pairs(V):
    """(lower, higher) indices of exact duplicate codes: neighbouring lanes, another wave (+ 64), the same thread one stride later (+ 256)."""
    return [(10, 11), (20, 84)] + ([(300, 556)] if V > 556 else [])


def needle_codes(V):
    return [j for j in (0, 63, 64, 255, 256) if j < V - 1] + [V - 1]


@functools.lru_cache(maxsize=None)
def argmin_inputs(D, V, n):
    """z fp32 [n, D], cb fp32 [V, D] (rows of norm 1 as fp32 F.normalize leaves them, code 7 of norm 0.9, three exact duplicate pairs), planted {row: index}.
    Rows: 0 = the needle at V - 1; then random; needles at 0, 63, 64, 255, 256; one vector on each duplicate pair; the zero vector; the rest random with norms from
    0.01 to 5.  The last row (the one the tail clamp re-reads) is a needle too."""
    g = _gen(D * 1_000_003 + V * 101 + n)
    cb = F.normalize(torch.randn(V, D, generator=g), dim=-1)
    cb[SHORT_CODE] *= SHORT_SCALE
    for lo, hi in dup_pairs(V):
        cb[hi] = cb[lo]
    z = torch.randn(n, D, generator=g) * (10.0 ** (torch.rand(n, 1, generator=g) * 2.7 - 2.0))
    planted = {}
    kinds = [("needle", V - 1), ("random", 0)] + [("needle", j) for j in needle_codes(V)[:-1]] + [("dup", p) for p in dup_pairs(V)] + [("zero", 0)]
    for r, (kind, arg) in enumerate(kinds):
        if r >= n:
            break
        if kind == "needle":
            z[r] = cb[arg] * (0.5 + r)
            planted[r] = arg
        elif kind == "dup":
            z[r] = cb[arg[0]] * 1.7
            planted[r] = arg[0]
        elif kind == "zero":
            z[r] = 0.0
            planted[r] = SHORT_CODE
    if n > len(kinds):
        z[n - 1] = cb[needle_codes(V)[1 % len(needle_codes(V))]] * 0.3
        planted[n - 1] = needle_codes(V)[1 % len(needle_codes(V))]
    return z, cb, planted


def argmin_dist(z, cb, mutant=None):
    """float64 distances [n, V] and the accepted-index error [n, V].  mutant "no_znorm": z is not normalised."""
    z64, e64 = z.to(F64), cb.to(F64)
    D = z64.shape[1]
    zn = z64 if mutant == "no_znorm" else z64 / z64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    zz, ee = (zn * zn).sum(-1, keepdim=True), (e64 * e64).sum(-1)[None, :]
    d = zz + ee - 2 * zn @ e64.t()
    S = zn.abs() @ e64.abs().t()
    err = U_F32 * ((2 * D + 6) * zz + (D + 2) * ee + (3 * D + 6) * S) + TINY
    return d, err


def argmin_ref(z, cb, mutant=None):
    """The float64 first minimum [n].  mutant: "last_tie" (the last of equal minima) | "no_znorm" | "v_floor256" (codes past V rounded down to 256 are never
    looked at; none at all: index 0x7fffffff, the kernels' initial value)."""
    d, _ = argmin_dist(z, cb, "no_znorm" if mutant == "no_znorm" else None)
    V = d.shape[1]
    if mutant == "v_floor256":
        if V // 256 == 0:
            return torch.full((d.shape[0],), 0x7fffffff, dtype=torch.int64)
        return d[:, :V // 256 * 256].argmin(-1)
    if mutant == "last_tie":
        return V - 1 - d.flip(-1).argmin(-1)
    return d.argmin(-1)


def argmin_check(idx, z, cb, planted):
    """dict(ok, worst: max over rows of (d_i - d_min) / (err_i + err_min), bad_rows, planted_bad).  An index outside [0, V) is rejected."""
    d, err = argmin_dist(z, cb)
    n, V = d.shape
    idx = idx.to(torch.int64).reshape(-1)
    inside = (idx >= 0) & (idx < V)
    safe = idx.clamp(0, V - 1)
    dmin, imin = d.min(-1)
    rows = torch.arange(n)
    tol = err[rows, safe] + err[rows, imin]
    ratio = (d[rows, safe] - dmin) / tol
    bad = (~inside) | (ratio > 1.0)
    planted_bad = [r for r, j in planted.items() if int(idx[r]) != j]
    return dict(ok=not bool(bad.any()) and not planted_bad, worst=float(ratio[inside].max()) if bool(inside.any()) else float("inf"),
                bad_rows=bad.nonzero().reshape(-1).tolist(), planted_bad=planted_bad)


def argmin_margins(z, cb, planted):
    """For every planted row: (float64 margin of the planted code to the nearest OTHER distinct code) / (2 x the accepted-index error there): must exceed 1.
    A duplicate of the planted code is not another code."""
    d, err = argmin_dist(z, cb)
    out = {}
    for r, j in planted.items():
        same = (cb == cb[j]).all(-1)
        others = d[r].clone()
        others[same] = float("inf")
        k = int(others.argmin())
        out[r] = float((others[k] - d[r, j]) / (2 * (err[r, j] + err[r, k])))
    return out


def argmin_emul(z, cb):
    """Both kernels' arithmetic in fp32 (the same expression sequence): fmaf chains, sqrtf, division, fmaf(-2, dot, zz + ee); first minimum."""
    z, cb = z.float(), cb.float()
    n, D = z.shape
    ss = torch.zeros(n)
    for d in range(D):
        ss = _fma32(z[:, d], z[:, d], ss)
    nrm = torch.sqrt(ss).clamp_min(torch.tensor(1e-12))
    zn = z / nrm[:, None]
    zz = torch.zeros(n)
    for d in range(D):
        zz = _fma32(zn[:, d], zn[:, d], zz)
    ee = torch.zeros(cb.shape[0])
    dot = torch.zeros(n, cb.shape[0])
    for d in range(D):
        ee = _fma32(cb[:, d], cb[:, d], ee)
        dot = _fma32(zn[:, d, None], cb[None, :, d], dot)
    dist = _fma32(torch.tensor(-2.0), dot, zz[:, None] + ee[None, :])
    return dist.argmin(-1)


# ============================================================================================================================== l2norm_rows
L2_CASES = [(1, 8), (257, 8), (1000, 4)]             # one thread per row: 1 row, 256 + 1 (a second block of one live thread), 1000 = 3.9 blocks


@functools.lru_cache(maxsize=None)
def l2_inputs(n, D):
    x = torch.randn(n, D, generator=_gen(n * 10 + D)) * (10.0 ** (torch.rand(n, 1, generator=_gen(n)) * 6 - 3))
    if n > 1:
        x[n // 2] = 0.0
    return x


def l2_ref(x):
    x64 = x.to(F64)
    return x64 / x64.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def l2_bound(x):
    return (x.shape[1] / 2 + 2) * U_F32 * l2_ref(x).abs() + TINY


def l2_emul(x):
    x = x.float()
    ss = torch.zeros(x.shape[0])
    for d in range(x.shape[1]):
        ss = ss + x[:, d] * x[:, d]
    return x / torch.sqrt(ss).clamp_min(torch.tensor(1e-12))[:, None]


# ============================================================================================================================== SigLIP's two-level batched GEMMs
# (B, NH, P, C), C = NH x 64, as pg_engine::vision_encode lays them out:
#   scores  A = qk [B P][2 C] (q | k): lda 2C, strideA P 2C, strideA2 64; W = qk + C: ldb 2C, strideB P 2C, strideB2 64; out fp32 [B][NH][P][P]: ldc P, strideC NH P P,
#           strideC2 P P; M = N = P, K = 64.
#   P . V   A = p [B][NH][P][P]: lda P, strideA NH P P, strideA2 P P; W = V^T [B][C][P]: ldb P, strideB C P, strideB2 64 P; out T [B P][C]: ldc C, strideC P C,
#           strideC2 = 64 -- a COLUMN offset inside rows of ldc = C; M = P, N = 64, K = P.
HEADS_CASES = [(1, 2, 64, 128), (3, 2, 192, 128), (2, 16, 128, 1024)]
HEADS_RAGGED = (2, 2, 72, 128)                       # fp32 engine only (the bf16 loaders need K % 64 == 0): ragged M and N on the 64 x 64 tiles
HEADS_GAP = 80                                       # the gapped P . V variant: heads 80 columns apart (ldc = NH x 80), 16 sentinel columns between neighbours
# gemm256_try's acceptance rule, restated: K % 64 == 0 and K >= 128; padded tile area <= 5/4 of M N; tiles x batch x batch2 >= 200.  SigLIP's scores have K = 64 and
# its P . V has N = 64 (a 256-wide tile is 4x padding): the rule takes NEITHER at any size.  It does not refuse batch2 > 1 as such: with heads of 128 (K = 128) the
# scores layout at P = 256 and 25 x 8 = 200 (image, head) pairs is the smallest it takes; 24 x 8 = 192 is refused.
T256_HEADS = (25, 8, 256, 128)                       # (B, NH, P, head dim)
T256_HEADS_BELOW = (24, 8, 256, 128)


def gemm256_takes(M, N, K, batches):
    ntm, ntn = -(-M // 256), -(-N // 256)
    return K % 64 == 0 and K >= 128 and ntm * 256 * ntn * 256 <= M * N * 5 // 4 and ntm * ntn * batches >= 200


@functools.lru_cache(maxsize=None)
def heads_inputs(B, NH, P, C, dtype, hd=64):
    """qk [B, P, 2 C], p [B, NH, P, P] (rows sum to 1), vt [B, C, P]; values of dtype.  A scale and an offset per head and per image: no two (image, head) blocks alike."""
    g = _gen(B * 7 + NH * 131 + P * 3 + C)
    hs = (torch.linspace(0.5, 1.5, NH).repeat_interleave(hd)[None, None, :] * torch.linspace(1.0, 1.6, B)[:, None, None])
    qk = torch.randn(B, P, 2 * C, generator=g) * torch.cat([hs, hs.flip(-1)], -1) + torch.linspace(-0.3, 0.3, 2 * C)
    p = torch.softmax(torch.randn(B, NH, P, P, generator=g) * 2.0, -1)
    vt = torch.randn(B, C, P, generator=g) * hs.transpose(1, 2) + torch.linspace(-1, 1, C)[None, :, None] * torch.linspace(1.0, 0.5, B)[:, None, None]
    return rnd(qk, dtype), rnd(p, dtype), rnd(vt, dtype)


def _blocks(B, NH, mutant):
    """(b, h) -> the operand block a kernel reads for output block (b, h).  mutant "swap_levels": the flat block index decoded with the two batch counts swapped."""
    for b in range(B):
        for h in range(NH):
            z = b * NH + h
            yield (b, h), ((z % B, z // B) if mutant == "swap_levels" else (b, h))


def scores_ref(qk, B, NH, P, C, hd=64, mutant=None):
    """(ref, bracket) float64 [B, NH, P, P]."""
    q64 = qk.to(F64)
    ref, mag = torch.empty(B, NH, P, P, dtype=F64), torch.empty(B, NH, P, P, dtype=F64)
    for (b, h), (sb, sh) in _blocks(B, NH, mutant):
        q, k = q64[sb, :, sh * hd:(sh + 1) * hd], q64[sb, :, C + sh * hd:C + (sh + 1) * hd]
        ref[b, h], mag[b, h] = q @ k.t(), q.abs() @ k.abs().t()
    return ref, mag


def pv_ref(p, vt, B, NH, P, C, ldc=None, stride2=64, mutant=None):
    """(ref, bracket) float64 as the FLAT output buffer [(B P - 1) ldc + (NH - 1) stride2 + 64] viewed as [B P, ldc] (NaN where no block writes: the gaps of the gapped
    layout).  mutant: "swap_levels" | "stride2_rows" (head h lands 64 h ROWS down in place of 64 h columns across; what falls outside the buffer is dropped)."""
    ldc = ldc or C
    p64, v64 = p.to(F64), vt.to(F64)
    ref = torch.full((B * P + (NH * stride2 if mutant == "stride2_rows" else 0), ldc), float("nan"), dtype=F64)
    mag = torch.zeros_like(ref)
    for (b, h), (sb, sh) in _blocks(B, NH, mutant if mutant == "swap_levels" else None):
        v = v64[sb, sh * 64:(sh + 1) * 64, :]
        o, m = p64[sb, sh] @ v.t(), p64[sb, sh].abs() @ v.abs().t()
        if mutant == "stride2_rows":
            ref[b * P + h * stride2:b * P + h * stride2 + P, :64] = o
        else:
            ref[b * P:(b + 1) * P, h * stride2:h * stride2 + 64], mag[b * P:(b + 1) * P, h * stride2:h * stride2 + 64] = o, m
    return ref[:B * P], mag[:B * P]


def heads_check(got, ref, mag, K, out_kind):
    """max err / bound over the elements a block owns; elements no block owns (ref NaN) must still hold the NaN pre-fill.  Returns (ratio, gaps_intact)."""
    own = ~torch.isnan(ref)
    g64 = got.to(F64)
    gaps = bool(torch.isnan(g64[~own]).all())
    r, _ = worst((g64[own] - ref[own]).abs(), gemm_bound(ref[own], mag[own], K, out_kind))
    return r, gaps


# ============================================================================================================================== lin() forms
# (name, M, N, K, inplace residual, act, output on the bf16 engine): x += proj(o) / x += fc2(h) (fp32 stream, out == residual), fc1 / the aligner (bias + erf GELU, bf16)
LIN_CASES = [("fc2", 130, 1024, 4096, True, 0, "f32"), ("fc1", 70, 4096, 1024, False, 1, "bf16"), ("proj", 130, 1024, 1024, True, 0, "f32")]


@functools.lru_cache(maxsize=None)
def lin_inputs(name, dtype):
    _, M, N, K, inplace, act, _ = next(c for c in LIN_CASES if c[0] == name)
    g = _gen(M + N + K)
    a = rnd(torch.randn(M, K, generator=g) * torch.linspace(0.5, 1.5, K), dtype)
    w = rnd(torch.randn(N, K, generator=g) * torch.linspace(0.6, 1.4, N)[:, None] / math.sqrt(K), dtype)
    bias = torch.linspace(-1.0, 1.0, N) + 0.01
    res = (torch.randn(M, N, generator=g) * 2 + torch.linspace(3.0, -3.0, N)) if inplace else None
    return a, w, bias, res


@functools.lru_cache(maxsize=None)
def lin_ref(name, dtype):
    _, M, N, K, inplace, act, _ = next(c for c in LIN_CASES if c[0] == name)
    a, w, bias, res = lin_inputs(name, dtype)
    ref, mag = gemm_ref(a[None], w[None], bias_n=bias, res=None if res is None else res[None], act=act)
    return ref[0], mag[0]
