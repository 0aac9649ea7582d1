"""References, input families, emulations and bounds of the VQ-16 decoder operator tests (tests/test_gpu_vq_ops.py, tests/test_vq_ref_cpu.py).

Everything here runs on the CPU in plain torch.  The kernels under test: the 3x3 convolutions in the forms pg_engine::conv3 runs (128 x 128 implicit GEMM,
256-tile kernel, halo kernel with its fast and generic epilogues, GroupNorm partial sums from the epilogue), GroupNorm statistics / apply, the AttnBlock's
row softmax and batched GEMMs, the four conv_out kernels and the code gather.

Notation: u32 = 2^-24, ub = 2^-8 (the unit roundoffs the tests use for fp32 and bf16), ``ref`` the float64 result on the SAME (already rounded) inputs.
Every bound is a function of the reference and the inputs only, first order in u, derived from the roundings the kernel performs; none has the form
c x max|ref| and no constant is fitted to a GPU run.

conv / GEMM (``dot_bound``)      the products of bf16 operands are exact in fp32; K of them are accumulated in fp32 in some order: (K - 1) u32 sum|a w|.  The
                                 epilogue adds bias (and bias_m) and the residual in fp32, one rounding each, on a partial result no larger than
                                 sum|a w| + |bias| + |res|.  Together: (K + 2) u32 (sum|a w| + |bias| + |res|) [+ 5 u32 |ref| for the erf GELU].  The fp32 engine
                                 rounds each fmaf once: the same expression.  A bf16 residual is exact in fp32 and the kernels do not round the sum
                                 separately, so it adds nothing of its own.  A bf16 store adds ub |ref|.
GroupNorm statistics             ``stat_bounds``: a (split, group) partial is an fp32 sum of n values in some order: |ds| <= n u32 sum|x|,
                                 |dq| <= (n + 1) u32 sum x^2 (the square is rounded too); the splits are added in double (no term).
                                 mean: dm = n u32 E|x| + u32 |m|.  var = E[x^2] - m^2: dvar = (n + 1) u32 E[x^2] + 2 |m| n u32 E|x|.
                                 rstd lies in [(var + dvar + eps)^-1/2 (1 - u32), (max(var - dvar, 0) + eps)^-1/2 (1 + u32)].
                                 The convolution epilogues sum the UNROUNDED fp32 values v, also when the output is stored as bf16 (Epi::store4_batch hands
                                 back v before pack_bf16x2; halo_epi_stores_impl sums v before it packs).  The bound covers only that: an fp32 output is
                                 compared with the statistics of the tensor read back; a bf16 output with the statistics of the float64 reference, every
                                 summed value being within the convolution bound d of it (E[d] on the mean, E[2 |x| d + d^2] on E[x^2]) -- a bf16
                                 rounding term (2^-8 E|x|) would hide a whole tile's partial taken from the neighbouring group.
                                 A group whose values all equal c = m 2^k (m odd) with n m^2 < 2^24 is summed exactly in any order (c^2 and every partial
                                 sum are representable multiples): mean = c and rstd = fp32(eps^-1/2) to the bit.
GroupNorm output                 ``gn_out_bound``: a = fl(rstd gamma), sh = fl(beta - mean a), t = fma(x, a, sh).  Both products use the SAME a, so
                                 t - t_ref = (x - m) da - a dm + roundings: |x - m| da + |a| dm + u32 (2 |m a| + |beta| + |t|), da = |gamma| dr + u32 |a|.
                                 swish s = t sigmoid(t): |s'| <= 1.1 carries dt; the evaluation (exp within (|t| + 2) u32 for the fast __expf = exp2(t log2 e),
                                 1 + e, reciprocal, product: one rounding each) adds (|t| + 5) u32 |s|; the store u_out |ref|.
softmax                          ``softmax_bound``: the exponent fl(fl(x s) - mx) is within 4 u32 |s| max|x| =: D of exact; expf 2 u32; the sum of n
                                 positive terms n u32; reciprocal and product 2 u32: p (u_T + 2 D + (n + 6) u32).
conv_out                         dot_bound with K = 9 x 128; the fused tail's operand is bf16(swish(fma(x, a, sh))) with the kernel's own coefficients:
                                 ``tail_operand_bound`` convolved with |w| on top.
vq_gather                        bit exact; the contract: codes < 0 read row 0, codes >= vocab read row vocab - 1.
A value of magnitude below 2^-126 may be flushed: every bound carries that absolute floor."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
TINY = 2.0 ** -126
EPS = float(torch.tensor(1e-6, dtype=torch.float32))      # the kernels take eps as a float
BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def u_of(dtype):
    return U_BF16 if dtype in ("bf16", BF) else U_F32


def rnd(t, dtype):
    """Round to the storage type and back to fp32."""
    return t.to(BF).float() if dtype in ("bf16", BF) else t.float()


# ============================================================================================================================== convolution
# (name, B, Hi, Wi, Cin, Cout, up, stride2).  halo128: exactly 128 tiles of 8 x 32 (grid = tiles); halo280: 280 tiles > the 256 persistent blocks, 56 per image, so
# blocks 0..23 walk two tiles and the second lies in another image; haloup: the nearest-2x form, 128 output tiles.
HALO_CASES = [("halo128", 2, 64, 256, 128, 128, 0, 0), ("halo280", 5, 64, 224, 128, 128, 0, 0), ("haloup", 2, 32, 128, 128, 128, 1, 0)]
# the 256-tile kernel with partials: N = 256, HW = 12800 (% 64 == 0), M = 51200 -> exactly 200 tiles of 256 x 256
T256_CASE = ("t256", 4, 128, 100, 64, 256, 0, 0)
# the 128 x 128 kernel (and the fp32 engine) on what only it takes: odd-sided stride 2 (Ho = Hi // 2, the last row / column never read), Cin != Cout, ragged M and N
SMALL_CASES = [("s2odd", 2, 11, 13, 64, 96, 0, 1), ("s2even", 1, 12, 16, 128, 160, 0, 1), ("up96", 1, 5, 7, 64, 96, 1, 0)]
RES_OUT = [(res, out) for res in ("none", "f32", "bf16") for out in ("bf16", "f32")]     # epk 0, 1, generic (f32 -> bf16), 3, 4, generic (bf16 -> f32)


def case_by_name(name):
    for c in HALO_CASES + [T256_CASE] + SMALL_CASES:
        if c[0] == name:
            return c
    raise KeyError(name)


def out_hw(case):
    _, B, Hi, Wi, Cin, Cout, up, s2 = case
    return (Hi // 2, Wi // 2) if s2 else (Hi << up, Wi << up)


@functools.lru_cache(maxsize=None)
def conv_inputs(name, dtype="bf16"):
    """x NHWC [B, Hi, Wi, Cin], w OIHW, bias [Cout], residual NHWC [B, Ho, Wo, Cout] (fp32 values; the bf16 residual is its rounding).  Asymmetric: a per-input-
    channel scale ramp on x, a per-output-channel ramp on w, a bias that moves every GroupNorm group's mean to its own offset in [-8, 8] (the convolution's
    own sigma is ~1) with a distinct value per channel, and a residual with its own per-channel offsets.  Cached: callers must not modify the tensors."""
    _, B, Hi, Wi, Cin, Cout, up, s2 = case_by_name(name)
    g = _gen(sum(map(ord, name)) * 131 + Cin)
    x = rnd(torch.randn(B, Hi, Wi, Cin, generator=g) * torch.linspace(0.5, 1.5, Cin), dtype)
    w = rnd(torch.randn(Cout, Cin, 3, 3, generator=g) * torch.linspace(0.6, 1.4, Cout)[:, None, None, None] / math.sqrt(9 * Cin), dtype)
    cpg = max(Cout // 32, 1)
    bias = torch.linspace(-8.0, 8.0, 32).repeat_interleave(cpg)[:Cout].clone() + 0.05 * torch.randn(Cout, generator=g)
    Ho, Wo = out_hw(case_by_name(name))
    res = torch.randn(B, Ho, Wo, Cout, generator=g) * 0.7 + torch.linspace(2.0, -2.0, Cout)
    return x, w, bias, res


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv(x_nhwc, w, up, s2, dt):
    xin = _nchw(x_nhwc).to(dt)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if s2:
        return F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.to(dt), None, stride=2).permute(0, 2, 3, 1)
    return F.conv2d(xin, w.to(dt), None, padding=1).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def conv_core(name, dtype="bf16"):
    """(sum_k a_k w_k, sum_k |a_k w_k|) in float64, NHWC, without bias / residual: computed once per case and shared."""
    case = case_by_name(name)
    x, w, _, _ = conv_inputs(name, dtype)
    return _conv(x, w, case[6], case[7], F64).contiguous(), _conv(x.abs(), w.abs(), case[6], case[7], F64).contiguous()


def conv_residual(name, res_kind):
    """The residual tensor as the kernel receives it (fp32 values), or None."""
    r = conv_inputs(name)[3]
    return None if res_kind == "none" else (r if res_kind == "f32" else rnd(r, "bf16"))


def conv_ref(name, res_kind, dtype="bf16"):
    """(ref, bound without the store term) float64 NHWC."""
    case = case_by_name(name)
    dot, absdot = conv_core(name, dtype)
    bias = conv_inputs(name, dtype)[2].to(F64)
    r = conv_residual(name, res_kind)
    ref = dot + bias
    mag = absdot + bias.abs()
    if r is not None:
        ref = ref + r.to(F64)
        mag = mag + r.to(F64).abs()
    return ref, dot_bound(mag, 9 * case[4])


def dot_bound(mag, K, ref=None, u_out=0.0, gelu=False):
    """(K + 2) u32 (sum|a w| + |bias| + |res|) [+ 5 u32 |ref| for GELU] + u_out |ref| + 2^-126.  mag = the bracket."""
    b = (K + 2) * U_F32 * mag + TINY
    if ref is not None:
        b = b + (u_out + (5 * U_F32 if gelu else 0.0)) * ref.abs()
    return b


@functools.lru_cache(maxsize=None)
def _conv_f32(name, dtype="bf16"):
    case = case_by_name(name)
    x, w, _, _ = conv_inputs(name, dtype)
    return _conv(x, w, case[6], case[7], torch.float32).contiguous()


def conv_emul(name, res_kind, out_kind, dtype="bf16"):
    """The operation in the production types in plain torch: fp32 convolution of the bf16-valued operands, + bias, + residual in fp32, stored as out_kind.
    Returns (stored tensor as fp32, the fp32 values before the store)."""
    case = case_by_name(name)
    x, w, bias, _ = conv_inputs(name, dtype)
    v = _conv_f32(name, dtype) + bias
    r = conv_residual(name, res_kind)
    if r is not None:
        v = v + r
    v = v.contiguous()
    return rnd(v, out_kind), v


# ------------------------------------------------------------------------------------------------------------------------------ statistics
def group_view(x, B, HW, C):
    return x.reshape(B, HW, 32, C // 32)


def stats_ref(x, B, HW, C, eps=EPS):
    """float64 (mean, rstd, var) [B, 32] of x [B, HW, C] (any float type)."""
    v = group_view(x.to(F64), B, HW, C)
    m = v.mean((1, 3))
    var = (v * v).mean((1, 3)) - m * m
    var = var.clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + eps), var


def exact_groups(x, B, HW, C):
    """[B, 32] bool: every value of the group equals c = m 2^k (m odd) with n m^2 < 2^24 -> c, c^2 and every partial sum of either are representable: summed
    exactly in any order."""
    v = group_view(x.to(F64), B, HW, C)
    lo, hi = v.amin((1, 3)), v.amax((1, 3))
    mant, _ = torch.frexp(hi)
    m = mant.abs() * 2.0 ** 24                       # integer when the value has <= 24 significant bits; its odd part is what is repeated
    odd = m.clone()
    for _ in range(24):
        odd = torch.where((odd % 2 == 0) & (odd > 0), odd / 2, odd)
    n = HW * (C // 32)
    return (lo == hi) & (odd * odd * n < 2.0 ** 24)


def stat_bounds(x, B, HW, C, n_split, elem_err=None, eps=EPS):
    """x: the tensor the statistics describe, or (elem_err given) a float64 tensor every summed value is within elem_err of.  n_split: values per (split, group)
    partial sum.  Returns (mean, dm, rstd, rstd_lo, rstd_hi) float64 [B, 32]."""
    v = group_view(x.to(F64), B, HW, C)
    m, rstd, var = stats_ref(x, B, HW, C, eps)
    e1, e2 = v.abs().mean((1, 3)), (v * v).mean((1, 3))
    ds = n_split * U_F32 * e1
    dq = (n_split + 1) * U_F32 * e2
    if elem_err is not None:
        d = group_view(elem_err.to(F64), B, HW, C)
        ds = ds + d.mean((1, 3))
        dq = dq + (2 * v.abs() * d + d * d).mean((1, 3))
    dm = ds + U_F32 * m.abs()
    dvar = dq + 2 * m.abs() * ds
    ex = exact_groups(x, B, HW, C) if elem_err is None else torch.zeros_like(m, dtype=torch.bool)
    dm = torch.where(ex, torch.zeros_like(dm), dm)
    dvar = torch.where(ex, torch.zeros_like(dvar), dvar)
    lo = (1.0 / torch.sqrt(var + dvar + eps)) * (1 - U_F32)
    hi = (1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + eps)) * (1 + U_F32)
    return m, dm + TINY, rstd, lo, hi


def stats_err_ratio(mean, rstd, bounds):
    """max over (image, group) of |mean - m| / dm and of the distance of rstd outside [lo, hi] relative to the interval's half-width + u32 rstd (<= 1 passes)."""
    m, dm, r, lo, hi = bounds
    a = ((mean.to(F64) - m).abs() / dm).max()
    half = (hi - lo) / 2
    b = ((rstd.to(F64) - (hi + lo) / 2).abs() / half).max()
    return float(a), float(b)


def tile_partials(v, th, tw):
    """fp32 (sum, sum of squares) per (image, tile, group) of v NHWC fp32 [B, H, W, C]: the convolution epilogues' partials, tiles in row-major order."""
    B, H, W, C = v.shape
    t = v.reshape(B, H // th, th, W // tw, tw, 32, C // 32)
    s = t.sum((2, 4, 6), dtype=torch.float32).reshape(B, -1, 32)
    q = (t * t).sum((2, 4, 6), dtype=torch.float32).reshape(B, -1, 32)
    return s, q


def split_partials(x, B, HW, C):
    """gn_stats_kernel's partials: nsplit = min(256, ceil(HW / 64)) splits of per = ceil(HW / nsplit) pixels; fp32 sums."""
    ns = gn_nsplit(HW)
    per = -(-HW // ns)
    v = torch.zeros(B, ns * per, C, dtype=torch.float32)
    v[:, :HW] = x.reshape(B, HW, C).float()
    t = v.reshape(B, ns, per, 32, C // 32)
    return t.sum((2, 4), dtype=torch.float32), (t * t).sum((2, 4), dtype=torch.float32), per


def gn_nsplit(HW):
    return max(1, min(256, (HW + 63) // 64))


def finalize_emul(s, q, cnt, eps=EPS):
    """gn_finalize_kernel: the splits in double, var clamped at 0, (mean, rstd) rounded to fp32."""
    sd, qd = s.double().sum(1), q.double().sum(1)
    mean = sd / cnt
    var = (qd / cnt - mean * mean).clamp_min(0.0)
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float()


# ============================================================================================================================== GroupNorm
# (B, HW, C): every C, every HW of the issue; 16400 > 16384 caps the splits at 256 with per = 65; (64, 576, 512): 144 (bf16) / 288 (fp32) blocks of vectors per
# image against the cap 4096 / 64 + 1 = 65 blocks -> four vectors in flight per thread with a ragged last one (144 = 65 + 65 + 14, bf16 output) and, for the fp32
# output, a second trip of the U = 4 stride loop that ends ragged (288 = 4 x 65 + 28).
GN_CASES = [(2, 1, 32), (2, 63, 96), (3, 64, 128), (2, 65, 256), (2, 576, 512), (3, 576, 96), (1, 16400, 32), (64, 576, 512)]
GN_PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16")]
CONST_GROUP, CONST_VALUE = 5, 2.0


@functools.lru_cache(maxsize=None)
def gn_inputs(B, HW, C, in_kind):
    """x [B, HW, C] (values of in_kind), gamma, beta.  Per-channel sigma ramp 0.5 .. 2, group means offset by up to +-8 sigma (different per image), group 5 constant."""
    g = _gen(B * 7919 + HW * 31 + C)
    cpg = C // 32
    sig = torch.linspace(0.5, 2.0, C)
    off = (torch.linspace(-8.0, 8.0, 32)[None, :] * torch.linspace(1.0, 0.5, B)[:, None]).repeat_interleave(cpg, dim=1)      # [B, C] in sigma units
    x = torch.randn(B, HW, C, generator=g) * sig + (off * sig)[:, None, :]
    x[:, :, CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = CONST_VALUE
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    return rnd(x, in_kind), gamma, beta


def swish64(t):
    return t * torch.sigmoid(t)


def gn_ref(x, gamma, beta, swish, eps=EPS):
    B, HW, C = x.shape
    m, r, _ = stats_ref(x, B, HW, C, eps)
    cpg = C // 32
    t = (x.to(F64) - m.repeat_interleave(cpg, 1)[:, None, :]) * (r.repeat_interleave(cpg, 1)[:, None, :] * gamma.to(F64)) + beta.to(F64)
    return swish64(t) if swish else t


def gn_out_bound(x, gamma, beta, swish, out_kind, bounds, eps=EPS):
    """See the module docstring.  bounds = stat_bounds(x, ..) of the statistics the apply pass used."""
    B, HW, C = x.shape
    cpg = C // 32
    m, dm, r, lo, hi = (t.repeat_interleave(cpg, 1)[:, None, :] for t in bounds)
    g64, b64, x64 = gamma.to(F64), beta.to(F64), x.to(F64)
    dr = torch.maximum(hi - r, r - lo)
    a = r * g64
    da = g64.abs() * dr + U_F32 * a.abs()
    t = (x64 - m) * a + b64
    dt = (x64 - m).abs() * da + a.abs() * dm + U_F32 * (2 * (m * a).abs() + b64.abs() + t.abs())
    if not swish:
        return dt + u_of(out_kind) * t.abs() + TINY
    s = swish64(t)
    return 1.1 * dt + (t.abs() + 5) * U_F32 * s.abs() + u_of(out_kind) * s.abs() + TINY


def gn_emul(x, gamma, beta, swish, out_kind, eps=EPS, defect=None):
    """launch_gn_stats + launch_gn_apply in the production types: fp32 split partials, double finalize, fp32 coefficients, fp32 fma, store.
    defect: None, "drop_split" (one 64-pixel split missing from the sums) or "mean_early" (mean taken before the last split is added)."""
    B, HW, C = x.shape
    cpg = C // 32
    s, q, _ = split_partials(x, B, HW, C)
    cnt = float(HW * cpg)
    if defect == "drop_split":
        s, q = s.clone(), q.clone()
        s[:, 1], q[:, 1] = 0, 0
    mean, rstd = finalize_emul(s, q, cnt, eps)
    if defect == "mean_early":
        last = (HW - 1) // (-(-HW // gn_nsplit(HW)))
        mean = ((s.double().sum(1) - s[:, last].double()) / cnt).float()
    a = rstd.repeat_interleave(cpg, 1) * gamma                               # fp32
    sh = beta - mean.repeat_interleave(cpg, 1) * a
    t = (x.double() * a.double()[:, None, :] + sh.double()[:, None, :]).float()      # fmaf: the product is exact in double, one rounding
    if swish:
        t = t * (1.0 / (1.0 + torch.exp(-t)))
    return rnd(t, out_kind), mean, rstd, torch.stack([a, sh], -1)


# ============================================================================================================================== softmax
SOFTMAX_CASES = [(1, 1, 128), (3, 63, 512), (4, 64, 128), (5, 65, 512), (2 * 576, 576, 512), (5, 577, 128), (2 * 576, 64, 128), (3, 576, 128)]   # (rows, n, C)


@functools.lru_cache(maxsize=None)
def softmax_inputs(rows, n, C):
    """fp32 scores [rows, n] with s x ~ 3 randn.  Row kinds by (r + n) % 4: random; needle (one dominant score); all equal; large negative scores."""
    g = _gen(rows * 1009 + n)
    x = torch.randn(rows, n, generator=g) * (3.0 * math.sqrt(C))
    for r in range(rows):
        k = (r + n) % 4
        if k == 1:
            x[r, (r * 37) % n] += 40.0 * math.sqrt(C)
        elif k == 2:
            x[r] = -1.25 * math.sqrt(C)
        elif k == 3:
            x[r] = x[r] - 3000.0 * math.sqrt(C)
    return x


def softmax_ref(x, scale):
    return torch.softmax(x.to(F64) * scale, -1)


def softmax_bound(x, scale, out_kind):
    n = x.shape[1]
    p = softmax_ref(x, scale)
    D = 4 * U_F32 * abs(scale) * x.to(F64).abs().amax(-1, keepdim=True)
    return p * (u_of(out_kind) + 2 * D + (n + 6) * U_F32) + TINY


def softmax_emul(x, scale, out_kind, defect=None):
    """fp32: z = x s, max, exp(z - max), sum, 1 / sum, product, store.  defect "lanes63": the sum misses lane 63's terms (columns 63, 127, ..);
    "bf16_scores": the scaled scores are rounded to bf16 before the max is subtracted."""
    z = x * torch.tensor(scale, dtype=torch.float32)
    if defect == "bf16_scores":
        z = z.to(BF).float()
    e = torch.exp(z - z.amax(-1, keepdim=True))
    if defect == "lanes63":
        keep = torch.ones(x.shape[1], dtype=torch.bool)
        keep[63::64] = False
        ssum = (e * keep).sum(-1, keepdim=True)
    else:
        ssum = e.sum(-1, keepdim=True)
    return rnd(e * (1.0 / ssum), out_kind)


# ============================================================================================================================== AttnBlock GEMMs
ATTN_SHAPES = [(128, 64), (512, 576)]           # (C, HW)


@functools.lru_cache(maxsize=None)
def attn_inputs(C, HW, batch, dtype="bf16"):
    """t1 [batch, HW, C] (GroupNorm output), q / k [batch, HW, C], P [batch, HW, HW] (rows sum to 1), V^T [batch, C, HW], attention output o, weights wv / wp
    [C, C] with row ramps, biases bv / bp [C] distinct per channel, fp32 skip tensor [batch, HW, C].  Values already rounded to dtype."""
    g = _gen(C * 13 + HW * 7 + batch)
    ramp = torch.linspace(0.5, 1.5, C)
    d = {}
    d["t1"] = rnd(torch.randn(batch, HW, C, generator=g) * ramp, dtype)
    d["q"] = rnd(torch.randn(batch, HW, C, generator=g) * ramp, dtype)
    d["k"] = rnd(torch.randn(batch, HW, C, generator=g) * ramp.flip(0) + 0.25, dtype)
    d["p"] = rnd(torch.softmax(torch.randn(batch, HW, HW, generator=g) * 2.0, -1), dtype)
    d["vt"] = rnd(torch.randn(batch, C, HW, generator=g) * ramp[:, None] + torch.linspace(-1, 1, C)[:, None], dtype)
    d["o"] = rnd(torch.randn(batch, HW, C, generator=g) * ramp, dtype)
    d["wv"] = rnd(torch.randn(C, C, generator=g) * torch.linspace(0.6, 1.4, C)[:, None] / math.sqrt(C), dtype)
    d["wp"] = rnd(torch.randn(C, C, generator=g) * torch.linspace(1.4, 0.6, C)[:, None] / math.sqrt(C), dtype)
    cpg = C // 32
    d["bv"] = torch.linspace(-3.0, 3.0, C) + 0.01
    d["bp"] = torch.linspace(-8.0, 8.0, 32).repeat_interleave(cpg) + 0.05 * torch.randn(C, generator=g)
    d["skip"] = torch.randn(batch, HW, C, generator=g) * 0.7 + torch.linspace(2.0, -2.0, C)
    return d


T256_GEMM = (128, 256, 200)                     # (C, HW, batch): scores of 256 x 256 per batch -> exactly 200 tiles of the 256-tile kernel; proj_out at N = 256, M = 200 x 256
GELU_CASE = (200, 72, 192, 80)                  # (M, N, K, ldc): ragged M / N, padded ldc
GELU_SCALE_ACT = [(1.0, 1), (0.37, 0), (0.37, 1)]


@functools.lru_cache(maxsize=None)
def t256_gemm_inputs():
    """q, k [batch, HW, C] bf16 values for the batched scores; a [M, 256], wp [256, 256], bp [256], skip [M, 256] for proj_out with partials."""
    C, HW, batch = T256_GEMM
    g = _gen(5)
    q = rnd(torch.randn(batch, HW, C, generator=g) * torch.linspace(0.5, 1.5, C), "bf16")
    k = rnd(torch.randn(batch, HW, C, generator=g) * torch.linspace(1.5, 0.5, C) + 0.25, "bf16")
    N, M = 256, batch * HW
    a = rnd(torch.randn(M, N, generator=g) * torch.linspace(0.5, 1.5, N), "bf16")
    wp = rnd(torch.randn(N, N, generator=g) * torch.linspace(1.4, 0.6, N)[:, None] / 16, "bf16")
    bp = torch.linspace(-8.0, 8.0, 32).repeat_interleave(N // 32) + 0.05 * torch.randn(N, generator=g)
    skip = torch.randn(M, N, generator=g) * 0.7 + torch.linspace(2.0, -2.0, N)
    return q, k, a, wp, bp, skip


@functools.lru_cache(maxsize=None)
def gelu_inputs():
    M, N, K, _ = GELU_CASE
    g = _gen(9)
    a = rnd(torch.randn(M, K, generator=g), "bf16")
    w = rnd(torch.randn(N, K, generator=g) * torch.linspace(0.5, 2.0, N)[:, None] / 8, "bf16")
    return a, w, torch.linspace(-1.0, 1.0, N)


def gemm_ref(A, W, bias_n=None, bias_m=None, res=None, scale=1.0, act=0):
    """A [batch or 1, M, K], W [batch or 1, N, K] -> (ref, bracket) float64 [batch, M, N]: v = A W^T scale + bias_n[col] + bias_m[row] + res; GELU(erf) when act."""
    A64, W64 = A.to(F64), W.to(F64)
    dot = torch.matmul(A64, W64.transpose(-1, -2)) * scale
    mag = torch.matmul(A64.abs(), W64.abs().transpose(-1, -2)) * abs(scale)
    if bias_n is not None:
        dot, mag = dot + bias_n.to(F64), mag + bias_n.to(F64).abs()
    if bias_m is not None:
        dot, mag = dot + bias_m.to(F64)[:, None], mag + bias_m.to(F64).abs()[:, None]
    if res is not None:
        dot, mag = dot + res.to(F64), mag + res.to(F64).abs()
    if act == 1:
        dot = 0.5 * dot * (1 + torch.erf(dot * 2.0 ** -0.5))       # |GELU'| <= 1.13: the bracket's error carries over with that factor (see gemm_bound)
    return dot, mag


def gemm_bound(ref, mag, K, out_kind, act=0, scaled=False):
    """dot_bound; a scale != 1 is one more rounding of the accumulator (K + 3).  GELU v/2 (1 + erf(v / sqrt 2)): its derivative is <= 1.13 on the incoming
    error; erff is accurate relative to |erf| <= 1, not to the result, so in the negative tail the evaluation error is ABSOLUTE: |v| / 2 times (erff 4 u32 + the
    argument's rounding through erf' z <= 1/2 + the sum's u32) <= 3 u32 |v| <= 3 u32 x bracket, taken as 4; plus 5 u32 |ref| for the two products."""
    b = (K + 2 + (1 if scaled else 0)) * U_F32 * mag * (1.13 if act == 1 else 1.0)
    if act == 1:
        b = b + 4 * U_F32 * mag + 5 * U_F32 * ref.abs()
    return b + u_of(out_kind) * ref.abs() + TINY


def gemm_emul(A, W, out_kind, bias_n=None, bias_m=None, res=None, scale=1.0, act=0, defect=None):
    """fp32 matmul + the epilogue in fp32, stored as out_kind.  defect "bias_m_as_n": the per-row bias indexed by the column (square outputs);
    "stridec_row": batch 1 of the output lands one row late (its first row keeps what was there: zeros)."""
    v = torch.matmul(A.float(), W.float().transpose(-1, -2)) * scale
    if bias_n is not None:
        v = v + bias_n
    if bias_m is not None:
        v = v + (bias_m[torch.arange(v.shape[-1]) % bias_m.numel()][None, :] if defect == "bias_m_as_n" else bias_m[:, None])
    if res is not None:
        v = v + res
    if act == 1:
        v = 0.5 * v * (1 + torch.erf(v * torch.tensor(2.0 ** -0.5, dtype=torch.float32)))
    v = rnd(v, out_kind)
    if defect == "stridec_row" and v.shape[0] > 1:
        v = v.clone()
        v[1] = torch.cat([torch.zeros_like(v[1, :1]), v[1, :-1]])
    return v


# ============================================================================================================================== conv_out
# form 1 (strip kernel): (B, H, W); forms 2 / 3 / 4: (B, H, W) with >= 64 tiles of 8 x 32: exactly 64, and 288 > 256
CONV_OUT_SMALL = [(2, 1, 1), (1, 5, 63), (2, 5, 65), (1, 1, 96)]
CONV_OUT_HALO = [(1, 64, 256), (3, 64, 384)]
CONV_OUT_REFUSED = [(1, 60, 256), (1, 64, 240), (1, 56, 256)]      # side not a multiple of the tile (8 / 4 rows, 32 columns); 7 x 8 = 56 < 64 tiles


@functools.lru_cache(maxsize=None)
def conv_out_inputs(B, H, W, Cout, dtype="bf16", Cin=128):
    """x NHWC [B, H, W, Cin] fp32 skip-stream values with the GroupNorm offsets, w [Cout, Cin, 3, 3], bias, gamma, beta."""
    g = _gen(B * 101 + H * 17 + W * 3 + Cout)
    cpg = Cin // 32
    sig = torch.linspace(0.5, 2.0, Cin)
    off = torch.linspace(-8.0, 8.0, 32).repeat_interleave(cpg)
    x = torch.randn(B, H, W, Cin, generator=g) * sig + off * sig
    w = rnd(torch.randn(Cout, Cin, 3, 3, generator=g) * torch.linspace(0.5, 1.5, Cin)[None, :, None, None] / math.sqrt(9 * Cin), dtype)
    bias = torch.tensor([0.3, -1.7, 2.9, -0.6])[:Cout].clone()
    gamma = 1 + 0.3 * torch.randn(Cin, generator=g)
    beta = 0.5 * torch.randn(Cin, generator=g)
    return x, w, bias, gamma, beta


def conv_out_ref(a_nhwc, w, bias):
    """(ref, bracket) float64 NCHW for the operand a (already what the kernel multiplies)."""
    ref = F.conv2d(_nchw(a_nhwc).to(F64), w.to(F64), bias.to(F64), padding=1)
    mag = F.conv2d(_nchw(a_nhwc).to(F64).abs(), w.to(F64).abs(), bias.to(F64).abs(), padding=1)
    return ref, mag


def tail_operand(x, coef):
    """float64 swish(x a + sh) with the kernel's own fp32 coefficients coef [B, C, 2], and the bound of bf16(fast swish(fma(x, a, sh))) against it."""
    a, sh = coef[..., 0].to(F64)[:, None, None, :], coef[..., 1].to(F64)[:, None, None, :]
    t = x.to(F64) * a + sh
    s = swish64(t)
    dt = U_F32 * t.abs()
    return s, 1.1 * dt + (t.abs() + 5) * U_F32 * s.abs() + U_BF16 * s.abs() + TINY


def conv_out_err_term(da_nhwc, w):
    return F.conv2d(_nchw(da_nhwc).to(F64), w.to(F64).abs(), None, padding=1)


# ============================================================================================================================== gather
GATHER_CASES = [(8, "f32"), (8, "bf16"), (256, "f32"), (256, "bf16")]      # (C, type); vocab 37, 200 codes
GATHER_VOCAB, GATHER_N = 37, 200


def gather_table(C, kind):
    return rnd(torch.randn(GATHER_VOCAB, C, generator=_gen(C)) * torch.linspace(0.5, 2.0, C), kind)


def gather_ref(table, codes):
    """The contract: codes < 0 read row 0, codes >= vocab read row vocab - 1."""
    return table[codes.clamp(0, table.shape[0] - 1).long()]


def gather_codes(n, vocab, seed=0):
    c = torch.randint(0, vocab, (n,), generator=_gen(seed + n), dtype=torch.int32)
    c[:6] = torch.tensor([0, vocab - 1, -1, vocab, -2 ** 31, 2 ** 31 - 1], dtype=torch.int64).to(torch.int32)
    return c


def worst(err, bound):
    """(max err / bound, flat index of the worst element); NaN anywhere gives inf."""
    r = (err / bound).reshape(-1)
    if torch.isnan(r).any():
        return float("inf"), int(torch.isnan(r).nonzero()[0])
    i = int(r.argmax())
    return float(r[i]), i
