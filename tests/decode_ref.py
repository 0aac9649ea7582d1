"""References, input families and bounds of the decode-step operator tests (tests/test_gpu_decode_ops.py, tests/test_decode_ref_cpu.py).

Everything here runs on the CPU in plain torch.  The kernels under test are the deferred-1/rms RMSNorm pair every bf16 decode step with 65..128
rows runs (round 6) and the slab-folding elementwise kernels around the decode GEMMs:

* producer ``rmsnorm_defer_kernel<4|8>``: ``x += sum_s partial[s]`` (fp32, slab order), ``xw = bf16(x . w)`` WITHOUT the 1/rms, and 8 partial sums
  of squares per row, ``ssq[m][j]`` = columns ``[256 j, 256 j + 256)``;
* consumer ``gemm_skinny3_kernel<4, NCK, 2, true, EPI, 8, TILED>`` with a non-null ssq: turns the 8 partials of a row into 1/rms and scales its
  fp32 result by it (slab epilogue) or the gate / up values before the SwiGLU (EPI 1);
* ``rmsnorm512_kernel<T, 0|4|8>``, ``silu_mul_kernel``, ``bias_act_kernel``.

Three references of the pair, y = W . RMSNorm(x_new) with x_new = x + sum_s partial[s]:

* ``true``  -- float64 throughout: ``W . (w * x_new * rsqrt(mean(x_new^2) + eps))``;
* ``emul``  -- the kernel's rounding points and nothing else: x_new summed in fp32 in slab order, ``xw = bf16(fp32(w) * x_new)`` (one rounding),
  the GEMM over xw in float64, times the float64 1/rms of the fp32 x_new;
* ``refbf`` -- the reference's own bf16 arithmetic (LlamaRMSNorm under bf16): ``bf16(w * bf16(x_hat))``, two roundings, then the float64 GEMM.
  Only the yardstick E_ref = |refbf - true| of the K-rule (tests/bf16ref.py).

Inputs are asymmetric so that a layout mistake cannot pass: per-row magnitudes spread over 1e-3 .. 1e3 (a row scale read from the wrong row is
wrong by orders of magnitude), a per-256-column block scale on x (swapped ssq slots change the slots' values by factors >= 1.5), two "massive
activation" columns (x 300), one in each half-row, and W rows scaled by linspace(0.5, 2).

Bounds are derived from the roundings, never fitted to a GPU run."""
from __future__ import annotations

import functools

import numpy as np
import torch

F64 = torch.float64
H = 2048                            # the launchers' contract: K = H = 2048
EPS = 1e-6
U_BF16 = 2.0 ** -8                  # unit roundoff of bf16 (8 significand bits, round to nearest even)
U_F32 = 2.0 ** -24
BLOCK_SCALE = (1.0, 0.25, 2.0, 0.5, 3.0, 0.125, 1.5, 0.75)         # per 256-column block: no two slots alike
SPIKE_COLS = (137, 1024 + 611)      # one per half-row (= per block of rmsnorm_defer_kernel)
SPIKE = 300.0
SSQ_RTOL = 256 * U_F32              # fp32 sum of 256 non-negative terms, any order (squares rounded once each: (n - 1 + 1) u)

# (M, N, S of the GEMM, S of the producer's partial): the GEMM splits give NCK 16, 8, 4, 2, 1; the producer S both SB instantiations
GEMM_CASES = [(65, 4096, 1, 1), (80, 4096, 2, 8), (100, 6144, 4, 5), (128, 4096, 8, 4), (127, 4096, 16, 2)]
SWIGLU_CASES = [(65, 4096, 4), (97, 4096, 5), (128, 11264, 8)]      # (M, 2 I, S of the producer's partial)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def norm_inputs(M, S, spikes=True, seed=0):
    """x [M, H] fp32, partial [S, M, H] fp32, w [H] bf16.  Cached: callers must not modify the tensors."""
    g = _gen(1000 * M + 10 * S + seed)
    rows = torch.logspace(-3, 3, M)[:, None]
    blk = torch.tensor(BLOCK_SCALE).repeat_interleave(256)[None, :]
    x = torch.randn(M, H, generator=g) * rows * blk
    partial = torch.randn(max(S, 1), M, H, generator=g)[:S] * (0.5 * rows * blk)
    if spikes:
        for c in SPIKE_COLS:
            x[:, c] *= SPIKE
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16)
    return x, partial, w


@functools.lru_cache(maxsize=None)
def gemm_weights(N, seed=0):
    """W [N, H] bf16, rows scaled by linspace(0.5, 2)."""
    g = _gen(7 * N + seed)
    return (torch.randn(N, H, generator=g) * torch.linspace(0.5, 2.0, N)[:, None] * 0.05).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def swiglu_weights(I, seed=0):
    """(w_gate, w_up) [I, H] bf16 with different scales: a swapped half changes h = silu(g) u by far more than the bound."""
    g = _gen(11 * I + seed)
    wg = (torch.randn(I, H, generator=g) * 0.02).to(torch.bfloat16)
    wu = (torch.randn(I, H, generator=g) * torch.linspace(0.5, 2.0, I)[:, None] * 0.06).to(torch.bfloat16)
    return wg, wu


def interleave_gate_up(wg, wu):
    """[8 gate | 8 up] rows per 16 (= one MFMA n-tile), as pg_load_tensor / Engine.op_swiglu_gemm lay the decode copy out."""
    I, K = wg.shape
    return torch.stack([wg.reshape(I // 8, 8, K), wu.reshape(I // 8, 8, K)], dim=1).reshape(2 * I, K)


# ------------------------------------------------------------------------------------------------------------------------------ producer
def x_new_f32(x, partial):
    """The residual after the slab fold: fp32 adds in slab order, ((x + p0) + p1) + ... (rmsnorm_row and rmsnorm_defer_kernel alike)."""
    v = x.clone()
    for s in range(partial.shape[0]):
        v = v + partial[s]
    return v


def x_new_f64(x, partial):
    return x.to(F64) + partial.to(F64).sum(0)


def xw_emul(xn32, w):
    """bf16(fp32(w) * x_new): one fp32 product, one round-to-nearest-even to bf16."""
    return (w.float() * xn32).to(torch.bfloat16)


def ssq_ref(xn32):
    """[M, 8] float64 sums of squares of the fp32 residual over columns [256 j, 256 j + 256)."""
    return xn32.to(F64).pow(2).view(xn32.shape[0], 8, 256).sum(-1)


def rs_f64(xn, eps=EPS):
    return torch.rsqrt(xn.to(F64).pow(2).mean(-1, keepdim=True) + eps)


# ------------------------------------------------------------------------------------------------------------------------------ the three references
def pre_true(x, partial, w, eps=EPS):
    """[M, H] float64 GEMM operand of the true reference: w * x_hat."""
    xn = x_new_f64(x, partial)
    return w.to(F64) * (xn * rs_f64(xn, eps))


def pre_refbf(x, partial, w, eps=EPS):
    """LlamaRMSNorm under bf16: statistics in fp32 on the fp32 residual, x_hat rounded to bf16, the bf16 product with w rounded again."""
    xn = x_new_f32(x, partial)
    xh = (xn * torch.rsqrt(xn.pow(2).mean(-1, keepdim=True) + eps)).to(torch.bfloat16)
    return (w * xh).to(F64)                                     # bf16 * bf16 -> bf16: the exact product rounded once


def gemm_true(x, partial, w, W, eps=EPS):
    return pre_true(x, partial, w, eps) @ W.to(F64).t()


def gemm_refbf(x, partial, w, W, eps=EPS):
    return pre_refbf(x, partial, w, eps) @ W.to(F64).t()


def gemm_emul(x, partial, w, W, S=1, eps=EPS):
    """[S, M, N] float64: slab s = the emulated operand's columns [s K / S, (s + 1) K / S) times W's, times the row's float64 1/rms."""
    xn = x_new_f32(x, partial)
    xw, rs = xw_emul(xn, w).to(F64), rs_f64(xn, eps)
    W64, kc = W.to(F64), H // S
    return torch.stack([(xw[:, s * kc:(s + 1) * kc] @ W64[:, s * kc:(s + 1) * kc].t()) * rs for s in range(S)])


def abs_gemm(x, partial, w, W, eps=EPS):
    """sum_k |W[n, k]| |w[k] x_hat[m, k]|: what one relative rounding of the operand can move the result by, per unit of roundoff."""
    return pre_true(x, partial, w, eps).abs() @ W.to(F64).abs().t()


def swiglu(y):
    """y [M, 2 I] float64 in [8 gate | 8 up] column order -> silu(g) * u [M, I]."""
    M, N = y.shape
    t = y.view(M, N // 16, 2, 8)
    g, u = t[:, :, 0].reshape(M, N // 2), t[:, :, 1].reshape(M, N // 2)
    return g * torch.sigmoid(g) * u


def stats(d):
    """max / p99 / p50 / mean of an error tensor (the K-rule's statistics)."""
    d = d.reshape(-1).to(F64).numpy()
    return {"max": float(d.max()), "p99": float(np.percentile(d, 99)), "p50": float(np.percentile(d, 50)), "mean": float(d.mean())}


def k_rule(e_hip, e_ref):
    """E / E_ref per statistic and the ones over K (quantiles, mean) or K_MAX (maximum) of tests/bf16ref.py."""
    import bf16ref
    a, b = stats(e_hip), stats(e_ref)
    ratios = {k: a[k] / b[k] for k in a}
    return ratios, {k: v for k, v in ratios.items() if v > (bf16ref.K_MAX if k == "max" else bf16ref.K)}


# ------------------------------------------------------------------------------------------------------------------------------ elementwise
def slab_sum_bound(x, partial):
    """(S + 1) 2^-24 sum|terms| per element: S fp32 adds, each within u of its exact sum, first order in u with one term of slack."""
    S = partial.shape[0] if partial is not None else 0
    tot = x.to(F64).abs() + (partial.to(F64).abs().sum(0) if S else 0)
    return (S + 1) * U_F32 * tot


def rmsnorm_ref(x, partial, w, eps=EPS):
    """(x_new float64, w * x_hat float64); partial None or [S, M, H]."""
    xn = x.to(F64) if partial is None or partial.shape[0] == 0 else x_new_f64(x, partial)
    return xn, w.to(F64) * (xn * rs_f64(xn, eps))


def silu_mul_ref(gu):
    """gu [S, M, 2 I] fp32, [8 gate | 8 up] interleaved -> float64 silu(sum g) * sum u [M, I]."""
    return swiglu(gu.to(F64).sum(0))


def bias_act_ref(partial, bias, act):
    v = partial.to(F64).sum(0)
    if bias is not None:
        v = v + bias.to(F64)
    return 0.5 * v * (1 + torch.erf(v * 2.0 ** -0.5)) if act == 1 else v


def elementwise_bound(ref, dtype):
    """f32: 1e-5 max|ref|; bf16: one rounding of the result on top of it."""
    b = 1e-5 * ref.abs().max()
    return b + U_BF16 * ref.abs() if dtype == "bf16" else b.expand_as(ref)
