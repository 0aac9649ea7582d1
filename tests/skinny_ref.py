"""References, inputs, comparators and planted errors of the decode GEMM dispatch's operator tests (tests/test_gpu_skinny_ops.py,
tests/test_skinny_ref_cpu.py).

Plain torch; every function works on whatever device its arguments live on (the GPU tests compute the float64 products on the device).  The kernels
under test are the skinny decode GEMMs of plangen_amd/csrc/gemm_skinny.h behind launch_gemm_skinny / launch_gemm_skinny_swiglu (gemm.hip):
v1 (gemm_skinny_kernel), v3 (gemm_skinny3_kernel, row-major or tiled W) and v4 (gemm_sk4_kernel, x by LDS-DMA), each in 16 / 32 / 64 / 128-row block
forms, instantiated for 1, 2, 4, 8, 11, 16 or 22 K chunks per split.

* slab s of the reference is ``x[:, ks:ke] . W[:, ks:ke]^T`` in float64, ks = s K / S, ke = (s + 1) K / S: the kernels write slab s at out + s M N
  and never reduce over splits, so the slabs are compared one by one and their sum against the whole product;
* the SwiGLU reference is ``silu(g) u`` in float64 from the de-interleaved columns of the whole product ([8 gate | 8 up] per 16-column n-tile).

Inputs are bf16-rounded and asymmetric: W row n (= output column n) is scaled by linspace(0.5, 2)[n], x row m by 1 + m / M, so a duplicated,
clamped or swapped row and a shifted column differ from the reference by far more than the bound.

Bounds (never fitted to a GPU run):
  slabs   |out - ref| <= 2e-4 max|ref slab| + 1e-4, the same formula for the sum of the slabs against the whole product: the bound this kernel
          family already carries in tests/test_gpu_ops.py.  The operands are exact in bf16, the products exact in fp32, so only the fp32
          accumulation of <= 2816 terms separates a kernel from the float64 value.
  SwiGLU  |h - ref| <= 2^-8 |ref| + 2e-4 max|ref|: one bf16 rounding of h (at most 2^-8 |h|, typically half of it) over the fp32 accumulation term."""
from __future__ import annotations

import functools

import torch

F64 = torch.float64
SK_BK = 128                         # K chunk of the kernels (gemm_skinny.h)
GUARD = 3                           # guard rows in front of / behind a buffer's valid rows
MAX_M = 512
# measured on the CPU against the float64 reference (tests/test_skinny_ref_cpu.py, M = 47, N = 208 / 4096, K = 2048 / 2816, S = 1 .. 16):
#   the reference rounded to fp32 sits at <= 2.5e-4 of the bound, torch's own fp32 matmul of the same operands at <= 1.3e-3 of it
SLAB_RTOL, SLAB_ATOL = 2e-4, 1e-4
# one round-to-nearest of h to bf16 (8 significand bits) moves it by at most 2^-9 of its binade's top, i.e. by up to 2^-8 |h| at the binade's bottom: the
# relative term is that worst case itself, the room is the absolute term.  Measured the same way (M = 47, 2 I = 512 / 4096): the reference rounded to bf16
# at 0.74 / 0.79 of the bound, the epilogue's formula on torch's fp32 matmul rounded to bf16 the same, and that fp32 arithmetic BEFORE the rounding at
# 1.1e-3 / 1.5e-3 of the absolute term -- which is what the fp32 accumulation has to fit into
SWIGLU_RTOL, SWIGLU_ATOL = 2.0 ** -8, 2e-4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _x_base(K):
    return torch.randn(MAX_M, K, generator=_gen(31 * K + 5))


def make_x(M, K):
    """x [M, K] bf16: seeded rows (the same first rows for every M) scaled by 1 + m / M."""
    return (_x_base(K)[:M] * (1.0 + torch.arange(M, dtype=torch.float32) / M)[:, None]).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def make_w(N, K, gain=0.05):
    """W [N, K] bf16 row-major, row n (output column n) scaled by linspace(0.5, 2)[n].  Cached: callers must not modify it."""
    return (torch.randn(N, K, generator=_gen(7 * N + K)) * torch.linspace(0.5, 2.0, N)[:, None] * gain).to(torch.bfloat16)


SWIGLU_GAIN = 0.02                  # gate pre-activations of a few units: the SiLU is neither the identity nor zero


# ------------------------------------------------------------------------------------------------------------------------------ references
def slab_refs(x, W, S):
    """[S, M, N] float64."""
    K = x.shape[1]
    assert K % S == 0
    x64, W64, kc = x.to(F64), W.to(F64), K // S
    return torch.stack([x64[:, s * kc:(s + 1) * kc] @ W64[:, s * kc:(s + 1) * kc].t() for s in range(S)])


def full_ref(x, W):
    return x.to(F64) @ W.to(F64).t()


def interleave_rows(wg, wu):
    """[8 gate | 8 up] rows per 16 (one MFMA n-tile), as pg_load_tensor lays the decode copy of gate|up out."""
    I, K = wg.shape
    return torch.stack([wg.reshape(I // 8, 8, K), wu.reshape(I // 8, 8, K)], dim=1).reshape(2 * I, K)


def deinterleave_cols(y):
    """y [M, 2 I] in [8 gate | 8 up] column order -> (g [M, I], u [M, I])."""
    M, N = y.shape
    t = y.reshape(M, N // 16, 2, 8)
    return t[:, :, 0].reshape(M, N // 2), t[:, :, 1].reshape(M, N // 2)


def swiglu_ref(x, W):
    """[M, N / 2] float64: silu(g) u of the whole product's de-interleaved columns."""
    g, u = deinterleave_cols(full_ref(x, W))
    return g * torch.sigmoid(g) * u


# ------------------------------------------------------------------------------------------------------------------------------ comparators
def _where(bad):
    """Forensics of a failure: the rows and 16-column tiles that are off (as test_skinny_gemm_on_tiled_decode_weights reports them)."""
    idx = bad.nonzero()
    return {"n": int(idx.shape[0]), "rows": sorted(set(idx[:, -2].tolist()))[:16], "n_tiles": sorted(set((idx[:, -1] // 16).tolist()))[:16]}


def check_slabs(out, ref):
    """out [S, M, N] fp32 against ref [S, M, N] float64: every slab, then the sum of the slabs against the sum of the reference's.  Returns
    {"ok", "worst" (max err / tol over the slabs and the sum; inf for a non-finite element), "where"}."""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    o = out.to(F64)
    worst, where = 0.0, None
    parts = [(f"slab {s}", o[s], ref[s]) for s in range(ref.shape[0])] + [("sum of slabs", o.sum(0), ref.sum(0))]
    for tag, a, b in parts:
        tol = SLAB_RTOL * float(b.abs().max()) + SLAB_ATOL
        d = (a - b).abs()
        bad = ~(d <= tol)                                           # NaN (an element never written) is bad
        if bool(bad.any()):
            r = float("inf") if not bool(torch.isfinite(a).all()) else float(d.max()) / tol
            if where is None:
                where = dict(_where(bad), part=tag, tol=tol)
        else:
            r = float(d.max()) / tol
        worst = max(worst, r)
    return {"ok": where is None, "worst": worst, "where": where}


def check_swiglu(h, ref):
    """h [M, I] bf16 against ref [M, I] float64, elementwise."""
    assert h.shape == ref.shape, (h.shape, ref.shape)
    a = h.to(F64)
    bound = SWIGLU_RTOL * ref.abs() + SWIGLU_ATOL * float(ref.abs().max())
    d = (a - ref).abs()
    bad = ~(d <= bound)
    if bool(bad.any()):
        worst = float("inf") if not bool(torch.isfinite(a).all()) else float((d / bound).max())
        return {"ok": False, "worst": worst, "where": _where(bad)}
    return {"ok": True, "worst": float((d / bound).max()), "where": None}


def agree(a, b, ref):
    """Two results of one shape (other kernel forms) against each other, slab by slab within the slab tolerance; max diff / tol."""
    worst = 0.0
    for s in range(ref.shape[0]):
        tol = SLAB_RTOL * float(ref[s].abs().max()) + SLAB_ATOL
        d = (a[s].to(F64) - b[s].to(F64)).abs()
        worst = max(worst, float("inf") if not bool(torch.isfinite(d).all()) else float(d.max()) / tol)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------ planted errors
def mutate(ref, kind, x, W):
    """The reference with one error a kernel of this family could make (ref [S, M, N], M >= 47, S >= 2).  A kernel with that bug differs from the
    true reference by what the mutant differs from it."""
    S, M, N = ref.shape
    r = ref.clone()
    if kind == "chunk_dropped":          # rows 12-15 of an m-tile lose one 128-wide K chunk of one split (the sk4_store_direct signature)
        s, kc = S - 1, x.shape[1] // S
        k0 = s * kc + (kc // SK_BK - 1) * SK_BK
        r[s, 12:16] -= x[12:16, k0:k0 + SK_BK].to(F64) @ W[:, k0:k0 + SK_BK].to(F64).t()
    elif kind == "rows_swapped":         # row M - 1 clamped one short / two rows exchanged
        r[:, [45, 46]] = r[:, [46, 45]]
    elif kind == "slabs_exchanged":      # out + split M N with the wrong split: the sum of the slabs cannot see it
        r[[0, 1]] = r[[1, 0]]
    elif kind == "tile_shifted":         # one 16-column n-tile stored 4 columns off
        t = (N // 16) // 2
        r[:, :, t * 16:(t + 1) * 16] = torch.roll(r[:, :, t * 16:(t + 1) * 16], 4, dims=-1)
    else:
        raise ValueError(kind)
    return r


MUTATIONS = ("chunk_dropped", "rows_swapped", "slabs_exchanged", "tile_shifted")
