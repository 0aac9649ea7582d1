"""ctypes bindings of the decode-step operator entry points of libplangen_diag.so (plangen_amd/csrc/diag_ops.hip) for
tests/test_gpu_decode_ops.py: each call runs the PRODUCTION launcher on device tensors.  Every output buffer carries canary rows behind its last
valid row and is pre-filled with NaN where the kernel must write; every input the kernel may clamp into carries NaN rows behind row M - 1."""
from __future__ import annotations

import ctypes as C

import torch

from decode_ref import H

PG_OK, PG_ERR_ARG = 0, -1
CANARY = 77.0
GUARD = 3                           # rows behind the last valid one

_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
_SIGS = {
    "pg_diag_op_rmsnorm_defer": [_P, _P, _I, _L, _P, _P, _P, _I, _I, _P],
    "pg_diag_op_gemm_deferred": [_P, _P, _P, _I, _I, _I, _I, _P, _F, _I, _P],
    "pg_diag_op_slab_epilogue": [_I, _I, _P, _I, _L, _P, _P, _I, _I, _I, _P],
}


def lib():
    from plangen_amd import _lib
    d = _lib.load_diag()
    for name, args in _SIGS.items():
        fn = getattr(d, name)
        fn.restype, fn.argtypes = C.c_int, args
    return d


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(rows, cols, dtype, dev, fill=float("nan")):
    """[rows + GUARD, cols]: the valid rows hold `fill`, the guard rows the canary."""
    t = torch.full((rows + GUARD, cols), CANARY, dtype=dtype, device=dev)
    t[:rows] = fill
    return t


def guard_intact(t, rows):
    return bool((t[rows:].float() == CANARY).all())


def run_rmsnorm_defer(x, partial, w, dev="cuda"):
    """Returns (x_new [M, H] fp32, xw [M, H] bf16, ssq [M, 8] fp32, guards intact) on the CPU.  The slabs of partial are (M + GUARD) rows apart and
    their surplus rows hold NaN: a slab index or a row that leaves its slab poisons the result."""
    M, S = x.shape[0], partial.shape[0]
    xd = _guarded(M, H, torch.float32, dev)
    xd[:M] = x.to(dev)
    pd = torch.full((S, M + GUARD, H), float("nan"), dtype=torch.float32, device=dev)
    pd[:, :M] = partial.to(dev)
    wd = w.to(dev)
    xw = _guarded(M, H, torch.bfloat16, dev)
    ssq = _guarded(M, 8, torch.float32, dev)
    rc = lib().pg_diag_op_rmsnorm_defer(_ptr(xd), _ptr(pd), S, (M + GUARD) * H, _ptr(wd), _ptr(xw), _ptr(ssq), M, H, _stream())
    assert rc == PG_OK, rc
    torch.cuda.synchronize()
    ok = guard_intact(xd, M) and guard_intact(xw, M) and guard_intact(ssq, M)
    return xd[:M].cpu(), xw[:M].cpu(), ssq[:M].cpu(), ok


def rmsnorm_defer_status(M, Hh, S, slab, dev="cuda"):
    """Status of the entry point on a shape its contract may exclude; buffers sized for whatever it could touch if it did launch."""
    rows = max(M, 1) + GUARD
    xd = torch.zeros(rows, max(Hh, H), device=dev)
    pd = torch.zeros(8 * rows * max(Hh, H) + 8, device=dev)
    wd = torch.ones(max(Hh, H), dtype=torch.bfloat16, device=dev)
    xw = torch.full((rows, max(Hh, H)), CANARY, dtype=torch.bfloat16, device=dev)
    ssq = torch.full((rows, 8), CANARY, device=dev)
    rc = lib().pg_diag_op_rmsnorm_defer(_ptr(xd), _ptr(pd), S, slab, _ptr(wd), _ptr(xw), _ptr(ssq), M, Hh, _stream())
    torch.cuda.synchronize()
    return rc, bool((xw.float() == CANARY).all() and (ssq == CANARY).all())


def run_gemm_deferred(xw, ssq, W, S, eps, swiglu=False, dev="cuda"):
    """xw [M, K] bf16, ssq [M, 8] fp32, W [N, K] bf16 row-major ([8 gate | 8 up] interleaved rows for swiglu).  Returns (out, guard intact):
    out fp32 [S, M, N], or bf16 [M, N / 2] for swiglu.  xw and ssq carry NaN rows behind row M - 1 (the kernel clamps its loads to M - 1)."""
    M, K = xw.shape
    N = W.shape[0]
    xd = torch.full((M + GUARD, K), float("nan"), dtype=torch.bfloat16, device=dev)
    xd[:M] = xw.to(dev)
    sd = torch.full((M + GUARD, 8), float("nan"), dtype=torch.float32, device=dev)
    sd[:M] = ssq.to(dev)
    Wd = W.to(dev)
    if swiglu:
        out = _guarded(M, N // 2, torch.bfloat16, dev)
        valid = M
    else:
        out = _guarded(S * M, N, torch.float32, dev)
        valid = S * M
    rc = lib().pg_diag_op_gemm_deferred(_ptr(xd), _ptr(Wd), _ptr(out), M, N, K, S, _ptr(sd), eps, int(swiglu), _stream())
    assert rc == PG_OK, rc
    torch.cuda.synchronize()
    ok = guard_intact(out, valid)
    o = out[:valid].cpu()
    return (o if swiglu else o.view(S, M, N)), ok


def gemm_deferred_status(M, N, K, S, swiglu=False, dev="cuda"):
    """(status, out untouched) on a shape deferred_norm_ok may refuse."""
    xd = torch.ones(M + GUARD, K, dtype=torch.bfloat16, device=dev)
    sd = torch.ones(M + GUARD, 8, device=dev)
    Wd = torch.ones(N, K, dtype=torch.bfloat16, device=dev)
    out = torch.full((S * M + GUARD, N), CANARY, device=dev)
    rc = lib().pg_diag_op_gemm_deferred(_ptr(xd), _ptr(Wd), _ptr(out), M, N, K, S, _ptr(sd), 1e-6, int(swiglu), _stream())
    torch.cuda.synchronize()
    return rc, bool((out == CANARY).all())


def run_slab_epilogue(kind, dtype, partial, bias, act, dev="cuda"):
    """kind 0: partial [S, M, 2 I] -> [M, I] (silu_mul); kind 1: partial [S, M, N] (+ bias [N]) -> [M, N] (bias_act).  The slabs are (M + GUARD)
    rows apart with NaN surplus rows.  Returns (out on the CPU, guard intact)."""
    S, M, C_ = partial.shape
    N = C_ // 2 if kind == 0 else C_
    pd = torch.full((S, M + GUARD, C_), float("nan"), dtype=torch.float32, device=dev)
    pd[:, :M] = partial.to(dev)
    bd = None if bias is None else bias.to(dev)
    out = _guarded(M, N, torch.bfloat16 if dtype == "bf16" else torch.float32, dev)
    rc = lib().pg_diag_op_slab_epilogue(kind, int(dtype == "bf16"), _ptr(pd), S, (M + GUARD) * C_, _ptr(bd), _ptr(out), M, N, act, _stream())
    assert rc == PG_OK, rc
    torch.cuda.synchronize()
    return out[:M].cpu(), guard_intact(out, M)
