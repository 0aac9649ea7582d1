"""ctypes bindings of the understanding path's operator entry points of libplangen_diag.so (plangen_amd/csrc/diag_ops.hip) for tests/test_gpu_vision_ops.py.
Guard bands, patterns and the NaN pre-fill as tests/vq_ops.py (imported from there); inputs a broken bounds test would read past are followed by NaN rows."""
from __future__ import annotations

import ctypes as C

import torch

from vq_ops import BAND, PG_ERR_ARG, PG_OK, Banded, Workspace, _bits, _ptr, _stream, tdt      # noqa: F401

_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
_SIGS = {
    "pg_diag_op_layernorm": [_I, _I, _P, _P, _P, _P, _I, _I, _F, _P],
    "pg_diag_op_patchify": [_I, _I, _P, _P, _I, _I, _I, _P],
    "pg_diag_op_add_pos": [_P, _P, _I, _I, _I, _P],
    "pg_diag_op_conv_in": [_I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "pg_diag_op_vq_argmin": [_I, _P, _P, _P, _I, _I, _I, _P],
    "pg_diag_op_l2norm_rows": [_P, _P, _I, _I, _P],
    "pg_diag_op_gemm_heads": [_I, _I, _P, _L, _L, _P, _L, _L, _P, _I, _L, _L, _P, _P, _P, _I, _L, _L, _F, _I, _I, _I, _I, _I, _I, _L, _L, _L, _I, _P, _L, _P, _F,
                              _P, _P],
}
I64_PATTERN = 0x5A175A175A175A17


def lib():
    from plangen_amd import _lib
    d = _lib.load_diag()
    for name, args in _SIGS.items():
        fn = getattr(d, name)
        fn.restype, fn.argtypes = C.c_int, args
    return d


def _padded_rows(t, extra, dtype, dev):
    """t [rows, n] on the device, followed by `extra` rows of NaN (what a kernel without its row bound would read)."""
    rows, n = t.shape
    d = torch.full((rows + extra, n), float("nan"), dtype=dtype, device=dev)
    d[:rows] = t.to(dev, dtype)
    return d


def run_layernorm(x, gamma, beta, form, out_kind, eps, dev="cuda", expect=PG_OK):
    """x fp32 [M, C] -> dict(rc, out CPU [M, C] in the stored type, guards, untouched)."""
    M, Cc = x.shape
    xd = _padded_rows(x, 4, torch.float32, dev)
    gd, bd = gamma.to(dev).contiguous(), beta.to(dev).contiguous()
    y = Banded(M * Cc, tdt(out_kind), dev)
    rc = lib().pg_diag_op_layernorm(int(out_kind == "bf16"), form, _ptr(xd), _ptr(gd), _ptr(bd), _ptr(y.t), M, Cc, eps, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return dict(rc=rc, out=y.t.view(M, Cc).cpu(), guards=y.intact(), untouched=bool(torch.isnan(y.t.float()).all()))


def run_patchify(img, ps, in_kind, out_kind, dev="cuda", expect=PG_OK):
    """img [B, 3, S, S] -> dict(rc, out CPU [B g g, 3 ps ps], guards, untouched)."""
    B, _, S, _ = img.shape
    g = S // ps
    d = img.to(dev, tdt(in_kind)).contiguous()
    out = Banded(B * g * g * 3 * ps * ps, tdt(out_kind), dev)
    rc = lib().pg_diag_op_patchify(int(in_kind == "bf16"), int(out_kind == "bf16"), _ptr(d), _ptr(out.t), B, S, ps, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return dict(rc=rc, out=out.t.view(B * g * g, 3 * ps * ps).cpu(), guards=out.intact(), untouched=bool(torch.isnan(out.t.float()).all()))


def run_add_pos(x, pos, B, dev="cuda"):
    """x fp32 [B P, C] += pos [P, C] in place inside guard bands -> (x CPU, guards)."""
    rows, Cc = x.shape
    buf = Banded(rows * Cc, torch.float32, dev)
    buf.t.copy_(x.reshape(-1).to(dev))
    pd = _padded_rows(pos, 2, torch.float32, dev)
    rc = lib().pg_diag_op_add_pos(_ptr(buf.t), _ptr(pd), B, pos.shape[0], Cc, _stream())
    torch.cuda.synchronize()
    assert rc == PG_OK, rc
    return buf.t.view(rows, Cc).cpu(), buf.intact()


def run_conv_in(x, w, bias, in_kind, out_kind, dev="cuda"):
    """x NCHW [B, 3, H, W], w [Cout, 3, 3, 3] -> (out CPU NHWC [B, H, W, Cout], guards)."""
    B, _, H, W = x.shape
    Cout = w.shape[0]
    xd = x.to(dev, tdt(in_kind)).contiguous()
    wd, bd = w.to(dev, torch.float32).contiguous(), bias.to(dev, torch.float32)
    out = Banded(B * H * W * Cout, tdt(out_kind), dev)
    rc = lib().pg_diag_op_conv_in(int(in_kind == "bf16"), int(out_kind == "bf16"), _ptr(xd), _ptr(wd), _ptr(bd), _ptr(out.t), B, H, W, Cout, _stream())
    torch.cuda.synchronize()
    assert rc == PG_OK, rc
    return out.t.view(B, H, W, Cout).cpu(), out.intact()


class BandedI64:
    """n int64 slots (pre-filled with -1) between two bands of I64_PATTERN."""

    def __init__(self, n, dev="cuda"):
        self.n = n
        self.buf = torch.full((n + 2 * 64,), I64_PATTERN, dtype=torch.int64, device=dev)
        self.t = self.buf[64:64 + n]
        self.t.fill_(-1)

    def intact(self):
        return bool((self.buf[:64] == I64_PATTERN).all() and (self.buf[64 + self.n:] == I64_PATTERN).all())


def run_vq_argmin(z, cb, form, dev="cuda", expect=PG_OK, D=None):
    """z fp32 [n, D], cb fp32 [V, D] -> dict(rc, idx CPU int64 [n], guards, untouched).  D: what the entry point is told (the refusal tests lie about it)."""
    n, V = z.shape[0], cb.shape[0]
    zd = _padded_rows(z, 8, torch.float32, dev)
    cd = _padded_rows(cb, 4, torch.float32, dev)
    idx = BandedI64(n, dev)
    rc = lib().pg_diag_op_vq_argmin(form, _ptr(zd), _ptr(cd), _ptr(idx.t), n, z.shape[1] if D is None else D, V, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return dict(rc=rc, idx=idx.t.cpu(), guards=idx.intact(), untouched=bool((idx.t == -1).all()))


def run_l2norm(x, dev="cuda"):
    n, D = x.shape
    xd = _padded_rows(x, 256, torch.float32, dev)
    out = Banded(n * D, torch.float32, dev)
    rc = lib().pg_diag_op_l2norm_rows(_ptr(xd), _ptr(out.t), n, D, _stream())
    torch.cuda.synchronize()
    assert rc == PG_OK, rc
    return out.t.view(n, D).cpu(), out.intact()


def run_gemm_heads(A, a_off, W, w_off, out_kind, M, N, K, batch, batch2, lda, strideA, strideA2, ldb, strideB, strideB2, ldc, strideC, strideC2, form=1,
                   engine="bf16", dev="cuda", expect=PG_OK):
    """A, W: tensors holding the operands in the layout the strides describe, read from element a_off / w_off on (W may be the same tensor as A: one upload).
    Returns dict(rc, out: the FLAT output buffer on the CPU ((batch - 1) strideC + (batch2 - 1) strideC2 + (M - 1) ldc + N elements, NaN where nothing was
    written), guards)."""
    T = tdt(engine)
    Ad = A.to(dev, T).contiguous()
    Wd = Ad if W is A else W.to(dev, T).contiguous()
    numel = (batch - 1) * strideC + (batch2 - 1) * strideC2 + (M - 1) * ldc + N
    out = Banded(numel, torch.float32 if out_kind == "f32" else T, dev)
    ws = Workspace(64, dev)
    nsp = C.c_int(-7)
    esz = Ad.element_size()
    rc = lib().pg_diag_op_gemm_heads(int(engine == "bf16"), form, Ad.data_ptr() + a_off * esz, lda, strideA, Wd.data_ptr() + w_off * esz, ldb, strideB, _ptr(out.t),
                                     int(out_kind == "f32"), ldc, strideC, None, None, None, 0, 0, 0, 1.0, 0, M, N, K, batch, batch2, strideA2, strideB2, strideC2,
                                     0, _ptr(ws.buf), 64, None, 1e-6, C.addressof(nsp), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return dict(rc=rc, out=out.t.cpu(), guards=out.intact() and ws.tail_intact(0), untouched=bool(torch.isnan(out.t.float()).all()))
