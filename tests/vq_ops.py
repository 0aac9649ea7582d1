"""ctypes bindings of the VQ-decoder operator entry points of libplangen_diag.so (plangen_amd/csrc/diag_ops.hip) for tests/test_gpu_vq_ops.py: each call runs
the PRODUCTION launcher on device tensors and synchronises.  Every output lives inside a larger allocation with a guard band of BAND elements on either side,
filled with a bit pattern that must come back bit for bit; the valid part is pre-filled with NaN (a slot the kernel skips surfaces); the workspace of the
GroupNorm partial sums is pre-filled with 0xff bytes (NaN), its tail behind the slots the kernel owns included."""
from __future__ import annotations

import ctypes as C

import torch

PG_OK, PG_ERR_ARG = 0, -1
BAND = 4096
WS_TAIL = 256                       # floats behind the partial sums
PATTERN = {torch.float32: 0x7B3C5A17, torch.bfloat16: 0x5A17, torch.int32: 0x7B3C5A17}

_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
_SIGS = {
    "pg_diag_op_conv3x3": [_I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P, _F, _P, _P],
    "pg_diag_op_groupnorm": [_I, _I, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _F, _P],
    "pg_diag_op_gn_stats_raw": [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "pg_diag_op_softmax_rows": [_I, _P, _P, _I, _I, _F, _P],
    "pg_diag_op_gemm_epi": [_I, _I, _P, _L, _L, _P, _L, _L, _P, _I, _L, _L, _P, _P, _P, _I, _L, _L, _F, _I, _I, _I, _I, _I, _I, _P, _L, _P, _F, _P, _P],
    "pg_diag_op_gemm_epi256": [_I, _P, _L, _L, _P, _L, _L, _P, _I, _L, _L, _P, _P, _P, _I, _L, _L, _F, _I, _I, _I, _I, _I, _P, _P],
    "pg_diag_op_conv_out": [_I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "pg_diag_op_vq_gather": [_I, _P, _P, _P, _I, _I, _I, _P],
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


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def tdt(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float32


class Banded:
    """numel elements of dtype between two guard bands.  .t: the valid part (a view); .intact(): both bands still hold the pattern."""

    def __init__(self, numel, dtype, dev="cuda", fill=float("nan")):
        self.n = numel
        self.buf = torch.empty(numel + 2 * BAND, dtype=dtype, device=dev)
        pat = PATTERN[dtype]
        _bits(self.buf).fill_(pat - (1 << 16) if dtype == torch.bfloat16 and pat >= (1 << 15) else pat)
        self.t = self.buf[BAND:BAND + numel]
        self.t.fill_(fill)
        self.want = _bits(self.buf)[0].item()

    def intact(self):
        b = _bits(self.buf)
        return bool((b[:BAND] == self.want).all() and (b[BAND + self.n:] == self.want).all())


class Workspace:
    """floats fp32, every byte 0xff (NaN); the kernel owns the first `used` of them.  tail_intact(used): nothing behind them was written."""

    def __init__(self, floats, dev="cuda"):
        self.n = floats + WS_TAIL
        self.buf = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.buf.view(torch.int32).fill_(-1)

    def tail_intact(self, used):
        return bool((self.buf.view(torch.int32)[used:] == -1).all())

    def used_all_written(self, used):
        return not bool(torch.isnan(self.buf[:used]).any())


def run_conv3x3(x, w_oihw, bias, residual, out_kind, res_kind, up, stride2, want_gn, form, engine="bf16", dev="cuda", expect=PG_OK):
    """x NHWC fp32 values, w OIHW, residual NHWC or None.  Returns dict(rc, out (CPU, stored type), nsplit, stats (CPU [B, 32, 2] or None), guards)."""
    T = tdt(engine)
    B, Hi, Wi, Cin = x.shape
    Cout = w_oihw.shape[0]
    Ho, Wo = (Hi // 2, Wi // 2) if stride2 else (Hi << up, Wi << up)
    xd = x.to(dev, T).contiguous()
    wd = w_oihw.permute(0, 2, 3, 1).reshape(Cout, 9, Cin).to(dev, T).contiguous()            # [Cout][tap][Cin], as Engine.op_conv3x3
    bd = bias.to(dev, torch.float32)
    rd = None if residual is None else residual.to(dev, torch.float32 if res_kind == "f32" else T).contiguous()
    out = Banded(B * Ho * Wo * Cout, torch.float32 if out_kind == "f32" else T, dev)
    need = B * max((Ho // 8) * (Wo // 32), Ho * Wo // 64, 1) * 64
    ws = Workspace(need, dev)
    stats = Banded(B * 64, torch.float32, dev)
    nsp = C.c_int(-7)
    rc = lib().pg_diag_op_conv3x3(int(engine == "bf16"), form, _ptr(xd), _ptr(wd), _ptr(bd), _ptr(rd), _ptr(out.t), int(out_kind == "f32"),
                                  int(res_kind == "f32"), B, Hi, Wi, Cin, Cout, up, stride2, int(want_gn), _ptr(ws.buf), need, _ptr(stats.t), 1e-6,
                                  C.addressof(nsp), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    n = nsp.value
    used = B * n * 64 if rc == PG_OK and n > 0 else 0
    return dict(rc=rc, out=out.t.view(B, Ho, Wo, Cout).cpu(), nsplit=n, stats=stats.t.view(B, 32, 2).cpu() if used else None,
                guards=out.intact() and stats.intact() and ws.tail_intact(used) and ws.used_all_written(used),
                untouched=bool(torch.isnan(out.t.float()).all()))


def run_groupnorm(x, gamma, beta, in_kind, out_kind, swishes=(0, 1), eps=1e-6, dev="cuda"):
    """x [B, HW, C].  One upload; returns {swish: dict(out, stats [B, 32, 2], coef [B, C, 2], guards)} (CPU tensors)."""
    B, HW, Cc = x.shape
    xd = x.to(dev, tdt(in_kind)).contiguous()
    gd, bd = gamma.to(dev), beta.to(dev)
    nsplit = max(1, min(256, (HW + 63) // 64))
    res = {}
    for sw in swishes:
        out = Banded(B * HW * Cc, tdt(out_kind), dev)
        stats, coef = Banded(B * 64, torch.float32, dev), Banded(B * Cc * 2, torch.float32, dev)
        ws = Workspace(B * nsplit * 64, dev)
        rc = lib().pg_diag_op_groupnorm(int(in_kind == "bf16"), int(out_kind == "bf16"), _ptr(xd), _ptr(gd), _ptr(bd), _ptr(out.t), _ptr(stats.t), _ptr(coef.t),
                                        _ptr(ws.buf), B * nsplit * 64, B, HW, Cc, sw, eps, _stream())
        torch.cuda.synchronize()
        assert rc == PG_OK, rc
        res[sw] = dict(out=out.t.view(B, HW, Cc).cpu(), stats=stats.t.view(B, 32, 2).cpu(), coef=coef.t.view(B, Cc, 2).cpu(),
                       guards=out.intact() and stats.intact() and coef.intact() and ws.tail_intact(B * nsplit * 64) and ws.used_all_written(B * nsplit * 64))
    return res


def groupnorm_status(in_kind, out_kind, B, HW, Cc, raw=False, dev="cuda"):
    """(status, stats untouched) of the entry point (raw: of launch_gn_stats itself) on a shape the contract may exclude; buffers sized as if it ran."""
    n = max(B, 1) * max(HW, 1) * max(Cc, 32)
    xd = torch.ones(n + 64, dtype=tdt(in_kind), device=dev)
    gd = torch.ones(max(Cc, 32) + 64, device=dev)
    out = torch.zeros(n + 64, dtype=tdt(out_kind), device=dev)
    stats, coef = Banded(max(B, 1) * 64, torch.float32, dev), Banded(max(B, 1) * max(Cc, 32) * 2, torch.float32, dev)
    wsn = max(B, 1) * 256 * 64
    ws = torch.zeros(wsn, device=dev)
    if raw:
        rc = lib().pg_diag_op_gn_stats_raw(int(in_kind == "bf16"), _ptr(xd), _ptr(gd), _ptr(gd), _ptr(stats.t), _ptr(coef.t), _ptr(ws), B, HW, Cc, _stream())
    else:
        rc = lib().pg_diag_op_groupnorm(int(in_kind == "bf16"), int(out_kind == "bf16"), _ptr(xd), _ptr(gd), _ptr(gd), _ptr(out), _ptr(stats.t), _ptr(coef.t),
                                        _ptr(ws), wsn, B, HW, Cc, 0, 1e-6, _stream())
    torch.cuda.synchronize()
    return rc, bool(torch.isnan(stats.t).all() and torch.isnan(coef.t).all() and stats.intact() and coef.intact())


def run_softmax(x, scale, out_kind, dev="cuda"):
    """x fp32 [rows, n] -> (y CPU, guards): the band behind the last row is the rows past `rows` (a block covers four)."""
    rows, n = x.shape
    xd = torch.full((rows + 4, n), float("nan"), device=dev)
    xd[:rows] = x.to(dev)
    y = Banded(rows * n, tdt(out_kind), dev)
    rc = lib().pg_diag_op_softmax_rows(int(out_kind == "bf16"), _ptr(xd), _ptr(y.t), rows, n, scale, _stream())
    torch.cuda.synchronize()
    assert rc == PG_OK, rc
    return y.t.view(rows, n).cpu(), y.intact()


def run_gemm_epi(A, W, out_kind, M, N, K, batch, lda, strideA, ldb, strideB, ldc, strideC, bias_n=None, bias_m=None, residual=None, res_kind="f32", ldr=0,
                 strideR=0, scale=1.0, act=0, gn_hw=0, form=1, engine="bf16", dev="cuda", expect=PG_OK, inplace=False, opt=None, dev_out=False):
    """A, W: flat or shaped tensors holding the operands in the layout the strides describe.  Returns dict(rc, out [batch, M, N] CPU (rows ldc apart are
    compacted), nsplit, stats, guards, gaps: the elements between rows / batches (ldc > N) still NaN, untouched: the whole output still NaN).  inplace: the fp32
    residual [batch, M, N] is laid into the output buffer itself and the kernel is handed ONE pointer as out and residual (pg_engine::lin's x += proj(o)); fp32
    output, ldr / strideR as the output's.  opt: form 2 through pg_diag_op_gemm_epi256 with pg_tune->gemm256 = opt (tile height / phase count pinned; no GroupNorm
    partials).  dev_out: ``out`` stays on the device (a compacted copy).  Operands already on the device in the right type are used where they lie."""
    T = tdt(engine)
    Ad, Wd = A.to(dev, T).contiguous(), W.to(dev, T).contiguous()
    bn = None if bias_n is None else bias_n.to(dev, torch.float32)
    bm = None if bias_m is None else bias_m.to(dev, torch.float32)
    rd = None if residual is None else residual.to(dev, torch.float32 if res_kind == "f32" else T).contiguous()
    numel = (batch - 1) * strideC + (M - 1) * ldc + N
    out = Banded(numel, torch.float32 if out_kind == "f32" else T, dev)
    if inplace:
        assert residual is not None and out_kind == "f32" and res_kind == "f32" and ldr in (0, ldc) and strideR == strideC
        torch.as_strided(out.t, (batch, M, N), (strideC, ldc, 1)).copy_(residual.reshape(batch, M, N).to(dev, torch.float32))
        rd = out.t
    need = (M // gn_hw) * ((gn_hw + 63) // 64) * 64 if gn_hw else 64
    ws = Workspace(need, dev)
    nb = M // gn_hw if gn_hw else 1
    stats = Banded(nb * 64, torch.float32, dev)
    nsp = C.c_int(-7)
    if opt is None:
        rc = lib().pg_diag_op_gemm_epi(int(engine == "bf16"), form, _ptr(Ad), lda, strideA, _ptr(Wd), ldb, strideB, _ptr(out.t), int(out_kind == "f32"), ldc, strideC,
                                       _ptr(bn), _ptr(bm), _ptr(rd), int(res_kind == "f32"), ldr, strideR, scale, act, M, N, K, batch, gn_hw, _ptr(ws.buf), need,
                                       _ptr(stats.t), 1e-6, C.addressof(nsp), _stream())
    else:
        assert form == 2 and engine == "bf16" and not gn_hw
        rc = lib().pg_diag_op_gemm_epi256(opt, _ptr(Ad), lda, strideA, _ptr(Wd), ldb, strideB, _ptr(out.t), int(out_kind == "f32"), ldc, strideC, _ptr(bn), _ptr(bm),
                                          _ptr(rd), int(res_kind == "f32"), ldr, strideR, scale, act, M, N, K, batch, C.addressof(nsp), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    n = nsp.value
    used = nb * n * 64 if rc == PG_OK and n > 0 else 0
    view = torch.as_strided(out.t, (batch, M, N), (strideC, ldc, 1))
    gaps = True
    if numel > batch * M * N:
        own = torch.zeros(numel, dtype=torch.bool, device=dev)
        torch.as_strided(own, (batch, M, N), (strideC, ldc, 1)).fill_(True)
        gaps = bool(torch.isnan(out.t[~own].float()).all())
    return dict(rc=rc, out=view.contiguous() if dev_out else view.cpu(), nsplit=n, stats=stats.t.view(nb, 32, 2).cpu() if used else None,
                guards=out.intact() and stats.intact() and ws.tail_intact(used) and ws.used_all_written(used), gaps=gaps,
                untouched=rc != PG_OK and bool(torch.isnan(out.t.float()).all()))


def run_conv_out(x, w_oihw, bias, out_kind, form, coef=None, swish=1, engine="bf16", dev="cuda", expect=PG_OK):
    """x NHWC: the operand (T) for forms 1-3, the fp32 skip tensor for form 4 (with coef [B, Cin, 2]).  Returns dict(rc, out NCHW CPU, guards, untouched)."""
    T = tdt(engine)
    B, H, W, Cin = x.shape
    Cout = w_oihw.shape[0]
    xd = x.to(dev, torch.float32 if form == 4 else T).contiguous()
    wd = w_oihw.permute(0, 2, 3, 1).reshape(Cout, 9, Cin).to(dev, T).contiguous()
    bd = bias.to(dev, torch.float32)
    cd = None if coef is None else coef.to(dev, torch.float32).contiguous()
    out = Banded(B * Cout * H * W, tdt(out_kind), dev)
    rc = lib().pg_diag_op_conv_out(int(engine == "bf16"), form, _ptr(xd), _ptr(cd), _ptr(wd), _ptr(bd), _ptr(out.t), int(out_kind == "bf16"), B, H, W, Cin, Cout,
                                   swish, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return dict(rc=rc, out=out.t.view(B, Cout, H, W).cpu(), guards=out.intact(), untouched=bool(torch.isnan(out.t.float()).all()))


def run_vq_gather(table, codes, kind, dev="cuda"):
    """table [vocab, C], codes int32 [n] -> (out CPU [n, C], guards).  The table sits between NaN rows: an unclamped code reads them."""
    vocab, Cc = table.shape
    T = tdt(kind)
    td = torch.full((vocab + 8, Cc), float("nan"), dtype=T, device=dev)
    td[4:4 + vocab] = table.to(dev, T)
    cd = codes.to(dev, torch.int32)
    out = Banded(codes.numel() * Cc, T, dev)
    rc = lib().pg_diag_op_vq_gather(int(kind == "bf16"), td[4:].data_ptr(), _ptr(cd), _ptr(out.t), codes.numel(), Cc, vocab, _stream())
    torch.cuda.synchronize()
    assert rc == PG_OK, rc
    return out.t.view(codes.numel(), Cc).cpu(), out.intact()
