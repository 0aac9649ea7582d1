"""ctypes binding of pg_diag_op_gemm_skinny (libplangen_diag.so, plangen_amd/csrc/diag_ops.hip) for tests/test_gpu_skinny_ops.py: each call runs the
PRODUCTION decode GEMM launchers on device tensors.  x carries GUARD NaN rows behind row M - 1 and the row-major W NaN rows behind row N - 1 (the
kernels clamp their loads to the last valid row: a load past it poisons the result); the output is a 16-byte aligned interior view of a larger
tensor, NaN where the kernel must write, with GUARD canary rows in front of slab 0 and behind the last slab."""
from __future__ import annotations

import ctypes as C
import functools

import torch

import skinny_ref as R

PG_OK, PG_ERR_ARG = 0, -1
CANARY = 77.0
GUARD = R.GUARD

_P, _I = C.c_void_p, C.c_int
_SIG = [_I, _I, _P, _P, _P, _I, _I, _I, _I, _P]


def lib():
    from plangen_amd import _lib
    d = _lib.load_diag()
    d.pg_diag_op_gemm_skinny.restype, d.pg_diag_op_gemm_skinny.argtypes = C.c_int, _SIG
    return d


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_tail(t, dev):
    """t [rows, cols] bf16 -> device copy with GUARD NaN rows behind the last row."""
    d = torch.full((t.shape[0] + GUARD, t.shape[1]), float("nan"), dtype=torch.bfloat16, device=dev)
    d[:t.shape[0]] = t.to(dev)
    return d


@functools.lru_cache(maxsize=16)
def dev_w(N, K, gain=0.05, dev="cuda"):
    """(W [N, K] on the device, the same with NaN guard rows).  Cached: the weights of a shape are uploaded once."""
    wd = _nan_tail(R.make_w(N, K, gain), dev)
    return wd[:N], wd


class OutBuf:
    """[GUARD canary rows | rows valid rows | GUARD canary rows] x cols; the entry point gets the address of the first valid row."""

    def __init__(self, rows, cols, dtype, dev, fill=float("nan")):
        self.rows = rows
        self.t = torch.full((rows + 2 * GUARD, cols), CANARY, dtype=dtype, device=dev)
        self.t[GUARD:GUARD + rows] = fill
        self.ptr = self.t[GUARD].data_ptr()
        assert self.ptr % 16 == 0

    def valid(self):
        return self.t[GUARD:GUARD + self.rows]

    def guards_intact(self):
        return bool((self.t[:GUARD].float() == CANARY).all() and (self.t[GUARD + self.rows:].float() == CANARY).all())

    def untouched(self):
        return bool((self.t.float() == CANARY).all())


def run(form, mask, xd, wd, M, N, K, S):
    """xd / wd: device tensors WITH their NaN guard rows.  Returns (status, out, guards intact): out fp32 [S, M, N] (forms 0, 1) or bf16 [M, N / 2]
    (forms 2, 3), still on the device."""
    dev = xd.device
    buf = OutBuf(M, N // 2, torch.bfloat16, dev) if form >= 2 else OutBuf(S * M, N, torch.float32, dev)
    rc = lib().pg_diag_op_gemm_skinny(form, mask, xd.data_ptr(), wd.data_ptr(), buf.ptr, M, N, K, S, _stream())
    torch.cuda.synchronize()
    out = buf.valid()
    return rc, (out if form >= 2 else out.view(S, M, N)), buf.guards_intact()


def case(M, N, K, gain=0.05, dev="cuda"):
    """(x [M, K] on the device, W [N, K] on the device, x with guard rows, W with guard rows)."""
    xd = _nan_tail(R.make_x(M, K), dev)
    W, wd = dev_w(N, K, gain, dev)
    return xd[:M], W, xd, wd
