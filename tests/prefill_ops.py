"""ctypes bindings of the prefill operator entry points of libplangen_diag.so (plangen_amd/csrc/diag_ops.hip) for tests/test_gpu_prefill_ops.py: each
call runs the PRODUCTION launchers on device tensors.  Every output buffer (qbuf, both caches, h) is pre-filled with the sentinel bit pattern of
tests/prefill_ref.py and carries guard rows behind its last valid row; the token-map arrays carry 256 entries behind token M - 1 that point at a row
owning no token (a kernel that used them would write where the sentinel screen looks)."""
from __future__ import annotations

import ctypes as C

import torch

import prefill_ref as P

PG_OK, PG_ERR_ARG = 0, -1

_P, _I, _L = C.c_void_p, C.c_int, C.c_long
_SIGS = {
    "pg_diag_op_qkv_rope": [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "pg_diag_op_rope_kv": [_I, _I, _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "pg_diag_op_gemm_swiglu256": [_I, _I, _P, _P, _P, _I, _I, _I, _P],
    "pg_diag_op_interleave": [_I, _P, _P, _P, _I, _I, _P],
}


def lib():
    from plangen_amd import _lib
    d = _lib.load_diag()
    for name, args in _SIGS.items():
        fn = getattr(d, name)
        fn.restype, fn.argtypes = C.c_int, args
    return d


def _ptr(t, byte_off=0):
    return None if t is None else t.data_ptr() + byte_off


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i32(x, dev, pad=0, pad_value=0):
    return torch.tensor(list(x) + [pad_value] * pad, dtype=torch.int32, device=dev)


class _MapDev:
    """Device copy of a token map (prefill_ref.make_token_map / make_decode_map) and of the RoPE tables."""

    def __init__(self, case, dev):
        tm = self.tm = case["tm"]
        spare = tm.get("empty_row", tm["R"] - 1)
        self.tok_row = _i32(tm["tok_row"], dev, 256, spare)
        self.tok_j = _i32(tm["tok_j"], dev, 256, 0)
        self.pos_off = _i32(tm["pos_off"], dev)
        self.len = _i32(tm["len"], dev, 256, 0) if "len" in tm else None
        self.n_dec = _i32([tm["n_dec"]], dev) if "n_dec" in tm else None
        self.cos, self.sin = case["cos"].to(dev), case["sin"].to(dev)


class QkvDev:
    """Device copy of a fused-QKV case; run() returns freshly sentinel-filled (qbuf, kc, vc) after one launch, still on the device."""

    def __init__(self, case, ref, dev="cuda"):
        self.case, self.ref, self.dev = case, ref, dev
        self.xn, self.W = case["xn"].to(dev), case["W"].to(dev)
        self.map = _MapDev(case, dev)

    def call(self, form, opt, bufs, xn=None, tok_row=None, tok_j=None, M=None, K=None, qbuf_off=0):
        c, tm, m = self.case, self.case["tm"], self.map
        qb, kc, vc = bufs
        return lib().pg_diag_op_qkv_rope(form, opt, _ptr(self.xn if xn is None else xn), _ptr(self.W), _ptr(qb, qbuf_off), _ptr(kc), _ptr(vc), _ptr(m.cos),
                                         _ptr(m.sin), _ptr(m.tok_row if tok_row is None else tok_row), _ptr(m.tok_j if tok_j is None else tok_j),
                                         _ptr(m.pos_off), c["M"] if M is None else M, c["nh"], c["K"] if K is None else K, tm["R"], tm["slots"],
                                         tm["max_pos"], _stream())

    def run(self, form, opt):
        bufs = P.rope_buffers(self.ref, "bf16", self.dev)
        rc = self.call(form, opt, bufs)
        assert rc == PG_OK, (form, opt, rc)
        torch.cuda.synchronize()
        return bufs


def rope_kv_call(case, ref, dtype, edit=None, dev="cuda", **over):
    """launch_rope_kv<T> alone on a make_rope_case: the slabs are (M + GUARD) rows apart with NaN surplus rows.  edit(map): changes the device token
    map first; over: M / nh / S / slab / qbuf_off in place of the case's.  Returns (status, (qbuf, kc, vc))."""
    tm, M, nh, S = case["tm"], case["M"], case["nh"], case["S"]
    m = _MapDev(case, dev)
    if edit:
        edit(m)
    N = 3 * nh * 128
    qkv = torch.full((S, M + P.GUARD, N), float("nan"), dtype=torch.float32, device=dev)
    qkv[:, :M] = case["qkv"].to(dev)
    bufs = P.rope_buffers(ref, dtype, dev)
    rc = lib().pg_diag_op_rope_kv(int(dtype == "bf16"), case["mode"], _ptr(qkv), over.get("S", S), over.get("slab", (M + P.GUARD) * N),
                                  _ptr(bufs[0], over.get("qbuf_off", 0)), _ptr(bufs[1]), _ptr(bufs[2]), _ptr(m.cos), _ptr(m.sin), _ptr(m.len), _ptr(m.n_dec),
                                  _ptr(m.tok_row) if case["mode"] else None, _ptr(m.tok_j) if case["mode"] else None, _ptr(m.pos_off), over.get("M", M),
                                  over.get("nh", nh), tm["R"], tm["slots"], tm["max_pos"], _stream())
    torch.cuda.synchronize()
    return rc, bufs


def run_rope_kv(case, ref, dtype, dev="cuda"):
    rc, bufs = rope_kv_call(case, ref, dtype, dev=dev)
    assert rc == PG_OK, rc
    return bufs


class SwigluDev:
    def __init__(self, case, dev="cuda"):
        self.case, self.dev = case, dev
        self.xn, self.W = case["xn"].to(dev), case["W"].to(dev)

    def call(self, form, opt, h, M=None, I=None, K=None, h_off=0):
        c = self.case
        return lib().pg_diag_op_gemm_swiglu256(form, opt, _ptr(self.xn), _ptr(self.W), _ptr(h, h_off), c["M"] if M is None else M, c["I"] if I is None else I,
                                               c["K"] if K is None else K, _stream())

    def buffer(self):
        return P.sentinel_like((self.case["M"] + P.GUARD, self.case["I"]), "bf16", self.dev)

    def run(self, form, opt):
        h = self.buffer()
        rc = self.call(form, opt, h)
        assert rc == PG_OK, (form, opt, rc)
        torch.cuda.synchronize()
        return h


def run_interleave_qk(W, nh, dev="cuda"):
    """launch_interleave_qk on W bf16 [3 nh 128, K]: (copy, guard rows behind it still sentinel)."""
    N, K = W.shape
    src = W.to(dev)
    dst = P.sentinel_like((N + P.GUARD, K), "bf16", dev)
    rc = lib().pg_diag_op_interleave(0, _ptr(src), None, _ptr(dst), nh, K, _stream())
    assert rc == PG_OK, rc
    torch.cuda.synchronize()
    return dst[:N].cpu(), bool(P.is_sentinel(dst[N:]).all())


def run_interleave16(wg, wu, dev="cuda"):
    """launch_convert_interleave16<bf16> with which = 0 (gate) and 1 (up) into one destination [2 I, H]."""
    I, H = wg.shape
    a, b = wg.to(dev), wu.to(dev)
    dst = P.sentinel_like((2 * I + P.GUARD, H), "bf16", dev)
    rc = lib().pg_diag_op_interleave(1, _ptr(a), _ptr(b), _ptr(dst), I, H, _stream())
    assert rc == PG_OK, rc
    torch.cuda.synchronize()
    return dst[:2 * I].cpu(), bool(P.is_sentinel(dst[2 * I:]).all())


def untouched(*bufs):
    torch.cuda.synchronize()
    return all(bool(P.is_sentinel(b).all()) for b in bufs)
