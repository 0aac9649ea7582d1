"""ctypes bindings of the weight-loading entry points of libplangen_diag.so (plangen_amd/csrc/diag_ops.hip: pg_diag_op_convert, pg_diag_op_rows;
diag_api.hip: pg_diag_read_weight) for tests/test_gpu_load_ops.py and tests/test_gpu_load_path.py.  Every destination is pre-filled with the sentinel bit
pattern of tests/load_ref.py and carries GUARD elements / rows of it on both sides; a call returns the written part and whether the guards are intact."""
from __future__ import annotations

import ctypes as C

import torch

import load_ref as R

PG_OK, PG_ERR_ARG, PG_ERR_HIP, PG_ERR_STATE, PG_ERR_NAME = 0, -1, -2, -3, -4
GUARD = 64                                                  # sentinel elements (convert) or rows (row movers) in front of and behind a destination

_P, _I, _L = C.c_void_p, C.c_int, C.c_long
_SIGS = {
    "pg_diag_op_convert": [_I, _I, _I, _P, _P, _L, _I, _I, _I, _I, C.POINTER(C.c_int), _P],
    "pg_diag_op_rows": [_I, _P, _P, _P, _I, _P, _P, _I, _L, _L, _L, _I, _I, _I, _I, _I, _I, _P],
    "pg_diag_read_weight": [_P, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int64)],
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


def _dev(t, dev="cuda"):
    return None if t is None else t.to(dev).contiguous()


def guarded(n, kind, dev="cuda"):
    """Sentinel-filled [GUARD + n + GUARD] destination; the payload starts GUARD elements in (16-byte aligned for both types)."""
    return R.sentinel_like((n + 2 * GUARD,), kind, dev)


def guards_intact(buf, n):
    torch.cuda.synchronize()
    return bool(R.is_sentinel(buf[:GUARD]).all()) and bool(R.is_sentinel(buf[GUARD + n:]).all())


def convert(src, dst_kind, kind=0, a=0, b=0, c=0, which=0, dst=None, n=None, src_off=0, dst_off=0, dev="cuda"):
    """pg_diag_op_convert on a host tensor ``src``: (status, payload [n] on the host, guards intact, kernel reported).  dst: an earlier call's guarded buffer
    (the second launch of an interleave pair); src_off / dst_off: byte offsets that misalign the pointers (the buffers are made that much larger)."""
    es_s, es_d = src.element_size(), 2 if dst_kind == "bf16" else 4
    n = src.numel() if n is None else n
    n_dst = 2 * src.numel() if kind == 2 else src.numel()
    flat = src.reshape(-1)
    s = torch.zeros(flat.numel() + 16, dtype=src.dtype, device=dev)
    so = src_off // es_s
    s[so:so + flat.numel()] = flat.to(dev)
    d = guarded(n_dst + 16, dst_kind, dev) if dst is None else dst
    k = C.c_int(-1)
    rc = lib().pg_diag_op_convert(kind, int(src.dtype == torch.bfloat16), int(dst_kind == "bf16"), _ptr(s, src_off), _ptr(d, GUARD * es_d + dst_off), n, a, b, c, which,
                                  C.byref(k), _stream())
    torch.cuda.synchronize()
    do = dst_off // es_d
    pay = d[GUARD + do:GUARD + do + n_dst]
    rest = torch.cat([d[:GUARD + do], d[GUARD + do + n_dst:]])
    return rc, pay.cpu(), bool(R.is_sentinel(rest).all()), k.value, d


def rows(op, src, dst_rows, width, dst_kind, n, ids=None, src_idx=None, dst_idx=None, src_rows=None, first=0, stride=1, ref=0, frm=0, dev="cuda", width_arg=None,
         src_off=0, dst_off=0):
    """pg_diag_op_rows: dst is a sentinel-filled [GUARD + dst_rows + GUARD, width] tensor of dst_kind.  Returns (status, dst rows [dst_rows, width] on the host,
    guards intact)."""
    s = _dev(src, dev)
    d = R.sentinel_like((dst_rows + 2 * GUARD, width), dst_kind, dev)
    es_d = d.element_size()
    i, si, di = _dev(ids, dev), _dev(src_idx, dev), _dev(dst_idx, dev)
    rc = lib().pg_diag_op_rows(op, _ptr(s, src_off), _ptr(d, GUARD * width * es_d + dst_off), _ptr(i), 0 if ids is None else ids.numel(), _ptr(si), _ptr(di), n,
                               width * (es_d if op == 1 else 1) if width_arg is None else width_arg, src.shape[0] if src_rows is None else src_rows, dst_rows,
                               int(src.dtype == torch.bfloat16), int(dst_kind == "bf16"), first, stride, ref, frm, _stream())
    torch.cuda.synchronize()
    ok = bool(R.is_sentinel(d[:GUARD]).all()) and bool(R.is_sentinel(d[GUARD + dst_rows:]).all())
    return rc, d[GUARD:GUARD + dst_rows].cpu(), ok


def rows_differ(ids, first, stride, ref, n, frm, dev="cuda", flag0=0):
    """launch_rows_differ on ids [rows, L]: (status, flag)."""
    i = _dev(ids, dev)
    flag = torch.full((4,), flag0, dtype=torch.int32, device=dev)
    rc = lib().pg_diag_op_rows(6, None, _ptr(flag), _ptr(i), ids.numel(), None, None, n, ids.shape[1], ids.shape[0], 1, 0, 0, first, stride, ref, frm, _stream())
    torch.cuda.synchronize()
    f = flag.cpu().tolist()
    assert f[1:] == [flag0] * 3
    return rc, f[0]


def read_weight(engine, name, dev="cuda"):
    """pg_diag_read_weight: (status, tensor in the device layout on the host or None, (elements, element size, kind))."""
    info = (C.c_int64 * 3)(0, 0, 0)
    probe = torch.zeros(16, dtype=torch.uint8, device=dev)
    rc = lib().pg_diag_read_weight(engine.h, name.encode(), _ptr(probe), 0, info)
    if rc != PG_OK:
        return rc, None, tuple(info)
    n, es, kind = tuple(info)
    dt = torch.float32 if es == 4 else torch.bfloat16
    out = R.sentinel_like((n + GUARD,), "f32" if es == 4 else "bf16", dev)
    rc = lib().pg_diag_read_weight(engine.h, name.encode(), _ptr(out), n * es, info)
    torch.cuda.synchronize()
    assert bool(R.is_sentinel(out[n:]).all()) and out.dtype == dt
    return rc, out[:n].cpu(), (n, es, kind)
