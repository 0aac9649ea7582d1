"""ctypes bindings of the attention operator entry points of libplangen_diag.so (plangen_amd/csrc/diag_ops.hip) for the attention tests:
each call runs the PRODUCTION launcher of one kernel form on device tensors and raises on a non-zero status."""
from __future__ import annotations

import ctypes as C

import torch

from attn_ref import TORCH_T

_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
_SIGS = {
    "pg_diag_op_attn_decode": [_I, _I, _I, _P, _I, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P, _P],
    "pg_diag_op_attn_prefill": [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P],
    "pg_diag_op_attn_vit": [_I, _P, _P, _P, _I, _I, _I, _I, _F, _P],
}


def lib():
    from plangen_amd import _lib
    d = _lib.load_diag()
    for name, args in _SIGS.items():
        fn = getattr(d, name)
        fn.restype, fn.argtypes = C.c_int, args
    return d


def _ptr(t, elem_off=0):
    return None if t is None else t.data_ptr() + elem_off * t.element_size()


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class DecodeDev:
    """Device copy of a decode case (attn_ref.make_decode_case): pristine caches kept for the byte-for-byte comparison and per-launch reset."""

    def __init__(self, d, dev="cuda"):
        self.d = d
        self.kc0, self.vc0 = d["kc"].to(dev), d["vc"].to(dev)
        self.kc, self.vc = self.kc0.clone(), self.vc0.clone()
        self.qkv = d["qkv"].to(dev)
        self.cos, self.sin = d["cos"].to(dev), d["sin"].to(dev)
        self.len = _i32(d["len"], dev)
        self.pos_off = _i32(d["pos_off"], dev)
        self.n_dec = _i32([d["n_dec"]], dev)
        self.order = None if d["row_order"] is None else _i32(d["row_order"], dev)
        self.obuf = torch.empty(d["M"], d["nh"] * 128, dtype=TORCH_T[d["dtype"]], device=dev)

    def run(self, form, path):
        d = self.d
        self.kc.copy_(self.kc0)
        self.vc.copy_(self.vc0)
        self.obuf.fill_(float("nan"))
        r0, nh, slots = d["r0"], d["nh"], d["slots"]
        cache_off = r0 * nh * slots * 128                   # the two-lane form: caches rebased by r0 rows, shared_row = 1 - r0 (< 0 when r0 > 1)
        shared_row = d["shared_row_abs"] - r0
        rc = lib().pg_diag_op_attn_decode(int(d["dtype"] == "bf16"), form, path, _ptr(self.qkv), d["S"], d["M"] * 3 * nh * 128,
                                          _ptr(self.obuf), _ptr(self.kc, cache_off), _ptr(self.vc, cache_off), _ptr(self.cos), _ptr(self.sin),
                                          _ptr(self.len), _ptr(self.pos_off), _ptr(self.n_dec), _ptr(self.order), d["shared_len"], shared_row,
                                          d["M"], nh, slots, d["max_pos"], d["scale"], None, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return self.obuf.cpu(), self.kc.cpu(), self.vc.cpu()


def run_prefill(p, path, obuf_pad=64, dev="cuda"):
    """Returns (obuf [Ntok, nh, 128], obuf rows past Ntok (must still hold their fill), the fill, kc, vc after the launch)."""
    T = TORCH_T[p["dtype"]]
    nh = p["nh"]
    q = p["q"].reshape(p["Ntok"], nh * 128).to(dev)
    kc, vc = p["kc"].to(dev), p["vc"].to(dev)
    fill = torch.full((obuf_pad, nh * 128), 77.0, dtype=T)
    obuf = torch.empty(p["Ntok"] + obuf_pad, nh * 128, dtype=T, device=dev)
    obuf[:p["Ntok"]] = float("nan")
    obuf[p["Ntok"]:] = fill.to(dev)
    row_off, ln = _i32(p["row_off"], dev), _i32(p["len"], dev)
    tr, tj = _i32(p["tok_row"], dev), _i32(p["tok_j"], dev)
    rc = lib().pg_diag_op_attn_prefill(int(p["dtype"] == "bf16"), path, _ptr(q), _ptr(obuf), _ptr(kc), _ptr(vc), _ptr(row_off), _ptr(ln),
                                       _ptr(tr), _ptr(tj), p["R"], p["max_len"], p["Ntok"], nh, p["slots"], p["scale"], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = obuf.cpu()
    return o[:p["Ntok"]].view(p["Ntok"], nh, 128), o[p["Ntok"]:], fill, kc.cpu(), vc.cpu()


def run_vit(v, form, dev="cuda"):
    qk, vt = v["qk"].to(dev), v["vt"].to(dev)
    o = torch.full((v["B"] * v["P"], v["C"]), float("nan"), dtype=torch.bfloat16, device=dev)
    rc = lib().pg_diag_op_attn_vit(form, _ptr(qk), _ptr(vt), _ptr(o), v["B"], v["P"], v["C"], v["NH"], v["scale"], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return o.cpu()
