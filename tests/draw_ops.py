"""ctypes binding of pg_diag_op_cfg_sample / pg_diag_op_text_draw (libplangen_diag.so, plangen_amd/csrc/diag_ops.hip) for tests/test_gpu_draws.py: each call
runs the PRODUCTION sampler launchers on device tensors.  The slab buffer is NaN wherever no slab row lies (between slabs when the stride exceeds the rows, and
GUARD rows behind the last row of the last slab), the embedding table carries GUARD NaN rows behind row V - 1 -- a read past either poisons a result the tests
compare by value.  Every output is an interior view of a larger tensor with GUARD canary rows in front and behind."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

PG_OK, PG_ERR_ARG = 0, -1
GUARD = 4
CANARY = 77
UNSET = -99                     # out_tok / out entries the kernels must leave alone
H = 8                           # embedding width of the crafted tables (a multiple of 4: 16-byte rows)

_P, _I, _F, _L, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_uint64
_SIG_CFG = [_I, _P, _I, _L, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _F, _F, _U64, _I, _F, _I, _I, _I, _I, _I, _P]
_SIG_TXT = [_I, _P, _I, _L, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _U64, _I, _P]


def lib():
    from plangen_amd import _lib
    d = _lib.load_diag()
    d.pg_diag_op_cfg_sample.restype, d.pg_diag_op_cfg_sample.argtypes = C.c_int, _SIG_CFG
    d.pg_diag_op_text_draw.restype, d.pg_diag_op_text_draw.argtypes = C.c_int, _SIG_TXT
    return d


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class Guarded:
    """[GUARD canary rows | rows valid rows | GUARD canary rows] x cols; the entry point gets the address of the first valid row."""

    def __init__(self, rows, cols, dtype, fill, dev="cuda"):
        self.rows, self.fill = rows, fill
        self.t = torch.full((rows + 2 * GUARD, cols), CANARY, dtype=dtype, device=dev)
        self.t[GUARD:GUARD + rows] = fill
        self.ptr = self.t[GUARD].data_ptr()

    def valid(self):
        return self.t[GUARD:GUARD + self.rows]

    def guards_intact(self):
        return bool((self.t[:GUARD] == CANARY).all() and (self.t[GUARD + self.rows:] == CANARY).all())


def slabs_dev(slabs, slab=None, dev="cuda"):
    """slabs [S, R, V] float32 (numpy) -> (flat device tensor, slab stride in floats): slab s at s * slab; NaN everywhere else, GUARD NaN rows at the end."""
    S, R, V = slabs.shape
    slab = R * V if slab is None else int(slab)
    assert slab >= R * V
    flat = torch.full(((S - 1) * slab + (R + GUARD) * V,), float("nan"), dtype=torch.float32, device=dev)
    src = torch.from_numpy(np.ascontiguousarray(slabs)).to(dev)
    for s in range(S):
        flat[s * slab:s * slab + R * V] = src[s].reshape(-1)
    return flat, slab


@functools.lru_cache(maxsize=16)
def table(V, dev="cuda"):
    """Embedding table [V + GUARD, H]: row v holds v + j / 16 (a gathered row names its index), NaN guard rows behind row V - 1."""
    t = torch.full((V + GUARD, H), float("nan"), dtype=torch.float32, device=dev)
    t[:V] = torch.arange(V, dtype=torch.float32, device=dev)[:, None] + torch.arange(H, dtype=torch.float32, device=dev)[None, :] / 16
    return t


def table_row(v):
    return torch.tensor([v + j / 16 for j in range(H)], dtype=torch.float32)


TAP_STEPS = 4                   # the tap buffers hold steps [0, TAP_STEPS): later steps run without a tap


def cfg_sample(flat, S, slab, bias, V, B, w, temperature, seed, step, T=576, img_off=0, b_off=0, B_total=None, force=None, mask=None, filtered=0, top_k=0,
               top_p=1.0, tap=None):
    """One step of the image sampler.  flat / slab: slabs_dev's; bias: device [V] or None; force / mask: CPU [B_total, T] or None.  Returns a dict: rc, tok
    [B_total, T] (UNSET where nothing was written), x [2B, H], tap [B, V] or None (the rows [step][b_off : b_off + B]), ok (every canary and every tap row of
    another step / image intact)."""
    B_total = b_off + B if B_total is None else B_total
    tap = (step < TAP_STEPS) if tap is None else tap
    dev = flat.device
    out = Guarded(B_total, T, torch.int32, UNSET, dev)
    x = Guarded(2 * B, H, torch.float32, float("nan"), dev)
    lg = Guarded(TAP_STEPS * B_total, V, torch.float32, CANARY, dev) if tap else None
    ft = torch.as_tensor(force, dtype=torch.int32).to(dev).contiguous() if force is not None else None
    fm = torch.as_tensor(mask, dtype=torch.uint8).to(dev).contiguous() if mask is not None else None
    rc = lib().pg_diag_op_cfg_sample(int(filtered), flat.data_ptr(), S, slab, _ptr(bias), V, B, _ptr(ft), _ptr(fm), out.ptr, lg.ptr if tap else None,
                                     table(V).data_ptr(), x.ptr, H, float(w), float(temperature), int(seed), int(top_k), float(top_p), T, step, img_off, b_off,
                                     B_total, _stream())
    torch.cuda.synchronize()
    ok = out.guards_intact() and x.guards_intact()
    rows = None
    if tap and rc != PG_OK:
        ok = ok and bool((lg.t == CANARY).all())
    elif tap:
        v = lg.valid().view(TAP_STEPS, B_total, V)
        rows = v[step, b_off:b_off + B].cpu()
        other = torch.ones(TAP_STEPS, B_total, dtype=torch.bool, device=dev)
        other[step, b_off:b_off + B] = False
        ok = ok and lg.guards_intact() and bool((v[other] == CANARY).all())
    return dict(rc=rc, tok=out.valid().cpu(), x=x.valid().cpu(), tap=rows, ok=ok)


def text_draw(flat, S, slab, V, B, mode, temperature, seed, step, eos, min_new=0, max_new=4096, row_off=0, unfinished=None, tap=None):
    """One step of the text sampler (mode 0: launch_text_argmax, 1: launch_text_sample).  Returns a dict: rc, out [B, max_new] (UNSET where nothing was written),
    x [B, H], unfinished [B], tap [B, V] or None, ok."""
    tap = (step < TAP_STEPS) if tap is None else tap
    dev = flat.device
    out = Guarded(B, max_new, torch.int64, UNSET, dev)
    x = Guarded(B, H, torch.float32, float("nan"), dev)
    unf = Guarded(1, B, torch.int32, 1, dev)
    if unfinished is not None:
        unf.valid()[0] = torch.as_tensor(unfinished, dtype=torch.int32).to(dev)
    lg = Guarded(TAP_STEPS * B, V, torch.float32, CANARY, dev) if tap else None
    rc = lib().pg_diag_op_text_draw(mode, flat.data_ptr(), S, slab, V, B, out.ptr, unf.ptr, lg.ptr if tap else None, table(V).data_ptr(), x.ptr, H, eos, min_new,
                                    max_new, step, float(temperature), int(seed), row_off, _stream())
    torch.cuda.synchronize()
    ok = out.guards_intact() and x.guards_intact() and unf.guards_intact()
    rows = None
    if tap and rc != PG_OK:
        ok = ok and bool((lg.t == CANARY).all())
    elif tap:
        v = lg.valid().view(TAP_STEPS, B, V)
        rows = v[step].cpu()
        other = torch.ones(TAP_STEPS, dtype=torch.bool, device=dev)
        other[step] = False
        ok = ok and lg.guards_intact() and bool((v[other] == CANARY).all())
    return dict(rc=rc, out=out.valid().cpu(), x=x.valid().cpu(), unfinished=unf.valid()[0].cpu(), tap=rows, ok=ok)
