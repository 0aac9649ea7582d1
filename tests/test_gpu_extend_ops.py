"""GPU: the extension attention (pg_prefill_extend's) through pg_diag_op_attn_extend, which runs the production launchers -- path 2 =
attn_extend_flash_kernel (bf16), path 0 = attn_kernel mode 1 (bf16 / f32) -- against the fp64 reference of tests/extend_ref.py.

One packed launch per case: rows with q0 in {0, 1, 63, 64, 65, 127, 128, 200, 831} crossed with n_new in {1, 2, 31, 32, 33, 64, 127, 128, 129,
300} (extend_ref.Q0_NNEW, a covering subset) and one row with row_off = -1.  The bound is attn_ref.prefill_bound of the same path (the
extension kernels have the prefill kernels' rounding points), never a fitted one.  Slots past q0 + n_new and the row without packed tokens
hold the poison keys; obuf rows of no packed token and both caches must come back untouched; rows with q0 = 0 must be torch.equal to what
attn_prefill_flash2_kernel gives on the same buffers."""
import ctypes as C

import pytest
import torch

import attn_ref as A
import extend_ref as E

pytestmark = pytest.mark.gpu

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
_SIG = [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P]
_REFS = {}


def _case(dtype, nh, needle):
    """The case and its references, computed once per (dtype, nh, family) and never modified."""
    key = (dtype, nh, needle)
    if key not in _REFS:
        p = E.make_extend_case(700 + nh + 2 * needle + (dtype == "bf16"), dtype, nh, needle=needle)
        _REFS[key] = (p, E.extend_ref(p, dtype, flash=dtype == "bf16"))
    return _REFS[key]


def _run_extend(p, path, obuf_pad=64, dev="cuda"):
    from attn_ops import _i32, _ptr, _stream, lib
    d = lib()
    d.pg_diag_op_attn_extend.restype, d.pg_diag_op_attn_extend.argtypes = C.c_int, _SIG
    T = A.TORCH_T[p["dtype"]]
    nh = p["nh"]
    q = p["q"].reshape(p["Ntok"], nh * 128).to(dev)
    kc, vc = p["kc"].to(dev), p["vc"].to(dev)
    fill = torch.full((obuf_pad, nh * 128), 77.0, dtype=T)
    obuf = torch.empty(p["Ntok"] + obuf_pad, nh * 128, dtype=T, device=dev)
    obuf[:p["Ntok"]] = float("nan")
    obuf[p["Ntok"]:] = fill.to(dev)
    args = [_i32(p[k], dev) for k in ("row_off", "len", "n_new", "tok_row", "tok_j")]
    rc = d.pg_diag_op_attn_extend(int(p["dtype"] == "bf16"), path, _ptr(q), _ptr(obuf), _ptr(kc), _ptr(vc), *[_ptr(a) for a in args],
                                  p["R"], p["max_new"], p["Ntok"], nh, p["slots"], p["scale"], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = obuf.cpu()
    return o[:p["Ntok"]].view(p["Ntok"], nh, 128), o[p["Ntok"]:], fill, kc.cpu(), vc.cpu()


@pytest.mark.parametrize("needle", [False, True], ids=["random", "causal_needle"])
@pytest.mark.parametrize("nh", [2, 16])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_extend_packed_rows(dtype, nh, needle):
    p, ref = _case(dtype, nh, needle)
    for path in ([2, 0] if dtype == "bf16" else [0]):
        flash = path > 0
        out, tail, fill, kc, vc = _run_extend(p, path)
        ok, mx, worst = A.check(out, ref["out"], A.prefill_bound(ref, dtype, flash))
        print(f"extend path {path} {dtype} nh={nh} needle={needle}: max |err| / bound = {mx:.3g} (worst flat index {worst})")
        assert ok, f"extend path {path}: error {mx:.3g} x the bound at flat index {worst}"
        assert torch.equal(tail, fill), f"path {path}: obuf rows of no packed token were written"
        assert torch.equal(kc, p["kc"]) and torch.equal(vc, p["vc"]), f"path {path}: the caches changed"


@pytest.mark.parametrize("needle", [False, True], ids=["random", "causal_needle"])
@pytest.mark.parametrize("nh", [2, 16])
def test_q0_zero_rows_equal_flash2(nh, needle):
    """Same tile order, same arithmetic: with q0 = 0 the query-offset form gives the bits of attn_prefill_flash2_kernel."""
    from attn_ops import run_prefill
    p, _ = _case("bf16", nh, needle)
    ext = _run_extend(p, 2)[0]
    pre = run_prefill(E.as_prefill_case(p), 2)[0]
    n = 0
    for off, a, b in zip(p["row_off"], p["q0"], p["n_new"]):
        if off >= 0 and a == 0:
            n += 1
            assert torch.equal(ext[off:off + b], pre[off:off + b]), f"row at packed offset {off} ({b} tokens)"
    assert n == 3


def test_entry_point_refuses_inconsistent_rows():
    """The operator launches nothing when the packed token lists do not describe the rows (every kernel trusts them for its bounds)."""
    from attn_ops import _i32, _ptr, _stream, lib
    d = lib()
    d.pg_diag_op_attn_extend.restype, d.pg_diag_op_attn_extend.argtypes = C.c_int, _SIG
    p = E.make_extend_case(3, "bf16", 2, rows=[(5, 3), (0, 2)], aliased_row=None)
    dev = "cuda"
    q = p["q"].reshape(p["Ntok"], 256).to(dev)
    kc, vc = p["kc"].to(dev), p["vc"].to(dev)
    obuf = torch.zeros_like(q)

    def call(**over):
        v = dict(p, **over)
        arrs = [_i32(v[k], dev) for k in ("row_off", "len", "n_new", "tok_row", "tok_j")]
        return d.pg_diag_op_attn_extend(1, v.get("path", 2), _ptr(q), _ptr(obuf), _ptr(kc), _ptr(vc), *[_ptr(a) for a in arrs], v["R"], v["max_new"],
                                        v["Ntok"], 2, v["slots"], v["scale"], _stream())
    assert call() == 0
    assert call(len=[p["slots"] + 1, 2]) == -1                # a row longer than the cache
    assert call(n_new=[9, 2]) == -1                           # more new tokens than the row holds
    assert call(tok_j=[0, 1, 2, 0, 1]) == -1                  # slots that ignore q0
    assert call(path=1) == -1                                 # no 64-query form
    torch.cuda.synchronize()
