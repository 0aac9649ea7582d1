"""Operator tests of the LoRA merge kernel through its PRODUCTION launcher (launch_lora_merge<T>, what pg_merge_lora launches) by way of
libplangen_diag.so's pg_diag_op_lora_merge, against the host model tests/lora_ref.py::merge_ref -- BIT FOR BIT (load_ref.same_bits): the merge's arithmetic is
a contract (fp32 products and sums, each rounded on its own, k ascending, one store), so there is no tolerance anywhere in this file.

W sits in a sentinel-filled buffer with load_ops.GUARD sentinel elements on both sides; the guards must survive every call.  The kernel's tile is 32 rows x 128
columns with k in chunks of 32, a thread owns 8 consecutive columns and moves them as 16-byte vectors where their address allows: the shapes below cover one
block and several, ragged rows / columns / ranks, a rank below, at, across (40, 33) and at twice the chunk, rows whose 16-byte alignment holds (in % 8 == 0),
alternates (in = 130, bf16: every fourth row) or never holds for a whole vector (in = 13), and the interleaved [8 gate | 8 up] layout."""
import ctypes as C

import pytest
import torch

import load_ops as O
import load_ref as R
import lora_ref as L

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
K_T, K_IL16_G, K_IL16_U = R.K_T, R.K_IL16_G, R.K_IL16_U
SHAPES = [(256, 256), (72, 136), (8, 1000), (1, 8), (33, 130), (5, 13)]
RANKS = [1, 3, 16, 32, 33, 40, 64]                          # the kernel's k-chunk is 32


def _lib():
    d = O.lib()
    d.pg_diag_op_lora_merge.restype = C.c_int
    d.pg_diag_op_lora_merge.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    return d


def merge_op(buf_host, layout, out, n, A, B, scale):
    """pg_diag_op_lora_merge on a host tensor of W's buffer ([out, n], or [2 out, n] for the interleave): (status, buffer after the call on the host, guards
    intact).  A / B go to the device as fp32 (the launcher's interface; bf16 values are exact in it)."""
    kind = R.kind_of(buf_host)
    total = buf_host.numel()
    d = O.guarded(total, kind)
    d[O.GUARD:O.GUARD + total] = buf_host.reshape(-1).cuda()
    a, b = A.float().cuda().contiguous(), B.float().cuda().contiguous()
    rc = _lib().pg_diag_op_lora_merge(int(kind == "bf16"), layout, d.data_ptr() + O.GUARD * d.element_size(), out, n, a.data_ptr(), b.data_ptr(),
                                      A.shape[0], float(scale), torch.cuda.current_stream().cuda_stream)
    ok = O.guards_intact(d, total)
    return rc, d[O.GUARD:O.GUARD + total].cpu().reshape(buf_host.shape), ok


def _inputs(out, n, r, seed, kind, ab):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(out, n, generator=g) * 0.05).to(R.tdtype(kind))
    A = (torch.randn(r, n, generator=g) * 0.3).to(ab)
    B = (torch.randn(out, r, generator=g) * 0.3).to(ab)
    return W, A, B


@pytest.mark.parametrize("ab", [torch.float32, BF], ids=["ab_f32", "ab_bf16"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_row_major(kind, ab):
    for si, (out, n) in enumerate(SHAPES):
        for r in RANKS:
            W, A, B = _inputs(out, n, r, 1000 * si + r, kind, ab)
            scale = 16.0 / r
            rc, got, guards = merge_op(W, K_T, out, n, A, B, scale)
            assert rc == O.PG_OK and guards, (out, n, r, rc, guards)
            res = R.same_bits(got, L.merge_ref(W, A, B, scale, kind))
            assert res["ok"], (out, n, r, res)
            assert not R.same_bits(got, W)["ok"]                                  # and it did something


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_the_planted_defects_are_not_what_the_kernel_does(kind):
    """The kernel's output on the CPU test's defect inputs equals the model, so it differs from every defect there (tests/test_lora_ref_cpu.py shows that each
    defect moves bits on these inputs) -- the FMA one included: the compiler did not contract the products into the sums."""
    g = torch.Generator().manual_seed(13)
    W = (torch.randn(256, 256, generator=g) * 0.05).to(R.tdtype(kind))
    A, B = torch.randn(40, 256, generator=g) * 0.3, torch.randn(256, 40, generator=g) * 0.3
    rc, got, guards = merge_op(W, K_T, 256, 256, A, B, 1.0 / 3)
    assert rc == O.PG_OK and guards
    assert R.same_bits(got, L.merge_ref(W, A, B, 1.0 / 3, kind))["ok"]
    for fn in (L.defect_transposed, L.defect_scale_per_term, L.defect_fma, L.defect_dropped_last_k, L.defect_no_final_add):
        assert not R.same_bits(got, fn(W, A, B, 1.0 / 3, kind))["ok"], fn.__name__


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_interleaved_halves(kind):
    """Gate rows o -> 16 (o / 8) + o % 8, up rows -> + 8, of one [2 I, in] buffer: the merged half equals the model, the other half keeps its bytes."""
    for I in (8, 24, 512):
        for n in (136, 256):
            g = torch.Generator().manual_seed(I + n)
            buf = (torch.randn(2 * I, n, generator=g) * 0.05).to(R.tdtype(kind))
            _, A, B = _inputs(I, n, 16, I * n, kind, torch.float32)
            for which, layout in ((0, K_IL16_G), (1, K_IL16_U)):
                rc, got, guards = merge_op(buf, layout, I, n, A, B, 0.75)
                assert rc == O.PG_OK and guards, (I, n, which)
                res = R.same_bits(got, L.merge_il16_ref(buf, A, B, 0.75, which, kind))
                assert res["ok"], (I, n, which, res)
                other = R.il16_rows(I, 1 - which)
                assert torch.equal(R.bits(got[other]), R.bits(buf[other])), (I, n, which)
                assert not R.same_bits(got, L.defect_wrong_half(buf, A, B, 0.75, which, kind))["ok"]


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_negative_and_zero_scale(kind):
    W, A, B = _inputs(72, 136, 40, 77, kind, torch.float32)
    rc, got, guards = merge_op(W, K_T, 72, 136, A, B, -1.25)
    assert rc == O.PG_OK and guards and R.same_bits(got, L.merge_ref(W, A, B, -1.25, kind))["ok"]
    assert not R.same_bits(got, L.merge_ref(W, A, B, 1.25, kind))["ok"]
    rc, got, guards = merge_op(W, K_T, 72, 136, A, B, 0.0)
    assert rc == O.PG_OK and guards and torch.equal(R.bits(got), R.bits(W))          # the bytes are unchanged (no -0.0 among these values)


def test_refusals_launch_nothing():
    W, A, B = _inputs(12, 16, 4, 5, "bf16", torch.float32)
    buf = torch.cat([W, W])
    for layout, out in ((1, 12), (4, 12), (-1, 12), (K_IL16_G, 12), (K_IL16_U, 4)):   # not a layout; I % 8 != 0
        rc, got, guards = merge_op(buf, layout, out, 16, A[:, :16], B[:out], 1.0)
        assert rc == O.PG_ERR_ARG and guards and torch.equal(R.bits(got), R.bits(buf)), (layout, out)
    d = _lib()
    x = torch.zeros(64, device="cuda")
    for args in ((0, K_T, None, 4, 4, x.data_ptr(), x.data_ptr(), 2), (0, K_T, x.data_ptr(), 4, 4, None, x.data_ptr(), 2),
                 (0, K_T, x.data_ptr(), 4, 4, x.data_ptr(), None, 2), (2, K_T, x.data_ptr(), 4, 4, x.data_ptr(), x.data_ptr(), 2),
                 (0, K_T, x.data_ptr(), 0, 4, x.data_ptr(), x.data_ptr(), 2), (0, K_T, x.data_ptr(), 4, 0, x.data_ptr(), x.data_ptr(), 2),
                 (0, K_T, x.data_ptr(), 4, 4, x.data_ptr(), x.data_ptr(), 0), (0, K_T, x.data_ptr() + 2, 4, 4, x.data_ptr(), x.data_ptr(), 2)):
        assert d.pg_diag_op_lora_merge(*args, 1.0, None) == O.PG_ERR_ARG, args
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0
