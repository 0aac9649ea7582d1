"""Operator tests of the weight converters pg_load_tensor launches and of the row movers of every prefill / step / score call, through the PRODUCTION launchers
(pg_diag_op_convert, pg_diag_op_rows of libplangen_diag.so) against the host models of tests/load_ref.py.  Every one of these transforms is exact: the results
are compared bit for bit (a NaN with isnan), every destination is pre-filled with a sentinel and carries sentinel guards on both sides.

Which kernel a case reaches (source type -> the test that reaches it):
  convert_kernel<float>          fp32 / bf16  test_convert[*-f32], test_convert_scalar_grid_wrap
  convert_kernel<bf16>           fp32 / bf16  test_convert[*-bf16] (fp32: n < 65536, n % 8 != 0 or a misaligned pointer), test_convert_scalar_grid_wrap
  convert_f32_bf16_vec_kernel    fp32 only    test_convert[65536 / 65544-f32-bf16], test_convert_vector_grid_wrap
  convert_conv_kernel<T>         fp32 / bf16  test_convert_conv, test_convert_conv_grid_wrap (bf16)
  convert_il16_kernel<T>         fp32 / bf16  test_convert_interleave16
  embed_gather / copy_rows / rows_to_f32 / t_to_rows<float> / t_to_rows<bf16> / rows_differ: test_row_movers, test_rows_differ"""
import pytest
import torch

import load_ops as O
import load_ref as R

pytestmark = pytest.mark.gpu

KINDS = ("f32", "bf16")
PAIRS = [(s, d) for s in KINDS for d in KINDS]
SCALAR_GRID = 4096 * 256                                    # elements one pass of the capped scalar grids covers
VECTOR_GRID = 8192 * 256 * 8                                # ... and of convert_f32_bf16_vec_kernel's


def _vector_expected(src, dst, n, aligned=True):
    return int(src == "f32" and dst == "bf16" and n >= 65536 and n % 8 == 0 and aligned)


def _check(got, want, what):
    res = R.same_bits(got, want)
    assert res["ok"], (what, res)


# ------------------------------------------------------------------------------------------------------------------------------ convert
@pytest.mark.parametrize("src,dst", PAIRS)
@pytest.mark.parametrize("n", [1, 7, 8, 65528, 65536, 65537, 65544])
def test_convert(n, src, dst):
    x = R.values(n, src, seed=n)
    for which in ((0, 1) if dst == "f32" else (0,)):         # fp32 destinations also through launch_to_f32 (the K_F32 slots)
        rc, got, intact, kernel, _ = O.convert(x, dst, which=which)
        assert rc == O.PG_OK and intact
        assert kernel == _vector_expected(src, dst, n), (n, src, dst, kernel)
        _check(got[:n], R.convert_ref(x, dst), (n, src, dst, which))


@pytest.mark.parametrize("src,dst", PAIRS)
def test_convert_misaligned_pointers_take_the_scalar_kernel(src, dst):
    n = 65536
    x = R.values(n, src, seed=77)
    rc, got, intact, kernel, _ = O.convert(x, dst, src_off=4)                  # the source 4 bytes off a 16-byte boundary
    assert rc == O.PG_OK and intact and kernel == 0
    _check(got[:n], R.convert_ref(x, dst), ("src + 4", src, dst))
    rc, got, intact, kernel, _ = O.convert(x, dst, dst_off=2)                  # the destination 2 bytes off
    if dst == "f32":                                                           # not a float address: refused, nothing written
        assert rc == O.PG_ERR_ARG and intact and bool(R.is_sentinel(got).all())
    else:
        assert rc == O.PG_OK and intact and kernel == 0
        _check(got[:n], R.convert_ref(x, dst), ("dst + 2", src, dst))


@pytest.mark.parametrize("src,dst", PAIRS)
def test_convert_scalar_grid_wrap(src, dst):
    n = SCALAR_GRID + 513                                                      # 4096 blocks cover 1048576: the last 513 elements are second-pass work
    x = R.values(n, src, seed=5)
    rc, got, intact, kernel, _ = O.convert(x, dst, src_off=4)                  # off alignment: fp32 -> bf16 stays on the scalar kernel too
    assert rc == O.PG_OK and intact and kernel == 0 and n > SCALAR_GRID
    _check(got[:n], R.convert_ref(x, dst), (src, dst))


def test_convert_vector_grid_wrap():
    n = 8 * (8192 * 256 + 300)                                                 # 8192 blocks x 256 threads x 8: 300 vectors of second-pass work
    x = R.values(n, "f32", seed=6)
    rc, got, intact, kernel, _ = O.convert(x, "bf16")
    assert rc == O.PG_OK and intact and kernel == 1 and n > VECTOR_GRID
    _check(got[:n], R.convert_ref(x, "bf16"), "vector wrap")


# ------------------------------------------------------------------------------------------------------------------------------ convert_conv
@pytest.mark.parametrize("src,dst", PAIRS)
@pytest.mark.parametrize("shape", [(1, 1, 9), (3, 5, 9), (4, 128, 9), (128, 64, 9), (64, 128, 1)], ids=lambda s: "x".join(map(str, s)))
def test_convert_conv(shape, src, dst):
    co, ci, kk = shape
    w = R.values(co * ci * kk, src, seed=co + ci).reshape(co, ci, kk)
    rc, got, intact, _, _ = O.convert(w, dst, kind=1, a=co, b=ci, c=kk)
    assert rc == O.PG_OK and intact
    _check(got[:w.numel()].reshape(co, kk, ci), R.conv_ref(w, dst), (shape, src, dst))


def test_convert_conv_grid_wrap():
    co, ci, kk = 256, 512, 9                                                   # 1179648 elements > 4096 x 256
    w = R.values(co * ci * kk, "bf16", seed=9).reshape(co, ci, kk)
    assert w.numel() > SCALAR_GRID
    rc, got, intact, _, _ = O.convert(w, "bf16", kind=1, a=co, b=ci, c=kk)
    assert rc == O.PG_OK and intact
    _check(got[:w.numel()].reshape(co, kk, ci), R.conv_ref(w, "bf16"), "conv wrap")


# ------------------------------------------------------------------------------------------------------------------------------ interleave16
@pytest.mark.parametrize("src,dst", PAIRS)
@pytest.mark.parametrize("IH", [(8, 8), (16, 24), (360, 128)], ids=lambda s: "x".join(map(str, s)))
def test_convert_interleave16(IH, src, dst):
    I, H = IH
    g, u = R.values(I * H, src, seed=I).reshape(I, H), R.values(I * H, src, seed=I + 1).reshape(I, H)
    for order in ((0, 1), (1, 0)):                                             # gate then up, up then gate: one destination
        buf = None
        for step, which in enumerate(order):
            rc, got, intact, _, buf = O.convert(g if which == 0 else u, dst, kind=2, a=I, b=H, which=which, dst=buf)
            assert rc == O.PG_OK and intact
            got = got[:2 * I * H].reshape(2 * I, H)
            if step == 0:                                                      # the other half is still untouched
                assert bool(R.is_sentinel(got[R.il16_rows(I, 1 - which)]).all())
                _check(got[R.il16_rows(I, which)], R.convert_ref(g if which == 0 else u, dst), (IH, src, dst, "first half"))
        _check(got, R.il16_ref(g, u, dst), (IH, src, dst, order))


# ------------------------------------------------------------------------------------------------------------------------------ row movers
@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("H", [4, 252, 256, 2048])
def test_row_movers(H, n):
    vocab, rows_src, rows_dst = 37, n + 5, n + 7
    table = R.values(vocab * H, "f32", seed=H).reshape(vocab, H)
    g = torch.Generator().manual_seed(H + n)
    ids = torch.randint(0, vocab, (n + 6,), generator=g).to(torch.int32)
    ids[:5] = torch.tensor([-1, 0, vocab - 1, vocab, R.INT32_MAX], dtype=torch.int32)[:min(5, n + 6)]
    # embed_gather: without src_idx (ids[t]) and through each index vector into ids
    rc, got, intact = O.rows(0, table, n, H, "f32", n, ids=ids)
    assert rc == O.PG_OK and intact
    _check(got, R.embed_gather_ref(table, ids[:n], None, vocab), ("gather", H, n))
    for name, idx in R.index_vectors(n, ids.numel(), seed=n).items():
        rc, got, intact = O.rows(0, table, n, H, "f32", n, ids=ids, src_idx=idx)
        assert rc == O.PG_OK and intact
        _check(got, R.embed_gather_ref(table, ids, idx, vocab), ("gather", name, H, n))
    for kind in KINDS:
        src = R.values(rows_src * H, kind, seed=H + 1).reshape(rows_src, H)
        gathers = R.index_vectors(n, rows_src, seed=n + 1)
        scatters = {k: v for k, v in R.index_vectors(n, rows_dst, seed=n + 2).items() if k != "repeats"}
        fill = R.sentinel_like((rows_dst, H), kind)
        # copy_rows: gather, scatter, both, neither
        for gname, gi in [("none", None)] + list(gathers.items()):
            for sname, si in [("none", None)] + list(scatters.items()):
                rc, got, intact = O.rows(1, src, rows_dst, H, kind, n, src_idx=gi, dst_idx=si)
                assert rc == O.PG_OK and intact
                _check(got, R.copy_rows_ref(src, gi, fill, si, n), ("copy", kind, gname, sname, H, n))
        # rows_to_f32
        for gname, gi in [("none", None)] + list(gathers.items()):
            rc, got, intact = O.rows(2, src, n, H, "f32", n, src_idx=gi)
            assert rc == O.PG_OK and intact
            _check(got, R.rows_to_f32_ref(src, gi, n), ("rows_to_f32", kind, gname, H, n))
        # f32_to_rows / t_to_rows<float> (fp32 source), t_to_rows<bf16> (bf16 source) into both destination types
        for op in ((3, 4) if kind == "f32" else (5,)):
            for dk in KINDS:
                dfill = R.sentinel_like((rows_dst, H), dk)
                for sname, si in [("none", None)] + list(scatters.items()):
                    rc, got, intact = O.rows(op, src, rows_dst, H, dk, n, dst_idx=si)
                    assert rc == O.PG_OK and intact
                    _check(got, R.t_to_rows_ref(src, dfill, si, n), ("to_rows", op, dk, sname, H, n))


@pytest.mark.parametrize("H", [4, 256])
def test_embed_gather_clamps_ids(H):
    vocab = 37
    table = R.values(vocab * H, "f32", seed=H + 3).reshape(vocab, H)
    ids = torch.tensor([-1, 0, vocab - 1, vocab, R.INT32_MAX, -2 ** 31, 5], dtype=torch.int32)
    rc, got, intact = O.rows(0, table, ids.numel(), H, "f32", ids.numel(), ids=ids)
    assert rc == O.PG_OK and intact
    want = table[torch.tensor([0, 0, vocab - 1, vocab - 1, vocab - 1, 0, 5])]
    _check(got, want, ("clamp", H))
    _check(got, R.embed_gather_ref(table, ids, None, vocab), ("clamp model", H))


def test_rows_differ():
    L, frm, rows_n = 300, 40, 9                                                # 300 columns: a second pass of the 256-thread loop
    base = torch.randint(0, 1000, (1, L), generator=torch.Generator().manual_seed(1)).to(torch.int32).repeat(rows_n, 1)
    first, stride, ref, n = 3, 2, 1, 3                                         # rows 3, 5, 7 against row 1

    def run(edit):
        ids = base.clone()
        for r, c in edit:
            ids[r, c] += 1
        rc, flag = O.rows_differ(ids, first, stride, ref, n, frm)
        assert rc == O.PG_OK and flag == R.rows_differ_ref(ids, first, stride, ref, n, frm)
        return flag

    assert run([]) == 0
    assert run([(7, frm - 1)]) == 0                                            # one element in front of ``from``
    assert run([(7, frm)]) == 1 and run([(3, L - 1)]) == 1 and run([(5, 299)]) == 1
    assert run([(ref, L - 1)]) == 1                                            # in the reference row only
    assert run([(4, 100), (8, 100), (0, 100)]) == 0                            # rows the stride skips
    assert run([(7, 0), (3, frm - 1)]) == 0
    rc, flag = O.rows_differ(base, first, stride, ref, n, frm, flag0=1)        # the flag is OR-ed into, never cleared
    assert rc == O.PG_OK and flag == 1
    rc, flag = O.rows_differ(base, first, stride, ref, n, L)                   # from == L: nothing is compared
    assert rc == O.PG_OK and flag == 0


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_convert_refusals_leave_the_destination_untouched():
    x32, x16 = R.values(64, "f32", 1), R.values(64, "bf16", 1)
    calls = [
        dict(src=x32, dst_kind="bf16", kind=3),                                # no such converter
        dict(src=x32, dst_kind="bf16", kind=-1),
        dict(src=x32, dst_kind="bf16", n=0),
        dict(src=x32, dst_kind="bf16", n=-5),
        dict(src=x32, dst_kind="bf16", src_off=2),                             # not a float address
        dict(src=x16, dst_kind="f32", dst_off=2),
        dict(src=x32, dst_kind="f32", kind=1, a=0, b=8, c=8),
        dict(src=x32, dst_kind="f32", kind=1, a=8, b=8, c=0),
        dict(src=x32.reshape(4, 16), dst_kind="bf16", kind=2, a=4, b=16, which=1),      # I % 8 != 0: the up rows would start behind row 2 I - 1
        dict(src=x32.reshape(8, 8), dst_kind="bf16", kind=2, a=8, b=8, which=2),
        dict(src=x32.reshape(8, 8), dst_kind="bf16", kind=2, a=8, b=0, which=0),
    ]
    for kw in calls:
        src = kw.pop("src")
        rc, got, intact, _, buf = O.convert(src, **kw)
        assert rc == O.PG_ERR_ARG and intact and bool(R.is_sentinel(buf).all()), kw
    d = O.guarded(64, "bf16")
    s = x32.cuda()
    L = O.lib()
    import ctypes as C
    k = C.c_int(-1)
    st = torch.cuda.current_stream().cuda_stream
    assert L.pg_diag_op_convert(0, 0, 1, None, d.data_ptr(), 64, 0, 0, 0, 0, C.byref(k), st) == O.PG_ERR_ARG
    assert L.pg_diag_op_convert(0, 0, 1, s.data_ptr(), None, 64, 0, 0, 0, 0, C.byref(k), st) == O.PG_ERR_ARG
    assert L.pg_diag_op_convert(0, 0, 1, s.data_ptr(), d.data_ptr(), 64, 0, 0, 0, 0, None, st) == O.PG_ERR_ARG
    assert L.pg_diag_op_convert(0, 2, 1, s.data_ptr(), d.data_ptr(), 64, 0, 0, 0, 0, C.byref(k), st) == O.PG_ERR_ARG
    torch.cuda.synchronize()
    assert bool(R.is_sentinel(d).all())


def test_row_mover_refusals_leave_the_destination_untouched():
    t6, t8 = R.values(5 * 6, "f32", 1).reshape(5, 6), R.values(5 * 8, "f32", 2).reshape(5, 8)
    b3 = R.values(5 * 3, "bf16", 3).reshape(5, 3)
    ids = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    calls = [
        dict(op=0, src=t6, dst_rows=4, width=6, dst_kind="f32", n=4, ids=ids),                              # H % 4 != 0: the kernel moves float4
        dict(op=0, src=t8, dst_rows=4, width=8, dst_kind="f32", n=4, ids=ids, src_off=4, src_rows=4),       # table rows off 16 bytes
        dict(op=0, src=t8, dst_rows=4, width=8, dst_kind="f32", n=4, ids=ids, dst_off=4),                   # destination rows off 16 bytes
        dict(op=0, src=t8, dst_rows=4, width=8, dst_kind="f32", n=4),                                       # no ids
        dict(op=0, src=t8, dst_rows=4, width=8, dst_kind="f32", n=4, ids=ids, src_idx=i32(0, 1, 2, 4)),     # src_idx past the ids
        dict(op=0, src=t8, dst_rows=4, width=8, dst_kind="f32", n=5, ids=ids),                              # more rows than ids / destination rows
        dict(op=1, src=b3, dst_rows=5, width=3, dst_kind="bf16", n=5),                                      # row_bytes = 6: not whole 32-bit words
        dict(op=1, src=t8, dst_rows=5, width=8, dst_kind="f32", n=2, width_arg=4 * 2 ** 31),                # row_bytes / 4 does not fit the kernel's int
        dict(op=1, src=t8, dst_rows=5, width=8, dst_kind="f32", n=2, width_arg=0),
        dict(op=1, src=t8, dst_rows=5, width=8, dst_kind="f32", n=3, src_idx=i32(0, 5, 1)),                 # gather past the source
        dict(op=1, src=t8, dst_rows=5, width=8, dst_kind="f32", n=3, src_idx=i32(0, -1, 1)),
        dict(op=1, src=t8, dst_rows=5, width=8, dst_kind="f32", n=3, dst_idx=i32(0, 5, 1)),                 # scatter past the destination
        dict(op=1, src=t8, dst_rows=5, width=8, dst_kind="f32", n=3, dst_idx=i32(2, 0, 2)),                 # two rows into one
        dict(op=1, src=t8, dst_rows=4, width=8, dst_kind="f32", n=5),                                       # identity past the destination
        dict(op=2, src=t8, dst_rows=4, width=8, dst_kind="f32", n=3, src_idx=i32(0, 9, 1)),
        dict(op=2, src=t8, dst_rows=2, width=8, dst_kind="f32", n=3),
        dict(op=3, src=t8, dst_rows=5, width=8, dst_kind="bf16", n=3, dst_idx=i32(1, 1, 0)),
        dict(op=4, src=t8, dst_rows=5, width=8, dst_kind="f32", n=6),                                       # more rows than the source has
        dict(op=5, src=b3, dst_rows=5, width=3, dst_kind="bf16", n=2, dst_idx=i32(0, 7)),
        dict(op=7, src=t8, dst_rows=5, width=8, dst_kind="f32", n=2),
        dict(op=2, src=t8, dst_rows=5, width=8, dst_kind="f32", n=0),
    ]
    for kw in calls:
        rc, got, intact = O.rows(**kw)
        assert rc == O.PG_ERR_ARG and intact and bool(R.is_sentinel(got).all()), kw
    m = torch.zeros(6, 10, dtype=torch.int32)
    for first, stride, ref, n, frm in [(3, 2, 1, 3, 4), (3, 2, 6, 2, 4), (3, 2, 1, 2, 11), (3, 0, 1, 2, 4), (-1, 2, 1, 2, 4), (3, 2, 1, 2, -1)]:
        rc, flag = O.rows_differ(m, first, stride, ref, n, frm, flag0=0x5A)
        assert rc == O.PG_ERR_ARG and flag == 0x5A, (first, stride, ref, n, frm)
