"""GPU: operator tests of the decode GEMM dispatch -- launch_gemm_skinny / launch_gemm_skinny_swiglu (plangen_amd/csrc/gemm.hip) over the v1 / v3 / v4
kernels of gemm_skinny.h -- through pg_diag_op_gemm_skinny (csrc/diag_ops.hip: the production launchers, the caller's split count and stream_gemm mask)
against the float64 references of tests/skinny_ref.py, computed on the device.

  row sweep      every row count around the 16 / 32 / 64 / 128-row block heights at the split count production picks (rows >= M are clamped on load
                 and masked on store: `m < M ? m : M - 1`, `if (m < M)`)
  row blocks     129 .. 512 rows: grid.z > 1 of the tiled and of the row-major v3 kernels
  split sweep    every chunks-per-split value the kernels are instantiated for (16, 8, 4, 2, 1, 22, 11) on ragged M, slab by slab (out + split M N)
  stream_gemm    the v4 / v3 choice per GEMM class, the SwiGLU epilogues (direct and LDS-transposed); all masks of a shape agree with each other
  row-major      Wt == nullptr: v3 on row-major weights and its v1 fallback
  screen         every refusal of the entry point leaves the buffers alone
  mutation       the comparator rejects four planted errors against a real kernel result

Bounds: tests/skinny_ref.py (2e-4 max|ref slab| + 1e-4 per slab and for the sum; 2^-8 |ref| + 2e-4 max|ref| for the bf16 SwiGLU output)."""
import pytest
import torch

import skinny_ref as R
from conftest import get_engine

pytestmark = pytest.mark.gpu

WIDE128, WIDE64, NARROW = 4096, 4160, 208           # 128-column blocks; wide but 64-column blocks (N % 128 != 0); a ragged last column block
K0 = 2048
_SPLITS = {}


def _production_splits(tiny_cfg, tiny_weights, x, W):
    """What skinny_pick_splits gives pg_op_gemm for the shape (depends on M through the block-count targets at 48 and 96 rows)."""
    key = (x.shape[0], W.shape[0], x.shape[1])
    if key not in _SPLITS:
        _SPLITS[key] = get_engine(tiny_cfg, tiny_weights, "bf16").op_gemm_splits(x, W)
    return _SPLITS[key]


def _slabs(form, mask, M, N, K, S, ref=None):
    """One launch checked slab by slab; returns (out, ref) on the device."""
    import skinny_ops as O
    x, W, xd, wd = O.case(M, N, K)
    if ref is None:
        ref = R.slab_refs(x, W, S)
    rc, out, guards = O.run(form, mask, xd, wd, M, N, K, S)
    assert rc == O.PG_OK, rc
    res = R.check_slabs(out, ref)
    print(f"skinny form={form} mask={mask} M={M} N={N} K={K} S={S} (nck {K // R.SK_BK // S}): worst err / tol = {res['worst']:.3g}, guards {guards}")
    assert res["ok"], res
    assert guards, "a canary row in front of slab 0 or behind the last slab was written"
    return out, ref


def _swiglu(form, mask, M, N2, K, ref=None):
    import skinny_ops as O
    x, W, xd, wd = O.case(M, N2, K, R.SWIGLU_GAIN)
    if ref is None:
        ref = R.swiglu_ref(x, W)
    rc, h, guards = O.run(form, mask, xd, wd, M, N2, K, 1)
    assert rc == O.PG_OK, rc
    res = R.check_swiglu(h, ref)
    print(f"skinny SwiGLU form={form} mask={mask} M={M} 2I={N2} K={K}: worst err / bound = {res['worst']:.3g}, guards {guards}")
    assert res["ok"], res
    assert guards, "a canary row in front of row 0 or behind row M - 1 of h was written"
    return h, ref


# ------------------------------------------------------------------------------------------------------------------------------ a. row sweep
@pytest.mark.parametrize("N", [WIDE128, WIDE64, NARROW])
@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 31, 33, 48, 63, 64, 65, 79, 96, 113, 127, 128])
def test_row_sweep_at_the_production_split(tiny_cfg, tiny_weights, M, N):
    """The production decode dispatch (tiled copy, default stream_gemm) at the split count the engine picks for the shape."""
    import skinny_ops as O
    x, W, _, _ = O.case(M, N, K0)
    S = _production_splits(tiny_cfg, tiny_weights, x, W)
    assert 1 <= S <= 16 and (K0 // R.SK_BK) % S == 0, S
    _slabs(0, -1, M, N, K0, S)


# ------------------------------------------------------------------------------------------------------------------------------ b. more than one row block
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("N", [WIDE128, NARROW])
@pytest.mark.parametrize("M", [129, 130, 257, 512])
def test_more_than_one_row_block(tiny_cfg, tiny_weights, M, N, form):
    """pg_engine::gemm_llm sends up to 512 rows this way: sk3_prod_tiled (form 0) / sk3_prod (form 1) with grid.z > 1, the last block one or two rows deep
    at 129 / 130 / 257."""
    import skinny_ops as O
    x, W, _, _ = O.case(M, N, K0)
    _slabs(form, -1, M, N, K0, _production_splits(tiny_cfg, tiny_weights, x, W))


# ------------------------------------------------------------------------------------------------------------------------------ c. split sweep
@pytest.mark.parametrize("K,S", [(2048, 1), (2048, 2), (2048, 4), (2048, 8), (2048, 16), (2816, 1), (2816, 2)])
@pytest.mark.parametrize("N", [WIDE128, WIDE64, NARROW])
@pytest.mark.parametrize("M", [13, 47, 100])
def test_split_sweep(M, N, K, S):
    """Chunks per split 16, 8, 4, 2, 1 (K = 2048) and 22, 11 (K = 2816) in the 16-row, 64-row and 65..128-row forms of the default dispatch; sk4_nck has
    no 1-chunk case, so S = 16 goes to v3 on the tiled copy."""
    _slabs(0, -1, M, N, K, S)


# ------------------------------------------------------------------------------------------------------------------------------ d. stream_gemm
@pytest.mark.parametrize("N,S", [(WIDE128, 2), (NARROW, 4)])
@pytest.mark.parametrize("M", [13, 47, 100, 128])
def test_stream_gemm_masks_slabs(M, N, S):
    """stream_gemm 0: v3 on the tiled copy at every M; 15: v4 everywhere (the 128-row wide-N block above 64 rows, which the default leaves to v3); -1: the
    default.  The split counts give 8 / 4 chunks per split: both have a v4 instantiation."""
    ref, outs = None, {}
    for mask in (0, 15, -1):
        outs[mask], ref = _slabs(0, mask, M, N, K0, S, ref)
    for mask in (15, -1):
        r = R.agree(outs[0], outs[mask], ref)
        print(f"skinny M={M} N={N} S={S}: mask {mask} against mask 0, max diff / slab tol = {r:.3g}")
        assert r <= 1.0, (mask, r)


@pytest.mark.parametrize("N2", [4096, 512])
@pytest.mark.parametrize("M", [13, 47, 65, 100, 128])
def test_stream_gemm_masks_swiglu(M, N2):
    """stream_gemm 0: v3 (skinny_store_swiglu); 4: v4 with the direct SwiGLU epilogue above 16 rows (8 is not set: v3 at 13 rows); 4 | 16: v4 with the
    LDS-transposed epilogue; -1: the default (v4 direct up to 64 rows, the 16-row kernel included; v3 above).  Two forms' bf16 results are roundings of
    fp32 values an accumulation order apart: they differ by at most one bf16 ulp, 2^-7 |ref|, beside the comparator's absolute term."""
    ref, outs = None, {}
    for mask in (0, 4, 4 | 16, -1):
        outs[mask], ref = _swiglu(2, mask, M, N2, K0, ref)
    bound = 2.0 ** -7 * ref.abs() + R.SWIGLU_ATOL * float(ref.abs().max())
    for mask in (4, 4 | 16, -1):
        d = (outs[mask].to(R.F64) - outs[0].to(R.F64)).abs()
        r = float((d / bound).max())
        print(f"skinny SwiGLU M={M} 2I={N2}: mask {mask} against mask 0, max diff / (one bf16 ulp) = {r:.3g}, elements that differ {int((d > 0).sum())}")
        assert r <= 1.0, (mask, r)


# ------------------------------------------------------------------------------------------------------------------------------ e. row-major weights
@pytest.mark.parametrize("K,S", [(2048, 2), (2048, 16), (1536, 1)])
@pytest.mark.parametrize("N", [WIDE128, NARROW])
@pytest.mark.parametrize("M", [13, 47, 100])
def test_row_major_slabs(M, N, K, S):
    """Wt == nullptr: sk3_prod on row-major weights (128-row blocks for wide N, 64-row ones for narrow N above 64 rows); K = 1536 unsplit is 12 chunks per
    split, which v3 is not instantiated for: gemm_skinny_kernel (v1) takes it."""
    _slabs(1, -1, M, N, K, S)


@pytest.mark.parametrize("N2", [4096, 512])
@pytest.mark.parametrize("M", [13, 47, 100])
def test_row_major_swiglu(M, N2):
    _swiglu(3, -1, M, N2, K0)


# ------------------------------------------------------------------------------------------------------------------------------ f. argument screen
def test_refusals_leave_the_buffers_alone():
    import skinny_ops as O
    L, dev = O.lib(), "cuda"
    Mx, Nx = R.MAX_M + 1, 4096
    xd = torch.ones(Mx + O.GUARD, K0, dtype=torch.bfloat16, device=dev)
    wd = torch.full((Nx + O.GUARD, K0), 0.01, dtype=torch.bfloat16, device=dev)
    buf = O.OutBuf(16 * Mx, Nx, torch.float32, dev, fill=O.CANARY)               # room for whatever a call that did launch could write
    st = O._stream()

    def call(form=0, mask=-1, x=xd.data_ptr(), w=wd.data_ptr(), out=buf.ptr, M=47, N=Nx, K=K0, S=2):
        rc = L.pg_diag_op_gemm_skinny(form, mask, x, w, out, M, N, K, S, st)
        torch.cuda.synchronize()
        return rc

    refused = {
        "null x": dict(x=None), "null W": dict(w=None), "null out": dict(out=None),
        "x not 16-byte aligned": dict(x=xd.data_ptr() + 8), "W not 16-byte aligned": dict(w=wd.data_ptr() + 2), "out not 16-byte aligned": dict(out=buf.ptr + 4),
        "M = 0": dict(M=0), "M = 513": dict(M=R.MAX_M + 1), "N = 0": dict(N=0), "N = 8": dict(N=8), "N % 16": dict(N=Nx - 8),
        "K % 128": dict(K=2000), "K = 0": dict(K=0), "S = 0": dict(S=0), "S = -1": dict(S=-1), "16 chunks over 3 splits": dict(S=3),
        "more splits than chunks": dict(S=32), "SwiGLU with S = 2": dict(form=2), "row-major SwiGLU with S = 2": dict(form=3),
        "form 4": dict(form=4), "form -1": dict(form=-1),
        # 12 chunks per split: neither launch_gemm_skinny_swiglu path has an instantiation and the launcher says so
        "SwiGLU launcher declines K = 1536": dict(form=2, K=1536, S=1), "row-major SwiGLU launcher declines K = 1536": dict(form=3, K=1536, S=1),
    }
    for what, kw in refused.items():
        assert call(**kw) == O.PG_ERR_ARG, what
        assert buf.untouched(), what
    # N K > 0x7fffffff (the tiled copy's 32-bit vector count): a W of that size exists, should the screen ever let it through
    Nbig = (1 << 20) + 16
    wbig = torch.empty((Nbig, K0), dtype=torch.bfloat16, device=dev)
    assert call(w=wbig.data_ptr(), M=1, N=Nbig, S=1) == O.PG_ERR_ARG and buf.untouched()
    assert call(form=1, w=wbig.data_ptr(), M=1, N=Nbig, S=1) == O.PG_ERR_ARG and buf.untouched()
    del wbig
    # the entry point stays usable
    assert call() == O.PG_OK
    assert buf.guards_intact() and not buf.untouched()
    got = buf.valid()[:2 * 47].view(2, 47, Nx)
    want = torch.full((2, 47, Nx), 1024 * float(wd[0, 0]), dtype=torch.float64, device=dev)             # ones . 1024 equal weights per split
    assert (got.to(R.F64) - want).abs().max() <= R.SLAB_RTOL * float(want.abs().max()) + R.SLAB_ATOL
    assert bool((buf.valid()[2 * 47:] == O.CANARY).all())
    _slabs(0, -1, 47, NARROW, K0, 2)
    _swiglu(2, -1, 47, 512, K0)


# ------------------------------------------------------------------------------------------------------------------------------ g. checker sensitivity
def test_real_kernel_result_against_mutated_references_is_rejected():
    """A REAL result of the v4 64-row kernel (M = 47, 8 chunks per split, write-through sk4_store_direct): accepted against the reference, rejected against
    each mutated reference (a kernel with that bug would differ from the true reference by what the mutant differs from it)."""
    import skinny_ops as O
    M, N, S = 47, WIDE128, 2
    out, ref = _slabs(0, -1, M, N, K0, S)
    x, W, _, _ = O.case(M, N, K0)
    for kind in R.MUTATIONS:
        res = R.check_slabs(out, R.mutate(ref, kind, x, W))
        print(f"mutant {kind}: worst err / tol = {res['worst']:.3g}, where {res['where']}")
        assert not res["ok"] and res["worst"] > 10.0, (kind, res)
