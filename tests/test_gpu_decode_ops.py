"""GPU: operator tests of the decode step at 65..128 rows -- the deferred-1/rms RMSNorm pair (rmsnorm_defer_kernel<4|8> and
gemm_skinny3_kernel<4, NCK, 2, true, EPI, 8, TILED> with a non-null ssq) -- and of the slab-folding elementwise kernels around the decode GEMMs
(rmsnorm512_kernel<T, 0|4|8>, silu_mul_kernel, bias_act_kernel), against the CPU references of tests/decode_ref.py, through the diagnostics
library's operator entry points (plangen_amd/csrc/diag_ops.hip), which run the production launchers.

Bounds (never fitted to a GPU run):
  producer     x_new and xw BIT-EQUAL to the fp32 / bf16 emulation (and x_new to pg_op_rmsnorm's); ssq within 256 x 2^-24 (fp32 sum of 256 squares)
  slab GEMM    every slab and their sum within 2e-4 max|ref| + 1e-4 of the emulation (the bound of this kernel family in test_gpu_ops.py);
               against float64 truth E_hip <= K E_ref, E_ref = the reference's own bf16 RMSNorm arithmetic, K / K_MAX of tests/bf16ref.py
  SwiGLU GEMM  1e-2 max|ref|: one bf16 rounding of h (test_decode_swiglu_gemm_epilogue's bound)
  rmsnorm512   x_new within (S + 1) 2^-24 sum|terms|; output within 1e-5 (f32) / 1e-2 (bf16) of the row's max|ref|
  elementwise  f32 1e-5 max|ref|; bf16 2^-8 |ref| + 1e-5 max|ref|
Every output carries canary rows behind its last valid row; every input a kernel may clamp into carries NaN rows behind row M - 1."""
import pytest
import torch

import decode_ref as D
from conftest import get_engine

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _report(tag, err, bound):
    r = float((err / bound).max())
    print(f"{tag}: max |err| / bound = {r:.3g}")
    return r


# ------------------------------------------------------------------------------------------------------------------------------ a. producer
@pytest.mark.parametrize("S", [1, 4, 5, 8])
@pytest.mark.parametrize("M", [65, 80, 128])
def test_rmsnorm_defer(tiny_cfg, tiny_weights, M, S):
    """Both SB instantiations (S <= 4, S > 4) and the clamped slab index (S not a multiple of SB): the residual keeps its bits, xw is the one-rounding
    operand, the 8 partial sums of squares sit in slot half * 4 + wave."""
    from decode_ops import run_rmsnorm_defer
    x, partial, w = D.norm_inputs(M, S)
    xn, xw, ssq, guards = run_rmsnorm_defer(x, partial, w)
    want = D.x_new_f32(x, partial)
    assert torch.equal(_bits(xn), _bits(want)), "x_new differs from the sequential fp32 sum"
    x_op, _ = get_engine(tiny_cfg, tiny_weights, "bf16").op_rmsnorm(x, w, D.EPS, partial)
    assert torch.equal(_bits(xn), _bits(x_op.cpu())), "x_new differs from the residual rmsnorm512_kernel leaves"
    assert torch.equal(_bits(xw), _bits(D.xw_emul(want, w))), "xw differs from bf16(fp32(w) * x_new)"
    q = D.ssq_ref(want)
    r = _report(f"rmsnorm_defer M={M} S={S} ssq", (ssq.to(F64) - q).abs(), D.SSQ_RTOL * q)
    assert r <= 1.0, r
    assert guards, "a guard row of x, xw or ssq was written"


def test_rmsnorm_defer_refuses_what_the_launcher_excludes():
    from decode_ops import PG_ERR_ARG, rmsnorm_defer_status
    M = 65
    for Hh, S, m, slab in [(1024, 4, M, M * 1024), (4096, 4, M, M * 4096), (2048, 0, M, M * 2048), (2048, 9, M, M * 2048), (2048, 4, 0, 2048),
                           (2048, 4, M, M * 2048 - 4), (2048, 4, M, 1 << 31)]:
        rc, untouched = rmsnorm_defer_status(m, Hh, S, slab)
        assert rc == PG_ERR_ARG and untouched, (Hh, S, m, slab, rc, untouched)


# ------------------------------------------------------------------------------------------------------------------------------ b. slab GEMM
@pytest.mark.parametrize("M,N,S,Sn", D.GEMM_CASES)
def test_deferred_slab_gemm(M, N, S, Sn):
    """qkv form at NCK 16 / 8 / 4 / 2 / 1, fed by the producer's own outputs; 65 <= M < 128 leaves the second 64-row block partly empty."""
    from decode_ops import run_gemm_deferred, run_rmsnorm_defer
    x, partial, w = D.norm_inputs(M, Sn)
    W = D.gemm_weights(N)
    _, xw, ssq, _ = run_rmsnorm_defer(x, partial, w)
    out, guard = run_gemm_deferred(xw, ssq, W, S, D.EPS)
    emul = D.gemm_emul(x, partial, w, W, S)
    worst = 0.0
    for s in range(S):
        tol = 2e-4 * float(emul[s].abs().max()) + 1e-4
        err = float((out[s].to(F64) - emul[s]).abs().max())             # NaN (an element never written) fails the comparison below
        worst = max(worst, err / tol)
        assert err < tol, f"slab {s}: {err:.3g} against {tol:.3g}"
    total, whole = out.to(F64).sum(0), emul.sum(0)
    tol = 2e-4 * float(whole.abs().max()) + 1e-4
    err = float((total - whole).abs().max())
    print(f"deferred GEMM M={M} N={N} S={S}: worst slab err / tol = {worst:.3g}, slab sum err / tol = {err / tol:.3g}")
    assert err < tol, (err, tol)
    assert guard, "rows behind the last slab were written"
    true = D.gemm_true(x, partial, w, W)
    ratios, bad = D.k_rule((total - true).abs(), (D.gemm_refbf(x, partial, w, W) - true).abs())
    print(f"deferred GEMM M={M} N={N} S={S}: E_hip / E_ref =", {k: round(v, 3) for k, v in ratios.items()})
    assert not bad, f"E_hip exceeds K x E_ref (a finding, not a tolerance to widen): {bad}"


@pytest.mark.parametrize("M,N,K,S", [(64, 4096, 2048, 1), (129, 4096, 2048, 1), (128, 2048, 2048, 1), (128, 4160, 2048, 1), (128, 4096, 4096, 1),
                                     (128, 4096, 2048, 3), (128, 4096, 2048, 32)])
def test_deferred_norm_ok_domain(M, N, K, S):
    from decode_ops import PG_ERR_ARG, gemm_deferred_status
    for swiglu in ([False, True] if S == 1 else [False]):
        rc, untouched = gemm_deferred_status(M, N, K, S, swiglu)
        assert rc == PG_ERR_ARG and untouched, (rc, untouched, swiglu)


# ------------------------------------------------------------------------------------------------------------------------------ c. SwiGLU GEMM
@pytest.mark.parametrize("M,N2,Sn", D.SWIGLU_CASES)
def test_deferred_swiglu_gemm(M, N2, Sn):
    """gate|up form (NCK 16, EPI 1) with the row scale applied before the SwiGLU; 2 I = 11264 is the production shape."""
    from decode_ops import run_gemm_deferred, run_rmsnorm_defer
    x, partial, w = D.norm_inputs(M, Sn)
    wg, wu = D.swiglu_weights(N2 // 2)
    W = D.interleave_gate_up(wg, wu)
    _, xw, ssq, _ = run_rmsnorm_defer(x, partial, w)
    h, guard = run_gemm_deferred(xw, ssq, W, 1, D.EPS, swiglu=True)
    ref = D.swiglu(D.gemm_emul(x, partial, w, W, 1)[0])
    err = float((h.to(F64) - ref).abs().max())
    tol = 1e-2 * float(ref.abs().max())
    print(f"deferred SwiGLU M={M} 2I={N2}: max |err| / (1e-2 max|ref|) = {err / tol:.3g}")
    assert err < tol, (err, tol)
    assert guard, "rows behind row M - 1 of h were written"


# ------------------------------------------------------------------------------------------------------------------------------ d. rmsnorm512
@pytest.mark.parametrize("S", [0, 1, 5, 8, 9, 11, 22])
@pytest.mark.parametrize("M", [1, 80])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rmsnorm512_slab_sweep(tiny_cfg, tiny_weights, dtype, M, S):
    """SB = 0 (S = 0), 4 and 8, and the batches-of-8 tail of rmsnorm_row (S > 8: one tail batch at 9 / 11, two at 22)."""
    e = get_engine(tiny_cfg, tiny_weights, dtype)
    x, partial, w = D.norm_inputs(M, S, False)
    w = w if dtype == "bf16" else w.float()
    xn, out = e.op_rmsnorm(x, w, D.EPS, partial if S else None)
    xr, ref = D.rmsnorm_ref(x, partial if S else None, w)
    r = _report(f"rmsnorm512 {dtype} M={M} S={S} x_new", (xn.cpu().to(F64) - xr).abs(), D.slab_sum_bound(x, partial if S else None))
    assert r <= 1.0, r
    tol = (1e-5 if dtype == "f32" else 1e-2) * ref.abs().amax(-1, keepdim=True)
    r = _report(f"rmsnorm512 {dtype} M={M} S={S} out", (out.cpu().to(F64) - ref).abs(), tol)
    assert r < 1.0, r


# ------------------------------------------------------------------------------------------------------------------------------ e. elementwise
@pytest.mark.parametrize("S", [1, 4, 5, 9])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_silu_mul(dtype, S):
    from decode_ops import run_slab_epilogue
    M = 3
    for I in (512, 1000):
        g = torch.Generator().manual_seed(100 * S + I)
        gu = torch.randn(S, M, 2 * I, generator=g) * torch.linspace(0.3, 1.5, 2 * I)
        gu.view(S, M, I // 8, 2, 8)[:, :, :, 1] *= 1.7                  # up columns on another scale than gate: swapped halves show
        out, guard = run_slab_epilogue(0, dtype, gu, None, 0)
        ref = D.silu_mul_ref(gu)
        r = _report(f"silu_mul {dtype} S={S} I={I}", (out.to(F64) - ref).abs(), D.elementwise_bound(ref, dtype))
        assert r < 1.0, r
        assert guard


@pytest.mark.parametrize("S", [1, 4, 5, 9])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bias_act(dtype, S):
    """launch_bias_act (the gen_head's GELU) and launch_bias_f32 (f32, act 0)."""
    from decode_ops import run_slab_epilogue
    M = 3
    for N in (256, 1000):
        g = torch.Generator().manual_seed(100 * S + N)
        p = torch.randn(S, M, N, generator=g) * torch.linspace(0.3, 1.5, N)
        bias = torch.randn(N, generator=g) * 2
        for act in (0, 1):
            for b in (None, bias):
                out, guard = run_slab_epilogue(1, dtype, p, b, act)
                ref = D.bias_act_ref(p, b, act)
                r = _report(f"bias_act {dtype} S={S} N={N} act={act} bias={b is not None}", (out.to(F64) - ref).abs(), D.elementwise_bound(ref, dtype))
                assert r < 1.0, r
                assert guard
