"""GPU: operator tests of the understanding path's input-side kernels -- SigLIP's LayerNorm (both kernels), patchify, add_pos, the VQ encoder's conv_in, the
nearest-code search (both kernels), l2norm_rows, the two-level batched GEMM of SigLIP's scores and P . V on both engines, and pg_engine::lin()'s in-place
residual and bias + GELU forms -- against the float64 references and derived bounds of tests/vision_ref.py, through the operator entry points of the
diagnostics library (plangen_amd/csrc/diag_ops.hip; bindings and guard bands: tests/vision_ops.py), which call the PRODUCTION launchers with one kernel form pinned.

Every comparison prints max err / bound (measurements for the record; no bound depends on them) before it asserts <= 1."""
import pytest
import torch

import vision_ref as V

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _report(tag, got, ref, bound):
    r, i = V.worst((got.to(F64) - ref).abs(), bound)
    print(f"{tag}: max |err| / bound = {r:.3g} at flat index {i}")
    return r


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("form,C,M", V.LN_CASES)
def test_layernorm(form, C, M):
    """form 0 = layernorm_kernel (C < 256, C % 256 != 0, C = 1024 too), form 1 = layernorm_wave_kernel<T, 4> with partly filled last blocks; fp32 and bf16 output;
    rows of mean 100 sigma, the constant row = beta; the rows behind M (guard band) untouched."""
    from vision_ops import run_layernorm
    x, g, b = V.ln_inputs(M, C)
    ref = V.ln_ref(x, g, b)
    for out_kind in ("f32", "bf16"):
        o = run_layernorm(x, g, b, form, out_kind, V.LN_EPS)
        assert o["guards"], "a row past M was written"
        r = _report(f"layernorm form {form} M={M} C={C} {out_kind}", o["out"].float(), ref, V.ln_bound(x, g, b, out_kind))
        assert r <= 1.0, r
        if M > V.LN_CONST_ROW and out_kind == "f32":
            assert torch.equal(o["out"][V.LN_CONST_ROW], b), "the constant row is not beta"


# ------------------------------------------------------------------------------------------------------------------------------ patchify / add_pos
@pytest.mark.parametrize("in_kind,out_kind", V.PATCH_TYPES)
@pytest.mark.parametrize("S,ps,B", V.PATCH_CASES)
def test_patchify_bit_exact(S, ps, B, in_kind, out_kind):
    from vision_ops import run_patchify
    img = V.patch_image(S, B, in_kind, out_kind)
    o = run_patchify(img, ps, in_kind, out_kind)
    assert o["guards"]
    want = V.patchify_ref(img, ps).to(o["out"].dtype)
    assert torch.equal(_bits(o["out"]), _bits(want))
    print(f"patchify S={S} ps={ps} B={B} {in_kind}->{out_kind}: bit exact, max |err| / bound = 0")


@pytest.mark.parametrize("B,P,C", V.ADD_POS_CASES)
def test_add_pos_bit_exact(B, P, C):
    from vision_ops import run_add_pos
    x, pos = V.add_pos_inputs(B, P, C)
    got, guards = run_add_pos(x, pos, B)
    assert guards and torch.equal(_bits(got), _bits(V.add_pos_ref(x, pos, B)))
    print(f"add_pos B={B} P={P} C={C}: bit exact, max |err| / bound = 0")


# ------------------------------------------------------------------------------------------------------------------------------ conv_in
@pytest.mark.parametrize("B,H,W,Cout", V.CONV_IN_CASES)
def test_conv_in(B, H, W, Cout):
    """conv3x3_in_kernel: one-pixel strips, 63 / 64 / 64 + 1 / 64 + 64 + 2 pixel rows, Cout below, at and above the 128 threads; fp32 / bf16 image and output."""
    from vision_ops import run_conv_in
    worst = 0.0
    for in_kind, out_kind in V.CONV_IN_TYPES:
        x, w, bias = V.conv_in_inputs(B, H, W, Cout, in_kind)
        ref, mag = V.conv_in_ref(x, w, bias)
        got, guards = run_conv_in(x, w, bias, in_kind, out_kind)
        assert guards
        worst = max(worst, _report(f"conv_in {B}x{H}x{W} Cout={Cout} {in_kind}->{out_kind}", got.float(), ref, V.conv_in_bound(ref, mag, out_kind)))
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------------------ nearest code
def _argmin(form, D, Vn, n):
    from vision_ops import run_vq_argmin
    z, cb, planted = V.argmin_inputs(D, Vn, n)
    o = run_vq_argmin(z, cb, form)
    assert o["guards"], "an index slot past n was written"
    res = V.argmin_check(o["idx"], z, cb, planted)
    print(f"vq_argmin form {form} D={D} V={Vn} n={n}: max (d_i - d_min) / accepted error = {res['worst']:.3g}, planted rows wrong: {res['planted_bad']}")
    assert res["ok"], res
    return o["idx"]


@pytest.mark.parametrize("form,D,Vn,n", V.ARGMIN_CASES)
def test_vq_argmin(form, D, Vn, n):
    """Every returned index within the derived distance error of the float64 minimum; needles at 0 / 63 / 64 / 255 / 256 / V - 1, the lower of duplicate codes and
    the zero vector's nearest code exactly; the slots behind idx[n - 1] untouched."""
    _argmin(form, D, Vn, n)


@pytest.mark.parametrize("D,Vn,n", V.ARGMIN_SHARED)
def test_vq_argmin_kernels_agree_bit_for_bit(D, Vn, n):
    assert torch.equal(_argmin(0, D, Vn, n), _argmin(1, D, Vn, n))


def test_vq_argmin_production_dispatch():
    """form 2 (launch_vq_argmin under the default tune): n = 63 runs the one-vector kernel, n = 64 the eight-vector kernel."""
    for n, form in ((63, 0), (64, 1)):
        assert torch.equal(_argmin(2, 8, 1000, n), _argmin(form, 8, 1000, n))


# ------------------------------------------------------------------------------------------------------------------------------ l2norm_rows
@pytest.mark.parametrize("n,D", V.L2_CASES)
def test_l2norm_rows(n, D):
    from vision_ops import run_l2norm
    x = V.l2_inputs(n, D)
    got, guards = run_l2norm(x)
    assert guards
    assert _report(f"l2norm_rows n={n} D={D}", got, V.l2_ref(x), V.l2_bound(x)) <= 1.0
    if n > 1:
        assert bool((got[n // 2] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------ SigLIP's heads GEMMs
def _scores(B, NH, P, C, engine, form, hd=64, inputs=None, expect=0):
    from vision_ops import run_gemm_heads
    qk = (inputs or V.heads_inputs(B, NH, P, C, engine, hd))[0]
    return run_gemm_heads(qk, 0, qk, C, "f32", P, P, hd, B, NH, 2 * C, P * 2 * C, hd, 2 * C, P * 2 * C, hd, P, NH * P * P, P * P, form=form, engine=engine,
                          expect=expect)


def _pv(B, NH, P, C, engine, form, ldc=None, stride2=64, expect=0):
    from vision_ops import run_gemm_heads
    _, p, vt = V.heads_inputs(B, NH, P, C, engine)
    ldc = ldc or C
    return run_gemm_heads(p, 0, vt, 0, engine, P, 64, P, B, NH, P, NH * P * P, P * P, P, C * P, 64 * P, ldc, P * ldc, stride2, form=form, engine=engine, expect=expect)


# the ragged P = 72 case is the fp32 engine's alone: the bf16 loaders need K % 64 == 0
@pytest.mark.parametrize("B,NH,P,C,engine", [c + (e,) for c in V.HEADS_CASES for e in ("bf16", "f32")] + [V.HEADS_RAGGED + ("f32",)])
def test_siglip_heads_gemms(B, NH, P, C, engine):
    """scores and P . V exactly as pg_engine::vision_encode lays them out (bf16: the 128 x 128 kernel, form 1; fp32: gemm_f32_kernel's blockIdx.z % / nbatch), per
    element against float64; P . V writes head h at COLUMN offset 64 h inside rows of ldc = C."""
    form = 1 if engine == "bf16" else 0
    qk, p, vt = V.heads_inputs(B, NH, P, C, engine)
    o = _scores(B, NH, P, C, engine, form)
    ref, mag = V.scores_ref(qk, B, NH, P, C)
    assert o["guards"]
    assert _report(f"scores B={B} NH={NH} P={P} {engine}", o["out"].view(B, NH, P, P), ref, V.gemm_bound(ref, mag, 64, "f32")) <= 1.0
    o = _pv(B, NH, P, C, engine, form)
    ref, mag = V.pv_ref(p, vt, B, NH, P, C)
    r, gaps = V.heads_check(o["out"].view(B * P, C).float(), ref, mag, P, engine)
    print(f"P.V B={B} NH={NH} P={P} {engine}: max |err| / bound = {r:.3g}")
    assert o["guards"] and gaps and r <= 1.0, r


@pytest.mark.parametrize("engine", ["bf16", "f32"])
def test_siglip_pv_heads_with_sentinel_gaps(engine):
    """The P . V layout with the heads 80 columns apart: the 16 columns between neighbouring heads' blocks must keep their NaN pre-fill."""
    B, NH, P, C = V.HEADS_CASES[1]
    _, p, vt = V.heads_inputs(B, NH, P, C, engine)
    ldc = NH * V.HEADS_GAP
    o = _pv(B, NH, P, C, engine, 1 if engine == "bf16" else 0, ldc=ldc, stride2=V.HEADS_GAP)
    ref, mag = V.pv_ref(p, vt, B, NH, P, C, ldc=ldc, stride2=V.HEADS_GAP)
    flat = torch.full((B * P * ldc,), float("nan"))
    flat[:o["out"].numel()] = o["out"].float()
    r, gaps = V.heads_check(flat.view(B * P, ldc), ref, mag, P, engine)
    print(f"P.V gapped {engine}: max |err| / bound = {r:.3g}, gaps intact: {gaps}")
    assert o["guards"] and gaps and r <= 1.0, r


def test_heads_gemms_and_the_256_tile():
    """gemm256_try takes NEITHER SigLIP layout at any size (scores: K = 64 < 128; P . V: N = 64 is a quarter of a tile): form 2 refuses both at 200 (image, head)
    pairs, output untouched.  It does not refuse batch2 > 1 as such: the scores layout with heads of 128 at P = 256 and 25 x 8 pairs (200 tiles) runs, bit-equal to
    the 128 x 128 kernel and inside the bound; 24 x 8 = 192 tiles is refused."""
    from vision_ops import PG_ERR_ARG, run_gemm_heads
    B, NH, P, hd = V.T256_HEADS
    C = NH * 64
    g = torch.Generator().manual_seed(11)
    qk = V.rnd(torch.randn(B, P, 2 * C, generator=g), "bf16")
    r = _scores(B, NH, P, C, "bf16", 2, inputs=(qk,), expect=PG_ERR_ARG)
    assert r["untouched"] and r["guards"]
    pvp = V.rnd(torch.softmax(torch.randn(B, NH, P, P, generator=g), -1), "bf16")
    vt = V.rnd(torch.randn(B, C, P, generator=g), "bf16")
    r = run_gemm_heads(pvp, 0, vt, 0, "bf16", P, 64, P, B, NH, P, NH * P * P, P * P, P, C * P, 64 * P, C, P * C, 64, form=2, expect=PG_ERR_ARG)
    assert r["untouched"] and r["guards"]
    C = NH * hd
    inputs = V.heads_inputs(B, NH, P, C, "bf16", hd)
    o2 = _scores(B, NH, P, C, "bf16", 2, hd=hd, inputs=inputs)
    o1 = _scores(B, NH, P, C, "bf16", 1, hd=hd, inputs=inputs)
    assert o1["guards"] and o2["guards"] and torch.equal(_bits(o1["out"]), _bits(o2["out"]))
    ref, mag = V.scores_ref(inputs[0], B, NH, P, C, hd)
    assert _report("scores hd=128 form 2 (25 x 8 blocks)", o2["out"].view(B, NH, P, P), ref, V.gemm_bound(ref, mag, hd, "f32")) <= 1.0
    Bb = V.T256_HEADS_BELOW[0]
    r = _scores(Bb, NH, P, C, "bf16", 2, hd=hd, inputs=(inputs[0][:Bb],), expect=PG_ERR_ARG)
    assert r["untouched"] and r["guards"]


# ------------------------------------------------------------------------------------------------------------------------------ lin() forms
@pytest.mark.parametrize("engine", ["bf16", "f32"])
@pytest.mark.parametrize("name", [c[0] for c in V.LIN_CASES])
def test_lin_forms(name, engine):
    """pg_engine::lin as SigLIP calls it: bias_n + fp32 residual with out == residual (x += proj(o), x += fc2(h)) at K = 1024 / 4096, bias_n + erf GELU at K = 1024."""
    from vq_ops import run_gemm_epi
    _, M, N, K, inplace, act, out_bf = next(c for c in V.LIN_CASES if c[0] == name)
    a, w, bias, res = V.lin_inputs(name, engine)
    ref, mag = V.lin_ref(name, engine)
    out_kind = out_bf if engine == "bf16" else "f32"
    o = run_gemm_epi(a, w, out_kind, M, N, K, 1, K, 0, K, 0, N, 0, bias_n=bias, residual=res, act=act, form=1 if engine == "bf16" else 0, engine=engine,
                     inplace=inplace)
    assert o["guards"] and o["nsplit"] == 0
    assert _report(f"lin {name} {M}x{N}x{K} {engine} inplace={inplace}", o["out"][0].float(), ref, V.gemm_bound(ref, mag, K, out_kind, act)) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_alone():
    from vision_ops import PG_ERR_ARG, run_layernorm, run_patchify, run_vq_argmin
    x, g, b = torch.randn(3, 512), torch.ones(512), torch.zeros(512)
    r = run_layernorm(x, g, b, 1, "f32", V.LN_EPS, expect=PG_ERR_ARG)          # form 1 names the wave kernel: C = 512 would run the generic one
    assert r["untouched"] and r["guards"]
    z, cb, _ = V.argmin_inputs(8, 256, 63)
    r = run_vq_argmin(torch.randn(63, 9), torch.randn(256, 9), 0, expect=PG_ERR_ARG)      # D = 9: zn[8] would overflow
    assert r["untouched"] and r["guards"]
    r = run_vq_argmin(z, cb, 1, expect=PG_ERR_ARG)                               # n = 63 < 64: the launcher would run the one-vector kernel
    assert r["untouched"] and r["guards"]
    r = run_vq_argmin(z, cb, 0, expect=PG_ERR_ARG, D=0)
    assert r["untouched"] and r["guards"]
    img = torch.zeros(1, 3, 40, 40)
    r = run_patchify(img, 16, "f32", "f32", expect=PG_ERR_ARG)                   # S % ps != 0
    assert r["untouched"] and r["guards"]


# ------------------------------------------------------------------------------------------------------------------------------ checker sensitivity
def test_perturbed_real_results_are_rejected():
    """The checkers on REAL kernel results: accepted as they are, rejected after one deliberate perturbation each."""
    from vision_ops import run_conv_in, run_layernorm, run_patchify, run_vq_argmin
    x, g, b = V.ln_inputs(6, 1024)
    ref, bound = V.ln_ref(x, g, b), V.ln_bound(x, g, b, "f32")
    out = run_layernorm(x, g, b, 1, "f32", V.LN_EPS)["out"]
    assert V.worst((out.to(F64) - ref).abs(), bound)[0] <= 1.0
    bad = out.clone()
    bad[5, 1023] += 3 * float(bound[5, 1023])                                   # one element, three bounds off
    assert V.worst((bad.to(F64) - ref).abs(), bound)[0] > 1.0
    bad = out.clone()
    bad[4], bad[5] = out[5], out[4]                                             # the last block's two rows swapped
    assert V.worst((bad.to(F64) - ref).abs(), bound)[0] > 1.0
    xi, w, bias = V.conv_in_inputs(2, 1, 65, 32, "f32")
    cref, cmag = V.conv_in_ref(xi, w, bias)
    cb_ = V.conv_in_bound(cref, cmag, "f32")
    got, _ = run_conv_in(xi, w, bias, "f32", "f32")
    assert V.worst((got.to(F64) - cref).abs(), cb_)[0] <= 1.0
    bad = got.clone()
    bad[:, :, 64] = got[:, :, 63]                                               # the second strip's only pixel repeats its neighbour
    assert V.worst((bad.to(F64) - cref).abs(), cb_)[0] > 1.0
    img = V.patch_image(32, 1, "bf16", "bf16")
    po = run_patchify(img, 16, "bf16", "bf16")["out"]
    want = V.patchify_ref(img, 16).to(torch.bfloat16)
    assert torch.equal(_bits(po), _bits(want))
    bad = po.clone()
    bad[0, 0], bad[0, 1] = po[0, 1], po[0, 0]
    assert not torch.equal(_bits(bad), _bits(want))
    z, cb, planted = V.argmin_inputs(8, 1000, 65)
    idx = run_vq_argmin(z, cb, 1)["idx"]
    assert V.argmin_check(idx, z, cb, planted)["ok"]
    lo, hi = V.dup_pairs(1000)[1]
    row = next(r for r, j in planted.items() if j == lo)
    bad = idx.clone()
    bad[row] = hi                                                               # the duplicate's higher index: same distance, wrong tie-break
    assert not V.argmin_check(bad, z, cb, planted)["ok"]
    bad = idx.clone()
    bad[1] = (int(idx[1]) + 1) % 1000                                           # a random row's neighbour code
    assert not V.argmin_check(bad, z, cb, planted)["ok"]
