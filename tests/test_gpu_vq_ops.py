"""GPU: operator tests of the VQ-16 decoder kernels in the forms pg_engine::vq_decode runs them, against the float64 references and the derived per-element
bounds of tests/vq_ref.py, through the operator entry points of the diagnostics library (plangen_amd/csrc/diag_ops.hip; bindings and guard bands:
tests/vq_ops.py), which call the PRODUCTION launchers with one kernel form pinned.

Every case asserts which kernel ran: forms that name one kernel return PG_ERR_ARG when that kernel's launcher declines, and the GroupNorm split count the
launcher reports is compared with the kernel's own ((H / 8)(W / 32) halo tiles, HW / 64 chunks of the 256-tile kernel, 0 for the 128 x 128 kernel).
Every comparison prints max err / bound and the worst flat index before it asserts (measurements for the record; no bound depends on them)."""
import math

import pytest
import torch

import vq_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _report(tag, got, ref, bound):
    r, i = R.worst((got.to(F64) - ref).abs(), bound)
    print(f"{tag}: max |err| / bound = {r:.3g} at flat index {i}")
    return r


def _check_stats(tag, res, tensor, n_split, elem_err=None):
    """tensor: the stored fp32 output read back, or (elem_err given: bf16 outputs, whose statistics are of the unrounded values) the float64 reference."""
    B, C = tensor.shape[0], tensor.shape[-1]
    HW = tensor.numel() // (B * C)
    bounds = R.stat_bounds(tensor.reshape(B, HW, C), B, HW, C, n_split, None if elem_err is None else elem_err.reshape(B, HW, C))
    a, b = R.stats_err_ratio(res["stats"][..., 0], res["stats"][..., 1], bounds)
    print(f"{tag}: statistics: mean err / bound = {a:.3g}, rstd offset / half interval = {b:.3g}")
    assert a <= 1.0 and b <= 1.0, (a, b)


# ------------------------------------------------------------------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("res_kind,out_kind", R.RES_OUT)
@pytest.mark.parametrize("name", [c[0] for c in R.HALO_CASES])
def test_conv3x3_halo_forms(name, res_kind, out_kind):
    """Cin = Cout = 128: the halo kernel with its fast epilogues (form 3: epk 0 / 1 / 3 / 4 and the generic one for fp32 -> bf16, bf16 -> fp32 and every residual
    under up = 1), its lock-step variant (form 4), the 128 x 128 implicit GEMM (form 1) and the production dispatch (form 0): each against float64 per element,
    all four bit-equal, and the GroupNorm statistics of the epilogue against the tensor it stored."""
    from vq_ops import run_conv3x3
    case = R.case_by_name(name)
    x, w, bias, _ = R.conv_inputs(name)
    res = R.conv_residual(name, res_kind)
    ref, dbound = R.conv_ref(name, res_kind)
    bound = dbound + R.u_of(out_kind) * ref.abs()
    want_gn = out_kind == "f32" or res_kind == "none"                          # fp32 outputs feed a GroupNorm; bf16 without residual is the mid_bf16 form
    Ho, Wo = R.out_hw(case)
    tiles = (Ho // 8) * (Wo // 32)
    outs = {}
    for form in (3, 4, 1, 0):
        o = run_conv3x3(x, w, bias, res, out_kind, res_kind, case[6], case[7], want_gn, form)
        assert o["nsplit"] == (tiles if want_gn and form != 1 else 0), (form, o["nsplit"], tiles)
        assert o["guards"], f"form {form}: a guard band or the workspace tail was written, or a partial-sum slot was not"
        r = _report(f"conv {name} res={res_kind} out={out_kind} form {form}", o["out"].float(), ref, bound)
        assert r <= 1.0, (form, r)
        if o["nsplit"]:
            if out_kind == "f32":
                _check_stats(f"conv {name} res={res_kind} out=f32 form {form}", o, o["out"], 8 * 32 * 4)
            else:
                _check_stats(f"conv {name} res={res_kind} out=bf16 form {form}", o, ref, 8 * 32 * 4, dbound)
        outs[form] = o["out"]
    for form in (4, 1, 0):
        assert torch.equal(_bits(outs[3]), _bits(outs[form])), f"form 3 and form {form} differ in bits"


def test_conv3x3_256_tile_with_partials():
    """The 256-tile kernel (form 2) on exactly 200 tiles with the GroupNorm partials of its epilogue switched on: nsplit = HW / 64, values per element,
    bit-equal to the 128 x 128 kernel, statistics against the stored tensor (a partial is 64 pixels x 8 channels)."""
    from vq_ops import run_conv3x3
    name = R.T256_CASE[0]
    case = R.case_by_name(name)
    x, w, bias, _ = R.conv_inputs(name)
    res = R.conv_residual(name, "f32")
    ref, bound = R.conv_ref(name, "f32")
    Ho, Wo = R.out_hw(case)
    o2 = run_conv3x3(x, w, bias, res, "f32", "f32", 0, 0, True, 2)
    assert o2["nsplit"] == Ho * Wo // 64 and o2["guards"], o2["nsplit"]
    assert _report(f"conv {name} form 2", o2["out"], ref, bound) <= 1.0
    _check_stats(f"conv {name} form 2", o2, o2["out"], 64 * (case[5] // 32))
    o1 = run_conv3x3(x, w, bias, res, "f32", "f32", 0, 0, True, 1)
    assert o1["nsplit"] == 0 and o1["guards"]
    assert torch.equal(_bits(o1["out"]), _bits(o2["out"]))
    o0 = run_conv3x3(x, w, bias, res, "f32", "f32", 0, 0, True, 0)          # production: the 256 tile without its partials (switch off by default)
    assert o0["nsplit"] == 0 and torch.equal(_bits(o0["out"]), _bits(o2["out"]))


@pytest.mark.parametrize("engine", ["bf16", "f32"])
@pytest.mark.parametrize("name", [c[0] for c in R.SMALL_CASES])
def test_conv3x3_small_shapes_fp32_output(name, engine):
    """Stride 2 (odd and even sides), Cin != Cout, ragged M / N, fp32 output with an fp32 residual on the 128 x 128 kernel and on the fp32 engine's
    gemm_f32_kernel<ConvLoaderB<float>>; the forms that name another kernel must refuse these shapes and leave the output alone."""
    from vq_ops import PG_ERR_ARG, run_conv3x3
    case = R.case_by_name(name)
    x, w, bias, _ = R.conv_inputs(name, engine)
    res = R.conv_residual(name, "f32")
    ref, bound = R.conv_ref(name, "f32", engine)
    o = run_conv3x3(x, w, bias, res, "f32", "f32", case[6], case[7], False, 1, engine)
    assert o["nsplit"] == 0 and o["guards"]
    assert _report(f"conv {name} {engine} form 1", o["out"], ref, bound) <= 1.0
    if engine == "bf16":
        for form in (2, 3):
            r = run_conv3x3(x, w, bias, res, "f32", "f32", case[6], case[7], False, form, engine, expect=PG_ERR_ARG)
            assert r["untouched"] and r["guards"], form


def test_conv3x3_refuses_what_the_loaders_exclude():
    from vq_ops import PG_ERR_ARG, run_conv3x3
    g = torch.Generator().manual_seed(0)
    for Cin, up, s2, Hi in [(96, 0, 0, 8), (32, 0, 0, 8), (64, 1, 1, 8), (64, 0, 1, 1)]:
        x = torch.randn(1, Hi, 8, Cin, generator=g)
        w = torch.randn(32, Cin, 3, 3, generator=g)
        r = run_conv3x3(x, w, torch.zeros(32), None, "f32", "f32", up, s2, False, 1, expect=PG_ERR_ARG)
        assert r["untouched"] and r["guards"], (Cin, up, s2, Hi)


# ------------------------------------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("in_kind,out_kind", R.GN_PAIRS)
@pytest.mark.parametrize("B,HW,C", R.GN_CASES)
def test_groupnorm(B, HW, C, in_kind, out_kind):
    """launch_gn_stats + launch_gn_apply, swish off and on: statistics against float64 of the input (cancellation-prone: group means up to 8 sigma from zero),
    the constant group exact, the output per element with the statistic error carried through; C = 96 takes the generic apply kernel."""
    from vq_ops import run_groupnorm
    x, gamma, beta = R.gn_inputs(B, HW, C, in_kind)
    per = -(-HW // R.gn_nsplit(HW))
    bounds = R.stat_bounds(x, B, HW, C, per * (C // 32))
    res = run_groupnorm(x, gamma, beta, in_kind, out_kind)
    for sw in (0, 1):
        o = res[sw]
        tag = f"groupnorm B={B} HW={HW} C={C} {in_kind}->{out_kind} swish={sw}"
        assert o["guards"], "a guard band or the workspace tail was written, or a partial-sum slot was not"
        a, b = R.stats_err_ratio(o["stats"][..., 0], o["stats"][..., 1], bounds)
        print(f"{tag}: mean err / bound = {a:.3g}, rstd offset / half interval = {b:.3g}")
        assert a <= 1.0 and b <= 1.0, (a, b)
        if HW * (C // 32) * 1 < 2 ** 24:                                       # the constant group: n m^2 < 2^24 with m = 1
            assert (o["stats"][:, R.CONST_GROUP, 0] == R.CONST_VALUE).all()
            assert (o["stats"][:, R.CONST_GROUP, 1] == torch.tensor(1.0 / math.sqrt(R.EPS), dtype=torch.float32)).all()
        ref = R.gn_ref(x, gamma, beta, sw)
        r = _report(tag, o["out"].float(), ref, R.gn_out_bound(x, gamma, beta, sw, out_kind, bounds))
        assert r <= 1.0, r


def test_groupnorm_refuses_what_the_kernels_exclude():
    """The entry point AND launch_gn_stats itself (raw): C / EPV > 256 would sum nothing and reduce unwritten LDS."""
    from vq_ops import PG_ERR_ARG, groupnorm_status
    for in_kind, out_kind, B, HW, C in [("f32", "f32", 1, 4, 2048), ("f32", "bf16", 1, 4, 1056), ("bf16", "f32", 1, 4, 64), ("f32", "f32", 1, 4, 48),
                                        ("f32", "f32", 1, 4, 16), ("bf16", "bf16", 1, 4, 4096), ("f32", "f32", 0, 4, 64), ("f32", "f32", 1, 0, 64)]:
        rc, untouched = groupnorm_status(in_kind, out_kind, B, HW, C)
        assert rc == PG_ERR_ARG and untouched, (in_kind, out_kind, B, HW, C, rc, untouched)
    for in_kind, B, HW, C in [("f32", 1, 4, 2048), ("f32", 1, 4, 1056), ("bf16", 1, 4, 4096), ("bf16", 1, 4, 2336), ("f32", 1, 4, 48), ("bf16", 1, 4, 100)]:
        rc, untouched = groupnorm_status(in_kind, "bf16", B, HW, C, raw=True)
        assert rc == PG_ERR_ARG and untouched, (in_kind, B, HW, C, rc, untouched)


# ------------------------------------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("out_kind", ["f32", "bf16"])
@pytest.mark.parametrize("rows,n,C", R.SOFTMAX_CASES)
def test_softmax_rows(rows, n, C, out_kind):
    from vq_ops import run_softmax
    x = R.softmax_inputs(rows, n, C)
    scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(C), dtype=torch.float32)))      # 1.0f / sqrtf((float)C)
    y, guards = run_softmax(x, scale, out_kind)
    assert guards, "rows past `rows` were written"
    r = _report(f"softmax rows={rows} n={n} C={C} {out_kind}", y.float(), R.softmax_ref(x, scale), R.softmax_bound(x, scale, out_kind))
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------------------------------------ AttnBlock GEMMs
@pytest.mark.parametrize("engine", ["bf16", "f32"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("C,HW", R.ATTN_SHAPES)
def test_attnblock_gemms(C, HW, batch, engine):
    """The four batched GEMMs as pg_engine::attnblock lays them out, on the 128 x 128 kernel (form 1; the fp32 engine: gemm_f32_kernel)."""
    from vq_ops import run_gemm_epi
    d = R.attn_inputs(C, HW, batch, engine)
    T = engine
    form = 1 if engine == "bf16" else 0
    # V^T[b] = Wv . t1[b]^T + bv[row]: A = the weight, broadcast (strideA = 0), B = t1, bf16 [C, HW] with ldc = HW
    o = run_gemm_epi(d["wv"], d["t1"], T, C, HW, C, batch, C, 0, C, HW * C, HW, C * HW, bias_m=d["bv"], form=form, engine=engine)
    ref, mag = R.gemm_ref(d["wv"][None], d["t1"], bias_m=d["bv"])
    assert o["guards"] and _report(f"V^T C={C} HW={HW} b={batch} {engine}", o["out"].float(), ref, R.gemm_bound(ref, mag, C, T)) <= 1.0
    # scores[b] = q[b] . k[b]^T, fp32, strideC = HW^2
    o = run_gemm_epi(d["q"], d["k"], "f32", HW, HW, C, batch, C, HW * C, C, HW * C, HW, HW * HW, form=form, engine=engine)
    ref, mag = R.gemm_ref(d["q"], d["k"])
    assert o["guards"] and _report(f"scores C={C} HW={HW} b={batch} {engine}", o["out"], ref, R.gemm_bound(ref, mag, C, "f32")) <= 1.0
    # o[b] = P[b] . V^T[b]^T: K = HW
    o = run_gemm_epi(d["p"], d["vt"], T, HW, C, HW, batch, HW, HW * HW, HW, C * HW, C, HW * C, form=form, engine=engine)
    ref, mag = R.gemm_ref(d["p"], d["vt"])
    assert o["guards"] and _report(f"P.V C={C} HW={HW} b={batch} {engine}", o["out"].float(), ref, R.gemm_bound(ref, mag, HW, T)) <= 1.0
    # proj_out over all images at once: bias_n, fp32 residual, fp32 out; the 128 x 128 kernel writes no partials (nsplit 0)
    M = batch * HW
    o = run_gemm_epi(d["o"].reshape(M, C), d["wp"], "f32", M, C, C, 1, C, 0, C, 0, C, 0, bias_n=d["bp"], residual=d["skip"].reshape(M, C),
                     gn_hw=HW if engine == "bf16" else 0, form=form, engine=engine)
    ref, mag = R.gemm_ref(d["o"].reshape(1, M, C), d["wp"][None], bias_n=d["bp"], res=d["skip"].reshape(1, M, C))
    assert o["nsplit"] == 0 and o["guards"]
    assert _report(f"proj_out C={C} HW={HW} b={batch} {engine}", o["out"], ref, R.gemm_bound(ref, mag, C, "f32")) <= 1.0


def test_attnblock_gemms_256_tile():
    """The 256-tile kernel (form 2) where it accepts the shape: batched scores sized to just reach 200 tiles (HW 256, batch 200), bit-equal to form 1; proj_out with
    the GroupNorm partials of its epilogue (M = 200 x 256 rows, N = 256: 200 tiles; nsplit = HW / 64); a shape below 200 tiles is refused."""
    from vq_ops import PG_ERR_ARG, run_gemm_epi
    C, HW, batch = R.T256_GEMM
    q, k, a, wp, bp, skip = R.t256_gemm_inputs()
    ref, mag = R.gemm_ref(q, k)
    o2 = run_gemm_epi(q, k, "f32", HW, HW, C, batch, C, HW * C, C, HW * C, HW, HW * HW, form=2)
    assert o2["guards"] and _report("scores form 2", o2["out"], ref, R.gemm_bound(ref, mag, C, "f32")) <= 1.0
    o1 = run_gemm_epi(q, k, "f32", HW, HW, C, batch, C, HW * C, C, HW * C, HW, HW * HW, form=1)
    assert torch.equal(_bits(o1["out"]), _bits(o2["out"]))
    r = run_gemm_epi(q[:199], k[:199], "f32", HW, HW, C, 199, C, HW * C, C, HW * C, HW, HW * HW, form=2, expect=PG_ERR_ARG)
    assert r["guards"] and bool(torch.isnan(r["out"]).all())
    # proj_out, N = 256
    C = 256
    M = batch * HW
    ref, mag = R.gemm_ref(a[None], wp[None], bias_n=bp, res=skip[None])
    o = run_gemm_epi(a, wp, "f32", M, C, C, 1, C, 0, C, 0, C, 0, bias_n=bp, residual=skip, gn_hw=HW, form=2)
    assert o["nsplit"] == HW // 64 and o["guards"], o["nsplit"]
    assert _report("proj_out form 2", o["out"], ref, R.gemm_bound(ref, mag, C, "f32")) <= 1.0
    _check_stats("proj_out form 2", o, o["out"].reshape(batch, HW, C), 64 * (C // 32))


def test_gemm_epilogue_gelu_and_scale():
    """act = 1 (erf GELU) and scale != 1: fields of the epilogue struct no VQ call sets, on the 128 x 128 kernel with ragged M / N and a padded ldc."""
    from vq_ops import run_gemm_epi
    M, N, K, ldc = R.GELU_CASE
    a, w, bn = R.gelu_inputs()
    for scale, act in R.GELU_SCALE_ACT:
        ref, mag = R.gemm_ref(a[None], w[None], bias_n=bn, scale=scale, act=act)
        o = run_gemm_epi(a, w, "bf16", M, N, K, 1, K, 0, K, 0, ldc, 0, bias_n=bn, scale=scale, act=act, form=1)
        assert o["guards"]
        assert _report(f"gemm scale={scale} act={act}", o["out"].float(), ref, R.gemm_bound(ref, mag, K, "bf16", act, scale != 1.0)) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------ conv_out
@pytest.mark.parametrize("engine", ["bf16", "f32"])
@pytest.mark.parametrize("Cout", [1, 3, 4])
@pytest.mark.parametrize("B,H,W", R.CONV_OUT_SMALL)
def test_conv_out_strip_kernel(B, H, W, Cout, engine):
    """conv3x3_small_kernel (form 1): one-pixel images, widths one short of / one past the 64-pixel strip, both engines, fp32 and bf16 NCHW output."""
    from vq_ops import run_conv_out
    x, w, bias, _, _ = R.conv_out_inputs(B, H, W, Cout, engine)
    a = R.rnd(x, engine)
    ref, mag = R.conv_out_ref(a, w, bias)
    for out_kind in ("f32", "bf16"):
        o = run_conv_out(a, w, bias, out_kind, 1, engine=engine)
        assert o["guards"]
        r = _report(f"conv_out strip {B}x{H}x{W} Cout={Cout} {engine}->{out_kind}", o["out"].float(), ref, R.dot_bound(mag, 9 * 128, ref, R.u_of(out_kind)))
        assert r <= 1.0, r


@pytest.mark.parametrize("Cout", [1, 3, 4])
@pytest.mark.parametrize("B,H,W", R.CONV_OUT_HALO)
def test_conv_out_halo_forms_and_fused_tail(B, H, W, Cout):
    """conv3x3_out2_kernel (form 2), conv3x3_out_halo_kernel (form 3) and the fused tail conv3x3_out_gn_kernel (form 4) fed the coefficients pg_diag_op_groupnorm
    produced: forms 2, 3, 4 bit-equal (and the strip kernel's values within the bound of the same reference); the fused tail against float64 with the
    kernel's own coefficients."""
    from vq_ops import run_conv_out, run_groupnorm
    x, w, bias, gamma, beta = R.conv_out_inputs(B, H, W, Cout)
    gn = run_groupnorm(x.reshape(B, H * W, 128), gamma, beta, "f32", "bf16", swishes=(1,))[1]
    a = gn["out"].float().reshape(B, H, W, 128)                              # the operand forms 2 / 3 multiply
    ref, mag = R.conv_out_ref(a, w, bias)
    s64, ds = R.tail_operand(x, gn["coef"])
    ref4, mag4 = R.conv_out_ref(s64, w, bias)
    extra4 = R.conv_out_err_term(ds, w)
    for out_kind in ("f32", "bf16"):
        outs = {}
        for form in (2, 3, 4):
            o = run_conv_out(x if form == 4 else a, w, bias, out_kind, form, coef=gn["coef"] if form == 4 else None)
            assert o["guards"], form
            outs[form] = o["out"]
        tag = f"conv_out {B}x{H}x{W} Cout={Cout} {out_kind}"
        assert _report(tag + " form 2", outs[2].float(), ref, R.dot_bound(mag, 9 * 128, ref, R.u_of(out_kind))) <= 1.0
        assert _report(tag + " form 4 (own coefficients)", outs[4].float(), ref4, R.dot_bound(mag4, 9 * 128, ref4, R.u_of(out_kind)) + extra4) <= 1.0
        assert torch.equal(_bits(outs[2]), _bits(outs[3])), "out2 and out_halo kernels differ in bits"
        assert torch.equal(_bits(outs[2]), _bits(outs[4])), "the fused tail differs in bits from gn_apply + conv_out"


@pytest.mark.parametrize("B,H,W", R.CONV_OUT_REFUSED)
def test_conv_out_try_refusals(B, H, W):
    """Sides that are no multiple of the tile, or fewer than 64 tiles: the *_try launchers decline, PG_ERR_ARG, output untouched."""
    from vq_ops import PG_ERR_ARG, run_conv_out
    x, w, bias, _, _ = R.conv_out_inputs(B, H, W, 3)
    coef = torch.ones(B, 128, 2)
    forms = (2, 3, 4) if (H % 8 or W % 32 or B * (H // 8) * (W // 32) < 64) else ()
    assert forms
    for form in forms:
        if form == 4 and H % 4 == 0 and W % 32 == 0 and B * (H // 4) * (W // 32) >= 64:
            continue                                                        # the fused tail's tile is 4 x 32: it takes this shape
        o = run_conv_out(x, w, bias, "f32", form, coef=coef if form == 4 else None, expect=PG_ERR_ARG)
        assert o["untouched"] and o["guards"], form


# ------------------------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("C,kind", R.GATHER_CASES)
def test_vq_gather_bit_exact_and_clamped(C, kind):
    from vq_ops import run_vq_gather
    table = R.gather_table(C, kind)
    codes = R.gather_codes(R.GATHER_N, R.GATHER_VOCAB)
    out, guards = run_vq_gather(table, codes, kind)
    assert guards
    assert torch.equal(_bits(out), _bits(R.gather_ref(table, codes).to(out.dtype)))
