"""CPU: the references, emulations and bounds of tests/vq_ref.py, which operator tests hold the VQ-decoder kernels to.

(a) the float64 references agree with torch.nn.functional in float64 and with the ResnetBlock / AttnBlock arithmetic of oracle/ref_cpu.py;
(b) a plain torch emulation of each operation in the production types stays inside the bound on every case's inputs;
(c) the same emulation with one named defect injected leaves the bound: a bound that lets one through is too loose."""
import math

import pytest
import torch
import torch.nn.functional as F

import vq_ref as R

F64 = torch.float64


def _ratio(got, ref, bound):
    return R.worst((got.to(F64) - ref).abs(), bound)[0]


# ------------------------------------------------------------------------------------------------------------------------------ (a) pins
def test_groupnorm_and_softmax_references_match_torch_float64():
    x, gamma, beta = R.gn_inputs(2, 65, 256, "f32")
    want = F.group_norm(x.to(F64).permute(0, 2, 1), 32, gamma.to(F64), beta.to(F64), eps=R.EPS).permute(0, 2, 1)
    assert (R.gn_ref(x, gamma, beta, 0) - want).abs().max() < 1e-11
    assert (R.gn_ref(x, gamma, beta, 1) - F.silu(want)).abs().max() < 1e-11
    s = R.softmax_inputs(5, 65, 512)
    assert (R.softmax_ref(s, 512 ** -0.5) - F.softmax(s.to(F64) * 512 ** -0.5, -1)).abs().max() < 1e-15


@pytest.mark.parametrize("name", ["s2odd", "s2even", "up96"])
def test_conv_reference_matches_torch_float64(name):
    case = R.case_by_name(name)
    x, w, bias, res = R.conv_inputs(name)
    xin = x.permute(0, 3, 1, 2).to(F64)
    if case[6]:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    want = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.to(F64), bias.to(F64), stride=2) if case[7] else F.conv2d(xin, w.to(F64), bias.to(F64), padding=1)
    ref, _ = R.conv_ref(name, "f32")
    assert tuple(ref.shape[1:3]) == R.out_hw(case)
    assert (ref - (want.permute(0, 2, 3, 1) + res.to(F64))).abs().max() < 1e-12


def test_references_match_the_oracle_resblock_and_attnblock():
    """ResnetBlock and AttnBlock of oracle/ref_cpu.py (float64 weights) rebuilt from vq_ref's pieces in the engine's layouts (NHWC, V^T, P . V)."""
    from oracle import ref_cpu as O
    g = torch.Generator().manual_seed(3)
    B, C, H, Wd = 2, 64, 5, 6
    HW = H * Wd
    W = {}
    for n in ("r.norm1", "r.norm2", "a.norm"):
        W[n + ".weight"], W[n + ".bias"] = (1 + 0.2 * torch.randn(C, generator=g)).to(F64), (0.3 * torch.randn(C, generator=g)).to(F64)
    for n in ("r.conv1", "r.conv2"):
        W[n + ".weight"], W[n + ".bias"] = (torch.randn(C, C, 3, 3, generator=g) / 24).to(F64), torch.randn(C, generator=g).to(F64)
    for n in ("a.q", "a.k", "a.v", "a.proj_out"):
        W[n + ".weight"], W[n + ".bias"] = (torch.randn(C, C, 1, 1, generator=g) / 8).to(F64), torch.randn(C, generator=g).to(F64)
    x = torch.randn(B, C, H, Wd, generator=g).to(F64) + 2.0
    xn = x.permute(0, 2, 3, 1).contiguous()                                 # NHWC

    def gn(name, t):
        return R.gn_ref(t.reshape(B, HW, C), W[name + ".weight"], W[name + ".bias"], 0, eps=1e-6).reshape(B, H, Wd, C)

    def conv(name, t):
        return R._conv(t, W[name + ".weight"], 0, 0, F64) + W[name + ".bias"]
    h = conv("r.conv1", R.swish64(gn("r.norm1", xn)))
    h = conv("r.conv2", R.swish64(gn("r.norm2", h)))
    assert ((xn + h).permute(0, 3, 1, 2) - O._resblock(W, "r", x)).abs().max() < 1e-11

    t1 = gn("a.norm", xn).reshape(B, HW, C)
    w2 = {n: W["a." + n + ".weight"].reshape(C, C) for n in ("q", "k", "v", "proj_out")}
    q, _ = R.gemm_ref(t1, w2["q"][None], bias_n=W["a.q.bias"])
    k, _ = R.gemm_ref(t1, w2["k"][None], bias_n=W["a.k.bias"])
    vt, _ = R.gemm_ref(w2["v"][None], t1, bias_m=W["a.v.bias"])             # [B, C, HW]
    sc, _ = R.gemm_ref(q, k)
    p = R.softmax_ref(sc, C ** -0.5)
    o, _ = R.gemm_ref(p, vt)
    out, _ = R.gemm_ref(o.reshape(1, B * HW, C), w2["proj_out"][None], bias_n=W["a.proj_out.bias"], res=xn.reshape(1, B * HW, C))
    assert (out.reshape(B, H, Wd, C).permute(0, 3, 1, 2) - O._attnblock(W, "a", x)).abs().max() < 1e-11


def test_gather_contract():
    table = torch.arange(12.0).reshape(4, 3)
    codes = R.gather_codes(8, 4)
    assert codes[:6].tolist() == [0, 3, -1, 4, -2 ** 31, 2 ** 31 - 1]
    assert R.gather_ref(table, codes)[:6, 0].tolist() == [0.0, 9.0, 0.0, 9.0, 0.0, 9.0]


# ------------------------------------------------------------------------------------------------------------------------------ (b) + (c) convolution
def _conv_cases():
    return [c[0] for c in R.HALO_CASES] + [R.T256_CASE[0]] + [c[0] for c in R.SMALL_CASES]


@pytest.mark.parametrize("name", _conv_cases())
def test_conv_emulation_inside_bound_and_statistics(name):
    case = R.case_by_name(name)
    halo = name.startswith("halo")
    combos = R.RES_OUT if halo else [("f32", "f32")]
    for res_kind, out_kind in combos:
        ref, bound = R.conv_ref(name, res_kind)
        stored, v = R.conv_emul(name, res_kind, out_kind)
        assert _ratio(stored, ref, bound + R.u_of(out_kind) * ref.abs()) <= 1.0, (res_kind, out_kind)
        if halo or name == "t256":
            th, tw = (8, 32) if halo else (1, 64)                           # t256: 64 consecutive pixels (W = 100 does not divide: flatten below)
            B, Ho, Wo, C = v.shape
            vv = v if halo else v.reshape(B, Ho * Wo // 64, 64, C)
            s, q = R.tile_partials(vv, th, tw)
            mean, rstd = R.finalize_emul(s, q, float(Ho * Wo * (C // 32)))
            n_split = th * tw * (C // 32)
            bounds = (R.stat_bounds(ref.reshape(B, Ho * Wo, C), B, Ho * Wo, C, n_split, bound.reshape(B, Ho * Wo, C)) if out_kind == "bf16"
                      else R.stat_bounds(stored.reshape(B, Ho * Wo, C), B, Ho * Wo, C, n_split))
            a, b = R.stats_err_ratio(mean, rstd, bounds)
            assert a <= 1.0 and b <= 1.0, (res_kind, out_kind, a, b)
    if name in ("s2odd", "s2even", "up96"):                                  # the fp32 engine on its own inputs
        ref, bound = R.conv_ref(name, "f32", "f32")
        assert _ratio(R.conv_emul(name, "f32", "f32", "f32")[0], ref, bound) <= 1.0


@pytest.mark.parametrize("out_kind", ["bf16", "f32"])
def test_conv_bound_rejects_seam_and_halo_defects(out_kind):
    """(1) at the first column of the second tile (x = 32) the tap (dy, dx) = (1, 0) reads its left neighbour's left neighbour; (2) on border column 0 the
    dx = 0 taps read the pixel the linear address wraps to (the last column) in place of the zero halo."""
    name = "halo128"
    x, w, bias, _ = R.conv_inputs(name)
    ref, bound = R.conv_ref(name, "f32")
    bound = bound + R.u_of(out_kind) * ref.abs()
    _, v = R.conv_emul(name, "f32", out_kind)
    assert _ratio(R.rnd(v, out_kind), ref, bound) <= 1.0
    seam = v.clone()
    seam[:, :, 32, :] += (x[:, :, 30, :] - x[:, :, 31, :]) @ w[:, :, 1, 0].t()
    assert _ratio(R.rnd(seam, out_kind), ref, bound) > 1.0
    wrap = v.clone()
    last = F.pad(x[:, :, -1, :], (0, 0, 1, 1))                               # [B, H + 2, Cin]: rows y - 1 .. y + 1 of the last column, zero above / below
    H = x.shape[1]
    for dy in range(3):
        wrap[:, :, 0, :] += last[:, dy:dy + H, :] @ w[:, :, dy, 0].t()
    assert _ratio(R.rnd(wrap, out_kind), ref, bound) > 1.0
    one = v.clone()                                                          # the same on ONE row of ONE image: localised defects must not average away
    one[1, 17, 32, :] = seam[1, 17, 32, :]
    assert _ratio(R.rnd(one, out_kind), ref, bound) > 1.0


@pytest.mark.parametrize("res_kind,out_kind", R.RES_OUT)
def test_conv_bound_rejects_small_localised_defects(res_kind, out_kind):
    """How tight the bound is: ONE pixel (image 1, row 17, column 32: the first column of a tile) whose 128 channels are off by a relative 1e-2 -- in turn the
    seam tap's contribution, the residual term of the epilogue (the epk 3 / 4 store), and the value as a whole -- must leave the bound at some channel.  With
    an fp32 output the bound is (K + 2) 2^-24 ~ 7e-5 of sum|a w| + |bias| + |res| (~1e-3 absolute here): a relative 1e-3 of the value or of the residual
    leaves it too.  Not claimed: 1e-2 of one of nine taps (~3e-3 absolute) under a bf16 store of values of magnitude 8 (2^-8 |ref| ~ 3e-2), and 1e-3 of a tap in fp32."""
    name = "halo128"
    x, w, _, _ = R.conv_inputs(name)
    ref, bound = R.conv_ref(name, res_kind)
    bound = bound + R.u_of(out_kind) * ref.abs()
    _, v = R.conv_emul(name, res_kind, out_kind)
    res = R.conv_residual(name, res_kind)
    tap = x[1, 17, 31, :] @ w[:, :, 1, 0].t()                                # what the tap (1, 0) adds at that pixel
    for eps in (1e-2,) + ((1e-3,) if out_kind == "f32" else ()):
        cands = {"tap": eps * tap, "value": eps * v[1, 17, 32, :]}
        if res is not None:
            cands["residual"] = eps * res[1, 17, 32, :]
        for what, delta in cands.items():
            bad = v.clone()
            bad[1, 17, 32, :] += delta
            if what == "tap" and (out_kind == "bf16" or eps < 1e-2):
                continue                                                     # not claimed (docstring)
            assert _ratio(R.rnd(bad, out_kind), ref, bound) > 1.0, (what, eps)


@pytest.mark.parametrize("out_kind", ["bf16", "f32"])
def test_conv_statistics_bound_rejects_a_swapped_group_partial(out_kind):
    """One tile's partial sums of one 4-channel group taken from the adjacent group."""
    name = "halo128"
    stored, v = R.conv_emul(name, "none", out_kind)
    B, H, W, C = v.shape
    ref, bound = R.conv_ref(name, "none")
    bounds = (R.stat_bounds(ref.reshape(B, H * W, C), B, H * W, C, 8 * 32 * 4, bound.reshape(B, H * W, C)) if out_kind == "bf16"
              else R.stat_bounds(stored.reshape(B, H * W, C), B, H * W, C, 8 * 32 * 4))
    s, q = R.tile_partials(v, 8, 32)
    cnt = float(H * W * 4)
    a, b = R.stats_err_ratio(*R.finalize_emul(s, q, cnt), bounds)
    assert a <= 1.0 and b <= 1.0
    s, q = s.clone(), q.clone()
    s[1, 37, 11], q[1, 37, 11] = s[1, 37, 12], q[1, 37, 12]
    a, b = R.stats_err_ratio(*R.finalize_emul(s, q, cnt), bounds)
    assert max(a, b) > 1.0, (a, b)


# ------------------------------------------------------------------------------------------------------------------------------ (b) + (c) GroupNorm
@pytest.mark.parametrize("in_kind,out_kind", R.GN_PAIRS)
@pytest.mark.parametrize("B,HW,C", R.GN_CASES)
def test_groupnorm_emulation_inside_bound(B, HW, C, in_kind, out_kind):
    x, gamma, beta = R.gn_inputs(B, HW, C, in_kind)
    per = -(-HW // R.gn_nsplit(HW))
    bounds = R.stat_bounds(x, B, HW, C, per * (C // 32))
    for sw in (0, 1):
        y, mean, rstd, _ = R.gn_emul(x, gamma, beta, sw, out_kind)
        a, b = R.stats_err_ratio(mean, rstd, bounds)
        assert a <= 1.0 and b <= 1.0, (sw, a, b)
        assert (mean[:, R.CONST_GROUP] == R.CONST_VALUE).all() and (rstd[:, R.CONST_GROUP] == torch.tensor(1.0 / math.sqrt(R.EPS), dtype=torch.float32)).all()
        assert _ratio(y, R.gn_ref(x, gamma, beta, sw), R.gn_out_bound(x, gamma, beta, sw, out_kind, bounds)) <= 1.0, sw


@pytest.mark.parametrize("defect", ["drop_split", "mean_early"])
@pytest.mark.parametrize("in_kind,out_kind", R.GN_PAIRS)
def test_groupnorm_bound_rejects_statistics_defects(in_kind, out_kind, defect):
    """One 64-pixel split dropped from the sums; the mean taken before the last split is added.  Both the statistics and the output must leave the bound."""
    B, HW, C = 2, 576, 512
    x, gamma, beta = R.gn_inputs(B, HW, C, in_kind)
    bounds = R.stat_bounds(x, B, HW, C, 64 * (C // 32))
    y, mean, rstd, _ = R.gn_emul(x, gamma, beta, 1, out_kind, defect=defect)
    a, b = R.stats_err_ratio(mean, rstd, bounds)
    assert max(a, b) > 1.0, (a, b)
    assert _ratio(y, R.gn_ref(x, gamma, beta, 1), R.gn_out_bound(x, gamma, beta, 1, out_kind, bounds)) > 1.0


# ------------------------------------------------------------------------------------------------------------------------------ (b) + (c) softmax
@pytest.mark.parametrize("out_kind", ["f32", "bf16"])
@pytest.mark.parametrize("rows,n,C", R.SOFTMAX_CASES)
def test_softmax_emulation_inside_bound(rows, n, C, out_kind):
    x = R.softmax_inputs(rows, n, C)
    scale = float(torch.tensor(1.0) / torch.sqrt(torch.tensor(float(C))))
    assert _ratio(R.softmax_emul(x, scale, out_kind), R.softmax_ref(x, scale), R.softmax_bound(x, scale, out_kind)) <= 1.0


@pytest.mark.parametrize("defect", ["lanes63", "bf16_scores"])
@pytest.mark.parametrize("out_kind", ["f32", "bf16"])
def test_softmax_bound_rejects_defects(out_kind, defect):
    """The normaliser summed over 63 of the 64 lanes; the scaled scores rounded to bf16 before the max is subtracted."""
    for rows, n, C in [(2 * 576, 576, 512), (4, 64, 128)]:
        x = R.softmax_inputs(rows, n, C)
        scale = float(torch.tensor(1.0) / torch.sqrt(torch.tensor(float(C))))
        assert _ratio(R.softmax_emul(x, scale, out_kind, defect), R.softmax_ref(x, scale), R.softmax_bound(x, scale, out_kind)) > 1.0, (rows, n)


# ------------------------------------------------------------------------------------------------------------------------------ (b) + (c) GEMMs
@pytest.mark.parametrize("engine", ["bf16", "f32"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("C,HW", R.ATTN_SHAPES)
def test_attnblock_gemm_emulation_inside_bound_and_defects_rejected(C, HW, batch, engine):
    d = R.attn_inputs(C, HW, batch, engine)
    ref, mag = R.gemm_ref(d["wv"][None], d["t1"], bias_m=d["bv"])
    bound = R.gemm_bound(ref, mag, C, engine)
    assert _ratio(R.gemm_emul(d["wv"][None], d["t1"], engine, bias_m=d["bv"]), ref, bound) <= 1.0
    assert _ratio(R.gemm_emul(d["wv"][None], d["t1"], engine, bias_m=d["bv"], defect="bias_m_as_n"), ref, bound) > 1.0
    ref, mag = R.gemm_ref(d["q"], d["k"])
    bound = R.gemm_bound(ref, mag, C, "f32")
    assert _ratio(R.gemm_emul(d["q"], d["k"], "f32"), ref, bound) <= 1.0
    if batch > 1:
        assert _ratio(R.gemm_emul(d["q"], d["k"], "f32", defect="stridec_row"), ref, bound) > 1.0
    ref, mag = R.gemm_ref(d["p"], d["vt"])
    assert _ratio(R.gemm_emul(d["p"], d["vt"], engine), ref, R.gemm_bound(ref, mag, HW, engine)) <= 1.0
    M = batch * HW
    ref, mag = R.gemm_ref(d["o"].reshape(1, M, C), d["wp"][None], bias_n=d["bp"], res=d["skip"].reshape(1, M, C))
    got = R.gemm_emul(d["o"].reshape(1, M, C), d["wp"][None], "f32", bias_n=d["bp"], res=d["skip"].reshape(1, M, C))
    assert _ratio(got, ref, R.gemm_bound(ref, mag, C, "f32")) <= 1.0


def test_256_tile_gemm_shapes_and_gelu_scale_emulation_inside_bound():
    """The batched 200-tile scores, proj_out at N = 256 with its statistics (64 rows x 8 channels per partial), and the act = 1 / scale != 1 cases."""
    C, HW, batch = R.T256_GEMM
    q, k, a, wp, bp, skip = R.t256_gemm_inputs()
    ref, mag = R.gemm_ref(q, k)
    assert _ratio(R.gemm_emul(q, k, "f32"), ref, R.gemm_bound(ref, mag, C, "f32")) <= 1.0
    ref, mag = R.gemm_ref(a[None], wp[None], bias_n=bp, res=skip[None])
    got = R.gemm_emul(a[None], wp[None], "f32", bias_n=bp, res=skip[None])
    assert _ratio(got, ref, R.gemm_bound(ref, mag, 256, "f32")) <= 1.0
    v = got.reshape(batch, HW // 64, 64, 256)
    sp, qp = R.tile_partials(v, 1, 64)
    bounds = R.stat_bounds(got.reshape(batch, HW, 256), batch, HW, 256, 64 * 8)
    x1, x2 = R.stats_err_ratio(*R.finalize_emul(sp, qp, float(HW * 8)), bounds)
    assert x1 <= 1.0 and x2 <= 1.0, (x1, x2)
    M, N, K, _ = R.GELU_CASE
    a, w, bn = R.gelu_inputs()
    for scale, act in R.GELU_SCALE_ACT:
        ref, mag = R.gemm_ref(a[None], w[None], bias_n=bn, scale=scale, act=act)
        bound = R.gemm_bound(ref, mag, K, "bf16", act, scale != 1.0)
        assert _ratio(R.gemm_emul(a[None], w[None], "bf16", bias_n=bn, scale=scale, act=act), ref, bound) <= 1.0, (scale, act)
        wrong = R.gemm_emul(a[None], w[None], "bf16", bias_n=bn, scale=scale, act=1 - act)       # the activation flag ignored / applied unasked
        assert _ratio(wrong, ref, bound) > 1.0, (scale, act)


@pytest.mark.parametrize("C,kind", R.GATHER_CASES)
def test_gather_reference_on_the_gpu_cases(C, kind):
    table, codes = R.gather_table(C, kind), R.gather_codes(R.GATHER_N, R.GATHER_VOCAB)
    want = torch.stack([table[min(max(int(c), 0), R.GATHER_VOCAB - 1)] for c in codes])
    assert torch.equal(R.gather_ref(table, codes), want)


# ------------------------------------------------------------------------------------------------------------------------------ (b) conv_out
@pytest.mark.parametrize("B,H,W", R.CONV_OUT_SMALL + R.CONV_OUT_HALO)
def test_conv_out_emulation_inside_bound(B, H, W):
    for Cout in (1, 3, 4):
        x, w, bias, gamma, beta = R.conv_out_inputs(B, H, W, Cout)
        y, _, _, coef = R.gn_emul(x.reshape(B, H * W, 128), gamma, beta, 1, "bf16")
        a = y.reshape(B, H, W, 128)
        ref, mag = R.conv_out_ref(a, w, bias)
        got = F.conv2d(a.permute(0, 3, 1, 2), w, bias, padding=1)
        for out_kind in ("f32", "bf16"):
            assert _ratio(R.rnd(got, out_kind), ref, R.dot_bound(mag, 9 * 128, ref, R.u_of(out_kind))) <= 1.0
        s64, ds = R.tail_operand(x, coef)                                    # the fused tail: the emulated operand against float64 of the same coefficients
        assert _ratio(a, s64, ds) <= 1.0
        ref4, mag4 = R.conv_out_ref(s64, w, bias)
        assert _ratio(got, ref4, R.dot_bound(mag4, 9 * 128, ref4, 0.0) + R.conv_out_err_term(ds, w)) <= 1.0
