"""CPU: the references, emulations, mutants and bounds of tests/vision_ref.py, which tests/test_gpu_vision_ops.py holds the understanding path's input-side kernels to.

(a) the float64 references agree with torch.nn.functional and, where it has the same operation, with oracle/ref_cpu.py (SigLIP's patch embedding + position
    embedding + LayerNorm; the quantiser's distance expression, restated from vq_encode, which does not expose it on its own);
(b) an fp32 emulation of each kernel's arithmetic, in its order, stays inside the bound on every GPU case, and every nearest-code case is decidable;
(c) every mutant reference leaves the bound on at least one case of its family: a bound that lets one through is too loose;
(d) the tile and edge arithmetic the case tables rely on."""
import pytest
import torch
import torch.nn.functional as F

import vision_ref as V

F64 = torch.float64


def _ratio(got, ref, bound):
    return V.worst((got.to(F64) - ref).abs(), bound)[0]


# ------------------------------------------------------------------------------------------------------------------------------ (a) pins
def test_layernorm_reference_matches_torch_float64():
    for M, C in [(5, 1000), (9, 1024), (5, 64)]:
        x, g, b = V.ln_inputs(M, C)
        want = F.layer_norm(x.to(F64), (C,), g.to(F64), b.to(F64), eps=V.LN_EPS)
        assert (V.ln_ref(x, g, b) - want).abs().max() < 1e-9             # rows of mean 100 sigma: 1e-16 x 100 x rstd
        assert torch.equal(V.ln_ref(x, g, b)[V.LN_CONST_ROW], b.to(F64))   # the constant row is beta exactly


@pytest.mark.parametrize("S,ps,B", V.PATCH_CASES)
def test_patchify_reference_matches_unfold_and_conv2d(S, ps, B):
    img = V.patch_image(S, B, "f32", "f32")
    ref = V.patchify_ref(img, ps)
    want = F.unfold(img, ps, stride=ps).transpose(1, 2).reshape(ref.shape)
    assert torch.equal(ref, want)
    w = torch.randn(5, 3, ps, ps, generator=torch.Generator().manual_seed(1)).to(F64)      # Conv2d(3, C, ps, stride ps) == patches . w^T
    conv = F.conv2d(img.to(F64), w, stride=ps).flatten(2).transpose(1, 2).reshape(-1, 5)
    assert (ref.to(F64) @ w.reshape(5, -1).t() - conv).abs().max() < 1e-6 * conv.abs().max()


def test_patchify_add_pos_layernorm_match_the_oracle_siglip_front_and_back():
    """oracle.ref_cpu.siglip_forward with zero blocks = LayerNorm(PatchEmbed(img) + pos_embed): the three references chained."""
    from oracle import ref_cpu as O
    g = torch.Generator().manual_seed(4)
    B, S, ps, C = 2, 32, 8, 40
    P = (S // ps) ** 2
    cfg = O.OracleCfg(vit_width=C, vit_layers=0, vit_heads=1, vit_patch=ps, vit_img=S)
    VT = "vision_model.vision_tower."
    W = {VT + "patch_embed.proj.weight": torch.randn(C, 3, ps, ps, generator=g).to(F64) / 14, VT + "patch_embed.proj.bias": torch.randn(C, generator=g).to(F64),
         VT + "pos_embed": torch.randn(1, P, C, generator=g).to(F64), VT + "norm.weight": 1 + 0.2 * torch.randn(C, generator=g).to(F64),
         VT + "norm.bias": torch.randn(C, generator=g).to(F64)}
    img = torch.randn(B, 3, S, S, generator=g).to(F64)
    img = img.float().to(F64)                                              # siglip_forward casts the image to fp32: feed it fp32-exact values
    x = F.conv2d(img, W[VT + "patch_embed.proj.weight"], W[VT + "patch_embed.proj.bias"], stride=ps).flatten(2).transpose(1, 2) + W[VT + "pos_embed"]
    want = F.layer_norm(x, (C,), W[VT + "norm.weight"], W[VT + "norm.bias"], eps=1e-6)
    got_o = O.siglip_forward({k: v.float() for k, v in W.items()}, cfg, img.float())
    patches = V.patchify_ref(img, ps)
    emb = patches @ W[VT + "patch_embed.proj.weight"].reshape(C, -1).t() + W[VT + "patch_embed.proj.bias"]
    emb = V.add_pos_ref(emb, W[VT + "pos_embed"][0], B)
    mine = V.ln_ref(emb, W[VT + "norm.weight"], W[VT + "norm.bias"], eps=1e-6).reshape(B, P, C)
    assert (mine - want).abs().max() < 1e-11
    assert (mine - got_o.to(F64)).abs().max() < 2e-5                      # the oracle runs in fp32


@pytest.mark.parametrize("B,H,W,Cout", V.CONV_IN_CASES[:4])
def test_conv_in_reference_matches_conv2d(B, H, W, Cout):
    x, w, bias = V.conv_in_inputs(B, H, W, Cout, "f32")
    ref, mag = V.conv_in_ref(x, w, bias)
    want = F.conv2d(x.to(F64), w.to(F64), bias.to(F64), padding=1).permute(0, 2, 3, 1)
    assert (ref - want).abs().max() < 1e-12 and bool((mag >= ref.abs() - 1e-12).all())


def test_quantiser_reference_matches_normalize_cdist_and_the_oracle_expression():
    z, cb, _ = V.argmin_inputs(8, 1000, 72)
    d, _ = V.argmin_dist(z, cb)
    zn = F.normalize(z.to(F64), dim=-1)
    assert (d - torch.cdist(zn, cb.to(F64)) ** 2).abs().max() < 1e-12
    # oracle.ref_cpu.vq_encode's lines, float64: sum(zf^2, 1, keepdim) + sum(emb^2, 1) - 2 einsum("bd,dn->bn", zf, emb.t())
    emb = cb.to(F64)
    d_o = torch.sum(zn ** 2, dim=1, keepdim=True) + torch.sum(emb ** 2, dim=1) - 2 * torch.einsum("bd,dn->bn", zn, emb.t().contiguous())
    assert (d - d_o).abs().max() < 1e-13
    assert torch.equal(V.argmin_ref(z, cb), torch.argmin(d_o, dim=1))
    x = V.l2_inputs(257, 8)
    assert (V.l2_ref(x) - F.normalize(x.to(F64), dim=-1)).abs().max() < 1e-15


def test_heads_references_match_scaled_dot_product_attention():
    """scores -> softmax -> P . V in the engine's layouts == F.scaled_dot_product_attention over [B, NH, P, 64]."""
    B, NH, P, C = 3, 2, 192, 128
    qk, _, vt = V.heads_inputs(B, NH, P, C, "f32")
    sc, _ = V.scores_ref(qk, B, NH, P, C)
    p = torch.softmax(sc / 8.0, -1)
    o, _ = V.pv_ref(p, vt, B, NH, P, C)
    q = qk[..., :C].to(F64).reshape(B, P, NH, 64).transpose(1, 2)
    k = qk[..., C:].to(F64).reshape(B, P, NH, 64).transpose(1, 2)
    v = vt.to(F64).transpose(1, 2).reshape(B, P, NH, 64).transpose(1, 2)
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * P, C)
    assert (o - want).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------ (b) emulations inside the bounds
@pytest.mark.parametrize("form,C,M", V.LN_CASES)
def test_layernorm_emulation_inside_bound(form, C, M):
    x, g, b = V.ln_inputs(M, C)
    ref = V.ln_ref(x, g, b)
    for out_kind in ("f32", "bf16"):
        bound = V.ln_bound(x, g, b, out_kind)
        assert _ratio(V.rnd(ref.float(), out_kind), ref, bound) <= 1.0          # the reference itself, rounded
        r = _ratio(V.ln_emul(x, g, b, form, out_kind), ref, bound)
        assert r <= 1.0, r
    if M > V.LN_CONST_ROW:                                                       # the constant row: beta to one rounding
        assert bool((V.ln_bound(x, g, b, "f32")[V.LN_CONST_ROW] <= 2 * V.U_F32 * b.abs().to(F64) + V.TINY).all())
        assert torch.equal(V.ln_emul(x, g, b, form, "f32")[V.LN_CONST_ROW], b)


@pytest.mark.parametrize("B,H,W,Cout", V.CONV_IN_CASES)
def test_conv_in_emulation_inside_bound(B, H, W, Cout):
    for in_kind, out_kind in V.CONV_IN_TYPES:
        x, w, bias = V.conv_in_inputs(B, H, W, Cout, in_kind)
        ref, mag = V.conv_in_ref(x, w, bias)
        bound = V.conv_in_bound(ref, mag, out_kind)
        assert _ratio(V.rnd(ref.float(), out_kind), ref, bound) <= 1.0
        r = _ratio(V.conv_in_emul(x, w, bias, out_kind), ref, bound)
        assert r <= 1.0, r


@pytest.mark.parametrize("D,V_,n", sorted({(D, Vv, n) for _, D, Vv, n in V.ARGMIN_CASES}))
def test_argmin_cases_are_decidable_and_the_emulation_is_accepted(D, V_, n):
    z, cb, planted = V.argmin_inputs(D, V_, n)
    m = V.argmin_margins(z, cb, planted)
    assert m and min(m.values()) > 1.0, m                                        # every planted row: margin > 2 x the accepted-index error
    ref = V.argmin_ref(z, cb)
    assert V.argmin_check(ref, z, cb, planted)["ok"]                             # the float64 answer is accepted, planted rows included
    res = V.argmin_check(V.argmin_emul(z, cb), z, cb, planted)
    assert res["ok"], res
    for lo, hi in V.dup_pairs(V_):
        assert torch.equal(cb[lo], cb[hi])
    assert planted[0] == V_ - 1 and (n < 12 or V.SHORT_CODE in planted.values())


@pytest.mark.parametrize("n,D", V.L2_CASES)
def test_l2norm_emulation_inside_bound(n, D):
    x = V.l2_inputs(n, D)
    assert _ratio(V.l2_emul(x), V.l2_ref(x), V.l2_bound(x)) <= 1.0
    if n > 1:
        assert bool((V.l2_emul(x)[n // 2] == 0).all())


@pytest.mark.parametrize("B,NH,P,C", V.HEADS_CASES + [V.HEADS_RAGGED])
def test_heads_emulation_inside_bound(B, NH, P, C):
    for dtype in ("bf16", "f32"):
        if dtype == "bf16" and P % 64:
            continue
        qk, p, vt = V.heads_inputs(B, NH, P, C, dtype)
        ref, mag = V.scores_ref(qk, B, NH, P, C)
        q = qk[..., :C].float().reshape(B, P, NH, 64).transpose(1, 2)
        k = qk[..., C:].float().reshape(B, P, NH, 64).transpose(1, 2)
        r, gaps = V.heads_check(q @ k.transpose(-1, -2), ref, mag, 64, "f32")
        assert r <= 1.0 and gaps, r
        ref, mag = V.pv_ref(p, vt, B, NH, P, C)
        o = (p.float() @ vt.float().reshape(B, NH, 64, P).transpose(-1, -2)).transpose(1, 2).reshape(B * P, C)
        r, gaps = V.heads_check(V.rnd(o, dtype), ref, mag, P, dtype)
        assert r <= 1.0 and gaps, r


@pytest.mark.parametrize("name", [c[0] for c in V.LIN_CASES])
def test_lin_emulation_inside_bound(name):
    _, M, N, K, inplace, act, out_bf = next(c for c in V.LIN_CASES if c[0] == name)
    from vq_ref import gemm_emul
    for dtype in ("bf16", "f32"):
        a, w, bias, res = V.lin_inputs(name, dtype)
        ref, mag = V.lin_ref(name, dtype)
        out_kind = out_bf if dtype == "bf16" else "f32"
        r = _ratio(gemm_emul(a, w, out_kind, bias_n=bias, res=res, act=act), ref, V.gemm_bound(ref, mag, K, out_kind, act))
        assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------------------------------------ (c) mutants leave the bounds
@pytest.mark.parametrize("mutant", ["unbiased", "no_eps", "pad256", "swap_gb", "row_xor1"])
def test_layernorm_mutants_are_rejected(mutant):
    hit = []
    for form, C, M in V.LN_CASES:
        x, g, b = V.ln_inputs(M, C)
        ref = V.ln_ref(x, g, b)
        for out_kind in ("f32", "bf16"):
            if _ratio(V.rnd(V.ln_ref(x, g, b, mutant=mutant).float(), out_kind), ref, V.ln_bound(x, g, b, out_kind)) > 1.0:
                hit.append((form, C, M, out_kind))
    assert hit, mutant
    forms = {h[0] for h in hit}
    assert forms == {0, 1} or mutant == "pad256", (mutant, hit)                 # both kernels' cases see it (pad256 changes nothing at C = 1024)


def test_index_map_mutants_are_rejected():
    for S, ps, B in V.PATCH_CASES:
        img = V.patch_image(S, B, "bf16", "bf16")
        for mutant in ("yx", "channel_last"):
            assert not torch.equal(V.patchify_ref(img, ps), V.patchify_ref(img, ps, mutant)), (S, ps, B, mutant)
        assert img.unique().numel() == img.numel() and img.to(torch.bfloat16).float().equal(img)      # distinct, and distinct as bf16
    assert V.patch_image(32, 1, "f32", "f32").to(torch.bfloat16).float().ne(V.patch_image(32, 1, "f32", "f32")).any()
    x, pos = V.add_pos_inputs(3, 9, 1000)
    assert not torch.equal(V.add_pos_ref(x, pos, 3), V.add_pos_ref(x, pos, 3, "row_div_b"))


@pytest.mark.parametrize("mutant", ["tap_t", "no_left_pad", "no_right_pad", "drop_last"])
def test_conv_in_mutants_are_rejected(mutant):
    hit = 0
    for B, H, W, Cout in V.CONV_IN_CASES:
        for in_kind, out_kind in V.CONV_IN_TYPES:
            x, w, bias = V.conv_in_inputs(B, H, W, Cout, in_kind)
            ref, mag = V.conv_in_ref(x, w, bias)
            bad, _ = V.conv_in_ref(x, w, bias, mutant)
            hit += _ratio(V.rnd(bad.float(), out_kind), ref, V.conv_in_bound(ref, mag, out_kind)) > 1.0
    assert hit >= len(V.CONV_IN_CASES), (mutant, hit)                            # well beyond one case; bf16 outputs included


@pytest.mark.parametrize("mutant", ["last_tie", "no_znorm", "v_floor256"])
def test_argmin_mutants_are_rejected(mutant):
    hit = []
    for D, V_, n in sorted({(D, Vv, n) for _, D, Vv, n in V.ARGMIN_CASES}):
        z, cb, planted = V.argmin_inputs(D, V_, n)
        if not V.argmin_check(V.argmin_ref(z, cb, mutant), z, cb, planted)["ok"]:
            hit.append((D, V_, n))
    assert hit, mutant
    if mutant == "last_tie":
        assert {(8, 1000, 63), (8, 1000, 64), (8, 100, 65)} <= set(hit), hit      # one-vector and eight-vector cases


@pytest.mark.parametrize("mutant", ["swap_levels", "stride2_rows"])
def test_heads_mutants_are_rejected(mutant):
    B, NH, P, C = V.HEADS_CASES[1]
    qk, p, vt = V.heads_inputs(B, NH, P, C, "bf16")
    ref, mag = V.pv_ref(p, vt, B, NH, P, C)
    bad, _ = V.pv_ref(p, vt, B, NH, P, C, mutant=mutant)
    r, gaps = V.heads_check(bad, ref, mag, P, "bf16")
    assert r > 1.0 or not gaps
    ref, mag = V.pv_ref(p, vt, B, NH, P, C, ldc=NH * V.HEADS_GAP, stride2=V.HEADS_GAP)
    bad, _ = V.pv_ref(p, vt, B, NH, P, C, ldc=NH * V.HEADS_GAP, stride2=V.HEADS_GAP, mutant=mutant)
    r, gaps = V.heads_check(bad, ref, mag, P, "bf16")
    assert r > 1.0 or not gaps
    if mutant == "swap_levels":
        ref, mag = V.scores_ref(qk, B, NH, P, C)
        bad, _ = V.scores_ref(qk, B, NH, P, C, mutant=mutant)
        assert V.heads_check(bad, ref, mag, 64, "f32")[0] > 1.0


# ------------------------------------------------------------------------------------------------------------------------------ (d) tile and edge arithmetic
def test_case_tables_reach_the_edges_they_name():
    # LayerNorm: which kernel a (C, ln_wave) selects; partly filled last blocks of the wave kernel
    assert [V.ln_form_of(C, 1) for C in (64, 512, 1000, 1024, 1152)] == [0, 0, 0, 1, 0] and V.ln_form_of(1024, 0) == 0
    assert all(C == 1024 for f, C, _ in V.LN_CASES if f == 1) and {C for f, C, _ in V.LN_CASES if f == 0} == {64, 128, 1000, 1024, 1152}
    assert [V.ln_rows_in_last_block(M) for f, _, M in V.LN_CASES if f == 1] == [1, 3, 4, 2, 1]
    assert any(C % 256 for _, C, _ in V.LN_CASES) and any(C < 256 for _, C, _ in V.LN_CASES)
    # patchify: K spans one or three 256-thread strides
    assert sorted({3 * ps * ps for _, ps, _ in V.PATCH_CASES}) == [192, 768]
    # conv_in: strips and the last strip's pixels
    assert [V.conv_in_strips(W) for W in (1, 63, 64, 65, 130)] == [(1, 1), (1, 63), (1, 64), (2, 1), (3, 2)]
    assert {c[2] for c in V.CONV_IN_CASES} == {1, 63, 64, 65, 130} and {c[1] for c in V.CONV_IN_CASES} == {1, 2, 5}
    assert {c[3] for c in V.CONV_IN_CASES} == {32, 128, 160} and {c[0] for c in V.CONV_IN_CASES} == {1, 2}
    # nearest code: the launcher's condition and the clamped slots
    assert [V.argmin_multi_taken(8, n) for n in (1, 63, 64, 65)] == [False, False, True, True] and not V.argmin_multi_taken(4, 64) and not V.argmin_multi_taken(8, 64, 0)
    assert [V.argmin_clamped_slots(n) for n in (64, 65, 71, 72)] == [0, 7, 1, 0]
    assert all(V.argmin_multi_taken(D, n) for f, D, _, n in V.ARGMIN_CASES if f == 1) and not any(V.argmin_multi_taken(D, n) for f, D, _, n in V.ARGMIN_CASES if f == 0)
    assert [v % 256 for v in V.ARGMIN_V] == [100, 0, 232, 0]
    # l2norm: blocks of 256 rows
    assert [(n + 255) // 256 for n, _ in V.L2_CASES] == [1, 2, 4]
    # heads GEMMs: what gemm256_try takes
    for B, NH, P, C in V.HEADS_CASES + [(25, 8, 256, 512)]:
        assert not V.gemm256_takes(P, P, 64, B * NH) and not V.gemm256_takes(P, 64, P, B * NH)
    B, NH, P, hd = V.T256_HEADS
    assert V.gemm256_takes(P, P, hd, B * NH) and B * NH == 200
    B, NH, P, hd = V.T256_HEADS_BELOW
    assert not V.gemm256_takes(P, P, hd, B * NH)
    for _, M, N, K, _, _, _ in V.LIN_CASES:
        assert not V.gemm256_takes(M, N, K, 1)                                  # the lin() cases stay on the 128 x 128 kernel under form 0 as well
