"""CPU: the fp64 attention references of tests/attn_ref.py (used by tests/test_gpu_attention.py) are pinned to torch's own
scaled_dot_product_attention in float64, and the checker is shown to reject subtly wrong kernels: every mutant of the reference below
(the bug a kernel could have) must fail the bound on the random or the needle family, at the shapes the GPU tests launch."""
import pytest
import torch
import torch.nn.functional as F

import attn_ref as A

F64 = torch.float64


def _sdpa(q, k, v, mask=None, causal=False):
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, is_causal=causal, scale=1.0)


def _decode_with_shared_prefix():
    # rows 0..5 of which odd rows alias row 1's prompt of 40 slots; r0 = 2: the two-lane form, row 1 lives outside the launch
    return A.make_decode_case(3, "bf16", 2, [70, 45, 8, 45, 81, 45], S=5, n_dec=5, shared_len=40, r0=2, row_order="perm")


def test_decode_reference_equals_sdpa_over_two_caches():
    d = _decode_with_shared_prefix()
    ref = A.decode_ref(d, "bf16")
    for r in range(d["M"]):
        nprev, kstart = A.decode_positions(d["len"], d["n_dec"], d["shared_len"], [d["r0"] + i for i in range(d["M"])])[r]
        a = d["r0"] + r
        if (a & 1):
            assert kstart == d["shared_len"]
        K = torch.cat([d["kc"][1, :, :kstart], d["kc"][a, :, kstart:nprev]], 1).to(F64)
        V = torch.cat([d["vc"][1, :, :kstart], d["vc"][a, :, kstart:nprev]], 1).to(F64)
        pos = d["pos_off"][r] + nprev
        qs, ks, v_t = A.decode_qkv_new(d["qkv"], d["cos"], d["sin"], r, d["nh"], pos, "bf16")
        K = torch.cat([K, ks[0][:, None]], 1)
        V = torch.cat([V, v_t[:, None]], 1)
        q = A.f32(qs[0] * torch.tensor(d["scale"], dtype=torch.float32).item())
        o = _sdpa(q[:, None], K, V)[:, 0]
        torch.testing.assert_close(ref["out"][r], o, rtol=1e-12, atol=1e-12)


def test_decode_rope_and_slab_sum():
    """q, k: rotate_half RoPE of the exact slab sum at position pos_off + len + n_dec; v = round(sum)."""
    d = A.make_decode_case(5, "f32", 2, [7, 9], S=8, n_dec=0)
    HD = 2 * 128
    for r in range(2):
        a = d["qkv"][:, r].double().sum(0)
        assert torch.equal(a.float().double(), a)                       # the fp32 slab sum is exact in any order
        pos = d["pos_off"][r] + d["len"][r]
        c, s = d["cos"][pos].double(), d["sin"][pos].double()
        qs, ks, v = A.decode_qkv_new(d["qkv"], d["cos"], d["sin"], r, 2, pos, "f32")
        x = a[:HD].view(2, 128)
        want = torch.cat([x[:, :64] * c - x[:, 64:] * s, x[:, 64:] * c + x[:, :64] * s], 1)
        torch.testing.assert_close(qs[0], want, rtol=2 ** -22, atol=1e-7)
        assert torch.equal(v, a[2 * HD:].view(2, 128).float().double())


def test_prefill_reference_equals_sdpa_causal_and_left_padded():
    p = A.make_prefill_case(7, "f32", 2, lens=[1, 5, 64, 65, 130])
    ref = A.prefill_ref(p, "f32", flash=False)
    sc = torch.tensor(p["scale"], dtype=torch.float32).item()
    Lmax = max(L for L, o in zip(p["len"], p["row_off"]) if o >= 0)
    for r, (off, L) in enumerate(zip(p["row_off"], p["len"])):
        if off < 0:
            continue
        q = A.f32(p["q"][off:off + L].double() * sc).transpose(0, 1)
        K, V = p["kc"][r, :, :L].double(), p["vc"][r, :, :L].double()
        torch.testing.assert_close(ref["out"][off:off + L].transpose(0, 1), _sdpa(q, K, V, causal=True), rtol=1e-12, atol=1e-12)
        # the same row left-padded to the longest row: pad keys masked, causal over the real tokens
        pad = Lmax - L
        qp = torch.cat([torch.zeros(2, pad, 128, dtype=F64), q], 1)
        Kp = torch.cat([torch.full((2, pad, 128), 9.0, dtype=F64), K], 1)
        Vp = torch.cat([torch.full((2, pad, 128), 9.0, dtype=F64), V], 1)
        i = torch.arange(Lmax)
        mask = (i[None, :] <= i[:, None]) & (i[None, :] >= pad)
        mask[:pad, :] = True                                          # pad queries: any finite row (discarded)
        o = _sdpa(qp, Kp, Vp, mask=mask)[:, pad:]
        torch.testing.assert_close(ref["out"][off:off + L].transpose(0, 1), o, rtol=1e-12, atol=1e-12)


def test_vit_reference_equals_sdpa_non_causal():
    v = A.make_vit_case(9, 2, 128, 128, 2)
    ref = A.vit_ref(v["qk"], v["vt"], 2, 128, 128, 2, v["scale"])
    x = v["qk"].double().view(2, 128, 2, 2, 64)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    vv = v["vt"].double().view(2, 2, 64, 128).transpose(2, 3)
    o = _sdpa(q * v["scale"], k, vv).permute(0, 2, 1, 3).reshape(256, 128)
    torch.testing.assert_close(ref["out"], o, rtol=1e-12, atol=1e-12)


def test_checker_accepts_the_rounded_reference():
    d = _decode_with_shared_prefix()
    ref = A.decode_ref(d, "bf16")
    ok, mx, _ = A.check(A.round_t(ref["out"], "bf16"), ref["out"], A.decode_bound(ref, "bf16"))
    assert ok, mx


# ---------------------------------------------------------------------------------------------------------- checker power: decode
DECODE_MUTANTS = [("no_new_key",), ("share_shift", 1), ("share_shift", -1), ("rope_pos", 1), ("rope_pos", -1), ("drop_slab", 0),
                  ("drop_slab", 3), ("v_head", 1)]


def _decode_fails(cases, dtype, mut):
    for d in cases:
        ref = A.decode_ref(d, dtype)
        bad = A.decode_ref(d, dtype, mut)
        ok, mx, _ = A.check(A.round_t(bad["out"], dtype), ref["out"], A.decode_bound(ref, dtype))
        if not ok:
            return mx
    return None


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_decode_checker_rejects_every_mutant(dtype):
    cases = [A.decode_counts_case(dtype, 16, S=4, order="lpt", needle=nd) for nd in (False, True)]
    cases += [A.decode_shared_case(dtype, 2, 40, 6, S=4, r0=2, needle=nd) for nd in (False, True)]
    muts = list(DECODE_MUTANTS)
    for form in (4, 8):
        _, kpw, ch = A.decode_geometry(dtype, form)
        muts += [("drop_key", kpw - 1), ("drop_key", kpw), ("drop_key", ch - 1), ("drop_key", ch)]
    for mut in muts:
        assert _decode_fails(cases, dtype, mut) is not None, mut


# ---------------------------------------------------------------------------------------------------------- checker power: prefill
@pytest.mark.parametrize("dtype,flash", [("bf16", True), ("bf16", False), ("f32", False)])
def test_prefill_checker_rejects_every_mutant(dtype, flash):
    cases = [A.make_prefill_case(11, dtype, 2, needle=nd) for nd in (False, True)]
    refs = [A.prefill_ref(p, dtype, flash) for p in cases]
    for mut in [("causal", 1), ("causal", -1), ("drop_key", 63), ("drop_key", 64), ("drop_key", 127), ("drop_key", 128), ("v_head", 1)]:
        failed = False
        for p, ref in zip(cases, refs):
            bad = A.prefill_ref(p, dtype, flash, mut)
            ok, _, _ = A.check(A.round_t(bad["out"], dtype), ref["out"], A.prefill_bound(ref, dtype, flash))
            failed |= not ok
        assert failed, mut


def test_prefill_flash_bound_is_five_times_tighter_than_five_percent_of_max():
    p = A.make_prefill_case(11, "bf16", 2)
    ref = A.prefill_ref(p, "bf16", True)
    b = A.prefill_bound(ref, "bf16", True)
    assert float(b.max()) <= 0.01 * float(ref["out"].abs().max())


def test_vit_checker_rejects_mutants():
    cases = [A.make_vit_case(13, 1, 192, 128, 2, needle=nd) for nd in (False, True)]
    for mut in [("drop_key", 63), ("drop_key", 64), ("v_head", 1)]:
        failed = False
        for v in cases:
            ref = A.vit_ref(v["qk"], v["vt"], 1, 192, 128, 2, v["scale"])
            bad = A.vit_ref(v["qk"], v["vt"], 1, 192, 128, 2, v["scale"], mut)
            ok, _, _ = A.check(A.round_t(bad["out"], "bf16"), ref["out"], A.vit_bound(ref))
            failed |= not ok
        assert failed, mut
