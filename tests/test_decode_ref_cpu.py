"""CPU: the references of tests/decode_ref.py (used by tests/test_gpu_decode_ops.py) agree with each other within what their roundings allow,
the emulated deferred-1/rms arithmetic satisfies the K-rule on the GPU tests' own inputs (so the rule has room before a kernel is involved), and
the checks reject the layout mistakes the pair could make: every mutant of the emulation below must fail the bound the GPU test applies."""
import pytest
import torch

import decode_ref as D

F64 = torch.float64


@pytest.fixture(scope="module", params=D.GEMM_CASES, ids=lambda c: "M%d-N%d-S%d-Sn%d" % c)
def case(request):
    M, N, S, Sn = request.param
    x, partial, w = D.norm_inputs(M, Sn)
    W = D.gemm_weights(N)
    return dict(M=M, N=N, S=S, x=x, partial=partial, w=w, W=W, true=D.gemm_true(x, partial, w, W), emul=D.gemm_emul(x, partial, w, W, S),
                refbf=D.gemm_refbf(x, partial, w, W), absg=D.abs_gemm(x, partial, w, W))


def test_inputs_are_asymmetric():
    x, partial, w = D.norm_inputs(80, 8)
    xn = D.x_new_f32(x, partial)
    rms = xn.to(F64).pow(2).mean(-1).sqrt()
    assert rms[-8:].min() / rms[:8].max() > 1e4                                # the rows' scales span orders of magnitude
    q = D.ssq_ref(xn)
    for a in range(8):
        for b in range(a + 1, 8):
            r = q[:, a] / q[:, b]
            assert ((r > 1.2) | (r < 1 / 1.2)).float().mean() > 0.9, (a, b)    # two slots swapped show in (nearly) every row; the spike's own value is random
    for c in D.SPIKE_COLS:
        assert (xn[:, c].abs() > 0).all()
    assert D.SPIKE_COLS[0] < 1024 <= D.SPIKE_COLS[1]


def test_emulation_and_reference_bf16_are_within_their_roundings_of_the_truth(case):
    """|emul - true| <= u A (one bf16 rounding of the operand), |refbf - true| <= (2 u + u^2) A (two), A = sum_k |W| |w x_hat|; the fp32 slab fold
    and the fp32 statistics move either by at most (S + 3) 2^-24 A more (2^-18 A covers S <= 8 with room)."""
    u, slack = D.U_BF16, 2.0 ** -18
    e_emul = (case["emul"].sum(0) - case["true"]).abs()
    e_ref = (case["refbf"] - case["true"]).abs()
    assert (e_emul <= (u + slack) * case["absg"]).all(), float((e_emul / case["absg"]).max())
    assert (e_ref <= (2 * u + u * u + slack) * case["absg"]).all(), float((e_ref / case["absg"]).max())
    assert e_emul.max() > 0 and e_ref.max() > 0


def test_emulated_deferred_arithmetic_satisfies_the_k_rule(case):
    """E_def = |emul - true| against E_ref = |refbf - true|: one rounding against two, so the ratios sit near 1 / sqrt(2)."""
    ratios, bad = D.k_rule((case["emul"].sum(0) - case["true"]).abs(), (case["refbf"] - case["true"]).abs())
    print("E_def / E_ref:", {k: round(v, 3) for k, v in ratios.items()})
    assert not bad, bad


def test_slab_split_of_the_emulation_sums_to_the_whole(case):
    whole = D.gemm_emul(case["x"], case["partial"], case["w"], case["W"], 1)[0]
    torch.testing.assert_close(case["emul"].sum(0), whole, rtol=0, atol=1e-11 * float(whole.abs().max()))


def _slab_tol(ref):
    return 2e-4 * float(ref.abs().max()) + 1e-4


def test_gemm_check_rejects_a_wrong_row_scale(case):
    """rs[row] -> rs[0] of the 64-row block, and rows clamped one short: both leave the slab tolerance by orders of magnitude."""
    x, partial, w, W = case["x"], case["partial"], case["w"], case["W"]
    xn = D.x_new_f32(x, partial)
    raw = D.xw_emul(xn, w).to(F64) @ W.to(F64).t()
    rs = D.rs_f64(xn)
    ref = case["emul"].sum(0)
    blk0 = rs[(torch.arange(case["M"]) // 64) * 64]
    assert ((raw * blk0 - ref).abs().max() > 100 * _slab_tol(ref))
    shifted = torch.cat([rs[:1], rs[:-1]])
    assert ((raw * shifted - ref).abs().max() > 100 * _slab_tol(ref))


def test_ssq_check_rejects_a_permuted_slot_order():
    x, partial, w = D.norm_inputs(65, 4)
    q = D.ssq_ref(D.x_new_f32(x, partial))
    half, wave = torch.arange(8) // 4, torch.arange(8) % 4
    wrong = q[:, wave * 2 + half]                                               # (tid >> 6) * 2 + half in place of half * 4 + (tid >> 6)
    assert (((wrong - q).abs() > D.SSQ_RTOL * q).sum(-1) >= 4).all()


def test_swiglu_reference_matches_torch_on_separate_halves():
    import torch.nn.functional as F
    M, N2, Sn = D.SWIGLU_CASES[0]
    x, partial, w = D.norm_inputs(M, Sn)
    wg, wu = D.swiglu_weights(N2 // 2)
    y = D.gemm_true(x, partial, w, D.interleave_gate_up(wg, wu))
    a = D.pre_true(x, partial, w)
    want = F.silu(a @ wg.to(F64).t()) * (a @ wu.to(F64).t())
    torch.testing.assert_close(D.swiglu(y), want, rtol=1e-12, atol=1e-12)
    swapped = D.swiglu(D.gemm_true(x, partial, w, D.interleave_gate_up(wu, wg)))
    assert (swapped - want).abs().max() > 0.1 * want.abs().max()                # swapped halves are far outside 1e-2 max|ref|


def test_elementwise_references():
    g = torch.Generator().manual_seed(3)
    gu = torch.randn(5, 3, 32, generator=g)
    t = gu.to(F64).sum(0)
    for n in (0, 7, 8, 15):
        gcol, ucol = (n >> 3) * 16 + (n & 7), (n >> 3) * 16 + (n & 7) + 8
        want = t[:, gcol] * torch.sigmoid(t[:, gcol]) * t[:, ucol]
        torch.testing.assert_close(D.silu_mul_ref(gu)[:, n], want, rtol=1e-14, atol=0)
    p, b = torch.randn(4, 3, 10, generator=g), torch.randn(10, generator=g)
    v = p.to(F64).sum(0) + b.to(F64)
    torch.testing.assert_close(D.bias_act_ref(p, b, 1), torch.nn.functional.gelu(v), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(D.bias_act_ref(p, None, 0), p.to(F64).sum(0), rtol=0, atol=0)
    x = torch.randn(3, D.H, generator=g)
    part = torch.randn(9, 3, D.H, generator=g)
    assert ((D.x_new_f32(x, part).to(F64) - D.x_new_f64(x, part)).abs() <= D.slab_sum_bound(x, part)).all()
