"""CPU checks of tests/cfg_score_ref.py: the fp64 reference against torch.log_softmax of the mixed fp64 logits, the derived bound against an
fp32 evaluation (accepted) and against every mutant on the families the GPU test uses (rejected), and the index builder of
Engine.score_image against a brute-force loop."""
import numpy as np
import pytest
import torch

import cfg_score_ref as CR
import score_ref as SR
from plangen_amd.engine import image_score_index

V, K = 1000, 128          # one of the GPU test's shapes: 4 column tiles, the last one ragged
WEIGHTS = (0.0, 1.0, 5.0, -1.5)
TEMPS = (0.0, 0.5, 1.0, 3.0)


@pytest.fixture(scope="module")
def case():
    return CR.gaussian_pairs(129, V, K, seed=3)


def test_reference_is_log_softmax_of_the_mix(case):
    X, W, bias, target, cond, uncond = case
    Xr, Wr = SR.round_operand(X, "bf16").double(), SR.round_operand(W, "bf16").double()
    for w in WEIGHTS:
        for T in TEMPS:
            yc, yu = Xr[cond] @ Wr.T + bias.double(), Xr[uncond] @ Wr.T + bias.double()
            y = yu + w * (yc - yu)
            if T > 0:
                y = y * float(np.float32(1.0) / np.float32(T))
            want = torch.log_softmax(y, -1).gather(1, target.long()[:, None])[:, 0].numpy()
            lp64, bound = CR.cfg_head_logprob_ref(X, W, bias, target, cond, uncond, w, T)
            np.testing.assert_allclose(lp64, want, rtol=0, atol=1e-11)
            assert (bound > 0).all() and np.isfinite(bound).all()
    t2 = target.clone()
    t2[0], t2[1] = -1, V
    lp64, _ = CR.cfg_head_logprob_ref(X, W, None, t2, cond, uncond, 5.0, 1.0)
    assert (lp64[:2] == -np.inf).all() and np.isfinite(lp64[2:]).all()


@pytest.mark.parametrize("operand", ("bf16", "f32"))
@pytest.mark.parametrize("w", WEIGHTS)
def test_bound_accepts_fp32(case, w, operand):
    """The reference passes its own bound when evaluated in fp32, with and without bias, at every temperature."""
    X, W, bias, target, cond, uncond = case
    for T in TEMPS:
        for b in (bias, None):
            lp64, bound = CR.cfg_head_logprob_ref(X, W, b, target, cond, uncond, w, T, operand)
            lp = CR.fp32_eval(X, W, b, target, cond, uncond, w, T, operand)
            assert SR.within(lp, lp64, bound).all(), (w, T, SR.worst(lp, lp64, bound))


@pytest.mark.parametrize("n,V_,K_", [(129, 1000, 128), (300, 257, 64), (127, 256, 64)])
def test_mutants_are_rejected(n, V_, K_):
    X, W, bias, target, cond, uncond = CR.gaussian_pairs(n, V_, K_, seed=5)
    w, T = 5.0, 0.5
    yc, yu, Sc, Su = CR.terms64(X, W, bias, cond, uncond)
    lp64 = SR.lp_at(CR.mix64(yc, yu, w, T), target)
    bound = CR.bound_of(yc, yu, Sc, Su, target, lp64, K_, w, T)

    def rejected(lp):
        return not SR.within(lp, lp64, bound).all()
    assert not rejected(lp64)
    assert rejected(CR.mutant_swapped(yc, yu, w, T, target))
    assert rejected(CR.mutant_bias_dropped(yc, yu, w, T, target, bias))
    assert rejected(CR.mutant_bias_after_mix(yc, yu, w, T, target, bias))
    assert rejected(CR.mutant_c_plus(yc, yu, w, T, target))
    assert rejected(CR.mutant_temperature_one_side(yc, yu, w, T, target))
    # the two index lists exchanged at the call site, at the weight where the mix is the cond row alone
    l1, b1 = CR.cfg_head_logprob_ref(X, W, bias, target, cond, uncond, 1.0, T)
    assert not SR.within(CR.cfg_head_logprob_ref(X, W, bias, target, uncond, cond, 1.0, T)[0], l1, b1).all()


def test_image_score_index_against_a_loop():
    for L, T, R in ((20, 64, 6), (1, 1, 2), (5, 1, 4), (1, 7, 2), (256, 576, 8)):
        cond, uncond = image_score_index(L, T, R)
        Wd = L + T - 1
        want_c, want_u = [], []
        for b in range(R // 2):
            for j in range(T):
                want_c.append((2 * b) * Wd + L - 1 + j)
                want_u.append((2 * b + 1) * Wd + L - 1 + j)
        assert cond.dtype == torch.int64 and cond.tolist() == want_c and uncond.tolist() == want_u
        assert max(want_u) == R * Wd - 1                                  # the last row's last column: nothing past the tensor
    for L, T, R in ((20, 64, 5), (20, 64, 0), (0, 64, 2), (20, 0, 2), (20, 64, -2)):
        with pytest.raises(ValueError):
            image_score_index(L, T, R)


def test_hidden_column_L_plus_j_is_rejected():
    """The path's rule on a made-up hidden tensor: image token j is scored from column L - 1 + j; scoring it from column L + j must not pass."""
    L, T, R = 20, 16, 6
    Wd = L + T - 1
    g = torch.Generator().manual_seed(8)
    hidden = torch.randn(R * Wd + 1, 64, generator=g)                     # one spare row: the shifted index of the last column stays readable
    W = torch.randn(256, 64, generator=g) * (2.0 / 8.0)
    bias = torch.randn(256, generator=g)
    codes = torch.randint(0, 256, (R // 2, T), generator=g)
    cond, uncond = image_score_index(L, T, R)
    args = (5.0, 1.0)
    lp64, bound = CR.cfg_head_logprob_ref(hidden, W, bias, codes.reshape(-1), cond, uncond, *args)
    assert SR.within(CR.fp32_eval(hidden, W, bias, codes.reshape(-1), cond, uncond, *args), lp64, bound).all()
    wrong, _ = CR.cfg_head_logprob_ref(hidden, W, bias, codes.reshape(-1), cond + 1, uncond + 1, *args)
    assert not SR.within(wrong, lp64, bound).all()
