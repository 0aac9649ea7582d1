"""CPU checks of tests/score_ref.py: the fp64 reference against torch.log_softmax, the derived bound against an fp32 evaluation (accepted)
and against every mutant on the input families (rejected), and the index builder of Engine.score_text on hand-made rows."""
import numpy as np
import pytest
import torch

import score_ref as SR
from plangen_amd.engine import head_logprob_geometry, score_index

V, K = 1000, 64          # 4 column tiles, the last one ragged


def fp32_eval(X, W, target, row_idx=None, temperature=0.0):
    """What a correct device computes, up to summation order: fp32 GEMM of the bf16-rounded operands, fp32 log-softmax."""
    x = SR.round_operand(X, "bf16")
    if row_idx is not None:
        x = x[torch.as_tensor(np.asarray(row_idx), dtype=torch.long)]
    y = x @ SR.round_operand(W, "bf16").T
    if temperature > 0:
        y = y * (np.float32(1.0) / np.float32(temperature))
    lp = torch.log_softmax(y, -1)
    t = torch.as_tensor(np.asarray(target), dtype=torch.long)
    out = lp.gather(1, t.clamp(0, y.shape[1] - 1)[:, None])[:, 0]
    return torch.where((t >= 0) & (t < y.shape[1]), out, torch.full_like(out, -np.inf)).numpy()


@pytest.fixture(scope="module")
def spikes():
    X, W, target, cols = SR.spike_case(V, K, seed=3)
    return X, W, target, cols, SR.geometry(len(target), V, K)


def test_geometry():
    g = head_logprob_geometry(8192, 102400, 2048)
    assert (g["ntm"], g["ntn"], g["G"], g["cpt"]) == (32, 400, 8, 50) and g["ws_bytes"] == 2 * 4 * 8 * 8192
    for n, v in ((1, 1), (3, 102400), (300, 4099), (40960, 102400)):
        g = head_logprob_geometry(n, v, 64)
        assert g["G"] * g["cpt"] >= g["ntn"] > (g["G"] - 1) * g["cpt"], g        # every group owns at least one column tile
    assert head_logprob_geometry(300, 4099, 64) == head_logprob_geometry(300, 4099, 2048)


def test_reference_is_log_softmax():
    X, W, target = SR.gaussian_case(40, V, K, seed=1)
    for temperature in (0.0, 0.7, 2.0):
        x64, _ = SR.scaled_logits64(X, W, None, temperature)
        want = torch.log_softmax(x64, -1).gather(1, target.long()[:, None])[:, 0].numpy()
        np.testing.assert_allclose(SR.lp_at(x64, target), want, rtol=0, atol=1e-12)
    assert (SR.lp_at(x64, [-1, V] + [0] * 38)[:2] == -np.inf).all()


@pytest.mark.parametrize("temperature", (0.0, 0.7, 2.0))
def test_bound_accepts_fp32(spikes, temperature):
    X, W, target, _, _ = spikes
    for Xc, Wc, tc, ri in ((X, W, target, None),) + tuple((*SR.gaussian_case(60, V, K, seed=s, rows=80), torch.arange(79, 19, -1)) for s in (4, 5)):
        lp64, bound = SR.head_logprob_ref(Xc, Wc, tc, ri, temperature)
        lp = fp32_eval(Xc, Wc, tc, ri, temperature)
        assert SR.within(lp, lp64, bound).all(), SR.worst(lp, lp64, bound)


def test_spike_family_covers_the_edges(spikes):
    X, W, target, cols, geom = spikes
    assert geom["G"] >= 2 and {0, SR.TILE - 1, SR.TILE, V - 1} <= set(cols)
    x64, _ = SR.scaled_logits64(X, W)
    assert (x64.argmax(-1).numpy() == np.repeat(cols, 2)).all()           # the spike is the row maximum, in the first and in the last group too
    big, _ = SR.scaled_logits64(*SR.gaussian_case(40, V, K, seed=1)[:2])
    assert big[-1].abs().max() > 200                                      # rows that need the rescale inside a group


def test_mutants_are_rejected(spikes):
    X, W, target, cols, geom = spikes
    T = 0.7
    lp64, bound = SR.head_logprob_ref(X, W, target, None, T)
    x64, _ = SR.scaled_logits64(X, W, None, T)

    def rejected(lp):
        return not SR.within(lp, lp64, bound).all()
    assert not rejected(SR.lp_at(x64, target))
    assert rejected(SR.mutant_target_shift(x64, target))
    assert rejected(SR.mutant_last_tile_dropped(x64, target))
    for g in range(geom["G"]):
        assert rejected(SR.mutant_group_dropped(x64, target, geom, g)), g
    assert rejected(SR.mutant_merge_without_rescale(x64, target, geom))
    assert rejected(SR.mutant_no_temperature(X, W, target, None))
    # row_idx ignored: a case whose row_idx is not the identity
    Xg, Wg, tg = SR.gaussian_case(60, V, K, seed=4, rows=80)
    ri = torch.arange(79, 19, -1)
    l64, b = SR.head_logprob_ref(Xg, Wg, tg, ri, T)
    assert not SR.within(SR.mutant_row_idx_ignored(Xg, Wg, tg, ri, T), l64, b).all()


def test_score_index():
    L = 6
    sel = score_index(L, pad_len=[0, 2, 3], score_from=[1, 4, 6])
    assert sel.tolist() == [1, 2, 3, 4, 5, 6 + 4, 6 + 5]                   # row 2 (score_from == L) scores nothing
    assert score_index(L, [0], [6]).numel() == 0
    for pad, sf in (([2], [2]), ([0], [0]), ([1], [7]), ([0, 0], [1])):
        with pytest.raises(ValueError):
            score_index(L, pad, sf)


def test_hidden_j_instead_of_j_minus_1_is_rejected():
    """The path's rule on a made-up hidden tensor: column j is scored from hidden[j - 1]; scoring it from hidden[j] must not pass."""
    R, L = 3, 12
    g = torch.Generator().manual_seed(8)
    hidden = torch.randn(R * L, K, generator=g)
    W = torch.randn(V, K, generator=g) * (2.0 / K ** 0.5)
    ids = torch.randint(0, V, (R, L), generator=g)
    sel = score_index(L, [0, 3, 5], [1, 6, 7])
    target = ids.reshape(-1)[sel]
    lp64, bound = SR.head_logprob_ref(hidden, W, target, sel - 1)
    assert SR.within(fp32_eval(hidden, W, target, sel - 1), lp64, bound).all()
    wrong, _ = SR.head_logprob_ref(hidden, W, target, sel.clamp(max=R * L - 1))
    assert not SR.within(wrong, lp64, bound).all()
