"""pg_op_cfg_head_logprob (the fused CFG-mixed gen_head + log-softmax kernel of pg_score_image_tokens, on caller-given operands) against the
fp64 reference and derived bound of tests/cfg_score_ref.py: pair counts around the 128-pair row tile, ragged vocabularies, the production
shape, edge-column and out-of-range targets, every guidance weight and temperature with and without bias, index-list forms, bit
invariances, canaries and the cross-check against the unguided head."""
import ctypes as C

import numpy as np
import pytest
import torch

import cfg_score_ref as CR
import score_ref as SR
from conftest import get_engine

pytestmark = pytest.mark.gpu

NS = (1, 3, 127, 128, 129, 300)           # 128 pairs make one row tile; 129 and 300 cross tiles
VKS = ((256, 64), (257, 64), (1000, 128))
WEIGHTS = (0.0, 1.0, 5.0, -1.5)
TEMPS = (0.0, 0.5, 1.0, 3.0)


@pytest.fixture(scope="module")
def eng(tiny_cfg, tiny_weights):
    return get_engine(tiny_cfg, tiny_weights, "bf16")


def edge_case(n, V, K, seed, with_bias=True):
    """gaussian_pairs with the edge columns as targets: pairs 2i and 2i + 1 read the same two rows, the cond row's logit at edge column c_i
    dominates (W[c_i] gets a multiple of that row added), pair 2i is scored ON c_i and pair 2i + 1 beside it; then -1 and V (out of range)."""
    X, W, bias, target, cond, uncond = CR.gaussian_pairs(n, V, K, seed, with_bias=with_bias)
    W = W.clone()
    cols = CR.edge_columns(n, V, K)
    k = 0
    for c in cols:
        if 2 * k + 1 >= n - 2:
            break
        cond[2 * k + 1], uncond[2 * k + 1] = cond[2 * k], uncond[2 * k]
        x = X[cond[2 * k]]
        W[c] += 8.0 * x / (x @ x)
        target[2 * k], target[2 * k + 1] = c, (c + V // 2 + 1) % V
        k += 1
    if n >= 3:
        target[n - 2], target[n - 1] = -1, V
    if n == 1:
        target[0] = V - 1
    return X, W, bias, target, cond, uncond


def run_and_check(eng, X, W, bias, target, cond, uncond, w, T, label, device="cpu"):
    lp = eng.cfg_head_logprob(X, W, bias, target, cond, uncond, w, T).cpu().numpy()
    lp64, bound = CR.cfg_head_logprob_ref(X, W, bias, target, cond, uncond, w, T, device=device)
    err, frac = SR.worst(lp, lp64, bound)
    print(f"{label}: max |lp - lp64| = {err:.3e}, max error / bound = {frac:.3f}")
    ok = SR.within(lp, lp64, bound)
    assert ok.all(), (label, np.nonzero(~ok)[0][:8], lp[~ok][:8], lp64[~ok][:8], bound[~ok][:8])
    return lp


@pytest.mark.parametrize("V,K", VKS)
@pytest.mark.parametrize("n", NS)
def test_shapes(eng, n, V, K):
    """Every (n, V, K) with edge-column and out-of-range targets; the guidance weight, the temperature and the bias rotate over the grid (all
    32 combinations are met at one ragged shape in test_weights_temperatures_bias)."""
    case = NS.index(n) * len(VKS) + VKS.index((V, K))
    w, T, with_bias = WEIGHTS[case % 4], TEMPS[(case // 4 + case) % 4], case % 3 != 0
    X, W, bias, target, cond, uncond = edge_case(n, V, K, seed=n * 131 + V, with_bias=with_bias)
    lp = run_and_check(eng, X, W, bias, target, cond, uncond, w, T, f"n={n} V={V} K={K} w={w} T={T} bias={with_bias}")
    if n >= 3:
        assert lp[n - 2] == -np.inf and lp[n - 1] == -np.inf


def test_production_shape(eng):
    """gen_head's own shape, V = 16 384 and K = 2048, at 129 pairs (two row tiles); fp64 reference on the device."""
    n, V, K = 129, 16384, 2048
    X, W, bias, target, cond, uncond = edge_case(n, V, K, seed=77)
    geom = SR.geometry(2 * n, V, K)
    print(f"V={V} K={K}: G={geom['G']} cpt={geom['cpt']} ntm={geom['ntm']}")
    lp = run_and_check(eng, X, W, bias, target, cond, uncond, 5.0, 1.0, "production shape", device=eng.device)
    assert lp[n - 2] == -np.inf and lp[n - 1] == -np.inf


@pytest.mark.parametrize("with_bias", (True, False))
def test_weights_temperatures_bias(eng, with_bias):
    n, V, K = 129, 1000, 128
    X, W, bias, target, cond, uncond = edge_case(n, V, K, seed=5, with_bias=with_bias)
    for w in WEIGHTS:
        for T in TEMPS:
            run_and_check(eng, X, W, bias, target, cond, uncond, w, T, f"bias={with_bias} w={w} T={T}")


def test_index_list_forms_and_bit_invariance(eng):
    n, V, K, rows = 300, 1000, 128, 400
    X, W, bias, target, cond, uncond = CR.gaussian_pairs(n, V, K, seed=11, rows=rows)
    g = torch.Generator().manual_seed(12)
    # one uncond row shared by many pairs (the batch-constant negative prompt), and pairs whose two indices name the same row
    shared = uncond.clone()
    shared[:200] = 7
    same = uncond.clone()
    same[::3] = cond[::3]
    for label, u in (("shared uncond row", shared), ("cond == uncond", same)):
        lp = run_and_check(eng, X, W, bias, target, cond, u, 5.0, 0.5, label)
    a = eng.cfg_head_logprob(X, W, bias, target, cond, uncond, 5.0, 0.5)
    b = eng.cfg_head_logprob(X, W, bias, target, cond, uncond, 5.0, 0.5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ"
    # the same pairs in another order (same n): the output bits move with them
    perm = torch.randperm(n, generator=g)
    c = eng.cfg_head_logprob(X, W, bias, target[perm], cond[perm], uncond[perm], 5.0, 0.5)
    assert torch.equal(c.view(torch.int32).cpu(), a.view(torch.int32).cpu()[perm]), "a pair's bits depend on its slot"
    # rows no index names hold large finite garbage: nothing changes
    X2 = X.clone()
    unused = torch.ones(rows, dtype=torch.bool)
    unused[cond] = False
    unused[uncond] = False
    assert unused.any()
    X2[unused] = 3.0e4
    d = eng.cfg_head_logprob(X2, W, bias, target, cond, uncond, 5.0, 0.5)
    assert torch.equal(d.view(torch.int32), a.view(torch.int32)), "rows outside the index lists leak into the result"


def test_canaries_and_workspace(tiny_cfg, tiny_weights):
    """Floats on both sides of out stay untouched; pg_device_bytes grows by the partials workspace only (8 * G * n bytes rounded up to 256)."""
    eng = get_engine(tiny_cfg, tiny_weights, "bf16", max_rows=2, max_images=1)        # a handle no other test uses: the workspace has never been allocated
    n, V, K = 300, 1000, 128
    X, W, bias, target, cond, uncond = CR.gaussian_pairs(n, V, K, seed=21)
    x = X.to(eng.device, torch.bfloat16).contiguous(); w = W.to(eng.device, torch.bfloat16).contiguous()
    b = bias.to(eng.device); t = target.to(eng.device)
    ci, ui = cond.int().to(eng.device), uncond.int().to(eng.device)
    buf = torch.full((n + 64,), 1234.5, dtype=torch.float32, device=eng.device)
    out = buf[32:32 + n]
    before = eng.device_bytes()
    rc = eng.lib.pg_op_cfg_head_logprob(eng.h, C.c_void_p(x.data_ptr()), X.shape[0], C.c_void_p(w.data_ptr()), V, K, C.c_void_p(b.data_ptr()),
                                        C.c_void_p(ci.data_ptr()), C.c_void_p(ui.data_ptr()), C.c_void_p(t.data_ptr()), n, C.c_float(5.0),
                                        C.c_float(1.0), C.c_void_p(out.data_ptr()), eng.stream)
    assert rc == 0, eng.lib.pg_last_error(eng.h)
    torch.cuda.synchronize()
    grown = eng.device_bytes() - before
    G = SR.geometry(2 * n, V, K)["G"]
    print(f"workspace {grown} bytes (G={G}), the two logit tensors would be {2 * 4 * n * V}")
    assert grown == (2 * 4 * G * n + 255) // 256 * 256
    assert (buf[:32] == 1234.5).all() and (buf[32 + n:] == 1234.5).all()
    lp64, bound = CR.cfg_head_logprob_ref(X, W, bias, target, cond, uncond, 5.0, 1.0)
    assert SR.within(out.cpu().numpy(), lp64, bound).all()


def test_weight_one_is_the_unguided_head(eng):
    """cfg_weight = 1 and no bias: the mix is the cond row, so the result lies within the sum of both bounds of Engine.head_logprob on the
    cond rows."""
    n, V, K = 300, 1000, 128
    X, W, _, target, cond, uncond = CR.gaussian_pairs(n, V, K, seed=31, with_bias=False)
    for T in (0.0, 0.5):
        a = eng.cfg_head_logprob(X, W, torch.zeros(V), target, cond, uncond, 1.0, T).cpu().numpy()
        h = eng.head_logprob(X, W, target, cond, T).cpu().numpy()
        _, ba = CR.cfg_head_logprob_ref(X, W, None, target, cond, uncond, 1.0, T)
        _, bh = SR.head_logprob_ref(X, W, target, cond, T)
        print(f"T={T}: max |cfg head - head| = {np.abs(a - h).max():.3e}, smallest allowance {float((ba + bh).min()):.3e}")
        assert (np.abs(a - h) <= ba + bh).all()


def test_errors_leave_the_handle_usable(eng):
    from plangen_amd.engine import PlanGenError
    X, W, bias, target, cond, uncond = CR.gaussian_pairs(5, 256, 64, seed=1)
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        eng.cfg_head_logprob(X[:, :48], W[:, :48], bias, target, cond, uncond)          # K = 48: not a multiple of the K step
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        eng.cfg_head_logprob(X, W, bias, target[:0], cond[:0], uncond[:0])              # n < 1
    with pytest.raises(PlanGenError, match="indices"):
        eng.cfg_head_logprob(X, W, bias, target, cond[:3], uncond)
    x = X.to(eng.device, torch.bfloat16)
    assert eng.lib.pg_op_cfg_head_logprob(eng.h, C.c_void_p(x.data_ptr()), 10, None, 256, 64, None, None, None, None, 5, C.c_float(5.0), C.c_float(1.0),
                                          None, eng.stream) == -1
    assert b"null" in eng.lib.pg_last_error(eng.h)
    run_and_check(eng, X, W, bias, target, cond, uncond, 5.0, 1.0, "after errors")
