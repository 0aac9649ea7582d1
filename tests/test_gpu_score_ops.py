"""pg_op_head_logprob (the fused lm_head + log-softmax kernel of pg_score_tokens, on caller-given weights) against the fp64 reference and
derived bound of tests/score_ref.py: ragged shapes around the 256-row / 256-column tiles, row_idx forms, temperatures, out-of-range
targets, the real vocabulary, bit invariances, canaries and the workspace accounting."""
import ctypes as C

import numpy as np
import pytest
import torch

import score_ref as SR
from conftest import get_engine

pytestmark = pytest.mark.gpu

NS = (1, 5, 127, 128, 129, 255, 256, 257, 300)      # 128 +- 1 as the issue lists them, and the kernel's own row-tile height 256 +- 1
VS = (1, 17, 1000, 4099)
KS = (64, 2048)
TEMPS = (0.0, 0.7, 2.0)


@pytest.fixture(scope="module")
def eng(tiny_cfg, tiny_weights):
    return get_engine(tiny_cfg, tiny_weights, "bf16")


_W = {}


def weights(V, K):
    """One W per (V, K) for the whole module (and its upload)."""
    if (V, K) not in _W:
        g = torch.Generator().manual_seed(1000 + V * 7 + K)
        _W[(V, K)] = torch.randn(V, K, generator=g) * (2.0 / K ** 0.5)
    return _W[(V, K)]


def run_and_check(eng, X, W, target, row_idx, temperature, label):
    lp = eng.head_logprob(X, W, target, row_idx, temperature).cpu().numpy()
    lp64, bound = SR.head_logprob_ref(X, W, target, row_idx, temperature)
    err, frac = SR.worst(lp, lp64, bound)
    print(f"{label}: max |lp - lp64| = {err:.3e}, max error / bound = {frac:.3f}")
    ok = SR.within(lp, lp64, bound)
    assert ok.all(), (label, np.nonzero(~ok)[0][:8], lp[~ok][:8], lp64[~ok][:8])
    return lp


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("n", NS)
def test_shapes(eng, n, V, K):
    """Every (n, V, K); the row_idx form (identity / permutation / repeats with rows > n) and the temperature rotate over the grid, all nine
    combinations are met at one ragged shape in test_row_idx_and_temperature.  Targets at -1 and V give -inf."""
    case = NS.index(n) + VS.index(V) + KS.index(K)
    mode, temperature = case % 3, TEMPS[(case // 3) % 3]
    rows = n if mode == 0 else n + 7
    g = torch.Generator().manual_seed(n * 131 + V)
    X = torch.randn(rows, K, generator=g)
    if rows >= 2:
        X[rows - max(1, rows // 4):] *= 100.0            # logits of a few hundred
    W = weights(V, K)
    target = torch.randint(0, V, (n,), generator=g).int()
    if n >= 5:
        target[1], target[n - 2] = -1, V
    row_idx = None if mode == 0 else (torch.randperm(rows, generator=g)[:n] if mode == 1 else torch.randint(0, rows, (n,), generator=g))
    lp = run_and_check(eng, X, W, target, row_idx, temperature, f"n={n} V={V} K={K} mode={mode} T={temperature}")
    if n >= 5:
        assert lp[1] == -np.inf and lp[n - 2] == -np.inf


@pytest.mark.parametrize("temperature", TEMPS)
@pytest.mark.parametrize("mode", ("identity", "permutation", "repeats"))
def test_row_idx_and_temperature(eng, mode, temperature):
    n, V, K = 129, 1000, 64
    rows = n if mode == "identity" else 200
    X, W, target = SR.gaussian_case(n, V, K, seed=5, rows=rows)
    g = torch.Generator().manual_seed(9)
    row_idx = {"identity": None, "permutation": torch.randperm(rows, generator=g)[:n], "repeats": torch.randint(0, 5, (n,), generator=g) * 37}[mode]
    run_and_check(eng, X, W, target, row_idx, temperature, f"{mode} T={temperature}")


@pytest.mark.parametrize("V,K", [(1000, 64), (4099, 64), (4099, 2048)])
def test_spikes_at_tile_and_group_edges(eng, V, K):
    """A dominating logit at column 0, tile - 1, tile, the first and last column of every group and V - 1: scored on it and beside it."""
    X, W, target, cols = SR.spike_case(V, K, seed=3)
    geom = SR.geometry(len(target), V, K)
    assert cols == SR.edge_columns(V, geom)
    print(f"V={V} K={K}: G={geom['G']} cpt={geom['cpt']} edge columns {len(cols)}")
    for temperature in (0.0, 0.7):
        run_and_check(eng, X, W, target, None, temperature, f"spikes V={V} K={K} T={temperature}")


def test_blocks_that_walk_several_column_tiles(eng):
    """16 row tiles x 17 column tiles: more tiles than the group count is sized for, so a block owns TWO column tiles (the last group one,
    ragged) and carries its running maximum and sum across them; rows whose logits reach a few hundred, every temperature."""
    n, V, K = 3900, 4099, 64
    geom = SR.geometry(n, V, K)
    assert geom["cpt"] == 2 and geom["G"] == 9 and geom["ntm"] == 16
    X, W, target = SR.gaussian_case(n, V, K, seed=41)
    cols = SR.edge_columns(V, geom)
    for i, c in enumerate(cols):                                    # spikes on the group edges of THIS geometry, scored on and beside
        W[c] += 40.0 * X[2 * i] / (X[2 * i] @ X[2 * i])
        X[2 * i + 1] = X[2 * i]
        target[2 * i], target[2 * i + 1] = c, (c + 300) % V
    for temperature in TEMPS:
        run_and_check(eng, X, W, target, None, temperature, f"cpt=2 T={temperature}")


def test_real_vocabulary(eng):
    """V = 102 400, K = 2048, n = 3: spikes at column 0, at a middle group boundary and at 102 399; fp64 reference on the device."""
    n, V, K = 3, 102400, 2048
    geom = SR.geometry(n, V, K)
    mid = (geom["G"] // 2) * geom["cpt"] * SR.TILE
    cols = [0, mid, V - 1]
    g = torch.Generator().manual_seed(77)
    X = torch.randn(n, K, generator=g)
    W = torch.randn(V, K, generator=g) * (2.0 / K ** 0.5)
    for i, c in enumerate(cols):
        W[c] += 40.0 * X[i] / (X[i] @ X[i])
    for target in (torch.tensor(cols).int(), torch.tensor([mid - 1, V - 1, 1]).int()):      # on the spike, and beside it
        lp = eng.head_logprob(X, W, target).cpu().numpy()
        lp64, bound = SR.head_logprob_ref(X, W, target, device=eng.device)
        err, frac = SR.worst(lp, lp64, bound)
        print(f"V=102400 G={geom['G']} cpt={geom['cpt']} targets {target.tolist()}: max |lp - lp64| = {err:.3e}, error / bound = {frac:.3f}")
        assert SR.within(lp, lp64, bound).all(), (lp, lp64, bound)


def test_bit_invariance(eng):
    n, V, K, rows = 300, 4099, 64, 400
    X, W, target = SR.gaussian_case(n, V, K, seed=11, rows=rows)
    g = torch.Generator().manual_seed(12)
    row_idx = torch.randperm(rows, generator=g)[:n]
    a = eng.head_logprob(X, W, target, row_idx, 0.7)
    b = eng.head_logprob(X, W, target, row_idx, 0.7)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ"
    # the same rows in another order (same n): the output bits move with them
    perm = torch.randperm(n, generator=g)
    c = eng.head_logprob(X, W, target[perm], row_idx[perm], 0.7)
    assert torch.equal(c.view(torch.int32).cpu(), a.view(torch.int32).cpu()[perm]), "a row's bits depend on its slot"
    # rows row_idx does not name hold large finite garbage: nothing changes
    X2 = X.clone()
    unused = torch.ones(rows, dtype=torch.bool)
    unused[row_idx] = False
    X2[unused] = 3.0e4
    d = eng.head_logprob(X2, W, target, row_idx, 0.7)
    assert torch.equal(d.view(torch.int32), a.view(torch.int32)), "rows outside row_idx leak into the result"


def test_canaries_and_workspace(tiny_cfg, tiny_weights):
    """Floats on both sides of out stay untouched; pg_device_bytes grows by the partials workspace only: 2 * 4 * G * n rounded up to 256
    bytes, far below the 4 * n * V of materialised logits; a smaller call afterwards allocates nothing."""
    eng = get_engine(tiny_cfg, tiny_weights, "bf16", max_rows=4)        # its own handle: the workspace has never been allocated
    n, V, K = 300, 4099, 64
    X, W, target = SR.gaussian_case(n, V, K, seed=21)
    x = X.to(eng.device, torch.bfloat16).contiguous(); w = W.to(eng.device, torch.bfloat16).contiguous()
    t = target.to(eng.device)
    buf = torch.full((n + 64,), 1234.5, dtype=torch.float32, device=eng.device)
    out = buf[32:32 + n]
    before = eng.device_bytes()
    rc = eng.lib.pg_op_head_logprob(eng.h, C.c_void_p(x.data_ptr()), n, C.c_void_p(w.data_ptr()), V, K, None, C.c_void_p(t.data_ptr()), n,
                                    C.c_float(0.0), C.c_void_p(out.data_ptr()), eng.stream)
    assert rc == 0, eng.lib.pg_last_error(eng.h)
    torch.cuda.synchronize()
    grown = eng.device_bytes() - before
    geom = SR.geometry(n, V, K)
    assert geom["ws_bytes"] == (2 * 4 * geom["G"] * n + 255) // 256 * 256
    print(f"workspace {grown} bytes (G={geom['G']}), logits would be {4 * n * V}")
    assert grown == geom["ws_bytes"] and grown * 20 < 4 * n * V
    assert (buf[:32] == 1234.5).all() and (buf[32 + n:] == 1234.5).all()
    lp64, bound = SR.head_logprob_ref(X, W, target)
    assert SR.within(out.cpu().numpy(), lp64, bound).all()
    eng.head_logprob(X[:5], W, target[:5])
    assert eng.device_bytes() - before == grown


def test_errors_leave_the_handle_usable(eng):
    from plangen_amd.engine import PlanGenError
    X, W, target = SR.gaussian_case(5, 17, 64, seed=1)
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        eng.head_logprob(X[:, :48], W[:, :48], target)                  # K = 48: not a multiple of the K step
    with pytest.raises(PlanGenError, match="PG_ERR_ARG"):
        eng.head_logprob(X, W, target[:0])                              # n < 1
    x = X.to(eng.device, torch.bfloat16)
    assert eng.lib.pg_op_head_logprob(eng.h, C.c_void_p(x.data_ptr()), 5, None, 17, 64, None, None, 5, C.c_float(0.0), None, eng.stream) == -1
    assert b"null" in eng.lib.pg_last_error(eng.h)
    run_and_check(eng, X, W, target, None, 0.0, "after errors")
