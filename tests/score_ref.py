"""fp64 reference of the scoring head (include/plangen_hip.h, pg_score_tokens / pg_op_head_logprob), its derived error bound, the input
families that make the bound bite, and wrong versions of the definition ("mutants") which the comparison has to reject.

Definition, per scored row i (t = target[i], r = row_idx[i] or i):
    y_v = sum_k X[r][k] * W[v][k]                     operands in the compute dtype, fp32 accumulation on the device
    x   = y * (1 / temperature) when temperature > 0 (the fp32 inverse, as pg_request_token_logprobs), else y
    lp  = x[t] - (m + log sum_v exp(x_v - m)),  m = max_v x_v;   t outside [0, V): -inf
The reference works on the ROUNDED operands (bf16 for a bf16 engine) in fp64: logits64 = X64 . W64^T, scaled, log-softmax at the target.

Bound (derived, not measured).  bf16 x bf16 products are exact in fp32, so whatever order the device adds them in,
|y_v - y64_v| <= K * 2^-24 * S_v with S_v = sum_k |x_k| |w_vk| (K - 1 additions, each within 2^-24 relative of a partial sum that is at
most S_v in magnitude).  logsumexp is 1-Lipschitz in the sup norm and the target logit moves by its own error, hence
    bound_i = s * K * 2^-24 * (S_t + max_v S_v) + ATOL + RTOL * |lp64|,     s = max(1, 1 / temperature),
where ATOL / RTOL are tests/logprob_ref.py's bound for the exp / log evaluation (the fp32 scaling product's own rounding, 2^-23 |y| / T,
sits inside the first term: K >= 64).  fp32 operands (parity mode) round their products too: the standard dot-product bound
gamma_K = K u / (1 - K u), u = 2^-24, replaces K * 2^-24."""
import numpy as np
import torch

from logprob_ref import ATOL, RTOL

TILE = 256          # the kernel's row-tile height and column-tile width (plangen_amd.engine.head_logprob_geometry)
U = 2.0 ** -24


def round_operand(a, operand: str) -> torch.Tensor:
    a = torch.as_tensor(a, dtype=torch.float32)
    return a.bfloat16().float() if operand == "bf16" else a


def scaled_logits64(X, W, row_idx=None, temperature: float = 0.0, operand: str = "bf16", device="cpu"):
    """(x64 [n, V], S [n, V]) as torch float64 on ``device``: the scaled logits of the rounded operands and S_v = sum_k |x_k| |w_vk|."""
    X = round_operand(X, operand).to(device).double()
    W = round_operand(W, operand).to(device).double()
    if row_idx is not None:
        X = X[torch.as_tensor(np.asarray(row_idx), dtype=torch.long, device=device)]
    y = X @ W.T
    S = X.abs() @ W.abs().T
    if temperature > 0:
        y = y * float(np.float32(1.0) / np.float32(temperature))
    return y, S


def lp_at(x64: torch.Tensor, target) -> np.ndarray:
    """log-softmax of every row of x64 at its target, float64; a target outside [0, V) gives -inf."""
    n, V = x64.shape
    t = torch.as_tensor(np.asarray(target), dtype=torch.long, device=x64.device).reshape(-1)
    ok = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    m = x64.max(-1).values
    lse = m + torch.log(torch.exp(x64 - m[:, None]).sum(-1))
    lp = x64.gather(1, tc[:, None])[:, 0] - lse
    return torch.where(ok, lp, torch.full_like(lp, -np.inf)).cpu().numpy()


def bound_of(S: torch.Tensor, target, lp64: np.ndarray, K: int, temperature: float, operand: str = "bf16") -> np.ndarray:
    n, V = S.shape
    t = torch.as_tensor(np.asarray(target), dtype=torch.long, device=S.device).reshape(-1).clamp(0, V - 1)
    St = S.gather(1, t[:, None])[:, 0].cpu().numpy()
    Smax = S.max(-1).values.cpu().numpy()
    s = max(1.0, 1.0 / temperature) if temperature > 0 else 1.0
    acc = K * U if operand == "bf16" else K * U / (1.0 - K * U)
    with np.errstate(invalid="ignore"):
        rel = RTOL * np.where(np.isfinite(lp64), np.abs(lp64), 0.0)
    return s * acc * (St + Smax) + ATOL + rel


def head_logprob_ref(X, W, target, row_idx=None, temperature: float = 0.0, operand: str = "bf16", device="cpu"):
    """-> (lp64 float64 [n], bound float64 [n])."""
    x64, S = scaled_logits64(X, W, row_idx, temperature, operand, device)
    lp64 = lp_at(x64, target)
    return lp64, bound_of(S, target, lp64, int(torch.as_tensor(X).shape[-1]), temperature, operand)


def within(lp, lp64, bound) -> np.ndarray:
    """bool [n]: |lp - lp64| <= bound; infinities must agree exactly, NaN never passes."""
    lp, lp64 = np.asarray(lp, dtype=np.float64), np.asarray(lp64, dtype=np.float64)
    inf = np.isinf(lp64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(lp - lp64) <= bound
    return np.where(inf, lp == lp64, ok & np.isfinite(lp))


def worst(lp, lp64, bound):
    """(largest |lp - lp64|, largest |lp - lp64| / bound) over the finite entries: what the tests print before they assert."""
    lp, lp64 = np.asarray(lp, dtype=np.float64), np.asarray(lp64, dtype=np.float64)
    f = np.isfinite(lp64) & np.isfinite(lp)
    if not f.any():
        return 0.0, 0.0
    d = np.abs(lp[f] - lp64[f])
    return float(d.max()), float((d / bound[f]).max())


# ---------------------------------------------------------------------------------------------------------------- geometry / inputs
def geometry(n: int, V: int, K: int) -> dict:
    from plangen_amd.engine import head_logprob_geometry
    return head_logprob_geometry(n, V, K)


def edge_columns(V: int, geom: dict) -> list:
    """0, tile - 1, tile, the first and last column of every group, V - 1 (those that exist)."""
    cols = {0, TILE - 1, TILE, V - 1}
    for g in range(geom["G"]):
        first = g * geom["cpt"] * TILE
        last = min(V, (g + 1) * geom["cpt"] * TILE) - 1
        cols.update((first, last))
    return sorted(c for c in cols if 0 <= c < V)


def gaussian_case(n: int, V: int, K: int, seed: int, rows: int = None, big_rows: bool = True):
    """Gaussian X [rows, K] and W [V, K] with a gain that gives logits a spread of ~2 units; the last quarter of the rows is scaled so that
    their logits reach a few hundred (online rescale inside a group).  Random in-range targets."""
    g = torch.Generator().manual_seed(seed)
    rows = n if rows is None else rows
    X = torch.randn(rows, K, generator=g)
    W = torch.randn(V, K, generator=g) * (2.0 / K ** 0.5)
    if big_rows and rows >= 2:
        X[rows - max(1, rows // 4):] *= 100.0
    target = torch.randint(0, V, (n,), generator=g).int()
    return X, W, target


def spike_case(V: int, K: int, seed: int, cols=None, height: float = 40.0):
    """Two rows per edge column c whose logit at c dominates the row (W[c] gets height * x_i / |x_i|^2 added for both): one scored on
    target = c, one (the same hidden state) on a target != c.  A lost or duplicated column, tile or group moves these rows by far more than the bound.  Rows
    whose spike sits in the first / the last group put the row maximum there (rescale-on-merge).  -> X [n, K], W, target, cols."""
    g = torch.Generator().manual_seed(seed)
    if cols is None:
        n_guess = 2 * len(edge_columns(V, geometry(1, V, K)))
        cols = edge_columns(V, geometry(max(1, n_guess), V, K))
    n = 2 * len(cols)
    X = torch.randn(len(cols), K, generator=g).repeat_interleave(2, dim=0)      # the two rows of a pair carry the same hidden state
    W = torch.randn(V, K, generator=g) * (2.0 / K ** 0.5)
    target = torch.zeros(n, dtype=torch.int32)
    for i, c in enumerate(cols):
        x = X[2 * i]
        W[c] += height * x / (x @ x)
        target[2 * i] = c
        target[2 * i + 1] = (c + V // 2 + 1) % V
    return X, W, target, cols


# ---------------------------------------------------------------------------------------------------------------- mutants
def mutant_target_shift(x64, target):
    return lp_at(x64, np.asarray(target) + 1)


def mutant_row_idx_ignored(X, W, target, row_idx, temperature, operand="bf16"):
    n = len(np.asarray(target))
    x64, _ = scaled_logits64(X, W, np.arange(n), temperature, operand)
    return lp_at(x64, target)


def _masked(x64, keep_cols):
    x = torch.full_like(x64, -np.inf)
    x[:, keep_cols] = x64[:, keep_cols]
    return x


def mutant_last_tile_dropped(x64, target):
    V = x64.shape[1]
    keep = torch.arange(0, ((V - 1) // TILE) * TILE)
    return lp_at(_masked(x64, keep), target)


def mutant_group_dropped(x64, target, geom, g: int):
    V = x64.shape[1]
    lo, hi = g * geom["cpt"] * TILE, min(V, (g + 1) * geom["cpt"] * TILE)
    keep = torch.cat([torch.arange(0, lo), torch.arange(hi, V)])
    return lp_at(_masked(x64, keep), target)


def mutant_merge_without_rescale(x64, target, geom):
    """Every group's sum of exponentials is taken relative to its OWN maximum and the sums are added as they are."""
    n, V = x64.shape
    ms, ss = [], []
    for g in range(geom["G"]):
        lo, hi = g * geom["cpt"] * TILE, min(V, (g + 1) * geom["cpt"] * TILE)
        m = x64[:, lo:hi].max(-1).values
        ms.append(m); ss.append(torch.exp(x64[:, lo:hi] - m[:, None]).sum(-1))
    m = torch.stack(ms).max(0).values
    lse = m + torch.log(torch.stack(ss).sum(0))
    t = torch.as_tensor(np.asarray(target), dtype=torch.long).clamp(0, V - 1)
    return (x64.gather(1, t[:, None])[:, 0] - lse).numpy()


def mutant_no_temperature(X, W, target, row_idx, operand="bf16"):
    x64, _ = scaled_logits64(X, W, row_idx, 0.0, operand)
    return lp_at(x64, target)
