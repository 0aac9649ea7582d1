"""fp64 reference of the CFG scoring head (include/plangen_hip.h, pg_score_image_tokens / pg_op_cfg_head_logprob), its derived error bound
and wrong versions of the definition ("mutants") which the comparison has to reject.

Definition, per scored position i (c = cond_idx[i], u = uncond_idx[i], t = target[i], w = cfg_weight):
    yc_v = sum_k X[c][k] W[v][k] + bias[v],  yu_v likewise       operands in the compute dtype, fp32 accumulation on the device
    y_v  = yu_v + w * (yc_v - yu_v)                               fp32 on the device
    x    = y * (1 / temperature) when temperature > 0 (the fp32 inverse), else y
    lp   = x[t] - (m + log sum_v exp(x_v - m)),  m = max_v x_v;   t outside [0, V): -inf
The reference evaluates this in fp64 on the ROUNDED operands (bf16 for a bf16 engine; the bias and w are fp32 values on both sides).

Bound (derived, not measured), built on tests/score_ref.py's argument.  With u = 2^-24 and S_v = sum_k |x_k| |w_vk|:
  * accumulation: |acc - acc64| <= A * S_v, A = K u for bf16 operands (exact products), gamma_K = K u / (1 - K u) for fp32 operands;
  * the bias addition rounds once: |yc - yc64| <= A Sc_v + u |yc_v|, the same for yu;
  * the mix is linear, y = (1 - w) yu + w yc, so it carries |w| of the cond error and |1 - w| of the uncond error; its own operations
    round the difference d = yc - yu (u |d|, amplified by |w|), the product w d (u |w d|) and the sum (u |y|) -- a fused multiply-add
    drops the middle one;
  * the scaling multiplies all of that by 1 / temperature (<= s = max(1, 1 / temperature), score_ref's factor) and rounds once (u |x|).
To first order in u (the second-order terms are below 2^-40 relative and sit inside ATOL):
    |x_v - x64_v| <= s A (|w| Sc_v + |1 - w| Su_v) + s M_v + u |x_v|,
    M_v = u (|w| (|yc_v| + 2 |yc_v - yu_v|) + |1 - w| |yu_v| + |y_v|).
logsumexp is 1-Lipschitz in the sup norm and the target logit moves by its own error, hence
    bound_i = s A (|w| (Sc_t + max_v Sc_v) + |1 - w| (Su_t + max_v Su_v)) + [s (M_t + max_v M_v) + u (|x_t| + max_v |x_v|)] + ATOL + RTOL |lp64|
with ATOL / RTOL tests/logprob_ref.py's bound for the exp / log evaluation.  No constant of this file is chosen by hand."""
import numpy as np
import torch

import score_ref as SR
from logprob_ref import ATOL, RTOL

U = SR.U
PAIRS = SR.TILE // 2          # pairs per row tile of the kernel


def _idx(a, device):
    return torch.as_tensor(np.asarray(a), dtype=torch.long, device=device).reshape(-1)


def terms64(X, W, bias, cond_idx, uncond_idx, operand: str = "bf16", device="cpu"):
    """(yc, yu, Sc, Su) float64 [n, V]: both logit tensors of the rounded operands (bias included) and their S_v = sum_k |x_k| |w_vk|."""
    X = SR.round_operand(X, operand).to(device).double()
    W = SR.round_operand(W, operand).to(device).double()
    b = torch.zeros(W.shape[0], dtype=torch.float64, device=device) if bias is None else torch.as_tensor(bias, dtype=torch.float32).to(device).double()
    Xc, Xu = X[_idx(cond_idx, device)], X[_idx(uncond_idx, device)]
    return Xc @ W.T + b, Xu @ W.T + b, Xc.abs() @ W.abs().T, Xu.abs() @ W.abs().T


def inv_t(temperature: float) -> float:
    return float(np.float32(1.0) / np.float32(temperature)) if temperature > 0 else 1.0


def mix64(yc, yu, cfg_weight: float, temperature: float):
    w = float(np.float32(cfg_weight))
    return (yu + w * (yc - yu)) * inv_t(temperature)


def bound_of(yc, yu, Sc, Su, target, lp64, K: int, cfg_weight: float, temperature: float, operand: str = "bf16") -> np.ndarray:
    V = yc.shape[1]
    t = _idx(target, yc.device).clamp(0, V - 1)[:, None]
    w = float(np.float32(cfg_weight))
    aw, a1w = abs(w), abs(1.0 - w)
    s = max(1.0, 1.0 / temperature) if temperature > 0 else 1.0
    A = K * U if operand == "bf16" else K * U / (1.0 - K * U)
    y = yu + w * (yc - yu)
    x = y * inv_t(temperature)
    M = U * (aw * (yc.abs() + 2 * (yc - yu).abs()) + a1w * yu.abs() + y.abs())

    def at_t_plus_max(q):
        return (q.gather(1, t)[:, 0] + q.max(-1).values).cpu().numpy()
    acc = s * A * (aw * at_t_plus_max(Sc) + a1w * at_t_plus_max(Su))
    mixr = s * at_t_plus_max(M) + U * at_t_plus_max(x.abs())
    with np.errstate(invalid="ignore"):
        rel = RTOL * np.where(np.isfinite(lp64), np.abs(lp64), 0.0)
    return acc + mixr + ATOL + rel


def cfg_head_logprob_ref(X, W, bias, target, cond_idx, uncond_idx, cfg_weight: float, temperature: float, operand: str = "bf16", device="cpu"):
    """-> (lp64 float64 [n], bound float64 [n])."""
    yc, yu, Sc, Su = terms64(X, W, bias, cond_idx, uncond_idx, operand, device)
    lp64 = SR.lp_at(mix64(yc, yu, cfg_weight, temperature), target)
    return lp64, bound_of(yc, yu, Sc, Su, target, lp64, int(torch.as_tensor(X).shape[-1]), cfg_weight, temperature, operand)


def fp32_eval(X, W, bias, target, cond_idx, uncond_idx, cfg_weight: float, temperature: float, operand: str = "bf16"):
    """What a correct device computes, up to summation order: fp32 GEMMs of the rounded operands, fp32 bias, mix, scaling and log-softmax."""
    X, W = SR.round_operand(X, operand), SR.round_operand(W, operand)
    b = torch.zeros(W.shape[0]) if bias is None else torch.as_tensor(bias, dtype=torch.float32)
    yc, yu = X[_idx(cond_idx, "cpu")] @ W.T + b, X[_idx(uncond_idx, "cpu")] @ W.T + b
    y = yu + np.float32(cfg_weight) * (yc - yu)
    if temperature > 0:
        y = y * (np.float32(1.0) / np.float32(temperature))
    lp = torch.log_softmax(y, -1)
    t = _idx(target, "cpu")
    out = lp.gather(1, t.clamp(0, y.shape[1] - 1)[:, None])[:, 0]
    return torch.where((t >= 0) & (t < y.shape[1]), out, torch.full_like(out, -np.inf)).numpy()


# ---------------------------------------------------------------------------------------------------------------- inputs
def gaussian_pairs(n: int, V: int, K: int, seed: int, rows: int = None, with_bias: bool = True):
    """score_ref.gaussian_case's X / W / target (the last quarter of the rows scaled x100) plus a bias of a few units and a random pairing:
    cond_idx / uncond_idx draw from all ``rows`` rows (default 2 n), so scaled and plain rows meet in one pair."""
    rows = 2 * n if rows is None else rows
    X, W, target = SR.gaussian_case(n, V, K, seed, rows=rows)
    g = torch.Generator().manual_seed(seed + 7919)
    bias = torch.randn(V, generator=g) * 3.0 if with_bias else None
    cond = torch.randint(0, rows, (n,), generator=g)
    uncond = torch.randint(0, rows, (n,), generator=g)
    return X, W, bias, target, cond, uncond


def edge_columns(n: int, V: int, K: int) -> list:
    """Column 0, 255, 256, the first and last column of every group, V - 1 -- for the geometry the kernel uses at n pairs (2 n rows)."""
    return SR.edge_columns(V, SR.geometry(2 * n, V, K))


# ---------------------------------------------------------------------------------------------------------------- mutants
def _lp(y, temperature, target):
    return SR.lp_at(y * inv_t(temperature), target)


def mutant_swapped(yc, yu, w, T, target):
    return _lp(yc + w * (yu - yc), T, target)                   # cond / uncond swapped: also the c + w (u - c) form


def mutant_bias_dropped(yc, yu, w, T, target, bias):
    b = torch.as_tensor(bias, dtype=torch.float64, device=yc.device)
    return _lp((yu - b) + w * ((yc - b) - (yu - b)), T, target)


def mutant_bias_after_mix(yc, yu, w, T, target, bias):
    b = torch.as_tensor(bias, dtype=torch.float64, device=yc.device)
    return _lp((yu - b) + w * (yc - yu) + w * b, T, target)    # bias added once, after the mix, with weight w


def mutant_c_plus(yc, yu, w, T, target):
    return _lp(yc + w * (yu - yc), T, target)                   # c + w (u - c)


def mutant_temperature_one_side(yc, yu, w, T, target):
    return SR.lp_at(yu + w * (yc * inv_t(T) - yu), target)      # temperature applied to the cond side only
