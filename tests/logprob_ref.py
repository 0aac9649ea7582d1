"""fp64 numpy restatement of the token log-probability (include/plangen_hip.h, pg_request_token_logprobs / pg_op_token_logprob), the
comparison the GPU tests use, and wrong versions of the definition ("mutants") which that comparison has to reject.

Definition, per row y (fp32 [V]) and emitted token tok:
    x = y * (1 / temperature) as an fp32 product when temperature > 0 (what the draw uses), else x = y;  NaN counts as -inf
    logprob = x[tok] - (m + log sum_v exp(x_v - m)),  m = max_v x_v                      (here: in fp64 on the fp32 x)
    x[tok] = -inf, a token outside [0, V) or a row without a finite entry: -inf;  m = +inf: the mass lies evenly on the +inf entries
Text loop: a row that was finished before a step scores 0.0 there.

Tolerance: |lp - lp64| <= ATOL + RTOL * |lp64|.  Each of V <= 102 400 terms carries <= ~2 ulp relative error (x - m rounding + expf); the
fp32 sum of <= ~100 sequential terms per thread plus a ~20-level tree adds <= ~120 * 2^-24 = 7e-6 relative, which is that much absolute in
the log; x[tok] - m at |x| <= 64 adds <= 4e-6; the bound is ~5x the sum.  (Rows scaled x40 reach |x[tok] - m| of a few hundred, where one
fp32 ulp is 3e-5: still inside ATOL, and RTOL covers the growth of |lp| itself.)
Measured on an MI355X (tests/test_gpu_logprobs.py prints every figure): operator, largest error 4.2e-5, on the x40 rows; rows of logit
scale 2.4 and the loops on the tiny fixture: <= 1.1e-6.  The x40 figure is within 2.5x of the bound, so the bound stays as derived."""
import numpy as np

ATOL, RTOL = 1e-4, 1e-6


def scaled_row(y, temperature: float) -> np.ndarray:
    """The fp32 row x the draw is made from, NaN -> -inf, as float64."""
    y = np.asarray(y, dtype=np.float32)
    if temperature > 0:
        y = y * (np.float32(1.0) / np.float32(temperature))               # fp32 product, as on the device
    x = y.astype(np.float64)
    return np.where(np.isnan(x), -np.inf, x)


def _lp_of_x(x: np.ndarray, tok: int) -> float:
    V = x.shape[0]
    if not 0 <= tok < V:
        return -np.inf
    m = x.max()
    if m == -np.inf or x[tok] == -np.inf:
        return -np.inf
    if m == np.inf:
        return -np.log(float((x == np.inf).sum())) if x[tok] == np.inf else -np.inf
    with np.errstate(under="ignore"):
        return float(x[tok] - (m + np.log(np.exp(x - m).sum())))


def token_logprob_ref(y, tok, temperature: float = 0.0) -> np.ndarray:
    """y [B, V] (or [V]) fp32, tok [B] -> float64 [B]."""
    y = np.asarray(y, dtype=np.float32)
    y = y[None] if y.ndim == 1 else y
    tok = np.asarray(tok).reshape(-1)
    return np.array([_lp_of_x(scaled_row(y[b], temperature), int(tok[b])) for b in range(y.shape[0])], dtype=np.float64)


def image_logprobs_ref(logits, tokens, temperature: float = 0.0) -> np.ndarray:
    """logits [T, B, V] (the logits_out tap), tokens [B, T] (emitted) -> float64 [B, T]."""
    logits, tokens = np.asarray(logits), np.asarray(tokens)
    T, B, _ = logits.shape
    return np.stack([token_logprob_ref(logits[t], tokens[:, t], temperature) for t in range(T)], axis=1).reshape(B, T)


def text_logprobs_ref(logits, tokens, eos: int, temperature: float = 0.0, zero_finished: bool = True) -> np.ndarray:
    """logits [n, B, V] (the text tap: EOS ban and automaton mask applied), tokens [B, n] -> float64 [B, n]; a row that emitted eos at
    an earlier step is finished and scores 0.0 (zero_finished=False is the "finished rows scored" mutant)."""
    logits, tokens = np.asarray(logits), np.asarray(tokens)
    n, B, _ = logits.shape
    out = np.zeros((B, n), dtype=np.float64)
    done = np.zeros(B, dtype=bool)
    for t in range(n):
        lp = token_logprob_ref(logits[t], tokens[:, t], temperature)
        out[:, t] = np.where(done & zero_finished, 0.0, lp)
        done |= tokens[:, t] == eos
    return out


def close(lp, lp64, atol: float = ATOL, rtol: float = RTOL) -> np.ndarray:
    """bool array: the issue's comparison; infinities must agree exactly, NaN never passes."""
    lp, lp64 = np.asarray(lp, dtype=np.float64), np.asarray(lp64, dtype=np.float64)
    inf = np.isinf(lp64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(lp - lp64) <= atol + rtol * np.abs(lp64)
    return np.where(inf, lp == lp64, ok & np.isfinite(lp))


def max_excess(lp, lp64) -> float:
    """Largest |lp - lp64| over the finite entries (what the tests print before they assert)."""
    lp, lp64 = np.asarray(lp, dtype=np.float64), np.asarray(lp64, dtype=np.float64)
    f = np.isfinite(lp64) & np.isfinite(lp)
    return float(np.abs(lp[f] - lp64[f]).max()) if f.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- mutants
def mutant_no_temperature(y, tok, temperature):
    return token_logprob_ref(y, tok, 0.0)


def mutant_mask_ignored(y_unmasked, allowed, tok, temperature):
    """The normaliser runs over every token, also the ones the automaton / the EOS ban removed."""
    return token_logprob_ref(y_unmasked, tok, temperature)


def mutant_topk_renormalised(y, tok, temperature, top_k: int):
    y = np.asarray(y, dtype=np.float32)
    out = []
    for b in range(y.shape[0]):
        kth = np.sort(y[b])[-top_k]
        out.append(token_logprob_ref(np.where(y[b] >= kth, y[b], -np.inf), [tok[b]], temperature)[0])
    return np.array(out)


def mutant_argmax_token(y, tok, temperature):
    y = np.asarray(y, dtype=np.float32)
    return token_logprob_ref(y, np.argmax(np.where(np.isnan(y), -np.inf, y), axis=-1), temperature)


def mutant_finished_scored(logits, tokens, eos, temperature):
    return text_logprobs_ref(logits, tokens, eos, temperature, zero_finished=False)
