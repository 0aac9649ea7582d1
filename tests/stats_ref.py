"""fp64 numpy restatement of the per-token uncertainty outputs (include/plangen_hip.h, pg_request_token_stats / pg_op_token_stats), the
input families and comparisons the GPU tests use, and wrong versions of the definition ("mutants") the comparisons have to reject.

Definition, per row y (fp32 [V]), emitted token tok and n_alt: x as in logprob_ref.scaled_row (the fp32 product y * (1 / temperature),
NaN -> -inf); from there in fp64, m = max x, s = sum exp(x - m), t = sum exp(x - m) (x - m), entries -inf adding 0 to both:
    logprob      logprob_ref's
    entropy      log s - t / s   (0 for a row without a finite entry; log k when m = +inf sits on k entries)
    rank         #{v: x_v > x_tok};  V when tok is outside [0, V) or x_tok = -inf
    alt_tok      the n_alt largest x_v, descending, lowest index first among equals;  -1 where fewer entries are above -inf
    alt_logprob  the logprob of each alternative;  -inf where alt_tok = -1
rank and alt_tok are exact: the device and this file order the SAME fp32 values x, so there is no rounding between them; the random
families still draw from a grid of 1/8 so that no two distinct entries are closer than any rounding anywhere.

Entropy bound, ENT_TOL(V) = (123 + 252 ln V) * 2^-24.  With u = 2^-24: a thread adds <= ceil(V / 1024) <= 100 terms in sequence, then
6 butterfly levels and 15 serial adds: a sum of same-sign terms carries <= 121 u relative error from the additions.  A term of s is
expf(d), d = x - m (one rounding, which moves the exponent by |d| u: over the row that is (|t| / s) u <= ln V * u relative to s,
counted in the 2 u below): <= 2 u;  a term of t is that times d, one more rounding, <= 4 u with d's own.  So s has <= 123 u, t (all terms
<= 0) <= 125 u, t / s <= 249 u relative.  H = logf(s) - t / s: the error of s enters the logarithm as <= 123 u absolute; logf and the final
subtraction add <= 2 u |ln s| + u |H|; the quotient adds 249 u |t / s|.  |ln s|, |t / s| = ln s - H and H are all <= ln V, which gives
(123 + 252 ln V) u: 1.8e-4 at V = 102 400, 3.2e-5 at V = 5.  It is a worst case (every rounding in one direction); nothing in it comes
from the kernel's output.  alt_logprob is the logprob expression: logprob_ref.close applies."""
import numpy as np

import logprob_ref as LR

U = 2.0 ** -24


def ent_tol(V: int) -> float:
    return (123.0 + 252.0 * np.log(max(V, 1))) * U


# ---------------------------------------------------------------------------------------------------------------- reference
def _entropy_of_x(x: np.ndarray, nan_on_holes: bool = False) -> float:
    m = x.max()
    if m == -np.inf:
        return 0.0
    if m == np.inf:
        return float(np.log((x == np.inf).sum()))
    with np.errstate(under="ignore", invalid="ignore"):
        d = x - m
        e = np.exp(d)
        td = e * d                                                         # 0 * -inf = NaN at the holes ...
        if not nan_on_holes:
            td = np.where(e > 0, td, 0.0)                                  # ... which count as 0
        s = e.sum()
        return float(np.log(s) - td.sum() / s)


def _rank_of_x(x: np.ndarray, tok: int, ge: bool = False) -> int:
    V = x.shape[0]
    if not 0 <= tok < V or x[tok] == -np.inf:
        return V
    return int((x >= x[tok]).sum()) if ge else int((x > x[tok]).sum())


def _alts_of_x(x: np.ndarray, n_alt: int, ascending: bool = False, ties_high: bool = False):
    V = x.shape[0]
    idx = np.arange(V)
    order = np.lexsort((-idx if ties_high else idx, -x))                   # value descending, then index ascending
    order = [int(v) for v in order[:n_alt] if x[v] > -np.inf]
    if ascending:
        order = order[::-1]
    tok = np.full(n_alt, -1, dtype=np.int64)
    lp = np.full(n_alt, -np.inf)
    for k, v in enumerate(order):
        tok[k] = v
        lp[k] = LR._lp_of_x(x, v)
    return tok, lp


def row_stats_ref(y, tok: int, temperature: float, n_alt: int, **mut) -> dict:
    x = LR.scaled_row(y, temperature)
    at, al = _alts_of_x(x, n_alt, mut.get("ascending", False), mut.get("ties_high", False))
    H = _entropy_of_x(x, mut.get("nan_on_holes", False))
    return dict(logprob=LR._lp_of_x(x, int(tok)), entropy=H / np.log(2.0) if mut.get("bits") else H,
                rank=_rank_of_x(x, int(tok), mut.get("ge", False)), alt_tok=at, alt_logprob=al)


def token_stats_ref(y, tok, temperature: float = 0.0, n_alt: int = 0, **mut) -> dict:
    """y [B, V] fp32, tok [B] -> dict of float64 / int64 arrays over [B] (alternatives [B, n_alt])."""
    y = np.asarray(y, dtype=np.float32)
    y = y[None] if y.ndim == 1 else y
    tok = np.asarray(tok).reshape(-1)
    rows = [row_stats_ref(y[b], int(tok[b]), temperature, n_alt, **mut) for b in range(y.shape[0])]
    return _stack(rows, n_alt)


def _stack(rows, n_alt):
    return dict(logprob=np.array([r["logprob"] for r in rows], dtype=np.float64), entropy=np.array([r["entropy"] for r in rows], dtype=np.float64),
                rank=np.array([r["rank"] for r in rows], dtype=np.int64),
                alt_tok=np.array([r["alt_tok"] for r in rows], dtype=np.int64).reshape(len(rows), n_alt),
                alt_logprob=np.array([r["alt_logprob"] for r in rows], dtype=np.float64).reshape(len(rows), n_alt))


def image_stats_ref(logits, tokens, temperature: float = 0.0, n_alt: int = 0) -> dict:
    """logits [T, B, V] (the logits_out tap), tokens [B, T] (emitted) -> dict over [B, T] (alternatives [B, T, n_alt])."""
    logits, tokens = np.asarray(logits), np.asarray(tokens)
    T, B, _ = logits.shape
    per_t = [token_stats_ref(logits[t], tokens[:, t], temperature, n_alt) for t in range(T)]
    return {k: np.stack([p[k] for p in per_t], axis=1) for k in per_t[0]}


FINISHED = dict(logprob=0.0, entropy=0.0, rank=0, alt_tok=-1, alt_logprob=0.0)       # a text row that was finished before the step


def text_stats_ref(logits, tokens, eos: int, temperature: float = 0.0, n_alt: int = 0) -> dict:
    """logits [n, B, V] (the text tap), tokens [B, n] -> dict over [B, n]; FINISHED where the row emitted eos at an earlier step."""
    out = image_stats_ref(logits, tokens, temperature, n_alt)
    tokens = np.asarray(tokens)
    hit = tokens == eos
    done = (np.cumsum(hit, axis=1) - hit) > 0
    for k, fill in FINISHED.items():
        out[k][done] = fill
    return out


# ---------------------------------------------------------------------------------------------------------------- comparisons
def mismatches(got: dict, ref: dict, V: int, keys=("logprob", "entropy", "rank", "alt_tok", "alt_logprob")) -> list:
    """The issue's comparison: rank / alt_tok exact, logprob / alt_logprob by logprob_ref.close, entropy within ent_tol(V) (NaN never passes).
    Returns the names of the outputs that disagree (empty: all agree)."""
    bad = []
    for k in keys:
        if k not in got:
            continue
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if g.shape != r.shape:
            bad.append(k + ":shape")
        elif k in ("rank", "alt_tok"):
            if not np.array_equal(g.astype(np.int64), r.astype(np.int64)):
                bad.append(k)
        elif k == "entropy":
            with np.errstate(invalid="ignore"):
                if not (np.abs(g.astype(np.float64) - r) <= ent_tol(V)).all():
                    bad.append(k)
        elif not LR.close(g, r).all():
            bad.append(k)
    return bad


def max_entropy_error(got, ref) -> float:
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float(np.nanmax(d)) if d.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- input families
def families(V: int, B: int, seed: int, n_alt: int = 8) -> dict:
    """name -> (y fp32 [B, V], tok int32 [B]).  Random values come from a grid of 1/8; ties are planted."""
    g = np.random.default_rng(seed)
    grid = lambda: (np.round(g.standard_normal((B, V)) * 2.4 * 8) / 8).astype(np.float32)
    rnd_tok = lambda: g.integers(0, V, B).astype(np.int32)
    spots = lambda n: g.choice(V, size=min(n, V), replace=False)
    fam = {"normal": (grid(), rnd_tok())}
    # ties: three entries share the maximum; below them n_alt - 4 distinct values, then three equal entries at places n_alt - 1 .. n_alt + 1
    # (counted from 0: the n_alt-th place is inside the tie); everything else lies lower (and ties there too, at the clip)
    y, tok = np.minimum(grid(), np.float32(4.0)), rnd_tok()
    for b in range(B):
        nd = max(n_alt - 4, 0)
        p = spots(3 + nd + 3)
        vals = [20.0] * 3 + [19.0 - k for k in range(nd)] + [5.0] * 3
        y[b, p] = np.array(vals[:len(p)], dtype=np.float32)
        tok[b] = p[min(b, len(p) - 1)] if b < 2 else p[-1]               # on a tied maximum (not always the first), and on the low tie
    fam["ties"] = (y, tok)
    y = grid()
    y[:, 0] = -np.inf
    if V > 4:
        y[:, V // 2] = np.nan
        y[0, V - 2] = -np.inf
        y[:, g.integers(0, V, max(V // 7, 1))] = -np.inf
    fam["holes"] = (y, rnd_tok())
    fam["empty"] = (np.full((B, V), -np.inf, dtype=np.float32), rnd_tok())
    y = grid()
    y[:, V - 1] = np.inf
    if V > 1:
        y[:, V // 3] = np.inf
    fam["plus_inf"] = (y, np.where(np.arange(B) % 2 == 0, V - 1, rnd_tok()).astype(np.int32))
    y = grid() - 10.0
    pk = rnd_tok()
    y[np.arange(B), pk] = 60.0
    fam["peaked"] = (y, np.where(np.arange(B) % 2 == 0, pk, rnd_tok()).astype(np.int32))
    fam["flat"] = (np.full((B, V), 1.5, dtype=np.float32), rnd_tok())
    y, tok = grid(), rnd_tok()
    y[np.arange(B), tok] = -np.inf
    fam["tok_on_neginf"] = (y, tok)
    fam["tok_outside"] = (grid(), np.array(([V, -1, V + 5] * B)[:B], dtype=np.int32))
    return fam


FINITE_FAMILIES = ("normal", "ties", "peaked", "flat")


# ---------------------------------------------------------------------------------------------------------------- fp32 restatement
def _shaped_sum_fp32(a: np.ndarray) -> np.float32:
    """An fp32 sum of the shape the bound assumes: 1024 threads add their (strided) terms in sequence, a 6-level butterfly per 64
    threads, then the 16 wave sums in sequence."""
    n = -(-a.shape[0] // 1024)
    p = np.zeros(n * 1024, dtype=np.float32)
    p[:a.shape[0]] = a
    lanes = np.cumsum(p.reshape(n, 1024), axis=0, dtype=np.float32)[-1].reshape(16, 64)       # cumsum: one addition per term, in order
    w = 64
    while w > 1:
        w //= 2
        lanes = (lanes[:, :w] + lanes[:, w:2 * w]).astype(np.float32)
    return np.cumsum(lanes[:, 0], dtype=np.float32)[-1]


def two_pass_fp32(y, temperature: float = 0.0) -> float:
    """The two passes in numpy fp32 with sums of the kernel's shape: a sanity figure for ent_tol (tests/test_stats_ref_cpu.py asserts
    that it stays inside the bound and prints how far; the bound is the derived one, not this)."""
    x = LR.scaled_row(y, temperature).astype(np.float32)
    m = x.max()
    if not np.isfinite(m):
        return 0.0 if m < 0 else float(np.log(np.float32((x == np.inf).sum())))
    with np.errstate(under="ignore", invalid="ignore"):
        d = (x - m).astype(np.float32)
        e = np.exp(d).astype(np.float32)
        td = np.where(e > 0, e * d, np.float32(0)).astype(np.float32)
        s, t = _shaped_sum_fp32(e), _shaped_sum_fp32(td)
        return float(np.log(s) - t / s)
