"""Host model of the samplers' draw (CPU only, no GPU import): the counter-based RNG of csrc/common.h (rng_bits, uniform_from_bits) in integer-exact
numpy uint64 arithmetic, the two stream keys, the fp64 Gumbel term, the Gumbel-max draw with its distance to the runner-up, the greedy rule and the
feedback rules of cfg_pick_kernel -- and the seeded input families of tests/test_gpu_draws.py, so that tests/test_draw_ref_cpu.py can show on the CPU that
the decided / undecided rule leaves (almost) every draw of those families decided.

A draw is the first index of the maximum of y = x / T + g, g = -log(-log(u)).  The device forms y in fp32 as x * (1 / T) - log(-log(u)) with fast
logarithms, so the model's winner is only BINDING when its fp64 lead over the runner-up exceeds what those roundings can move: decided(gap, scale, E_g)."""
from __future__ import annotations

import numpy as np

U64 = np.uint64
KEY_MUL = 1000003
NONE = -1                       # draw / greedy: nothing can be chosen (every entry -inf, NaN or outside keep)
UNDECIDED_CAP = 0.01            # share of a parametrisation's draws that may be undecided
E_G_CPU = 2.0 ** -16            # the conservative Gumbel-term error the CPU tests use


def _u64(x):
    """Anything integer -> uint64 array, mod 2^64 (Python integers of any size included)."""
    if isinstance(x, (int, np.integer)):
        return np.array(int(x) % (1 << 64), dtype=U64)
    a = np.asarray(x)
    if a.dtype == object:
        return np.array([int(v) % (1 << 64) for v in a.ravel()], dtype=U64).reshape(a.shape)
    return a.astype(U64)


def rng_bits(seed, a, b):
    """splitmix64 finaliser over seed + G (a + 1) + M (b + 1), all mod 2^64 (uint64 arrays wrap silently)."""
    seed, a, b = _u64(seed), _u64(a), _u64(b)
    with np.errstate(over="ignore"):
        z = seed + U64(0x9E3779B97F4A7C15) * (a + U64(1)) + U64(0xBF58476D1CE4E5B9) * (b + U64(1))
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def uniform(bits):
    """((bits >> 41) + 0.5) / 2^23: 23 random bits, exact in fp32 and therefore in fp64; inside [2^-24, 1 - 2^-24]."""
    return ((_u64(bits) >> U64(41)).astype(np.float64) + 0.5) * (1.0 / 8388608.0)


def gumbel(u):
    return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def image_key(b, b_off, img_off, step):
    with np.errstate(over="ignore"):
        return (_u64(b) + _u64(b_off) + _u64(img_off)) * U64(KEY_MUL) + _u64(step)


def text_key(row, row_off, step):
    with np.errstate(over="ignore"):
        return (_u64(row) + _u64(row_off)) * U64(KEY_MUL) + _u64(step)


def noise(seed, stream, V):
    """g [n, V]: the Gumbel term of entry v of the rows whose stream keys are ``stream`` [n]."""
    stream = np.atleast_1d(_u64(stream))
    return gumbel(uniform(rng_bits(seed, stream[:, None], np.arange(V, dtype=U64)[None, :])))


def _f32(t):
    return float(np.float32(t))


def draw_top2(rows, temperature, seed, stream, keep=None):
    """rows [n, V] (the fp32 rows the device draws from, any float dtype), stream [n] keys -> (token [n], gap [n], scale [n], runner-up [n]).
    token: first index of the maximum of x / T + g in fp64 over the entries inside ``keep`` (bool [n, V]) that are neither NaN nor -inf; NONE when
    there is no such entry.  gap: the fp64 lead over the runner-up (inf when there is none, or when the winner is +inf: the device's value is +inf
    there too and ties go to the first index).  scale: max(|x / T| + |g|) over the top two."""
    x = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    n, V = x.shape
    g = noise(seed, stream, V)
    with np.errstate(invalid="ignore"):
        xt = x / _f32(temperature)
        y = xt + g
    out = np.isnan(y)
    if keep is not None:
        out |= ~np.atleast_2d(np.asarray(keep, dtype=bool))
    y = np.where(out, -np.inf, y)
    tok = np.argmax(y, axis=1)
    r = np.arange(n)
    top = y[r, tok]
    y2 = y.copy()
    y2[r, tok] = -np.inf
    ru = np.argmax(y2, axis=1)
    second = y2[r, ru]
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isposinf(top) | np.isneginf(second), np.inf, top - second)
        mag = np.abs(xt) + np.abs(g)
        s1 = np.where(np.isfinite(top), mag[r, tok], 0.0)
        s2 = np.where(np.isfinite(second), mag[r, ru], 0.0)
    token = np.where(np.isneginf(top), NONE, tok)
    return token.astype(np.int64), gap, np.maximum(s1, s2), ru.astype(np.int64)


def draw(rows, temperature, seed, stream, keep=None):
    """(token, gap, scale) of draw_top2."""
    return draw_top2(rows, temperature, seed, stream, keep)[:3]


def decided(gap, scale, E_g):
    """Two fp32 roundings of x * (1 / T) - g (or one, contracted) and the rounding of 1 / T: at most 3 * 2^-24 * scale; the device's Gumbel term is within
    E_g of the fp64 one.  Either candidate can move by that much, so the lead must exceed twice the sum."""
    return np.asarray(gap) > 2.0 * (E_g + 3.0 * 2.0 ** -24 * np.asarray(scale))


def greedy(rows, keep=None):
    """temperature <= 0: first index of the maximum; NaN (and -inf: nothing compares greater than the start value) never chosen; NONE when nothing is left."""
    x = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    out = np.isnan(x)
    if keep is not None:
        out |= ~np.atleast_2d(np.asarray(keep, dtype=bool))
    y = np.where(out, -np.inf, x)
    tok = np.argmax(y, axis=1)
    return np.where(np.isneginf(y[np.arange(len(y)), tok]), NONE, tok).astype(np.int64)


def cfg_mix(cond, uncond, w):
    """mixed = u + w (c - u) in fp64 (the tests choose values for which the fp32 result is the same number)."""
    c, u = np.asarray(cond, dtype=np.float64), np.asarray(uncond, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return u + float(w) * (c - u)


def clamp(t, V):
    return 0 if t < 0 else (V - 1 if t >= V else int(t))


def cfg_pick(token, V, T, step, force=None, mask=None, none_token=None):
    """The feedback rules of cfg_pick_kernel for one image.  token: the draw (NONE -> none_token, the pinned rule of the form that drew); force / mask: this
    image's [T] rows or None.  Returns (emit, feed): emit is None when step >= T (nothing is written); feed indexes the embedding table."""
    i = clamp(none_token if token == NONE else token, V)
    emit = feed = i
    if step < T and force is not None:
        f = int(force[step])
        if mask is not None:
            if int(mask[step]) == 0:
                emit = feed = f
        else:
            feed = f
    return (emit if step < T else None), clamp(feed, V)


def text_pick(token, unfinished, eos, V):
    """text_argmax_kernel: NONE -> 0; a finished row emits eos.  Returns (token, still unfinished, embedding row)."""
    i = 0 if token == NONE else int(token)
    tok = i if unfinished else eos
    return tok, int(bool(unfinished) and tok != eos), clamp(tok, V)


# ---------------------------------------------------------------------------------------------------------------- input families (shared with the GPU tests)
# Slab values are multiples of 2^-6 with |value| <= 4: any sum of <= 10 of them, and u + w (c - u) for w in {0, 1, 5}, is exact in fp32 (< 2^9 in units of
# 2^-6, 24-bit significand), so the device's row is known bit for bit.  A standard deviation of ~2.4 per row is what the heads produce.
Q = 64.0


def dyadic_slabs(rng, S, R, V, std):
    """[S, R, V] float32 multiples of 1 / Q, clipped to +-4; their sum over S has standard deviation ~std per entry."""
    x = np.rint(rng.standard_normal((S, R, V)) * (std / np.sqrt(S)) * Q) / Q
    return np.clip(x, -4.0, 4.0).astype(np.float32)


IMG_V = (1, 17, 1000, 16384)
IMG_S = (1, 2, 4, 5, 9)
IMG_W = (0.0, 1.0, 5.0)
IMG_T = (0.0, 0.7, 1.3)
IMG_B = (1, 3)
IMG_STEPS = (0, 1, 575)               # the decorrelation check's steps
IMG_CASE_STEPS = (0, 1, 2, 3, 574, 575)  # every sub-case of the operator test is drawn at each of these
IMG_SEED = (1 << 63) + 0x1234567
IMG_OFFS = ((0, 0), (2, 5), (1, 4000))          # (b_off, img_off)


def image_cases(V, S, with_bias):
    """The sub-cases of one (V, S, bias) parametrisation of the image operator test: every (cfg_weight, temperature, B), offsets and steps rotating.
    Yields dicts with slabs [S, 2B, V], bias [V] or None and the scalars."""
    rng = np.random.default_rng(100000 + V * 64 + S * 2 + int(with_bias))
    i = 0
    for w in IMG_W:
        for T in IMG_T:
            for B in IMG_B:
                b_off, img_off = IMG_OFFS[i % 3]
                # cond and uncond of std 1.5 each: mixed has std 1.5 (w = 0, 1) and 1.5 sqrt(41) = 9.6 (w = 5: 5 c - 4 u)
                slabs = dyadic_slabs(rng, S, 2 * B, V, 1.5)
                bias = (np.rint(rng.standard_normal(V) * 0.5 * Q) / Q).astype(np.float32) if with_bias else None
                yield dict(w=w, T=T, B=B, b_off=b_off, img_off=img_off, B_total=b_off + B + 1, steps=IMG_CASE_STEPS, slabs=slabs, bias=bias, seed=IMG_SEED + i)
                i += 1


def image_mixed(c):
    """fp64 mixed rows [B, V] of an image case."""
    s = c["slabs"].astype(np.float64).sum(0)
    if c["bias"] is not None:
        s = s + c["bias"].astype(np.float64)[None, :]
    return cfg_mix(s[0::2], s[1::2], c["w"])


TXT_V_SCALAR = (1, 3, 255)
TXT_V_VECTOR = (4, 4100, 102400)
TXT_S = (1, 2, 3)
TXT_SEED = (1 << 63) + 0xABCDEF
TXT_B = 6


def text_cases(V, S):
    """Sub-cases of one (V, S) parametrisation of the text operator test: (temperature, steps, row_off, min_new) variants over fresh rows; every step
    of a sub-case draws from the same rows with another key (and, below min_new, with the EOS entry banned)."""
    rng = np.random.default_rng(200000 + V * 8 + S)
    out = []
    variants = ((0.0, (0,), 0, 0), (0.7, (0, 1, 2, 3), 0, 0), (1.0, (3, 4, 5, 6), 7, 5), (1.3, (4092, 4093, 4094, 4095), 4000, 0),
                (0.7, (0, 1, 2, 3), 1, 3), (1.0, (10, 11, 12, 13), 0, 0))
    for i, (T, steps, row_off, min_new) in enumerate(variants):
        slabs = dyadic_slabs(rng, S, TXT_B, V, 2.4)
        out.append(dict(T=T, steps=steps, row_off=row_off, min_new=min_new, max_new=4096, eos=min(V - 1, 2), slabs=slabs, seed=TXT_SEED + 17 * i))
    return out


def text_rows(c, step):
    """fp64 rows [B, V] of a text case at ``step``, the EOS ban applied."""
    x = c["slabs"].astype(np.float64).sum(0)
    if step < c["min_new"]:
        x[:, c["eos"]] = -np.inf
    return x
