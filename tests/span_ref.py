"""Reference, input families and error bound for the attention-mass-on-spans kernel (csrc/attn_span.hip, pg_op_attn_span_mass,
pg_request_attn_spans; definition: include/plangen_hip.h).

    A[r, i, s] = 1 / nh * sum_h sum_{k in span(r, s), k <= q_i, k real} softmax_k(scale * Q[r, h, q_i] . K[r, h, k])

``span_mass_ref`` evaluates that in fp64 from the bf16 values of q and K.  ``span_mass_emulated`` is a numpy model of the ARITHMETIC the kernel
was built with (fp32 scores, the scale on the fp32 score, 64-key tiles with a running maximum and sum, __expf, P split into hi + lo bf16 halves
for the span MFMA, one rescale per tile, fixed-order head mean) with switches that plant the defects a span kernel can have.

The bound (absolute, on A in [0, 1]), derived from that arithmetic, u = 2^-24:
  * a score is an fp32 sum of 128 exact bf16 products in an unknown order (<= 127 u sum|q_d k_d|), times the scale (u |s|), minus the running
    maximum (u |s - m| <= 2 u max|s|): |ds| <= 131 u scale max_k sum_d |q_d| |k_d| =: d.  Scores moved by at most d move every softmax weight
    by a factor within exp(+-2 d), so a mass (a sum of weights, <= 1) by at most expm1(2 d);
  * __expf(x) = v_exp_f32(x log2 e): the product's rounding is a relative |x| u of the result, the instruction 1 ulp.  Weighted by the
    probability itself, sum_k p_k |x_k| u <= n u / e relative to sum_k p_k >= 1: (n + 4) u for the span sum and the same for the total;
  * the span sum and the total are fp32 sums of n terms: n u each;
  * one rescale per 64-key tile: the SAME alpha multiplies the span sum and the total, so only the two products' roundings count: 4 u per
    tile with the additions that follow;
  * P enters the span MFMA as hi + lo, hi = bf16(p), lo = bf16(p - hi): the residue is <= 2^-18 p, taken as 2^-17 with the rounding of lo;
  * the division and the head mean over nh heads: (nh + 3) u.
  bound = expm1(2 d) + (4 n + 8 + 4 tiles + nh + 3) u + 2^-17, per (row, query) with d the largest over the heads.  It must stay below 2^-7
  (checked where a family is built): masses lie in [0, 1] and a looser bound could hide a miscounted key.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
BOUND_CAP = 2.0 ** -7
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(128.0)))        # the engine's 1.0f / sqrtf(128.0f)
DEFECTS = ("lo_plus1", "hi_plus1", "no_causal", "pad_keys", "no_rescale", "no_head_div", "col_as_slot")
FAMILIES = ("flat", "peaked", "large")
LENGTHS = (1, 63, 64, 65, 130, 200)
FRAME = 208                                                          # columns of the padded frame: pad_len[r] = FRAME - LENGTHS[r]


def bf16(x):
    """fp32 array -> the nearest bf16 values (round to nearest even), as float32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


def spans_for(pad, n, q_col0, n_q, n_spans):
    """The span kinds of the operator test, [n_spans][2] columns for a row with ``pad`` leading pad columns and ``n`` tokens."""
    L = pad + n
    q_last = min(q_col0 + n_q, L) - 1
    s = [
        (pad + 60, pad + 70),                      # crosses the 64-key tile edge
        (pad + 5, pad + 5),                        # empty
        (pad + min(3, n - 1), pad + min(3, n - 1) + 1),   # one key
        (max(pad - 5, 0), pad + 2),                # starts in the padding
        (max(q_last - 1, 0), L),                   # ends past the last query
        (q_col0 - 3, q_col0 + 3),                  # contains the (first) query
        (pad + 10, pad + 40), (pad + 30, pad + 50),        # two overlapping spans
        (pad + 20, pad + 10),                      # hi < lo: empty
        (0, L),                                    # everything
        (pad + 63, pad + 64), (pad + 64, pad + 65), (pad + 127, pad + 129),   # single keys at the tile boundaries
        (pad, pad + 1),                            # the first real key
        (pad + n - 1, L),                          # the last real key
        (pad + 90, pad + 100),
    ]
    return np.array(s[:n_spans], dtype=np.int32)


def make_case(family, q_col0, n_q, n_spans, nh=2, seed=0, partition=False):
    """One packed batch: rows of LENGTHS tokens in a FRAME-column left-padded frame, q [tokens][nh][128] and k [R][nh][slots][128] as bf16
    values in float32, spans per ``spans_for`` (or, with ``partition``, n_spans chunks that tile [0, FRAME))."""
    assert family in FAMILIES
    rng = np.random.default_rng(1000 * seed + FAMILIES.index(family))
    R, slots = len(LENGTHS), 208
    length = np.array(LENGTHS, dtype=np.int32)
    pad = (FRAME - length).astype(np.int32)
    row_off = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int32)
    ntok = int(length.sum())
    if partition:
        edges = np.linspace(0, FRAME, n_spans + 1).round().astype(np.int32)
        lo = np.tile(edges[:-1], (R, 1)); hi = np.tile(edges[1:], (R, 1))
    else:
        sp = np.stack([spans_for(int(pad[r]), int(length[r]), q_col0, n_q, n_spans) for r in range(R)])
        lo, hi = sp[..., 0].copy(), sp[..., 1].copy()
    e0 = np.zeros(128, dtype=np.float32); e0[::2] = 1.0 / 8.0            # unit vector spread over 64 dimensions
    q = rng.standard_normal((ntok, nh, 128)).astype(np.float32)
    k = np.zeros((R, nh, slots, 128), dtype=np.float32)
    k[:] = rng.standard_normal(k.shape).astype(np.float32) * 7.0        # slots past len hold junk the kernel must never count
    for r in range(R):
        n, p, off = int(length[r]), int(pad[r]), int(row_off[r])
        kr = rng.standard_normal((nh, n, 128)).astype(np.float32)
        if family == "flat":
            q[off:off + n] *= 0.02; kr *= 0.02
        elif family == "peaked":
            # every query shares the component 8 e0; the keys at span edges, next to them, at the tile boundaries, at the first query and
            # right behind it carry ~ 17 e0: score ~ 12 there against ~ 0 elsewhere, so each such key <= q holds a large share of the mass
            q[off:off + n] = q[off:off + n] * 0.1 + 8.0 * e0
            kr *= 0.1
            hot = {63, 64, 127, 128, q_col0 - p, q_col0 - p + 1}
            for a, b in zip(lo[r], hi[r]):
                hot |= {int(a) - p - 1, int(a) - p, int(b) - p - 1, int(b) - p}
            for j in sorted(hot):
                if 0 <= j < n:
                    kr[:, j] += (17.0 * (0.9 + 0.2 * rng.random())) * e0
        else:
            # scores rise with the key index (up to ~ 60): the running maximum rises in every later tile, the mass sits on the latest keys
            q[off:off + n] = q[off:off + n] * 0.1 + 8.0 * e0
            kr = kr * 0.1 + (85.0 * (np.arange(n, dtype=np.float32)[None, :, None] + 1) / 200.0) * e0
        k[r, :, :n] = kr
    case = dict(family=family, q=bf16(q), k=bf16(k), row_off=row_off, length=length, pad=pad, lo=lo.astype(np.int32), hi=hi.astype(np.int32),
                q_col0=int(q_col0), n_q=int(n_q), nh=nh, slots=slots, scale=SCALE)
    return case


def partition_bound(nk, nh):
    """The bound's terms that do not come from the scores, for queries that see ``nk`` keys: what is left for the SUM over a partition's spans
    (per span), where moved scores cancel -- the weights still sum to one."""
    nk = np.asarray(nk)
    return (4 * nk + 8 + 4 * ((nk - 1) // 64 + 1) + nh + 3) * U + 2.0 ** -17


def span_mass_ref(case):
    """(A fp64 [R, n_q, S], bound fp64 [R, n_q]) of the definition; pad queries and rows without tokens give 0 (bound 0: exact)."""
    q, k = case["q"].astype(np.float64), case["k"].astype(np.float64)
    R, S, n_q, nh = len(case["length"]), case["lo"].shape[1], case["n_q"], case["nh"]
    A = np.zeros((R, n_q, S)); bound = np.zeros((R, n_q))
    for r in range(R):
        n, p, off = int(case["length"][r]), int(case["pad"][r]), int(case["row_off"][r])
        qs = np.arange(case["q_col0"], case["q_col0"] + n_q) - p
        ok = (qs >= 0) & (qs < n)
        if off < 0 or not ok.any():
            continue
        Q, K = q[off + qs[ok]], k[r, :, :n]                                   # [nv, nh, 128], [nh, n, 128]
        s = np.einsum("ihd,hkd->hik", Q, K) * case["scale"]
        future = np.arange(n)[None, None, :] > qs[ok][None, :, None]
        s = np.where(future, -np.inf, s)
        P = np.exp(s - s.max(-1, keepdims=True)); P /= P.sum(-1, keepdims=True)
        sabs = np.where(future, 0.0, np.einsum("ihd,hkd->hik", np.abs(Q), np.abs(K)) * case["scale"]).max(-1).max(0)     # [nv]
        col = np.arange(n) + p
        for j in range(S):
            ind = (col >= case["lo"][r, j]) & (col < case["hi"][r, j])
            A[r, ok, j] = (P * ind).sum(-1).mean(0)
        nk = qs[ok] + 1
        bound[r, ok] = np.expm1(2 * 131 * U * sabs) + partition_bound(nk, nh)
    assert bound.max() <= BOUND_CAP, f"family {case['family']}: bound {bound.max():.3e} exceeds 2^-7"
    return A, bound


def span_mass_emulated(case, defect=None):
    """The kernel's arithmetic in numpy float32 -> [R, n_q, S]; ``defect`` (one of DEFECTS) plants the named mistake."""
    assert defect is None or defect in DEFECTS
    f32 = np.float32
    q, k = case["q"], case["k"]
    R, S, n_q, nh = len(case["length"]), case["lo"].shape[1], case["n_q"], case["nh"]
    scale = f32(case["scale"])
    out = np.zeros((R, n_q, S), dtype=f32)
    for r in range(R):
        n, p, off = int(case["length"][r]), int(case["pad"][r]), int(case["row_off"][r])
        shift = 0 if defect == "col_as_slot" else p                          # the defect reads columns as slots
        qs = np.arange(case["q_col0"], case["q_col0"] + n_q) - shift
        ok = (qs >= 0) & (qs < n)
        if off < 0 or not ok.any():
            continue
        qv = qs[ok]
        lo = case["lo"][r] - shift + (1 if defect == "lo_plus1" else 0)
        hi = case["hi"][r] - shift + (1 if defect == "hi_plus1" else 0)
        K = k[r, :, :n]
        nkeys = n
        if defect == "pad_keys":                                             # the p pad columns counted as keys (zero vectors) in front of the real ones
            K = np.concatenate([np.zeros((nh, p, 128), dtype=f32), K], axis=1)
            nkeys, qv, lo, hi = n + p, qv + p, lo + p, hi + p
        hsum = np.zeros((len(qv), S), dtype=f32)
        for h in range(nh):
            s = (q[off + qs[ok], h] @ K[h].T).astype(f32) * scale             # [nv, nkeys]
            limit = nkeys if defect == "no_causal" else qv.max() + 1
            m = np.full(len(qv), -np.inf, dtype=f32); l = np.zeros(len(qv), dtype=f32); e = np.zeros((len(qv), S), dtype=f32)
            for kb in range(0, int(limit), 64):
                keys = np.arange(kb, min(kb + 64, nkeys))
                st = s[:, keys].copy()
                if defect != "no_causal":
                    st[keys[None, :] > qv[:, None]] = -np.inf
                mx = np.maximum(m, st.max(-1))
                alpha = np.exp(m - mx, dtype=f32)
                pr = np.exp(st - mx[:, None], dtype=f32)
                hi_p = bf16(pr); lo_p = bf16(pr - hi_p)
                E = ((keys[:, None] >= lo[None, :]) & (keys[:, None] < hi[None, :])).astype(f32)
                l = l * alpha + pr.sum(-1, dtype=f32)
                if defect != "no_rescale":
                    e = e * alpha[:, None]
                e = (e + hi_p @ E + lo_p @ E).astype(f32)
                m = mx
            hsum += e / l[:, None]
        out[r, ok] = hsum if defect == "no_head_div" else hsum * f32(1.0 / nh)
    return out


def worst(got, ref, bound):
    """(largest |got - ref|, largest |got - ref| / bound over the entries with bound > 0, all exact entries equal)."""
    d = np.abs(got.astype(np.float64) - ref)
    b = np.broadcast_to(bound[..., None], d.shape)
    pos = b > 0
    return float(d.max()), float((d[pos] / b[pos]).max()) if pos.any() else 0.0, bool((d[~pos] == 0).all())
