"""Host model of one image-sampler step under dual guidance (pg_decode_image_tokens_dual, include/plangen_hip.h), built on tests/draw_ref.py like
tests/plan_ref.py: three rows per image -- 3b = f (caption + layout), 3b + 1 = p (caption only), 3b + 2 = u (negative) --

    mixed = (u + w_caption (p - u)) + w_layout (f - p)

in fp64 on dyadic slabs and dyadic weights (every intermediate is exact in fp32, so the device's row is known bit for bit), then the draw of draw_ref with the
stream key of the global image.  The ``mutant`` argument plants one wrong reading of the definition; tests/test_dual_ref_cpu.py shows that the comparison the
GPU test makes catches each of them on the families below.  Also the three-row greedy decode loop over the oracle's model functions (``sample_image_dual``).
CPU only."""
from __future__ import annotations

import numpy as np

import draw_ref as D
from plan_ref import keep_set, stream_key  # noqa: F401  (re-exported: the GPU tests take them from here)

MUTANTS = ("fp_swapped", "w_swapped", "layout_vs_u", "pair_stride", "w_image0_chunk0")
DUAL_V = (1, 17, 1000, 16384)
DUAL_S = (1, 2, 5)
DUAL_B = 3
DUAL_T = 576
CHUNKS = 16                                                   # CFG_CHUNKS of the scan's grid
# (w_caption, w_layout): dyadic and unequal.  Slab sums are multiples of 2^-6 below 40 (+ bias), so every term of the mix is a multiple of 2^-8 below
# 40 + 7 * 80 + 7 * 80 < 2^11: 19 bits at most, exact in fp32 whichever way the compiler contracts the expression
DUAL_W = ((5.0, 1.0), (1.0, 5.0), (2.5, 7.0), (0.0, 3.0), (1.5, 0.0), (5.0, 0.25))
DUAL_T_ = (0.0, 0.7, 1.3)
# (b_off, img_off, B_total): the launch covers images [b_off, b_off + B) of B_total
DUAL_OFFS = ((0, 0, DUAL_B + 1), (2, 5, 8), (1, 4000, 6))


def rows_fpu(slabs, bias=None, mutant=None):
    """(f, p, u) [B, V] fp64 from slabs [S, 3B, V]: bias first, then the slabs in index order (exact on dyadic values, so the order does not show here)."""
    s = np.asarray(slabs, dtype=np.float64).sum(0)
    if bias is not None:
        s = s + np.asarray(bias, dtype=np.float64)[None, :]
    B = s.shape[0] // 3
    if mutant == "pair_stride":
        idx = 2 * np.arange(B)
        return s[idx], s[idx + 1], s[idx + 2]
    return s[0::3], s[1::3], s[2::3]


def mix(f, p, u, w_caption, w_layout, mutant=None):
    """mixed [B, V] in fp64."""
    wc, wl = float(w_caption), float(w_layout)
    if mutant == "fp_swapped":
        f, p = p, f
    if mutant == "w_swapped":
        wc, wl = wl, wc
    with np.errstate(invalid="ignore"):
        if mutant == "layout_vs_u":
            return (u + wc * (p - u)) + wl * (f - u)
        out = (u + wc * (p - u)) + wl * (f - p)
        if mutant == "w_image0_chunk0":                       # the layout weight reaches the first chunk of image 0 only; everything else gets w_caption for both
            V = out.shape[1]
            per = (V + CHUNKS - 1) // CHUNKS
            wrong = (u + wc * (p - u)) + wc * (f - p)
            wrong[0, :per] = out[0, :per]
            return wrong
        return out


def step_model(slabs, bias, w_caption, w_layout, temperature, top_k, top_p, b_off, img_off, step, seed, mutant=None):
    """One dual step for the images [b_off, b_off + B).  Returns (mixed [B, V] fp64, token [B], gap [B], scale [B], runner-up [B], keep [B, V] or None);
    greedy (temperature <= 0): gap = inf, the token binds whenever the row has no tie to fp64."""
    f, p, u = rows_fpu(slabs, bias, mutant)
    mixed = mix(f, p, u, w_caption, w_layout, mutant)
    B = len(mixed)
    if temperature <= 0:
        tok = D.greedy(mixed)
        return mixed, tok, np.full(B, np.inf), np.zeros(B), tok.copy(), None
    keep = None
    if top_k > 0 or top_p < 1.0:
        keep = np.stack([keep_set(mixed[b], temperature, top_k, top_p) for b in range(B)])
    tok, gap, scale, ru = D.draw_top2(mixed, temperature, seed, D.image_key(np.arange(B), b_off, img_off, step), keep)
    return mixed, tok, gap, scale, ru, keep


def dual_cases(V, S, with_bias=False):
    """The sub-cases of one (V, S) parametrisation of the operator test: every weight pair, temperatures and offsets rotating, and (V >= 1000) every
    third sampled case filtered.  Yields dicts: slabs [S, 3B, V], bias, w_caption, w_layout, T (temperature), top_k, top_p, b_off, img_off, B_total, seed, steps."""
    rng = np.random.default_rng(400000 + V * 64 + S * 2 + int(with_bias))
    i = n_sampled = 0
    for wc, wl in DUAL_W:
        for t in DUAL_T_:
            b_off, img_off, B_total = DUAL_OFFS[i % len(DUAL_OFFS)]
            slabs = D.dyadic_slabs(rng, S, 3 * DUAL_B, V, 1.5)
            bias = (np.rint(rng.standard_normal(V) * 0.5 * D.Q) / D.Q).astype(np.float32) if with_bias else None
            top_k, top_p = 0, 1.0
            if t > 0:
                if V >= 1000 and n_sampled % 3 == 1:
                    top_k, top_p = 50, 0.9
                n_sampled += 1
            yield dict(slabs=slabs, bias=bias, w_caption=wc, w_layout=wl, T=t, top_k=top_k, top_p=top_p, b_off=b_off, img_off=img_off, B_total=B_total,
                       seed=D.IMG_SEED + 31 * i, steps=D.IMG_CASE_STEPS)
            i += 1


def case_model(c, step, mutant=None):
    return step_model(c["slabs"], c["bias"], c["w_caption"], c["w_layout"], c["T"], c["top_k"], c["top_p"], c["b_off"], c["img_off"], step, c["seed"], mutant)


# ---------------------------------------------------------------------------------------------------------------- the decode loop (oracle model functions)
def collate_triples(full_ids, caption_ids, neg_ids, pad_id, img_tokens):
    """ids [3B, L], mask [3B, L + img_tokens]: row 3b = full_ids[b], 3b + 1 = caption_ids[b], 3b + 2 = neg_ids (one shared list, or one per sample); every row
    left-padded to the longest of all."""
    import torch
    from oracle.ref_cpu import pad_input_ids
    B = len(full_ids)
    negs = [list(n) for n in neg_ids] if len(neg_ids) > 0 and not isinstance(neg_ids[0], int) else [list(neg_ids)] * B
    rows = []
    for b in range(B):
        rows += [list(full_ids[b]), list(caption_ids[b]), negs[b]]
    ids, mask = pad_input_ids(rows, pad_id)
    mask = torch.cat([mask, torch.ones((3 * B, img_tokens)).to(mask)], dim=-1)
    return ids.int(), mask.int()


def sample_image_dual(W, cfg, inputs_embeds, mask, w_caption, w_layout, n_tokens=None, force_tokens=None, edit_region=None, gt_labels=None,
                      return_logits=False):
    """oracle.ref_cpu.sample_image over triples of rows, greedy: inputs_embeds [3B, L, H] (3b = f, 3b + 1 = p, 3b + 2 = u), mask [3B, L + T].
    ``force_tokens`` [B, T] teacher-forces the fed-back token; ``edit_region`` / ``gt_labels`` is the use_teacher_forcing branch (where edit_region == 0
    the emitted and fed-back token is the label).  Returns tokens int32 [B, T] (+ mixed logits [T, B, V])."""
    import torch
    from oracle.ref_cpu import gen_head, llama_forward, prepare_gen_img_embeds
    R = inputs_embeds.shape[0]
    assert R % 3 == 0
    B = R // 3
    T = cfg.img_tokens if n_tokens is None else n_tokens
    tokens = torch.zeros((B, T), dtype=torch.int32)
    all_logits = []
    cache = None
    x = inputs_embeds
    for i in range(T):
        past = 0 if cache is None else cache.length()
        q = x.shape[1]
        pos = torch.arange(past, past + q)[None].expand(R, q)
        hidden, cache = llama_forward(W, cfg, x, mask, pos, cache)
        logits = gen_head(W, hidden[:, -1, :])
        f, p, u = logits[0::3], logits[1::3], logits[2::3]
        mixed = (u + w_caption * (p - u)) + w_layout * (f - p)
        nxt = torch.argmax(mixed, dim=-1).to(torch.int32)
        if return_logits:
            all_logits.append(mixed)
        if edit_region is not None:
            nxt = torch.where(edit_region[:, i] == 0, gt_labels[:, i].to(torch.int32), nxt)
        tokens[:, i] = nxt
        feed = nxt if force_tokens is None else force_tokens[:, i].to(torch.int32)
        x = prepare_gen_img_embeds(W, torch.stack([feed, feed, feed], dim=1).view(-1))[:, None, :]
    if return_logits:
        return tokens, torch.stack(all_logits)
    return tokens
