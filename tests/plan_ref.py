"""Host model of one image-sampler step under a sample plan (pg_request_sample_plan, include/plangen_hip.h), built on tests/draw_ref.py: the CFG mix with
w[bg, step], and per image its temperature (<= 0: greedy, filter ignored), its keep set of (top_k, top_p) and its image_key in the RNG stream key.  The
``mutant`` argument plants one wrong reading of the definition; tests/test_plan_ref_cpu.py shows that the comparison the GPU tests make catches each of them
on the families below.  CPU only."""
from __future__ import annotations

import numpy as np

import draw_ref as D

MUTANTS = ("w_local_b", "w_step_major", "temp_of_image0", "key_ignored", "greedy_perturbed", "filter_shifted")
PLAN_V = (1, 17, 1000, 16384)
PLAN_S = (1, 2, 5)
PLAN_B = 3
PLAN_T = 576
# (b_off, B_total): draw_ref.IMG_OFFS read as the first global image of the launch and the images of the plan (the operator indexes the plan by bg = b_off + b)
PLAN_OFFS = tuple((b_off, max(b_off + PLAN_B, min(n, 8))) for b_off, n in D.IMG_OFFS)


def stream_key(key, step):
    with np.errstate(over="ignore"):
        return D._u64(key) * D.U64(D.KEY_MUL) + D._u64(step)


def cfg_mix(cond, uncond, w, b_off, step, mutant=None):
    """mixed [B, V] in fp64: u + w[bg, step] (c - u), bg = b_off + b.  w [B_total, T]."""
    B = len(cond)
    T = w.shape[1]
    if mutant == "w_local_b":
        wb = w[np.arange(B), step]
    elif mutant == "w_step_major":
        wb = w.reshape(-1)[(step * w.shape[0] + b_off + np.arange(B)) % w.size]
    else:
        wb = w[b_off + np.arange(B), step]
    c, u = np.asarray(cond, dtype=np.float64), np.asarray(uncond, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return u + wb.astype(np.float64)[:, None] * (c - u)


def keep_set(row, temperature, top_k, top_p):
    """bool [V]: the kept set of the filtered sampler's rule (sampling_filter_ref.rule_keep); everything finite-or-+inf when the filter is off."""
    if top_k <= 0 and top_p >= 1.0:
        return None
    import torch
    import sampling_filter_ref as F
    return F.rule_keep(torch.from_numpy(np.asarray(row, dtype=np.float32))[None], float(temperature), int(top_k), float(top_p))[0].numpy()


def step_model(cond, uncond, plan, b_off, step, seed, mutant=None):
    """One planned step for the images [b_off, b_off + B).  plan: dict of w [B_total, T], temperature, top_k, top_p, key [B_total].  Returns (mixed [B, V] fp64,
    token [B], gap [B], scale [B], runner-up [B], sampled [B]); a greedy image has gap = inf (its token binds whenever the row has no tie to fp64)."""
    B, V = np.asarray(cond).shape
    mixed = cfg_mix(cond, uncond, plan["w"], b_off, step, mutant)
    tok = np.zeros(B, dtype=np.int64); gap = np.full(B, np.inf); scale = np.zeros(B); ru = np.zeros(B, dtype=np.int64); sampled = np.zeros(B, dtype=bool)
    for b in range(B):
        bg = b_off + b
        t = float(plan["temperature"][0 if mutant == "temp_of_image0" else bg])
        fb = min(bg + 1, len(plan["top_k"]) - 1) if mutant == "filter_shifted" else bg
        key = bg if mutant == "key_ignored" else int(plan["key"][bg])
        if t <= 0 and mutant == "greedy_perturbed":
            t = 1.0
        if t <= 0:
            tok[b] = D.greedy(mixed[b:b + 1])[0]
            ru[b] = tok[b]
            continue
        keep = keep_set(mixed[b], t, int(plan["top_k"][fb]), float(plan["top_p"][fb]))
        k, g, s, r = D.draw_top2(mixed[b:b + 1], t, seed, stream_key(key, step), None if keep is None else keep[None])
        tok[b], gap[b], scale[b], ru[b], sampled[b] = k[0], g[0], s[0], r[0], True
    return mixed, tok, gap, scale, ru, sampled


def plan_cases(V, S):
    """The sub-cases of one (V, S) parametrisation: draw_ref.image_cases(V, S, bias off) at B = 3, each given a plan over B_total images -- per-image
    temperatures from draw_ref.IMG_T and weights from draw_ref.IMG_W varying over images AND steps, distinct keys that are not the image index, and
    (V >= 1000) one image with an active filter.  Yields dicts: slabs [S, 2B, V], plan, b_off, B_total, seed, steps."""
    rng = np.random.default_rng(300000 + V * 8 + S)
    i = 0
    for c in D.image_cases(V, S, False):
        if c["B"] != PLAN_B:
            continue
        b_off, B_total = PLAN_OFFS[i % len(PLAN_OFFS)]
        w = rng.choice(np.asarray(D.IMG_W, dtype=np.float32), size=(B_total, PLAN_T))
        for step in D.IMG_CASE_STEPS:                                     # at the steps drawn, neighbouring images and steps differ
            w[:, step] = np.roll(np.resize(np.asarray(D.IMG_W, dtype=np.float32), B_total), step + i)
        temperature = np.roll(np.resize(np.asarray(D.IMG_T, dtype=np.float32), B_total), i)
        key = (rng.permutation(4096)[:B_total] + 7).astype(np.int32)
        top_k = np.zeros(B_total, dtype=np.int32); top_p = np.ones(B_total, dtype=np.float32)
        if V >= 1000:
            top_k[b_off + 1] = 50; top_p[b_off + 1] = 0.9
        yield dict(slabs=c["slabs"], b_off=b_off, B_total=B_total, seed=c["seed"], steps=D.IMG_CASE_STEPS,
                   plan=dict(w=w, temperature=temperature, top_k=top_k, top_p=top_p, key=key))
        i += 1


def cond_uncond(c):
    s = c["slabs"].astype(np.float64).sum(0)
    return s[0::2], s[1::2]


def filtered(plan):
    return bool(((plan["temperature"] > 0) & ((plan["top_k"] > 0) | (plan["top_p"] < 1))).any())
