#!/usr/bin/env python3
"""What the per-token uncertainty request (pg_request_token_stats) costs next to the log-probability request, on ONE engine in ONE process
(full-size synthetic weights, bf16; the shapes of tools/logprob_cost.py):
  bench      the bench shape (64 images = 128 rows, prompt 256, 576 sampled steps): the image loop
  stage1     uni_2stage stage 1 (32 rows, prompt 128, 256 forced-length sampled tokens at vocab 102 400): the text loop
each without any request, with the log-prob request, and with the stats request at n_alt = 0 and n_alt = 8.  The four forms alternate
``reps`` times after one warm-up of each; times are device events (the library's own pair around the image loop: pg_get_timing; torch
events on the engine's stream around the text call).  The forms of one run are compared with each other, never with a stored figure; the
spread of a form's repeats is printed beside every median.  Tokens of every form are asserted equal.  Writes profiles/token_stats_cost.md.
usage: token_stats_cost.py [reps=3] [out.md|-] [shapes=bench,stage1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bench import synth_prompts
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_md = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "token_stats_cost.md")
shapes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else ("bench", "stage1")
out_md = None if out_md == "-" else out_md

FORMS = {"plain": {}, "logprobs": {"return_logprobs": True}, "stats_n0": {"return_stats": True}, "stats_n8": {"return_stats": 8}}
NAMES = {"plain": "no request", "logprobs": "log-prob request", "stats_n0": "stats request, n_alt = 0", "stats_n8": "stats request, n_alt = 8"}

cfg = PlanGenConfig.janus_pro_1b()
T, L, NT = cfg.img_tokens, 256, 256
e = Engine(cfg, dtype="bf16", max_rows=128, max_prompt=L, max_new=T, max_images=64, with_lm_head=True)
e.init_synthetic(seed=0)


def med(v):
    return sorted(v)[len(v) // 2]


def alternate(run):
    outs = {f: run(f)[0] for f in FORMS}
    res = {f: [] for f in FORMS}
    for _ in range(reps):
        for f in FORMS:
            res[f].append(run(f)[1])
    for f in FORMS:
        assert torch.equal(outs[f], outs["plain"]), f"the {f} request changed the tokens"
    return {f: {"median_ms": round(med(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for f, v in res.items()}


def added(s, steps):
    out = {}
    for f in FORMS:
        if f != "plain":
            d = s[f]["median_ms"] - s["plain"]["median_ms"]
            out[f] = {"added_ms": round(d, 3), "added_us_per_step": round(d * 1e3 / steps, 2), "added_share": round(d / s["plain"]["median_ms"], 5)}
    return out


rep = {"reps": reps, "shapes": {}}
if "bench" in shapes:
    B = 64
    ids, mask = synth_prompts(B, L, cfg.vocab, cfg.pad_id, seed=0)
    mask = torch.cat([mask, torch.ones((2 * B, T), dtype=torch.int32)], 1)
    pad = Engine.pad_len_from_mask(mask, L)
    shared = Engine.uncond_rows_shared(ids, pad)

    def run(form):
        e.prefill(ids, pad, position_mode=0, uncond_shared=shared)
        out = e.decode_image_tokens(T=T, cfg_weight=cfg.cfg_weight, temperature=1.0, seed=0, **FORMS[form])
        torch.cuda.synchronize()
        return (out[0] if FORMS[form] else out).cpu(), e.timing()["decode_ms"]

    s = alternate(run)
    rep["shapes"]["bench"] = {"title": f"Bench shape: {B} images, prompt {L}, {T} steps (image loop)", "steps": T, "ms": s, "added": added(s, T)}
    print(json.dumps(rep["shapes"]["bench"]), flush=True)

if "stage1" in shapes:
    B, Lt = 32, 128
    g = torch.Generator().manual_seed(0)
    tids = torch.randint(10, cfg.vocab - 2048, (B, Lt), generator=g).int()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(form):
        e.prefill(tids, [0] * B, position_mode=1)
        ev0.record()
        out = e.generate_text(NT, cfg.eos_id, min_new_tokens=NT, temperature=1.0, top_k=50, top_p=0.9, seed=0, **FORMS[form])
        ev1.record()
        torch.cuda.synchronize()
        toks = out[0] if FORMS[form] else out
        assert toks.shape == (B, NT)
        return toks.cpu(), ev0.elapsed_time(ev1)

    s = alternate(run)
    rep["shapes"]["stage1"] = {"title": f"uni_2stage stage 1: {B} rows, {NT} tokens, vocab {cfg.vocab} (top-k 50, top-p 0.9; text loop)", "steps": NT,
                               "ms": s, "added": added(s, NT)}
    print(json.dumps(rep["shapes"]["stage1"]), flush=True)

e.close()
if out_md:
    md = ["# Cost of the per-token uncertainty request (entropy, rank, top-N) next to the log-probability request", "",
          f"`tools/token_stats_cost.py`: one engine, one process, bf16, synthetic weights; the four forms alternate, {reps} repeats after a warm-up",
          "of each; device-event times in ms (median, min - max of the repeats).  The tokens of all forms are equal (asserted).", ""]
    for b in rep["shapes"].values():
        md += [f"## {b['title']}", "", "| form | median | min - max | added ms | added us / step | share of the loop |", "|---|---|---|---|---|---|"]
        for f in FORMS:
            s, a = b["ms"][f], b["added"].get(f)
            tail = f"{a['added_ms']} | {a['added_us_per_step']} | {100 * a['added_share']:.2f} %" if a else "| |"
            md.append(f"| {NAMES[f]} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {tail} |")
        lp, s8 = b["added"]["logprobs"]["added_ms"], b["added"]["stats_n8"]["added_ms"]
        md += ["", f"Stats request (n_alt = 8) / log-prob request: {s8} ms / {lp} ms" + (f" = {s8 / lp:.2f}x." if lp > 0 else "."), ""]
    with open(out_md, "w") as f:
        f.write("\n".join(md))
