#!/usr/bin/env python3
"""What token log-probabilities cost, and what select_best saves, on ONE engine in ONE process (full-size synthetic weights, bf16).
  bench      the bench shape (64 images = 128 rows, prompt 256, 576 sampled steps): the decode loop with and without a score request
  stage1     uni_2stage stage 1 (32 rows, prompt 128, 256 forced-length sampled tokens at vocab 102 400): the text loop with and without
  select     16 prompts x 4 replicas (128 rows, share_replicas): scored loop + VQ decode of the 16 kept images against the plain
             parallel_size = 4 form, unscored loop + VQ decode of all 64
Every pair alternates A/B ``reps`` times after one warm-up of each form; times are device events (the library's own pair around the image
loop and the VQ decode: pg_get_timing; torch events on the engine's stream around the text call).  The forms of one run are compared
with each other, never with a stored figure; the spread of a form's repeats is printed beside every difference.  Tokens of the scored and
the unscored form are asserted equal.  Writes profiles/logprob_cost.json and .md.
usage: logprob_cost.py [reps=3] [out.json|-] [out.md|-] [shapes=bench,stage1,select]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bench import synth_prompts
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine
from plangen_amd.system import System

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_json = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "logprob_cost.json")
out_md = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "logprob_cost.md")
shapes = tuple(sys.argv[4].split(",")) if len(sys.argv) > 4 else ("bench", "stage1", "select")
out_json = None if out_json == "-" else out_json
out_md = None if out_md == "-" else out_md

cfg = PlanGenConfig.janus_pro_1b()
T, L, NT = cfg.img_tokens, 256, 256
e = Engine(cfg, dtype="bf16", max_rows=128, max_prompt=L, max_new=T, max_images=64, with_lm_head=True)
e.init_synthetic(seed=0)


def med(v):
    return sorted(v)[len(v) // 2]


def alternate(forms, run):
    """one warm-up per form (returns its output), then ``reps`` rounds A, B, A, B ...; -> (outputs, {form: [ms dicts]})"""
    outs = {f: run(f)[0] for f in forms}
    res = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            res[f].append(run(f)[1])
    return outs, res


def summary(res, key):
    return {f: {"median_ms": round(med([r[key] for r in v]), 3), "min_ms": round(min(r[key] for r in v), 3),
                "max_ms": round(max(r[key] for r in v), 3)} for f, v in res.items()}


rep = {"reps": reps, "dtype": "bf16", "weights": "synthetic seed 0", "shapes": {}}

if "bench" in shapes:
    B = 64
    ids, mask = synth_prompts(B, L, cfg.vocab, cfg.pad_id, seed=0)
    mask = torch.cat([mask, torch.ones((2 * B, T), dtype=torch.int32)], 1)
    pad = Engine.pad_len_from_mask(mask, L)
    shared = Engine.uncond_rows_shared(ids, pad)

    def run(form):
        e.prefill(ids, pad, position_mode=0, uncond_shared=shared)
        out = e.decode_image_tokens(T=T, cfg_weight=cfg.cfg_weight, temperature=1.0, seed=0, return_logprobs=form == "scored")
        torch.cuda.synchronize()
        toks = out[0] if form == "scored" else out
        return toks.cpu(), {"decode_ms": e.timing()["decode_ms"]}

    outs, res = alternate(("plain", "scored"), run)
    assert torch.equal(outs["plain"], outs["scored"]), "a score request changed the tokens"
    s = summary(res, "decode_ms")
    d = s["scored"]["median_ms"] - s["plain"]["median_ms"]
    rep["shapes"]["bench"] = {"images": B, "rows": 2 * B, "prompt_len": L, "steps": T, "decode_ms": s,
                              "added_ms": round(d, 3), "added_us_per_step": round(d * 1e3 / T, 2),
                              "added_share": round(d / s["plain"]["median_ms"], 5)}
    print(json.dumps(rep["shapes"]["bench"]), flush=True)

if "stage1" in shapes:
    B, Lt = 32, 128
    g = torch.Generator().manual_seed(0)
    tids = torch.randint(10, cfg.vocab - 2048, (B, Lt), generator=g).int()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(form):
        e.prefill(tids, [0] * B, position_mode=1)
        ev0.record()
        out = e.generate_text(NT, cfg.eos_id, min_new_tokens=NT, temperature=1.0, top_k=50, top_p=0.9, seed=0,
                              return_logprobs=form == "scored")
        ev1.record()
        torch.cuda.synchronize()
        toks = out[0] if form == "scored" else out
        assert toks.shape == (B, NT)
        return toks.cpu(), {"text_ms": ev0.elapsed_time(ev1)}

    for name, kw in (("filtered_k50_p0.9", None),):
        outs, res = alternate(("plain", "scored"), run)
        assert torch.equal(outs["plain"], outs["scored"]), "a score request changed the tokens"
        s = summary(res, "text_ms")
        d = s["scored"]["median_ms"] - s["plain"]["median_ms"]
        rep["shapes"]["stage1"] = {"rows": B, "prompt_len": Lt, "tokens": NT, "vocab": cfg.vocab, "sampler": name, "text_ms": s,
                                   "added_ms": round(d, 3), "added_us_per_step": round(d * 1e3 / NT, 2),
                                   "added_share": round(d / s["plain"]["median_ms"], 5)}
    print(json.dumps(rep["shapes"]["stage1"]), flush=True)

if "select" in shapes:
    from types import SimpleNamespace
    B0, P = 16, 4
    ids, mask = synth_prompts(B0, L, cfg.vocab, cfg.pad_id, seed=0)
    mask = torch.cat([mask, torch.ones((2 * B0, T), dtype=torch.int32)], 1)
    base = dict(seed=0, parallel_size=P, cfg_weight=cfg.cfg_weight, temperature=1.0, top_k=0, top_p=1.0, use_teacher_forcing=False,
                debug_max_seq_len=None, janus_hw=cfg.img_size, neg_prompt="", use_neg_box=False, share_replicas=1)
    systems = {"plain": System(cfg, e, SimpleNamespace(**base)), "select_best": System(cfg, e, SimpleNamespace(select_best=True, **base))}

    def run(form):
        s = systems[form]
        dec, _ = s.t2i(ids, mask)
        torch.cuda.synchronize()
        t = e.timing()
        assert dec.shape[0] == (B0 if form == "select_best" else B0 * P)
        return s.last_generated_tokens.cpu(), {"decode_ms": t["decode_ms"], "vq_ms": t["vq_ms"], "loop_plus_vq_ms": t["decode_ms"] + t["vq_ms"]}

    outs, res = alternate(("plain", "select_best"), run)
    rows = systems["select_best"].last_selection["replica"].cpu() * B0 + torch.arange(B0)
    assert torch.equal(outs["select_best"], outs["plain"][rows]), "select_best kept rows that are not the plain run's"
    s = {k: summary(res, k) for k in ("decode_ms", "vq_ms", "loop_plus_vq_ms")}
    d = s["loop_plus_vq_ms"]["select_best"]["median_ms"] - s["loop_plus_vq_ms"]["plain"]["median_ms"]
    rep["shapes"]["select"] = {"prompts": B0, "replicas": P, "rows": 2 * B0 * P, "prompt_len": L, "steps": T, **s,
                               "select_best_minus_plain_ms": round(d, 3),
                               "share_of_plain": round(d / s["loop_plus_vq_ms"]["plain"]["median_ms"], 5),
                               "images_returned": {"plain": B0 * P, "select_best": B0}}
    print(json.dumps(rep["shapes"]["select"]), flush=True)

e.close()
if out_json:
    with open(out_json, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
if out_md:
    def line(name, s):
        return f"| {name} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} |"
    md = ["# Cost of token log-probabilities, saving of select_best", "",
          f"`tools/logprob_cost.py`: one engine, one process, bf16, synthetic weights; every pair alternates A/B, {reps} repeats after a warm-up;",
          "device-event times in ms (median, min - max of the repeats).  Tokens of the scored and unscored forms are equal (asserted).", ""]
    sh = rep["shapes"]
    if "bench" in sh:
        b = sh["bench"]
        md += [f"## Bench shape: {b['images']} images, prompt {b['prompt_len']}, {b['steps']} steps (decode loop)", "", "| form | median | min - max |", "|---|---|---|",
               line("no request", b["decode_ms"]["plain"]), line("with log-probs", b["decode_ms"]["scored"]), "",
               f"Added by the request: {b['added_ms']} ms = {b['added_us_per_step']} us per step = {100 * b['added_share']:.2f} % of the loop.", ""]
    if "stage1" in sh:
        b = sh["stage1"]
        md += [f"## uni_2stage stage 1: {b['rows']} rows, {b['tokens']} tokens, vocab {b['vocab']} ({b['sampler']})", "", "| form | median | min - max |", "|---|---|---|",
               line("no request", b["text_ms"]["plain"]), line("with log-probs", b["text_ms"]["scored"]), "",
               f"Added by the request: {b['added_ms']} ms = {b['added_us_per_step']} us per step = {100 * b['added_share']:.2f} % of the loop.", ""]
    if "select" in sh:
        b = sh["select"]
        md += [f"## select_best: {b['prompts']} prompts x {b['replicas']} replicas (share_replicas), loop + VQ decode", "",
               "| form | loop median | VQ median | loop + VQ median | min - max |", "|---|---|---|---|---|"]
        for f, name in (("plain", f"parallel_size = {b['replicas']}: VQ of {b['images_returned']['plain']}"),
                        ("select_best", f"select_best: scored loop, VQ of {b['images_returned']['select_best']}")):
            t = b["loop_plus_vq_ms"][f]
            md.append(f"| {name} | {b['decode_ms'][f]['median_ms']} | {b['vq_ms'][f]['median_ms']} | {t['median_ms']} | {t['min_ms']} - {t['max_ms']} |")
        md += ["", f"select_best minus plain: {b['select_best_minus_plain_ms']} ms = {100 * b['share_of_plain']:.2f} % of the plain form's loop + VQ time "
               "(the PCIe copy and the files of the 48 images that are no longer produced are not in these figures).", ""]
    with open(out_md, "w") as f:
        f.write("\n".join(md))
