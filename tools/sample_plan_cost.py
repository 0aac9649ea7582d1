#!/usr/bin/env python3
"""What a sample plan costs in the image decode loop, on ONE engine in ONE process (full-size synthetic weights, bf16): the bench shape (64 images =
128 rows, prompt 256, 576 sampled steps) with no request and with a FULL plan -- all five arrays, a different weight at every (image, step), per-image
temperatures around 1, no active filter (the planned unfiltered route: the same three launches per step) -- alternated A/B ``reps`` times after one
warm-up of each form.  Times are the library's own device-event pair around the loop (pg_get_timing).  The per-step difference is printed with the
spread of each form's repeats.  A constant plan is asserted to give the tokens of the call without one.
``lib=PATH`` loads another build of libplangen_hip.so (the parent commit's, which has no plan entry point: then only the no-request loop runs), so
that the no-request figure of this build can be set beside the parent's from the same tool on the same machine.
usage: sample_plan_cost.py [reps=5] [out.json|-] [out.md|-] [lib=PATH]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if not a.startswith("lib=")]
alt_lib = next((a[4:] for a in sys.argv[1:] if a.startswith("lib=")), None)
from plangen_amd import _lib

has_plan = True
if alt_lib:
    import ctypes as C
    import torch  # noqa: F401  (its HIP runtime must be the one mapped before any build of the library is opened: _lib.load)
    _lib.LIB_PATH = os.path.abspath(alt_lib)
    probe = C.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    have = lambda n: probe is not None and hasattr(probe, n)
    has_plan = have("pg_request_sample_plan")
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if have(s[0])]           # an older build: bind what it exports
import numpy as np
import torch
from bench import synth_prompts
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine

reps = int(args[0]) if len(args) > 0 else 5
out_json = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "sample_plan_cost.json")
out_md = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "sample_plan_cost.md")
out_json = None if out_json == "-" else out_json
out_md = None if out_md == "-" else out_md

cfg = PlanGenConfig.janus_pro_1b()
T, L, B = cfg.img_tokens, 256, 64
e = Engine(cfg, dtype="bf16", max_rows=2 * B, max_prompt=L, max_new=T, max_images=B, with_lm_head=True)
e.init_synthetic(seed=0)
ids, mask = synth_prompts(B, L, cfg.vocab, cfg.pad_id, seed=0)
mask = torch.cat([mask, torch.ones((2 * B, T), dtype=torch.int32)], 1)
pad = Engine.pad_len_from_mask(mask, L)
shared = Engine.uncond_rows_shared(ids, pad)
plans = {}
if has_plan:
    from plangen_amd.guidance import SamplePlan
    rng = np.random.default_rng(0)
    plans["planned"] = SamplePlan(cfg_weight=rng.uniform(3.0, 9.0, size=(B, T)), temperature=rng.uniform(0.8, 1.2, size=B), top_k=np.zeros(B, dtype=np.int64),
                                  top_p=np.ones(B), image_key=rng.permutation(B))
    plans["constant"] = SamplePlan(cfg_weight=np.full((B, T), cfg.cfg_weight), temperature=np.ones(B), top_k=np.zeros(B, dtype=np.int64), top_p=np.ones(B),
                                   image_key=np.arange(B))


def run(form):
    e.prefill(ids, pad, position_mode=0, uncond_shared=shared)
    kw = {"plan": plans[form]} if form in plans else {}
    out = e.decode_image_tokens(T=T, cfg_weight=cfg.cfg_weight, temperature=1.0, seed=0, **kw)
    torch.cuda.synchronize()
    return out.cpu(), e.timing()["decode_ms"]


def stat(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3), "spread_ms": round(v[-1] - v[0], 3)}


forms = ("plain", "planned") if has_plan else ("plain",)
warm = {f: run(f)[0] for f in forms}
if has_plan:
    assert torch.equal(run("constant")[0], warm["plain"]), "a constant plan changed the tokens"
res = {f: [] for f in forms}
for _ in range(reps):
    for f in forms:
        res[f].append(run(f)[1])
e.close()
rep = {"reps": reps, "dtype": "bf16", "weights": "synthetic seed 0", "library": alt_lib or "this build", "images": B, "rows": 2 * B, "prompt_len": L, "steps": T,
       "decode_ms": {f: stat(v) for f, v in res.items()}, "runs_ms": {f: [round(x, 3) for x in v] for f, v in res.items()}}
if has_plan:
    d = rep["decode_ms"]["planned"]["median_ms"] - rep["decode_ms"]["plain"]["median_ms"]
    rep.update(added_ms=round(d, 3), added_us_per_step=round(d * 1e3 / T, 2), added_share=round(d / rep["decode_ms"]["plain"]["median_ms"], 5))
print(json.dumps(rep), flush=True)
if out_json:
    with open(out_json, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
if out_md:
    md = ["# Cost of a sample plan in the image decode loop", "",
          f"`tools/sample_plan_cost.py`: one engine, one process, bf16, synthetic weights, {B} images, prompt {L}, {T} steps; A/B alternated, {reps} repeats after a",
          "warm-up of each form; the library's device-event time of the loop in ms.  A constant plan gives the tokens of the call without one (asserted).", "",
          "| form | median | min - max | spread |", "|---|---|---|---|"]
    for f, name in (("plain", "no request"), ("planned", "full plan (five arrays, a weight per image and step)")):
        if f in rep["decode_ms"]:
            s = rep["decode_ms"][f]
            md.append(f"| {name} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {s['spread_ms']} |")
    if has_plan:
        md += ["", f"Added by the plan: {rep['added_ms']} ms = {rep['added_us_per_step']} us per step = {100 * rep['added_share']:.3f} % of the loop.", ""]
    with open(out_md, "w") as f:
        f.write("\n".join(md))
