#!/usr/bin/env python3
"""What dual guidance costs in the image decode loop, on ONE engine in ONE process (full-size synthetic weights, bf16): the bench shape's 64 images with
the pair loop (128 rows, the shared negative prompt as the bench runs it) and with the dual loop (192 rows: full prompt, a caption-only prompt of half
the length, negative prompt; no sharing), prompt 256, 576 sampled steps, alternated A/B ``reps`` times after one warm-up of each form.  Times are the
library's own device-event pair around the loop (pg_get_timing); the prefill is not in them.
``lib=PATH`` loads another build of libplangen_hip.so (the parent commit's, which has no dual entry point: then only the pair loop runs), so that the
pair figure of this build can be set beside the parent's from the same tool on the same machine.  Such a run writes its record to
profiles/dual_guidance_cost_parent.json and no report of its own; the report of a run of this build (profiles/dual_guidance_cost.md) ends with the
comparison whenever that record lies beside its own JSON.  ``render`` rewrites the report from the two committed records without a GPU.
usage: dual_guidance_cost.py [reps=3] [out.json|-] [out.md|-] [lib=PATH]
       dual_guidance_cost.py render [in.json] [out.md]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = [a for a in sys.argv[1:] if not a.startswith("lib=")]
alt_lib = next((a[4:] for a in sys.argv[1:] if a.startswith("lib=")), None)
PROFILES = os.path.join(ROOT, "profiles")


def parent_record_path(json_path):
    """The record of the ``lib=`` run that belongs to a record of this build: NAME.json -> NAME_parent.json."""
    return json_path[:-5] + "_parent.json" if json_path and json_path.endswith(".json") else None


def render(rep, parent, out_md):
    B, L, T, reps = rep["images"], rep["prompt_len"], rep["steps"], rep["reps"]
    md = ["# Cost of dual guidance in the image decode loop", "",
          f"`tools/dual_guidance_cost.py` ({rep['library']}): one engine, one process, bf16, synthetic weights, {B} images, prompt {L}, {T} sampled steps; A/B",
          f"alternated, {reps} repeats after a warm-up of each form; the library's device-event time of the loop in ms (prefill excluded).", "",
          "| loop | rows | median | min - max | spread |", "|---|---|---|---|---|"]
    for f, name in (("pair", "pair (cond / uncond, shared negative prompt)"), ("dual", "dual (full / caption / negative, nothing shared)")):
        if f in rep["decode_ms"]:
            s = rep["decode_ms"][f]
            md.append(f"| {name} | {rep['rows'][f]} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {s['spread_ms']} |")
    if "dual_over_pair" in rep:
        md += ["", f"Dual over pair: {rep['dual_over_pair']} x for 1.5 x the rows."]
    if parent is not None:
        a, b = rep["decode_ms"]["pair"], parent["decode_ms"]["pair"]
        md += ["", f"The pair loop against another build (`lib={parent['library']}`, the same tool in a process of its own, {parent['reps']} repeats): this build",
               f"{a['median_ms']} ms ({a['min_ms']} - {a['max_ms']}), that build {b['median_ms']} ms ({b['min_ms']} - {b['max_ms']}): "
               f"{100.0 * (a['median_ms'] / b['median_ms'] - 1.0):+.2f} %."]
    with open(out_md, "w") as f:
        f.write("\n".join(md) + "\n")


if args and args[0] == "render":
    src = args[1] if len(args) > 1 else os.path.join(PROFILES, "dual_guidance_cost.json")
    pp = parent_record_path(src)
    render(json.load(open(src)), json.load(open(pp)) if pp and os.path.exists(pp) else None, args[2] if len(args) > 2 else src[:-5] + ".md")
    sys.exit(0)
from plangen_amd import _lib

has_dual = True
if alt_lib:
    import ctypes as C
    import torch  # noqa: F401  (its HIP runtime must be the one mapped before any build of the library is opened: _lib.load)
    _lib.LIB_PATH = os.path.abspath(alt_lib)
    probe = C.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    have = lambda n: probe is not None and hasattr(probe, n)
    has_dual = have("pg_decode_image_tokens_dual")
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if have(s[0])]           # an older build: bind what it exports
import torch
from bench import synth_prompts
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine
from plangen_amd.system import t2i_dual_collate_batch

reps = int(args[0]) if len(args) > 0 else 3
out_json = args[1] if len(args) > 1 else os.path.join(PROFILES, "dual_guidance_cost_parent.json" if alt_lib else "dual_guidance_cost.json")
out_md = args[2] if len(args) > 2 else ("-" if alt_lib else os.path.join(PROFILES, "dual_guidance_cost.md"))
out_json = None if out_json == "-" else out_json
out_md = None if out_md == "-" else out_md

cfg = PlanGenConfig.janus_pro_1b()
T, L, B = cfg.img_tokens, 256, 64
e = Engine(cfg, dtype="bf16", max_rows=3 * B if has_dual else 2 * B, max_prompt=L, max_new=T, max_images=B, with_lm_head=True)
e.init_synthetic(seed=0)
ids, mask = synth_prompts(B, L, cfg.vocab, cfg.pad_id, seed=0)
pad = Engine.pad_len_from_mask(torch.cat([mask, torch.ones((2 * B, T), dtype=torch.int32)], 1), L)
shared = Engine.uncond_rows_shared(ids, pad)
rows = [ids[r][mask[r].bool()].tolist() for r in range(2 * B)]
ids3, mask3 = t2i_dual_collate_batch(rows[0::2], [r[:max(1, len(r) // 2)] for r in rows[0::2]], rows[1::2], cfg.pad_id, T)
pad3 = Engine.pad_len_from_mask(mask3, ids3.shape[1])


def run(form):
    if form == "pair":
        e.prefill(ids, pad, position_mode=0, uncond_shared=shared)
        out = e.decode_image_tokens(T=T, cfg_weight=cfg.cfg_weight, temperature=1.0, seed=0)
    else:
        e.prefill(ids3, pad3, position_mode=0, uncond_shared=False)
        out = e.decode_image_tokens_dual(T, cfg.cfg_weight, 2.0, temperature=1.0, seed=0)
    torch.cuda.synchronize()
    return out.cpu(), e.timing()["decode_ms"]


def stat(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3), "spread_ms": round(v[-1] - v[0], 3)}


forms = ("pair", "dual") if has_dual else ("pair",)
for f in forms:
    run(f)
res = {f: [] for f in forms}
for _ in range(reps):
    for f in forms:
        res[f].append(run(f)[1])
e.close()
rep = {"reps": reps, "dtype": "bf16", "weights": "synthetic seed 0", "library": alt_lib or "this build", "images": B, "rows": {"pair": 2 * B, "dual": 3 * B},
       "prompt_len": L, "steps": T, "pair_negative_prompt_shared": bool(shared), "decode_ms": {f: stat(v) for f, v in res.items()},
       "runs_ms": {f: [round(x, 3) for x in v] for f, v in res.items()}}
if has_dual:
    rep["dual_over_pair"] = round(rep["decode_ms"]["dual"]["median_ms"] / rep["decode_ms"]["pair"]["median_ms"], 4)
print(json.dumps(rep), flush=True)
if out_json:
    with open(out_json, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
if out_md:
    pp = parent_record_path(out_json)
    render(rep, json.load(open(pp)) if pp and os.path.exists(pp) else None, out_md)
