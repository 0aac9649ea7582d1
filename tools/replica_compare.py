#!/usr/bin/env python3
"""parallel_size replicas, three ways, in ONE process on ONE handle: 16 images x p = 4 replicas (128 rows), prompt length L, 576 sampled steps
(temperature 1), bf16, synthetic weights (bench.py's).  (a) plain: pg_prefill of the replicated ids; (b) pg_prefill_replicated alias = 0 (one
prefill, prompt K/V copied into the replicas' rows, today's decode kernels); (c) alias = 1 (replicas read their owner's prompt K/V in the
grouped decode attention).  After one warm-up each the three forms alternate ``rounds`` times (box drift shows as the spread between a form's
rounds); every pass reports prefill_ms and decode_ms, then one instrumented pass per form (time_attn on every 8th step) reports the attention
class: us per launch and algorithmic bytes.  The forms of one run are compared with each other, never with a stored figure.
Under a profiler: ``forms`` restricts the run to some of the three (e.g. "plain" or "alias1") and rounds = 0 leaves the warm-up pass only.
usage: replica_compare.py [L=256] [rounds=2] [steps=576] [out.json|-] [out.md|-] [forms=plain,alias0,alias1]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bench import synth_prompts
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine

L = int(sys.argv[1]) if len(sys.argv) > 1 else 256
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
T = int(sys.argv[3]) if len(sys.argv) > 3 else 576
out_json = sys.argv[4] if len(sys.argv) > 4 else None
out_md = sys.argv[5] if len(sys.argv) > 5 else None
B0, P = 16, 4
cfg = PlanGenConfig.janus_pro_1b()
ids, mask = synth_prompts(B0, L, cfg.vocab, cfg.pad_id, seed=0)
mask = torch.cat([mask, torch.ones((2 * B0, cfg.img_tokens), dtype=torch.int32)], 1)
pad = Engine.pad_len_from_mask(mask, L)
ids_rep, pad_rep = torch.cat([ids] * P), pad * P
shared = Engine.uncond_rows_shared(ids_rep, pad_rep)
e = Engine(cfg, dtype="bf16", max_rows=2 * B0 * P, max_prompt=L, max_new=cfg.img_tokens, max_images=B0 * P)
e.init_synthetic(seed=0)
FORMS = tuple(sys.argv[6].split(",")) if len(sys.argv) > 6 else ("plain", "alias0", "alias1")
out_json = None if out_json == "-" else out_json
out_md = None if out_md == "-" else out_md


def loop(form, timed=False):
    e.set_option("time_attn", int(timed))
    e.set_option("time_stride", 8)
    if form == "plain":
        e.prefill(ids_rep, pad_rep, position_mode=0, uncond_shared=shared)
    else:
        e.prefill_replicated(ids, pad, P, alias=form == "alias1", uncond_shared=shared)
    toks = e.decode_image_tokens(T=T, cfg_weight=cfg.cfg_weight, temperature=1.0, seed=0)
    torch.cuda.synchronize()
    return toks.cpu(), e.timing(), (e.class_timing() if timed else None)


rep = {"images": B0, "replicas": P, "rows": 2 * B0 * P, "prompt_len": L, "steps": T, "uncond_shared": bool(shared),
       "prefill_ms": {f: [] for f in FORMS}, "decode_ms": {f: [] for f in FORMS}}
toks = {f: loop(f)[0] for f in FORMS}                               # warm-up (and the tokens)
for _ in range(rounds):
    for f in FORMS:
        t = loop(f)[1]
        rep["prefill_ms"][f].append(round(t["prefill_ms"], 3))
        rep["decode_ms"][f].append(round(t["decode_ms"], 2))
rep["attention_class"] = {}
if rounds < 1 or len(FORMS) < 3:          # profiler pass: nothing to compare
    print(json.dumps({"forms": FORMS, "steps": T, "prompt_len": L}))
    sys.exit(0)
for f in FORMS:
    a = loop(f, timed=True)[2]["decode_attention"]
    rep["attention_class"][f] = {"ms_sum": round(a["ms_sum"], 3), "launches": a["launches"], "bytes_sum": a["bytes_sum"], "time_stride": 8,
                                 "us_per_launch": round(1e3 * a["ms_sum"] / max(a["launches"], 1), 2)}
e.set_option("time_attn", 0)
rep["alias1_tokens_equal_alias0"] = bool(torch.equal(toks["alias1"], toks["alias0"]))
rep["tokens_equal_plain_share"] = round(float((toks["alias1"] == toks["plain"]).float().mean()), 4)
rep["spread_decode_ms"] = {f: round(max(v) - min(v), 2) for f, v in rep["decode_ms"].items()}
mn = {f: min(v) for f, v in rep["decode_ms"].items()}
rep["alias1_over_plain_decode"] = round(mn["alias1"] / mn["plain"], 4)
rep["alias0_over_plain_decode"] = round(mn["alias0"] / mn["plain"], 4)
line = json.dumps(rep)
print(line)
if out_json:
    with open(out_json, "a") as fh:
        fh.write(line + "\n")
if out_md:
    with open(out_md, "a") as fh:
        fh.write(f"\n### {B0} images x {P} replicas = {2 * B0 * P} rows, L = {L}, {T} sampled steps, bf16 (one process, forms alternated, {rounds} rounds)\n\n")
        fh.write("| form | prefill ms (rounds) | decode ms (rounds) | spread ms | attention us / launch | attention algorithmic GB (timed launches) |\n|---|---|---|---|---|---|\n")
        for f in FORMS:
            a = rep["attention_class"][f]
            fh.write(f"| {f} | {rep['prefill_ms'][f]} | {rep['decode_ms'][f]} | {rep['spread_decode_ms'][f]} | {a['us_per_launch']} | {a['bytes_sum'] / 1e9:.2f} |\n")
        fh.write(f"\nalias1 / plain decode time (best rounds): {rep['alias1_over_plain_decode']}; alias0 / plain: {rep['alias0_over_plain_decode']}; "
                 f"alias1 tokens == alias0 tokens: {rep['alias1_tokens_equal_alias0']}.\n")
