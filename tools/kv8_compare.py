#!/usr/bin/env python3
"""bf16 KV cache against the opt-in FP8 KV cache at the bench shape, in ONE process: 2 x batch rows, prompt length 256, 576 greedy steps,
bf16 compute, uncond_shared_hint = 1, synthetic weights (bench.py's).  After one warm-up per handle the two handles alternate ``rounds``
times (box drift shows as the spread between a handle's rounds); every pass reports pg_get_timing().decode_ms, then one instrumented pass
per handle (time_attn) reports the attention class: time, bytes actually read, GB/s.  Also the free-running greedy token agreement of the
two modes on these prompts.  The comparison is between the two handles of this run, never against a stored figure.
usage: kv8_compare.py [batch=64] [rounds=2] [steps=576] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bench import synth_prompts
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
T = int(sys.argv[3]) if len(sys.argv) > 3 else 576
out_path = sys.argv[4] if len(sys.argv) > 4 else None
cfg = PlanGenConfig.janus_pro_1b()
L = 256
ids, mask = synth_prompts(B, L, cfg.vocab, cfg.pad_id, seed=0)
mask = torch.cat([mask, torch.ones((2 * B, cfg.img_tokens), dtype=torch.int32)], 1)
pad = Engine.pad_len_from_mask(mask, L)
shared = Engine.uncond_rows_shared(ids, pad)
eng = {}
for kv in ("bf16", "fp8"):
    e = Engine(cfg, dtype="bf16", max_rows=2 * B, max_prompt=L, max_new=cfg.img_tokens, max_images=B, kv_dtype=kv)
    e.init_synthetic(seed=0)
    eng[kv] = e


def loop(e, timed=False):
    e.set_option("time_attn", int(timed))
    e.set_option("time_stride", 8)
    e.prefill(ids, pad, position_mode=0, uncond_shared=shared)
    toks = e.decode_image_tokens(T=T, cfg_weight=cfg.cfg_weight, temperature=0.0)
    torch.cuda.synchronize()
    t = e.timing()
    return toks.cpu(), t, (e.class_timing() if timed else None)


rep = {"batch": B, "rows": 2 * B, "prompt_len": L, "steps": T, "uncond_shared": bool(shared), "device_bytes": {k: e.device_bytes() for k, e in eng.items()},
       "decode_ms": {"bf16": [], "fp8": []}}
toks = {}
for kv, e in eng.items():
    toks[kv], _, _ = loop(e)                                   # warm-up (and the tokens)
for _ in range(rounds):
    for kv, e in eng.items():
        rep["decode_ms"][kv].append(round(loop(e)[1]["decode_ms"], 2))
rep["attention_class"] = {}
for kv, e in eng.items():
    _, t, cls = loop(e, timed=True)
    a = cls["decode_attention"]
    rep["attention_class"][kv] = {"ms_sum": round(a["ms_sum"], 3), "launches": a["launches"], "bytes_sum": a["bytes_sum"],
                                  "GB_per_s": round(a["bytes_sum"] / max(a["ms_sum"], 1e-9) / 1e6, 1), "time_stride": 8,
                                  "us_per_launch": round(1e3 * a["ms_sum"] / max(a["launches"], 1), 2)}
    e.set_option("time_attn", 0)
same = (toks["bf16"] == toks["fp8"])
rep["free_running_token_agreement"] = round(float(same.float().mean()), 4)
rep["first_divergence_step_median"] = float(torch.where(same.all(1), torch.tensor(T), (~same).int().argmax(1)).float().median())
mb, m8 = min(rep["decode_ms"]["bf16"]), min(rep["decode_ms"]["fp8"])
rep["fp8_over_bf16_loop_time"] = round(m8 / mb, 4)
line = json.dumps(rep)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
