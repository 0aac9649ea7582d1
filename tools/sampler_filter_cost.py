#!/usr/bin/env python3
"""What top-k / top-p filtering costs the image decode loop on the bench workload (full-size synthetic weights, bs 64, L 256,
576 steps, CFG 5, T 1): whole-loop decode_ms (pg_get_timing) with filters off and with top_k=1000, top_p=0.95, alternated and
repeated, plus the sampler class time (class 7) of one time_attn=1 pass of each.  One JSON line per measurement, a summary last.
usage: sampler_filter_cost.py [--reps 3] [--batch 64] [--prompt-len 256]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--top-p", type=float, default=0.95)
    a = ap.parse_args()
    import torch
    from bench import synth_prompts
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    cfg = PlanGenConfig.janus_pro_1b()
    B, L, T = a.batch, a.prompt_len, cfg.img_tokens
    eng = Engine(cfg, dtype="bf16", max_rows=2 * B, max_prompt=L, max_new=T, max_images=B)
    eng.init_synthetic(seed=0)
    ids, mask = synth_prompts(B, L, cfg.vocab, cfg.pad_id, seed=0)
    pad = Engine.pad_len_from_mask(mask, L)
    shared = Engine.uncond_rows_shared(ids, pad)
    modes = {"off": (0, 1.0), "on": (a.top_k, a.top_p)}

    def loop(mode, seed):
        k, p = modes[mode]
        eng.prefill(ids, pad, position_mode=0, uncond_shared=shared)
        toks = eng.decode_image_tokens(T=T, cfg_weight=5.0, temperature=1.0, seed=seed, top_k=k, top_p=p)
        torch.cuda.synchronize()
        return toks, eng.timing()["decode_ms"]

    for mode in modes:                                           # warm-up (graph capture, first-call allocations)
        loop(mode, 1)
    res = {m: [] for m in modes}
    for r in range(a.reps):
        for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):
            _, ms = loop(mode, 100 + r)
            res[mode].append(ms)
            print(json.dumps({"rep": r, "mode": mode, "decode_ms": round(ms, 3)}), flush=True)
    cls = {}
    for mode in modes:
        eng.set_option("time_attn", 1)
        loop(mode, 7)
        eng.set_option("time_attn", 0)
        c = eng.class_timing()
        name = "decode_cfg_sampler"
        cls[mode] = {"sampler_ms_sum": round(c[name]["ms_sum"], 3), "launches": c[name]["launches"],
                     "us_per_step": round(c[name]["ms_sum"] * 1e3 / T, 2)}
    med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
    out = {"workload": f"bs{B} L{L} T{T} cfg5 temp1", "filters_on": {"top_k": a.top_k, "top_p": a.top_p},
           "decode_ms_off": [round(x, 3) for x in res["off"]], "decode_ms_on": [round(x, 3) for x in res["on"]],
           "median_off": round(med["off"], 3), "median_on": round(med["on"], 3),
           "spread_off": round(max(res["off"]) - min(res["off"]), 3), "spread_on": round(max(res["on"]) - min(res["on"]), 3),
           "added_us_per_step": round((med["on"] - med["off"]) * 1e3 / T, 2), "sampler_class": cls}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
