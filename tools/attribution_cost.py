#!/usr/bin/env python3
"""What the attention-span request (pg_request_attn_spans) adds to score_image's prefill, on ONE engine in ONE process
(full-size synthetic weights, bf16): 16 images, L = 256 prompt columns, T = 576 image tokens -> 32 rows of 831 columns through
pg_prefill_embeds,
      plain     the prefill alone
      spans     the same prefill with a request for ALL layers, 16 spans per row, the 576 predicting queries (columns L - 1 .. L + T - 2)
alternated ``reps`` times after one warm-up of each (device events on the engine's stream; the two forms of one run are compared with each
other, never with a stored figure).  The added time is the number; no threshold is set.  Also recorded: the bytes the request writes against
the [R, heads, W, W] bf16 tensor per layer that output_attentions=True would hold.  Writes profiles/attribution_cost.md.
usage: attribution_cost.py [reps=5] [out.md|-]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_md = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "attribution_cost.md")
out_md = None if out_md == "-" else out_md

cfg = PlanGenConfig.janus_pro_1b()
B, L, T, S = 16, 256, cfg.img_tokens, 16
R, W = 2 * B, L + T - 1
e = Engine(cfg, dtype="bf16", max_rows=R, max_prompt=W, max_new=1, max_images=1)
e.init_synthetic(seed=0)
g = torch.Generator().manual_seed(1)
pad = [int(v) for v in torch.randint(0, 64, (R,), generator=g)]
emb = (torch.randn(R, W, cfg.hidden, generator=g) * 0.05).to(e.device)
edges = torch.linspace(0, L, S + 1).round().int()
lo, hi = edges[:-1].repeat(R, 1), edges[1:].repeat(R, 1)             # 16 spans that tile the prompt columns
spans = (lo, hi, L - 1, T, None)


def med(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); out = fn(); t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def plain():
    return e.prefill_embeds(emb, pad, position_mode=0)


def with_spans():
    return e.prefill_embeds(emb, pad, position_mode=0, attn_spans=spans)[1]


plain(); mass = with_spans()
torch.cuda.synchronize()
t_plain, t_spans = [], []
for _ in range(reps):
    t_plain.append(timed(plain)[1])
    t_spans.append(timed(with_spans)[1])
a, b = med(t_plain), med(t_spans)
written = mass.numel() * 4
held = R * cfg.n_heads * W * W * 2
lines = [
    "# Cost of the attention-span request (tools/attribution_cost.py)",
    "",
    f"One MI355X, bf16, full-size synthetic weights; {B} images, L = {L}, T = {T}: {R} rows x {W} columns, {sum(W - p for p in pad)} packed tokens;",
    f"request: all {cfg.n_layers} layers, {S} spans per row, {T} queries.  Medians of {reps} alternated runs, device events.",
    "",
    "| form | prefill ms |",
    "|---|---|",
    f"| plain | {a:.2f} |",
    f"| with the request | {b:.2f} |",
    f"| added | {b - a:.2f} ({100 * (b - a) / a:.1f} %), {(b - a) / cfg.n_layers * 1e3:.0f} us per layer |",
    "",
    f"Written by the request: {written / 2 ** 20:.1f} MiB in all ({written // cfg.n_layers / 2 ** 20:.2f} MiB per layer); the [R, {cfg.n_heads}, W, W] bf16 probabilities",
    f"the reference route holds: {held / 2 ** 20:.0f} MiB PER LAYER ({held / (written // cfg.n_layers):.0f}x).",
    f"Check: the {S} spans tile the prompt, so at the first predicting query (column L - 1: all of its keys lie in the prompt) they sum to 1;",
    f"largest |sum_s A - 1| over layers and rows there: {float((mass[:, :, 0].sum(-1) - 1.0).abs().max()):.2e}.",
]
text = "\n".join(lines) + "\n"
print(text)
if out_md:
    with open(out_md, "w") as f:
        f.write(text)
