#!/usr/bin/env python3
"""What merging a LoRA checkpoint costs at load time, on ONE bf16 engine of Janus-Pro-1B size with synthetic weights: a rank-256 adapter on
q / k / v / o_proj of all 24 layers (tuning_mode 'lora': 96 pg_merge_lora calls, each a host -> device copy of A and B, the fp32 staging and the merge
kernel, synchronous) beside the pg_finalize_weights that follows it, and the merge kernel alone on one 2048 x 2048 bf16 weight (device events,
pg_diag_op_lora_merge on device buffers).  ``reps`` repeats after one warm-up; host wall-clock around synchronous calls for the first two, device events
for the third.  No threshold: this is load-time work outside bench.py's timed region.  Writes a markdown table.
usage: lora_merge_cost.py [reps=3] [out.md=profiles/lora_merge.md]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from plangen_amd import _lib
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_md = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lora_merge.md")
RANK, ALPHA = 256, 128.0                                   # lora_rank / lora_alpha of the reference's cfg/base.py

cfg = PlanGenConfig.janus_pro_1b()
e = Engine(cfg, dtype="bf16", max_rows=2, max_prompt=64, max_new=8, max_images=1, diag=True)
e.init_synthetic(seed=0)
H, HD = cfg.hidden, cfg.n_heads * cfg.head_dim
g = torch.Generator().manual_seed(0)
adapters = {}
for i in range(cfg.n_layers):
    for mod, (o, n) in (("q_proj", (HD, H)), ("k_proj", (HD, H)), ("v_proj", (HD, H)), ("o_proj", (H, HD))):
        adapters[f"language_model.model.layers.{i}.self_attn.{mod}.weight"] = (torch.randn(RANK, n, generator=g) * 1e-3, torch.randn(o, RANK, generator=g) * 1e-3)


def med(v):
    return sorted(v)[len(v) // 2]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


merge_ms, fin_ms = [], []
for it in range(reps + 1):                                  # the merges stack (the adapters are small): the time does not depend on the contents
    m, f = wall(lambda: e.load_lora(adapters, ALPHA)), wall(lambda: e.finalize())
    if it:
        merge_ms.append(m); fin_ms.append(f)

d = _lib.load_diag()
d.pg_diag_op_lora_merge.restype = C.c_int
d.pg_diag_op_lora_merge.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
W = (torch.randn(H, H, generator=g) * 0.02).to(torch.bfloat16).cuda()
A, B = (torch.randn(RANK, H, generator=g) * 1e-3).cuda(), (torch.randn(H, RANK, generator=g) * 1e-3).cuda()
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
kern_ms = []
for it in range(reps + 1):
    ev0.record()
    rc = d.pg_diag_op_lora_merge(1, 0, W.data_ptr(), H, H, A.data_ptr(), B.data_ptr(), RANK, ALPHA / RANK, torch.cuda.current_stream().cuda_stream)
    ev1.record()
    torch.cuda.synchronize()
    assert rc == 0
    if it:
        kern_ms.append(ev0.elapsed_time(ev1))
e.close()


def row(name, v):
    return f"| {name} | {med(v):.2f} | {min(v):.2f} - {max(v):.2f} |"


mb = sum(a.numel() + b.numel() for a, b in adapters.values()) * 4 / 2 ** 20
md = ["# Cost of merging a LoRA checkpoint at load time", "",
      f"`tools/lora_merge_cost.py`: one bf16 engine of Janus-Pro-1B size, synthetic weights; rank {RANK}, alpha {ALPHA:g}, q / k / v / o_proj of {cfg.n_layers} layers",
      f"({len(adapters)} pairs, {mb:.0f} MiB of fp32 A and B on the host); {reps} repeats after a warm-up; ms (median, min - max).  Load-time work, outside bench.py's timed region.", "",
      "| what | median | min - max |", "|---|---|---|",
      row(f"Engine.load_lora: {len(adapters)} x pg_merge_lora (copy + staging + kernel, synchronous; host wall-clock)", merge_ms),
      row("Engine.finalize after it (pg_finalize_weights; host wall-clock)", fin_ms),
      row(f"merge kernel alone, one {H} x {H} bf16 weight, rank {RANK} (device events)", kern_ms), "",
      f"The kernel alone over {len(adapters)} weights: {med(kern_ms) * len(adapters):.1f} ms of the {med(merge_ms):.1f} ms; the rest is the pageable host -> device copies and the",
      "per-call synchronisation.", ""]
print("\n".join(md))
with open(out_md, "w") as f:
    f.write("\n".join(md))
