#!/usr/bin/env python3
"""What scoring given text costs, on ONE engine in ONE process (full-size synthetic weights, bf16, the real lm_head at vocab 102 400).
  a   n =  8 192 hidden rows (uni_2stage: 32 rows x 256 layout tokens)
  b   n = 40 960 hidden rows (mmu: 64 rows x 640)
Forms, alternated A / B ``reps`` times after one warm-up of each (device events on the engine's stream; the forms of one run are compared
with each other, never with a stored figure):
  fused      pg_score_tokens: the fused lm_head + log-softmax kernel, logits never written
  composed   what works without it: pg_op_gemm (the 256x256 MFMA kernel) into fp32 logits [rows, vocab], then pg_op_token_logprob --
             in chunks of 8 192 rows (one chunk at shape a), so its workspace is 3.4 GB
and the whole Engine.score_text call (prefill + index build + fused head) at shape a.  Results of both forms are compared (they differ
by summation order only).  Gate: at shape a the fused head is not slower than the composition.  Writes profiles/score_cost.md.
usage: score_cost.py [reps=5] [out.md|-] [shapes=a,b]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine, head_logprob_geometry

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_md = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "score_cost.md")
out_md = None if out_md == "-" else out_md
shapes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else ("a", "b")

cfg = PlanGenConfig.janus_pro_1b()
V, K, CHUNK = cfg.vocab, cfg.hidden, 8192
PEAK = 2.5e15            # bf16 MFMA peak of an MI355X
R, L = 32, 256
e = Engine(cfg, dtype="bf16", max_rows=R, max_prompt=L, max_new=8, max_images=1, with_lm_head=True)
e.init_synthetic(seed=0)
dev = e.device
g = torch.Generator(device=dev).manual_seed(1)
# the composition needs the weights as a caller tensor: the same synthetic draw is not reachable through the ABI, so both forms run on a
# caller-given W through pg_op_head_logprob / pg_op_gemm (same device code as pg_score_tokens), and score_text runs on the engine's own
W = (torch.randn(V, K, generator=g, device=dev) * 0.02).bfloat16()
logits = torch.empty((CHUNK, V), dtype=torch.float32, device=dev)


def med(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); out = fn(); t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def fused(x, tgt, out):
    rc = e.lib.pg_op_head_logprob(e.h, e._p(x), x.shape[0], e._p(W), V, K, None, e._p(tgt), x.shape[0], C.c_float(0.0), e._p(out), e.stream)
    assert rc == 0, e.lib.pg_last_error(e.h)
    return out


def composed(x, tgt, out):
    S = C.c_int(0)
    for r0 in range(0, x.shape[0], CHUNK):
        xc, n = x[r0:r0 + CHUNK], min(CHUNK, x.shape[0] - r0)
        rc = e.lib.pg_op_gemm(e.h, e._p(xc), e._p(W), e._p(logits), n, V, K, 0, C.byref(S), e.stream)
        assert rc == 0 and S.value == 1, e.lib.pg_last_error(e.h)
        rc = e.lib.pg_op_token_logprob(e.h, e._p(logits), n, V, e._p(tgt[r0:]), C.c_float(0.0), e._p(out[r0:]), e.stream)
        assert rc == 0, e.lib.pg_last_error(e.h)
    return out


lines = ["# Scoring given text: the fused lm_head + log-softmax head against GEMM + token_logprob", "",
         f"One process, one bf16 engine (Janus-Pro-1B shapes, vocab {V}, hidden {K}), forms alternated {reps}x after a warm-up of each; device events.",
         "", "| shape | n | form | median ms | min | max | extra device bytes | TFLOP/s | MFMA rate |", "|---|---|---|---|---|---|---|---|---|"]
gate = None
for name in shapes:
    n = {"a": 8192, "b": 40960}[name]
    x = (torch.randn(n, K, generator=g, device=dev)).bfloat16()
    tgt = torch.randint(0, V, (n,), generator=g, device=dev).int()
    outs = {f: torch.zeros(n, dtype=torch.float32, device=dev) for f in ("fused", "composed")}
    before = e.device_bytes()
    forms = {"fused": fused, "composed": composed}
    for f, fn in forms.items():
        fn(x, tgt, outs[f])
    torch.cuda.synchronize()
    ws = e.device_bytes() - before
    diff = (outs["fused"] - outs["composed"]).abs().max().item()
    ms = {f: [] for f in forms}
    for _ in range(reps):
        for f, fn in forms.items():
            ms[f].append(timed(lambda: fn(x, tgt, outs[f]))[1])
    geom = head_logprob_geometry(n, V, K)
    extra = {"fused": max(ws, geom["ws_bytes"]) if ws else geom["ws_bytes"], "composed": 4 * min(n, CHUNK) * V}
    for f in forms:
        m = med(ms[f]); fl = 2.0 * n * V * K / (m * 1e-3)
        lines.append(f"| {name} | {n} | {f} | {m:.3f} | {min(ms[f]):.3f} | {max(ms[f]):.3f} | {extra[f]} | {fl / 1e12:.0f} | {fl / PEAK:.3f} |")
        print(lines[-1], flush=True)
    lines.append(f"| {name} | {n} | max abs difference of the two forms' results | {diff:.2e} | | | G = {geom['G']}, {geom['cpt']} column tiles per group | | |")
    print(lines[-1], flush=True)
    if name == "a":
        gate = (med(ms["fused"]), med(ms["composed"]))

if "a" in shapes:
    gi = torch.Generator().manual_seed(2)
    ids = torch.randint(8, V, (R, L), generator=gi).int()
    pad = [int(v) for v in torch.randint(0, 32, (R,), generator=gi)]
    sf = [p + 1 for p in pad]
    e.score_text(ids, pad, sf); torch.cuda.synchronize()
    t = [timed(lambda: e.score_text(ids, pad, sf))[1] for _ in range(reps)]
    nsc = sum(L - s for s in sf)
    lines += ["", f"Engine.score_text, {R} rows x {L} columns ({nsc} scored tokens; prefill with hidden output + index build + fused head): "
              f"median {med(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f})."]
    print(lines[-1], flush=True)
if gate:
    lines += ["", f"Gate (shape a, fused not slower than the composition): fused {gate[0]:.3f} ms, composed {gate[1]:.3f} ms -> "
              f"{'MET' if gate[0] <= gate[1] else 'MISSED'} (ratio {gate[0] / gate[1]:.3f})."]
    print(lines[-1], flush=True)
if out_md:
    os.makedirs(os.path.dirname(out_md), exist_ok=True)
    with open(out_md, "w") as f:
        f.write("\n".join(lines) + "\n")
