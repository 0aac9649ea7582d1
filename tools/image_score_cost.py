#!/usr/bin/env python3
"""What scoring given images costs, on ONE engine in ONE process (full-size synthetic weights, bf16, gen_head at 16 384 x 2048).
(a) head only, n = 16 x 576 and 64 x 576 scored positions (every position its own cond and uncond row: 2 n rows of layer-1 output):
      fused      pg_op_cfg_head_logprob: the fused CFG-mixed gen_head layer 2 + log-softmax kernel, no logits written
      composed   what works without it, in chunks of pairs whose fp32 logits stay <= 64 MB: gather [cond rows | uncond rows], pg_op_gemm (the
                 256x256 MFMA kernel) into fp32 logits, the mix (torch.lerp + the bias add, two elementwise passes), pg_op_token_logprob
    Gate: the fused head is not slower than the composition (at both sizes).
(b) end to end, 16 images, L = 256, T = 576:
      score_image   embeddings + ONE teacher-forced prefill of 256 + 575 columns + pg_score_image_tokens
      loop          prefill + decode_image_tokens(force_tokens=codes, force_mask=zeros, return_logprobs=True): 576 decode steps
    Gate: score_image is shorter.  The ratio is reported, not fixed in advance.
Forms are alternated ``reps`` times after one warm-up of each (device events on the engine's stream; the forms of one run are compared with
each other, never with a stored figure).  Writes profiles/image_score_cost.md and .json.
usage: image_score_cost.py [reps=5] [out.md|-] [parts=a,b]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from plangen_amd.config import PlanGenConfig
from plangen_amd.engine import Engine, head_logprob_geometry

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_md = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "image_score_cost.md")
out_md = None if out_md == "-" else out_md
parts = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else ("a", "b")

cfg = PlanGenConfig.janus_pro_1b()
V, K, T = cfg.img_vocab, cfg.gen_head_dim, cfg.img_tokens
PEAK = 2.5e15            # bf16 MFMA peak of an MI355X
B, L = 16, 256
CFG_W, TEMP = 5.0, 1.0
CHUNK = (64 << 20) // (8 * V)          # pairs per chunk of the composition: 2 * CHUNK fp32 logit rows = 64 MB
e = Engine(cfg, dtype="bf16", max_rows=2 * B, max_prompt=L + T - 1, max_new=T, max_images=1)
e.init_synthetic(seed=0)
dev = e.device
g = torch.Generator(device=dev).manual_seed(1)
W = (torch.randn(V, K, generator=g, device=dev) * 0.02).bfloat16()
bias = torch.randn(V, generator=g, device=dev) * 0.1
logits = torch.empty((2 * CHUNK, V), dtype=torch.float32, device=dev)


def med(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); out = fn(); t1.record()
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def fused(x, ci, ui, tgt, out):
    n = tgt.numel()
    rc = e.lib.pg_op_cfg_head_logprob(e.h, e._p(x), x.shape[0], e._p(W), V, K, e._p(bias), e._p(ci), e._p(ui), e._p(tgt), n, C.c_float(CFG_W),
                                      C.c_float(TEMP), e._p(out), e.stream)
    assert rc == 0, e.lib.pg_last_error(e.h)
    return out


def composed(x, ci, ui, tgt, out):
    S = C.c_int(0)
    n = tgt.numel()
    for r0 in range(0, n, CHUNK):
        cn = min(CHUNK, n - r0)
        xg = torch.cat([x.index_select(0, ci[r0:r0 + cn].long()), x.index_select(0, ui[r0:r0 + cn].long())])
        rc = e.lib.pg_op_gemm(e.h, e._p(xg), e._p(W), e._p(logits), 2 * cn, V, K, 0, C.byref(S), e.stream)
        assert rc == 0 and S.value == 1, e.lib.pg_last_error(e.h)
        mixed = logits[:cn]
        torch.lerp(logits[cn:2 * cn], logits[:cn], CFG_W, out=mixed)      # u + w (c - u), in place over the cond rows
        mixed.add_(bias)
        rc = e.lib.pg_op_token_logprob(e.h, e._p(mixed), cn, V, e._p(tgt[r0:]), C.c_float(TEMP), e._p(out[r0:]), e.stream)
        assert rc == 0, e.lib.pg_last_error(e.h)
    return out


result = dict(reps=reps, V=V, K=K, T=T, cfg_weight=CFG_W, temperature=TEMP, head=[], end_to_end=None)
lines = ["# Scoring given images: the fused CFG gen_head + log-softmax head, and one prefill against the 576-step loop", "",
         f"One process, one bf16 engine (Janus-Pro-1B shapes, img_vocab {V}, gen_head_dim {K}), forms alternated {reps}x after a warm-up of each; device events.",
         "", "## (a) head only", "", "| images | n | form | median ms | min | max | extra device bytes | TFLOP/s | MFMA rate |", "|---|---|---|---|---|---|---|---|---|"]
gates = []
if "a" in parts:
    for images in (16, 64):
        n = images * T
        x = torch.randn(2 * n, K, generator=g, device=dev).bfloat16()
        ci = (2 * torch.arange(n, device=dev)).int()
        ui = ci + 1
        tgt = torch.randint(0, V, (n,), generator=g, device=dev).int()
        forms = {"fused": fused, "composed": composed}
        outs = {f: torch.zeros(n, dtype=torch.float32, device=dev) for f in forms}
        for f, fn in forms.items():
            fn(x, ci, ui, tgt, outs[f])
        torch.cuda.synchronize()
        diff = (outs["fused"] - outs["composed"]).abs().max().item()
        ms = {f: [] for f in forms}
        for _ in range(reps):
            for f, fn in forms.items():
                ms[f].append(timed(lambda: fn(x, ci, ui, tgt, outs[f]))[1])
        geom = head_logprob_geometry(2 * n, V, K)
        extra = {"fused": (8 * geom["G"] * n + 255) // 256 * 256, "composed": 4 * 2 * CHUNK * V + 2 * 2 * CHUNK * K}
        for f in forms:
            m = med(ms[f]); fl = 2.0 * 2 * n * V * K / (m * 1e-3)
            lines.append(f"| {images} | {n} | {f} | {m:.3f} | {min(ms[f]):.3f} | {max(ms[f]):.3f} | {extra[f]} | {fl / 1e12:.0f} | {fl / PEAK:.3f} |")
            print(lines[-1], flush=True)
        lines.append(f"| {images} | {n} | max abs difference of the two forms' results | {diff:.2e} | | | G = {geom['G']}, {geom['cpt']} column tiles per group | | |")
        print(lines[-1], flush=True)
        gates.append((images, med(ms["fused"]), med(ms["composed"])))
        result["head"].append(dict(images=images, n=n, fused_ms=ms["fused"], composed_ms=ms["composed"], max_abs_diff=diff, G=geom["G"], cpt=geom["cpt"],
                                   fused_ws_bytes=extra["fused"], composed_ws_bytes=extra["composed"]))
        del x, outs
    for images, f_ms, c_ms in gates:
        lines += ["", f"Gate ({images} images, fused not slower than the composition): fused {f_ms:.3f} ms, composed {c_ms:.3f} ms -> "
                  f"{'MET' if f_ms <= c_ms else 'MISSED'} (ratio {f_ms / c_ms:.3f})."]
        print(lines[-1], flush=True)

if "b" in parts:
    gi = torch.Generator().manual_seed(2)
    ids = torch.randint(8, cfg.vocab, (2 * B, L), generator=gi).int()
    pad = [int(v) for v in torch.randint(0, 32, (2 * B,), generator=gi)]
    codes = torch.randint(0, V, (B, T), generator=gi).int()
    zeros = torch.zeros((B, T), dtype=torch.uint8)

    def score():
        return e.score_image(ids, pad, codes, CFG_W, TEMP)

    def loop():
        e.prefill(ids, pad, position_mode=0)
        return e.decode_image_tokens(T, CFG_W, TEMP, force_tokens=codes, force_mask=zeros, return_logprobs=True)[1]
    forms = {"score_image": score, "loop": loop}
    res = {f: fn() for f, fn in forms.items()}
    torch.cuda.synchronize()
    diff = (res["score_image"] - res["loop"]).abs().max().item()
    ms = {f: [] for f in forms}
    for _ in range(reps):
        for f, fn in forms.items():
            ms[f].append(timed(fn)[1])
    s_ms, l_ms = med(ms["score_image"]), med(ms["loop"])
    lines += ["", f"## (b) end to end, {B} images, L = {L}, T = {T}", "", "| form | median ms | min | max |", "|---|---|---|---|"]
    for f in forms:
        lines.append(f"| {f} | {med(ms[f]):.2f} | {min(ms[f]):.2f} | {max(ms[f]):.2f} |")
        print(lines[-1], flush=True)
    lines += ["", f"Largest |score_image - loop| over the {B * T} tokens (bf16: one whole-sequence pass against 576 single steps, different GEMM shapes and "
              f"attention kernels): {diff:.3e}.",
              "", f"Gate (score_image shorter than the teacher-forced loop): {s_ms:.2f} ms against {l_ms:.2f} ms -> {'MET' if s_ms < l_ms else 'MISSED'} "
              f"(the loop takes {l_ms / s_ms:.2f}x as long)."]
    print(lines[-1], flush=True)
    result["end_to_end"] = dict(images=B, L=L, T=T, score_image_ms=ms["score_image"], loop_ms=ms["loop"], max_abs_diff=diff)
if out_md:
    os.makedirs(os.path.dirname(out_md), exist_ok=True)
    with open(out_md, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.splitext(out_md)[0] + ".json", "w") as f:
        json.dump(result, f, indent=1)
