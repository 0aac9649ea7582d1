#!/usr/bin/env python3
"""What pg_prefill_extend saves, on ONE engine in ONE process (synthetic weights, bf16).
  forced   the bench shape (64 pairs = 128 rows, prompt 256, 576 image tokens), every token forced: the parent-capability 576-step forced
           loop against  prefill + extend(t0) + (576 - t0) steps  for t0 in {64, 288, 512}
  mmu      64 rows, one image each (1 + vit_tokens + tail embeddings): System.mmu_ask with 4 questions against 4 independent mmu runs
Same build, same process, forms alternated ``reps`` times after one warm-up of each, medians; torch events on the current stream around the
whole form (prefill included: the extension path prefills without the shared negative prompt, which is part of its cost).  Forced tokens
of both forms are asserted equal.  No figure here is a pass / fail criterion.  Writes profiles/extend_cost.md.
usage: extend_cost.py [reps=3] [out.md|-] [shapes=forced,mmu] [config=full|tiny]"""
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
out_md = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "extend_cost.md")
shapes = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else ("forced", "mmu")
tiny = len(sys.argv) > 4 and sys.argv[4] == "tiny"

cfg = PlanGenConfig.tiny() if tiny else PlanGenConfig.janus_pro_1b()
T = cfg.img_tokens
B, L, BM, NQ, QLEN = (2, 16, 2, 4, 6) if tiny else (64, 256, 64, 4, 32)
T0S = [t for t in ((8, 32, 56) if tiny else (64, 288, 512))]
LM = 1 + cfg.vit_tokens + QLEN
e = Engine(cfg, dtype="bf16", max_rows=2 * B, max_prompt=max(L, LM), max_new=T, max_images=4, with_lm_head=True, with_vision=True,
           max_vision_images=BM)
e.init_synthetic(seed=0)
sysm = System(cfg, e)


def med(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def alternate(forms):
    """forms: name -> callable.  One warm-up each (its output is kept), then reps rounds in turn; -> (outputs, {name: [ms]})"""
    outs = {k: f() for k, f in forms.items()}
    res = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            res[k].append(timed(f)[1])
    return outs, res


lines = ["# Cost of continuing a cached batch in one pass (`tools/extend_cost.py`)", "",
         f"{'tiny' if tiny else 'Janus-Pro-1B-shaped'} synthetic weights, bf16, one process, forms alternated, {reps} repeats, medians (min .. max).", ""]

if "forced" in shapes:
    ids, mask = synth_prompts(B, L, cfg.vocab, cfg.pad_id, seed=0)
    pad = Engine.pad_len_from_mask(mask, L)
    gt = torch.randint(0, cfg.img_vocab, (B, T), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(e.device)
    fm = torch.zeros((B, T), dtype=torch.uint8, device=e.device)

    def loop():
        e.prefill(ids, pad)
        return e.decode_image_tokens(T, 5.0, 1.0, 0, gt, fm)

    def prefixed(t0):
        def run():
            e.prefill(ids, pad, uncond_shared=False)
            e.extend(embeds=e.gen_embed(gt[:, :t0].repeat_interleave(2, 0), dtype=torch.bfloat16).view(2 * B, t0, cfg.hidden))
            dec = e.decode_image_tokens(T - t0, 5.0, 1.0, 0, gt[:, t0:].contiguous(), fm[:, t0:].contiguous())
            return torch.cat([gt[:, :t0], dec.to(torch.int32)], 1)
        return run
    forms = {"loop": loop}
    forms.update({f"t0={t0}": prefixed(t0) for t0 in T0S})
    outs, res = alternate(forms)
    for k, v in outs.items():
        assert torch.equal(v.to(torch.int32), gt), k
    lines += [f"## Forced image tokens: {B} pairs, prompt {L}, {T} tokens (prefill + loop, ms)", "", "| form | median | min .. max | vs loop |", "|---|---|---|---|"]
    base = med(res["loop"])
    for k, v in res.items():
        lines.append(f"| {k} | {med(v):.1f} | {min(v):.1f} .. {max(v):.1f} | {med(v) / base:.3f} |")
    lines.append("")

if "mmu" in shapes:
    g = torch.Generator().manual_seed(2)
    P = cfg.vit_tokens
    px = torch.rand(BM, 1, 3, cfg.vit_img, cfg.vit_img, generator=g) * 2 - 1
    hi = cfg.vocab - 2048 if cfg.vocab > 4096 else cfg.vocab
    qs = []
    for q in range(NQ):
        ids_q = torch.cat([torch.ones(BM, 1, dtype=torch.long), torch.zeros(BM, P, dtype=torch.long), torch.randint(10, hi, (BM, QLEN), generator=g)], 1)
        seq = torch.zeros((BM, LM), dtype=torch.bool)
        seq[:, 1:1 + P] = True
        qs.append(dict(input_ids=ids_q, pixel_values=px, images_seq_mask=seq, images_emb_mask=torch.ones((BM, 1, P), dtype=torch.bool),
                       attention_mask=torch.ones((BM, LM), dtype=torch.int32)))
    NEW = 8 if tiny else 64

    def independent():
        return [sysm.uni_generate(dict(prepare_inputs_infer=q), pred_image=False, is_mmu=True, max_new_tokens=NEW, min_new_tokens=NEW)["pr_text_ids"] for q in qs]

    def ask():
        sysm.mmu_ask(dict(prepare_inputs_infer=qs[0]), qs, max_new_tokens=NEW, min_new_tokens=NEW)
        return sysm.last_ask_ids
    outs, res = alternate({"4 x mmu": independent, "mmu_ask": ask})
    same = sum(float((a == b).float().mean()) for a, b in zip(outs["4 x mmu"], outs["mmu_ask"])) / NQ
    lines += [f"## {NQ} questions about {BM} images: {LM} prompt embeddings, {NEW} greedy tokens each (whole call, SigLIP included, ms)", "",
              "| form | median | min .. max | vs 4 x mmu |", "|---|---|---|---|"]
    base = med(res["4 x mmu"])
    for k, v in res.items():
        lines.append(f"| {k} | {med(v):.1f} | {min(v):.1f} .. {max(v):.1f} | {med(v) / base:.3f} |")
    lines += ["", f"Token agreement of the two forms (bf16, greedy): {same:.3f}.", ""]

text = "\n".join(lines)
print(text)
if out_md != "-":
    with open(out_md, "w") as f:
        f.write(text + "\n")
