#!/usr/bin/env python3
"""What the grammar constraint costs the text decode step, on one build and against the parent build's library.

* whole step, 32 rows x vocab 102 400 (the generate_fullvocab model: Janus width, 2 layers, bf16, synthetic weights): the greedy loop
  (min_new = max_new, every step runs), the same loop timed a second time ("greedy_b": the run-to-run spread every difference is read
  against), the constrained loop under an automaton that allows every token (EOS only where the budget forces it, so every step runs too),
  greedy and sampled; ``--parent-lib`` adds the greedy loop of another build of libplangen_hip.so on a second handle in the same rotation,
  twice per repetition ("greedy_parent", "greedy_parent_b"): the parent-vs-parent spread that "greedy_vs_parent_us" is read against.
* the scan + pick pair alone: pg_op_text_constrain over fp32 rows [B, 102 400] at 32 and 128 rows, device events around 20 calls.  The
  unconstrained pair has no operator entry (pg_op_text_sample is the select kernel), so its cost is read from the step difference above.

The only prior is arithmetic: the mask adds one 2-byte class per 4 * S bytes of logits (S split-K slabs) to the scan's reads.
One JSON line per measurement, a summary last.  usage: text_dfa_cost.py [--reps 7] [--tokens 64] [--parent-lib /path/to/libplangen_hip.so]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from text_sampler_cost import parent_engine  # noqa: E402

V = 102400


def free_dfa(vocab, eos):
    cls = np.zeros(vocab, np.int16)
    cls[eos] = 1
    return SimpleNamespace(token_class=cls, next_state=np.array([[0, 1], [-1, -1]], np.int16), dist=np.array([1, 0], np.int32), start_state=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    from fullwidth_cfg import FULLV
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    cfg = PlanGenConfig(**FULLV)
    B, L, nt = 32, 64, a.tokens
    eos = cfg.eos_id
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(10, cfg.vocab - 2048, (B, L), generator=g).int()
    kw = dict(dtype="bf16", max_rows=128, max_prompt=L, max_new=nt, max_images=1, with_lm_head=True)
    engines = {"new": Engine(cfg, **kw)}
    if a.parent_lib:
        engines["parent"] = parent_engine(a.parent_lib, cfg, **kw)
    for e in engines.values():
        e.init_synthetic(seed=0)
    new = engines["new"]
    new.set_text_dfa(free_dfa(cfg.vocab, eos))
    MODES = {"greedy": None, "greedy_b": None, "dfa_greedy": dict(temperature=0.0), "t1": dict(temperature=1.0), "dfa_t1": dict(temperature=1.0),
             "k50_p0.9": dict(temperature=1.0, top_k=50, top_p=0.9), "dfa_k50_p0.9": dict(temperature=1.0, top_k=50, top_p=0.9)}
    modes = list(MODES) + (["greedy_parent", "greedy_parent_b"] if a.parent_lib else [])

    def run(mode, seed):
        e = engines["parent" if mode.startswith("greedy_parent") else "new"]
        e.prefill(ids, [0] * B, position_mode=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if MODES.get(mode) is None:
            out = e.generate_text_greedy(nt, eos, min_new_tokens=nt)
        elif mode.startswith("dfa_"):
            out = e.generate_text_constrained(nt, eos, seed=seed, **MODES[mode])
        else:
            out = e.generate_text(nt, eos, min_new_tokens=nt, seed=seed, **MODES[mode])
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    outs = {m: run(m, 1)[0] for m in modes}                            # warm-up: first-call allocations, code objects
    assert torch.equal(outs["greedy"], outs["greedy_b"])
    if a.parent_lib:
        assert torch.equal(outs["greedy"], outs["greedy_parent"]), "greedy ids differ from the parent build's"
    steps = {m: int(outs[m].shape[1]) for m in modes}
    res = {m: [] for m in modes}
    for r in range(a.reps):
        for m in modes[r % len(modes):] + modes[:r % len(modes)]:
            _, ms = run(m, 100 + r)
            res[m].append(ms)
            print(json.dumps({"rep": r, "mode": m, "text_decode_ms": round(ms, 3)}), flush=True)
    med = {m: sorted(v)[len(v) // 2] / steps[m] * 1e3 for m, v in res.items()}                 # us per step
    summ = {"rows": B, "vocab": cfg.vocab, "tokens": nt, "steps_run": steps, "reps": a.reps,
            "step_us_median": {m: round(v, 2) for m, v in med.items()},
            "step_us_min_max": {m: [round(min(v) / steps[m] * 1e3, 2), round(max(v) / steps[m] * 1e3, 2)] for m, v in res.items()},
            "greedy_vs_greedy_us": round(med["greedy_b"] - med["greedy"], 2),
            "dfa_added_us": {m: round(med["dfa_" + m] - med[m], 2) for m in ("greedy", "t1", "k50_p0.9")}}
    if a.parent_lib:
        summ["greedy_vs_parent_us"] = round(med["greedy"] - med["greedy_parent"], 2)
        summ["parent_vs_parent_us"] = round(med["greedy_parent_b"] - med["greedy_parent"], 2)
        both = sorted(res["greedy_parent"] + res["greedy_parent_b"])
        summ["parent_runs_min_max_us"] = [round(both[0] / steps["greedy_parent"] * 1e3, 2), round(both[-1] / steps["greedy_parent"] * 1e3, 2)]
    print(json.dumps(summ), flush=True)
    # ---- the pair alone
    for rows in (32, 128):
        x = (torch.randn(rows, V, generator=g) * 2.4).to(new.device)
        st = torch.zeros(rows, dtype=torch.int32, device=new.device)
        for name, okw in (("greedy", {}), ("t1", dict(temperature=1.0)), ("k50_p0.9", dict(temperature=1.0, top_k=50, top_p=0.9))):
            new.text_constrain(x, st, 50, eos, **okw)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            n = 20
            ev[0].record()
            for i in range(n):
                new.text_constrain(x, st, 50, eos, step=i, **okw)
            ev[1].record()
            torch.cuda.synchronize()
            us = ev[0].elapsed_time(ev[1]) / n * 1e3
            print(json.dumps({"pair": name, "rows": rows, "us_per_call": round(us, 2), "logit_mb": round(rows * V * 4 / 1e6, 1),
                              "class_mb": round(rows * V * 2 / 1e6, 1), "note": "includes the keep-mask store [B, V] u8 and one parameter kernel"}), flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
