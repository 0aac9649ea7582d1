#!/usr/bin/env python3
"""What sampling costs the text decode loop at the two shapes of bench.py's ``secondary`` block (full-size synthetic weights, bf16):
uni_2stage (32 rows, prompt 128, 256 forced-length tokens) and mmu (64 rows, prompt 640, 256 tokens); min_new = max_new so every step runs.
Four modes of one build -- greedy, T=1 unfiltered, top_k=50, top_k=50 + top_p=0.9 -- are timed interleaved in one process (host clock around
the call, device synchronised), the order rotated every repetition.  ``--parent-lib`` adds the greedy loop of another build of
libplangen_hip.so (the parent commit's) on a second handle in the same rotation; "greedy_b" is the same build's greedy loop timed a second
time per repetition: the greedy-vs-greedy spread every difference is read against.  One JSON line per measurement, a summary per shape last.
usage: text_sampler_cost.py [--reps 5] [--shapes uni_2stage,mmu] [--parent-lib /path/to/libplangen_hip.so]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NT = 256
SHAPES = {"uni_2stage": (32, 128), "mmu": (64, 640)}                   # rows, prompt length
MODES = {"greedy": dict(temperature=0.0), "greedy_b": dict(temperature=0.0), "t1": dict(temperature=1.0),
         "k50": dict(temperature=1.0, top_k=50), "k50_p0.9": dict(temperature=1.0, top_k=50, top_p=0.9)}
CU_LOAD_GBS = 64 * 2.4          # one CU's vector-memory return path: 64 B / clk at 2.4 GHz (MI355X_MICROARCH)
HBM_GBS = 8000.0


def parent_engine(path, *a, **kw):
    """An Engine whose handle lives in another build of the library (symbols that build lacks stay unbound)."""
    from plangen_amd import _lib
    from plangen_amd.engine import Engine
    lib = C.CDLL(path)
    for name, res, args in _lib.SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
    saved, _lib._lib = _lib._lib, lib
    try:
        return Engine(*a, **kw)
    finally:
        _lib._lib = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="uni_2stage,mmu")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--tokens", type=int, default=NT)
    a = ap.parse_args()
    import torch
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.engine import Engine
    cfg = PlanGenConfig.janus_pro_1b()
    nt = a.tokens
    for shape in a.shapes.split(","):
        B, L = SHAPES[shape]
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(10, cfg.vocab - 2048, (B, L), generator=g).int()
        kw = dict(dtype="bf16", max_rows=B, max_prompt=L, max_new=nt, max_images=1, with_lm_head=True)
        engines = {"new": Engine(cfg, **kw)}
        if a.parent_lib:
            engines["parent"] = parent_engine(a.parent_lib, cfg, **kw)
        for e in engines.values():
            e.init_synthetic(seed=0)

        def run(mode, seed):
            e = engines["parent" if mode == "greedy_parent" else "new"]
            e.prefill(ids, [0] * B, position_mode=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "greedy_parent":
                out = e.generate_text_greedy(nt, cfg.eos_id, min_new_tokens=nt)
            else:
                out = e.generate_text(nt, cfg.eos_id, min_new_tokens=nt, seed=seed, **MODES[mode])
            torch.cuda.synchronize()
            assert out.shape == (B, nt)
            return out, (time.perf_counter() - t0) * 1e3

        modes = list(MODES) + (["greedy_parent"] if a.parent_lib else [])
        outs = {m: run(m, 1)[0] for m in modes}                        # warm-up: first-call allocations, code objects
        assert torch.equal(outs["greedy"], outs["greedy_b"])
        if a.parent_lib:
            assert torch.equal(outs["greedy"], outs["greedy_parent"]), "greedy ids differ from the parent build's"
        res = {m: [] for m in modes}
        for r in range(a.reps):
            order = modes[r % len(modes):] + modes[:r % len(modes)]
            for m in order:
                _, ms = run(m, 100 + r)
                res[m].append(ms)
                print(json.dumps({"shape": shape, "rep": r, "mode": m, "text_decode_ms": round(ms, 3)}), flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
        row_mb = B * cfg.vocab * 4 / 1e6
        # floor of the filtered path: the [B, V] fp32 workspace written and read once more at HBM rate (it is L2 / Infinity-Cache
        # resident, so this is generous) + the three row passes of one block per row (histogram, compaction, draw) at one CU's load rate
        floor_us = 2 * row_mb / HBM_GBS * 1e3 + 3 * cfg.vocab * 4 / CU_LOAD_GBS * 1e-3
        summ = {"shape": shape, "rows": B, "prompt": L, "tokens": nt, "reps": a.reps,
                "median_ms": {m: round(v, 3) for m, v in med.items()},
                "min_max_ms": {m: [round(min(v), 3), round(max(v), 3)] for m, v in res.items()},
                "greedy_step_us": round(med["greedy"] * 1e3 / nt, 2),
                "greedy_vs_greedy_us_per_step": round((med["greedy_b"] - med["greedy"]) * 1e3 / nt, 2),
                "added_us_per_step_over_greedy": {m: round((med[m] - med["greedy"]) * 1e3 / nt, 2) for m in modes if m != "greedy"},
                "added_share_of_greedy_step": {m: round((med[m] - med["greedy"]) / med["greedy"], 4) for m in modes if m != "greedy"},
                "filtered_floor_us_per_step": round(floor_us, 2), "workspace_mb": round(row_mb, 1)}
        print(json.dumps(summ), flush=True)
        for e in engines.values():
            e.close()


if __name__ == "__main__":
    main()
