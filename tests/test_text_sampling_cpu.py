"""CPU: the sampled text decode's public surface -- the facade hands do_sample / temperature / top_k / top_p / seed to
Engine.generate_text, System.x2t reads the text_* keys, the CLI keys are off by default, the header / map / bindings declare both new
entry points, the fp64 references agree at the real vocabulary within the ambiguity cap the GPU test uses, and the new kernels compile
for gfx950 without scratch."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT


class _StubEngine:
    """Records what the facade asks of the engine (no GPU)."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def prefill_embeds(self, emb, pad, position_mode=0, **kw):
        self.calls.append(("prefill_embeds", position_mode))

    def generate_text_greedy(self, max_new, eos, min_new=0):
        self.calls.append(("greedy", max_new, eos, min_new))
        return torch.zeros((2, 1), dtype=torch.int64)

    def generate_text(self, max_new, eos, min_new=0, **kw):
        self.calls.append(("sampled", max_new, eos, min_new, kw))
        return torch.zeros((2, 1), dtype=torch.int64)


def test_facade_generate_plumbs_the_sampling_arguments():
    from plangen_amd.engine import PlanGenError
    from plangen_amd.janus import _LanguageModel
    eng = _StubEngine()
    lm = _LanguageModel(eng)
    emb = torch.zeros(2, 3, 4)
    lm.generate(inputs_embeds=emb, eos_token_id=7, max_new_tokens=5, do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=11,
                min_new_tokens=2)
    assert eng.calls[-2] == ("prefill_embeds", 1)
    assert eng.calls[-1] == ("sampled", 5, 7, 2, dict(temperature=0.7, top_k=50, top_p=0.9, seed=11))
    lm.generate(inputs_embeds=emb, eos_token_id=7, max_new_tokens=5, do_sample=True)                 # HF defaults: T 1, filters off
    assert eng.calls[-1] == ("sampled", 5, 7, 0, dict(temperature=1.0, top_k=0, top_p=1.0, seed=0))
    # do_sample=False ignores the sampling arguments, like HF
    lm.generate(inputs_embeds=emb, eos_token_id=7, max_new_tokens=5, do_sample=False, temperature=0.7, top_k=50, top_p=0.9)
    assert eng.calls[-1] == ("greedy", 5, 7, 0)
    with pytest.raises(PlanGenError):
        lm.generate(inputs_embeds=emb, eos_token_id=7, do_sample=True, temperature=0.0)


def test_x2t_reads_the_text_keys_from_args():
    from plangen_amd.config import PlanGenConfig
    from plangen_amd.system import System
    cfg = PlanGenConfig.tiny()
    eng = _StubEngine()
    emb = torch.zeros(2, 3, 4)
    s = System(cfg, eng)                                                 # default args: greedy
    s.x2t(emb, None, max_new_tokens=4)
    assert eng.calls[-1] == ("greedy", 4, cfg.eos_id, 0)
    s = System(cfg, eng, SimpleNamespace(seed=5, text_temperature=0.8, text_top_k=40, text_top_p=0.95, debug_max_seq_len=None))
    s.x2t(emb, None, max_new_tokens=4, min_new_tokens=1)
    assert eng.calls[-1] == ("sampled", 4, cfg.eos_id, 1, dict(temperature=0.8, top_k=40, top_p=0.95, seed=5))
    s.x2t(emb, None, max_new_tokens=4, temperature=0.0)                  # per-call override back to greedy
    assert eng.calls[-1] == ("greedy", 4, cfg.eos_id, 0)


def test_cfg_defaults_are_off_and_cli_keys_reach_system_args(monkeypatch):
    import project.plangen.plangen_base as pb
    import train
    from plangen_amd.config import PlanGenConfig
    c = PlanGenConfig.janus_pro_1b()
    assert c.text_temperature == 0.0 and c.text_top_k == 0 and c.text_top_p == 1.0
    seen = {}
    monkeypatch.setattr(pb, "Engine", lambda cfg, **kw: None)
    monkeypatch.setattr(pb._HotPath, "__init__", lambda self, cfg, eng, args=None, codec=None: seen.update(args=args))

    def args(*opts):
        return train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", "test=True",
                                 "tiny=True", "test_batch_size=1", "dtype='f32'", *opts])
    a = args()
    assert a.text_temperature == 0.0 and a.text_top_k == 0 and a.text_top_p == 1.0
    pb.System(a, None)
    assert (seen["args"].text_temperature, seen["args"].text_top_k, seen["args"].text_top_p) == (0.0, 0, 1.0)
    pb.System(args("text_temperature=1.0", "text_top_k=50", "text_top_p=0.9"), None)
    assert (seen["args"].text_temperature, seen["args"].text_top_k, seen["args"].text_top_p) == (1.0, 50, 0.9)


def test_header_map_and_bindings_declare_the_text_sampler():
    h = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    assert re.search(r"int pg_generate_text_sampled\(pg_handle h, int max_new, int min_new, int eos_id, float temperature, int32_t top_k,\s+"
                     r"float top_p, uint64_t seed, int64_t\* out_dev, int\* out_len_host,\s+float\* logits_out_dev, pg_stream s\);", h)
    assert re.search(r"int pg_op_text_sample\(pg_handle h, const float\* logits_dev /\*\[B,V\]\*/, int B, int V, float temperature, int top_k,\s+"
                     r"float top_p, uint64_t seed, int row_offset, int step, uint8_t\* keep_dev /\*\[B,V\]\*/,\s+int32_t\* tok_dev /\*\[B\]\*/, "
                     r"pg_stream s\);", h)
    assert "int pg_generate_text_greedy(pg_handle h, int max_new, int min_new, int eos_id, int64_t* out_dev,\n" in h      # unchanged
    m = open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    from plangen_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    for sym in ("pg_generate_text_sampled", "pg_op_text_sample"):
        assert sym in names and f"{sym};" in m


@pytest.mark.parametrize("seed", [102400 + 1000, 7, 8])
def test_references_agree_at_the_real_vocabulary_within_the_ambiguity_cap(seed):
    """Gaussian rows at the measured logit std: the rule and the transformers warpers agree outside ambiguous(...), whose share stays
    under the cap the GPU test asserts (seed 103 400 is the GPU test's V = 102 400 generator)."""
    from sampling_filter_ref import ambiguous, hf_keep, rule_keep
    rows = torch.randn(3, 102400, generator=torch.Generator().manual_seed(seed)) * 2.4
    for temp, k, p in ((1.0, 0, 0.9), (0.7, 1000, 0.95), (1.0, 50, 1.0), (1.0, 50, 0.9)):
        amb = ambiguous(rows, temp, k, p)
        assert amb.float().mean(-1).max().item() <= 1e-3, (temp, k, p)
        assert torch.equal(rule_keep(rows, temp, k, p)[~amb], hf_keep(rows, temp, k, p)[~amb]), (temp, k, p)


HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.mark.skipif(not HIPCC, reason="hipcc not available")
def test_text_sampler_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """The code object's metadata (.private_segment_fixed_size) of every text_scan_kernel instantiation and of text_select_kernel."""
    src = os.path.join(ROOT, "plangen_amd", "csrc", "sampler.hip")
    asm = str(tmp_path / "sampler.s")
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-mllvm",
                        "-amdgpu-kernarg-preload-count=16", src, "-o", asm], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    text = open(asm).read()
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text):
        found[m.group(1)] = int(m.group(2))
    sel = {k: v for k, v in found.items() if "text_select_kernel" in k}
    scan = {k: v for k, v in found.items() if "text_scan_kernel" in k}
    assert len(sel) == 1 and len(scan) == 6, (sel, scan)                  # greedy / sampled / store, each with and without the logits tap
    assert all(v == 0 for v in {**sel, **scan}.values()), {**sel, **scan}
