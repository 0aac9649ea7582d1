"""CPU: the top-k / top-p sampler's public surface -- the CLI keys reach System.args with off-by-default values, the header declares
both new entry points, and the fp64 references agree with each other on rows without ties at a threshold."""
import os
import re

import torch

from conftest import ROOT


def _args(*opts):
    import train
    return train.parse_args(["--cfg", os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py"), "--opt", "test=True",
                             "tiny=True", "test_batch_size=1", "dtype='f32'", *opts])


def _system_args(monkeypatch, a):
    """project.plangen.plangen_base.System.__init__ up to the engine: what it hands to the hot path as ``args``."""
    import project.plangen.plangen_base as pb
    seen = {}

    def fake_hot_init(self, cfg, eng, args=None, codec=None):
        seen["args"] = args

    monkeypatch.setattr(pb, "Engine", lambda cfg, **kw: None)
    monkeypatch.setattr(pb._HotPath, "__init__", fake_hot_init)
    pb.System(a, None)
    return seen["args"]


def test_cli_keys_reach_system_args(monkeypatch):
    a = _args()
    assert a.top_k == 0 and a.top_p == 1.0
    s = _system_args(monkeypatch, a)
    assert s.top_k == 0 and s.top_p == 1.0
    a = _args("top_k=7", "top_p=0.5")
    assert a.top_k == 7 and a.top_p == 0.5
    s = _system_args(monkeypatch, a)
    assert s.top_k == 7 and s.top_p == 0.5


def test_config_defaults_are_off():
    from plangen_amd.config import PlanGenConfig
    c = PlanGenConfig.janus_pro_1b()
    assert c.top_k == 0 and c.top_p == 1.0


def test_header_declares_the_filtered_sampler():
    h = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    assert re.search(r"int pg_decode_image_tokens_filtered\(pg_handle h, int T, float cfg_weight, float temperature, int32_t top_k, "
                     r"float top_p,\s+uint64_t seed,", h)
    assert re.search(r"int pg_op_sample_filter\(pg_handle h, const float\* logits_dev /\*\[B,V\]\*/, int B, int V, float temperature, "
                     r"int top_k,\s+float top_p, uint8_t\* keep_dev /\*\[B,V\]\*/, pg_stream s\);", h)
    from plangen_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"pg_decode_image_tokens_filtered", "pg_op_sample_filter"} <= names


def test_rule_reference_matches_the_transformers_warpers():
    from sampling_filter_ref import ambiguous, hf_keep, rule_keep
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(32, 512, generator=g) * 2.5
    for temp, k, p in ((1.0, 0, 0.9), (0.7, 40, 1.0), (1.3, 100, 0.6), (1.0, 1, 1.0), (1.0, 0, 1e-6), (1.0, 512, 1.0)):
        amb = ambiguous(rows, temp, k, p)
        assert amb.sum() <= 0.01 * rows.numel()
        assert torch.equal(rule_keep(rows, temp, k, p)[~amb], hf_keep(rows, temp, k, p)[~amb]), (temp, k, p)
