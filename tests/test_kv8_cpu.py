"""CPU: the FP8 KV cache's format contract (tests/kv8_ref.py), its place in the ABI / Python / cfg surface, and the reference rule."""
import os
import re

import pytest
import torch

import kv8_ref
from conftest import ROOT, load_golden
from oracle import ref_cpu as R


def test_quantize_roundtrip_bounds():
    x = kv8_ref.row_families().float()
    codes, scale = kv8_ref.quantize(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scale.shape == x.shape[:1]
    m, _ = torch.frexp(scale)
    assert torch.all(m == 0.5), "every scale is a power of two"
    amax = x.abs().amax(-1)
    scaled = x / scale[:, None]
    assert scaled.abs().max() <= 448.0
    nz = amax > 0
    assert torch.all(amax[nz] / scale[nz] > 224.0), "e is the SMALLEST exponent"
    assert scale[~nz].eq(1.0).all()
    y = kv8_ref.dequantize(codes, scale)
    err = (y - x).abs()
    big = x.abs() >= amax[:, None] * 2.0 ** -6
    assert torch.all(err[big] <= x.abs()[big] * 2.0 ** -4)                   # e4m3's half ulp on normal values
    assert torch.all(err <= torch.maximum(x.abs() * 2.0 ** -4, amax[:, None].expand_as(x) * 2.0 ** -10))   # half the subnormal spacing below
    # idempotent, bit for bit, in the VALUES: a row whose amax rounds down onto 224 * 2^e re-quantises one exponent lower, with every code
    # doubled -- the same numbers
    assert torch.equal(kv8_ref.qdq(y).view(torch.int32), y.view(torch.int32))
    c2, s2 = kv8_ref.quantize(y)
    same = s2 == scale
    assert torch.equal(c2[same], codes[same]) and torch.all(s2[~same] * 2 == scale[~same])
    # the checked conversions of the contract
    t = torch.tensor([0.0175, 17.0, 19.0, 2.0 ** -10]).to(torch.float8_e4m3fn).float()
    assert t.tolist() == [0.017578125, 16.0, 20.0, 0.0]


def test_exponent_edges():
    a = torch.tensor([448.0, 449.0, 224.0, 1.0, 0.0, 448.0 * 2.0 ** -7, 2.0 ** 120, 2.0 ** -120])
    assert kv8_ref.exponent(a).tolist() == [0, 1, -1, -8, 0, -7, 100, -100]


def test_abi_and_python_surface():
    from plangen_amd import _lib
    from plangen_amd.config import PlanGenConfig
    assert _lib.pg_config._fields_[-1][0] == "kv_dtype"
    assert _lib.PG_FP8_E4M3 == 4
    assert any(n == "pg_op_kv_quantize" for n, _, _ in _lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    assert re.search(r"PG_FP8_E4M3\s*=\s*4", hdr) and "pg_op_kv_quantize(" in hdr
    assert re.search(r"int32_t\s+kv_dtype;", hdr)
    body = hdr[hdr.index("typedef struct pg_config"):hdr.index("} pg_config;")]
    assert body.rstrip().endswith("*/") and "kv_dtype" in body.split("max_vision_images")[-1], "kv_dtype is the trailing field"
    assert "pg_op_kv_quantize" in open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    assert PlanGenConfig().kv_dtype == "bf16" and PlanGenConfig(kv_dtype="fp8").kv_dtype == "fp8"
    api = open(os.path.join(ROOT, "plangen_amd", "csrc", "engine_api.hip")).read()
    opts = api[api.index("int pg_set_option("):api.index("int64_t pg_device_bytes(")]
    assert "kv_dtype" not in opts and "fp8" not in opts.lower(), "the mode changes results: it belongs in the config, not in pg_set_option"


def test_cfg_key_and_cli_override():
    ns = {}
    exec(open(os.path.join(ROOT, "project", "plangen", "cfg", "base.py")).read(), ns)
    assert ns["kv_dtype"] == "bf16"
    import inspect
    from plangen_amd.engine import Engine
    assert inspect.signature(Engine.__init__).parameters["kv_dtype"].default == "bf16"
    src = open(os.path.join(ROOT, "project", "plangen", "plangen_base.py")).read()
    assert "kv_dtype" in src


def test_forward_kv8_with_identity_quantiser_is_the_oracle(ocfg, tiny_weights):
    g = load_golden("sample_image_tiny.npz")
    ids, mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"])
    emb = R.embed_tokens(tiny_weights, ids)
    pos = torch.arange(ids.shape[1])[None].expand(ids.shape[0], -1)
    a, ca = R.llama_forward(tiny_weights, ocfg, emb, mask, pos)
    b, cb = kv8_ref.llama_forward_kv8(tiny_weights, ocfg, emb, mask, pos, quant=lambda t: t)
    assert torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(ca.k + ca.v, cb.k + cb.v))
    t0 = R.sample_image(tiny_weights, ocfg, emb, mask, 5.0, n_tokens=4, return_logits=True)
    t1 = kv8_ref.sample_image_kv8(tiny_weights, ocfg, emb, mask, 5.0, n_tokens=4, return_logits=True, quant=lambda t: t)
    assert torch.equal(t0[0], t1[0]) and torch.equal(t0[1], t1[1])
    t2 = kv8_ref.sample_image_kv8(tiny_weights, ocfg, emb, mask, 5.0, n_tokens=4, return_logits=True)
    assert torch.equal(t2[1][0], t0[1][0]), "the first step attends to exact prefill K / V"
    assert not torch.equal(t2[1][1:], t0[1][1:]), "later steps read the quantised cache"
