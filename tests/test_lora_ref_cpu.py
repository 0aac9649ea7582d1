"""CPU: the host model of the LoRA merge (tests/lora_ref.py) against fp64 and against its planted defects, the key handling of
weights.split_peft_state_dict, load_checkpoint's order of calls with a stub engine, and pg_merge_lora in the header, the export map and the binding."""
import os
import re

import pytest
import torch

import load_ref as R
import lora_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEFECT_SEED = 13                                            # a seed at which every planted defect moves at least one bf16 bit of a 256 x 256 merge (asserted below)


def _case(out, n, r, seed, kind, ab_dtype=F32):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(out, n, generator=g) * 0.05).to(R.tdtype(kind))
    A = (torch.randn(r, n, generator=g) * 0.3).to(ab_dtype)
    B = (torch.randn(out, r, generator=g) * 0.3).to(ab_dtype)
    return W, A, B


# ------------------------------------------------------------------------------------------------------------------------------ the model against fp64
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("out,n,r,scale", [(64, 48, 16, 0.5), (40, 72, 40, -2.0), (8, 136, 256, 0.5), (16, 16, 1, 8.0), (24, 8, 3, 1.0 / 3)])
def test_model_against_fp64(kind, out, n, r, scale):
    """Before the store the model is within (r + 2) 2^-24 (|W| + |scale| sum_k |B_ok A_ki|) of fp64; after the bf16 rounding within one bf16 ulp."""
    W, A, B = _case(out, n, r, 100 + r, kind)
    m64, mag = L.merge_f64(W, A, B, scale)
    m32 = L.merged_f32(W, A, B, scale)
    err = (m32.to(F64) - m64).abs()
    bound = L.model_bound(mag, r)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) > 0 or r == 1                                       # the comparison is not against itself
    got = L.merge_ref(W, A, B, scale, kind)
    assert got.dtype == R.tdtype(kind)
    if kind == "f32":
        assert torch.equal(R.bits(got), R.bits(m32))
        return
    # one bf16 ulp at m64: the spacing 2^(e - 7) of its binade (bf16 has 8 significand bits); below the smallest normal the spacing is 2^-133
    e = torch.floor(torch.log2(m64.abs().clamp_min(2.0 ** -126)))
    ulp = torch.exp2(e - 7)
    assert bool(((got.to(F64) - m64).abs() <= ulp).all())
    assert torch.equal(R.bits(got), R.bits(m32.to(BF)))                          # torch's own conversion is the second model of the rounding


def test_model_is_order_sensitive_where_the_contract_says_so():
    """k ascending is part of the contract: the reversed order gives other fp32 bits on the same inputs."""
    W, A, B = _case(32, 32, 40, 7, "f32")
    fwd = L.merge_ref(W, A, B, 0.5, "f32")
    rev = L.merge_ref(W, A.flip(0), B.flip(1), 0.5, "f32")
    assert not R.same_bits(rev, fwd)["ok"]
    assert bool(((rev.double() - fwd.double()).abs() <= 2 * L.model_bound(L.merge_f64(W, A, B, 0.5)[1], 40)).all())


def test_bf16_adapters_are_exact_in_fp32():
    W, A, B = _case(16, 24, 8, 3, "bf16", ab_dtype=BF)
    assert R.same_bits(L.merge_ref(W, A, B, 2.0, "bf16"), L.merge_ref(W, A.float(), B.float(), 2.0, "bf16"))["ok"]


def test_zero_scale_and_stacking():
    W, A, B = _case(16, 24, 8, 4, "bf16")
    assert R.same_bits(L.merge_ref(W, A, B, 0.0, "bf16"), W)["ok"]
    once = L.merge_ref(W, A, B, 0.25, "bf16")
    twice = L.merge_ref(once, A, B, 0.25, "bf16")
    assert not R.same_bits(twice, once)["ok"] and not R.same_bits(twice, L.merge_ref(W, A, B, 0.5, "bf16"))["ok"]   # two roundings are not one


# ------------------------------------------------------------------------------------------------------------------------------ defects
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_every_planted_defect_changes_bits(kind):
    """Each defect differs from the model in at least one stored bit on these seeds -- bf16 bits for the bf16 engine -- so same_bits catches it."""
    scale = 1.0 / 3
    W, A, B = _case(256, 256, 40, DEFECT_SEED, kind)
    want = L.merge_ref(W, A, B, scale, kind)
    assert R.same_bits(L.merge_ref(W.clone(), A.clone(), B.clone(), scale, kind), want)["ok"]
    for name, fn in (("transposed", L.defect_transposed), ("scale per term", L.defect_scale_per_term), ("fma", L.defect_fma),
                     ("dropped last k", L.defect_dropped_last_k), ("no final add", L.defect_no_final_add)):
        res = R.same_bits(fn(W, A, B, scale, kind), want)
        assert not res["ok"] and res["n_bad"] > 0, (name, kind)
    I = 24
    g = torch.Generator().manual_seed(5)
    buf = (torch.randn(2 * I, 48, generator=g) * 0.05).to(R.tdtype(kind))
    _, A2, B2 = _case(I, 48, 16, 12, kind)
    for which in (0, 1):
        good = L.merge_il16_ref(buf, A2, B2, scale, which, kind)
        other = R.il16_rows(I, 1 - which)
        assert torch.equal(R.bits(good[other]), R.bits(buf[other]))                # the other half keeps its bytes
        assert not R.same_bits(good, buf)["ok"]
        assert not R.same_bits(L.defect_wrong_half(buf, A2, B2, scale, which, kind), good)["ok"], which


def test_fma_defect_is_the_small_one():
    """The FMA defect is the hardest to see: it stays inside the model's own fp64 bound and moves a handful of the 65536 bf16 values (7 at this seed; seeds 11
    and 12 move one), which is why the defect cases use a 256 x 256 matrix."""
    W, A, B = _case(256, 256, 40, DEFECT_SEED, "bf16")
    fma = L.defect_fma(W, A, B, 1.0 / 3, "bf16")
    want = L.merge_ref(W, A, B, 1.0 / 3, "bf16")
    n_bad = R.same_bits(fma, want)["n_bad"]
    assert 0 < n_bad < 64, n_bad
    m64, mag = L.merge_f64(W, A, B, 1.0 / 3)
    acc = L.defect_fma(W.float(), A, B, 1.0 / 3, "f32")
    assert bool(((acc.double() - m64).abs() <= L.model_bound(mag, 40)).all())


# ------------------------------------------------------------------------------------------------------------------------------ keys
def _pairs(seed=0, r=4):
    g = torch.Generator().manual_seed(seed)
    q = "language_model.model.layers.0.self_attn.q_proj.weight"
    v = "language_model.model.layers.1.self_attn.v_proj.weight"
    return {q: (torch.randn(r, 8, generator=g), torch.randn(6, r, generator=g)), v: (torch.randn(r, 8, generator=g), torch.randn(6, r, generator=g))}


@pytest.mark.parametrize("prefix", ["vl_gpt.base_model.model.", "base_model.model.", "vl_gpt.", ""])
@pytest.mark.parametrize("adapter", ["default", "plangen", None])
def test_split_accepts_every_key_form(prefix, adapter):
    from plangen_amd.weights import split_peft_state_dict
    ad = _pairs()
    emb = "language_model.model.embed_tokens.weight"
    o = "language_model.model.layers.0.self_attn.o_proj.weight"
    full = {emb: torch.randn(5, 8), o: torch.randn(8, 6)}
    sd = L.peft_state_dict(ad, plain=full, adapter=adapter, prefix=prefix, base_layer=(o,))
    assert any(".base_layer.weight" in k for k in sd) and all(k.startswith(prefix) for k in sd)
    plain, adapters = split_peft_state_dict(sd)
    assert set(plain) == {emb, o} and all(plain[k] is full[k] for k in full)
    assert set(adapters) == set(ad)
    for k, (A, B) in ad.items():
        assert adapters[k][0] is A and adapters[k][1] is B


def test_split_passes_a_plain_overlay_through():
    from plangen_amd.weights import split_peft_state_dict
    sd = {"vl_gpt.gen_head.vision_head.bias": torch.zeros(3), "gen_embed.weight": torch.ones(2, 2)}
    plain, adapters = split_peft_state_dict(sd)
    assert adapters == {} and set(plain) == {"gen_head.vision_head.bias", "gen_embed.weight"}


def test_split_refusals_name_the_key():
    from plangen_amd.engine import PlanGenError
    from plangen_amd.weights import split_peft_state_dict
    P = "vl_gpt.base_model.model."
    base = L.peft_state_dict(_pairs(), prefix=P)
    q = P + "language_model.model.layers.0.self_attn.q_proj"

    def refused(sd, key, word=None):
        with pytest.raises(PlanGenError) as ei:
            split_peft_state_dict(sd)
        assert key in str(ei.value) and (word is None or word in str(ei.value)), str(ei.value)

    sd = dict(base); del sd[q + ".lora_B.default.weight"]
    refused(sd, q + ".lora_A.default.weight", "without its lora_B")
    sd = dict(base); del sd[q + ".lora_A.default.weight"]
    refused(sd, q + ".lora_B.default.weight", "without its lora_A")
    sd = dict(base)
    k2 = P + "language_model.model.layers.1.self_attn.q_proj"
    sd[k2 + ".lora_A.other.weight"], sd[k2 + ".lora_B.other.weight"] = torch.zeros(4, 8), torch.zeros(6, 4)
    refused(sd, k2 + ".lora_A.other.weight", "adapter")
    sd = dict(base); sd[q + ".lora_B.default.weight"] = torch.zeros(6, 5)           # A has rank 4
    refused(sd, q + ".lora_B.default.weight", "rank")
    sd = dict(base)
    sd[k2 + ".lora_A.default.weight"], sd[k2 + ".lora_B.default.weight"] = torch.zeros(2, 8), torch.zeros(6, 2)   # another rank than the other modules
    refused(sd, k2 + ".lora_A.default.weight", "rank")
    e = P + "language_model.model.embed_tokens"
    for key in (e + ".lora_embedding_A.default", e + ".lora_embedding_B.default", q + ".lora_magnitude_vector.default.weight", q + ".lora_B.default.bias"):
        sd = dict(base); sd[key] = torch.zeros(4, 4)
        refused(sd, key)


# ------------------------------------------------------------------------------------------------------------------------------ loader
class _StubEngine:
    """Records the calls load_checkpoint makes; owns the names of a Llama layer's projections, embed_tokens and one bias."""

    def __init__(self):
        self.calls = []

    def _owns(self, name):
        name = name[len("vl_gpt."):] if name.startswith("vl_gpt.") else name
        return name.startswith("language_model.model.") and ".lora_" not in name and "base_model" not in name or name == "gen_head.vision_head.bias"

    def load_tensors(self, sd):
        own = [k for k in sd if self._owns(k)]
        self.calls.append(("load_tensors", sorted(own)))
        return len(own), [k for k in sd if not self._owns(k)]

    def load_lora(self, adapters, alpha):
        self.calls.append(("load_lora", sorted(adapters), float(alpha), {A.shape[0] for A, _ in adapters.values()}))
        return len(adapters)

    def finalize(self, strict=True):
        self.calls.append(("finalize", strict))
        return 0


@pytest.fixture()
def lora_checkpoint(tmp_path):
    from safetensors.torch import save_file
    ad = _pairs()
    emb = "language_model.model.embed_tokens.weight"
    base = {k: torch.randn(6, 8) for k in ad}
    base[emb] = torch.randn(5, 8)
    save_file(base, str(tmp_path / "model.safetensors"))
    ck = tmp_path / "checkpoint-3"
    ck.mkdir()
    torch.save(L.peft_state_dict(ad, plain={emb: torch.randn(5, 8)}), str(ck / "trainable_model_parameters.pth"))
    return str(tmp_path), str(ck), ad, emb


def test_load_checkpoint_order_base_plain_adapters_finalize(lora_checkpoint):
    from plangen_amd.weights import load_checkpoint
    base_dir, ck, ad, emb = lora_checkpoint
    e = _StubEngine()
    info = load_checkpoint(e, base_dir, overlay=ck, lora_alpha=8.0, lora_rank=4)
    kinds = [c[0] for c in e.calls]
    assert kinds == ["load_tensors", "load_tensors", "load_lora", "finalize"], kinds
    assert e.calls[0][1] == sorted(list(ad) + [emb])                              # the base directory
    assert e.calls[1][1] == [emb]                                                 # the overlay's full tensor, under its base name
    assert e.calls[2][1:] == (sorted(ad), 8.0, {4})
    assert info["loaded"] == [str(len(ad) + 1 + 1 + len(ad))] and info["skipped"] == []


def test_load_checkpoint_without_alpha_refuses_as_before(lora_checkpoint):
    from plangen_amd.engine import PlanGenError
    from plangen_amd.weights import load_checkpoint
    base_dir, ck, ad, emb = lora_checkpoint
    e = _StubEngine()
    with pytest.raises(PlanGenError, match="refusing to run the base weights silently"):
        load_checkpoint(e, base_dir, overlay=ck)
    assert [c[0] for c in e.calls] == ["load_tensors", "load_tensors"]            # nothing merged, nothing finalized
    e = _StubEngine()
    with pytest.raises(PlanGenError, match="refusing to run the base weights silently"):
        load_checkpoint(e, base_dir, overlay=ck, lora_rank=4)                     # a rank alone does not make up for the missing alpha


def test_load_checkpoint_checks_the_rank_and_the_adapters(lora_checkpoint, tmp_path):
    from plangen_amd.engine import PlanGenError
    from plangen_amd.weights import load_checkpoint
    base_dir, ck, ad, emb = lora_checkpoint
    e = _StubEngine()
    with pytest.raises(PlanGenError, match="lora_rank=64"):
        load_checkpoint(e, base_dir, overlay=ck, lora_alpha=16.0, lora_rank=64)
    assert "load_lora" not in [c[0] for c in e.calls] and "finalize" not in [c[0] for c in e.calls]
    plain = tmp_path / "plain.pth"
    torch.save({"vl_gpt.gen_head.vision_head.bias": torch.zeros(3)}, str(plain))
    with pytest.raises(PlanGenError, match="no lora_A / lora_B"):
        load_checkpoint(_StubEngine(), base_dir, overlay=str(plain), lora_alpha=16.0)
    e = _StubEngine()
    load_checkpoint(e, base_dir, overlay=str(plain))                              # and a plain overlay loads as it always did
    assert [c[0] for c in e.calls] == ["load_tensors", "load_tensors", "finalize"]


def test_config_and_cli_carry_alpha_and_rank():
    import train
    from plangen_amd.config import PlanGenConfig
    c = PlanGenConfig()
    assert c.lora_alpha is None and c.lora_rank is None
    assert "lora_alpha" not in c.model_dict() and "lora_rank" not in c.model_dict()
    cfg = os.path.join(ROOT, "project/plangen/cfg/uni/h_text_ump+oimsam.py")
    a = train.parse_args(["--cfg", cfg, "--opt", "test=True", "resume=None"])
    assert a.lora_alpha is None and a.lora_rank is None
    a = train.parse_args(["--cfg", cfg, "--opt", "test=True", "resume=None", "lora_alpha=128", "lora_rank=256"])
    assert a.lora_alpha == 128 and a.lora_rank == 256
    src = open(os.path.join(ROOT, "project", "plangen", "plangen_base.py")).read()
    assert "lora_alpha=self.cfg.lora_alpha" in src and "lora_rank=self.cfg.lora_rank" in src


# ------------------------------------------------------------------------------------------------------------------------------ ABI
def test_pg_merge_lora_is_declared_exported_and_bound():
    from plangen_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "plangen_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+pg_merge_lora\s*\(([^)]*)\)\s*;", code)
    assert m, "pg_merge_lora is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0].startswith("pg_handle") and args[1].startswith("const char*") and args[-1] == "float scale"
    comment = hdr[:hdr.index("int pg_merge_lora(")].rsplit("/*", 1)[1]
    for word in ("ONE rounding", "fp32 source", "Non-finite", "un-merge", "pg_finalize_weights", "PG_ERR_NAME", "PG_ERR_STATE", "PG_ERR_ARG", "1024"):
        assert word in comment, word
    vmap = open(os.path.join(ROOT, "plangen_amd", "csrc", "plangen_hip.map")).read()
    assert re.search(r"\bpg_merge_lora;", vmap)
    sym = {n: (res, a) for n, res, a in _lib.SYMBOLS}
    assert "pg_merge_lora" in sym and len(sym["pg_merge_lora"][1]) == 10
    api = open(os.path.join(ROOT, "plangen_amd", "csrc", "engine_api.hip")).read()
    body = api[api.index("int pg_set_option("):api.index("int64_t pg_device_bytes(")]
    assert "lora" not in body                                                     # no option key came with it
