"""Host model of the LoRA merge (pg_merge_lora, plangen_amd/csrc/lora_merge.hip) for tests/test_lora_ref_cpu.py, tests/test_gpu_lora_ops.py and
tests/test_gpu_lora_path.py.  Plain torch on the CPU; nothing imports the package.

The merge's arithmetic is a contract (include/plangen_hip.h), every operation rounded to fp32 on its own, k ascending:

    acc = 0;  acc = acc (+) B[o][k] (*) A[k][i]  for k = 0 .. r - 1;   m = (float)W[o][i] (+) scale (*) acc;   W[o][i] = T(m)

``merge_ref`` is that loop with one elementwise fp32 multiply and one elementwise fp32 add per k in torch: on an IEEE host each is correctly rounded and torch
fuses nothing between two tensor operations, so the model is EXACT and the comparator is ``load_ref.same_bits``.  The bf16 engine's last step is
``load_ref.f32_to_bf16_bits`` (round to nearest even on the bit pattern).

The planted defects are what a wrong kernel would compute; tests/test_lora_ref_cpu.py shows that ``same_bits`` tells each from the model."""
from __future__ import annotations

import torch

import load_ref as R

F64 = torch.float64
F32 = torch.float32
TARGETS_QKVO = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj")
TARGETS_QV = ("self_attn.q_proj", "self_attn.v_proj")
TARGETS_ALL = TARGETS_QKVO + ("mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(x):
    return torch.tensor(float(x), dtype=F32)


def _store(m, engine_kind):
    return R.from_bits(R.f32_to_bf16_bits(m), "bf16").reshape(m.shape) if engine_kind == "bf16" else m


# ------------------------------------------------------------------------------------------------------------------------------ the model
def delta_acc(A, B):
    """acc [out, in] fp32: the k loop of the contract."""
    A, B = A.float(), B.float()
    acc = torch.zeros(B.shape[0], A.shape[1], dtype=F32)
    for k in range(A.shape[0]):
        acc = acc + B[:, k:k + 1] * A[k:k + 1, :]
    return acc


def merged_f32(W, A, B, scale):
    """m [out, in] fp32, before the store."""
    return W.float() + _f32(scale) * delta_acc(A, B)


def merge_ref(W, A, B, scale, engine_kind):
    """What the slot holds after the merge: W [out, in] as the engine holds it (bf16 / fp32 values), A [r, in], B [out, r] fp32 or bf16."""
    assert W.dtype == R.tdtype(engine_kind) and A.shape[0] == B.shape[1] and W.shape == (B.shape[0], A.shape[1])
    return _store(merged_f32(W, A, B, scale), engine_kind)


def merge_il16_ref(buf, A, B, scale, which, engine_kind):
    """The [2 I, in] interleaved gate|up buffer after a merge into its gate (which = 0) or up (1) rows; the other half keeps its bytes."""
    rows = R.il16_rows(B.shape[0], which)
    out = buf.clone()
    out[rows] = merge_ref(buf[rows], A, B, scale, engine_kind)
    return out


def merge_f64(W, A, B, scale):
    """(m, magnitude) in fp64 on the fp32 values of the inputs (scale as the fp32 the call receives): m = W + scale B A, magnitude = |W| + |scale| |B| |A|."""
    s = _f32(scale).to(F64)
    m = W.to(F64) + s * (B.to(F64) @ A.to(F64))
    return m, W.to(F64).abs() + s.abs() * (B.to(F64).abs() @ A.to(F64).abs())


def model_bound(mag, r):
    """r products, r sums (the first onto 0 is exact), the scale and the final sum: at most r + 2 roundings of relative size 2^-24 on terms whose
    magnitudes sum to ``mag``."""
    return (r + 2) * R.U_F32 * mag


# ------------------------------------------------------------------------------------------------------------------------------ planted defects
def defect_transposed(W, A, B, scale, engine_kind):
    """(B A)^T added: needs out == in."""
    return _store(W.float() + _f32(scale) * delta_acc(A, B).t(), engine_kind)


def defect_scale_per_term(W, A, B, scale, engine_kind):
    A, B, s = A.float(), B.float(), _f32(scale)
    acc = torch.zeros(B.shape[0], A.shape[1], dtype=F32)
    for k in range(A.shape[0]):
        acc = acc + s * (B[:, k:k + 1] * A[k:k + 1, :])
    return _store(W.float() + acc, engine_kind)


def defect_fma(W, A, B, scale, engine_kind):
    """acc = fma(b, a, acc): the product is exact in fp64 (48 bits), so one rounding of the fp64 sum to fp32 is the fused operation up to double rounding."""
    A, B = A.to(F64), B.to(F64)
    acc = torch.zeros(B.shape[0], A.shape[1], dtype=F32)
    for k in range(A.shape[0]):
        acc = (acc.to(F64) + B[:, k:k + 1] * A[k:k + 1, :]).float()
    return _store(W.float() + _f32(scale) * acc, engine_kind)


def defect_wrong_half(buf, A, B, scale, which, engine_kind):
    return merge_il16_ref(buf, A, B, scale, 1 - which, engine_kind)


def defect_dropped_last_k(W, A, B, scale, engine_kind):
    return _store(merged_f32(W, A[:-1], B[:, :-1], scale), engine_kind)


def defect_no_final_add(W, A, B, scale, engine_kind):
    """T(scale acc) stored over W."""
    return _store(_f32(scale) * delta_acc(A, B), engine_kind)


# ------------------------------------------------------------------------------------------------------------------------------ adapters
def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def make_adapters(W, targets, r, alpha, seed, ratio=0.5, n_layers=None, dtype=F32):
    """base weight name -> (A [r, in], B [out, r]) for ``targets`` (module names inside a layer) of every layer of the state dict W.  A and B are normal with
    one std per weight, chosen so that RMS(scale B A) = scale sqrt(r) std^2 is about ``ratio`` x RMS(W) (scale = alpha / r)."""
    g = _gen(seed)
    out = {}
    layers = sorted({int(k.split(".")[3]) for k in W if k.startswith("language_model.model.layers.")})
    for i in layers[:n_layers]:
        for t in targets:
            name = f"language_model.model.layers.{i}.{t}.weight"
            o, n = W[name].shape
            std = (ratio * rms(W[name]) / (alpha / r * r ** 0.5)) ** 0.5
            out[name] = ((torch.randn(r, n, generator=g) * std).to(dtype), (torch.randn(o, r, generator=g) * std).to(dtype))
    return out


def delta_ratio(W, name, A, B, scale):
    """RMS(scale B A) / RMS(W[name]) in fp64."""
    return rms(float(scale) * (B.double() @ A.double())) / rms(W[name])


def merged_state_dict(W, adapters, alpha, engine_kind, times=1):
    """W (values the engine holds exactly: bf16-representable for a bf16 engine) with every adapter merged by the model, ``times`` times; tensors of
    ``engine_kind``'s type for the merged names, the others as they are."""
    out = dict(W)
    for name, (A, B) in adapters.items():
        w = W[name].to(R.tdtype(engine_kind))
        for _ in range(times):
            w = merge_ref(w, A, B, alpha / A.shape[0], engine_kind)
        out[name] = w
    return out


def peft_state_dict(adapters, plain=None, adapter="default", prefix="vl_gpt.base_model.model.", base_layer=()):
    """The keys a peft-wrapped model saves: <prefix><module>.lora_A.<adapter>.weight / lora_B (adapter = None: the older form without the name), full tensors
    of ``plain`` under <prefix><name> -- those listed in ``base_layer`` as <module>.base_layer.weight."""
    mid = "" if adapter is None else "." + adapter
    sd = {}
    for name, t in (plain or {}).items():
        sd[prefix + (name[:-len("weight")] + "base_layer.weight" if name in base_layer else name)] = t
    for name, (A, B) in adapters.items():
        mod = name[:-len(".weight")]
        sd[f"{prefix}{mod}.lora_A{mid}.weight"] = A
        sd[f"{prefix}{mod}.lora_B{mid}.weight"] = B
    return sd
