"""Checkpoint formats of the path (SURVEY.md 8f-4, section 5 'Checkpoint / resume').

* base weights: HF ``deepseek-ai/Janus-Pro-1B`` directory (``*.safetensors`` shards, optionally a
  ``model.safetensors.index.json``) -- what ``AutoModelForCausalLM.from_pretrained(janus_path)`` reads
  (plangen_base.py:95);
* PlanGen overlay: ``checkpoint-*/trainable_model_parameters.pth`` written by ``Base_System.save_para``
  (base_system.py:166-189), a plain ``torch.save`` dict whose keys carry the ``vl_gpt.`` prefix; loaded
  by the reference with ``load_state_dict(strict=False)`` (base_system.py:153-155).  With ``tuning_mode`` ``lora`` / ``lora_ranni``
  (plangen_base.py:162-185) the model is peft-wrapped and the file holds ``lora_A`` / ``lora_B`` tensors under peft's key names:
  ``split_peft_state_dict`` maps them and ``load_checkpoint(lora_alpha=)`` merges them into the weights (``pg_merge_lora``).

Both are streamed tensor by tensor into ``pg_load_tensor`` (the engine converts to its own layouts);
names the engine does not own (e.g. ``vision_model.*`` when the understanding encoder is disabled) are
reported as skipped, like ``strict=False`` does.
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from .engine import Engine, PlanGenError


def iter_safetensors(model_dir: str) -> Iterator[Tuple[str, torch.Tensor]]:
    from safetensors import safe_open
    index = os.path.join(model_dir, "model.safetensors.index.json")
    if os.path.exists(index):
        files = sorted(set(json.load(open(index))["weight_map"].values()))
    else:
        files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(model_dir, "*.safetensors")))
    if not files:
        raise PlanGenError(f"no .safetensors files in {model_dir}")
    for fn in files:
        with safe_open(os.path.join(model_dir, fn), framework="pt", device="cpu") as f:
            for k in f.keys():
                yield k, f.get_tensor(k)


def latest_checkpoint(out_dir: str) -> Optional[str]:
    """``resume='latest'``: newest ``checkpoint-{step}`` directory (base_system.py:137-144)."""
    cands = [d for d in glob.glob(os.path.join(out_dir, "checkpoint-*")) if os.path.isdir(d)]
    if not cands:
        return None
    return max(cands, key=lambda d: int(d.rsplit("-", 1)[-1]))


_PEFT_PREFIX = "base_model.model."
_PEFT_REFUSED = ("lora_embedding_A", "lora_embedding_B", "lora_magnitude_vector", "lora_bias")


def split_peft_state_dict(sd: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, Tuple[torch.Tensor, torch.Tensor]]]:
    """Split a state dict saved from a peft-wrapped model (``tuning_mode`` ``lora`` / ``lora_ranni``, plangen_base.py:162-185: ``save_para`` stores
    ``named_parameters()`` of the system, so a key reads ``vl_gpt.base_model.model.<module>.lora_A.default.weight``) into

    * ``plain``: full tensors under their base state_dict names -- ``<module>.base_layer.weight`` becomes ``<module>.weight``, tensors of modules peft did
      not wrap (``language_model.model.embed_tokens.weight`` with ``tune_token_when_lora``) keep their names;
    * ``adapters``: base weight name ``<module>.weight`` -> ``(lora_A [r, in], lora_B [out, r])``.

    An optional ``vl_gpt.`` and then an optional ``base_model.model.`` prefix are removed.  Adapter keys are ``<module>.lora_A.<adapter>.weight`` /
    ``<module>.lora_B.<adapter>.weight`` or the older ``<module>.lora_A.weight`` / ``<module>.lora_B.weight``.  A dict without peft keys comes back as
    ``(its tensors under base names, {})``.  Raises ``PlanGenError`` naming the key for: an A without its B or a B without its A, more than one adapter
    name, ranks that do not match (A against B, or one module against another), and what a merge of ``W + scale B A`` does not cover:
    ``lora_embedding_*``, ``lora_magnitude_vector`` (DoRA), a LoRA bias."""
    plain: Dict[str, torch.Tensor] = {}
    halves: Dict[str, Dict[str, Tuple[str, torch.Tensor]]] = {}
    adapter_names: Dict[str, str] = {}
    for key, t in sd.items():
        name = key[len("vl_gpt."):] if key.startswith("vl_gpt.") else key
        if name.startswith(_PEFT_PREFIX):
            name = name[len(_PEFT_PREFIX):]
        parts = name.split(".")
        bad = [p for p in parts if p in _PEFT_REFUSED]
        if bad:
            raise PlanGenError(f"peft key {key!r}: {bad[0]} is not supported (only lora_A / lora_B of linear layers are merged)")
        which = [i for i, p in enumerate(parts) if p in ("lora_A", "lora_B")]
        if not which:
            plain[name.replace(".base_layer.", ".")] = t
            continue
        i = which[0]
        tail = parts[i + 1:]
        if len(which) != 1 or i == 0 or tail[-1:] == ["bias"] or tail[-1:] != ["weight"] or len(tail) > 2:
            raise PlanGenError(f"peft key {key!r}: expected <module>.{parts[i]}[.<adapter>].weight"
                               + (" (a LoRA bias is not supported)" if tail[-1:] == ["bias"] else ""))
        adapter_names.setdefault(tail[0] if len(tail) == 2 else "", key)
        if len(adapter_names) > 1:
            raise PlanGenError(f"peft key {key!r}: a second adapter name beside {next(iter(adapter_names.values()))!r}; one adapter can be merged")
        base = ".".join(parts[:i]) + ".weight"
        if parts[i] in halves.setdefault(base, {}):
            raise PlanGenError(f"peft key {key!r}: {parts[i]} of {base} twice")
        if t.dim() != 2:
            raise PlanGenError(f"peft key {key!r}: a {t.dim()}-D tensor, expected 2-D")
        halves[base][parts[i]] = (key, t)
    adapters: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
    rank = None
    for base, h in halves.items():
        if len(h) != 2:
            (have, (key, _)), = h.items()
            raise PlanGenError(f"peft key {key!r}: {have} without its {'lora_B' if have == 'lora_A' else 'lora_A'}")
        (ka, A), (kb, B) = h["lora_A"], h["lora_B"]
        if A.shape[0] != B.shape[1]:
            raise PlanGenError(f"peft key {kb!r}: rank {B.shape[1]} of lora_B against rank {A.shape[0]} of lora_A")
        if rank is not None and A.shape[0] != rank[0]:
            raise PlanGenError(f"peft key {ka!r}: rank {A.shape[0]}, but {rank[1]!r} has rank {rank[0]} (one lora_alpha / r scale per checkpoint)")
        rank = rank or (A.shape[0], ka)
        adapters[base] = (A, B)
    return plain, adapters


def load_checkpoint(engine: Engine, janus_path: str, overlay: Optional[str] = None, strict: bool = True,
                    lora_alpha: Optional[float] = None, lora_rank: Optional[int] = None) -> Dict[str, List[str]]:
    """Load base weights then the PlanGen overlay (later tensors replace earlier ones); the engine's derived
    tables and decode layouts are built ONCE at the end (``Engine.finalize``).

    A LoRA overlay (``tuning_mode`` ``lora`` / ``lora_ranni``: lora_A / lora_B tensors, plus ``embed_tokens`` with ``tune_token_when_lora``) needs
    ``lora_alpha``: the file does not hold it, and without it the call refuses as it does for any overlay of which nothing would take effect.  With it
    the order is base tensors, the overlay's full tensors, the adapters (``Engine.load_lora``, scale = lora_alpha / r), finalize.  ``lora_rank``, when
    given, must be the rank found in the file."""
    skipped: List[str] = []
    loaded = 0
    sd = {}
    for name, t in iter_safetensors(janus_path):
        sd[name] = t
        if len(sd) >= 64:                         # bounded host memory: hand over in groups, finalize once
            n, sk = engine.load_tensors(sd)
            loaded += n; skipped += sk; sd = {}
    n, sk = engine.load_tensors(sd)
    loaded += n; skipped += sk
    if overlay:
        path = overlay if overlay.endswith(".pth") else os.path.join(overlay, "trainable_model_parameters.pth")
        if not os.path.exists(path):
            raise FileNotFoundError(f"PlanGen overlay not found: {path}")
        ov = torch.load(path, map_location="cpu", weights_only=True)
        if lora_alpha is None:
            n, sk = engine.load_tensors(ov)       # "vl_gpt." prefix is stripped by pg_load_tensor
            if ov and n == 0:
                # e.g. a LoRA-only checkpoint (lora_A / lora_B keys) and no lora_alpha: nothing of it would take effect
                raise PlanGenError(f"overlay {path}: none of its {len(ov)} tensors is a weight of this engine "
                                   f"(first key {next(iter(ov))!r}); refusing to run the base weights silently")
        else:
            plain, adapters = split_peft_state_dict(ov)
            if not adapters:
                raise PlanGenError(f"overlay {path}: lora_alpha={lora_alpha} given, but the file holds no lora_A / lora_B tensors")
            r = next(iter(adapters.values()))[0].shape[0]
            if lora_rank is not None and int(lora_rank) != r:
                raise PlanGenError(f"overlay {path}: lora_rank={lora_rank} given, the file's adapters have rank {r}")
            n, sk = engine.load_tensors(plain)
            n += engine.load_lora(adapters, lora_alpha)
        loaded += n; skipped += sk
    engine.finalize(strict)
    return {"loaded": [str(loaded)], "skipped": skipped}
