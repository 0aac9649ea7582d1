"""Drop-in facade with the attribute / call surface PlanGen's ``System`` uses on
``self.vl_gpt`` (Janus ``MultiModalityCausalLM``, three_party/Janus/janus/models/
modeling_vlm.py:190-271) -- SURVEY.md section 8b.  Every call lands in the C ABI.

    vl_gpt.language_model.get_input_embeddings()(ids)             plangen_base.py:371,548
    vl_gpt.language_model.model(inputs_embeds=, attention_mask=,  plangen_base.py:571-577
                                use_cache=True, past_key_values=)
    vl_gpt.gen_head(h)                                            plangen_base.py:579
    vl_gpt.prepare_gen_img_embeds(tok)                            plangen_base.py:603
    vl_gpt.gen_vision_model.decode_code(codes, shape=, ...)       plangen_base.py:555
    vl_gpt.gen_vision_model.encode(x)                             plangen_base.py:532
    vl_gpt.language_model.generate(inputs_embeds=, ...)           plangen_base.py:513-523
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .engine import Engine, PlanGenError


@dataclass
class PastKeyValues:
    """Opaque token standing for the engine-resident KV cache (the reference passes HF's
    DynamicCache back verbatim; here the cache never leaves HBM)."""
    engine: Engine
    epoch: int
    seen: int            # cached positions (padded layout), like DynamicCache.get_seq_length()

    def get_seq_length(self) -> int:
        return self.seen


@dataclass
class ModelOutput:
    last_hidden_state: torch.Tensor
    past_key_values: PastKeyValues


class _Embedding:
    def __init__(self, eng: Engine):
        self.eng = eng

    def __call__(self, ids: torch.Tensor) -> torch.Tensor:
        return self.eng.embed_tokens(ids)


class _LlamaModel:
    """``language_model.model``: prefill on the first call, one decode step on later calls."""

    def __init__(self, eng: Engine, position_mode: int = 0):
        self.eng = eng
        self.epoch = 0
        self.position_mode = position_mode

    def __call__(self, inputs_embeds: torch.Tensor = None, attention_mask: Optional[torch.Tensor] = None,
                 use_cache: bool = True, past_key_values: Optional[PastKeyValues] = None, input_ids: Optional[torch.Tensor] = None,
                 replicas: int = 1, alias: bool = True, **kw) -> ModelOutput:
        eng = self.eng
        if past_key_values is None and replicas > 1:
            # parallel_size replicas of one CFG batch, every prompt prefilled once (pg_prefill_replicated): takes the UN-replicated ids [R0, L] (the
            # engine embeds them) and the mask of those rows; the cache then holds replicas * R0 rows and later calls take [replicas * R0, 1, H].
            # last_hidden_state is the LAST position only, [replicas * R0, 1, H] -- all the reference's loop reads (hidden_states[:, -1, :]).
            if input_ids is None or attention_mask is None:
                raise PlanGenError("language_model.model(replicas > 1) needs input_ids [R0, L] and their attention_mask")
            R0, L = input_ids.shape
            eng.prefill_replicated(input_ids, Engine.pad_len_from_mask(attention_mask[:R0], L), replicas, alias=alias)
            hid = eng.debug_read("hfin", 0, R0 * replicas * eng.cfg.hidden, eng.tdtype).view(R0 * replicas, 1, eng.cfg.hidden)
            self.epoch += 1
            return ModelOutput(hid, PastKeyValues(eng, self.epoch, L))
        if inputs_embeds is None:
            raise PlanGenError("language_model.model: inputs_embeds is required (the reference never passes input_ids)")
        R, q, _ = inputs_embeds.shape
        out_dtype = inputs_embeds.dtype if inputs_embeds.dtype in (torch.float32, torch.bfloat16) else torch.float32
        if past_key_values is None:
            if attention_mask is None:
                pad = [0] * R
            else:
                # mask is [R, L+576] at every step (App. B-3): only its first q columns describe the prompt
                pad = Engine.pad_len_from_mask(attention_mask, q)
            hid = eng.prefill_embeds(inputs_embeds, pad, position_mode=self.position_mode, return_hidden=True,
                                     hidden_dtype=out_dtype)
            self.epoch += 1
            return ModelOutput(hid, PastKeyValues(eng, self.epoch, q))
        if past_key_values.epoch != self.epoch or past_key_values.engine is not eng:
            raise PlanGenError("stale past_key_values: the engine holds one KV cache per handle")
        if q != 1:
            raise PlanGenError("decode calls take one new position per row")
        hid = eng.step(inputs_embeds[:, 0, :], hidden_dtype=out_dtype)
        past_key_values.seen += 1
        return ModelOutput(hid[:, None, :], past_key_values)


class _LanguageModel:
    def __init__(self, eng: Engine):
        self.eng = eng
        self.model = _LlamaModel(eng, position_mode=0)
        self._emb = _Embedding(eng)

    def get_input_embeddings(self):
        return self._emb

    def generate(self, inputs_embeds: torch.Tensor = None, attention_mask: Optional[torch.Tensor] = None,
                 pad_token_id: Optional[int] = None, bos_token_id: Optional[int] = None,
                 eos_token_id: Optional[int] = None, max_new_tokens: int = 512, do_sample: bool = False,
                 use_cache: bool = True, min_new_tokens: int = 0, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, seed: int = 0, dfa=None, return_logprobs: bool = False, return_stats=False, **kw) -> torch.Tensor:
        """HF GenerationMixin.generate (System.x2t, plangen_base.py:513-523): returns the NEW tokens only, int64
        [B, n<=max_new_tokens], finished rows padded with eos.  do_sample=False (the reference's call) is greedy and
        ignores temperature / top_k / top_p like HF; do_sample=True draws with them (temperature -> top-k -> top-p,
        0 / 1.0 = filter off) from the engine's counter RNG keyed on (``seed``, row, step) -- not torch's generator.
        ``dfa`` (a ``grammar.TokenDFA``): the same decode with every step's logits masked by the automaton (HF's logits-processor slot);
        min_new_tokens does not apply there, the automaton says where EOS may stand.
        ``return_logprobs`` (HF's output_scores + compute_transition_scores): returns (tokens, fp32 [B, n] log-probabilities of the emitted tokens).
        ``return_stats`` (True, or an int n_alt; HF's output_scores reduced on the device): also (last) the dict of
        ``Engine._request_stats`` over [B, n]: entropy, rank and the top-n_alt alternatives of every emitted token."""
        if do_sample and not temperature > 0:
            raise PlanGenError(f"do_sample=True needs temperature > 0 (got {temperature})")
        if do_sample and top_k is None:
            top_k = 0
        if do_sample and top_p is None:
            top_p = 1.0
        if eos_token_id is None:
            raise PlanGenError("eos_token_id is required")
        R, L, _ = inputs_embeds.shape
        pad = [0] * R if attention_mask is None else Engine.pad_len_from_mask(attention_mask, L)
        self.eng.prefill_embeds(inputs_embeds, pad, position_mode=1)
        self.model.epoch += 1          # invalidates any sample_image cache token
        lpkw = {"return_logprobs": True} if return_logprobs else {}       # without it: exactly the calls made before scores existed
        if return_stats is not False and return_stats is not None:
            lpkw["return_stats"] = return_stats
        if dfa is not None:
            if getattr(self.eng, "uploaded_dfa", None) is not dfa:         # the cached automaton of layout_token_dfa: uploaded once
                self.eng.set_text_dfa(dfa)
            return self.eng.generate_text_constrained(max_new_tokens, int(eos_token_id), temperature=float(temperature) if do_sample else 0.0,
                                                      top_k=int(top_k or 0), top_p=float(1.0 if top_p is None else top_p), seed=int(seed), **lpkw)
        if not do_sample:
            if lpkw:
                return self.eng.generate_text(max_new_tokens, int(eos_token_id), min_new_tokens, temperature=0.0, **lpkw)
            return self.eng.generate_text_greedy(max_new_tokens, int(eos_token_id), min_new_tokens)
        return self.eng.generate_text(max_new_tokens, int(eos_token_id), min_new_tokens, temperature=float(temperature),
                                      top_k=int(top_k), top_p=float(top_p), seed=int(seed), **lpkw)


class _GenVisionModel:
    def __init__(self, eng: Engine):
        self.eng = eng

    def decode_code(self, code_b: torch.Tensor, shape=None, channel_first: bool = True) -> torch.Tensor:
        """VQModel.decode_code (vq_model.py:505-508): int [B, g*g] -> [B,3,S,S]."""
        cfg = self.eng.cfg
        if shape is not None and (shape[1] != cfg.img_dim or shape[2] != cfg.grid or shape[3] != cfg.grid):
            raise PlanGenError(f"decode_code: shape {list(shape)} does not match the configured VQ ({cfg.img_dim},{cfg.grid},{cfg.grid})")
        if not channel_first:
            # vq_model.py:297-298: channel_first=False makes get_codebook_entry return z_q.view(shape) with shape = (B, H, W, C) -- an NHWC tensor that
            # the reference's own decode() then feeds to post_quant_conv (a Conv2d over dim 1): with H = W = 24 != 8 channels it raises there.  The only call
            # in the reference passes channel_first=True (plangen_base.py:555); refusing the other form is the reference's error behaviour, stated up front.
            raise PlanGenError("decode_code: only channel_first=True (the reference's call) is supported")
        B = shape[0] if shape is not None else code_b.shape[0]
        return self.eng.vq_decode(code_b.reshape(B, -1))

    def encode(self, x: torch.Tensor):
        """VQModel.encode (vq_model.py:494-498) -> (quant, losses, (None, None, indices));
        only the indices are produced (all the reference reads: ``encode(x)[-1][-1]``)."""
        idx = self.eng.vq_encode(x)
        return None, (None, None, None), (None, None, idx)


class MultiModalityCausalLM:
    """What ``self.vl_gpt`` is in PlanGen's System, backed by one MI355X engine."""

    def __init__(self, engine: Engine):
        self.engine = engine
        self.language_model = _LanguageModel(engine)
        self.gen_vision_model = _GenVisionModel(engine)
        self.training = False

    def gen_head(self, h: torch.Tensor) -> torch.Tensor:
        return self.engine.gen_head(h)

    def prepare_gen_img_embeds(self, image_ids: torch.Tensor) -> torch.Tensor:
        return self.engine.gen_embed(image_ids)

    def prepare_inputs_embeds(self, input_ids: torch.Tensor, pixel_values: torch.Tensor,
                              images_seq_mask: torch.Tensor, images_emb_mask: torch.Tensor, **kwargs) -> torch.Tensor:
        """MultiModalityCausalLM.prepare_inputs_embeds (modeling_vlm.py:221-268): SigLIP + aligner on
        the device, then the masked scatter of the image embeddings into the text embeddings."""
        bs, n = pixel_values.shape[0:2]
        images = pixel_values.reshape(bs * n, *pixel_values.shape[2:])
        images_embeds = self.engine.vision_encode(images)                   # [b*n, T2, D]
        images_embeds = images_embeds.reshape(bs, n * images_embeds.shape[1], -1)
        images_emb_mask = images_emb_mask.reshape(bs, -1).to(self.engine.device).bool()
        ids = input_ids.to(self.engine.device).clone()
        ids[ids < 0] = 0
        inputs_embeds = self.language_model.get_input_embeddings()(ids)
        inputs_embeds[images_seq_mask.to(self.engine.device).bool()] = images_embeds[images_emb_mask].to(inputs_embeds.dtype)
        return inputs_embeds

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise PlanGenError("training is out of scope of the MI355X generation path (SURVEY 3.4)")
        return self

    def parameters(self):
        # device / dtype discovery only (plangen_base.py:1183-1189)
        yield torch.empty(0, dtype=self.engine.tdtype, device=self.engine.device)
