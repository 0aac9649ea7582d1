"""Host-side mirror of the inference methods of PlanGen's ``System``
(project/plangen/plangen_base.py): same names, argument meaning and tensor contracts for
``pad_input_ids`` (:699-725), ``t2i_infer_collate_batch`` (:636-697), ``t2i`` (:525-565),
``sample_image`` (:567-607) and ``x2t`` (:513-523), running on the MI355X engine.

Prompts enter as token-id lists -- what ``wrap_uni_prompt`` returns (:232-261); with a tokenizer plugged in
(``System(codec=...)``, plangen_amd/textproc.py) the text steps either side of the path run too: the chat template,
``decode_plan_text_batch`` / ``decode_mmu_text_batch`` (:296-325), the stage-1 -> stage-2 re-prompt (:380-390) and
``trans_gr_to_creati`` (:460-473).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

import torch

from .config import PlanGenConfig
from .engine import Engine, PlanGenError
from .janus import MultiModalityCausalLM


def pad_input_ids(all_inputs_ids: Sequence[Sequence[int]], pad_id: int, max_length: Optional[int] = None,
                  debug_max_seq_len: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """System.pad_input_ids, test-mode branch: LEFT-pad to the longest (or forced) length."""
    bs = len(all_inputs_ids)
    if debug_max_seq_len is not None:
        max_length = debug_max_seq_len
    if max_length is None:
        max_length = max(map(len, all_inputs_ids))
    ids = torch.full((bs, max_length), pad_id, dtype=torch.int32)
    mask = torch.zeros((bs, max_length), dtype=torch.int32)
    for i, t in enumerate(all_inputs_ids):
        n = len(t)
        if n > max_length:
            raise PlanGenError(f"prompt {i} has {n} tokens > max_length {max_length}")
        if n:
            ids[i, max_length - n:] = torch.as_tensor(list(t), dtype=torch.int32)
            mask[i, max_length - n:] = 1
    return ids, mask


def t2i_infer_collate_batch(cond_ids: Sequence[Sequence[int]], neg_ids, pad_id: int, img_tokens: int,
                            debug_max_seq_len: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """System.t2i_infer_collate_batch: CFG pairs.  ``neg_ids`` is one shared negative prompt
    (``use_neg_box=False``, :672-686) or one per sample (``use_neg_box=True``, :652-670).
    Returns cfg_inputs_ids int32 [2B, L] (row 2k cond, 2k+1 uncond, :690-691) and
    cfg_attention_mask int32 [2B, L+img_tokens] (image part all ones, :778)."""
    bs = len(cond_ids)
    per_sample = len(neg_ids) > 0 and isinstance(neg_ids[0], (list, tuple, torch.Tensor))
    negs = [list(n) for n in neg_ids] if per_sample else [list(neg_ids)] * bs
    if len(negs) != bs:
        raise PlanGenError("one negative prompt per sample expected")
    L = max(max(map(len, cond_ids)), max(map(len, negs)))
    if debug_max_seq_len is not None:
        L = debug_max_seq_len
    c_ids, c_mask = pad_input_ids(cond_ids, pad_id, L)
    n_ids, n_mask = pad_input_ids(negs, pad_id, L)
    ones = torch.ones((bs, img_tokens), dtype=torch.int32)
    ids = torch.stack([c_ids, n_ids], dim=1).view(bs * 2, -1)
    mask = torch.stack([torch.cat([c_mask, ones], -1), torch.cat([n_mask, ones], -1)], dim=1).view(bs * 2, -1)
    return ids.int(), mask.int()


def t2i_dual_collate_batch(cond_ids: Sequence[Sequence[int]], caption_ids: Sequence[Sequence[int]], neg_ids, pad_id: int, img_tokens: int,
                           debug_max_seq_len: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The batch of the dual-guidance loop: triples.  Row 3k = the full prompt (caption + layout), 3k + 1 = the caption-only prompt,
    3k + 2 = the negative prompt (one shared, or one per sample, as in ``t2i_infer_collate_batch``); every row left-padded to the longest.
    Returns ids int32 [3B, L] and mask int32 [3B, L + img_tokens] (image part all ones)."""
    bs = len(cond_ids)
    if len(caption_ids) != bs:
        raise PlanGenError(f"one caption-only prompt per sample expected (got {len(caption_ids)} for {bs})")
    per_sample = len(neg_ids) > 0 and isinstance(neg_ids[0], (list, tuple, torch.Tensor))
    negs = [list(n) for n in neg_ids] if per_sample else [list(neg_ids)] * bs
    if len(negs) != bs:
        raise PlanGenError("one negative prompt per sample expected")
    caps = [list(c) for c in caption_ids]
    L = max(max(map(len, cond_ids)), max(map(len, caps)), max(map(len, negs)))
    if debug_max_seq_len is not None:
        L = debug_max_seq_len
    parts = [pad_input_ids(rows, pad_id, L) for rows in (cond_ids, caps, negs)]
    ones = torch.ones((bs, img_tokens), dtype=torch.int32)
    ids = torch.stack([i for i, _ in parts], dim=1).view(bs * 3, -1)
    mask = torch.stack([torch.cat([m, ones], -1) for _, m in parts], dim=1).view(bs * 3, -1)
    return ids.int(), mask.int()


def _stats_on(v) -> bool:
    """The ``token_stats`` key / ``return_stats`` argument: False (or None) is off, True is n_alt = 0, an int is n_alt."""
    return v is not None and v is not False


def check_codec_capacity(codec, vocab: int) -> None:
    """A tokenizer that knows its length (HFCodec: the files' vocabulary + the added tokens) must fit the embedding table: an id at or
    past ``vocab`` has no row there.  Refused where the tokenizer meets the model, before any id is embedded."""
    n = len(codec) if hasattr(codec, "__len__") else None
    if n is not None and n > int(vocab):
        raise PlanGenError(f"the tokenizer holds {n} tokens ({getattr(codec, 'n_added', 0)} of them added by use_special_tokens / "
                           f"use_numhw_tokens) but the model's embedding table has vocab={int(vocab)} rows: ids {int(vocab)}..{n - 1} cannot be embedded")


def denorm_pt(pt: torch.Tensor) -> torch.Tensor:
    """src/utils/funcs.py:511."""
    return (pt.clamp(-1, 1) + 1) / 2


class System:
    """Inference half of PlanGen's System on one MI355X.

    args carries the cfg keys the path reads (cfg/base.py): seed, parallel_size, cfg_weight,
    temperature, use_teacher_forcing, debug_max_seq_len, janus_hw; optionally share_replicas (parallel_size > 1: prefill every prompt once,
    off when absent), top_k / top_p (image sampling filters, off when absent)
    and text_temperature / text_top_k / text_top_p (sampled layout / caption decode, greedy when absent); select_best (parallel_size > 1:
    keep each prompt's most probable replica, off when absent) and layout_best_of (stage 1: draw N layouts per row and keep the most
    probable, 1 when absent); score_gt_layout (plan / uni_2stage / mmu: also score batch['gt_grounding'], see score_layouts; off when absent);
    score_gt_image (uni / uni_2stage: also score batch['image'], see score_images; off when absent); the sample-plan keys cfg_schedule /
    cfg_weight_end / cfg_weights / same_noise / cfg_weight_in_box / temperatures / top_ks / top_ps (see build_sample_plan; off when absent).
    cfg_weight_layout (uni / uni_2stage; absent or None: off): dual guidance -- three rows per image, cfg_weight weighs the caption and this key the
    layout (see t2i_dual).
    """

    def __init__(self, cfg: PlanGenConfig, engine: Engine, args: Optional[SimpleNamespace] = None, codec=None):
        check_codec_capacity(codec, cfg.vocab)
        self.cfg = cfg
        self.engine = engine
        self.codec = codec                # tokenizer (plangen_amd.textproc.HFCodec / TagWordCodec); None: ids only
        self.last_generated_tokens = None
        self.last_token_stats = None      # args.token_stats: the stats dict [B, T] of the last t2i (+ "summary": image_token_stats_summary)
        self.last_sample_plan = None      # the sample-plan cfg keys: the record of the last t2i's plan (build_sample_plan), None when no key is set
        self.last_forced_prefix = None    # prefill_forced_prefix: t0 of the last t2i (0: nothing could be prefilled), None when the key is off
        self.last_selection = None        # select_best: dict(replica int64 [B0], score fp32 [B0], scores fp32 [p, B0]) of the last t2i
        self.last_dual_guidance = None    # cfg_weight_layout: dict(w_caption, w_layout) of the last t2i_dual, None when the key is off
        self.last_logprobs = None         # t2i_dual(return_logprobs=True): fp32 [B * p, T] of the last t2i_dual, None without it
        self.vl_gpt = MultiModalityCausalLM(engine)
        self.args = args or SimpleNamespace(seed=cfg.seed, parallel_size=1, cfg_weight=cfg.cfg_weight,
                                            temperature=cfg.temperature, top_k=cfg.top_k, top_p=cfg.top_p, use_teacher_forcing=False,
                                            debug_max_seq_len=None, janus_hw=cfg.img_size, neg_prompt="", use_neg_box=False)
        self.image_token_num_per_image = cfg.img_tokens
        self.device = engine.device

    # -------------------------------------------------------------- collate
    def pad_input_ids(self, all_inputs_ids, max_length=None):
        return pad_input_ids(all_inputs_ids, self.cfg.pad_id, max_length, self.args.debug_max_seq_len)

    def t2i_infer_collate_batch(self, cond_ids, neg_ids):
        return t2i_infer_collate_batch(cond_ids, neg_ids, self.cfg.pad_id, self.image_token_num_per_image,
                                       self.args.debug_max_seq_len)

    # -------------------------------------------------------------- hot path
    @torch.no_grad()
    def sample_image(self, tokens: torch.Tensor, mask: torch.Tensor, cfg_weight: float, temperature: float,
                     seed: int = 0, edit_region: Optional[torch.Tensor] = None,
                     gt_labels: Optional[torch.Tensor] = None, force_tokens: Optional[torch.Tensor] = None,
                     n_tokens: Optional[int] = None, return_logits: bool = False, top_k: Optional[int] = None,
                     top_p: Optional[float] = None, replicas: int = 1, alias: bool = True, return_logprobs: bool = False,
                     return_stats=False, plan=None):
        """The 576-step CFG loop, fused on device (one pg_prefill + one pg_decode_image_tokens).
        tokens int32 [2B, L] CFG-interleaved ids, mask [2B, L+T].  temperature<=0 -> greedy.
        top_k / top_p (default: self.args, else off) filter the sampled draws.
        replicas > 1: ``tokens`` is the UN-replicated batch [2B0, L] and the loop runs on replicas * 2B0 rows (row t * 2B0 + r = replica t of
        row r) with every prompt prefilled once (Engine.prefill_replicated); mask / edit_region / gt_labels / force_tokens are the replicated ones.
        return_logprobs: the emitted tokens' log-probabilities fp32 [B, T] are appended to what is returned.
        return_stats (True, or an int n_alt): the ``Engine._request_stats`` dict over [B, T] is appended (last).
        plan (``guidance.SamplePlan`` over the B images of the loop): per-image sampler parameters, per-step guidance weights."""
        top_k = getattr(self.args, "top_k", 0) if top_k is None else top_k
        top_p = getattr(self.args, "top_p", 1.0) if top_p is None else top_p
        L = tokens.shape[1]
        if replicas > 1:
            pad = Engine.pad_len_from_mask(mask[:tokens.shape[0]], L)
            self.engine.prefill_replicated(tokens, pad, replicas, alias=alias)
        else:
            pad = Engine.pad_len_from_mask(mask, L)
            self.engine.prefill(tokens, pad, position_mode=0)
        fm = ft = None
        if edit_region is not None:                        # use_teacher_forcing branch (:593-598)
            ft, fm = gt_labels, (edit_region != 0).to(torch.uint8)
        elif force_tokens is not None:
            ft = force_tokens
        lpkw = {"return_logprobs": True} if return_logprobs else {}        # without it: exactly the call made before scores existed
        if _stats_on(return_stats):
            lpkw["return_stats"] = return_stats
        if plan is not None:
            lpkw["plan"] = plan
        return self.engine.decode_image_tokens(n_tokens, cfg_weight, temperature, seed, ft, fm, return_logits, top_k=top_k, top_p=top_p, **lpkw)

    @staticmethod
    def forced_prefix_len(edit_region: torch.Tensor) -> int:
        """t0 of ``prefill_forced_prefix``: the smallest raster index, over the batch, with ``edit_region != 0`` (T when no cell of any row
        is edited).  Every image token in front of it is forced to the ground-truth code in every row."""
        free = (edit_region.reshape(edit_region.shape[0], -1) != 0).any(0)
        hit = torch.nonzero(free)
        return int(hit[0]) if hit.numel() else int(free.numel())

    @torch.no_grad()
    def sample_image_forced_prefix(self, tokens: torch.Tensor, mask: torch.Tensor, cfg_weight: float, temperature: float, seed: int,
                                   edit_region: torch.Tensor, gt_labels: torch.Tensor, t0: int, top_k: int = 0, top_p: float = 1.0):
        """``sample_image`` under teacher forcing with the first ``t0`` image tokens (forced in every row) fed in ONE pass: prefill without the
        shared negative prompt (an extension cannot follow the aliased rows), ``Engine.extend`` both rows of every pair with
        prepare_gen_img_embeds(gt[:, :t0]), then T - t0 decode steps with the force arrays sliced.  Sampled draws count their RNG steps from
        the first DECODED step: another, equally valid noise stream than the unaccelerated loop's; greedy is unaffected."""
        L = tokens.shape[1]
        T = gt_labels.shape[1]
        eng = self.engine
        eng.prefill(tokens, Engine.pad_len_from_mask(mask, L), position_mode=0, uncond_shared=False)
        gt = gt_labels.to(eng.device, torch.int32)
        eng.extend(embeds=eng.gen_embed(gt[:, :t0].repeat_interleave(2, 0)).view(tokens.shape[0], t0, self.cfg.hidden))
        fm = (edit_region.reshape(gt.shape[0], -1)[:, t0:] != 0).to(torch.uint8).contiguous()
        dec = eng.decode_image_tokens(T - t0, cfg_weight, temperature, seed, gt[:, t0:].contiguous(), fm, False, top_k=top_k, top_p=top_p)
        return torch.cat([gt[:, :t0], dec.to(torch.int32)], dim=1)

    @staticmethod
    def image_token_stats_summary(stats: dict, forced: Optional[torch.Tensor] = None) -> dict:
        """Per image, from the [B, T] arrays of a stats request: mean entropy (nats), mean rank of the emitted token and the share of
        positions where it was the mode.  forced bool [B, T] (teacher forcing: the positions that carry the given image's token): also
        top1 / top5, the share of the forced positions whose given token ranked 0 / below 5 (null for an image without forced positions)."""
        ent, rank = stats["entropy"].float(), stats["rank"]
        s = dict(mean_entropy=ent.mean(1).cpu().tolist(), mean_rank=rank.float().mean(1).cpu().tolist(),
                 rank0_share=(rank == 0).float().mean(1).cpu().tolist())
        if forced is not None:
            f = forced.to(rank.device)
            n = f.sum(1)
            for name, k in (("top1", 1), ("top5", 5)):
                hit = ((rank < k) & f).sum(1)
                s[name] = [h / c if c else None for h, c in zip(hit.cpu().tolist(), n.cpu().tolist())]
        return s

    PLAN_KEYS = ("cfg_schedule", "cfg_weight_end", "cfg_weights", "same_noise", "cfg_weight_in_box", "temperatures", "top_ks", "top_ps")

    def plan_keys_set(self) -> List[str]:
        """The sample-plan cfg keys that are on (cfg_schedule other than 'constant', same_noise true, any other key not None)."""
        a = self.args
        on = []
        for k in self.PLAN_KEYS:
            v = getattr(a, k, None)
            if (k == "cfg_schedule" and v not in (None, "constant")) or (k == "same_noise" and bool(v)) or (k not in ("cfg_schedule", "same_noise") and v is not None):
                on.append(k)
        return on

    def _prompt_box_texts(self, row_ids) -> List[str]:
        """The box texts of the ``<ref>..</ref><box>..</box>`` items of one prompt row, found by their tag ids as ``attribute_layout`` finds them."""
        from .textproc import layout_spans
        if self.codec is None:
            raise PlanGenError("cfg_weight_in_box needs a tokenizer (System(codec=...)): the layout's boxes are found by their tag ids")
        tags = {t: self.codec.token_id(t) for t in ("<ref>", "</ref>", "<box>", "</box>")}
        return [self.decode_text(row_ids[a:z]) for a, z in layout_spans(row_ids, tags, "box")]

    def build_sample_plan(self, cond_rows, p: int, cfg_weight: float, T: int):
        """The plan of the cfg keys for ``p`` replicas of the prompts ``cond_rows`` (one id list per prompt) in the replica layout (image t * B0 + i =
        replica t of prompt i), or (None, None) when no key is set.  Replica t's weight runs by ``cfg_schedule`` from cfg_weights[t] (else cfg_weight)
        to cfg_weight_end (else it stays); positions inside a box of prompt i's layout take cfg_weight_in_box; temperatures / top_ks / top_ps are
        per-replica lists; same_noise gives the replicas of prompt i the RNG key of its first replica.  Returns (SamplePlan, record for the batch JSON)."""
        import numpy as np
        from . import guidance as G
        on = self.plan_keys_set()
        if not on:
            return None, None
        a = self.args
        B0 = len(cond_rows)
        def per_replica(key):
            v = getattr(a, key, None)
            if v is None:
                return None
            v = list(v)
            if len(v) != p:
                raise PlanGenError(f"{key} holds {len(v)} entries, parallel_size is {p}")
            return v
        kind = getattr(a, "cfg_schedule", None) or "constant"
        starts = per_replica("cfg_weights") or [float(cfg_weight)] * p
        end = getattr(a, "cfg_weight_end", None)
        ends = [float(s) if end is None or kind == "constant" else float(end) for s in starts]
        in_box = getattr(a, "cfg_weight_in_box", None)
        share = [0.0] * (B0 * p)
        w = None
        if kind != "constant" or getattr(a, "cfg_weights", None) is not None or end is not None or in_box is not None:
            g = self.cfg.grid
            w = np.stack([G.schedule(kind, starts[t], ends[t], T) for t in range(p) for _ in range(B0)])
            if in_box is not None:
                if T != g * g:
                    raise PlanGenError(f"cfg_weight_in_box needs a full image of {g * g} positions (got T = {T})")
                for i, row in enumerate(cond_rows):
                    cells = G.box_weights(self._prompt_box_texts(row), g, 1.0, 0.0, bool(getattr(a, "use_centerhw", False))) > 0
                    for t in range(p):
                        w[t * B0 + i, cells] = np.float32(in_box)
                        share[t * B0 + i] = float(cells.mean())
        rep = lambda v: None if v is None else np.repeat(np.asarray(v), B0)
        key = None
        if bool(getattr(a, "same_noise", False)):
            key = np.tile(np.arange(B0, dtype=np.int64) + int(getattr(self.engine, "rng_image_offset", 0)), p)
        plan = G.SamplePlan(cfg_weight=w, temperature=rep(per_replica("temperatures")), top_k=rep(per_replica("top_ks")), top_p=rep(per_replica("top_ps")),
                            image_key=key)
        record = dict(schedule=kind, weight_start=[float(v) for v in starts], weight_end=ends, weight_in_box=None if in_box is None else float(in_box),
                      in_box_share=share, same_noise=bool(getattr(a, "same_noise", False)), keys=on)
        return plan, record

    @staticmethod
    def select_best_replicas(logprobs: torch.Tensor, p: int, scored: Optional[torch.Tensor] = None):
        """The select_best rule on the device.  logprobs fp32 [p * B0, T] in the replica layout (row t * B0 + i = replica t of prompt i);
        scored bool [B0, T] or None: the positions that count (teacher forcing: the positions that were NOT forced -- the first replica is
        forced there, and the others are scored on the same positions so that the means compare).  A replica's score is the mean of its
        scored log-probs (0 scored positions: 0.0); per prompt the arg-max wins, ties go to the lowest t, and a replica with a -inf
        token (score -inf) loses to any finite one.  Returns (rows int64 [B0] = t * B0 + i, replica int64 [B0], scores fp32 [p, B0])."""
        n, T = logprobs.shape
        B0 = n // p
        lp = logprobs.view(p, B0, T)
        if scored is None:
            scores = lp.sum(-1) / T
        else:
            m = scored.to(lp.device).bool().reshape(1, B0, T)
            scores = torch.where(m, lp, torch.zeros_like(lp)).sum(-1) / m.sum(-1).clamp(min=1)
        scores = torch.nan_to_num(scores, nan=float("-inf"), posinf=float("inf"), neginf=float("-inf"))
        # first maximum along t: max over (score, -t) -- torch.argmax's choice among equal values is not part of its contract on every device
        best = scores.max(0, keepdim=True).values
        t_idx = torch.arange(p, device=lp.device).view(p, 1).expand(p, B0)
        replica = torch.where(scores == best, t_idx, torch.full_like(t_idx, p)).min(0).values
        rows = replica * B0 + torch.arange(B0, device=lp.device)
        return rows, replica, scores

    @torch.no_grad()
    def sample_image_stepwise(self, inputs_embeds: torch.Tensor, mask: torch.Tensor, cfg_weight: float,
                              n_tokens: Optional[int] = None) -> torch.Tensor:
        """The reference's own loop shape (:567-607) through the drop-in facade, greedy: one
        ``language_model.model`` call + ``gen_head`` + ``prepare_gen_img_embeds`` per token."""
        T = self.image_token_num_per_image if n_tokens is None else n_tokens
        num_gen = inputs_embeds.shape[0] // 2
        generated = torch.zeros((num_gen, T), dtype=torch.int, device=self.device)
        outputs = None
        for i in range(T):
            outputs = self.vl_gpt.language_model.model(inputs_embeds=inputs_embeds, attention_mask=mask, use_cache=True,
                                                       past_key_values=outputs.past_key_values if i != 0 else None)
            hidden_states = outputs.last_hidden_state
            logits = self.vl_gpt.gen_head(hidden_states[:, -1, :])
            logit_cond, logit_uncond = logits[0::2, :], logits[1::2, :]
            logits = logit_uncond + cfg_weight * (logit_cond - logit_uncond)
            next_token = torch.argmax(logits, dim=-1, keepdim=True)
            generated[:, i] = next_token.squeeze(-1)
            next_token = torch.cat([next_token.unsqueeze(1), next_token.unsqueeze(1)], dim=1).view(-1)
            inputs_embeds = self.vl_gpt.prepare_gen_img_embeds(next_token).unsqueeze(1)
        return generated

    @torch.no_grad()
    def t2i(self, tokens: torch.Tensor, mask: torch.Tensor, cfg_weight: Optional[float] = None,
            temperature: Optional[float] = None, gt_image: Optional[torch.Tensor] = None,
            edit_region: Optional[torch.Tensor] = None, parallel_size: Optional[int] = None,
            top_k: Optional[int] = None, top_p: Optional[float] = None):
        """System.t2i (plangen_base.py:525-565): (teacher forcing: VQ-encode the ground truth :528-532) -> replicate x
        parallel_size (:547) -> sample_image -> decode_code (:555).  Returns ``(dec, mask_image)`` like the reference:
        dec [B*p,3,S,S] fp32; mask_image = the edit region resized to janus_hw (:557-560) under use_teacher_forcing,
        else None.  The generated tokens stay in ``self.last_generated_tokens`` (int32 [B*p, T]).
        args.select_best with p > 1: the loop also returns every token's log-probability, each prompt keeps the replica with the highest
        mean (``select_best_replicas``; a device arg-max + gather, no host round trip) and ONLY those B rows go through the VQ decoder:
        dec is [B,3,S,S] in prompt order, ``last_generated_tokens`` [B, T], and ``self.last_selection`` holds replica / score / scores."""
        a = self.args
        cfg_weight = a.cfg_weight if cfg_weight is None else cfg_weight
        temperature = a.temperature if temperature is None else temperature
        p = a.parallel_size if parallel_size is None else parallel_size
        top_k = getattr(a, "top_k", 0) if top_k is None else top_k
        top_p = getattr(a, "top_p", 1.0) if top_p is None else top_p
        gt_labels = None
        if a.use_teacher_forcing and gt_image is not None:
            bs = gt_image.shape[0]
            # the reference encodes gt_image.bfloat16() (:530): in bf16 mode the encoder sees bf16 pixels
            gi = gt_image.to(torch.bfloat16) if self.engine.dtype == "bf16" else gt_image
            gt_labels = self.vl_gpt.gen_vision_model.encode(gi)[-1][-1].reshape(bs, -1).to(torch.int32)
        force_region = edit_region
        # share_replicas (cfg key, default 0): the ids stay un-replicated and every prompt is prefilled once; the mask, the forced labels and the
        # all-ones regions of replicas 2..p are built as below either way
        share = p > 1 and bool(int(getattr(a, "share_replicas", 0)))
        B0 = tokens.shape[0] // 2
        num_gen = B0 * p
        select = p > 1 and bool(getattr(a, "select_best", False))
        self.last_selection = None
        want_stats = getattr(a, "token_stats", False)
        stats_on = _stats_on(want_stats)
        self.last_token_stats = None
        if p > 1:
            if not share:
                tokens = torch.cat([tokens] * p)
            mask = torch.cat([mask] * p)
            if gt_labels is not None:
                # The reference's forcing loop runs over ``len(batch['edit_region'])`` = the B un-replicated rows (:593-598), so only the
                # FIRST replica of every image is teacher-forced and replicas 2..p sample freely.  Matched here (VERDICT r3 missing 5):
                # the extra replicas get an all-ones region (= nothing forced); the returned mask_image stays the B-row one (:557-560).
                gt_labels = torch.cat([gt_labels] * p)
                force_region = torch.cat([edit_region] + [torch.ones_like(edit_region)] * (p - 1))
        # the sample-plan cfg keys (all off by default, and then nothing changes): one plan over the B0 * p images of the loop
        L0 = tokens.shape[1]
        plan, self.last_sample_plan = (None, None)
        if self.plan_keys_set():
            cond_rows = [tokens[2 * i][mask[2 * i, :L0].bool()].tolist() for i in range(B0)]
            plan, self.last_sample_plan = self.build_sample_plan(cond_rows, p, cfg_weight, self.image_token_num_per_image)
        # prefill_forced_prefix (cfg key, default False; use_teacher_forcing only): the image tokens in front of the first edited cell are known
        # before the loop starts -- one extension instead of t0 decode steps
        t0 = 0
        self.last_forced_prefix = None
        if bool(getattr(a, "prefill_forced_prefix", False)) and gt_labels is not None:
            clash = [k for k, on in (("select_best", select), ("token_stats", stats_on), ("return_logprobs", bool(getattr(a, "return_logprobs", False))),
                                     ("a sample plan (" + ", ".join(self.plan_keys_set()) + ")", plan is not None), ("share_replicas", share)) if on]
            if clash:
                raise PlanGenError(f"prefill_forced_prefix cannot be combined with {' / '.join(clash)}: the prefilled tokens never pass through the "
                                   "sampler, so they have no log-probabilities, statistics or plan steps (and replicated prompts cannot be extended)")
            t0 = min(self.forced_prefix_len(force_region), self.image_token_num_per_image - 1)      # at least one step stays in the loop
            self.last_forced_prefix = t0
        if t0 >= 1:
            toks = self.sample_image_forced_prefix(tokens, mask, cfg_weight, temperature, a.seed, force_region, gt_labels, t0, top_k=top_k, top_p=top_p)
        else:
            toks = self.sample_image(tokens, mask, cfg_weight, temperature, a.seed,
                                     force_region if gt_labels is not None else None, gt_labels, top_k=top_k, top_p=top_p,
                                     replicas=p if share else 1, **({"return_logprobs": True} if select else {}), **({"plan": plan} if plan is not None else {}),
                                     **({"return_stats": want_stats} if stats_on else {}))
        if stats_on:
            toks, stats = toks[:-1], toks[-1]
            toks = toks if select else toks[0]
        if select:
            toks, lp = toks
            scored = (edit_region != 0).reshape(B0, -1) if gt_labels is not None else None
            rows, replica, scores = self.select_best_replicas(lp, p, scored)
            toks = toks.index_select(0, rows)
            if stats_on:
                stats = {k: v.index_select(0, rows) for k, v in stats.items()}
            num_gen = B0
            self.last_selection = dict(replica=replica, score=scores.gather(0, replica.view(1, B0))[0], scores=scores)
        dec = self.vl_gpt.gen_vision_model.decode_code(toks.to(dtype=torch.int),
                                                       shape=[num_gen, self.cfg.img_dim, self.cfg.grid, self.cfg.grid])
        self.last_generated_tokens = toks
        if stats_on:
            # under teacher forcing the rank at the forced positions (edit_region == 0) of the first replica is the model's accuracy there
            forced = None
            if gt_labels is not None and not select:
                forced = torch.cat([(edit_region == 0).reshape(B0, -1)] + [torch.zeros((B0 * (p - 1), toks.shape[1]), dtype=torch.bool, device=edit_region.device)] * (p > 1))
            self.last_token_stats = dict(stats, summary=self.image_token_stats_summary(stats, forced))
        mask_image = None
        if a.use_teacher_forcing and edit_region is not None:
            er = edit_region.to(dec.device)
            bs = er.shape[0]
            g = self.cfg.grid
            # resize_pt = torchvision Resize (bilinear, antialias) of the [bs,3,g,g] map to janus_hw (funcs.py:523-528); the
            # edit map is piecewise constant on the g x g grid and janus_hw is a multiple of g: bilinear without antialias here
            mask_image = torch.nn.functional.interpolate(er.reshape(bs, 1, g, g).repeat(1, 3, 1, 1).float(), size=(a.janus_hw, a.janus_hw),
                                                         mode="bilinear", align_corners=False).to(dec)
        return dec, mask_image

    # -------------------------------------------------------------- dual guidance
    DUAL_REFUSED_KEYS = ("share_replicas", "prefill_forced_prefix", "select_best", "token_stats", "score_gt_image")

    def dual_weight_layout(self) -> Optional[float]:
        """The ``cfg_weight_layout`` cfg key: None (absent or None) is off, and then nothing changes."""
        v = getattr(self.args, "cfg_weight_layout", None)
        return None if v is None else float(v)

    def check_dual_keys(self) -> None:
        """The cfg keys the dual loop does not serve, refused by name before anything runs."""
        a = self.args
        on = [k for k in self.DUAL_REFUSED_KEYS if (_stats_on(getattr(a, k, False)) if k == "token_stats" else bool(int(getattr(a, k, 0) or 0)))]
        on += self.plan_keys_set()
        if on:
            raise PlanGenError(f"cfg_weight_layout (dual guidance) cannot be combined with {' / '.join(on)}: the three-row loop has no replica sharing, "
                               "no sample plan, no prefilled prefix and no statistics; select_best and score_gt_image would score another distribution")

    def t2i_dual_collate_batch(self, cond_ids, caption_ids, neg_ids):
        return t2i_dual_collate_batch(cond_ids, caption_ids, neg_ids, self.cfg.pad_id, self.image_token_num_per_image, self.args.debug_max_seq_len)

    @torch.no_grad()
    def t2i_dual(self, tokens3: torch.Tensor, mask3: torch.Tensor, w_caption: Optional[float] = None, w_layout: Optional[float] = None,
                 temperature: Optional[float] = None, gt_image: Optional[torch.Tensor] = None, edit_region: Optional[torch.Tensor] = None,
                 parallel_size: Optional[int] = None, top_k: Optional[int] = None, top_p: Optional[float] = None, return_logprobs: bool = False):
        """``t2i`` under dual guidance: tokens3 int32 [3B, L] / mask3 [3B, L + T] are triples (``t2i_dual_collate_batch``: full prompt, caption-only
        prompt, negative prompt); mixed = u + w_caption (p - u) + w_layout (f - p) with w_caption = args.cfg_weight and w_layout =
        args.cfg_weight_layout unless given.  One prefill with uncond_shared=False, ``Engine.decode_image_tokens_dual``, then the VQ decoder.
        Teacher forcing (use_teacher_forcing + gt_image + edit_region) takes the force arguments of ``t2i``; parallel_size > 1 replicates the triples
        (first replica forced, the others free); top_k / top_p as in ``t2i``.  return_logprobs: the emitted tokens' log-probabilities fp32
        [B * p, T] stay in ``self.last_logprobs`` (None otherwise).  Returns ``(dec, mask_image)`` like ``t2i``."""
        a = self.args
        self.check_dual_keys()
        w_caption = a.cfg_weight if w_caption is None else w_caption
        w_layout = self.dual_weight_layout() if w_layout is None else w_layout
        if w_layout is None:
            raise PlanGenError("t2i_dual needs w_layout (or the cfg key cfg_weight_layout)")
        temperature = a.temperature if temperature is None else temperature
        p = a.parallel_size if parallel_size is None else parallel_size
        top_k = getattr(a, "top_k", 0) if top_k is None else top_k
        top_p = getattr(a, "top_p", 1.0) if top_p is None else top_p
        want_lp = bool(return_logprobs)
        if tokens3.shape[0] % 3:
            raise PlanGenError(f"t2i_dual: {tokens3.shape[0]} rows are not triples")
        B0 = tokens3.shape[0] // 3
        if 3 * B0 * p > self.engine.max_rows:
            raise PlanGenError(f"cfg_weight_layout (dual guidance): 3 x {B0} prompts x parallel_size {p} = {3 * B0 * p} rows exceed the engine's "
                               f"max_rows={self.engine.max_rows}")
        gt_labels = None
        if a.use_teacher_forcing and gt_image is not None:
            gi = gt_image.to(torch.bfloat16) if self.engine.dtype == "bf16" else gt_image
            gt_labels = self.vl_gpt.gen_vision_model.encode(gi)[-1][-1].reshape(gt_image.shape[0], -1).to(torch.int32)
        force_region = edit_region
        if p > 1:
            tokens3, mask3 = torch.cat([tokens3] * p), torch.cat([mask3] * p)
            if gt_labels is not None:          # as in t2i: only the first replica of every image is teacher-forced
                gt_labels = torch.cat([gt_labels] * p)
                force_region = torch.cat([edit_region] + [torch.ones_like(edit_region)] * (p - 1))
        L = tokens3.shape[1]
        self.engine.prefill(tokens3, Engine.pad_len_from_mask(mask3, L), position_mode=0, uncond_shared=False)
        ft = fm = None
        if gt_labels is not None and force_region is not None:
            ft, fm = gt_labels, (force_region.reshape(gt_labels.shape[0], -1) != 0).to(torch.uint8)
        res = self.engine.decode_image_tokens_dual(None, w_caption, w_layout, temperature, a.seed, ft, fm, False, top_k=top_k, top_p=top_p,
                                                   **({"return_logprobs": True} if want_lp else {}))
        toks, self.last_logprobs = (res if want_lp else (res, None))
        self.last_dual_guidance = dict(w_caption=float(w_caption), w_layout=float(w_layout))
        dec = self.vl_gpt.gen_vision_model.decode_code(toks.to(dtype=torch.int), shape=[B0 * p, self.cfg.img_dim, self.cfg.grid, self.cfg.grid])
        self.last_generated_tokens = toks
        mask_image = None
        if a.use_teacher_forcing and edit_region is not None:
            er = edit_region.to(dec.device)
            bs, g = er.shape[0], self.cfg.grid
            mask_image = torch.nn.functional.interpolate(er.reshape(bs, 1, g, g).repeat(1, 3, 1, 1).float(), size=(a.janus_hw, a.janus_hw),
                                                         mode="bilinear", align_corners=False).to(dec)
        return dec, mask_image

    def _cfg_prompt_dual(self, batch: dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """The triples of the image stage under dual guidance: the rows ``_cfg_prompt`` builds, and between them the caption-only row
        wrap_uni_prompt(base_caption[i], '') -- the form the negative prompt uses for an absent layout -- or batch['caption_inputs_ids'] (one id
        list per sample) for callers who stay on ids -> (ids [3B, L], mask [3B, L + T])."""
        ids2, mask2 = self._cfg_prompt(batch)
        L = ids2.shape[1]
        rows = [ids2[r][mask2[r, :L].bool()].tolist() for r in range(ids2.shape[0])]
        bs = len(rows) // 2
        caps = batch.get("caption_inputs_ids")
        if caps is not None:
            caps = [[int(t) for t in c] for c in caps]
        elif batch.get("base_caption") is not None and self.codec is not None:
            caps = [self.wrap_uni_prompt(c, "")[1].tolist() for c in batch["base_caption"]]
        else:
            raise PlanGenError("cfg_weight_layout (dual guidance) needs the caption-only prompts: batch['caption_inputs_ids'], or batch['base_caption'] "
                               "with a tokenizer (System(codec=...))")
        if len(caps) != bs:
            raise PlanGenError(f"cfg_weight_layout (dual guidance): {len(caps)} caption-only prompts for {bs} samples")
        return self.t2i_dual_collate_batch(rows[0::2], caps, rows[1::2])

    # -------------------------------------------------------------- a12: text either side of the path
    def wrap_uni_prompt(self, caption: str, grounding: Optional[str] = None, in_stage1: bool = False):
        """plangen_base.py:232-261 -> (prompt string, ids LongTensor)."""
        from .textproc import wrap_uni_prompt_ids
        prompt, ids = wrap_uni_prompt_ids(self._codec(), caption, grounding, in_stage1)
        return prompt, torch.as_tensor(ids, dtype=torch.long)

    def _codec(self):
        if self.codec is None:
            raise PlanGenError("this step needs a tokenizer: pass codec=HFCodec(janus_path) (or TagWordCodec for offline runs) to System")
        return self.codec

    def decode_text(self, inputs_ids) -> str:
        return self._codec().decode([int(t) for t in inputs_ids])

    def decode_plan_text_batch(self, inputs_ids) -> List[str]:
        from .textproc import cut_plan_text
        return [cut_plan_text(self.decode_text(t)) for t in inputs_ids]

    def decode_mmu_text_batch(self, inputs_ids) -> List[str]:
        from .textproc import cut_at_eos
        eos = self._codec().eos_token_id
        return [self.decode_text(cut_at_eos([int(v) for v in t], eos)) for t in inputs_ids]

    @staticmethod
    def trans_gr_to_creati(prompt: str):
        from .textproc import trans_gr_to_creati
        return trans_gr_to_creati(prompt)

    @torch.no_grad()
    def uni_generate(self, batch: dict, gen_path: Optional[str] = None, batch_idx=None, pred_layout: bool = True,
                     pred_image: bool = True, save_local: bool = False, use_uni_prompt_in_t2i: bool = True, is_mmu: bool = False,
                     layout_to_prompt=None, max_new_tokens: int = 512, min_new_tokens: int = 0, **kwargs) -> dict:
        """System.uni_generate (plangen_base.py:327-458) without the box-drawing tail (PIL visualisation is outside the path).

        task_type 'uni'        : pred_layout=False -> t2i on batch['uni_inputs_ids'/'uni_attention_mask'].
        task_type 'uni_2stage' : stage 1 layout tokens (greedy; sampled when args.text_temperature > 0, see x2t) from batch['uni_stage1_inputs_ids'/'uni_stage1_attention_mask']
            (x2t, :371-377) -> decode_plan_text_batch (:382) -> wrap_uni_prompt(base_caption, layout) per sample
            (:385-388) -> pad_input_ids (:389) -> t2i.  ``layout_to_prompt(i, new_ids) -> list[int]`` replaces the tokenizer
            round trip when the caller wants to stay on ids.
        task_type 'mmu'        : is_mmu, pred_image=False -> prepare_inputs_embeds(**batch['prepare_inputs_infer']) (:365-366)
            + greedy decode + decode_mmu_text_batch (:379-380).
        task_type 'plan'       : pred_image=False: layout text only.
        Negative prompt: batch['neg_inputs_ids'] (ids of wrap_uni_prompt(neg_prompt, ''), :673-686; or one list per sample for
        use_neg_box, :652-670); when absent it is built from args.neg_prompt through the codec.
        Returns dict(pr_grounding, pr_image) like the reference (+ pr_layout_ids / pr_text_ids / pr_tokens)."""
        out = {}
        dev = self.device
        base_caption = batch.get("base_caption")
        pr_grounding = batch.get("gt_grounding")
        if pred_layout:
            if is_mmu:
                pin = batch["prepare_inputs_infer"]
                emb = self.vl_gpt.prepare_inputs_embeds(**{k: v for k, v in pin.items() if k != "attention_mask"})
                attention_mask = pin["attention_mask"]
            else:
                ids1 = batch["uni_stage1_inputs_ids"].to(dev)
                attention_mask = batch["uni_stage1_attention_mask"]
                emb = self.vl_gpt.language_model.get_input_embeddings()(ids1)
            dfa = None
            if not is_mmu and getattr(self.args, "layout_grammar", False):
                # the layout string only: mmu captions stay free text
                if self.codec is None:
                    raise PlanGenError("layout_grammar needs a tokenizer (System(codec=...)): the automaton is built over its vocabulary")
                from .grammar import layout_token_dfa
                dfa = layout_token_dfa(self.codec, self.cfg.vocab)
            best_of = 1 if is_mmu else int(getattr(self.args, "layout_best_of", 1))
            if best_of > 1:
                # draw N layouts per row and keep the one the model finds most probable: the batch is replicated like parallel_size replicates
                # images (row t * B + i = draw t of row i; different global rows, hence different draws), generated with log-probs, and each row
                # is scored by its sequence log-probability / its number of scored tokens (up to and including its EOS)
                nb = emb.shape[0]
                if not float(getattr(self.args, "text_temperature", 0.0)) > 0:
                    raise PlanGenError(f"layout_best_of={best_of} needs text_temperature > 0: greedy decode would draw the same layout {best_of} times")
                if best_of * nb > self.engine.max_rows:
                    raise PlanGenError(f"layout_best_of={best_of} x {nb} stage-1 rows = {best_of * nb} rows exceed the engine's max_rows={self.engine.max_rows}")
                emb = torch.cat([emb] * best_of)
                attention_mask = torch.cat([attention_mask] * best_of)
            want_stats = getattr(self.args, "token_stats", False)
            outputs = self.x2t(emb, attention_mask.to(dev), max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens,
                               **({} if dfa is None else {"dfa": dfa}), **({} if best_of == 1 else {"return_logprobs": True}),
                               **({"return_stats": want_stats} if _stats_on(want_stats) else {}))
            tstats = None
            if _stats_on(want_stats):
                tstats, outputs = outputs[-1], (outputs[:-1] if best_of > 1 else outputs[0])
            if best_of > 1:
                outputs, lp = outputs
                rows_best, replica, score = self.select_best_layouts(outputs, lp, best_of, self.cfg.eos_id)
                outputs = outputs.index_select(0, rows_best)
                out["pr_layout_replica"], out["pr_layout_score"] = replica, score
                if tstats is not None:
                    tstats = {k: v.index_select(0, rows_best) for k, v in tstats.items()}
            if tstats is not None:
                out["text_token_stats"] = self.text_token_stats_summary(outputs, tstats, self.cfg.eos_id)
            out["pr_text_ids" if is_mmu else "pr_layout_ids"] = outputs
            rows = outputs.cpu().tolist()
            if self.codec is not None:
                pr_grounding = self.decode_mmu_text_batch(rows) if is_mmu else self.decode_plan_text_batch(rows)
            else:
                pr_grounding = None
            if pred_image:
                if layout_to_prompt is not None:
                    all_ids = [list(layout_to_prompt(i, r)) for i, r in enumerate(rows)]
                elif pr_grounding is not None and base_caption is not None:
                    all_ids = [self.wrap_uni_prompt(c, g)[1].tolist() for c, g in zip(base_caption, pr_grounding)]
                else:
                    raise PlanGenError("uni_2stage needs a tokenizer (System(codec=...)) with batch['base_caption'], or layout_to_prompt")
                uni_ids, uni_mask = self.pad_input_ids(all_ids)
                bs = len(all_ids)
                batch = dict(batch, uni_inputs_ids=uni_ids,
                             uni_attention_mask=torch.cat([uni_mask, torch.ones((bs, self.image_token_num_per_image), dtype=uni_mask.dtype)], -1))
        if pred_image:
            if not use_uni_prompt_in_t2i:
                raise PlanGenError("use_uni_prompt_in_t2i=False: the reference asserts False on this branch too (plangen_base.py:645-648)")
            self.last_dual_guidance = None
            if self.dual_weight_layout() is not None:
                # cfg_weight_layout (cfg key, absent / None: off): triples and the dual loop; cfg_weight is the caption weight
                self.check_dual_keys()
                self.last_token_stats = self.last_sample_plan = self.last_forced_prefix = self.last_selection = None
                ids3, mask3 = self._cfg_prompt_dual(batch)
                dec, edit_mask = self.t2i_dual(ids3, mask3, gt_image=batch.get("image"), edit_region=batch.get("edit_region"))
                out["dual_guidance"] = self.last_dual_guidance
            else:
                cfg_ids, cfg_mask = self._cfg_prompt(batch)
                dec, edit_mask = self.t2i(cfg_ids, cfg_mask, gt_image=batch.get("image"), edit_region=batch.get("edit_region"))
            out["pr_tokens"] = self.last_generated_tokens
            if self.last_token_stats is not None:
                out["image_token_stats"] = self.last_token_stats["summary"]
                out["image_entropy"] = self.last_token_stats["entropy"].view(-1, self.cfg.grid, self.cfg.grid)
            if self.last_sample_plan is not None:
                out["sample_plan"] = self.last_sample_plan
            if self.last_forced_prefix is not None:
                out["forced_prefix"] = self.last_forced_prefix
            if self.last_selection is not None:
                out["pr_replica"], out["pr_score"] = self.last_selection["replica"], self.last_selection["score"]
            out["pr_image"] = dec.float()
            out["edit_mask"] = edit_mask
        else:
            out["pr_image"] = batch.get("image")
        out["pr_grounding"] = pr_grounding
        if getattr(self.args, "score_gt_image", False) and pred_image and batch.get("image") is not None:
            # uni / uni_2stage: P(ground-truth image | the prompt the image above was generated from) under the guided distribution.  Runs after
            # the generation: it re-prefills.
            sc = self.score_images(batch, scored=(batch["edit_region"] != 0) if batch.get("edit_region") is not None else None)
            out["gt_image_logprob"] = {k: sc[k] for k in ("sum", "mean", "n_tokens")}
        if getattr(self.args, "layout_attribution", False) and pred_image:
            # uni / uni_2stage: attention of the image positions on the layout items of the prompt, scored on the tokens just generated (replica 0
            # when parallel_size > 1).  Runs after the generation: it re-prefills.
            att = self.attribute_layout(batch, codes=self.last_generated_tokens[:batch["uni_inputs_ids"].shape[0]])
            out["layout_attribution"] = [[dict(phrase=p, inside=(None if v != v else v)) for p, v in zip(a["phrases"], a["inside"])] for a in att]
            out["layout_attribution_maps"] = [a["maps"] for a in att]
        if getattr(self.args, "score_gt_layout", False) and pred_layout and batch.get("gt_grounding") is not None:
            # plan / uni_2stage: P(ground-truth layout | caption); mmu: P(ground-truth layout | image).  Runs after the generation: it re-prefills.
            sc = self.score_layouts(batch, given="image" if is_mmu else "caption")
            out["gt_layout_logprob"] = {k: sc[k] for k in ("sum", "mean", "n_tokens")}
        if save_local and gen_path is not None:
            # the reference's per-batch layout record (:416-420); its annotated PNG grid is box drawing, not part of the path
            import json
            import os
            os.makedirs(gen_path, exist_ok=True)
            with open(os.path.join(gen_path, f"{batch_idx}_layout.json"), "w") as f:
                extra = {k: out[k].cpu().tolist() for k in ("pr_replica", "pr_score", "pr_layout_replica", "pr_layout_score") if k in out}
                if "gt_layout_logprob" in out:
                    extra["gt_layout_logprob"] = out["gt_layout_logprob"]
                if "gt_image_logprob" in out:
                    extra["gt_image_logprob"] = out["gt_image_logprob"]
                for k in ("image_token_stats", "text_token_stats", "sample_plan", "dual_guidance", "forced_prefix"):
                    if k in out:
                        extra[k] = out[k]
                if "image_entropy" in out:
                    import numpy as np
                    np.save(os.path.join(gen_path, f"{batch_idx}_entropy.npy"), out["image_entropy"].float().cpu().numpy())
                if "layout_attribution" in out:
                    import numpy as np
                    extra["layout_attribution"] = out["layout_attribution"]
                    maps = out["layout_attribution_maps"]          # [B, most items of a row, grid, grid], NaN where a row has fewer
                    arr = np.full((len(maps), max((m.shape[0] for m in maps), default=0), self.cfg.grid, self.cfg.grid), np.nan, dtype=np.float32)
                    for b, m in enumerate(maps):
                        arr[b, :m.shape[0]] = m.numpy()
                    np.save(os.path.join(gen_path, f"{batch_idx}_attribution.npy"), arr)
                json.dump(dict(base_caption=base_caption, gt_grounding=batch.get("gt_grounding"),
                               pr_grounding=pr_grounding if pred_layout else "", **extra), f)
        return out

    def _cfg_prompt(self, batch: dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """The CFG batch of the image stage: cond rows from batch['uni_inputs_ids' / 'uni_attention_mask'], the negative prompt from
        batch['neg_inputs_ids'] / args.use_neg_box / args.neg_prompt -> (cfg_inputs_ids [2B, L], cfg_attention_mask [2B, L + T])."""
        ids, mask = batch["uni_inputs_ids"], batch["uni_attention_mask"]
        L = ids.shape[1]
        m = mask[:, :L]
        cond = [ids[i][m[i].bool()].tolist() for i in range(ids.shape[0])]
        neg = batch.get("neg_inputs_ids")
        if getattr(self.args, "use_neg_box", False):
            # plangen_base.py:652-670: ONE negative prompt PER SAMPLE, wrap_uni_prompt(neg_base_caption, neg_gt_grounding)
            if "neg_base_caption" in batch and self.codec is not None:
                neg = [self.wrap_uni_prompt(c, g)[1].tolist() for c, g in zip(batch["neg_base_caption"], batch["neg_gt_grounding"])]
            elif not (neg is not None and len(neg) and isinstance(neg[0], (list, tuple, torch.Tensor))):
                raise PlanGenError("use_neg_box=True needs batch['neg_base_caption'] / ['neg_gt_grounding'] (with a tokenizer) "
                                   "or one pre-tokenised negative prompt per sample in batch['neg_inputs_ids']")
        if neg is None:
            neg = self.wrap_uni_prompt(getattr(self.args, "neg_prompt", ""), "")[1].tolist()
        return self.t2i_infer_collate_batch(cond, neg)

    @torch.no_grad()
    def score_images(self, batch: dict, scored: Optional[torch.Tensor] = None, cfg_weight: Optional[float] = None,
                     temperature: Optional[float] = None) -> dict:
        """How probable the model finds the images of ``batch['image']`` given the image-stage prompt: log P(image tokens | caption, layout)
        under the guided distribution the sampler draws from (args.cfg_weight; args.temperature when > 0, else 1.0 -- greedy decoding has no
        distribution of its own), nothing generated.  The images are VQ-encoded (the engine needs with_vq_encoder, PlanGenError otherwise),
        the CFG prompt is the one ``uni_generate`` hands to ``t2i`` (``_cfg_prompt``), and the batch is scored in chunks of as many images as
        the engine's max_rows and ``Engine.score_image_max_tokens`` allow, each one teacher-forced prefill + the fused CFG scoring head
        (``Engine.score_image``).  scored: bool [B, T] (e.g. ``edit_region != 0``) -- only those positions count; None: all T.
        Returns dict(sum, mean, n_tokens: one entry per image; logprobs fp32 [B, T], every position): mean = sum / n_tokens (0.0 when
        nothing is scored)."""
        eng = self.engine
        if self.plan_keys_set():
            raise PlanGenError(f"score_images / score_gt_image: the fused score head has one cfg_weight and cannot follow a sample plan ({', '.join(self.plan_keys_set())} "
                               "set).  Score under a plan with the decode loop instead: Engine.decode_image_tokens(force_tokens=codes, "
                               "force_mask=zeros, return_logprobs=True, plan=...)")
        if not eng._c.with_vq_encoder:
            raise PlanGenError("score_images VQ-encodes batch['image']: the engine must be created with_vq_encoder=True")
        a = self.args
        cfg_weight = a.cfg_weight if cfg_weight is None else cfg_weight
        if temperature is None:
            temperature = a.temperature if float(a.temperature) > 0 else 1.0
        img = batch["image"]
        B = img.shape[0]
        gi = img.to(torch.bfloat16) if eng.dtype == "bf16" else img
        codes = self.vl_gpt.gen_vision_model.encode(gi)[-1][-1].reshape(B, -1).to(torch.int32)
        T = codes.shape[1]
        cfg_ids, cfg_mask = self._cfg_prompt(batch)
        L = cfg_ids.shape[1]
        pad = Engine.pad_len_from_mask(cfg_mask, L)
        per = min(eng.max_rows // 2, eng.score_image_max_tokens() // (2 * (L + T - 1)))
        if per < 1:
            raise PlanGenError(f"score_images: one image pair of {L + T - 1} columns does not fit the engine (max_rows={eng.max_rows}, "
                               f"at most {eng.score_image_max_tokens()} packed tokens per prefill)")
        lp = torch.cat([eng.score_image(cfg_ids[2 * b0:2 * (b0 + per)], pad[2 * b0:2 * (b0 + per)], codes[b0:b0 + per], cfg_weight, temperature)
                        for b0 in range(0, B, per)])
        m = torch.ones((B, T), dtype=torch.bool, device=lp.device) if scored is None else scored.to(lp.device).bool().reshape(B, T)
        n_tok = m.sum(-1)
        sums = torch.where(m, lp, torch.zeros_like(lp)).sum(-1)
        return dict(sum=sums.cpu().tolist(), mean=(sums / n_tok.clamp(min=1)).cpu().tolist(), n_tokens=n_tok.cpu().tolist(), logprobs=lp)

    @torch.no_grad()
    def attribute_layout(self, batch: dict, codes: Optional[torch.Tensor] = None, kind: str = "entity", layers=None) -> List[dict]:
        """Was the model reading entity e of the layout while it painted inside box e?  For every image of the batch, the share of attention
        that the query positions predicting its image tokens put on the prompt tokens of each ``<ref>...</ref><box>...</box>`` item of its
        image-stage prompt (``_cfg_prompt``, the conditional row), from one teacher-forced prefill per pass (``Engine.attribute_image``):
        ``codes`` int [B, T] (e.g. the tokens just generated), or None: ``batch['image']`` is VQ-encoded as in ``score_images``.  kind
        'entity' / 'phrase' / 'box': which tokens of an item count (``textproc.layout_spans``).  layers: layer indices, None: all; the
        maps are their mean.  A row with more than 16 items takes ceil(E / 16) passes.  Needs a tokenizer (the tags are found by their
        ids), a bf16 engine with max_prompt >= L + T - 1.
        Returns one dict per image: ``phrases`` [E] str, ``maps`` fp32 [E, grid, grid] (attention mass of image position (y, x) on item e),
        ``inside`` [E]: the share of item e's mass over the image that falls into the cells of its own box (``textproc.box_cells`` with
        args.use_centerhw) -- NaN when the box holds no cell or the mass is 0."""
        from .textproc import box_cells, layout_spans
        eng, g = self.engine, self.cfg.grid
        if self.codec is None:
            raise PlanGenError("attribute_layout needs a tokenizer (System(codec=...)): the layout items are found by their tag ids")
        tags = {t: self.codec.token_id(t) for t in ("<ref>", "</ref>", "<box>", "</box>")}
        if codes is None:
            if not eng._c.with_vq_encoder:
                raise PlanGenError("attribute_layout VQ-encodes batch['image']: the engine must be created with_vq_encoder=True (or pass codes)")
            img = batch["image"]
            gi = img.to(torch.bfloat16) if eng.dtype == "bf16" else img
            codes = self.vl_gpt.gen_vision_model.encode(gi)[-1][-1].reshape(img.shape[0], -1)
        codes = codes.to(torch.int32)
        B, T = codes.shape
        cfg_ids, cfg_mask = self._cfg_prompt(batch)
        if cfg_ids.shape[0] != 2 * B or T != g * g:
            raise PlanGenError(f"attribute_layout: codes {tuple(codes.shape)} do not match the batch's {cfg_ids.shape[0] // 2} prompts x {g * g} image tokens")
        L = cfg_ids.shape[1]
        pad = Engine.pad_len_from_mask(cfg_mask, L)
        use_chw = bool(getattr(self.args, "use_centerhw", False))
        rows = [cfg_ids[2 * b].tolist() for b in range(B)]
        spans = [layout_spans(r, tags, kind) for r in rows]
        phrases = [[self.decode_text(r[a:z]) for a, z in layout_spans(r, tags, "phrase")] for r in rows]
        cells = [[box_cells(self.decode_text(r[a:z]), g, use_chw) for a, z in layout_spans(r, tags, "box")] for r in rows]
        e_max = max((len(s) for s in spans), default=0)
        mass = torch.zeros((B, T, e_max), dtype=torch.float32)
        per = min(eng.max_rows // 2, eng.score_image_max_tokens() // (2 * (L + T - 1)))
        if per < 1:
            raise PlanGenError(f"attribute_layout: one image pair of {L + T - 1} columns does not fit the engine (max_rows={eng.max_rows}, "
                               f"at most {eng.score_image_max_tokens()} packed tokens per prefill)")
        for e0 in range(0, e_max, 16):
            S = min(16, e_max - e0)
            lo = torch.zeros((B, S), dtype=torch.int32)
            hi = torch.zeros((B, S), dtype=torch.int32)          # rows with fewer items: empty spans
            for b, sp in enumerate(spans):
                for j, (a, z) in enumerate(sp[e0:e0 + S]):
                    lo[b, j], hi[b, j] = a, z
            for b0 in range(0, B, per):
                m = eng.attribute_image(cfg_ids[2 * b0:2 * (b0 + per)], pad[2 * b0:2 * (b0 + per)], codes[b0:b0 + per], lo[b0:b0 + per],
                                        hi[b0:b0 + per], layers)
                mass[b0:b0 + per, :, e0:e0 + S] = m.mean(0).cpu()
        out = []
        for b in range(B):
            E = len(spans[b])
            maps = mass[b, :, :E].t().reshape(E, g, g).contiguous()
            inside = []
            for e in range(E):
                tot, c = float(maps[e].double().sum()), torch.from_numpy(cells[b][e])
                inside.append(float(maps[e][c].double().sum()) / tot if c.any() and tot > 0 else float("nan"))
            out.append(dict(phrases=phrases[b], maps=maps, inside=inside))
        return out

    def _layout_ids(self, grounding: str, strip_open: bool) -> List[int]:
        """Token ids of a layout string without BOS; strip_open: also without the leading ``<grounding>`` the stage-1 prompt already carries."""
        codec = self._codec()

        def enc(text):
            ids = [int(t) for t in codec.encode(text)]
            return ids[1:] if ids and ids[0] == getattr(codec, "bos_token_id", None) else ids
        ids = enc(grounding)
        if strip_open:
            from .textproc import GROUNDING_OPEN
            opn = enc(GROUNDING_OPEN)
            if ids[:len(opn)] == opn:
                ids = ids[len(opn):]
        return ids

    @torch.no_grad()
    def score_layouts(self, batch: dict, given: str = "caption", temperature: float = 0.0) -> dict:
        """How probable the model finds the layouts of ``batch['gt_grounding']``: one teacher-forced prefill + the fused scoring head
        (``Engine.score_text`` / ``score_text_embeds``), nothing generated.
        given='caption': P(layout | caption) -- the stage-1 prompt ``wrap_uni_prompt(caption, '<grounding>', in_stage1=True)`` followed by
            the layout's tokens (without the ``<grounding>`` the prompt ends with) and EOS: what stage 1 would have to emit.
        given='image'  : P(layout | image) through the understanding path (the ``mmu`` form) -- ``prepare_inputs_embeds`` of
            ``batch['prepare_inputs_infer']`` (vision_encode + the embedding assembly) followed by the embeddings of the whole layout string and EOS.
        Only the appended tokens are scored.  Returns dict(sum, mean, n_tokens: one entry per row; logprobs fp32 [B, L], 0.0 at unscored
        columns): sum = the sequence log-probability, n_tokens = layout tokens + 1 (EOS), mean = sum / n_tokens."""
        if given not in ("caption", "image"):
            raise PlanGenError(f"score_layouts: given={given!r} must be 'caption' or 'image'")
        eos, eng = int(self.cfg.eos_id), self.engine
        lay = [self._layout_ids(g, strip_open=given == "caption") + [eos] for g in batch["gt_grounding"]]
        if given == "caption":
            prompts = [self.wrap_uni_prompt(c, "<grounding>", in_stage1=True)[1].tolist() for c in batch["base_caption"]]
            seqs = [p + l for p, l in zip(prompts, lay)]
            ids, _ = pad_input_ids(seqs, self.cfg.pad_id)
            L = ids.shape[1]
            lp = eng.score_text(ids, [L - len(q) for q in seqs], [L - len(l) for l in lay], position_mode=1, temperature=temperature)
        else:
            pin = batch["prepare_inputs_infer"]
            emb = self.vl_gpt.prepare_inputs_embeds(**{k: v for k, v in pin.items() if k != "attention_mask"})
            Lp = emb.shape[1]
            plen = [int(v) for v in pin["attention_mask"][:, :Lp].sum(-1)]
            L = max(p + len(l) for p, l in zip(plen, lay))
            embeds = torch.zeros((len(lay), L, emb.shape[2]), dtype=emb.dtype, device=emb.device)
            target = torch.full((len(lay), L), int(self.cfg.pad_id), dtype=torch.int32)
            embed = self.vl_gpt.language_model.get_input_embeddings()
            for i, (p, l) in enumerate(zip(plen, lay)):
                embeds[i, L - len(l) - p:L - len(l)] = emb[i, Lp - p:]
                embeds[i, L - len(l):] = embed(torch.tensor(l, dtype=torch.int32)).to(emb.dtype)
                target[i, L - len(l):] = torch.tensor(l, dtype=torch.int32)
            lp = eng.score_text_embeds(embeds, [L - p - len(l) for p, l in zip(plen, lay)], target, [L - len(l) for l in lay],
                                       position_mode=1, temperature=temperature)
        n_tok = [len(l) for l in lay]
        sums = lp.sum(-1).cpu().tolist()
        return dict(sum=sums, mean=[s / n for s, n in zip(sums, n_tok)], n_tokens=n_tok, logprobs=lp)

    @staticmethod
    def text_token_stats_summary(tokens: torch.Tensor, stats: dict, eos_id: int) -> dict:
        """Per row of a text decode with a stats request: the mean entropy over the row's own tokens (up to and including its EOS) and, with
        n_alt > 0, the alternatives' ids at each of them."""
        toks = tokens.cpu()
        count = [row.index(eos_id) + 1 if eos_id in row else len(row) for row in toks.tolist()]
        ent = stats["entropy"].float().cpu()
        s = dict(mean_entropy=[float(ent[i, :c].mean()) if c else 0.0 for i, c in enumerate(count)], n_tokens=count)
        if "alt_tok" in stats:
            alt = stats["alt_tok"].cpu()
            s["alt_tok"] = [alt[i, :c].tolist() for i, c in enumerate(count)]
        return s

    @staticmethod
    def select_best_layouts(tokens: torch.Tensor, logprobs: torch.Tensor, n: int, eos_id: int):
        """The layout_best_of rule.  tokens int64 [n * B, L] and logprobs fp32 [n * B, L] of one replicated stage-1 batch (row t * B + i =
        draw t of row i).  A row's score = sum of its log-probs (finished columns are 0.0) / the number of scored columns = up to and
        including its first EOS (L when it has none).  Per row the arg-max wins, ties -> the lowest t, -inf loses to any finite score.
        Returns (rows int64 [B], replica int64 [B], score fp32 [B])."""
        N, L = tokens.shape
        B = N // n
        is_eos = tokens == eos_id
        first = torch.where(is_eos.any(-1), is_eos.int().argmax(-1) + 1, torch.full((N,), L, device=tokens.device))
        total = logprobs.sum(-1) if L else logprobs.new_zeros((N,))
        score = total / first.clamp(min=1)
        rows, replica, scores = System.select_best_replicas(score.view(N, 1), n)
        return rows, replica, scores.gather(0, replica.view(1, B))[0]

    @torch.no_grad()
    def mmu_ask(self, batch: dict, questions: Sequence[dict], max_new_tokens: int = 512, min_new_tokens: int = 0) -> List[list]:
        """Several questions about the images of one mmu batch, with each row's prompt up to and including its image block prefilled ONCE.
        ``questions``: one ``prepare_inputs_infer``-style dict per question (input_ids [B, Lq] left-padded, images_seq_mask, attention_mask: what
        the mmu collate builds for that question; pixel_values / images_emb_mask are taken from ``batch['prepare_inputs_infer']``, the first
        question's).  Per row the columns in front of ``textproc.image_block_split`` must carry the same ids in every question.  Then per
        question: ``Engine.rewind`` to the prefix, ``Engine.extend`` with the question's tail tokens, and the text loop ``x2t`` is configured
        with (greedy, or text_temperature / text_top_k / text_top_p).  Returns one answer list per question: decoded texts with a codec, else
        the rows' new ids cut at EOS; the raw id tensors stay in ``self.last_ask_ids``."""
        from .textproc import cut_at_eos, image_block_split
        eng, dev = self.engine, self.device
        pin0 = dict(batch["prepare_inputs_infer"])
        qs = [dict(pin0, **{k: v for k, v in q.items() if k in ("input_ids", "images_seq_mask", "attention_mask")}) for q in questions]
        if not qs:
            return []
        end_id = None
        if self.codec is not None:
            from .textproc import IMAGE_END_TAG
            end_id = self.codec.token_id(IMAGE_END_TAG)
        B = qs[0]["input_ids"].shape[0]
        geo = []                                            # per question, per row: (pad, split, L)
        for q in qs:
            ids, L = q["input_ids"], q["input_ids"].shape[1]
            pad = Engine.pad_len_from_mask(q["attention_mask"], L)
            geo.append([(pad[r], image_block_split(q["images_seq_mask"][r].tolist(), ids[r].tolist(), end_id), L) for r in range(B)])
        for qi, q in enumerate(qs[1:], 1):
            for r in range(B):
                (p0, s0, _), (p1, s1, _) = geo[0][r], geo[qi][r]
                if s0 - p0 != s1 - p1 or not torch.equal(qs[0]["input_ids"][r, p0:s0].cpu(), q["input_ids"][r, p1:s1].cpu()):
                    raise PlanGenError(f"mmu_ask: row {r} of question {qi} differs from question 0 in front of the end of its image block")
        # the shared prefix, from question 0's embeddings (SigLIP + aligner run once), left-padded to the longest prefix
        emb0 = self.vl_gpt.prepare_inputs_embeds(**{k: v for k, v in qs[0].items() if k != "attention_mask"})
        plen = [s - p for p, s, _ in geo[0]]
        Lp = max(plen)
        pre = torch.zeros((B, Lp, self.cfg.hidden), dtype=emb0.dtype, device=emb0.device)
        for r, (p, s, _) in enumerate(geo[0]):
            pre[r, Lp - plen[r]:] = emb0[r, p:s]
        eng.prefill_embeds(pre, [Lp - n for n in plen], position_mode=1)
        self.vl_gpt.language_model.model.epoch += 1       # invalidates any sample_image cache token, like generate
        a = self.args
        temperature = float(getattr(a, "text_temperature", 0.0))
        answers, self.last_ask_ids = [], []
        embed = self.vl_gpt.language_model.get_input_embeddings()
        for qi, q in enumerate(qs):
            n_new = [L - s for _, s, L in geo[qi]]
            if min(n_new) < 1:
                raise PlanGenError(f"mmu_ask: question {qi} has a row with nothing behind its image block")
            tail = torch.full((B, max(n_new)), 0, dtype=torch.long)
            for r, (_, s, L) in enumerate(geo[qi]):
                tail[r, :n_new[r]] = q["input_ids"][r, s:L].cpu().clamp_min(0)
            if qi > 0:
                eng.rewind(plen)
            eng.extend(embeds=embed(tail.to(dev)), n_new=n_new)
            if temperature > 0:
                out = eng.generate_text(max_new_tokens, self.cfg.eos_id, min_new_tokens, temperature=temperature, top_k=int(getattr(a, "text_top_k", 0)),
                                        top_p=float(getattr(a, "text_top_p", 1.0)), seed=int(getattr(a, "seed", 0)))
            else:
                out = eng.generate_text_greedy(max_new_tokens, self.cfg.eos_id, min_new_tokens)
            self.last_ask_ids.append(out)
            rows = out.cpu().tolist()
            answers.append(self.decode_mmu_text_batch(rows) if self.codec is not None else [cut_at_eos(r, self.cfg.eos_id) for r in rows])
        return answers

    @torch.no_grad()
    def x2t(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
            max_new_tokens: int = 512, min_new_tokens: int = 0, temperature: Optional[float] = None,
            top_k: Optional[int] = None, top_p: Optional[float] = None, dfa=None, return_logprobs: bool = False,
            return_stats=False) -> torch.Tensor:
        """System.x2t (:513-523): text / layout-token decode.  Greedy like the reference unless ``text_temperature`` > 0 (argument,
        else self.args, else 0): then every row is sampled with ``text_top_k`` / ``text_top_p`` (HF order temperature -> top-k -> top-p)
        from seed = args.seed, the seed t2i uses.  The draw is keyed on the row's index in the batch, so two rows that carry the same
        prompt get different layouts: repeat a caption N times in one batch for N layouts of it.
        ``dfa`` (grammar.TokenDFA): the decode is constrained to the automaton's language, greedy or sampled (``layout_grammar``).
        return_logprobs: returns (tokens, fp32 [B, n] log-probabilities of the emitted tokens, 0.0 once a row has finished)."""
        a = self.args
        temperature = float(getattr(a, "text_temperature", 0.0)) if temperature is None else float(temperature)
        top_k = int(getattr(a, "text_top_k", 0)) if top_k is None else int(top_k)
        top_p = float(getattr(a, "text_top_p", 1.0)) if top_p is None else float(top_p)
        kw = dict(do_sample=False)
        if temperature > 0:
            kw = dict(do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p, seed=int(getattr(a, "seed", 0)))
        if dfa is not None:
            kw["dfa"] = dfa
        if return_logprobs:
            kw["return_logprobs"] = True
        if _stats_on(return_stats):                        # the stats dict over [B, n] comes back last
            kw["return_stats"] = return_stats
        return self.vl_gpt.language_model.generate(inputs_embeds=inputs_embeds, attention_mask=attention_mask,
                                                   pad_token_id=self.cfg.eos_id, bos_token_id=None,
                                                   eos_token_id=self.cfg.eos_id, max_new_tokens=max_new_tokens,
                                                   use_cache=True, min_new_tokens=min_new_tokens, **kw)
