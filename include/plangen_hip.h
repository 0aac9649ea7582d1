/*
 * plangen_hip.h -- C ABI of the MI355X-native PlanGen layout->image generation path.
 *
 * The reference (360CVGroup/PlanGen) has no FFI of its own: its hot path is Python
 * calling torch/transformers.  The entry points below are the boundary SURVEY.md
 * section 8b defines: each replaces one Python-level call the reference's
 * ``System`` makes on ``self.vl_gpt`` (file:line cited per function, relative to the
 * reference tree).  The Python facade in ``plangen_amd/`` binds them with ctypes and
 * re-exposes the reference's call surface.
 *
 * Conventions
 *   - return 0 on success, negative pg_status on failure; never throws across the ABI;
 *     ``pg_last_error`` gives the message for the handle (or the global one for create).
 *   - "dev" pointers are device (HBM) memory owned by the caller (PyTorch-ROCm tensors);
 *     "host" pointers are small per-row metadata in host memory.
 *   - the library owns weights, KV cache and workspaces (hipMalloc at pg_create).
 *   - every call is asynchronous on the caller's hipStream_t; no hidden device syncs
 *     except where stated (pg_generate_text_greedy / _sampled poll the finished-flag; pg_prefill reads ONE
 *     4-byte flag back when it probes for a batch-constant negative prompt -- ONLY when the caller
 *     did not supply the answer through the one-shot ``uncond_shared_hint`` option (0 / 1): with
 *     the hint set, pg_prefill performs no device->host read and no stream synchronisation).
 *   - one handle per (process, GPU); a handle is not thread-safe.
 */
#ifndef PLANGEN_HIP_H
#define PLANGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pg_engine* pg_handle;
typedef void* pg_stream;              /* hipStream_t */

typedef enum { PG_F32 = 0, PG_BF16 = 1, PG_I32 = 2, PG_I64 = 3, PG_FP8_E4M3 = 4 /* pg_config.kv_dtype only */ } pg_dtype;

typedef enum {
    PG_OK = 0,
    PG_ERR_ARG = -1,        /* bad argument / shape */
    PG_ERR_HIP = -2,        /* HIP runtime error (message in pg_last_error) */
    PG_ERR_STATE = -3,      /* call out of order (e.g. decode before prefill) */
    PG_ERR_NAME = -4,       /* unknown tensor name */
    PG_ERR_CAPACITY = -5    /* exceeds rows / KV slots / images configured at create */
} pg_status;

#define PG_MAX_VQ_LEVELS 8

/* Shapes of the path.  Defaults for Janus-Pro-1B as used by PlanGen: SURVEY App. A. */
typedef struct pg_config {
    int32_t hidden, inter, n_layers, n_heads, head_dim;   /* 2048 5632 24 16 128 */
    int32_t vocab;                                        /* 102400 */
    int32_t img_vocab, img_dim, grid, gen_head_dim;       /* 16384 8 24 2048 */
    int32_t vq_ch, vq_levels, vq_ch_mult[PG_MAX_VQ_LEVELS], vq_z, vq_res_blocks; /* 128 5 {1,1,2,2,4} 256 2 */
    float   rms_eps, rope_theta;                          /* 1e-6 10000 */
    int32_t compute_dtype;   /* PG_BF16: bf16 weights/activations/KV, fp32 accumulate, fp32
                                residual stream and norm/softmax statistics (what
                                torch.autocast(bf16) does at plangen_base.py:360).
                                PG_F32 : everything fp32 (BASELINE config 1 / parity mode). */
    int32_t max_rows;        /* R capacity (2 x images for CFG) */
    int32_t max_prompt;      /* longest real prompt (tokens, without padding) */
    int32_t max_new;         /* decode capacity (576 image tokens, or text tokens) */
    int32_t max_images;      /* VQ decode batch capacity */
    int32_t with_lm_head;    /* allocate lm_head (text/layout decode, a11) */
    int32_t with_vq_encoder; /* allocate VQ encoder (a14) */
    /* SigLIP understanding encoder + aligner (a13, task_type='mmu'); siglip_large_patch16_384:
       width 1024, 24 layers, 16 heads (64 each), MLP 4096, patch 16, image 384 (siglip_vit.py:628-637) */
    int32_t with_vision, vit_width, vit_layers, vit_heads, vit_mlp, vit_patch, vit_img;
    int32_t max_vision_images;   /* images per pg_vision_encode call */
    int32_t kv_dtype;        /* 0 = compute dtype (default); PG_FP8_E4M3 = 4: the opt-in FP8 KV cache (below).  Zero-initialised
                                callers keep the compute-dtype cache and every result bit of it. */
} pg_config;

/* The FP8 KV cache (kv_dtype = PG_FP8_E4M3; compute_dtype must be PG_BF16, PG_F32 is PG_ERR_ARG at pg_create).
 * Every 128-element K row (after RoPE) and V row of a (row, head, slot) -- the bf16-rounded values the bf16 cache would
 * hold -- is stored as 128 one-byte codes and one fp32 scale, K and V separately:
 *   codes  OCP e4m3fn (the gfx950-native format, not MI300X fnuz), code = e4m3_rne(x * 2^-e), round to nearest even;
 *   scale  s = 2^e, e the smallest integer with amax(|x[0:128]|) * 2^-e <= 448, clamped to [-100, 100]; amax == 0: e = 0.
 * Power-of-two scales make x * 2^-e and code * 2^e exact in fp32 (no division, nothing that can round differently on host
 * and device), lose nothing against amax / 448 (e4m3's relative precision is the same in every binade) and keep the scaled
 * value at or below 448, so saturation never happens.  Quantisation is idempotent.  Non-finite K / V are not covered.
 * Prefill attention runs on the exact bf16 K / V (a one-layer bf16 scratch, quantised into the cache after each layer's
 * attention); a decode step attends to its own new key / value unquantised and appends their codes at its end; cached keys
 * are read as code * scale.  The K/V bytes a decode step streams drop to 264 / 512 of the bf16 cache's, the cache footprint
 * with them.  Results differ from the bf16 cache's (this is why the mode is in the config, not an option).  Not supported:
 * the "lanes" = 2 decode (PG_ERR_ARG at decode time). */

/* -- lifetime ------------------------------------------------------------------------ */
/* Replaces AutoModelForCausalLM.from_pretrained(...).cuda() (plangen_base.py:95). */
int pg_create(pg_handle* out, const pg_config* cfg, int device_id);
int pg_destroy(pg_handle h);
const char* pg_last_error(pg_handle h /* may be NULL */);

/* Load one tensor by its reference state_dict name (MultiModalityCausalLM keys,
 * modeling_vlm.py:190-219; a leading "vl_gpt." from PlanGen's .pth overlay,
 * base_system.py:153-155, is accepted).  ``src`` is HOST memory, dtype PG_F32 or PG_BF16.
 * Unknown-but-irrelevant names (vision_model.*, aligner.*, encoder when not configured)
 * return PG_ERR_NAME so the caller can count what it skipped. */
int pg_load_tensor(pg_handle h, const char* name, const void* src, int dtype,
                   const int64_t* shape, int ndim);
/* Merge one LoRA adapter pair into a weight that is already loaded:  W <- W + scale * B A  (peft's get_delta_weight with
 * scale = lora_alpha / r; dropout is the identity in eval mode), on the device, in the layout the weight already has.
 * ``weight_name`` is the BASE state_dict name of the weight (a leading "vl_gpt." is accepted); the targets are the seven
 * projections of every Llama layer: self_attn.{q,k,v,o}_proj.weight and mlp.{gate,up,down}_proj.weight.  ``a_host`` is
 * lora_A [r, in_features], ``b_host`` is lora_B [out_features, r], HOST memory, each PG_F32 or PG_BF16 (converted to fp32,
 * which is exact).  Per element, every operation rounded to fp32 on its own (no FMA), k ascending:
 *     acc = 0;  acc = acc + B[o][k] * A[k][i]  (k = 0 .. r - 1);   W[o][i] = T((float)W[o][i] + scale * acc)
 * with T the handle's compute type (bf16: round to nearest even).  A bf16 handle loaded from a bf16 checkpoint (what
 * Janus-Pro is) therefore holds ONE rounding of W + scale B A; a bf16 handle loaded from an fp32 source has rounded W once
 * before.  Non-finite inputs are not covered.
 * The weight is updated from its CURRENT contents: a second merge stacks on the first, pg_load_tensor of the base weight
 * starts it afresh.  There is no un-merge: load the base tensor again.  Synchronous (NULL stream, ends with a device
 * synchronisation) like pg_load_tensor, and like it the call un-finalizes the handle: call pg_finalize_weights afterwards,
 * which rebuilds the decode layouts from the merged weights.
 * PG_ERR_NAME: an unknown name or one that is not among the seven targets.  PG_ERR_STATE: the base weight was never loaded.
 * PG_ERR_ARG: a null pointer, a dtype other than PG_F32 / PG_BF16, out_features / in_features that are not the weight's
 * shape, r < 1 or r > 1024, a scale that is not finite.  Nothing is launched on a refusal and the handle stays usable. */
int pg_merge_lora(pg_handle h, const char* weight_name,
                  const void* a_host, int a_dtype, const void* b_host, int b_dtype,
                  int out_features, int in_features, int r, float scale);
/* After all tensors: build derived tables (gen_embed->gen_aligner table, L2-normalised
 * codebook -> post_quant_conv table, RoPE cos/sin).  ``missing`` (may be NULL) receives the
 * number of required tensors never loaded. */
int pg_finalize_weights(pg_handle h, int* missing, pg_stream s);

/* -- language-model path ---------------------------------------------------------------- */
/* Replaces the first call of  vl_gpt.language_model.model(inputs_embeds=embed(ids),
 * attention_mask=mask, use_cache=True)  (plangen_base.py:548,571-577) for a LEFT-padded
 * batch.  ids_dev int32 [R, L]; pad_len_host int32 [R] = number of leading pad slots of
 * each row (mask==0 prefix, plangen_base.py:711-712).  Pad slots are skipped (SURVEY App.
 * B-9).  position_mode 0: RoPE position of slot j = j (absolute slot index incl. padding,
 * what sample_image gets because it passes no position_ids, App. B-1); 1: position =
 * j - pad_len (HF generate: mask.cumsum-1).  Resets the KV cache. hidden_out_dev (may be
 * NULL) receives last_hidden_state in ``hidden_dtype`` laid out [R, L, hidden] (pad slots
 * zero). */
int pg_prefill(pg_handle h, const int32_t* ids_dev, const int32_t* pad_len_host, int R, int L,
               int position_mode, void* hidden_out_dev, int hidden_dtype, pg_stream s);
/* pg_prefill of ``replicas`` copies of one CFG batch -- t2i's  tokens = torch.cat([tokens] * parallel_size)  (plangen_base.py:547)
 * followed by the first language_model.model call -- with every distinct prompt prefilled ONCE.  ids_dev int32 [R0, L] and
 * pad_len_host [R0] are the UN-replicated, left-padded, CFG-interleaved batch, exactly what pg_prefill takes.  Afterwards the handle
 * is in the state of pg_prefill(R = R0 * replicas rows, position_mode 0, no hidden output) of the replicated ids: row t * R0 + r is
 * replica t of row r (the reference's [all pairs] x p layout), and pg_decode_image_tokens* / pg_step run on R rows.  Only the rows
 * that own a prompt are packed and run through the layer stack: owner(row) = the shared negative prompt's row for odd rows when the
 * negative prompt is shared (decided as pg_prefill decides it on the R replicated rows: share_uncond, uncond_shared_hint, the device
 * probe; R0 = 2 with replicas = 2 qualifies), else row % R0; a row with owner(row) != row takes its first hidden state from its owner.
 *   alias = 1: a replica's prompt slots [0, len) are NEVER written; the decode attention reads them from the owner row (grouped
 *              form of the fused decode-attention kernels) with cached loads, so that the replicas of a prompt are served from one
 *              copy in L2 (measured at 128 rows, 4 replicas: L2 misses of the launch x0.37, decode loop -2.6 % at L = 256 and -9.5 % at
 *              L = 512; DESIGN 4.5, profiles/replica_compare.md).  Slots from
 *              len on (the replica's own decode keys) live in its own cache row.  pg_debug_read("kcache" / "vcache" / "kscale" /
 *              "vscale") of a replica's prompt slots returns unspecified bytes.  lanes = 2 is rejected at decode time (PG_ERR_ARG).
 *   alias = 0: the A/B fallback: the same single prefill, then one copy kernel writes the owner's prompt K/V (FP8 cache: codes and
 *              both scales) into every replica's own row, and the decode loop runs exactly the kernels it runs after pg_prefill.
 * Both modes give the same bits (equality-tested on the GPU).  The cache footprint is not reduced: all R rows stay allocated.
 * replicas = 1 is exactly pg_prefill(h, ids_dev, pad_len_host, R0, L, 0, NULL, PG_F32, s).
 * PG_ERR_ARG: replicas < 1, R0 < 1, alias not 0 / 1, or a handle without the fused decode attention; PG_ERR_CAPACITY:
 * R0 * replicas > max_rows.  pg_generate_text_* after it (replicas > 1): PG_ERR_STATE (image-sampling positions). */
int pg_prefill_replicated(pg_handle h, const int32_t* ids_dev, const int32_t* pad_len_host, int R0, int L,
                          int replicas, int alias, pg_stream s);
/* Same, from caller-provided embeddings [R, L, hidden] (dtype PG_F32/PG_BF16): the
 * ``emb is not None`` branch of t2i (plangen_base.py:543-545) and x2t (:513). */
int pg_prefill_embeds(pg_handle h, const void* embeds_dev, int embeds_dtype,
                      const int32_t* pad_len_host, int R, int L, int position_mode,
                      void* hidden_out_dev, int hidden_dtype, pg_stream s);

/* Continue the cached sequences with many tokens in one pass (HF: a second  model(inputs_embeds=[R, n, H], past_key_values=...)  call).
 * cur[r] is the number of K/V slots row r holds: its prompt length plus the decode steps run since (pg_step, or T - 1 / the steps a
 * pg_decode_image_tokens* / pg_generate_text_* loop ran: the token a loop emitted LAST was never fed back and is not in the cache).
 * Exactly one of ids_dev int32 [R, Lx] / embeds_dev [R, Lx, hidden] (PG_F32 or PG_BF16) is given, R = the rows of the preceding
 * prefill.  The first n_new_host[r] columns of row r are its new tokens (LEFT-aligned; columns past them are ignored).  New token i of
 * row r takes slot cur[r] + i and RoPE position pos_off[r] + cur[r] + i -- the position rule the preceding prefill chose (position_mode)
 * -- and attends to slots 0 .. cur[r] + i of its own row.  Only the new tokens go through the GEMMs.  Afterwards row r has length
 * cur[r] + n_new_host[r], the step counters are zero, the input of the first gen_head / lm_head is the final-norm hidden state of each
 * row's last new token, hidden_out_dev (may be NULL) holds all of them as [R, Lx, hidden] in hidden_dtype (unused columns zero), and
 * every decode entry point continues exactly as after a prefill of the longer sequences; a decode call (pg_decode_image_tokens*,
 * pg_generate_text_*, pg_step) whose steps would leave the KV slots (max_prompt + max_new) or the RoPE table is PG_ERR_CAPACITY (host
 * checks that cannot fire after a plain prefill, whose own limits imply them).  Asynchronous on ``s``: n_new_host travels through pinned staging like pad_len_host.
 * bf16 handles run the query-offset form of the 128-query flash kernel (flash_prefill = 0 and PG_F32 handles: the generic kernel).
 * Nothing is launched on a refusal and the handle stays usable:
 *   PG_ERR_STATE     before a prefill; after pg_prefill_replicated with replicas > 1; when the batch shares its negative prompt (it
 *                    lives in row 1's slots, which the prefill attention kernels do not follow: prefill with the one-shot
 *                    pg_set_option("uncond_shared_hint", 0));
 *   PG_ERR_ARG       an FP8 KV handle (past keys exist only as codes); n_new_host[r] outside [1, Lx]; both or neither input pointer; a
 *                    dtype other than PG_F32 / PG_BF16; a pending pg_request_attn_spans (consumed by this call, which cannot serve it);
 *   PG_ERR_CAPACITY  cur[r] + n_new_host[r] exceeds the KV slots, the last position exceeds the RoPE table, or sum n_new_host exceeds
 *                    the packed-token capacity max_rows * max_prompt. */
int pg_prefill_extend(pg_handle h, const int32_t* ids_dev /*[R, Lx] or NULL*/, const void* embeds_dev /*[R, Lx, hidden] or NULL*/,
                      int embeds_dtype, const int32_t* n_new_host /*[R]*/, int Lx, void* hidden_out_dev /*[R, Lx, hidden] or NULL*/,
                      int hidden_dtype, pg_stream s);
/* Cut row r back to its first len_host[r] slots, 1 <= len_host[r] <= cur[r] (else PG_ERR_ARG); e.g. back to the prompt after
 * pg_generate_text_*, whose early-finished rows hold EOS filler.  Zeroes the step counters and recomputes the longest-first row order;
 * launches only small copies.  Slots past the new length keep stale keys and are never read.  The hidden state the next sample is drawn
 * from is NOT recomputed: a pg_prefill_extend follows before anything samples, and until it has, pg_decode_image_tokens* and
 * pg_generate_text_* answer PG_ERR_STATE (pg_step, whose input is the caller's, is allowed).  Refuses the same handle states as
 * pg_prefill_extend. */
int pg_rewind(pg_handle h, const int32_t* len_host /*[R]*/, pg_stream s);

/* One decode step behind  language_model.model(inputs_embeds=[R,1,H], past_key_values=...)
 * (plangen_base.py:571-577, i>0): consumes embeds_dev [R, hidden], appends K/V, writes
 * last_hidden_state [R, hidden] (after the final RMSNorm) to hidden_out_dev. */
int pg_step(pg_handle h, const void* embeds_dev, int embeds_dtype, void* hidden_out_dev,
            int hidden_dtype, pg_stream s);

/* vl_gpt.gen_head(h) (modeling_vlm.py:47-51; call site plangen_base.py:579):
 * h_dev [R, hidden] -> logits_dev fp32 [R, img_vocab]. */
int pg_gen_head(pg_handle h, const void* h_dev, int h_dtype, float* logits_dev, int R, pg_stream s);

/* vl_gpt.prepare_gen_img_embeds(tok) (modeling_vlm.py:270-271; plangen_base.py:603):
 * tok_dev int32 [R] -> out_dev [R, hidden]. */
int pg_gen_embed(pg_handle h, const int32_t* tok_dev, void* out_dev, int out_dtype, int R, pg_stream s);

/* language_model.get_input_embeddings()(ids) (plangen_base.py:371,548): ids int32 [n]. */
int pg_embed_tokens(pg_handle h, const int32_t* ids_dev, void* out_dev, int out_dtype, int n, pg_stream s);

/* The whole System.sample_image loop (plangen_base.py:567-607) on device after a
 * pg_prefill of R = 2B CFG-interleaved rows: T steps of {layer stack, gen_head, CFG mix
 * (:580-587), sample (:588-591), gen_embed+gen_aligner feedback (:602-604)}.
 * temperature <= 0: greedy argmax, ties -> lowest index (parity mode);
 * > 0: sample softmax(logits/temperature) by the Gumbel-max trick with a counter-based
 * RNG keyed on (seed, image, step).
 * force_tok_dev  int32 [B, T] or NULL: token fed back instead of the sampled one
 *     (teacher-forced parity protocol); with force_mask_dev uint8 [B, T] != NULL it is the
 *     reference's use_teacher_forcing branch (:593-598): where mask==0 the emitted AND
 *     fed-back token is force_tok (gt label), elsewhere the model's own.
 * out_tok_dev    int32 [B, T]: emitted tokens.
 * logits_out_dev fp32 [T, B, img_vocab] or NULL: CFG-mixed logits per step (tests). */
int pg_decode_image_tokens(pg_handle h, int T, float cfg_weight, float temperature, uint64_t seed,
                           const int32_t* force_tok_dev, const uint8_t* force_mask_dev,
                           int32_t* out_tok_dev, float* logits_out_dev, pg_stream s);
/* pg_decode_image_tokens with top-k / top-p (nucleus) filtering of the sampled draw (an extension
 * beyond the reference; HF generate order temperature -> top-k -> top-p).  Per image and step,
 * x = mixed / temperature:
 *   top_k > 0:      keep v iff #{u : x_u > x_v} < top_k (ties at the k-th value all kept;
 *                   top_k >= V keeps everything); top_k == 0: off.
 *   0 < top_p < 1:  on softmax(x) over the top-k survivors, keep v iff the mass of survivors
 *                   with a strictly larger x is < top_p (ties at the boundary all kept; the top
 *                   token always kept); top_p == 1: off.
 * The token is drawn from softmax(x) over the kept set by the same Gumbel-max noise as
 * pg_decode_image_tokens, so when the unfiltered draw survives the filter the filtered draw
 * equals it.  NaN counts as -inf; -inf is never kept; if nothing is kept token 0 is emitted.
 * temperature <= 0 (greedy) ignores top_k / top_p.  Forcing is unchanged (filters apply to the
 * model's own draw only).  (top_k, top_p) = (0, 1) is exactly pg_decode_image_tokens.
 * top_k < 0, top_p <= 0, top_p > 1 or NaN: PG_ERR_ARG, nothing launched.  The filtered
 * sampler needs img_vocab <= 16384. */
int pg_decode_image_tokens_filtered(pg_handle h, int T, float cfg_weight, float temperature, int32_t top_k, float top_p,
                                    uint64_t seed, const int32_t* force_tok_dev, const uint8_t* force_mask_dev,
                                    int32_t* out_tok_dev, float* logits_out_dev, pg_stream s);
/* Dual guidance (an extension beyond the reference; the decomposed form of InstructPix2Pix): the image loop of
 * pg_decode_image_tokens_filtered over THREE rows per image, after a pg_prefill of R = 3B rows interleaved as
 *   row 3b     = f: the full prompt (caption + layout)
 *   row 3b + 1 = p: the caption alone
 *   row 3b + 2 = u: the negative prompt
 * with, per image, step and vocabulary entry, in fp32,
 *   mixed = (u + w_caption * (p - u)) + w_layout * (f - p).
 * Everything behind the mixed row -- greedy / Gumbel-max draw keyed on (seed, global image, step), top-k / top-p, forcing,
 * the logits tap [T, B, img_vocab], the token fed back to all three rows -- is pg_decode_image_tokens_filtered's, with
 * B = R / 3.  Two degenerate cases hold bit for bit against the pair loop on the same logits: p == f gives
 * u + w_caption * (f - u), p == u gives u + w_layout * (f - u); w_caption == w_layout == w is ordinary CFG up to rounding.
 * One-shot pg_request_token_logprobs / pg_request_token_stats are honoured (capacity B * T, B = R / 3).  An FP8 KV
 * cache is allowed.  Refused, nothing launched: R % 3 != 0 (PG_ERR_ARG); a prefill that shared the negative prompt
 * across odd rows (PG_ERR_STATE: prefill with the one-shot pg_set_option("uncond_shared_hint", 0)); replicas that alias
 * their owner's prompt (PG_ERR_STATE); lanes = 2 (PG_ERR_ARG); a pending pg_request_sample_plan (PG_ERR_ARG; the plan
 * is consumed); non-finite weights, top_k / top_p out of range (PG_ERR_ARG); filtering with img_vocab > 16384
 * (PG_ERR_CAPACITY); and every state pg_decode_image_tokens refuses. */
int pg_decode_image_tokens_dual(pg_handle h, int T, float w_caption, float w_layout, float temperature, int32_t top_k,
                                float top_p, uint64_t seed, const int32_t* force_tok_dev, const uint8_t* force_mask_dev,
                                int32_t* out_tok_dev, float* logits_out_dev, pg_stream s);

/* language_model.generate(inputs_embeds=..., do_sample=False, max_new_tokens=...,
 * eos_token_id=pad_token_id=eos) (System.x2t, plangen_base.py:513-523) after a
 * pg_prefill*(position_mode=1) of B rows: greedy argmax(lm_head(h[:, -1])), finished rows
 * emit eos, stops when every row is finished.  out_dev int64 [B, max_new]; *out_len_host =
 * number of columns produced (new tokens only).  min_new suppresses EOS for the first
 * min_new steps (benchmark workload).  Synchronises the stream every few steps to read
 * the all-finished flag. */
int pg_generate_text_greedy(pg_handle h, int max_new, int min_new, int eos_id, int64_t* out_dev,
                            int* out_len_host, pg_stream s);
/* language_model.generate(..., do_sample=True, temperature=, top_k=, top_p=): the same loop with a
 * sampled token (an extension beyond the reference, whose x2t is greedy).  HF's order: min_new EOS
 * suppression -> temperature -> top-k -> top-p -> draw.  Per row and step, on
 * x = logits / temperature (formed as logits * (1 / temperature) in fp32):
 *   top_k > 0     : keep v iff fewer than top_k entries are strictly larger (ties at the k-th
 *                   value all kept; top_k >= vocab keeps all); top_k == 0: off.
 *   0 < top_p < 1 : on softmax(x) over the top-k survivors keep v iff the mass of survivors with
 *                   a strictly larger x is < top_p (boundary ties kept; the top token always
 *                   kept); top_p == 1: off.
 * The token is the Gumbel-max over the kept set, with the noise expression of the image sampler
 * keyed on (seed, global row = row + the "rng_image_offset" option, step): a draw that survives
 * the filter equals the unfiltered draw for the same key; a row's tokens depend on neither the
 * other rows of the batch nor on how a batch is split over handles.  Two rows with the same
 * prompt have different global rows and draw different texts.  NaN counts as -inf; -inf is never
 * kept; EOS while step < min_new is -inf before the filters; nothing kept: token 0.
 * temperature <= 0 is pg_generate_text_greedy bit for bit (same kernels, same launches; top_k /
 * top_p ignored).  Finished rows emit eos and the loop stops when every row is finished, as there.
 * All five values live in device memory: a captured step graph replays with new ones.
 * top_k < 0, top_p <= 0, top_p > 1 or NaN: PG_ERR_ARG, nothing launched.
 * logits_out_dev: fp32 [max_new, B, vocab] or NULL (tests): the logits each emitted token was
 * drawn from, after EOS suppression, before temperature; steps the loop did not run stay untouched. */
int pg_generate_text_sampled(pg_handle h, int max_new, int min_new, int eos_id, float temperature, int32_t top_k,
                             float top_p, uint64_t seed, int64_t* out_dev, int* out_len_host,
                             float* logits_out_dev, pg_stream s);

/* Grammar-constrained text decode: a finite automaton over TOKENS masks the logits of every step,
 * so a row can only spell a sentence of the automaton's language and is certain to finish inside its
 * budget (plangen_amd/grammar.py builds the layout language's automaton over a tokenizer).
 *   token_class_host [vocab]             class of every token id, 0 .. n_classes-1
 *   next_state_host  [n_states, n_classes]  next state, or -1: a token of this class is not allowed here
 *   dist_host        [n_states]          fewest further tokens (the EOS included) until the row can
 *                                        finish; >= 2^30: it cannot finish from here
 * pg_set_text_dfa validates on the host, before anything is launched (PG_ERR_ARG: n_states outside
 * 1..4096, n_classes outside 1..1024, start_state or a class id or a next state out of range, a negative
 * dist, or a state with 0 < dist < 2^30 from which no class that holds a token leads to a state with
 * dist <= its own - 1: the promise the budget rule rests on), then copies the tables through pinned
 * staging on s without synchronising the stream.  The device buffers are allocated once, at those
 * limits, by the first upload (counted by pg_device_bytes; that one call also waits for the buffers'
 * zero fill on the NULL stream): a captured step graph keeps valid addresses and replays with whatever
 * automaton was uploaded last.  dfa == NULL forgets the automaton.
 * The tables do not say which token is EOS, so one property is the builder's to keep: a state with
 * dist == 0 is entered by eos_id only (grammar.py's automata do).  A hand-made automaton that lets
 * another token into such a state is accepted, but its rows may reach column max_new - 1 without EOS. */
typedef struct pg_text_dfa {
    const int16_t* token_class_host;
    const int16_t* next_state_host;
    const int32_t* dist_host;
    int32_t n_states, n_classes, start_state;
} pg_text_dfa;
int pg_set_text_dfa(pg_handle h, const pg_text_dfa* dfa /* NULL: forget it */, pg_stream s);
/* pg_generate_text_sampled under the automaton.  Every row starts in start_state.  Per row and step,
 * with remaining = max_new - step (this step counted), token v is ALLOWED in state st iff
 *   nx = next_state[st][token_class[v]] >= 0   and   dist[nx] <= remaining - 1
 * (the budget rule: a row only moves to states it can still finish from; dist[start_state] <= max_new is
 * checked, PG_ERR_ARG otherwise, so every unfinished row emits EOS no later than column max_new - 1,
 * given the property above).
 * Disallowed logits become -inf BEFORE temperature, top-k and top-p (where HF applies logits processors
 * and where the min_new EOS suppression sits); the draw is then exactly pg_generate_text_sampled's: same
 * noise keyed on (seed, row + "rng_image_offset", step), same filter rule, lowest index on ties;
 * temperature <= 0 is the masked argmax.  Nothing kept (every allowed logit -inf or NaN): the row emits
 * eos_id, finishes and keeps its state (not token 0, which could lie outside the language).  An unfinished
 * row's state becomes next_state[state][token_class[tok]] once its token is chosen; a finished row keeps
 * its state and emits eos.  There is no min_new: the automaton says where EOS may stand.
 * state_out_dev int32 [B] or NULL: the final states.  logits_out_dev fp32 [max_new, B, vocab] or NULL:
 * each step's row after the mask (disallowed entries -inf).  PG_ERR_STATE: no automaton set, and
 * whatever pg_generate_text_sampled answers so; PG_ERR_ARG: top_k / top_p as there; PG_ERR_CAPACITY:
 * max_new as there.  The handle stays usable after every error.  pg_generate_text_greedy / _sampled
 * ignore the automaton: same launches, same bits, and scan kernels whose instruction streams are
 * unchanged (the automaton is a template parameter that is off for them). */
int pg_generate_text_constrained(pg_handle h, int max_new, int eos_id, float temperature, int32_t top_k, float top_p,
                                 uint64_t seed, int64_t* out_dev, int* out_len_host, int32_t* state_out_dev /*[B] or NULL*/,
                                 float* logits_out_dev, pg_stream s);

/* Token log-probabilities: how likely the model found every token a decode loop emitted (HF's output_scores /
 * compute_transition_scores), reduced on the device next to the sampler: one float per row and step instead of the logits_out tap.
 * A row is an image of the CFG loop or a sequence of the text loop.  Per row and step, with tok the EMITTED token and y the fp32 row
 * the draw is made from, before top-k and top-p:
 *   image loop  y = u + w (c - u), bit for bit what logits_out_dev receives;
 *   text loop   y = the reduced lm_head row after the min_new EOS suppression and after the automaton's mask (disallowed entries
 *               -inf), bit for bit what logits_out_dev receives;
 *   x = y * (1 / temperature) when temperature > 0 (the fp32 product the draw uses), else x = y; NaN counts as -inf;
 *   logprob = (x[tok] - m) - logf(sum_v expf(x_v - m)),  m = max_v x_v,  all fp32 with the accurate expf / logf.
 * top-k and top-p do NOT renormalise it (scores of runs with different filters stay comparable); the automaton's mask and the EOS
 * ban do, because they change which tokens exist.  x[tok] = -inf gives -inf (a forced token on a masked entry; the "nothing kept"
 * emission of token 0 / eos_id), and so does a row without a finite entry; when m = +inf the mass lies evenly on the +inf entries.
 * Forcing: tok is what out_tok_dev receives.  With force_mask_dev it is force_tok where mask == 0 -- force_mask = zeros is the SCORING
 * MODE: the log-likelihood of a given image under the model; with force_tok_dev alone the emitted token is the model's own, and so
 * is the score.  Text: a row that was finished BEFORE a step gets 0.0 there, so that a row's sum is its sequence log-probability; the
 * step that emits its EOS is scored like any other.
 * pg_request_token_logprobs is ONE-SHOT: the request is consumed by the next pg_decode_image_tokens[_filtered] /
 * pg_generate_text_{greedy,sampled,constrained} on this handle, whether that call succeeds or not, and that call also writes
 * out_dev fp32 [B, T] (image loop) or [B, max_new] (text loop; columns >= *out_len_host are left untouched).  out_dev must stay valid
 * until that call's work on the stream is done.  Inside the loop the scores go to a library-owned buffer (allocated by the first
 * request, counted by pg_device_bytes) and are copied to out_dev at the end, as the tokens are; a captured step graph is re-captured
 * when a call's request differs from the capture's.  A call without a request launches exactly what it launched before this
 * entry point existed.  out_dev == NULL cancels a pending request.
 * PG_ERR_ARG: capacity_floats < 1 here; at the consuming call, nothing launched and the handle still usable: capacity_floats below
 * B * T / B * max_new, or the "lanes" = 2 decode. */
int pg_request_token_logprobs(pg_handle h, float* out_dev, int64_t capacity_floats);

/* Per-token uncertainty: what else the model was considering where a decode loop emitted a token.  Rows, y, x = y * (1 / temperature)
 * (NaN as -inf), tok and the forcing rules are those of pg_request_token_logprobs above; top-k and top-p renormalise nothing, the EOS
 * ban and the automaton's mask do (a masked entry is -inf in y and is never an alternative).  Per row and step, all fp32 with the
 * accurate expf / logf, m = max_v x_v, s = sum_v expf(x_v - m), t = sum_v expf(x_v - m) (x_v - m) (an entry -inf adds 0 to both):
 *   logprob      (x[tok] - m) - logf(s): bit for bit what pg_request_token_logprobs writes for the same call;
 *   entropy      H = logf(s) - t / s of softmax(x), in nats (>= 0 up to rounding; log V for a flat row);
 *   rank         #{v : x_v > x[tok]}, exact: 0 says the emitted token was the mode;
 *   alt_tok      the n_alt largest x_v, descending, the lowest index first among equals, exact;
 *   alt_logprob  (x_v - m) - logf(s) of each alternative (alt_logprob[0] is the logprob a token alt_tok[0] would have got).
 * A row without a finite entry: H = 0, rank = V_row (the row's length), logprob -inf.  m = +inf: the mass lies evenly on the k entries
 * +inf, H = logf(k).  A token outside the row or on a -inf entry: rank = V_row.  Fewer than n_alt entries above -inf: the missing
 * places hold alt_tok = -1, alt_logprob = -inf.  Text: a row that was finished BEFORE a step gets logprob 0, entropy 0, rank 0,
 * alt_tok -1, alt_logprob 0 there; columns >= *out_len_host are left untouched.
 * The arrays are [B, T] (image loop) or [B, max_new] (text loop), the alt_* ones [.., n_alt]; a NULL pointer skips that output. */
typedef struct pg_token_stats {
    float*   logprob_dev;
    float*   entropy_dev;
    int32_t* rank_dev;
    int32_t* alt_tok_dev;        /* [.., n_alt] */
    float*   alt_logprob_dev;    /* [.., n_alt] */
    int32_t  n_alt;              /* 0..8 */
    int64_t  capacity;           /* positions (B * T, B * max_new) every non-NULL array can hold */
} pg_token_stats;
/* ONE-SHOT like pg_request_token_logprobs and independent of it: the request (copied here) is consumed by the next
 * pg_decode_image_tokens[_filtered] / pg_generate_text_{greedy,sampled,constrained} on this handle, whether that call succeeds or
 * not; both requests may be pending for one call, and then their logprob arrays hold the same bits.  The arrays must stay valid
 * until that call's work on the stream is done.  Inside the loop one more 1024-thread block per row reduces the stored row (the route
 * pg_request_token_logprobs uses) into a library-owned buffer (allocated by the first request, counted by pg_device_bytes), copied
 * out at the end; a captured step graph is re-captured when a call's request differs from the capture's.  A call without a request
 * launches exactly what it launched before this entry point existed.  req == NULL cancels a pending request.
 * PG_ERR_ARG (nothing launched, the handle still usable): here, n_alt outside 0..8, capacity < 1, n_alt > 0 with exactly one of
 * the two alt_* pointers, all five pointers NULL; at the consuming call, capacity below B * T / B * max_new, or the "lanes" = 2
 * decode. */
int pg_request_token_stats(pg_handle h, const pg_token_stats* req);

/* -- sample plans: per-image sampler parameters, per-(image, step) guidance ---------------------
 * A sample plan replaces the scalar sampler parameters of the NEXT pg_decode_image_tokens[_filtered] by per-image values; the guidance
 * weight is per image AND per step.  For the global image bg (local image + the lane's first image) at step t:
 *   mixed = u + w[bg, t] * (c - u)              fp32, the expression of the unplanned sampler; logits_out_dev and the stored row the
 *                                               log-prob / stats reducers read receive exactly this value;
 *   temperature[bg] <= 0                        the image is greedy: lowest index on ties, its top_k / top_p ignored; greedy and sampled
 *                                               images may share a call;
 *   temperature[bg] > 0                         Gumbel-max over mixed * (1 / temperature[bg]) with the noise of (seed, key[bg] * 1000003 + t,
 *                                               v), restricted to the kept set of (top_k[bg], top_p[bg]) by the rule of
 *                                               pg_decode_image_tokens_filtered.  Two images with the same key and seed draw the same noise.
 * The filtered route (store, select, pick) is taken when any image of the plan is sampled with top_k > 0 or top_p < 1; an image with
 * (0, 1.0) draws there exactly what the unfiltered sampler draws.  The log-prob and stats requests use temperature[bg].  A NULL array
 * stands for the call's scalar (image_key: bg + "rng_image_offset"), so a plan whose arrays are constant and equal to the call's scalars
 * gives the bits of the call without a plan: tokens, logits_out, log-probs and stats.  Forcing (force_tok, force_mask) is unchanged.
 * The arrays are HOST arrays, validated and copied here (pinned staging on s guarded by an event, no stream synchronisation; the consuming call's stream
 * waits on that event, so s need not be the stream of that call) into a
 * library-owned device copy sized by max_rows / 2 and max_new (allocated by the first request, counted by pg_device_bytes).  The
 * values reach the kernels through device memory: a captured step graph replays with a new plan, its key only gains "a plan is present".
 * A call without a plan launches exactly what it launched before this entry point existed. */
typedef struct pg_sample_plan {
    const float*   cfg_weight_host;   /* [B, T] or NULL: the call's scalar */
    const float*   temperature_host;  /* [B]    or NULL */
    const int32_t* top_k_host;        /* [B]    or NULL */
    const float*   top_p_host;        /* [B]    or NULL */
    const int32_t* image_key_host;    /* [B]    or NULL: global image index used in the RNG stream key instead of
                                         b + "rng_image_offset"; two images with the same key and seed draw the same noise */
    int32_t B, T;                     /* must equal the consuming call's images and steps */
} pg_sample_plan;
/* ONE-SHOT, with the rules of pg_request_token_logprobs: the next pg_decode_image_tokens[_filtered] on the handle consumes it, whether
 * or not that call succeeds; independent of the log-prob and stats requests (all three may be pending for one call); the text loops
 * neither consume nor see it.  plan == NULL forgets a pending plan.
 * PG_ERR_ARG here (nothing pending afterwards): B or T < 1, a non-finite weight or temperature, top_k < 0, top_p outside (0, 1] or NaN,
 * a negative key (key * 1000003 + T fits the 64-bit stream word for every int32 key >= 0), all five pointers NULL.  PG_ERR_CAPACITY
 * here: B > max_rows / 2 or T > max_new.  PG_ERR_ARG at the consuming call (nothing launched, the handle still usable): B / T differ
 * from the call's, the "lanes" = 2 decode, a filtered image with img_vocab > 16384. */
int pg_request_sample_plan(pg_handle h, const pg_sample_plan* plan /* NULL: forget it */, pg_stream s);

/* -- attention mass on prompt spans ------------------------------------------------------------
 * What output_attentions=True would be reduced to, without the [R, heads, W, W] tensor: for one layer, query column q_i and span s of
 * row r,
 *   A[r, i, s] = (1 / n_heads) * sum_h  sum_{k in span(r, s), k <= q_i, k a real token}  softmax_k( scale * Q[r,h,q_i] . K[r,h,k] ),
 * the softmax over ALL real keys k <= q_i of the row (the prefill attention's causal and left-pad rule: slots 0 .. len[r), slot =
 * column - pad_len[r]), scale = 1 / sqrt(128), Q / K the RoPE'd bf16 tensors the prefill attention of that layer reads.  The queries
 * are the n_q columns from q_col0, the same for every row; span(r, s) = [lo, hi) in columns of the padded [R, L] frame.  A query column
 * inside a row's padding gives zeros; an empty span (hi <= lo) gives zeros; a span that reaches into the padding or past the query
 * counts only the real keys <= q_i; spans may overlap.  A partition of [0, L) sums to 1 on every real query.
 * Arithmetic (attn_span.hip): scores by bf16 MFMA with fp32 accumulation, the scale applied to the FP32 score (the attention kernel
 * itself rounds a pre-scaled Q to bf16: its probabilities differ from these in the last bf16 bits of q), running maximum and sum per
 * query in fp32 with __expf, the span sum by one more MFMA against the 0/1 span matrix with P split into hi + lo bf16 halves (relative
 * 2^-17), rescaled when the maximum rises; the head mean is a fixed-order fp32 sum inside one block, so two calls give the same bits.
 * rows must be the R of the consuming call (the struct carries it because the host arrays are copied when the request is made). */
typedef struct pg_attn_spans {
    const int32_t* span_lo_host;  /* [rows * n_spans] columns */
    const int32_t* span_hi_host;  /* [rows * n_spans] */
    int32_t rows;                 /* = R of the prefill that serves it */
    int32_t n_spans;              /* 1..16 */
    int32_t q_col0, n_q;          /* reported queries: columns [q_col0, q_col0 + n_q) */
    uint64_t layer_mask;          /* bit l = report layer l; non-zero, within n_layers */
    float* out_dev;               /* fp32 [popcount(layer_mask)][R][n_q][n_spans], layers ascending */
    int64_t capacity_floats;
} pg_attn_spans;
/* ONE-SHOT in front of the NEXT pg_prefill / pg_prefill_embeds on this handle, like pg_request_token_logprobs: consumed by that call
 * whatever it answers; req == NULL forgets a pending request.  The host arrays are copied here; out_dev must stay valid until that
 * call's work on the stream is done.  The serving prefill launches one more kernel (and a memset of the layer's block) after the
 * attention of every selected layer -- flash or not -- and, with kv_dtype = PG_FP8_E4M3, reads the bf16 scratch K the prefill attention
 * itself reads, before it is quantised: the FP8 handle returns the bf16 handle's bits.  A shared negative prompt is not shared in that
 * call (every row keeps its own Q and K).  A prefill without a pending request launches exactly what it launched before.
 * PG_F32 handles REFUSE the request at the prefill (the kernel is bf16; no fallback).
 * PG_ERR_ARG, here (nothing pending afterwards): a null pointer, rows outside 1..max_rows, n_spans outside 1..16, q_col0 < 0, n_q < 1,
 * layer_mask zero or naming a layer >= n_layers, capacity_floats < 1.  At the consuming call, before anything is launched (the
 * prefill does not happen, nothing stays pending): PG_ERR_ARG when rows != R, q_col0 + n_q > L, a span bound outside [0, L], a
 * PG_F32 handle, or the call is pg_prefill_replicated (only owner rows are packed there); PG_ERR_CAPACITY when capacity_floats <
 * popcount(layer_mask) * R * n_q * n_spans. */
int pg_request_attn_spans(pg_handle h, const pg_attn_spans* req /* NULL: forget it */);

/* -- scoring given text ---------------------------------------------------------------------
 * log softmax(lm_head(hidden))[target] for n chosen rows of a hidden-state tensor, logits never materialised: the evaluation half of
 * pg_request_token_logprobs.  hidden_dev [rows, hidden] in the compute dtype (hidden_dtype must say so) -- typically what pg_prefill /
 * pg_prefill_embeds wrote to hidden_out_dev, viewed as [R * L, hidden]; row_idx_dev int32 [n] names the rows to score (NULL: rows
 * 0 .. n-1), target_dev int32 [n] the token each is scored on:
 *   y_v = sum_k hidden[row_idx[i]][k] * lm_head[v][k]   (fp32 accumulation; operands in the compute dtype),
 *   x = y * (1 / temperature) when temperature > 0 (the rounded fp32 product of pg_request_token_logprobs), else x = y,
 *   logprob[i] = (x[t] - m) - logf(sum_v expf(x_v - m)),  m = max_v x_v,  t = target[i];  t outside [0, vocab) gives -inf.
 * Non-finite hidden states or weights are NOT covered (the NaN-as--inf rule of the sampling loops is not reproduced).
 * PG_BF16 handles run one fused kernel over the vocabulary (MFMA tiles of 256 rows x 256 columns, running maximum and sum of
 * exponentials per row in registers) and a small merge kernel; the only HBM traffic besides the operands is a library-owned partials
 * workspace of 8 * G * n bytes (G column groups, a function of (n, vocab, hidden) alone), allocated on first use, grown on demand
 * (growing frees the old one) and counted by pg_device_bytes.  A row's bits depend on its hidden row, lm_head, its target, the
 * temperature and (n, vocab, hidden) only -- not on its slot in the batch nor on the other rows.  PG_F32 handles (parity mode) compose
 * the f32 GEMM and the scoring kernel of pg_op_token_logprob over row chunks whose logits stay <= 64 MB (same workspace rule).
 * Asynchronous on s, no synchronisation; the sequence state of the handle is not touched.  hidden must be a multiple of 64 (the
 * kernel's K step).  row_idx entries outside [0, rows) are the caller's fault: they are never read on the host.
 * PG_ERR_STATE: a handle without lm_head (with_lm_head = 0) or before pg_finalize_weights.  PG_ERR_ARG: a null pointer, n < 1, rows < 1,
 * hidden_dtype != compute dtype, hidden % 64 != 0, row_idx_dev == NULL with n > rows.  After an error the handle stays usable. */
int pg_score_tokens(pg_handle h, const void* hidden_dev, int hidden_dtype /* = compute dtype */, int64_t rows,
                    const int32_t* row_idx_dev /*[n] or NULL*/, const int32_t* target_dev /*[n]*/, int64_t n,
                    float temperature, float* logprob_dev /*[n]*/, pg_stream s);

/* -- scoring given images ---------------------------------------------------------------------
 * The image-side counterpart of pg_score_tokens: the log-probability of given image tokens under the GUIDED distribution the image
 * sampler draws from, for n positions of a hidden-state tensor, without the 576-step loop and without logits in HBM.  hidden_dev
 * [rows, hidden] in the compute dtype (hidden_dtype must say so) -- typically what pg_prefill_embeds(position_mode = 0) wrote to
 * hidden_out_dev for [prompt | image embeddings], viewed as [R * L, hidden].  Position i names its conditional row cond_idx_dev[i], its
 * unconditional row uncond_idx_dev[i] (both int32 [n], indices into the rows of hidden_dev; the two lists may name the same row, and one row
 * may serve many positions) and the image token target_dev[i] it is scored on:
 *   g       = GELU_erf(hidden . W1^T + b1) in the compute dtype        (gen_head layer 1, as pg_gen_head / the decode loop leave it),
 *   yc_v    = sum_k g[cond_idx[i]][k] * W2[v][k] + b2[v],  yu_v likewise with uncond_idx[i]   (fp32 accumulation),
 *   y_v     = yu_v + cfg_weight * (yc_v - yu_v)                         (fp32; the sampler's expression),
 *   x       = y * (1 / temperature) when temperature > 0 (the rounded fp32 product of pg_request_token_logprobs), else x = y,
 *   logprob[i] = (x[t] - m) - logf(sum_v expf(x_v - m)),  m = max_v x_v,  t = target[i];  t outside [0, img_vocab) gives -inf.
 * Non-finite hidden states or weights are NOT covered.
 * Layer 1 runs over ALL ``rows`` rows of hidden_dev (one large-M GEMM with the bias and the GELU in its epilogue; no compaction: pass
 * only the rows worth a GEMM row); its output [rows, gen_head_dim] lives in the library-owned scoring workspace.  PG_BF16 handles then run
 * one fused kernel: 256 x 256 MFMA tiles that hold 128 (cond, uncond) pairs, the mix and a running maximum and sum of exponentials per
 * pair in registers, and a small merge kernel; besides the operands it moves 8 * G * n bytes of partials (G column groups, a function
 * of (n, img_vocab, gen_head_dim) alone).  A position's bits depend on its two hidden rows, the weights, its target, cfg_weight, the
 * temperature and (n, img_vocab, gen_head_dim) only -- not on its slot nor on the other positions.  PG_F32 handles (parity mode)
 * compose the f32 GEMM, a mix kernel and the scoring kernel of pg_op_token_logprob over chunks of pairs whose logits stay <= 64 MB.
 * The workspace is the one of pg_score_tokens: allocated on first use, grown on demand (growing frees the old one), counted by
 * pg_device_bytes.  Asynchronous on s, no synchronisation; the sequence state of the handle is not touched.  Index entries outside
 * [0, rows) are the caller's fault: they are never read on the host.
 * PG_ERR_STATE: before pg_finalize_weights.  PG_ERR_ARG: a null pointer, n < 1 or n > 2^29, rows < 1 or rows * max(hidden, gen_head_dim)
 * >= 2^31, hidden_dtype != compute dtype.  After an error the handle stays usable. */
int pg_score_image_tokens(pg_handle h, const void* hidden_dev, int hidden_dtype /* = compute dtype */, int64_t rows,
                          const int32_t* cond_idx_dev /*[n]*/, const int32_t* uncond_idx_dev /*[n]*/, const int32_t* target_dev /*[n]*/,
                          int64_t n, float cfg_weight, float temperature, float* logprob_dev /*[n]*/, pg_stream s);

/* -- VQ-16 tokenizer ---------------------------------------------------------------------- */
/* gen_vision_model.decode_code(codes, shape=[B,8,g,g]) (vq_model.py:505-508; call site
 * plangen_base.py:555): codes_dev int32 [B, g*g] -> img_out_dev [B, 3, S, S] (NCHW like the
 * reference), S = g * 2^(levels-1). */
int pg_vq_decode(pg_handle h, const int32_t* codes_dev, void* img_out_dev, int out_dtype, int B, pg_stream s);
/* gen_vision_model.encode(x)[-1][-1] (vq_model.py:494-498; plangen_base.py:532):
 * img_dev [B,3,S,S] -> idx_out_dev int64 [B*g*g]. */
int pg_vq_encode(pg_handle h, const void* img_dev, int img_dtype, int64_t* idx_out_dev, int B, pg_stream s);

/* -- understanding encoder ------------------------------------------------------------------ */
/* aligner(vision_model(images)) of MultiModalityCausalLM.prepare_inputs_embeds
 * (modeling_vlm.py:243-250): CLIPVisionTower.forward (clip_encoder.py:107-122) ->
 * VisionTransformer.forward_features (siglip_vit.py:562-572; no cls token, learned pos-embed,
 * LayerNorm eps 1e-6, non-causal MHA, GELU MLP) -> MlpProjector mlp_gelu (projector.py:38-44).
 * img_dev [B,3,S,S] -> out_dev [B, (S/patch)^2, hidden].  The masked scatter into the text
 * embeddings (modeling_vlm.py:263-266) is data movement done by the caller. */
int pg_vision_encode(pg_handle h, const void* img_dev, int img_dtype, void* out_dev, int out_dtype, int B, pg_stream s);

/* -- image pre-processing for the understanding path -------------------------------------------- */
/* VLChatProcessor.image_processor of the mmu path (VLMImageProcessor, three_party/Janus/janus/models/image_processing_vlm.py:41-52,127-192,
 * reached through hack_image_proc, plangen_base.py:99-101,136-147) on the device.  The resample is Pillow's 8-bit fixed-point bicubic
 * (torchvision's resize of a PIL image is PIL.Image.resize(BICUBIC); libImaging/Resample.c), so the result equals Pillow +
 * transformers bit for bit.
 *   input   B images, each uint8 RGB, HWC, in device memory, with its own pointer, height, width and row stride in BYTES (images_host
 *           is a host array; sizes differ within a batch; rows need not be contiguous or aligned).
 *   size    m = max(h, w); oh = max((int)(h / m * S), min_size), ow likewise, in double, in that order (:137-143): 64 x 97 at
 *           S = 48 is 31 x 48.
 *   coeffs  precompute_coeffs + normalize_coeffs_8bpc per image and axis: scale = in / out, fs = max(scale, 1), support = 2 fs; for
 *           output xx: c = (xx + 0.5) scale, xmin = max((int)(c - support + 0.5), 0), n = min((int)(c + support + 0.5), in) - xmin,
 *           w_x = bicubic((x + xmin - c + 0.5) * (1 / fs)) with a = -0.5, summed in ascending x, each divided by the sum,
 *           k = (int)(w * 2^22 +- 0.5) (half away from zero).  Computed on the device in fp64 with contraction off by a kernel in
 *           front of the resample: no host tables, and the doubles are the ones x86 computes.
 *   passes  horizontal first, then vertical; a pass whose size does not change is skipped.  One value = clamp((2^21 + sum pixel * k)
 *           >> 22, 0, 255) in int32 with an arithmetic shift; the image between the passes is uint8 (its rounding is part of the result).
 *   pad     the resized image is pasted at ((S - ow) / 2, 0) or (0, (S - oh) / 2) into an S x S canvas of ``background`` (expand2square).
 *   values  every uint8 v of channel c becomes lut_host[c * 256 + v] (fp32; the caller fills it with transformers' rescale + normalize
 *           arithmetic, so any mean / std are exact by construction); PG_BF16 output is the round-to-nearest-even of that fp32 value
 *           (the .to(torch.bfloat16) of modeling_vlm.py:249).
 *   output  out_dev [B, 3, S, S] NCHW, PG_F32 or PG_BF16; every element is written, the padding included.
 * Asynchronous on ``s``, no synchronisation: descriptors and table travel through pinned staging like pg_prefill's pad_len_host; the
 * library-owned workspace (coefficient tables + uint8 intermediates) is allocated on first use, grows when a batch needs more (growing
 * frees the old one, which waits for work that still uses it) and is counted by pg_device_bytes.  Calls on one handle must be ordered on
 * one stream.  Works on any handle (no weights needed).
 * PG_ERR_ARG, nothing launched: a null pointer (handle, images_host, an image's pix_dev, background, lut_host, out_dev), B < 1, an image
 * side < 1, min_size < 1, S < min_size, S > 16384, a down-scaling ratio in / out above 64 on an axis (caps the taps per output at 257
 * and the workspace with it), out_dtype other than PG_F32 / PG_BF16. */
typedef struct pg_image_u8 { const uint8_t* pix_dev; int32_t height, width; int64_t row_stride; } pg_image_u8;
int pg_preprocess_images(pg_handle h, const pg_image_u8* images_host, int B, int out_size, int min_size,
                         const uint8_t background[3], const float* lut_host /* [3][256] */,
                         void* out_dev, int out_dtype, pg_stream s);

/* -- introspection (tests / bench) -------------------------------------------------------- */
/* Last-launch timing of the decode loop measured with HIP events on ``s`` inside the
 * library: fills ms for the whole pg_decode_image_tokens call and, when per-kernel
 * timing was enabled with pg_set_option("time_attn", 1), the summed duration and launch
 * count of the decode-attention kernel. */
typedef struct pg_timing {
    float  decode_ms;          /* whole last pg_decode_image_tokens */
    float  attn_ms_sum;        /* sum over timed decode-attention launches */
    int32_t attn_launches;
    double attn_bytes_sum;     /* algorithmic K/V bytes those launches had to read */
    float  prefill_ms;         /* whole last pg_prefill* */
    float  vq_ms;              /* whole last pg_vq_decode */
} pg_timing;
int pg_get_timing(pg_handle h, pg_timing* out);
/* Per-kernel-class sums of the last instrumented decode loop (pg_set_option("time_attn", 1); call pg_get_timing
 * first: it collects the events).  cls 0..8: decode attention, QKV / O / gate|up(+SwiGLU) / down GEMMs, RMSNorm
 * (+ split-K reduce + residual), gen_head, CFG sampler, 8: event pairs around nothing (instrumentation overhead); *bytes_sum = algorithmic HBM bytes of the timed launches
 * (weights once per launch; K/V once per launch).  Returns PG_ERR_ARG past the last class. */
int pg_get_class_timing(pg_handle h, int cls, const char** name, double* ms_sum, int* launches, double* bytes_sum);
/* Switches of the product library (defaults in parentheses), PER HANDLE.  NONE changes what a handle returns: they are measurement taps,
 * per-call hints, and A/B fallbacks that produce the same results (each is equality-tested on the GPU).  Experiments that lost their
 * measurement were removed in round 5; kernel-variant tables, timing ablations and the "decode step without attention" measurement
 * mode live in a SEPARATE library (libplangen_diag.so: pg_diag_set_option, pg_bench_*; csrc/diag_api.hip) that this header does not cover.
 *   measurement
 *     time_attn (0)          per-launch HIP events around every decode kernel class (eager loop) -> pg_get_timing / pg_get_class_timing
 *     time_stride (1)        ... on every n-th decode step only
 *   per-call hints
 *     rng_image_offset (0)   global index of this handle's image 0: prompt-sharded ranks sample exactly what one big batch would
 *     uncond_shared_hint     ONE-SHOT, consumed by the next pg_prefill: 1 = the caller has compared the ids on the host (its collate built
 *                            them, plangen_base.py:672-686 replicates one negative prompt) and every odd row equals row 1 -> no device
 *                            probe, pg_prefill does not synchronise; 0 = they differ; -1 (default) = probe on the device (one 4-byte
 *                            read + stream sync)
 *     allow_partial_weights (0)  run although required tensors were never loaded (they read as zeros)
 *   decode loop
 *     share_uncond (1)       prefill / store a batch-constant negative prompt once (0: every uncond row keeps a private copy)
 *     use_graph (0)          replay the decode step as a hipGraph (one launch per step from the host; env PG_USE_GRAPH=1).  Off by
 *                            default: same-stream launches of the ~175 kernels of a step measure 1-3 % faster than graph replay
 *     lanes (1)              2: two row-range lanes on two streams (measured 6 % slower at bs=64; kept as a documented fallback)
 *     stream_gemm (-1 auto)  bit mask of the decode GEMM classes on the v4 kernel (x tile by LDS-DMA): 1 wide-N slabs, 2 narrow-N slabs,
 *                            4 SwiGLU gate|up, 8 the M <= 16 kernels, 16 SwiGLU through the LDS-transposed epilogue; 0 = v3 everywhere;
 *                            128 = v3 wide-N blocks of 64 columns / 4 waves instead of 128 columns / 8 waves
 *     split_target_big (128) decode split-K block-count target at >= 96 rows (per-handle isolation is tested with it)
 *   prefill
 *     flash_prefill (1)      MFMA flash attention for prefill (0: per-query streaming kernel)
 *     prefill_attn (2)       MFMA prefill attention: 2 = 128 queries per block, K/V by LDS-DMA, V through the LDS transpose read; 1 = 64-query kernel
 *     prefill_rope_epi (1)   QKV projection: RoPE + KV-cache write in the 256x256 GEMM's epilogue when the packed batch takes that kernel
 *                            (plangen_base.py:571 -> LlamaAttention.forward); 0 = GEMM -> fp32 q|k|v -> RoPE / KV-fill kernel.  Same bits.
 *     prefill_res_epi (1)    o_proj / down_proj: residual add in the GEMM epilogue; 0 = fp32 slab folded in by the norm kernel.  Same bits.
 *     gemm256 (1)            256x256 MFMA GEMM for large shapes (0: 128x128 kernel everywhere; 4 / 5 / 6 pin the tile height to 256 / 224 / 192 rows
 *                            instead of choosing it per launch; +8 = four phases per K tile instead of two).  Bit-identical results in every form.
 *   VQ-16
 *     conv_halo (1)          direct halo-tile 3x3 convolution for Cin=Cout=128 (2: lock-step variant with the generic epilogue and the one-patch conv_out, 0: implicit-GEMM kernel)
 *     vq_mid_bf16 (1)        bf16 mode: the tensor between a ResnetBlock's two convolutions is bf16 (statistics from the fp32
 *                            accumulators); 0 keeps it fp32 like the skip stream
 *     vq_tail_fused (0)      1 = decoder tail conv_out(swish(norm_out(h))) (vq_model.py:210-214) in one pass over the fp32 skip stream instead of a GroupNorm
 *                            apply pass + conv_out.  Bit-identical pixels; measured slower in round 6 (4.05 vs 3.4 ms at 64 images), hence off.
 *     vq_argmin_multi (1)    nearest-code search: 8 latent vectors per block (0: one per block); identical indices
 *   SigLIP
 *     vit_attn (2)           2 = K / V^T of a head resident in LDS, 16 waves per block; 4 / 8 / 12 / 16 = that kernel with so many waves;
 *                            1 = the 64-key tile kernel of rounds 2-3 (bit-identical results)
 *     ln_wave (1)            LayerNorm (width 1024): wave-per-row register kernel; 0 = block-per-row kernel
 * Returns PG_ERR_ARG for an unknown key. */
int pg_set_option(pg_handle h, const char* key, int64_t value);
/* Bytes of device memory the handle owns (weights + KV + workspace). */
int64_t pg_device_bytes(pg_handle h);
/* Debug taps for parity tests: copy an internal buffer to dst_dev.
 * name: "kcache"/"vcache" (layer in ``index``; compute dtype [max_rows, heads, slots, 128] -- with the FP8 KV cache the uint8 codes of
 * the same shape, and "kscale"/"vscale" return the scales as fp32 [max_rows, heads, slots]), "x" (residual stream), "xn", "hfin", "gen_table", "pq_table", "qbuf", "obuf",
 * "vit_feat" (SigLIP features of the last pg_vision_encode, after the final LayerNorm, compute dtype [B, P, vit_width]),
 * "score_mid" (gen_head layer-1 output of the last pg_score_image_tokens, compute dtype [rows, gen_head_dim]; PG_ERR_NAME once another
 * scoring call has reused the workspace), "len" (int32 [max_rows]: the rows' lengths as the last prefill / pg_prefill_extend / pg_rewind
 * set them) and "n_dec" (int32 [1]: decode steps run since; len[r] + n_dec = the K/V slots row r holds). */
int pg_debug_read(pg_handle h, const char* name, int index, void* dst_dev, int64_t max_bytes, pg_stream s);

/* Stand-alone operator entry points (unit parity tests call these through the ABI;
 * the engine uses the same kernels internally). All tensors device memory. */
int pg_op_rmsnorm(pg_handle h, float* x_dev /*[M,H] in/out*/, const float* partial_dev /*[S,M,H]|NULL*/,
                  int S, const void* w_dev /*compute dtype [H]*/, void* out_dev /*compute dtype [M,H]*/,
                  int M, int H, float eps, pg_stream s);
int pg_op_gemm(pg_handle h, const void* a_dev /*[M,K]*/, const void* w_dev /*[N,K]*/, float* out_dev /*[S,M,N]*/,
               int M, int N, int K, int force_kind /*0 auto,1 skinny,2 big,3 f32,4 skinny on the tiled decode copy of W*/,
               int* S_out, pg_stream s);
/* The decode gate|up GEMM with SwiGLU in its epilogue (transformers LlamaMLP: down(silu(gate(x)) * up(x))):
 * a_dev bf16 [M,K]; wgu_dev bf16 [2I,K] with gate/up rows interleaved in blocks of 8 (rows 16j..16j+7 = gate rows
 * 8j..8j+7, rows 16j+8..16j+15 = the matching up rows: the engine's internal layout); h_out_dev bf16 [M,I]. */
int pg_op_swiglu_gemm(pg_handle h, const void* a_dev, const void* wgu_dev, void* h_out_dev, int M, int I, int K, pg_stream s);
/* The sampler's RNG output stage: raw 64-bit generator outputs bits_dev [n] -> out_dev fp32 [2n] =
 * (uniform u in (0,1) | Gumbel noise -log(-log u)) exactly as cfg_scan_kernel computes them. */
int pg_op_uniform(pg_handle h, const uint64_t* bits_dev, float* out_dev, int n, pg_stream s);
/* The top-k / top-p selection of pg_decode_image_tokens_filtered on caller-given rows:
 * logits_dev fp32 [B, V] (V <= img_vocab, <= 16384) -> keep_dev uint8 [B, V] = 1 where the entry
 * is in the kept set of x = logits / temperature (same rule and device code).  temperature > 0. */
int pg_op_sample_filter(pg_handle h, const float* logits_dev /*[B,V]*/, int B, int V, float temperature, int top_k,
                        float top_p, uint8_t* keep_dev /*[B,V]*/, pg_stream s);

/* The selection and draw of pg_generate_text_sampled on caller-given rows (same device code):
 * logits_dev fp32 [B, V], 1 <= V <= vocab -> keep_dev uint8 [B, V] (or NULL) = 1 where the entry is
 * in the kept set, tok_dev int32 [B] (or NULL) = the token drawn for key (seed, row + row_offset,
 * step).  temperature > 0. */
int pg_op_text_sample(pg_handle h, const float* logits_dev /*[B,V]*/, int B, int V, float temperature, int top_k,
                      float top_p, uint64_t seed, int row_offset, int step, uint8_t* keep_dev /*[B,V]*/,
                      int32_t* tok_dev /*[B]*/, pg_stream s);

/* One step of pg_generate_text_constrained on caller-given rows and states (same device code; the uploaded
 * automaton): logits_dev fp32 [B, V] (16-byte aligned), 1 <= B <= max_rows, 1 <= V <= vocab, state_dev int32 [B]
 * (a state outside [0, n_states) allows nothing) -> tok_dev int32 [B] = the token for key (seed, row + row_offset,
 * step), eos_id when nothing was kept; next_state_dev int32 [B] (may be state_dev); keep_dev uint8 [B, V] or NULL
 * = 1 where the entry is allowed, above -inf and inside the top-k / top-p kept set.  temperature <= 0: masked argmax.
 * PG_ERR_STATE without an automaton. */
int pg_op_text_constrain(pg_handle h, const float* logits_dev /*[B,V]*/, int B, int V, const int32_t* state_dev /*[B]*/,
                         int remaining, int eos_id, float temperature, int top_k, float top_p, uint64_t seed,
                         int row_offset, int step, uint8_t* keep_dev /*[B,V] or NULL*/, int32_t* tok_dev /*[B]*/,
                         int32_t* next_state_dev /*[B]*/, pg_stream s);

/* The scoring kernel of pg_request_token_logprobs on caller-given rows (same device code): x_dev fp32 [B, V] (the row y above; any
 * B >= 1, V >= 1), tok_dev int32 [B], temperature as above -> logprob_dev fp32 [B].  A token outside [0, V) gives -inf.  Works on
 * any handle.  PG_ERR_ARG: a null pointer, B < 1, V < 1. */
int pg_op_token_logprob(pg_handle h, const float* x_dev, int B, int V, const int32_t* tok_dev, float temperature,
                        float* logprob_dev, pg_stream s);

/* The reducer of pg_request_token_stats on caller-given rows (same device code): x_dev fp32 [B, V] (the row y; any B >= 1, V >= 1, any
 * 4-byte alignment), tok_dev int32 [B], temperature as above -> the arrays of out ([B] and [B, n_alt]; capacity >= B; a NULL pointer
 * skips that output).  logprob equals pg_op_token_logprob on the same inputs bit for bit.  Works on any handle.  PG_ERR_ARG: a null
 * x_dev / tok_dev / out, B < 1, V < 1, and what pg_request_token_stats refuses. */
int pg_op_token_stats(pg_handle h, const float* x_dev, int B, int V, const int32_t* tok_dev, float temperature,
                      const pg_token_stats* out, pg_stream s);

/* The device code of pg_score_tokens on caller-given weights: x_dev [rows, K], w_dev [V, K] row-major, both in the handle's compute
 * dtype; any n >= 1 and V >= 1, K a positive multiple of 64.  Works on any handle.  PG_ERR_ARG as pg_score_tokens. */
int pg_op_head_logprob(pg_handle h, const void* x_dev, int64_t rows, const void* w_dev, int V, int K,
                       const int32_t* row_idx_dev, const int32_t* target_dev, int64_t n, float temperature,
                       float* logprob_dev, pg_stream s);

/* The head of pg_score_image_tokens (everything after layer 1) on caller-given operands: x_dev [rows, K] and w_dev [V, K] row-major in the
 * handle's compute dtype, bias_dev fp32 [V] or NULL (no bias); any n >= 1 and V >= 1, K a positive multiple of 64.  Works on any handle.
 * PG_ERR_ARG: a null pointer (bias_dev excepted), n < 1 or n > 2^29, rows < 1, V < 1, K not a positive multiple of 64. */
int pg_op_cfg_head_logprob(pg_handle h, const void* x_dev, int64_t rows, const void* w_dev, int V, int K, const float* bias_dev /*[V] or NULL*/,
                           const int32_t* cond_idx_dev, const int32_t* uncond_idx_dev, const int32_t* target_dev, int64_t n,
                           float cfg_weight, float temperature, float* logprob_dev, pg_stream s);

/* The quantiser of the FP8 KV cache (the device code the decode append and the prefill conversion run; format above):
 * x_dev bf16 [n, 128] -> codes_dev uint8 [n, 128] (e4m3fn), scale_dev fp32 [n] (powers of two).  Works on any handle. */
int pg_op_kv_quantize(pg_handle h, const void* x_dev /*bf16 [n,128]*/, uint8_t* codes_dev /*[n,128]*/, float* scale_dev /*[n]*/,
                      int64_t n, pg_stream s);

/* The kernel of pg_request_attn_spans on caller-provided device arrays, one layer (semantics above): q_dev packed bf16
 * [tokens][nh * 128] (row r's slot j at token row_off[r] + j; row_off[r] < 0: the row has no tokens and gives zeros), k_dev bf16
 * [R][nh][slots][128], row_off_dev / len_dev / pad_len_dev int32 [R], span_lo_dev / span_hi_dev int32 [R][n_spans] (columns),
 * out_dev fp32 [R][n_q][n_spans] (every element is written).  len[r] <= slots and the extent of q_dev are the caller's.
 * PG_ERR_ARG: a null pointer, a PG_F32 handle, R outside 1..65535, nh / slots / n_q < 1, q_col0 < 0, n_spans outside 1..16. */
int pg_op_attn_span_mass(pg_handle h, const void* q_dev, const void* k_dev, const int32_t* row_off_dev, const int32_t* len_dev,
                         const int32_t* pad_len_dev, const int32_t* span_lo_dev, const int32_t* span_hi_dev, int R, int nh, int slots,
                         int n_spans, int q_col0, int n_q, float scale, float* out_dev, pg_stream s);

/* 3x3 convolution over NHWC activations (compute dtype), the VQ-16 ResnetBlock / Upsample /
 * Downsample conv (vq_model.py:337-352, :417-427, :440-447).  w_dev is [Cout][9][Cin]
 * (tap-major, the engine's internal layout), bias fp32; up=1 folds a nearest-2x upsample of
 * the input in; stride2=1 is the encoder's pad-(0,1,0,1) stride-2 form. */
int pg_op_conv3x3(pg_handle h, const void* x_dev, const void* w_dev, const float* bias_dev, const void* residual_dev,
                  void* out_dev, int B, int Hi, int Wi, int Cin, int Cout, int up, int stride2, pg_stream s);
/* GroupNorm(32, eps=1e-6) (+ optional swish) over NHWC activations (vq_model.py:393-403):
 * x_dev fp32 (the VQ skip stream is kept in fp32), out_dev compute dtype. */
int pg_op_groupnorm(pg_handle h, const void* x_dev, const float* gamma_dev, const float* beta_dev, void* out_dev, int B,
                    int HW, int C, int swish, pg_stream s);

#ifdef __cplusplus
}
#endif
#endif /* PLANGEN_HIP_H */
