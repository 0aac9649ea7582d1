# Keys of the reference's project/plangen/cfg/base.py that the layout->image path reads
# ("Config / flags"); everything training-related is intentionally absent.
seed = 0                               # base.py:3
janus_path = "models/Janus-Pro-1B"     # base.py:8,12  (HF safetensors directory; synthetic weights if missing)
system_cls_path = "project.plangen.plangen_base"
out_path = "out/plangen"
resume = "latest"                      # base.py:47: newest checkpoint-* under out_path, a path, or None
lora_alpha = None                      # base.py: lora_alpha of tuning_mode 'lora' (128 there; 'lora_ranni' trains with 16).  A LoRA checkpoint (lora_A / lora_B tensors) is merged into the weights at load time with scale lora_alpha / r; None: such a checkpoint is refused, the value is not in the file
lora_rank = None                       # base.py: lora_rank (256 there; 'lora_ranni' uses 64).  When set, checked against the rank found in the checkpoint
test = False
janus_hw = 384                         # base.py:83
parallel_size = 1                      # base.py:158
cfg_weight = 5.0                       # base.py:162
temperature = 1.0
top_k = 0                              # top-k filtering of sampled image tokens (0: off); an extension beyond the reference
top_p = 1.0                            # top-p (nucleus) filtering of sampled image tokens (1.0: off); an extension beyond the reference
text_temperature = 0.0                 # layout / caption decode (x2t): 0 = greedy like the reference; > 0 samples (an extension beyond the reference)
text_top_k = 0                         # top-k filtering of sampled text tokens (0: off)
text_top_p = 1.0                       # top-p (nucleus) filtering of sampled text tokens (1.0: off)
layout_grammar = False                 # True: the stage-1 layout decode (uni_2stage, plan) can only emit a well-formed layout string that ends inside max_new_tokens (an extension beyond the reference)
kv_dtype = 'bf16'                      # KV cache: 'bf16' = the compute dtype; 'fp8' = e4m3 codes + power-of-two scales (about half the cache bytes; an extension beyond the reference)
prefill_forced_prefix = False         # use_teacher_forcing: feed the image tokens in front of the first edited cell in one pass (Engine.extend) instead of one decode step each; same greedy tokens, sampled draws count RNG steps from the first decoded step
share_replicas = 0                     # parallel_size > 1: 1 = prefill every prompt once and let its replicas read its K/V in the decode loop (same tokens; an extension beyond the reference)
select_best = False                    # parallel_size > 1: score every replica by the mean log-probability of its image tokens, VQ-decode and keep only the best one per prompt (an extension beyond the reference)
layout_best_of = 1                     # uni_2stage / plan with text_temperature > 0: draw this many layouts per row and keep the one with the highest mean token log-probability (an extension beyond the reference)
score_gt_layout = False                # plan / uni_2stage / mmu: also write gt_layout_logprob = {sum, mean, n_tokens} per row to the batch JSON: log P(gt_grounding + EOS | caption) (mmu: | image) from one teacher-forced prefill (an extension beyond the reference)
score_gt_image = False                 # uni / uni_2stage: also write gt_image_logprob = {sum, mean, n_tokens} per row to the batch JSON: log P(VQ tokens of the ground-truth image | prompt) under the guided distribution (cfg_weight, temperature), from one teacher-forced prefill; with edit_region only the edited positions count (an extension beyond the reference)
token_stats = False                    # True, or an int n_alt in 1..8: per-token uncertainty from the decode loops, reduced on the device. uni / uni_2stage / t2i: image_token_stats (per image: mean entropy, mean rank, share of rank-0 positions; with use_teacher_forcing also top1 / top5 over edit_region == 0) in the batch JSON and <batch_idx>_entropy.npy fp32 [B * parallel_size, grid, grid]; plan / uni_2stage stage 1 / mmu: text_token_stats (per row: mean entropy, with n_alt > 0 the alternatives' ids) (an extension beyond the reference)
layout_attribution = False             # uni / uni_2stage (bf16): after generating, one more teacher-forced prefill on the generated tokens reports the attention the image positions put on every <ref>..</ref><box>..</box> item of the prompt: layout_attribution (per item: phrase, inside = share of its mass inside its own box) in the batch JSON and <batch_idx>_attribution.npy fp32 [B, items, grid, grid] (layer mean; NaN rows where a prompt has fewer items); the prompt capacity grows by the image's length (an extension beyond the reference)
use_centerhw = False                   # base.py:100: boxes are cx,cy,h,w instead of x1,y1,x2,y2 (read by layout_attribution's box cells)
# sample plans (an extension beyond the reference; all off by default, and then nothing changes): per-replica sampler parameters and per-step guidance in ONE batch
cfg_schedule = 'constant'              # 'constant' | 'linear' | 'cosine': the guidance weight runs from cfg_weight to cfg_weight_end over the image positions
cfg_weight_end = None                  # the schedule's last weight (None: the weight stays)
cfg_weights = None                     # list of length parallel_size: replica t of every prompt starts at cfg_weights[t] (with and without share_replicas)
same_noise = False                     # the replicas of a prompt share their RNG key: they differ by their plan only
cfg_weight_in_box = None               # positions whose cell centre lies in a box of the row's layout use this weight instead of the scheduled one
temperatures = None                    # per-replica lists like cfg_weights (temperature <= 0: that replica is greedy)
top_ks = None
top_ps = None
use_numhw_tokens = False               # base.py:65: add <h0> <w0> ... <h99> <w99> to the tokenizer (plangen_base.py:120-127)
use_special_tokens = False             # base.py:69: add <grounding> </grounding> <box> </box> <ref> </ref> to the tokenizer (plangen_base.py:110-118)
use_teacher_forcing = False            # base.py:36
use_neg_box = False                    # base.py:121
neg_prompt = ""                        # base.py:129: wrapped as wrap_uni_prompt(neg_prompt, '') for every uncond CFG row (:673)
neg_prompt_ids = None                  # optional pre-tokenised negative prompt (no tokenizer files needed)
max_new_tokens = 512                   # x2t (:513-523)
test_start = 0                         # base.py: skip batches before this index (:1135)
synthetic = False                      # True: seeded random-init weights + offline tokenizer (plumbing runs only)
max_test_len = 8                       # base.py:34: number of test batches
debug_max_seq_len = None               # base.py:135
dtype = "bf16"
test_batch_size = 8
test_data = dict(
    data_name="synthetic",             # 'synthetic' or the dataset tag used in the output path
    task_type="uni",                   # 't2i' | 'uni_2stage' | 'uni' | 'mmu' | 'plan'   (plangen_base.py:1112-1127)
    data_file=None,                    # JSONL: text rows (base_caption / gt_grounding / image_id) or pre-tokenised rows
)
