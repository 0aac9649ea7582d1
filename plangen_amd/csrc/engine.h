// Host side of libplangen_hip.so: the engine behind include/plangen_hip.h (struct pg_engine; member functions in engine_core.hip =
// create / weights, engine_llm.hip = prefill / decode loop / text decode, engine_vq.hip = VQ-16 decoder + encoder, engine_vision.hip =
// SigLIP + aligner, engine_api.hip = the C ABI).  One engine per (process, GPU).  Owns weights (converted to the compute dtype and to
// the layouts the kernels want), the KV cache [layer][K|V][row][head][slot][128], workspaces, and the decode-step hipGraph.  No torch
// types anywhere: plain pointers and sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/plangen_hip.h"
#include "kernels.h"

#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) {                                                                          \
            char _b[512];                                                                                \
            snprintf(_b, sizeof _b, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            this->err = _b;                                                                              \
            return PG_ERR_HIP;                                                                           \
        }                                                                                                \
    } while (0)
#define FAIL(code, ...)                       \
    do {                                      \
        char _b[512];                         \
        snprintf(_b, sizeof _b, __VA_ARGS__); \
        this->err = _b;                       \
        return code;                          \
    } while (0)
#define TRY(expr)                  \
    do {                           \
        int _rc = (expr);          \
        if (_rc != PG_OK) return _rc; \
    } while (0)

enum SlotKind { K_T = 0, K_F32, K_IL16_G, K_IL16_U, K_CONV };
struct Slot {
    void* dst = nullptr; SlotKind kind = K_T; long n = 0;
    int a = 0, b = 0, c = 0;
    bool loaded = false;
    std::vector<int64_t> shape;       // expected state_dict shape (empty: only the element count is checked)
};
struct ConvW { void* w = nullptr; float* b = nullptr; int cin = 0, cout = 0, k = 3; };
struct NormW { float* g = nullptr; float* b = nullptr; int c = 0; };
struct ResBlockW { NormW n1, n2; ConvW c1, c2, nin; bool has_nin = false; };
struct AttnW { NormW n; ConvW q, k, v, p; };
struct VqLevel { std::vector<ResBlockW> res; std::vector<AttnW> attn; ConvW resample; bool has_resample = false; };
struct LinW { void* w = nullptr; float* b = nullptr; int out = 0, in = 0; };
struct VitBlockW { NormW n1, n2; LinW qkv, proj, fc1, fc2; };
struct VqNet { ConvW conv_in; ResBlockW mid0, mid2; AttnW mid1; std::vector<VqLevel> levels; NormW norm_out; ConvW conv_out; };

// The rows one chain of launches works on: the row-indexed workspaces already offset to its first row, its own split-K slab buffer and step
// counter, where its rows sit in the KV cache, and the (S, slab) pair its last GEMM left in ``part`` for the kernel that folds the reduction in.
// A plain value built by pg_engine::view and passed down by reference: nothing it describes is engine state, so nothing has to be put back.
struct DecodeView {
    int r0 = 0, rows = 0;             // first row (also the offset into h_len) and row count
    float* x; void *xn, *qbuf, *obuf, *hbuf, *hfin, *gh_mid; float* part; int32_t *d_len, *d_pos_off, *d_ndec; float* cfg_pv; int* cfg_pi; float* cfg_mix;
    size_t kv_row_off;                // byte offset of the first row inside a K or V layer block
    int shared_row;                   // the shared uncond prompt's row (batch row 1), counted from r0
    const int32_t* row_order;         // longest-first launch order of the decode attention: the whole batch only
    int S_last = 1; long slab_last = 0;
};
// pg_request_token_logprobs / pg_request_token_stats as the decode / generate call they were armed for took them (pg_engine::take_requests)
struct TokenRequests { float* lp_out; int64_t lp_cap; pg_token_stats ts; bool stats; };
// pg_request_attn_spans as the prefill that took it serves it: device copies of pad_len [R] and the spans [R][n_spans], where layer li's block goes
struct AttnSpanRun { const int32_t *d_pad, *d_lo, *d_hi; int n_spans, q_col0, n_q; uint64_t mask; float* out; long layer_floats; };

struct pg_engine {
    pg_config cfg{};
    int dev = 0;
    bool bf = true;
    size_t esz = 2;
    std::string err;
    std::vector<void*> allocs;
    int64_t bytes = 0;
    std::map<std::string, Slot> slots_map;

    // ---- weights
    struct Layer { void *wqkv, *wo, *wgu, *wd, *ln1, *ln2; void *wqkv_t = nullptr, *wo_t = nullptr, *wgu_t = nullptr, *wd_t = nullptr;
                   void* wqkv_p = nullptr; };      // wqkv_p: [8 | 8]-interleaved q / k rows for the prefill RoPE epilogue (bf16)
    void *gh_w1_t = nullptr, *gh_w2_t = nullptr, *lm_head_t = nullptr;
    int tile_one(hipStream_t s, const void* src, void** dst, int N, int K);
    std::vector<Layer> layers;
    void* norm_w = nullptr; float* embed = nullptr; void* lm_head = nullptr;
    void *gh_w1 = nullptr, *gh_w2 = nullptr; float *gh_b1 = nullptr, *gh_b2 = nullptr;
    float *ge_w = nullptr, *al_w0 = nullptr, *al_b0 = nullptr, *al_w2 = nullptr, *al_b2 = nullptr;
    float* gen_table = nullptr;
    float *codebook = nullptr, *codebook_n = nullptr, *pq_w = nullptr, *pq_b = nullptr;
    void* pq_table = nullptr;
    void* qc_w = nullptr; float* qc_b = nullptr;                 // encoder quant_conv (z -> img_dim)
    float *enc_in_w = nullptr, *enc_in_b = nullptr;              // encoder conv_in (3 -> ch), fp32 [Cout][3][3][3]
    VqNet dec, enc;
    // SigLIP + aligner (a13)
    LinW vit_patch, al0, al2; float* vit_pos = nullptr; std::vector<VitBlockW> vit_blocks; NormW vit_norm;
    float* vx = nullptr; void *vt = nullptr, *vqk = nullptr, *vvt = nullptr, *vo = nullptr, *vh = nullptr, *vp = nullptr, *val = nullptr;
    float* vscore = nullptr;
    float *cos_t = nullptr, *sin_t = nullptr; int max_pos = 0;
    void* zeros = nullptr;
    bool finalized = false;
    bool allow_partial = false;       // pg_set_option("allow_partial_weights", 1): run with missing tensors (they read as zeros)

    // ---- sequence state
    int R = 0, L = 0, slots = 0; bool prefilled = false;
    int n_dec_host = 0;
    std::vector<int> h_len;
    // pg_prefill_extend / pg_rewind: host copy of d_pos_off (written by prefill), the new-token counts of the running extension on the device
    // (d_nnew [max_rows]; ext_nnew is non-null only while pg_prefill_extend runs its layers, like as_run) and their maximum
    std::vector<int> h_pos_off; int32_t* d_nnew = nullptr; const int32_t* ext_nnew = nullptr; int ext_max_new = 0;
    int32_t *d_len = nullptr, *d_pos_off = nullptr, *d_ndec = nullptr, *d_tok_row = nullptr, *d_tok_j = nullptr,
            *d_tok_src = nullptr, *d_last = nullptr, *d_unf = nullptr, *d_anyunf = nullptr, *d_row_off = nullptr;
    int max_len_host = 0; bool flash_prefill = true;
    int32_t* h_stage2[2] = {nullptr, nullptr};                   // pinned host staging, double-buffered
    hipEvent_t ev_stage[2] = {nullptr, nullptr}; bool stage_used[2] = {false, false}; int stage_sel = 0;
    int32_t* d_flag = nullptr; int32_t* h_flag = nullptr;        // uncond-sharing probe result
    float* cfg_pv = nullptr; int* cfg_pi = nullptr;              // sampler stage-1 winners
    float* txt_mix = nullptr;                                    // top-k / top-p text sampler: reduced logit rows [max_rows, vocab] (first filtered call)
    float* cfg_mix = nullptr;                                    // top-k / top-p sampler: CFG-mixed rows [max_rows/2, img_vocab] (first filtered call)
    SampleParams* d_sparams = nullptr; TextParams* d_tparams = nullptr;   // per-call parameters the graphs read from HBM
    DualWeights* d_dual = nullptr;                                // pg_decode_image_tokens_dual: (w_caption, w_layout), read from HBM in the same way
    // grammar-constrained text decode (pg_set_text_dfa): device tables allocated once at the limits (first upload), so a captured step keeps
    // valid addresses when another automaton is uploaded; pinned staging guarded by an event, like the prefill's row metadata
    int16_t* d_dfa_class = nullptr; int16_t* d_dfa_next = nullptr; int32_t* d_dfa_dist = nullptr; TextDfaHdr* d_dfa_hdr = nullptr;
    int32_t* d_dfa_state = nullptr;                               // [max_rows] the rows' states of the running constrained call
    TextParams* d_op_tparams = nullptr; int32_t* d_op_step = nullptr;     // pg_op_text_constrain's parameters and step
    unsigned char* h_dfa = nullptr; size_t h_dfa_bytes = 0; hipEvent_t ev_dfa = nullptr; bool dfa_staged = false;
    bool dfa_set = false; int32_t dfa_dist_start = 0;
    int32_t *d_out_tok = nullptr, *d_force_tok = nullptr; uint8_t* d_force_mask = nullptr; int64_t* d_text_out = nullptr;
    // pg_request_token_logprobs: the caller's destination for the NEXT decode / generate call (one-shot, like uncond_hint) and the library-owned
    // [B, T] / [B, max_new] buffer the loop's kernels write (allocated by the first request, so a captured step keeps a valid address)
    float* lp_req = nullptr; int64_t lp_req_cap = 0; float* d_logprob = nullptr;
    // pg_request_token_stats: the same one-shot scheme, independent of lp_req.  d_stats (first request) holds P = max_rows * (max_new + 1)
    // positions of every output at the widest request: [logprob P | entropy P | rank P | alt_tok 8 P | alt_logprob 8 P] (stats_out)
    pg_token_stats ts_req{}; bool ts_pending = false; float* d_stats = nullptr;
    const char* check_stats_request(const pg_token_stats* r) const;      // null, or why pg_request_token_stats / pg_op_token_stats refuse it
    TokenStatsOut stats_out(int n_alt) const {
        const size_t P = (size_t)cfg.max_rows * (cfg.max_new + 1);
        return TokenStatsOut{d_stats, d_stats + P, (int32_t*)(d_stats + 2 * P), (int32_t*)(d_stats + 3 * P), d_stats + 11 * P, n_alt};
    }
    int stats_copy_out(const pg_token_stats& r, int B, int cols, int pitch_cols, hipStream_t s);   // the first cols columns of [B, pitch_cols]
    // pg_request_attn_spans: one-shot in front of the next pg_prefill / pg_prefill_embeds (consumed whatever that call answers).  The host arrays
    // are copied at request time; d_as (first request) holds [pad_len max_rows | lo 16 max_rows | hi 16 max_rows]; as_run is non-null only while
    // the prefill that took the request runs its layers
    pg_attn_spans as_req{}; bool as_pending = false; std::vector<int32_t> as_lo, as_hi; int32_t* d_as = nullptr; const AttnSpanRun* as_run = nullptr;
    int request_attn_spans(const pg_attn_spans* req);
    int op_attn_span_mass(const void* q, const void* k, const int32_t* row_off, const int32_t* len, const int32_t* pad_len, const int32_t* lo,
                          const int32_t* hi, int R_, int nh, int slots_, int n_spans, int q_col0, int n_q, float scale, float* out, hipStream_t s);
    // pg_request_sample_plan: one-shot in front of the next image decode.  The host arrays are validated and staged at request time into d_plan
    // (first request): [w Bmax * max_new | temperature Bmax | top_k Bmax | top_p Bmax | key Bmax], Bmax = max_rows / 2; plan_mask says which arrays
    // the request carried -- the consuming call fills the others with its scalars (launch_plan_fill).  The host copies of temperature / top_k /
    // top_p choose the kernel route before anything is launched.  Pinned staging guarded by an event, like the automaton's.
    struct PlanRequest { bool pending = false; int B = 0, T = 0, mask = 0; std::vector<float> temp, top_p; std::vector<int32_t> top_k; };
    PlanRequest plan_req; float* d_plan = nullptr; unsigned char* h_plan = nullptr; hipEvent_t ev_plan = nullptr; bool plan_staged = false;
    SamplePlanDev plan_dev() const {
        const size_t Bm = (size_t)cfg.max_rows / 2, nw = Bm * cfg.max_new;
        return SamplePlanDev{d_plan, d_plan + nw, (const int32_t*)(d_plan + nw + Bm), d_plan + nw + 2 * Bm, (const int32_t*)(d_plan + nw + 3 * Bm)};
    }
    int request_sample_plan(const pg_sample_plan* plan, hipStream_t s);
    int rng_image_offset = 0;                                    // pg_set_option("rng_image_offset", lo): this rank's first image in the global batch
    PgTune tune;                                                 // per-handle tuning knobs (pg_set_option)
    int tune_epoch = 0;                                          // bumped by every option that changes what a captured graph contains
    void* kv = nullptr;
    // ---- workspaces
    long max_tok = 0;
    float* x = nullptr; void* xn = nullptr; float* part = nullptr; long part_elems = 0, decode_part_elems = 0;
    float* ssq_part = nullptr;        // [max_rows][8] partial sums of squares of the residual rows: the deferred-1/rms decode norm (round 6)
    bool defer_norm = true;           // decode at 65..128 rows, bf16: norm = barrier-free elementwise pass, 1/rms applied in the consumer GEMM's epilogue
    void *qbuf = nullptr, *obuf = nullptr, *hbuf = nullptr, *hfin = nullptr, *gh_in = nullptr, *gh_mid = nullptr;
    // VQ: cur / t1 / t2 / t3 rotate through vbuf
    void* vbuf[4] = {nullptr, nullptr, nullptr, nullptr}; long vbuf_elems = 0;
    void *cur = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr;
    void *aq = nullptr, *ak = nullptr, *avt = nullptr, *ao = nullptr, *ap = nullptr; float* ascore = nullptr;
    float *gn_stats = nullptr, *gn_ws = nullptr, *gn_coef = nullptr;
    bool gn_refused = false;                                             // launch_gn_stats declined a shape: the entry point that ran it returns PG_ERR_ARG
    const void* gn_part_of = nullptr; int gn_part_n = 0, gn_part_b = 0;   // gn_ws holds conv-epilogue partials of this tensor
    float* enc_z = nullptr;
    void* stage_dev = nullptr; long stage_bytes = 0;
    // pg_preprocess_images (imgproc.hip): device workspace (descriptors | coefficient tables | uint8 intermediates), allocated on first use and grown
    // when a batch needs more, and its own double-buffered pinned staging for the descriptors
    void* ip_dev = nullptr; long ip_dev_bytes = 0;
    uint8_t* ip_host[2] = {nullptr, nullptr}; long ip_host_bytes[2] = {0, 0};
    hipEvent_t ip_ev[2] = {nullptr, nullptr}; bool ip_used[2] = {false, false}; int ip_sel = 0;
    // pg_score_tokens / pg_op_head_logprob: library-owned workspace, allocated on first use and grown on demand (the old one is freed, like ip_dev).
    // bf16: the fused head's (max, sum) partials [G][n][2]; f32 (parity mode): one row chunk's logits (<= 64 MB) + its gathered rows
    // pg_score_image_tokens / pg_op_cfg_head_logprob use it too: [gen_head layer-1 output of all rows | the head's own part, as above with pairs]
    void* sh_ws = nullptr; long sh_ws_bytes = 0;
    long sh_mid_bytes = 0;              // bytes of gen_head layer-1 output the last pg_score_image_tokens left at the start of sh_ws (debug tap "score_mid")
    // ---- streams / graph / timing
    hipStream_t istream = nullptr; hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr, ev_p0 = nullptr, ev_p1 = nullptr, ev_v0 = nullptr, ev_v1 = nullptr;
    hipGraphExec_t gexec = nullptr; std::vector<int64_t> gkey;
    hipGraphExec_t gexec_txt = nullptr; std::vector<int64_t> gkey_txt;      // text-decode step (lm_head + argmax + stack)
    void drop_graphs() { if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; } if (gexec_txt) { (void)hipGraphExecDestroy(gexec_txt); gexec_txt = nullptr; } }
    bool use_graph = false;   // decode step replayed as a hipGraph; OFF by default: same-stream launches measure 1 % (bs=64) to 3.3 % (bs=8/16) faster than graph replay on ROCm 7.2 and the host loop keeps ahead at every batch size
    bool prefill_rope_epi = true;     // prefill QKV: RoPE + KV write in the 256x256 GEMM's epilogue when the shape takes that kernel (0: GEMM -> fp32 q|k|v -> rope_kv_kernel)
    bool prefill_res_epi = true;      // prefill o / down: residual add in the GEMM epilogue (0: slab + norm-kernel form, for A/B)
    bool time_attn = false; bool fuse_rope = true; bool force_swiglu = true; bool mid_bf16 = true;
    bool skip_attn = false;                                      // libplangen_diag.so only (pg_diag_set_option): the decode step WITHOUT its attention launches -- results are garbage; no entry point of libplangen_hip.so can set it
    // per-kernel-class HIP-event timing of the decode loop (eager instrumented pass, pg_set_option("time_attn", 1)):
    // one event pair per launch group on the launch stream, on every ``time_stride``-th decode step
    enum { TC_ATTN = 0, TC_QKV, TC_O, TC_GU, TC_DOWN, TC_NORM, TC_HEAD, TC_SAMPLE, TC_EMPTY, TC_N };
    std::vector<hipEvent_t> tc_ev; size_t tc_used = 0; std::vector<std::pair<int, double>> tc_meta; int time_stride = 1;
    double tc_ms[TC_N] = {}, tc_bytes[TC_N] = {}; int tc_launches[TC_N] = {};
    bool tc_on = false; hipStream_t tc_stream = nullptr;
    void tic(hipStream_t s) {
        if (!tc_on) return;
        while (tc_ev.size() < tc_used + 2) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { tc_on = false; return; } tc_ev.push_back(e); }
        (void)hipEventRecord(tc_ev[tc_used], s);
    }
    void toc(hipStream_t s, int cls, double bytes) {
        if (!tc_on || tc_ev.size() < tc_used + 2) return;
        (void)hipEventRecord(tc_ev[tc_used + 1], s);
        tc_meta.emplace_back(cls, bytes); tc_used += 2;
    }
    pg_timing timing{};
    bool have_decode_t = false, have_prefill_t = false, have_vq_t = false;

    template <typename U> int dalloc(U** p, size_t n_bytes, bool zero = true) {
        void* q = nullptr;
        if (n_bytes == 0) n_bytes = 16;
        HIPCHK(hipMalloc(&q, n_bytes));
        if (zero) HIPCHK(hipMemsetAsync(q, 0, n_bytes, nullptr));      // weights never loaded read as zeros, not as stale HBM
        allocs.push_back(q); bytes += (int64_t)n_bytes; *p = (U*)q;
        return PG_OK;
    }
    int H() const { return cfg.hidden; }
    int HD() const { return cfg.n_heads * cfg.head_dim; }
    int img_tokens() const { return cfg.grid * cfg.grid; }
    int img_size() const { return cfg.grid << (cfg.vq_levels - 1); }
    size_t kv_layer_elems() const { return (size_t)cfg.max_rows * cfg.n_heads * slots * 128; }
    // FP8 KV cache (cfg.kv_dtype = PG_FP8_E4M3, bf16 compute only; format: kv8.h): ``kv`` holds the e4m3fn codes of every layer, ``kv_scale`` the
    // interleaved (K, V) fp32 scales, and kc(li) / vc(li) -- used by the PREFILL kernels only in this mode -- resolve to ONE layer-sized bf16
    // scratch that every layer reuses: prefill runs unchanged on bf16 and kv_quantize_kernel converts the packed tokens after each layer's attention.
    bool kv8 = false; float* kv_scale = nullptr; void* kv_scratch = nullptr;
    size_t kv_layer_slots() const { return (size_t)cfg.max_rows * cfg.n_heads * slots; }
    void* kc(const DecodeView& v, int layer) const { return kv8 ? kv_scratch : (char*)kv + ((size_t)layer * 2 + 0) * kv_layer_elems() * esz + v.kv_row_off; }
    void* vc(const DecodeView& v, int layer) const { return kv8 ? (char*)kv_scratch + kv_layer_elems() * 2 : (char*)kv + ((size_t)layer * 2 + 1) * kv_layer_elems() * esz + v.kv_row_off; }
    uint8_t* kc8(int layer) const { return (uint8_t*)kv + ((size_t)layer * 2 + 0) * kv_layer_elems(); }
    uint8_t* vc8(int layer) const { return (uint8_t*)kv + ((size_t)layer * 2 + 1) * kv_layer_elems(); }
    float* kvs(int layer) const { return kv_scale + (size_t)layer * 2 * kv_layer_slots(); }
    int shared_len = 0; bool share_uncond = true;
    int uncond_hint = -1;             // next pg_prefill only: 1 = caller guarantees every odd row carries row 1's ids, 0 = it does not, -1 = probe on the device (one 4-byte read + stream sync)
    // decode lanes: the batch's rows split into independent chains on separate streams.  A lane is a DecodeView of its row range -- view(first row,
    // rows, lane) -- and the whole batch is view(0, R, 0): the workspace pointers above stay the whole-batch bases and are never rebased.  Lane 1
    // brings its own slab buffer, step counter and stream (part2, d_ndec2, istream2); ev_fork / ev_join tie the two streams together once per step.
    int lanes_opt = -1;               // -1 auto, 1, 2
    float* part2 = nullptr; hipStream_t istream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int32_t* d_ndec2 = nullptr;
    int32_t* d_row_order = nullptr; bool lpt_order = true; bool order_valid = false; int order_rows = 0;
    // pg_prefill_replicated: the batch is `replicas_n` copies of R / replicas_n distinct rows (row t * R0 + r = replica t of row r); group_rows = R0 while
    // the replicas' prompt slots alias their owner rows (alias = 1), 0 otherwise (plain prefill, alias = 0 after the copy, replicas = 1)
    int group_rows = 0, replicas_n = 1;
    DecodeView view(int r0, int rows, int lane) const {
        const size_t r = (size_t)r0, Hh = H(), HDm = HD();
        DecodeView v; v.r0 = r0; v.rows = rows;
        v.x = x + r * Hh; v.xn = (char*)xn + r * Hh * esz; v.qbuf = (char*)qbuf + r * HDm * esz; v.obuf = (char*)obuf + r * HDm * esz;
        v.hbuf = (char*)hbuf + r * cfg.inter * esz; v.hfin = (char*)hfin + r * Hh * esz; v.gh_mid = (char*)gh_mid + r * cfg.gen_head_dim * esz;
        v.part = lane ? part2 : part; v.d_len = d_len + r; v.d_pos_off = d_pos_off + r; v.d_ndec = lane ? d_ndec2 : d_ndec;
        v.cfg_pv = cfg_pv + r * 8; v.cfg_pi = cfg_pi + r * 8; v.cfg_mix = cfg_mix ? cfg_mix + (r / 2) * cfg.img_vocab : nullptr;
        v.kv_row_off = r * cfg.n_heads * (size_t)slots * 128 * esz; v.shared_row = 1 - r0;
        v.row_order = (lpt_order && order_valid && r0 == 0 && rows == order_rows) ? d_row_order : nullptr;
        return v;
    }
    SeqState seq(const DecodeView& v) const { return SeqState{v.d_len, v.d_pos_off, v.d_ndec, d_tok_row, d_tok_j, shared_len, v.shared_row, v.row_order, group_rows}; }

    int create();
    void add_slot(const std::string& name, void* dst, SlotKind k, long n, int a = 0, int b = 0, int c = 0);
    void slot_shape(const std::string& name, std::initializer_list<int64_t> shp) { slots_map[name].shape = shp; }
    int alloc_conv(const std::string& name, ConvW& cw, int cout, int cin, int k);
    int alloc_norm(const std::string& name, NormW& nw, int c);
    int alloc_gnorm(const std::string& name, NormW& nw, int c);
    int alloc_res(const std::string& name, ResBlockW& r, int cin, int cout);
    int alloc_attn(const std::string& name, AttnW& a, int c);
    int build_vq();
    int alloc_lin(const std::string& name, LinW& l, int out, int in);
    int build_vision();
    template <typename T> void lin(hipStream_t s, const LinW& l, const T* in, void* out, int out_f32, const void* residual, int res_f32, int act, long M);
    template <typename T> int vision_encode(const void* img, int img_dtype, void* out, int out_dtype, int B, hipStream_t s);
    int load_tensor(const char* name, const void* src, int dtype, const int64_t* shape, int ndim);
    int merge_lora(const char* name, const void* a_host, int a_dtype, const void* b_host, int b_dtype, int out_f, int in_f, int r, float scale);
    int finalize(int* missing, hipStream_t s);
    // pad_len: [R0] rows; replicas > 1 (pg_prefill_replicated): the batch is R0 * replicas virtual rows of which only the R0 distinct ones are packed
    int prefill(const int32_t* ids_dev, const void* emb_dev, int emb_dtype, const int32_t* pad_len, int R0, int L_,
                int pmode, void* hidden_out, int hidden_dtype, hipStream_t s, int replicas = 1, int alias = 0, bool replicated_api = false);
    // cur[r] = h_len[r] + n_dec_host: the K/V slots row r holds.  extend: n_new_host [R] new tokens per row, left-aligned in [R, Lx]
    bool hfin_stale = false;                                                // pg_rewind ran last: hfin belongs to the sequence it cut, nothing may sample from it
    int max_pos_end() const { int m = 0; for (int r = 0; r < R && r < (int)h_len.size(); ++r) m = std::max(m, h_pos_off[r] + h_len[r]); return m; }   // RoPE position of the next slot, largest over the rows
    int check_extendable(const char* who);                                  // PG_OK, or why pg_prefill_extend / pg_rewind refuse the handle's state
    int set_lengths(const int32_t* s_len, int32_t* s_ord, hipStream_t s);   // h_len, max_len_host, the row order and zeroed step counters, host and device
    int prefill_extend(const int32_t* ids_dev, const void* emb_dev, int emb_dtype, const int32_t* n_new_host, int Lx, void* hidden_out,
                       int hidden_dtype, hipStream_t s);
    int rewind(const int32_t* len_host, hipStream_t s);
    template <typename T> void gemm_residual(hipStream_t s, DecodeView& v, const T* a, const T* W, int M, int N, int K);
    template <typename T> void gemm_llm(hipStream_t s, DecodeView& v, const T* a, const T* W, int M, int N, int K, bool allow_skinny, const void* Wt = nullptr);
    template <typename T> void run_layers(hipStream_t s, DecodeView& v, int M, int mode, T* final_out, int32_t* advance = nullptr);
    template <typename T> void head_logits(hipStream_t s, DecodeView& v, const T* in, int M);
    void forward_decode(hipStream_t s, DecodeView& v);
    // what both decode loops share: the one-shot requests, the hop to the engine's own stream and back, the captured step
    TokenRequests take_requests() { TokenRequests q{lp_req, lp_req_cap, ts_req, ts_pending}; lp_req = nullptr; lp_req_cap = 0; ts_pending = false; return q; }
    int reserve_requests(const TokenRequests& q);
    int hop_in(hipStream_t s);
    int hop_out(hipStream_t ws, hipStream_t s);
    template <typename F> int graph_step(hipGraphExec_t& exec, std::vector<int64_t>& cached, const std::vector<int64_t>& key, hipStream_t s, F&& record);
    // the image decode loop behind both entry points: what the entry point is and allows; everything else is the call's own arguments
    struct ImageLoopSpec {
        const char* name;                                         // the entry point, for messages
        int rows_per_image;                                       // 2: cond / uncond; 3: dual guidance
        float w, w_layout;                                        // cfg_weight, or (w_caption, w_layout)
        bool takes_plan, two_lanes, shared_negative, aliased_replicas;
    };
    int image_loop(const ImageLoopSpec& sp, int T, float temp, int top_k, float top_p, uint64_t seed, const int32_t* force_tok, const uint8_t* force_mask,
                   int32_t* out_tok, float* logits_out, hipStream_t s);
    int decode_image(int T, float cfgw, float temp, int top_k, float top_p, uint64_t seed, const int32_t* force_tok,
                     const uint8_t* force_mask, int32_t* out_tok, float* logits_out, hipStream_t s);
    int decode_image_dual(int T, float w_caption, float w_layout, float temp, int top_k, float top_p, uint64_t seed, const int32_t* force_tok,
                          const uint8_t* force_mask, int32_t* out_tok, float* logits_out, hipStream_t s);
    int step(const void* emb, int emb_dtype, void* hidden_out, int hidden_dtype, hipStream_t s);
    int gen_head(const void* h_dev, int h_dtype, float* logits, int R_, hipStream_t s);
    int text_greedy(int max_new, int min_new, int eos, int64_t* out, int* out_len, hipStream_t s) {
        return text_generate(max_new, min_new, eos, 0.f, 0, 1.f, 0, out, out_len, nullptr, s);
    }
    // constrained: every step's logits are masked by the automaton of set_text_dfa (min_new unused); state_out [R] or null: the final states
    int text_generate(int max_new, int min_new, int eos, float temp, int top_k, float top_p, uint64_t seed, int64_t* out, int* out_len,
                      float* logits_out, hipStream_t s, bool constrained = false, int32_t* state_out = nullptr);
    int set_text_dfa(const pg_text_dfa* dfa, hipStream_t s);
    int token_logprob(const float* x, int B, int V, const int32_t* tok, float temp, float* out, hipStream_t s);
    int token_stats(const float* x, int B, int V, const int32_t* tok, float temp, const pg_token_stats* out, hipStream_t s);
    int head_logprob(const char* who, const void* x, int64_t rows, const void* w, int V, int K, const int32_t* row_idx, const int32_t* target, int64_t n,
                     float temp, float* out, hipStream_t s);
    int sh_reserve(long need);
    long cfg_head_need(int64_t n, int V, int K) const;
    int cfg_head_run(const char* who, const void* x, const void* w, int V, int K, const float* bias, const int32_t* cond_idx, const int32_t* uncond_idx,
                     const int32_t* target, int64_t n, float cfgw, float temp, float* out, hipStream_t s, char* ws);
    int cfg_head_logprob(const char* who, const void* x, int64_t rows, const void* w, int V, int K, const float* bias, const int32_t* cond_idx,
                         const int32_t* uncond_idx, const int32_t* target, int64_t n, float cfgw, float temp, float* out, hipStream_t s);
    int score_image_tokens(const void* hidden, int64_t rows, const int32_t* cond_idx, const int32_t* uncond_idx, const int32_t* target, int64_t n,
                           float cfgw, float temp, float* out, hipStream_t s);
    int text_constrain(const float* logits, int B, int V, const int32_t* state, int remaining, int eos, float temp, int top_k, float top_p,
                       uint64_t seed, int row_offset, int step, uint8_t* keep, int32_t* tok, int32_t* next_state, hipStream_t s);
    template <typename T> int vq_decode(const int32_t* codes, void* img_out, int out_dtype, int B, hipStream_t s);
    template <typename T> int vq_encode(const void* img, int img_dtype, int64_t* idx, int B, hipStream_t s);
    template <typename T> void conv3(hipStream_t s, const ConvW& cw, const T* in, void* out, int out_f32, const void* residual, int res_f32, int B, int Hi, int Wi, int up, int stride2, int feeds_gn = -1);
    template <typename T> void conv1(hipStream_t s, const ConvW& cw, const T* in, void* out, int out_f32, const void* residual, int res_f32, long M, int gn_hw = 0);   // gn_hw > 0: the output feeds a GroupNorm (pixels per image)
    template <typename T> void resblock(hipStream_t s, const ResBlockW& r, int B, int Hs, int Ws);
    template <typename T> void attnblock(hipStream_t s, const AttnW& a, int B, int HW);
    template <typename TI> void gn_coefs(hipStream_t s, const NormW& n, const TI* in, int B, int HW);      // statistics (conv epilogue partials or the stats kernel) -> gn_coef
    template <typename T, typename TI = float> void gn(hipStream_t s, const NormW& n, const TI* in, T* out, int B, int HW, int swish);
    int preprocess_images(const pg_image_u8* images, int B, int S, int min_size, const uint8_t* background, const float* lut_host, void* out_dev,
                          int out_dtype, hipStream_t s);
    int fetch_timing();
    void destroy();
};

struct TuneGuard {          // points this thread's kernel launchers at the handle's knobs for the duration of one ABI call
    const PgTune* saved;
    explicit TuneGuard(pg_handle h) : saved(pg_tune) { if (h) pg_tune = &h->tune; }
    ~TuneGuard() { pg_tune = saved; }
};

