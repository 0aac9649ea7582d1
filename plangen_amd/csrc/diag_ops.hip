// libplangen_diag.so only: operator entry points of the attention kernels (tests/test_gpu_attention.py), of the decode step's deferred-RMSNorm
// pair and slab-folding elementwise kernels (tests/test_gpu_decode_ops.py), of the VQ-16 decoder kernels (tests/test_gpu_vq_ops.py) and of the prefill
// GEMM epilogues -- RoPE + KV write (act 3), SwiGLU (act 2), rope_kv_kernel alone and the two weight interleavers (tests/test_gpu_prefill_ops.py) -- and of
// the understanding path's input-side kernels (SigLIP LayerNorm / patchify / add_pos, the VQ encoder's conv_in and nearest-code search, l2norm_rows, the
// two-level batched GEMM of SigLIP's scores and P . V: tests/test_gpu_vision_ops.py) and of the decode GEMM dispatch itself -- launch_gemm_skinny /
// launch_gemm_skinny_swiglu on the tiled copy or on row-major weights, with the caller's split count and stream_gemm mask: tests/test_gpu_skinny_ops.py --
// and of the samplers' draw -- launch_cfg_step and launch_text_argmax / launch_text_sample on the caller's slabs: tests/test_gpu_draws.py --
// and of the weight converters pg_engine::load_tensor launches and the row movers of every prefill / step / score call (tests/test_gpu_load_ops.py) --
// for the operator tests.  Each one points the calling thread's pg_tune at a local PgTune (no diagnostics hooks, one kernel-form selector set), calls the PRODUCTION launcher and restores
// pg_tune.  Shapes the kernels do not support are refused with PG_ERR_ARG and never launched.  Head dimension: 128 for the LLM kernels (implied
// by the [.., nh * 128] layouts), 64 for SigLIP (C / NH).  Row lengths, slots and token maps live in device memory; they are copied back and
// checked on the host before anything is launched (these are test entry points: the synchronisation does not matter).
#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <vector>
#include "kernels.h"
#include "diag.h"
#include "gemm_skinny.h"       // SK_BK: the K chunk of the tiled decode copy
#include "../../include/plangen_hip.h"

namespace {
struct LocalTune {                  // the thread's pg_tune points at `t` for the lifetime of this object
    PgTune t;
    const PgTune* saved;
    LocalTune() : saved(pg_tune) { t.diag = nullptr; pg_tune = &t; }
    ~LocalTune() { pg_tune = saved; }
};
constexpr int kMaxGridYZ = 65535;
bool opt256_ok(int o) { return o == 1 || o == 4 || o == 5 || o == 6 || o == 12 || o == 13 || o == 14; }      // gemm256.hip pick_tile_height: auto, 256 / 224 / 192 rows, + 8 = four phases
bool to_host(std::vector<int32_t>& dst, const int32_t* src, int n) {
    dst.assign(n > 0 ? n : 0, 0);
    if (n <= 0) return true;
    if (!src) return false;
    return hipMemcpy(dst.data(), src, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
}
int launched(hipStream_t s) { (void)s; return hipGetLastError() == hipSuccess ? PG_OK : PG_ERR_HIP; }
}  // namespace

extern "C" {

// Fused decode attention (path 0: launch_attn_decode_fused) or the unfused pair (path 1: launch_rope_kv mode 0 into qbuf, then launch_attn mode 0;
// no shared-prompt aliasing in that pair, so shared_len must be 0).  form: 0 = the production choice, 4 = big (4-wave), 8 = small (8-wave).
// qbuf: [M][nh * 128] T scratch for path 1, or null (allocated here).  len / pos_off: [rows] device, n_dec: [1] device, row_order: [M] or null.
int pg_diag_op_attn_decode(int is_bf16, int form, int path, const float* qkv, int S, long slab, void* obuf, void* kc, void* vc,
                           const float* cos_t, const float* sin_t, const int32_t* len, const int32_t* pos_off, const int32_t* n_dec,
                           const int32_t* row_order, int shared_len, int shared_row, int M, int nh, int slots, int max_pos, float scale,
                           void* qbuf, pg_stream stream) {
    if (!qkv || !obuf || !kc || !vc || !cos_t || !sin_t || !len || !pos_off || !n_dec) return PG_ERR_ARG;
    if (form != 0 && form != 4 && form != 8) return PG_ERR_ARG;
    if (path != 0 && path != 1) return PG_ERR_ARG;
    if (M < 1 || M > kMaxGridYZ || nh < 1 || nh > kMaxGridYZ || S < 1 || slab < (long)M * 3 * nh * 128 || slots < 1 || max_pos < 1) return PG_ERR_ARG;
    if (shared_len < 0 || shared_len > slots || (path == 1 && shared_len > 0)) return PG_ERR_ARG;
    std::vector<int32_t> hl, hn, ho;
    if (!to_host(hl, len, M) || !to_host(hn, n_dec, 1) || !to_host(ho, row_order, row_order ? M : 0)) return PG_ERR_HIP;
    for (int r = 0; r < M; ++r) {
        const long slot = (long)hl[r] + hn[0];
        if (hl[r] < 0 || hn[0] < 0 || slot >= slots) return PG_ERR_ARG;          // the append slot must exist
    }
    if (row_order) {                                                            // a permutation of [0, M)
        std::vector<char> seen(M, 0);
        for (int i = 0; i < M; ++i) {
            if (ho[i] < 0 || ho[i] >= M || seen[ho[i]]) return PG_ERR_ARG;
            seen[ho[i]] = 1;
        }
    }
    LocalTune lt;
    lt.t.attn_waves = form;
    const hipStream_t s = (hipStream_t)stream;
    SeqState st{len, pos_off, n_dec, nullptr, nullptr, shared_len, shared_row, row_order};
    if (path == 0) {
        if (is_bf16) launch_attn_decode_fused<bf16>(s, qkv, S, slab, (bf16*)obuf, (bf16*)kc, (bf16*)vc, cos_t, sin_t, st, M, nh, slots, max_pos, scale);
        else launch_attn_decode_fused<float>(s, qkv, S, slab, (float*)obuf, (float*)kc, (float*)vc, cos_t, sin_t, st, M, nh, slots, max_pos, scale);
        return launched(s);
    }
    void* q = qbuf;
    if (!q && hipMalloc(&q, (size_t)M * nh * 128 * (is_bf16 ? 2 : 4)) != hipSuccess) return PG_ERR_HIP;
    if (is_bf16) {
        launch_rope_kv<bf16>(s, qkv, S, slab, (bf16*)q, (bf16*)kc, (bf16*)vc, cos_t, sin_t, st, 0, M, nh, slots, max_pos);
        launch_attn<bf16>(s, (const bf16*)q, (bf16*)obuf, (const bf16*)kc, (const bf16*)vc, st, 0, M, nh, slots, scale);
    } else {
        launch_rope_kv<float>(s, qkv, S, slab, (float*)q, (float*)kc, (float*)vc, cos_t, sin_t, st, 0, M, nh, slots, max_pos);
        launch_attn<float>(s, (const float*)q, (float*)obuf, (const float*)kc, (const float*)vc, st, 0, M, nh, slots, scale);
    }
    const int rc = launched(s);
    if (!qbuf) { (void)hipStreamSynchronize(s); (void)hipFree(q); }
    return rc;
}

// Fused decode attention over the FP8 KV cache (launch_attn_decode_kv8, bf16 compute): arguments as pg_diag_op_attn_decode with the e4m3fn codes
// kc8 / vc8 [rows][nh][slots][128] and the interleaved scales kvs fp32 [rows][nh][slots][2] = (K, V) in place of kc / vc.  form as above.
int pg_diag_op_attn_decode_kv8(int form, const float* qkv, int S, long slab, void* obuf, void* kc8, void* vc8, float* kvs,
                               const float* cos_t, const float* sin_t, const int32_t* len, const int32_t* pos_off, const int32_t* n_dec,
                               const int32_t* row_order, int shared_len, int shared_row, int M, int nh, int slots, int max_pos, float scale,
                               pg_stream stream) {
    if (!qkv || !obuf || !kc8 || !vc8 || !kvs || !cos_t || !sin_t || !len || !pos_off || !n_dec) return PG_ERR_ARG;
    if (form != 0 && form != 4 && form != 8) return PG_ERR_ARG;
    if (M < 1 || M > kMaxGridYZ || nh < 1 || nh > kMaxGridYZ || S < 1 || slab < (long)M * 3 * nh * 128 || slots < 1 || max_pos < 1) return PG_ERR_ARG;
    if (shared_len < 0 || shared_len > slots) return PG_ERR_ARG;
    std::vector<int32_t> hl, hn, ho;
    if (!to_host(hl, len, M) || !to_host(hn, n_dec, 1) || !to_host(ho, row_order, row_order ? M : 0)) return PG_ERR_HIP;
    for (int r = 0; r < M; ++r) {
        const long slot = (long)hl[r] + hn[0];
        if (hl[r] < 0 || hn[0] < 0 || slot >= slots) return PG_ERR_ARG;          // the append slot must exist
    }
    if (row_order) {                                                            // a permutation of [0, M)
        std::vector<char> seen(M, 0);
        for (int i = 0; i < M; ++i) {
            if (ho[i] < 0 || ho[i] >= M || seen[ho[i]]) return PG_ERR_ARG;
            seen[ho[i]] = 1;
        }
    }
    LocalTune lt;
    lt.t.attn_waves = form;
    const hipStream_t s = (hipStream_t)stream;
    SeqState st{len, pos_off, n_dec, nullptr, nullptr, shared_len, shared_row, row_order};
    launch_attn_decode_kv8(s, qkv, S, slab, (bf16*)obuf, (uint8_t*)kc8, (uint8_t*)vc8, kvs, cos_t, sin_t, st, M, nh, slots, max_pos, scale);
    return launched(s);
}

// Grouped form of the fused decode attention (SeqState::group_rows > 0: what pg_prefill_replicated with alias = 1 launches): arguments as
// pg_diag_op_attn_decode (path 0 only) plus group_rows in [1, M]; rows off the shared uncond prompt read their prompt slots [0, len[row]) from
// row (row % group_rows).  The caches are the caller's: the kernel can be tested without an engine state.
}  // extern "C"
namespace {
// the argument screen of both grouped operators: PG_OK, or the status to return (nothing is launched on a refusal)
int screen_grouped(int form, const int32_t* len, const int32_t* n_dec, const int32_t* row_order, int shared_len, int shared_row, int group_rows, int M, int nh,
                   int S, long slab, int slots, int max_pos) {
    if (group_rows < 1 || group_rows > M) return PG_ERR_ARG;
    if (form != 0 && form != 4 && form != 8) return PG_ERR_ARG;
    if (M < 1 || M > kMaxGridYZ || nh < 1 || nh > kMaxGridYZ || S < 1 || slab < (long)M * 3 * nh * 128 || slots < 1 || max_pos < 1) return PG_ERR_ARG;
    if (shared_len < 0 || shared_len > slots || (shared_len > 0 && (shared_row < 0 || shared_row >= M))) return PG_ERR_ARG;
    std::vector<int32_t> hl, hn, ho;
    if (!to_host(hl, len, M) || !to_host(hn, n_dec, 1) || !to_host(ho, row_order, row_order ? M : 0)) return PG_ERR_HIP;
    for (int r = 0; r < M; ++r) {
        const long slot = (long)hl[r] + hn[0];
        if (hl[r] < 0 || hn[0] < 0 || slot >= slots) return PG_ERR_ARG;          // the append slot must exist
        if (hl[r] != hl[r % group_rows]) return PG_ERR_ARG;                       // a replica carries its owner's prompt length
    }
    if (row_order) {                                                            // a permutation of [0, M)
        std::vector<char> seen(M, 0);
        for (int i = 0; i < M; ++i) {
            if (ho[i] < 0 || ho[i] >= M || seen[ho[i]]) return PG_ERR_ARG;
            seen[ho[i]] = 1;
        }
    }
    return PG_OK;
}
}  // namespace
extern "C" {
int pg_diag_op_attn_decode_grouped(int is_bf16, int form, const float* qkv, int S, long slab, void* obuf, void* kc, void* vc,
                                   const float* cos_t, const float* sin_t, const int32_t* len, const int32_t* pos_off, const int32_t* n_dec,
                                   const int32_t* row_order, int shared_len, int shared_row, int group_rows, int M, int nh, int slots, int max_pos,
                                   float scale, pg_stream stream) {
    if (!qkv || !obuf || !kc || !vc || !cos_t || !sin_t || !len || !pos_off || !n_dec) return PG_ERR_ARG;
    const int rc = screen_grouped(form, len, n_dec, row_order, shared_len, shared_row, group_rows, M, nh, S, slab, slots, max_pos);
    if (rc != PG_OK) return rc;
    LocalTune lt;
    lt.t.attn_waves = form;
    const hipStream_t s = (hipStream_t)stream;
    SeqState st{len, pos_off, n_dec, nullptr, nullptr, shared_len, shared_row, row_order, group_rows};
    if (is_bf16) launch_attn_decode_fused<bf16>(s, qkv, S, slab, (bf16*)obuf, (bf16*)kc, (bf16*)vc, cos_t, sin_t, st, M, nh, slots, max_pos, scale);
    else launch_attn_decode_fused<float>(s, qkv, S, slab, (float*)obuf, (float*)kc, (float*)vc, cos_t, sin_t, st, M, nh, slots, max_pos, scale);
    return launched(s);
}

// FP8 twin: arguments as pg_diag_op_attn_decode_kv8 plus group_rows.
int pg_diag_op_attn_decode_grouped_kv8(int form, const float* qkv, int S, long slab, void* obuf, void* kc8, void* vc8, float* kvs,
                                       const float* cos_t, const float* sin_t, const int32_t* len, const int32_t* pos_off, const int32_t* n_dec,
                                       const int32_t* row_order, int shared_len, int shared_row, int group_rows, int M, int nh, int slots,
                                       int max_pos, float scale, pg_stream stream) {
    if (!qkv || !obuf || !kc8 || !vc8 || !kvs || !cos_t || !sin_t || !len || !pos_off || !n_dec) return PG_ERR_ARG;
    const int rc = screen_grouped(form, len, n_dec, row_order, shared_len, shared_row, group_rows, M, nh, S, slab, slots, max_pos);
    if (rc != PG_OK) return rc;
    LocalTune lt;
    lt.t.attn_waves = form;
    const hipStream_t s = (hipStream_t)stream;
    SeqState st{len, pos_off, n_dec, nullptr, nullptr, shared_len, shared_row, row_order, group_rows};
    launch_attn_decode_kv8(s, qkv, S, slab, (bf16*)obuf, (uint8_t*)kc8, (uint8_t*)vc8, kvs, cos_t, sin_t, st, M, nh, slots, max_pos, scale);
    return launched(s);
}

// Prefill attention over the packed tokens: path 2 = attn_prefill_flash2_kernel, 1 = attn_prefill_flash_kernel (both bf16), 0 = attn_kernel mode 1.
// qbuf / obuf: [Ntok][nh * 128] T; caches [R][nh][slots][128] T; row_off / len: [R] device (row_off -1: the row has no packed token);
// tok_row / tok_j: [Ntok] device.  The packed tokens of row r must be row_off[r] .. row_off[r] + len[r] - 1 with tok_j = 0 .. len[r] - 1.
int pg_diag_op_attn_prefill(int is_bf16, int path, const void* qbuf, void* obuf, const void* kc, const void* vc, const int32_t* row_off,
                            const int32_t* len, const int32_t* tok_row, const int32_t* tok_j, int R, int max_len, int Ntok, int nh, int slots,
                            float scale, pg_stream stream) {
    if (!qbuf || !obuf || !kc || !vc || !row_off || !len || !tok_row || !tok_j) return PG_ERR_ARG;
    if (path < 0 || path > 2 || (path > 0 && !is_bf16)) return PG_ERR_ARG;
    if (R < 1 || R > kMaxGridYZ || nh < 1 || nh > kMaxGridYZ || Ntok < 1 || Ntok > 0x7fffffff / 8 || max_len < 1 || max_len > slots) return PG_ERR_ARG;
    std::vector<int32_t> hoff, hlen, hrow, hj;
    if (!to_host(hoff, row_off, R) || !to_host(hlen, len, R) || !to_host(hrow, tok_row, Ntok) || !to_host(hj, tok_j, Ntok)) return PG_ERR_HIP;
    for (int m = 0; m < Ntok; ++m)
        if (hrow[m] < 0 || hrow[m] >= R || hj[m] < 0 || hj[m] >= slots) return PG_ERR_ARG;
    for (int r = 0; r < R; ++r) {
        if (hlen[r] < 0 || hlen[r] > max_len) return PG_ERR_ARG;
        if (hoff[r] < 0) continue;
        if (hlen[r] < 1 || (long)hoff[r] + hlen[r] > Ntok) return PG_ERR_ARG;
        for (int j = 0; j < hlen[r]; ++j)
            if (hrow[hoff[r] + j] != r || hj[hoff[r] + j] != j) return PG_ERR_ARG;
    }
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (path > 0) {
        lt.t.prefill_attn = path;
        launch_attn_prefill_flash(s, (const bf16*)qbuf, (bf16*)obuf, (const bf16*)kc, (const bf16*)vc, row_off, len, R, max_len, nh, slots, scale);
        return launched(s);
    }
    SeqState st{len, nullptr, nullptr, tok_row, tok_j, 0, 1, nullptr};
    if (is_bf16) launch_attn<bf16>(s, (const bf16*)qbuf, (bf16*)obuf, (const bf16*)kc, (const bf16*)vc, st, 1, Ntok, nh, slots, scale);
    else launch_attn<float>(s, (const float*)qbuf, (float*)obuf, (const float*)kc, (const float*)vc, st, 1, Ntok, nh, slots, scale);
    return launched(s);
}

// Extension attention (pg_prefill_extend) over the packed NEW tokens: path 2 = attn_extend_flash_kernel (bf16), 0 = attn_kernel mode 1.
// len [R]: the rows' lengths after the extension; n_new [R]: new tokens per row (ignored where row_off is -1).  The packed tokens of row r must
// be row_off[r] .. row_off[r] + n_new[r] - 1 with tok_j = len[r] - n_new[r] .. len[r] - 1.  Other arguments as pg_diag_op_attn_prefill.
int pg_diag_op_attn_extend(int is_bf16, int path, const void* qbuf, void* obuf, const void* kc, const void* vc, const int32_t* row_off,
                           const int32_t* len, const int32_t* n_new, const int32_t* tok_row, const int32_t* tok_j, int R, int max_new, int Ntok,
                           int nh, int slots, float scale, pg_stream stream) {
    if (!qbuf || !obuf || !kc || !vc || !row_off || !len || !n_new || !tok_row || !tok_j) return PG_ERR_ARG;
    if ((path != 0 && path != 2) || (path > 0 && !is_bf16)) return PG_ERR_ARG;
    if (R < 1 || R > kMaxGridYZ || nh < 1 || nh > kMaxGridYZ || Ntok < 1 || Ntok > 0x7fffffff / 8 || max_new < 1 || max_new > slots) return PG_ERR_ARG;
    std::vector<int32_t> hoff, hlen, hnew, hrow, hj;
    if (!to_host(hoff, row_off, R) || !to_host(hlen, len, R) || !to_host(hnew, n_new, R) || !to_host(hrow, tok_row, Ntok) || !to_host(hj, tok_j, Ntok)) return PG_ERR_HIP;
    for (int m = 0; m < Ntok; ++m)
        if (hrow[m] < 0 || hrow[m] >= R || hj[m] < 0 || hj[m] >= slots) return PG_ERR_ARG;
    for (int r = 0; r < R; ++r) {
        if (hoff[r] < 0) continue;
        if (hlen[r] < 1 || hlen[r] > slots || hnew[r] < 1 || hnew[r] > hlen[r] || hnew[r] > max_new || (long)hoff[r] + hnew[r] > Ntok) return PG_ERR_ARG;
        for (int i = 0; i < hnew[r]; ++i)
            if (hrow[hoff[r] + i] != r || hj[hoff[r] + i] != hlen[r] - hnew[r] + i) return PG_ERR_ARG;
    }
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (path == 2) {
        launch_attn_extend_flash(s, (const bf16*)qbuf, (bf16*)obuf, (const bf16*)kc, (const bf16*)vc, row_off, len, n_new, R, max_new, nh, slots, scale);
        return launched(s);
    }
    SeqState st{len, nullptr, nullptr, tok_row, tok_j, 0, 1, nullptr};
    if (is_bf16) launch_attn<bf16>(s, (const bf16*)qbuf, (bf16*)obuf, (const bf16*)kc, (const bf16*)vc, st, 1, Ntok, nh, slots, scale);
    else launch_attn<float>(s, (const float*)qbuf, (float*)obuf, (const float*)kc, (const float*)vc, st, 1, Ntok, nh, slots, scale);
    return launched(s);
}

// SigLIP attention (bf16, heads of 64, non-causal): qk [B * P][2C] (q | k), vt [B][C][P] (V transposed), o [B * P][C].
// form 1 = the 64-key tile kernel; 4 / 8 / 12 / 16 = the LDS-resident kernel with that many waves (the launcher still falls back to the
// tile kernel when K / V^T of a head do not fit the LDS).
int pg_diag_op_attn_vit(int form, const void* qk, const void* vt, void* o, int B, int P, int C, int NH, float scale, pg_stream stream) {
    if (!qk || !vt || !o) return PG_ERR_ARG;
    if (form != 1 && form != 4 && form != 8 && form != 12 && form != 16) return PG_ERR_ARG;
    if (B < 1 || B > kMaxGridYZ || NH < 1 || NH > kMaxGridYZ || C != NH * 64 || P < 64 || P % 64 || (long)B * P * 2 * C > 0x7fffffffL) return PG_ERR_ARG;
    LocalTune lt;
    lt.t.vit_attn = form;
    const hipStream_t s = (hipStream_t)stream;
    launch_attn_vit_flash(s, (const bf16*)qk, (const bf16*)vt, (bf16*)o, B, P, C, NH, scale);
    return launched(s);
}

// ------------------------------------------------------------------------------------------------ decode step, 65..128 rows (round 6 pair)
// Producer of the deferred-1/rms pair (launch_rmsnorm_defer): x [M][2048] fp32 += the S slabs of partial (slab elements apart), xw [M][2048] bf16 =
// bf16(x . w) WITHOUT the 1/rms, ssq [M][8] fp32 = sums of squares of columns [256 j, 256 j + 256).  The launcher's contract is enforced here.
int pg_diag_op_rmsnorm_defer(float* x, const float* partial, int S, long slab, const void* w, void* xw, float* ssq, int M, int H, pg_stream stream) {
    if (!x || !partial || !w || !xw || !ssq) return PG_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)partial | (uintptr_t)ssq) & 15 || ((uintptr_t)w | (uintptr_t)xw) & 7) return PG_ERR_ARG;      // f32x4 / 4 x bf16 vectors
    if (H != 2048 || S < 1 || S > 8 || M < 1 || M > 0x7fffffff / 2 / H) return PG_ERR_ARG;
    if (slab < (long)M * H || slab > 0x7fffffffL || (slab & 3)) return PG_ERR_ARG;      // 32-bit stride, 16-byte loads
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    launch_rmsnorm_defer(s, x, partial, S, slab, (const bf16*)w, (bf16*)xw, ssq, M, H);
    return launched(s);
}

// Consumer of the pair: W [N][K] bf16 row-major is re-tiled exactly like pg_op_gemm kind 4 / pg_finalize_weights do, then
// launch_gemm_skinny_deferred (swiglu 0: out fp32 [S][M][N]) or launch_gemm_skinny_swiglu_deferred (swiglu 1, S == 1: out bf16 [M][N / 2]; W rows
// already [8 gate | 8 up] interleaved, as for pg_op_swiglu_gemm).  The shape is NOT screened against deferred_norm_ok here: the launcher itself must
// refuse (return false -> PG_ERR_ARG, out untouched; the tiled copy built before it never touches out), so the tests pin that BOTH launchers consult the
// predicate.  Only what keeps the tiled copy's own construction in bounds (N % 16, K % SK_BK, sizes) and the consumer's 16-byte loads of ssq is checked.
int pg_diag_op_gemm_deferred(const void* xw, const void* W_rowmajor, void* out, int M, int N, int K, int S, const float* ssq, float eps, int swiglu,
                             pg_stream stream) {
    if (!xw || !W_rowmajor || !out || !ssq) return PG_ERR_ARG;
    if (swiglu != 0 && swiglu != 1) return PG_ERR_ARG;
    if (M < 1 || N < 16 || (N & 15) || K < SK_BK || (K % SK_BK) || S < 1 || (swiglu && S != 1) || (long)N * K > 0x7fffffffL) return PG_ERR_ARG;
    if (((uintptr_t)ssq | (uintptr_t)xw | (uintptr_t)out | (uintptr_t)W_rowmajor) & 15) return PG_ERR_ARG;     // ssq: two f32x4 per row; xw / W / out: 16-byte vectors
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    bf16* wt = nullptr;
    if (hipMalloc((void**)&wt, (size_t)N * K * 2) != hipSuccess) return PG_ERR_HIP;
    launch_tile_weights(s, (const bf16*)W_rowmajor, wt, N, K);
    const bool ok = swiglu ? launch_gemm_skinny_swiglu_deferred(s, (const bf16*)xw, wt, (bf16*)out, M, N, K, ssq, eps)
                           : launch_gemm_skinny_deferred(s, (const bf16*)xw, wt, (float*)out, M, N, K, S, ssq, eps);
    const int rc = launched(s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(wt);
    return ok ? rc : PG_ERR_ARG;
}

// Slab-folding elementwise kernels: kind 0 = launch_silu_mul (partial [S][M][2 N] fp32 with [8 gate | 8 up] interleaved columns -> out [M][N] T,
// N = I, I % 8 == 0; bias / act unused), kind 1 = launch_bias_act (partial [S][M][N] fp32 (+ bias [N] fp32 or null) -> out [M][N] T; act 0 = none,
// 1 = erf GELU; is_bf16 0 with act 0 is launch_bias_f32).
int pg_diag_op_slab_epilogue(int kind, int is_bf16, const float* partial, int S, long slab, const float* bias, void* out, int M, int N, int act,
                             pg_stream stream) {
    if (!partial || !out) return PG_ERR_ARG;
    if ((kind != 0 && kind != 1) || M < 1 || M > kMaxGridYZ || N < 1 || S < 1) return PG_ERR_ARG;
    if (kind == 0 && ((N & 7) || bias || act)) return PG_ERR_ARG;
    if (kind == 1 && act != 0 && act != 1) return PG_ERR_ARG;
    if (slab < (long)M * N * (kind == 0 ? 2 : 1)) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (kind == 0) {
        if (is_bf16) launch_silu_mul<bf16>(s, partial, S, slab, (bf16*)out, M, N);
        else launch_silu_mul<float>(s, partial, S, slab, (float*)out, M, N);
    } else if (is_bf16) launch_bias_act<bf16>(s, partial, S, slab, bias, (bf16*)out, M, N, act);
    else if (act == 0) launch_bias_f32(s, partial, S, slab, bias, (float*)out, M, N);
    else launch_bias_act<float>(s, partial, S, slab, bias, (float*)out, M, N, act);
    return launched(s);
}

// ------------------------------------------------------------------------------------------------ VQ-16 decoder operators (tests/test_gpu_vq_ops.py)
// Every entry point below synchronises the stream before it returns.  Which kernel ran is part of the result: forms that name ONE kernel call that kernel's
// own launcher (conv_halo_try, gemm256_try, conv_out_halo_try, conv_out_gn_try) and return PG_ERR_ARG, output untouched, when it declines the shape; form 0
// (the production dispatch) reports it through *nsplit_out.
}  // extern "C"
namespace {
int finish(hipStream_t s) {
    const hipError_t a = hipGetLastError(), b = hipStreamSynchronize(s);
    return a == hipSuccess && b == hipSuccess ? PG_OK : PG_ERR_HIP;
}
bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
struct ZeroPage {                   // the convolutions' zero halo source (>= 256 B)
    void* p = nullptr;
    bool ok() { return hipMalloc(&p, 1024) == hipSuccess && hipMemset(p, 0, 1024) == hipSuccess; }
    ~ZeroPage() { if (p) (void)hipFree(p); }
};
}  // namespace
extern "C" {

// 3x3 convolution through the engine's own call (pg_engine::conv3): x NHWC [B][Hi][Wi][Cin] T, w [Cout][9][Cin] T (Engine.op_conv3x3's layout), bias fp32 [Cout],
// residual [B][Ho][Wo][Cout] fp32 (res_f32) or T, or null; out [B][Ho][Wo][Cout] fp32 (out_f32) or T.  engine_bf16 0: gemm_f32_kernel<ConvLoaderB<float>> (form 0 / 1,
// fp32 residual and output, no partials).  form: 0 launch_gemm as the engine calls it, 1 the 128 x 128 implicit GEMM (conv_halo = gemm256 = 0), 2 gemm256_try
// (gn_epilogue256 = want_gn), 3 conv_halo_try with the fast epilogues (conv_halo = 1), 4 conv_halo_try lock-step (conv_halo = 2).  want_gn: GroupNorm partials into
// ws (ws_floats fp32 available); *nsplit_out = splits per image the kernel wrote (0: none) and, when > 0, launch_gn_finalize -> stats [B][32][2] = (mean, rstd).
int pg_diag_op_conv3x3(int engine_bf16, int form, const void* x, const void* w, const float* bias, const void* residual, void* out, int out_f32, int res_f32,
                       int B, int Hi, int Wi, int Cin, int Cout, int up, int stride2, int want_gn, float* ws, long ws_floats, float* stats, float eps,
                       int* nsplit_out, pg_stream stream) {
    if (!x || !w || !bias || !out || !nsplit_out) return PG_ERR_ARG;
    if (form < 0 || form > 4 || (!engine_bf16 && form > 1)) return PG_ERR_ARG;
    if ((up != 0 && up != 1) || (stride2 != 0 && stride2 != 1) || (up && stride2)) return PG_ERR_ARG;
    if (B < 1 || Hi < 1 || Wi < 1 || Cin < 1 || Cout < 1 || (stride2 && (Hi < 2 || Wi < 2))) return PG_ERR_ARG;
    if (Hi > 16384 || Wi > 16384 || (long)B * Hi * Wi * Cin >= (1L << 31)) return PG_ERR_ARG;       // 32-bit element offsets of the slim loader, packed (y, x)
    const int Ho = stride2 ? Hi / 2 : (Hi << up), Wo = stride2 ? Wi / 2 : (Wi << up);
    const long M = (long)B * Ho * Wo;
    if (M * Cout >= (1L << 31)) return PG_ERR_ARG;
    if (engine_bf16) {
        if (!pow2(Cin) || Cin < 64 || Cin > 512) return PG_ERR_ARG;                                  // ConvLoader: 64-element K tiles inside one tap, shift / mask
        if (((uintptr_t)x | (uintptr_t)w) & 15) return PG_ERR_ARG;                                  // 16-byte LDS-DMA
    } else if (!out_f32 || (residual && !res_f32) || want_gn) return PG_ERR_ARG;
    if (((uintptr_t)out | (uintptr_t)residual | (uintptr_t)bias) & 15) return PG_ERR_ARG;
    *nsplit_out = 0;
    if (want_gn) {
        if (!ws || !stats || Cout % 32) return PG_ERR_ARG;
        const long t_halo = (long)(Ho / 8) * (Wo / 32), t_256 = (long)Ho * Wo / 64;
        if (t_halo > 1024 || t_256 > 1024) return PG_ERR_ARG;                                        // pg_engine::conv3 asks for partials up to 1024 tiles per image
        if (ws_floats < (long)B * (t_halo > t_256 ? t_halo : t_256) * 64) return PG_ERR_ARG;
    }
    ZeroPage z;
    if (!z.ok()) return PG_ERR_HIP;
    LocalTune lt;
    lt.t.conv_halo = form == 0 || form == 3 ? 1 : form == 4 ? 2 : 0;
    lt.t.gemm256 = form == 1 ? 0 : 1;
    lt.t.gn_epilogue256 = form == 2 && want_gn ? 1 : 0;
    const hipStream_t s = (hipStream_t)stream;
    GemmA a; a.kind = stride2 ? 2 : 1; a.ptr = x; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.up = up; a.zeros = z.p;
    GemmEpi e; e.out = out; e.out_f32 = out_f32; e.ldc = Cout; e.bias_n = bias; e.residual = residual; e.res_f32 = res_f32;
    int nsp = 0;
    if (want_gn) { a.gn_part = ws; a.gn_nsplit = &nsp; }
    bool taken = true;
    if (!engine_bf16) launch_gemm<float>(s, a, (const float*)w, 9L * Cin, 0, e, (int)M, Cout, 9 * Cin, 1);
    else if (form == 2) taken = gemm256_try(s, a, (const bf16*)w, 9L * Cin, 0, e, (int)M, Cout, 9 * Cin, 1, 1, 0);
    else if (form >= 3) taken = conv_halo_try(s, a, (const bf16*)w, e, (int)M, Cout, 9 * Cin, ws && want_gn ? ws : nullptr, want_gn ? &nsp : nullptr);
    else launch_gemm<bf16>(s, a, (const bf16*)w, 9L * Cin, 0, e, (int)M, Cout, 9 * Cin, 1);
    if (taken && nsp > 0) launch_gn_finalize(s, ws, stats, nullptr, nullptr, nullptr, B, nsp, Ho * Wo, Cout, eps);
    const int rc = finish(s);
    if (!taken) return PG_ERR_ARG;
    *nsplit_out = nsp;
    return rc;
}

// GroupNorm(32) as pg_engine::gn runs it: launch_gn_stats (x [B][HW][C], fp32 or bf16) -> stats [B][32][2], coef [B][C][2]; launch_gn_apply -> out (fp32 or bf16).
// (in, out) one of the three instantiated pairs: fp32 -> fp32, fp32 -> bf16, bf16 -> bf16.  ws: the partial sums, ws_floats fp32 available.
int pg_diag_op_groupnorm(int in_bf16, int out_bf16, const void* x, const float* gamma, const float* beta, void* out, float* stats, float* coef, float* ws,
                         long ws_floats, int B, int HW, int C, int swish, float eps, pg_stream stream) {
    if (!x || !gamma || !beta || !out || !stats || !coef || !ws) return PG_ERR_ARG;
    if (in_bf16 && !out_bf16) return PG_ERR_ARG;                                                     // no bf16 -> fp32 instantiation
    if (B < 1 || B > kMaxGridYZ || HW < 1 || C < 32 || C % 32 || (long)B * HW * C >= (1L << 40)) return PG_ERR_ARG;
    const int epv_in = in_bf16 ? 8 : 4, epv_out = out_bf16 ? 8 : 4;
    if (C % epv_in || C / epv_in > 256 || C % epv_out) return PG_ERR_ARG;                            // gn_stats_kernel: a thread per 16-byte vector of a pixel; gn_apply: whole vectors
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)coef) & 15) return PG_ERR_ARG;
    const long nsplit = HW > 16384 ? 256 : (HW + 63) / 64;
    if (ws_floats < (long)B * nsplit * 64) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (!launch_gn_stats(s, x, in_bf16, stats, ws, B, HW, C, eps, coef, gamma, beta)) return PG_ERR_ARG;
    if (in_bf16) launch_gn_apply<bf16, bf16>(s, (const bf16*)x, coef, (bf16*)out, B, HW, C, swish);
    else if (out_bf16) launch_gn_apply<float, bf16>(s, (const float*)x, coef, (bf16*)out, B, HW, C, swish);
    else launch_gn_apply<float, float>(s, (const float*)x, coef, (float*)out, B, HW, C, swish);
    return finish(s);
}

// launch_gn_stats alone on whatever shape the caller names: the LAUNCHER must refuse what its kernel cannot do (false -> PG_ERR_ARG, stats untouched).
// Buffers must be sized for the shape as if it ran.
int pg_diag_op_gn_stats_raw(int in_bf16, const void* x, const float* gamma, const float* beta, float* stats, float* coef, float* ws, int B, int HW, int C,
                            pg_stream stream) {
    if (!x || !gamma || !beta || !stats || !coef || !ws) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    const bool ok = launch_gn_stats(s, x, in_bf16, stats, ws, B, HW, C, 1e-6f, coef, gamma, beta);
    const int rc = finish(s);
    return ok ? rc : PG_ERR_ARG;
}

// softmax(x * scale) over the rows of x fp32 [rows][n] -> y [rows][n] fp32 or bf16 (launch_softmax_rows).
int pg_diag_op_softmax_rows(int out_bf16, const float* x, void* y, int rows, int n, float scale, pg_stream stream) {
    if (!x || !y || rows < 1 || n < 1 || (long)rows * n >= (1L << 40)) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (out_bf16) launch_softmax_rows<bf16>(s, x, (bf16*)y, rows, n, scale);
    else launch_softmax_rows<float>(s, x, (float*)y, rows, n, scale);
    return finish(s);
}

// C = A . W^T through launch_gemm (kind 0) with the whole epilogue struct: A [batch][M][K] (lda, strideA; strideA 0 broadcasts), W [batch][N][K] (ldb, strideB),
// out fp32 (out_f32) or T (ldc, strideC), v = acc scale + bias_n[col] + bias_m[row] + residual (fp32 when res_f32, else T; ldr / strideR, 0: as out), act 0 / 1 (erf GELU).
// engine_bf16 0: gemm_f32_kernel.  form: 0 launch_gemm as the engine calls it, 1 the 128 x 128 kernel (gemm256 = 0), 2 gemm256_try (gn_epilogue256 = gn_hw > 0).
// gn_hw > 0: GroupNorm partials of the output (pixels per image) -> ws, *nsplit_out, stats as pg_diag_op_conv3x3.
// gemm256_opt (pg_diag_op_gemm_epi256 only; 1 everywhere else): pg_tune->gemm256 of a form-2 launch.
}  // extern "C"
namespace {
// Output blocks of a two-level batched GEMM: block (b, b2) starts at b strideC + b2 strideC2 and covers M rows of N elements, ldc apart.  Seen on the grid of
// ldc-wide rows a block is the rectangle rows [q, q + M) x columns [p, p + N) with start = q ldc + p; a block that wraps the row pitch (p + N > ldc) is refused,
// and no two rectangles may intersect -- that covers the dense layouts and the column-offset one (strideC2 < ldc: the heads side by side inside a row).
bool blocks_disjoint(int M, int N, long ldc, int batch, int batch2, long strideC, long strideC2) {
    struct Rect { long q, p; };
    std::vector<Rect> r;
    r.reserve((size_t)batch * batch2);
    for (int b = 0; b < batch; ++b)
        for (int b2 = 0; b2 < batch2; ++b2) {
            const long o = (long)b * strideC + (long)b2 * strideC2;
            if (o % ldc + N > ldc) return false;
            r.push_back({o / ldc, o % ldc});
        }
    std::sort(r.begin(), r.end(), [](const Rect& a, const Rect& b) { return a.q < b.q || (a.q == b.q && a.p < b.p); });
    for (size_t i = 0; i < r.size(); ++i)
        for (size_t j = i + 1; j < r.size() && r[j].q < r[i].q + M; ++j)
            if (r[j].p < r[i].p + N && r[i].p < r[j].p + N) return false;
    return true;
}
int gemm_epi_impl(int engine_bf16, int form, const void* A, long lda, long strideA, const void* W, long ldb, long strideB, void* out, int out_f32, long ldc,
                  long strideC, const float* bias_n, const float* bias_m, const void* residual, int res_f32, long ldr, long strideR, float scale, int act,
                  int M, int N, int K, int batch, int batch2, long strideA2, long strideB2, long strideC2, int gn_hw, float* ws, long ws_floats, float* stats,
                  float eps, int* nsplit_out, pg_stream stream, int gemm256_opt = 1) {
    if (!A || !W || !out || !nsplit_out) return PG_ERR_ARG;
    if (form < 0 || form > 2 || (!engine_bf16 && form == 2) || (act != 0 && act != 1)) return PG_ERR_ARG;
    if (gemm256_opt != 1 && (form != 2 || gn_hw || !opt256_ok(gemm256_opt))) return PG_ERR_ARG;       // a pinned tile height / phase count names gemm256_try's plain launch
    if (M < 1 || N < 1 || K < 1 || batch < 1 || batch > kMaxGridYZ || lda < K || ldb < K || ldc < N || strideA < 0 || strideB < 0 || strideC < 0) return PG_ERR_ARG;
    if (batch2 < 1 || (long)batch * batch2 > kMaxGridYZ || strideA2 < 0 || strideB2 < 0 || strideC2 < 0) return PG_ERR_ARG;      // gemm_f32_kernel: grid z = batch x batch2
    if (batch2 == 1) {
        if (batch > 1 && strideC < (long)(M - 1) * ldc + N) return PG_ERR_ARG;                       // batches must not overlap in the output
    } else {
        if (residual || gn_hw) return PG_ERR_ARG;                                                    // the kernels have no second-level residual stride; partials need batch 1
        if (!blocks_disjoint(M, N, ldc, batch, batch2, strideC, strideC2)) return PG_ERR_ARG;
    }
    if (residual && ((ldr && ldr < N) || strideR < 0)) return PG_ERR_ARG;
    if (engine_bf16) {
        // PlainLoaderB / the weight rows: 64-element K tiles fetched as 16-byte LDS-DMA chunks
        if (K % 64 || ((lda | ldb | strideA | strideB | strideA2 | strideB2) & 7) || (((uintptr_t)A | (uintptr_t)W) & 15)) return PG_ERR_ARG;
    } else if (!out_f32 || (residual && !res_f32) || gn_hw) return PG_ERR_ARG;
    if (((uintptr_t)out | (uintptr_t)residual | (uintptr_t)bias_n) & 15) return PG_ERR_ARG;         // vec_ok() looks at the leading dimensions and offsets only
    *nsplit_out = 0;
    if (gn_hw) {
        if (gn_hw < 1 || !ws || !stats || N % 32 || M % gn_hw || batch != 1) return PG_ERR_ARG;
        if (ws_floats < (long)(M / gn_hw) * ((gn_hw + 63) / 64) * 64) return PG_ERR_ARG;
    }
    LocalTune lt;
    lt.t.gemm256 = form == 1 ? 0 : gemm256_opt;
    lt.t.gn_epilogue256 = form == 2 && gn_hw ? 1 : 0;
    const hipStream_t s = (hipStream_t)stream;
    GemmA a; a.ptr = A; a.lda = lda; a.strideA = strideA; a.strideA2 = strideA2;
    GemmEpi e; e.out = out; e.out_f32 = out_f32; e.ldc = ldc; e.strideC = strideC; e.strideC2 = strideC2; e.bias_n = bias_n; e.bias_m = bias_m; e.residual = residual;
    e.res_f32 = res_f32; e.ldr = ldr; e.strideR = strideR; e.scale = scale; e.act = act;
    int nsp = 0;
    if (gn_hw) { a.gn_part = ws; a.gn_nsplit = &nsp; a.gn_hw = gn_hw; }
    bool taken = true;
    if (!engine_bf16) launch_gemm<float>(s, a, (const float*)W, ldb, strideB, e, M, N, K, batch, batch2, strideB2);
    else if (form == 2) taken = gemm256_try(s, a, (const bf16*)W, ldb, strideB, e, M, N, K, batch, batch2, strideB2);
    else launch_gemm<bf16>(s, a, (const bf16*)W, ldb, strideB, e, M, N, K, batch, batch2, strideB2);
    if (taken && nsp > 0) launch_gn_finalize(s, ws, stats, nullptr, nullptr, nullptr, M / gn_hw, nsp, gn_hw, N, eps);
    const int rc = finish(s);
    if (!taken) return PG_ERR_ARG;
    *nsplit_out = nsp;
    return rc;
}
}  // namespace
extern "C" {
int pg_diag_op_gemm_epi(int engine_bf16, int form, const void* A, long lda, long strideA, const void* W, long ldb, long strideB, void* out, int out_f32, long ldc,
                        long strideC, const float* bias_n, const float* bias_m, const void* residual, int res_f32, long ldr, long strideR, float scale, int act,
                        int M, int N, int K, int batch, int gn_hw, float* ws, long ws_floats, float* stats, float eps, int* nsplit_out, pg_stream stream) {
    return gemm_epi_impl(engine_bf16, form, A, lda, strideA, W, ldb, strideB, out, out_f32, ldc, strideC, bias_n, bias_m, residual, res_f32, ldr, strideR, scale, act,
                         M, N, K, batch, 1, 0, 0, 0, gn_hw, ws, ws_floats, stats, eps, nsplit_out, stream);
}

// pg_diag_op_gemm_epi, form 2 only, with pg_tune->gemm256 = gemm256_opt (4 / 5 / 6 pin 256 / 224 / 192 rows, + 8 = four phases per K tile; 1 = what
// pg_diag_op_gemm_epi runs): every instantiation of gemm256_try's plain launch by name (tests/test_gpu_prefill_lin_ops.py).  No GroupNorm partials.
int pg_diag_op_gemm_epi256(int gemm256_opt, const void* A, long lda, long strideA, const void* W, long ldb, long strideB, void* out, int out_f32, long ldc,
                           long strideC, const float* bias_n, const float* bias_m, const void* residual, int res_f32, long ldr, long strideR, float scale, int act,
                           int M, int N, int K, int batch, int* nsplit_out, pg_stream stream) {
    return gemm_epi_impl(1, 2, A, lda, strideA, W, ldb, strideB, out, out_f32, ldc, strideC, bias_n, bias_m, residual, res_f32, ldr, strideR, scale, act,
                         M, N, K, batch, 1, 0, 0, 0, 0, nullptr, 0, nullptr, 0.f, nsplit_out, stream, gemm256_opt);
}

// The decoder's conv_out (Cin -> Cout <= 4), NHWC in -> NCHW out (fp32, or bf16 when out_bf16).  form 1: launch_conv3x3_small<T> (x, w T; engine_bf16 picks T);
// 2: conv_out_halo_try with conv_halo = 1 (conv3x3_out2_kernel); 3: conv_out_halo_try with conv_halo = 2 (conv3x3_out_halo_kernel); 4: conv_out_gn_try
// (conv3x3_out_gn_kernel: x is the FP32 skip tensor, coef [B][Cin][2] the GroupNorm coefficients, swish as the decoder's tail).  Forms 2-4: bf16 weights.
int pg_diag_op_conv_out(int engine_bf16, int form, const void* x, const float* coef, const void* w, const float* bias, void* out, int out_bf16, int B, int H,
                        int Wd, int Cin, int Cout, int swish, pg_stream stream) {
    if (!x || !w || !bias || !out || form < 1 || form > 4 || (form > 1 && !engine_bf16) || (form == 4 && !coef)) return PG_ERR_ARG;
    if (B < 1 || B > kMaxGridYZ || H < 1 || H > kMaxGridYZ || Wd < 1 || Cin < 1 || Cout < 1 || Cout > 4) return PG_ERR_ARG;
    if ((long)B * H * Wd * Cin >= (1L << 31) || (((uintptr_t)x | (uintptr_t)w | (uintptr_t)coef) & 15)) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    bool taken = true;
    if (form == 1) {
        const int epv = engine_bf16 ? 8 : 4, esz = engine_bf16 ? 2 : 4;
        if (Cin % (4 * epv)) return PG_ERR_ARG;                                                      // four channel quarters of whole 16-byte vectors per pixel
        if ((size_t)3 * 66 * (Cin * esz + 16) + (size_t)Cout * 9 * Cin * 4 > 160 * 1024) return PG_ERR_ARG;     // the strip and the fp32 weights live in LDS
        if (engine_bf16) launch_conv3x3_small<bf16>(s, (const bf16*)x, (const bf16*)w, bias, out, out_bf16, B, H, Wd, Cin, Cout);
        else launch_conv3x3_small<float>(s, (const float*)x, (const float*)w, bias, out, out_bf16, B, H, Wd, Cin, Cout);
    } else if (form == 4) {
        lt.t.conv_halo = 1;
        taken = conv_out_gn_try(s, (const float*)x, coef, (const bf16*)w, bias, out, out_bf16, B, H, Wd, Cin, Cout, swish);
    } else {
        ZeroPage z;
        if (!z.ok()) return PG_ERR_HIP;
        lt.t.conv_halo = form == 2 ? 1 : 2;
        taken = conv_out_halo_try(s, (const bf16*)x, (const bf16*)w, bias, (const bf16*)z.p, out, out_bf16, B, H, Wd, Cin, Cout);
        const int rc = finish(s);                                                                    // before the zero page goes away
        return taken ? rc : PG_ERR_ARG;
    }
    const int rc = finish(s);
    return taken ? rc : PG_ERR_ARG;
}

// out [n][C] = table[clamp(codes[p], 0, vocab - 1)] (launch_vq_gather), T = bf16 or fp32.
int pg_diag_op_vq_gather(int is_bf16, const void* table, const int32_t* codes, void* out, int n, int C, int vocab, pg_stream stream) {
    if (!table || !codes || !out || n < 1 || C < 1 || vocab < 1) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (is_bf16) launch_vq_gather<bf16>(s, (const bf16*)table, codes, (bf16*)out, n, C, vocab);
    else launch_vq_gather<float>(s, (const float*)table, codes, (float*)out, n, C, vocab);
    return finish(s);
}

// ------------------------------------------------------------------------------------------------ prefill GEMM epilogues (tests/test_gpu_prefill_ops.py)
// Every entry point below synchronises the stream before it returns.
}  // extern "C"
namespace {
bool aligned16(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* p : ps) a |= (uintptr_t)p;
    return (a & 15) == 0;
}
// Token map of a RoPE + KV write: token m -> (row[m], slot[m]).  rows inside [0, R), slots >= 0, pos_off inside [0, max_pos), no cache slot with two owners
// (the kernels' stores would race).  slot >= slots is what the kernels' capacity guard is for and is ALLOWED -- but only below 2 * slots and in a row that is
// not the last one, so that even a kernel without the guard writes inside the caches [R][nh][slots][128], where the callers' sentinel screen sees it.
int screen_token_map(const std::vector<int32_t>& row, const std::vector<int32_t>& slot, const std::vector<int32_t>& pos, int M, int R, int slots, int max_pos) {
    for (int r = 0; r < R; ++r)
        if (pos[r] < 0 || pos[r] >= max_pos) return PG_ERR_ARG;
    std::vector<char> owned((size_t)R * slots, 0);
    for (int m = 0; m < M; ++m) {
        if (row[m] < 0 || row[m] >= R || slot[m] < 0) return PG_ERR_ARG;
        if (slot[m] >= slots) {
            if (row[m] == R - 1 || slot[m] >= 2L * slots) return PG_ERR_ARG;
            continue;
        }
        char& o = owned[(size_t)row[m] * slots + slot[m]];
        if (o) return PG_ERR_ARG;
        o = 1;
    }
    return PG_OK;
}
struct Scratch {
    void* p = nullptr;
    bool get(size_t bytes) { return hipMalloc(&p, bytes) == hipSuccess; }
    ~Scratch() { if (p) (void)hipFree(p); }
};
// What the three image sampler step operators allocate and fill alike: SampleParams (p.has_force / has_mask from the pointers), the step counter,
// the 16 B winner slots, the mixed rows when the route stores them, and the SampleArgs over the caller's buffers.  Lives until finish(s).
struct SamplerStep {
    Scratch sp, nd, pv, pi, mix;
    SampleArgs a{};
    int setup(hipStream_t s, SampleParams p, bool need_mix, const float* partial, int S, long slab, const float* bias, int V, int B, const int32_t* force_tok,
              const uint8_t* force_mask, int32_t* out_tok, float* logits_out, const float* embed_table, float* x, int H, int step, int b_off, int B_total) {
        if (!sp.get(sizeof(SampleParams)) || !nd.get(4) || !pv.get((size_t)B * 16 * 4) || !pi.get((size_t)B * 16 * 4)) return PG_ERR_HIP;
        if (need_mix && !mix.get((size_t)B * V * 4)) return PG_ERR_HIP;
        const int32_t hstep = step;
        if (hipMemcpy(nd.p, &hstep, 4, hipMemcpyHostToDevice) != hipSuccess) return PG_ERR_HIP;
        p.has_force = force_tok != nullptr; p.has_mask = force_mask != nullptr;
        launch_set_sample_params(s, (SampleParams*)sp.p, p);
        a.logits_partial = partial; a.S = S; a.slab = slab; a.bias = bias; a.V = V; a.p = (const SampleParams*)sp.p;
        a.force_tok = force_tok; a.force_mask = force_mask; a.out_tok = out_tok; a.logits_out = logits_out;
        a.embed_table = embed_table; a.x = x; a.H = H; a.n_dec = (const int32_t*)nd.p; a.b_off = b_off; a.B_total = B_total;
        return PG_OK;
    }
    void launch(hipStream_t s, const SamplePlanDev* plan, const DualWeights* dw, int rows_per_image, int B, bool filtered, bool stored) {
        launch_cfg_step(s, a, plan, dw, rows_per_image, B, filtered, stored, (float*)pv.p, (int*)pi.p, (float*)mix.p);
    }
};
}  // namespace
extern "C" {

// Prefill QKV projection + RoPE + KV write.  xn bf16 [M][K], Wqkv bf16 [3 * nh * 128][K] row-major and UN-interleaved; qbuf bf16 [M][nh * 128], kc / vc bf16
// [R][nh][slots][128], cos_t / sin_t fp32 [max_pos][64], tok_row / tok_j [M] and pos_off [R] device.  form 0: launch_interleave_qk into scratch, then gemm256_try
// with act = 3 as run_layers calls it, pg_tune->gemm256 = gemm256_opt (1, 4, 5, 6, 12, 13, 14 and nothing else); PG_ERR_ARG when gemm256_try declines the shape.
// form 1: the engine's unfused path, launch_gemm<bf16> -> fp32 [M][3 * nh * 128] on the un-interleaved weights (gemm256_opt as above, or 0 = the 128 x 128
// kernel), then launch_rope_kv<bf16> mode 1 with S = 1.
int pg_diag_op_qkv_rope(int form, int gemm256_opt, const void* xn, const void* Wqkv, void* qbuf, void* kc, void* vc, const float* cos_t, const float* sin_t,
                        const int32_t* tok_row, const int32_t* tok_j, const int32_t* pos_off, int M, int nh, int K, int R, int slots, int max_pos,
                        pg_stream stream) {
    if (!xn || !Wqkv || !qbuf || !kc || !vc || !cos_t || !sin_t || !tok_row || !tok_j || !pos_off) return PG_ERR_ARG;
    if ((form != 0 && form != 1) || !(opt256_ok(gemm256_opt) || (form == 1 && gemm256_opt == 0))) return PG_ERR_ARG;
    if (M < 1 || nh < 1 || nh > 1024 || K < 128 || K % 64 || R < 1 || slots < 1 || max_pos < 1) return PG_ERR_ARG;
    const long N = 3L * nh * 128;
    if ((long)M * N >= (1L << 31) || N * K >= (1L << 31) || (long)R * slots > (1L << 28) || (long)R * nh * slots * 128 >= (1L << 40)) return PG_ERR_ARG;
    if (!aligned16({xn, Wqkv, qbuf, kc, vc, cos_t, sin_t, tok_row, tok_j, pos_off})) return PG_ERR_ARG;
    std::vector<int32_t> hrow, hj, hpos;
    if (!to_host(hrow, tok_row, M) || !to_host(hj, tok_j, M) || !to_host(hpos, pos_off, R)) return PG_ERR_HIP;
    const int sc = screen_token_map(hrow, hj, hpos, M, R, slots, max_pos);
    if (sc != PG_OK) return sc;
    LocalTune lt;
    lt.t.gemm256 = gemm256_opt;
    const hipStream_t s = (hipStream_t)stream;
    Scratch tmp;
    GemmA ga; ga.ptr = xn; ga.lda = K;
    if (form == 0) {
        if (!tmp.get((size_t)N * K * 2)) return PG_ERR_HIP;
        launch_interleave_qk(s, (const bf16*)Wqkv, (bf16*)tmp.p, nh, K);
        GemmEpi ge; ge.act = 3; ge.out = qbuf; ge.out_f32 = 0; ge.ldc = N;
        ge.rope.qbuf = qbuf; ge.rope.kc = kc; ge.rope.vc = vc; ge.rope.cos_t = cos_t; ge.rope.sin_t = sin_t;
        ge.rope.tok_row = tok_row; ge.rope.tok_j = tok_j; ge.rope.pos_off = pos_off;
        ge.rope.nh = nh; ge.rope.slots = slots; ge.rope.max_pos = max_pos;
        const bool taken = gemm256_try(s, ga, (const bf16*)tmp.p, K, 0, ge, M, (int)N, K, 1, 1, 0);
        const int rc = finish(s);                                                                    // before the interleaved copy goes away
        return taken ? rc : PG_ERR_ARG;
    }
    if (!tmp.get((size_t)M * N * 4)) return PG_ERR_HIP;
    GemmEpi e; e.out = tmp.p; e.out_f32 = 1; e.ldc = N;
    launch_gemm<bf16>(s, ga, (const bf16*)Wqkv, K, 0, e, M, (int)N, K, 1);
    SeqState st{nullptr, pos_off, nullptr, tok_row, tok_j, 0, 0, nullptr};
    launch_rope_kv<bf16>(s, (const float*)tmp.p, 1, (long)M * N, (bf16*)qbuf, (bf16*)kc, (bf16*)vc, cos_t, sin_t, st, 1, M, nh, slots, max_pos);
    return finish(s);
}

// launch_rope_kv<T> alone.  qkv fp32 [S][M][3 * nh * 128] (slab elements apart); buffers as pg_diag_op_qkv_rope in T (bf16 or fp32).  mode 0 (decode): token m is
// row m (R >= M), slot len[m] + n_dec[0]; mode 1 (prefill): tok_row / tok_j.  The token map goes through the same screen in both modes.
int pg_diag_op_rope_kv(int is_bf16, int mode, const float* qkv, int S, long slab, void* qbuf, void* kc, void* vc, const float* cos_t, const float* sin_t,
                       const int32_t* len, const int32_t* n_dec, const int32_t* tok_row, const int32_t* tok_j, const int32_t* pos_off, int M, int nh, int R,
                       int slots, int max_pos, pg_stream stream) {
    if (!qkv || !qbuf || !kc || !vc || !cos_t || !sin_t || !pos_off) return PG_ERR_ARG;
    if ((mode != 0 && mode != 1) || (mode == 0 && (!len || !n_dec)) || (mode == 1 && (!tok_row || !tok_j))) return PG_ERR_ARG;
    if (M < 1 || nh < 1 || nh > 1024 || R < 1 || (mode == 0 && R < M) || slots < 1 || max_pos < 1 || S < 1 || S > 64) return PG_ERR_ARG;
    if (slab < (long)M * 3 * nh * 128 || (long)R * slots > (1L << 28) || (long)R * nh * slots * 128 >= (1L << 40)) return PG_ERR_ARG;
    if (!aligned16({qkv, qbuf, kc, vc, cos_t, sin_t, len, n_dec, tok_row, tok_j, pos_off})) return PG_ERR_ARG;
    std::vector<int32_t> hrow, hj, hpos, hn;
    if (!to_host(hpos, pos_off, R)) return PG_ERR_HIP;
    if (mode == 0) {
        if (!to_host(hj, len, M) || !to_host(hn, n_dec, 1)) return PG_ERR_HIP;
        if (hn[0] < 0 || hn[0] > (1 << 28)) return PG_ERR_ARG;
        hrow.resize(M);
        for (int m = 0; m < M; ++m) {
            if (hj[m] < 0 || hj[m] > (1 << 28)) return PG_ERR_ARG;
            hrow[m] = m; hj[m] += hn[0];
        }
    } else if (!to_host(hrow, tok_row, M) || !to_host(hj, tok_j, M)) return PG_ERR_HIP;
    const int sc = screen_token_map(hrow, hj, hpos, M, R, slots, max_pos);
    if (sc != PG_OK) return sc;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    SeqState st{len, pos_off, n_dec, tok_row, tok_j, 0, 0, nullptr};
    if (is_bf16) launch_rope_kv<bf16>(s, qkv, S, slab, (bf16*)qbuf, (bf16*)kc, (bf16*)vc, cos_t, sin_t, st, mode, M, nh, slots, max_pos);
    else launch_rope_kv<float>(s, qkv, S, slab, (float*)qbuf, (float*)kc, (float*)vc, cos_t, sin_t, st, mode, M, nh, slots, max_pos);
    return finish(s);
}

// Prefill gate|up projection + SwiGLU.  xn bf16 [M][K], Wgu bf16 [2 I][K] with rows ALREADY [8 gate | 8 up] interleaved, h bf16 [M][I].  form 0: gemm256_try with
// act = 2 as run_layers calls it (gemm256_opt as pg_diag_op_qkv_rope; I % 8 refused: the interleave is in blocks of 8); PG_ERR_ARG when it declines.  form 1:
// launch_gemm<bf16> -> fp32 [M][2 I] (gemm256_opt, or 0 = the 128 x 128 kernel), then launch_silu_mul<bf16> with S = 1.
int pg_diag_op_gemm_swiglu256(int form, int gemm256_opt, const void* xn, const void* Wgu, void* h, int M, int I, int K, pg_stream stream) {
    if (!xn || !Wgu || !h) return PG_ERR_ARG;
    if ((form != 0 && form != 1) || !(opt256_ok(gemm256_opt) || (form == 1 && gemm256_opt == 0))) return PG_ERR_ARG;
    if (M < 1 || M > kMaxGridYZ || I < 8 || (I & 7) || K < 128 || K % 64) return PG_ERR_ARG;                  // silu_mul_kernel: a grid row per token
    if ((long)M * 2 * I >= (1L << 31) || 2L * I * K >= (1L << 31)) return PG_ERR_ARG;
    if (!aligned16({xn, Wgu, h})) return PG_ERR_ARG;
    LocalTune lt;
    lt.t.gemm256 = gemm256_opt;
    const hipStream_t s = (hipStream_t)stream;
    GemmA ga; ga.ptr = xn; ga.lda = K;
    if (form == 0) {
        GemmEpi ge; ge.out = h; ge.out_f32 = 0; ge.ldc = I; ge.act = 2;
        const bool taken = gemm256_try(s, ga, (const bf16*)Wgu, K, 0, ge, M, 2 * I, K, 1, 1, 0);
        const int rc = finish(s);
        return taken ? rc : PG_ERR_ARG;
    }
    Scratch tmp;
    if (!tmp.get((size_t)M * 2 * I * 4)) return PG_ERR_HIP;
    GemmEpi e; e.out = tmp.p; e.out_f32 = 1; e.ldc = 2 * I;
    launch_gemm<bf16>(s, ga, (const bf16*)Wgu, K, 0, e, M, 2 * I, K, 1);
    launch_silu_mul<bf16>(s, (const float*)tmp.p, 1, (long)M * 2 * I, (bf16*)h, M, I);
    return finish(s);
}

// The two weight interleavers (bf16).  kind 0: launch_interleave_qk, src0 [3 * a * 128][b] -> dst (a = nh, b = K; src1 unused).  kind 1:
// launch_convert_interleave16<bf16> with which = 0 on src0 (gate [a][b]) and which = 1 on src1 (up [a][b]) into the one dst [2 a][b] (a = I, b = H).
int pg_diag_op_interleave(int kind, const void* src0, const void* src1, void* dst, int a, int b, pg_stream stream) {
    if (!src0 || !dst || (kind != 0 && kind != 1) || (kind == 1 && !src1)) return PG_ERR_ARG;
    if (a < 1 || b < 8 || (b & 7) || (kind == 0 && a > 1024) || (kind == 1 && (a & 7)) || (kind == 0 ? 384L : 2L) * a * b >= (1L << 31)) return PG_ERR_ARG;
    if (!aligned16({src0, src1, dst})) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (kind == 0) launch_interleave_qk(s, (const bf16*)src0, (bf16*)dst, a, b);
    else {
        launch_convert_interleave16<bf16>(s, src0, 1, (bf16*)dst, a, b, 0);
        launch_convert_interleave16<bf16>(s, src1, 1, (bf16*)dst, a, b, 1);
    }
    return finish(s);
}

// ------------------------------------------------------------------------------------------------ understanding path, input side (tests/test_gpu_vision_ops.py)
// Every entry point below synchronises the stream before it returns.

// LayerNorm over the last dimension: x fp32 [M][C], gamma / beta fp32 [C] -> y [M][C] fp32 or bf16 (launch_layernorm<T>).  form 0: ln_wave = 0, layernorm_kernel
// (a block per row, any C).  form 1: ln_wave = 1, layernorm_wave_kernel<T, 4> -- the launcher takes it at C == 1024 only, so every other C is REFUSED here (a
// caller then knows which kernel ran); its 16-byte row, gamma and beta loads and 8- / 16-byte stores need 16-byte aligned pointers.
int pg_diag_op_layernorm(int out_bf16, int form, const float* x, const float* gamma, const float* beta, void* y, int M, int C, float eps, pg_stream stream) {
    if (!x || !gamma || !beta || !y || (form != 0 && form != 1)) return PG_ERR_ARG;
    if (M < 1 || C < 1 || (long)M * C >= (1L << 40) || !(eps >= 0.f)) return PG_ERR_ARG;
    if (form == 1 && (C != 1024 || !aligned16({x, gamma, beta, y}))) return PG_ERR_ARG;
    LocalTune lt;
    lt.t.ln_wave = form;
    const hipStream_t s = (hipStream_t)stream;
    if (out_bf16) launch_layernorm<bf16>(s, x, gamma, beta, (bf16*)y, M, C, eps);
    else launch_layernorm<float>(s, x, gamma, beta, (float*)y, M, C, eps);
    return finish(s);
}

// PatchEmbed's gather: img NCHW [B][3][S][S] fp32 or bf16 -> out [B (S / ps)^2][3 ps^2] fp32 or bf16, k = (c, py, px) (launch_patchify<T>).  S % ps != 0 is refused:
// the kernel's grid g = S / ps would drop the last partial patch silently.
int pg_diag_op_patchify(int img_bf16, int out_bf16, const void* img, void* out, int B, int S, int ps, pg_stream stream) {
    if (!img || !out || B < 1 || ps < 1 || S < ps || S > 16384 || S % ps) return PG_ERR_ARG;
    if ((long)B * (S / ps) * (S / ps) > 0x7fffffffL) return PG_ERR_ARG;                               // a block per patch
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (out_bf16) launch_patchify<bf16>(s, img, img_bf16, (bf16*)out, B, S, ps);
    else launch_patchify<float>(s, img, img_bf16, (float*)out, B, S, ps);
    return finish(s);
}

// x fp32 [B][P][C] += pos fp32 [P][C] (launch_add_pos).
int pg_diag_op_add_pos(float* x, const float* pos, int B, int P, int C, pg_stream stream) {
    if (!x || !pos || B < 1 || P < 1 || C < 1 || (long)B * P > 0x7fffffffL) return PG_ERR_ARG;      // a block per row
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    launch_add_pos(s, x, pos, B, P, C);
    return finish(s);
}

// The VQ encoder's conv_in (launch_conv3x3_in<T>, Cin = 3): x NCHW [B][3][H][W] fp32 or bf16, w fp32 [Cout][3][3][3], bias fp32 [Cout] -> out NHWC [B][H][W][Cout]
// fp32 or bf16.  The grid is (ceil(W / 64), H, B).
int pg_diag_op_conv_in(int x_bf16, int out_bf16, const void* x, const float* w, const float* bias, void* out, int B, int H, int W, int Cout, pg_stream stream) {
    if (!x || !w || !bias || !out) return PG_ERR_ARG;
    if (B < 1 || B > kMaxGridYZ || H < 1 || H > kMaxGridYZ || W < 1 || Cout < 1 || (long)B * H * W * (Cout > 3 ? Cout : 3) >= (1L << 40)) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (out_bf16) launch_conv3x3_in<bf16>(s, x, x_bf16, w, bias, (bf16*)out, B, H, W, 3, Cout);
    else launch_conv3x3_in<float>(s, x, x_bf16, w, bias, (float*)out, B, H, W, 3, Cout);
    return finish(s);
}

// Nearest code: z fp32 [n][D], cb fp32 [V][D] (already L2-normalised by the caller) -> idx int64 [n].  form 0: vq_argmin_kernel (vq_argmin_multi = 0); form 1:
// vq_argmin_multi_kernel<8> (vq_argmin_multi = 1), refused unless D == 8 && n >= 64 -- the launcher's own condition, so the form names the kernel; form 2:
// launch_vq_argmin under the default tune, as the engine calls it.  D outside [1, 8] is refused: both kernels keep the vector in zn[8], and in the product only
// pg_create's img_dim check stands between a larger D and an overflow of that array.  The eight-vector kernel reads a code as two 16-byte vectors: cb aligned.
int pg_diag_op_vq_argmin(int form, const float* z, const float* cb, int64_t* idx, int n, int D, int V, pg_stream stream) {
    if (!z || !cb || !idx || form < 0 || form > 2) return PG_ERR_ARG;
    if (n < 1 || D < 1 || D > 8 || V < 1 || (long)V * D > 0x7fffffffL) return PG_ERR_ARG;
    const bool multi = D == 8 && n >= 64;
    if (form == 1 && !multi) return PG_ERR_ARG;
    if (form != 0 && multi && ((uintptr_t)cb & 15)) return PG_ERR_ARG;
    LocalTune lt;
    if (form != 2) lt.t.vq_argmin_multi = form;
    const hipStream_t s = (hipStream_t)stream;
    launch_vq_argmin(s, z, cb, idx, n, D, V);
    return finish(s);
}

// dst fp32 [n][D] = src[r] / max(|src[r]|, 1e-12) (launch_l2norm_rows: the codebook's F.normalize).
int pg_diag_op_l2norm_rows(const float* src, float* dst, int n, int D, pg_stream stream) {
    if (!src || !dst || n < 1 || D < 1 || (long)n * D >= (1L << 40)) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    launch_l2norm_rows(s, src, dst, n, D);
    return finish(s);
}

// pg_diag_op_gemm_epi with the second batch level (SigLIP's heads): block (b, b2) reads A + b strideA + b2 strideA2 and W + b strideB + b2 strideB2 and writes at
// out + b strideC + b2 strideC2 (launch_gemm<T>(.., batch, batch2, strideB2); form 0 / 1 / 2 as pg_diag_op_gemm_epi).  With batch2 > 1 no residual and no GroupNorm
// partials (the kernels have no second-level stride for either), and no two output blocks may overlap (blocks_disjoint: strideC2 < ldc, the heads side by
// side inside a row, included).
int pg_diag_op_gemm_heads(int engine_bf16, int form, const void* A, long lda, long strideA, const void* W, long ldb, long strideB, void* out, int out_f32, long ldc,
                          long strideC, const float* bias_n, const float* bias_m, const void* residual, int res_f32, long ldr, long strideR, float scale, int act,
                          int M, int N, int K, int batch, int batch2, long strideA2, long strideB2, long strideC2, int gn_hw, float* ws, long ws_floats,
                          float* stats, float eps, int* nsplit_out, pg_stream stream) {
    return gemm_epi_impl(engine_bf16, form, A, lda, strideA, W, ldb, strideB, out, out_f32, ldc, strideC, bias_n, bias_m, residual, res_f32, ldr, strideR, scale, act,
                         M, N, K, batch, batch2, strideA2, strideB2, strideC2, gn_hw, ws, ws_floats, stats, eps, nsplit_out, stream);
}

// ------------------------------------------------------------------------------------------------ decode GEMM dispatch (tests/test_gpu_skinny_ops.py)
// The skinny decode GEMMs through their production launchers.  x bf16 [M][K], W_rowmajor bf16 [N][K].  form 0: launch_gemm_skinny with a tiled copy built by
// launch_tile_weights, as pg_finalize_weights / pg_op_gemm kind 4 do (the decode dispatch: v4, v3 on the tiled copy); form 1: launch_gemm_skinny with Wt == nullptr
// (row-major v3, which falls back to v1 when the chunk count has no instantiation); out fp32 [S][M][N], slab s at out + s M N.  form 2 / 3: launch_gemm_skinny_swiglu
// with / without the tiled copy, S == 1, W rows already [8 gate | 8 up] interleaved, out bf16 [M][N / 2]; PG_ERR_ARG, out untouched, when the launcher has no fused
// instantiation for the shape.  stream_gemm: PgTune::stream_gemm (-1 auto, else the bit mask of gemm.hip sk4_prod).  S is the caller's, not skinny_pick_splits'.
// M <= 512 is what pg_engine::gemm_llm sends this way.  Synchronises the stream before it returns.
int pg_diag_op_gemm_skinny(int form, int stream_gemm, const void* x, const void* W_rowmajor, void* out, int M, int N, int K, int S, pg_stream stream) {
    if (!x || !W_rowmajor || !out || form < 0 || form > 3) return PG_ERR_ARG;
    if (!aligned16({x, W_rowmajor, out})) return PG_ERR_ARG;                                          // 16-byte x / W loads (LDS-DMA in v4), 16-byte slab stores
    if (M < 1 || M > 512 || N < 16 || (N & 15) || K < SK_BK || (K % SK_BK) || S < 1 || (K / SK_BK) % S) return PG_ERR_ARG;
    if ((long)N * K > 0x7fffffffL || (form >= 2 && S != 1)) return PG_ERR_ARG;
    LocalTune lt;
    lt.t.stream_gemm = stream_gemm;
    const hipStream_t s = (hipStream_t)stream;
    Scratch wt;
    if (form == 0 || form == 2) {
        if (!wt.get((size_t)N * K * 2)) return PG_ERR_HIP;
        launch_tile_weights(s, (const bf16*)W_rowmajor, (bf16*)wt.p, N, K);
    }
    bool ok = true;
    if (form < 2) launch_gemm_skinny(s, (const bf16*)x, (const bf16*)W_rowmajor, (float*)out, M, N, K, S, (const bf16*)wt.p);
    else ok = launch_gemm_skinny_swiglu(s, (const bf16*)x, (const bf16*)W_rowmajor, (bf16*)out, M, N, K, (const bf16*)wt.p);
    const int rc = finish(s);                                                                        // before the tiled copy goes away
    return ok ? rc : PG_ERR_ARG;
}

// ------------------------------------------------------------------------------------------------ the samplers' draw (tests/test_gpu_draws.py)
// The image sampler's step through its production launcher, launch_cfg_step (the filtered route when filtered != 0), on the caller's buffers.
// partial fp32: slab s at partial + s * slab, rows [2B][V] (row 2b = cond, 2b + 1 = uncond), slab >= 2 B V; bias fp32 [V] or null; force_tok int32 [B_total][T] or
// null (has_force), force_mask uint8 [B_total][T] or null (has_mask; needs force_tok); out_tok int32 [B_total][T]; logits_out fp32 [T][B_total][V] or null (then
// step < T); embed_table fp32 [V][H]; x fp32 [2B][H].  The launch covers images [b_off, b_off + B) of B_total.  SampleParams, the step counter, the 16 B winner
// slots and (filtered) the mixed rows are allocated here.  Synchronises the stream before it returns.
int pg_diag_op_cfg_sample(int filtered, const float* partial, int S, long slab, const float* bias, int V, int B, const int32_t* force_tok, const uint8_t* force_mask,
                          int32_t* out_tok, float* logits_out, const float* embed_table, float* x, int H, float cfg_weight, float temperature, uint64_t seed,
                          int top_k, float top_p, int T, int step, int img_off, int b_off, int B_total, pg_stream stream) {
    if (!partial || !out_tok || !embed_table || !x || (force_mask && !force_tok)) return PG_ERR_ARG;
    if (S < 1 || V < 1 || B < 1 || B > kMaxGridYZ / 2 || H < 4 || (H & 3) || T < 1 || step < 0 || img_off < 0 || b_off < 0 || B_total < 1) return PG_ERR_ARG;
    if ((long)b_off + B > B_total || slab < 2L * B * V || (long)V * H >= (1L << 40) || !aligned16({embed_table, x})) return PG_ERR_ARG;
    if (logits_out && step >= T) return PG_ERR_ARG;                                                  // the tap has T steps
    if (!(cfg_weight == cfg_weight) || !(temperature == temperature)) return PG_ERR_ARG;
    if (filtered && (V > SEL_MAXV || !(temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f))) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    SampleParams p{};
    p.cfg_weight = cfg_weight; p.temperature = temperature; p.seed = seed; p.T = T; p.img_off = img_off; p.top_k = top_k; p.top_p = top_p;
    SamplerStep st;
    const int rc = st.setup(s, p, filtered != 0, partial, S, slab, bias, V, B, force_tok, force_mask, out_tok, logits_out, embed_table, x, H, step, b_off, B_total);
    if (rc != PG_OK) return rc;
    st.launch(s, nullptr, nullptr, 2, B, filtered != 0, false);
    return finish(s);                                                                                // before the scratch goes away
}

// pg_diag_op_cfg_sample under a sample plan (tests/test_gpu_sample_plan_ops.py): device plan arrays in place of the five scalars -- w fp32 [B_total][T],
// temperature fp32 / top_k int32 / top_p fp32 / key int32 [B_total], all indexed by the global image b_off + b -- through launch_cfg_step's planned route.  filtered != 0
// takes the store -> select -> pick route (the caller says so: the arrays live on the device; V <= SEL_MAXV); stored != 0 also runs the store scan on the
// unfiltered route.  Everything else as pg_diag_op_cfg_sample.
int pg_diag_op_cfg_sample_plan(int filtered, int stored, const float* partial, int S, long slab, const float* bias, int V, int B, const int32_t* force_tok,
                               const uint8_t* force_mask, int32_t* out_tok, float* logits_out, const float* embed_table, float* x, int H, const float* w_dev,
                               const float* temperature_dev, const int32_t* top_k_dev, const float* top_p_dev, const int32_t* key_dev, uint64_t seed, int T,
                               int step, int b_off, int B_total, pg_stream stream) {
    if (!partial || !out_tok || !embed_table || !x || (force_mask && !force_tok)) return PG_ERR_ARG;
    if (!w_dev || !temperature_dev || !top_k_dev || !top_p_dev || !key_dev) return PG_ERR_ARG;
    if (S < 1 || V < 1 || B < 1 || B > kMaxGridYZ / 2 || H < 4 || (H & 3) || T < 1 || step < 0 || b_off < 0 || B_total < 1) return PG_ERR_ARG;
    if ((long)b_off + B > B_total || slab < 2L * B * V || (long)V * H >= (1L << 40) || !aligned16({embed_table, x})) return PG_ERR_ARG;
    if (logits_out && step >= T) return PG_ERR_ARG;                                                  // the tap has T steps
    if (filtered && V > SEL_MAXV) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    SampleParams p{};
    p.seed = seed; p.T = T; p.top_p = 1.f;
    SamplerStep st;
    const int rc = st.setup(s, p, filtered || stored, partial, S, slab, bias, V, B, force_tok, force_mask, out_tok, logits_out, embed_table, x, H, step, b_off, B_total);
    if (rc != PG_OK) return rc;
    const SamplePlanDev plan{w_dev, temperature_dev, top_k_dev, top_p_dev, key_dev};
    st.launch(s, &plan, nullptr, 2, B, filtered != 0, stored != 0);
    return finish(s);                                                                                // before the scratch goes away
}

// One dual-guidance step (tests/test_gpu_dual_ops.py) through launch_cfg_step at three rows per image: rows [3B][V] per slab (3b = f, 3b + 1 = p, 3b + 2 = u), slab >= 3 B V, x fp32
// [3B][H].  filtered != 0: store scan -> select -> pick (V <= SEL_MAXV, temperature > 0); stored != 0: the unfiltered route also runs the store scan.  mix_out
// fp32 [B][V] or null: the mixed rows the store scan left (filtered or stored).  Everything else as pg_diag_op_cfg_sample.
int pg_diag_op_cfg3_sample(int filtered, int stored, const float* partial, int S, long slab, const float* bias, int V, int B, const int32_t* force_tok,
                           const uint8_t* force_mask, int32_t* out_tok, float* logits_out, float* mix_out, const float* embed_table, float* x, int H, float w_caption,
                           float w_layout, float temperature, uint64_t seed, int top_k, float top_p, int T, int step, int img_off, int b_off, int B_total,
                           pg_stream stream) {
    if (!partial || !out_tok || !embed_table || !x || (force_mask && !force_tok)) return PG_ERR_ARG;
    if (S < 1 || V < 1 || B < 1 || B > kMaxGridYZ / 3 || H < 4 || (H & 3) || T < 1 || step < 0 || img_off < 0 || b_off < 0 || B_total < 1) return PG_ERR_ARG;
    if ((long)b_off + B > B_total || slab < 3L * B * V || (long)V * H >= (1L << 40) || !aligned16({embed_table, x})) return PG_ERR_ARG;
    if (logits_out && step >= T) return PG_ERR_ARG;                                                  // the tap has T steps
    if (!(w_caption == w_caption) || !(w_layout == w_layout) || !(temperature == temperature)) return PG_ERR_ARG;
    if (filtered && (V > SEL_MAXV || !(temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f))) return PG_ERR_ARG;
    if (mix_out && !filtered && !stored) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    SampleParams p{};
    p.cfg_weight = w_caption; p.temperature = temperature; p.seed = seed; p.T = T; p.img_off = img_off; p.top_k = top_k; p.top_p = top_p;
    SamplerStep st;
    Scratch dw;
    if (!dw.get(sizeof(DualWeights))) return PG_ERR_HIP;
    const int rc = st.setup(s, p, filtered || stored, partial, S, slab, bias, V, B, force_tok, force_mask, out_tok, logits_out, embed_table, x, H, step, b_off, B_total);
    if (rc != PG_OK) return rc;
    launch_set_dual_weights(s, (DualWeights*)dw.p, DualWeights{w_caption, w_layout});
    st.launch(s, nullptr, (const DualWeights*)dw.p, 3, B, filtered != 0, stored != 0);
    if (mix_out && hipMemcpyAsync(mix_out, st.mix.p, (size_t)B * V * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return PG_ERR_HIP;
    return finish(s);                                                                                // before the scratch goes away
}

// The text sampler's step through launch_text_argmax (mode 0) or launch_text_sample (mode 1: the in-scan Gumbel draw, temperature > 0).  partial fp32: slab s at
// partial + s * slab, rows [B][V], slab >= B V -- an odd slab or V sends the scan down its scalar branch, multiples of 4 down the 16-byte one (then partial and
// logits_out are 16-byte aligned).  out int64 [B][max_new] (written when step < max_new); unfinished int32 [B] in / out; logits_out fp32 [max_new][B][V] or null
// (then step < max_new); embed_table fp32 [V][H]; x fp32 [B][H].  TextParams, the step counter, the winner slots and the any-unfinished ring are allocated here.
// Synchronises the stream before it returns.
int pg_diag_op_text_draw(int mode, const float* partial, int S, long slab, int V, int B, int64_t* out, int32_t* unfinished, float* logits_out,
                         const float* embed_table, float* x, int H, int eos, int min_new, int max_new, int step, float temperature, uint64_t seed, int row_off,
                         pg_stream stream) {
    if (!partial || !out || !unfinished || !embed_table || !x || (mode != 0 && mode != 1)) return PG_ERR_ARG;
    if (S < 1 || V < 1 || B < 1 || B > kMaxGridYZ || H < 4 || (H & 3) || max_new < 1 || min_new < 0 || step < 0 || row_off < 0) return PG_ERR_ARG;
    if (slab < (long)B * V || (long)V * H >= (1L << 40) || !aligned16({embed_table, x})) return PG_ERR_ARG;
    if (((V | (int)(slab & 3)) & 3) == 0 && !aligned16({partial, logits_out})) return PG_ERR_ARG;     // the 16-byte branch of the scan
    if (logits_out && step >= max_new) return PG_ERR_ARG;                                            // the tap has max_new steps
    if (mode == 1 && !(temperature > 0.f)) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    Scratch tp, nd, pv, pi, any;
    if (!tp.get(sizeof(TextParams)) || !nd.get(4) || !pv.get((size_t)B * 16 * 4) || !pi.get((size_t)B * 16 * 4) || !any.get(1024 * 4)) return PG_ERR_HIP;
    if (hipMemsetAsync(any.p, 0, 1024 * 4, s) != hipSuccess) return PG_ERR_HIP;
    TextParams p{};
    p.eos = eos; p.min_new = min_new; p.max_new = max_new; p.temperature = temperature; p.top_p = 1.f; p.row_off = row_off; p.seed = seed;
    launch_set_text_op_params(s, (TextParams*)tp.p, p, (int32_t*)nd.p, step);
    TextArgs a{};
    a.logits_partial = partial; a.S = S; a.slab = slab; a.V = V; a.p = (const TextParams*)tp.p; a.out = out; a.unfinished = unfinished;
    a.any_unfinished = (int32_t*)any.p; a.embed_table = embed_table; a.x = x; a.H = H; a.n_dec = (const int32_t*)nd.p; a.logits_out = logits_out;
    if (mode == 1) launch_text_sample(s, a, B, (float*)pv.p, (int*)pi.p);
    else launch_text_argmax(s, a, B, (float*)pv.p, (int*)pi.p);
    return finish(s);                                                                                // before the scratch goes away
}

// ------------------------------------------------------------------------------------------------ weight converters and row movers (tests/test_gpu_load_ops.py)
// Every entry point below synchronises the stream before it returns.

// The converters of pg_engine::load_tensor: src fp32 or bf16 (src_bf16) -> dst fp32 or bf16 (dst_bf16).  kind 0: launch_convert<T> on n elements (T = float is
// launch_to_f32 too); *kernel_out = 1 when launch_convert's own condition sends the call to convert_f32_bf16_vec_kernel (fp32 -> bf16, n >= 65536, n % 8 == 0, both
// pointers 16-byte aligned), 0 = convert_kernel<T>.  kind 1: launch_convert_conv<T>, src [a = Cout][b = Cin][c = kk] -> dst [Cout][kk][Cin].  kind 2:
// launch_convert_interleave16<T>, src [a = I][b = H] -> rows (r / 8) * 16 + which * 8 + r % 8 of dst [2 I][H]; I % 8 != 0 is refused (the last block's rows would
// fall behind row 2 I - 1).  Pointers must be aligned to their element.
int pg_diag_op_convert(int kind, int src_bf16, int dst_bf16, const void* src, void* dst, long n, int a, int b, int c, int which, int* kernel_out,
                       pg_stream stream) {
    if (!src || !dst || kind < 0 || kind > 2 || (src_bf16 != 0 && src_bf16 != 1) || (dst_bf16 != 0 && dst_bf16 != 1)) return PG_ERR_ARG;
    if (((uintptr_t)src & (src_bf16 ? 1 : 3)) || ((uintptr_t)dst & (dst_bf16 ? 1 : 3))) return PG_ERR_ARG;
    if (kind == 0) {
        if (n < 1 || n >= (1L << 40) || !kernel_out) return PG_ERR_ARG;
    } else {
        if (a < 1 || b < 1 || (long)a * b >= (1L << 40)) return PG_ERR_ARG;
        if (kind == 1 && (c < 1 || (long)a * b * c >= (1L << 40))) return PG_ERR_ARG;
        if (kind == 2 && ((a & 7) || (which != 0 && which != 1))) return PG_ERR_ARG;
    }
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    if (kind == 0) {
        *kernel_out = dst_bf16 && !src_bf16 && n % 8 == 0 && n >= 65536 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;      // launch_convert's condition, restated
        if (dst_bf16) launch_convert<bf16>(s, src, src_bf16, (bf16*)dst, n);
        else if (which) launch_to_f32(s, src, src_bf16, (float*)dst, n);                                      // which = 1: through launch_to_f32 (the K_F32 slots)
        else launch_convert<float>(s, src, src_bf16, (float*)dst, n);
    } else if (kind == 1) {
        if (dst_bf16) launch_convert_conv<bf16>(s, src, src_bf16, (bf16*)dst, a, b, c);
        else launch_convert_conv<float>(s, src, src_bf16, (float*)dst, a, b, c);
    } else {
        if (dst_bf16) launch_convert_interleave16<bf16>(s, src, src_bf16, (bf16*)dst, a, b, which);
        else launch_convert_interleave16<float>(s, src, src_bf16, (float*)dst, a, b, which);
    }
    return finish(s);
}

// launch_lora_merge<T> (pg_merge_lora's kernel, tests/test_gpu_lora_ops.py) on the caller's device buffers: W fp32 or bf16 (w_bf16), updated in place, [out][in]
// row-major (layout 0 = K_T) or the gate (2 = K_IL16_G) / up (3 = K_IL16_U) rows of a [2 out][in] interleaved buffer (out % 8 == 0); A fp32 [r][in], B fp32
// [out][r]; any out, in, r >= 1.  W must be aligned to its element, A and B to 4 bytes.
int pg_diag_op_lora_merge(int w_bf16, int layout, void* W, int out, int in, const float* A, const float* B, int r, float scale, pg_stream stream) {
    if (!W || !A || !B || (w_bf16 != 0 && w_bf16 != 1) || out < 1 || in < 1 || r < 1) return PG_ERR_ARG;
    if (((uintptr_t)W & (w_bf16 ? 1 : 3)) || (((uintptr_t)A | (uintptr_t)B) & 3)) return PG_ERR_ARG;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    const bool ok = w_bf16 ? launch_lora_merge<bf16>(s, (bf16*)W, layout, out, in, A, B, r, scale)
                           : launch_lora_merge<float>(s, (float*)W, layout, out, in, A, B, r, scale);
    if (!ok) return PG_ERR_ARG;
    return finish(s);
}
}  // extern "C"
namespace {
// idx [n] device (or null: the identity, n <= rows) inside [0, rows); distinct: no value twice (a scatter's rows must not race)
int screen_rows(const int32_t* idx, int n, long rows, bool distinct) {
    if (!idx) return n <= rows ? PG_OK : PG_ERR_ARG;
    std::vector<int32_t> h;
    if (!to_host(h, idx, n)) return PG_ERR_HIP;
    std::vector<char> seen(distinct ? (size_t)rows : 0, 0);
    for (int i = 0; i < n; ++i) {
        if (h[i] < 0 || h[i] >= rows) return PG_ERR_ARG;
        if (distinct) { if (seen[h[i]]) return PG_ERR_ARG; seen[h[i]] = 1; }
    }
    return PG_OK;
}
}  // namespace
extern "C" {

// The row movers.  n rows are moved; width = H elements (ops 0, 2 - 5), row_bytes (op 1) or L (op 6).  src has src_rows rows and dst dst_rows; an index vector
// ([n] int32 device, or null = the identity) is copied back and screened against them before anything is launched, a scatter's for duplicates too.
//   0  launch_embed_gather: src = table fp32 [src_rows = vocab][H], ids [n_ids] (ANY value: the kernel clamps to [0, vocab - 1]), src_idx [n] into ids or null
//      (then n <= n_ids), dst fp32 [dst_rows >= n][H].  The kernel moves 16-byte vectors: H % 4 != 0 or a table / dst that is not 16-byte aligned is refused.
//   1  launch_copy_rows: src [src_rows][row_bytes] gathered by src_idx, dst [dst_rows][row_bytes] scattered by dst_idx.  The kernel copies 32-bit words and counts
//      them in an int: row_bytes % 4 != 0, row_bytes / 4 > INT_MAX or a pointer that is not 4-byte aligned is refused.
//   2  launch_rows_to_f32: src fp32 / bf16 (src_bf16) [src_rows][H] gathered by src_idx -> dst fp32 [dst_rows >= n][H].
//   3  launch_f32_to_rows, 4 launch_t_to_rows<float>, 5 launch_t_to_rows<bf16>: src fp32 (5: bf16) [src_rows >= n][H] -> dst fp32 / bf16 (dst_bf16) [dst_rows][H]
//      scattered by dst_idx.
//   6  launch_rows_differ: ids [src_rows][L]; dst = flag int32 [1] |= 1 when a row first, first + stride, ... (n rows) differs from row ref in columns [from, L).
int pg_diag_op_rows(int op, const void* src, void* dst, const int32_t* ids, int n_ids, const int32_t* src_idx, const int32_t* dst_idx, int n, long width,
                    long src_rows, long dst_rows, int src_bf16, int dst_bf16, int first, int stride, int ref, int from, pg_stream stream) {
    if (op < 0 || op > 6 || !dst || (op != 6 && !src) || n < 1 || width < 1 || src_rows < 1 || dst_rows < 1) return PG_ERR_ARG;
    if ((src_bf16 != 0 && src_bf16 != 1) || (dst_bf16 != 0 && dst_bf16 != 1)) return PG_ERR_ARG;
    if (op != 1 && width > 0x7fffffffL) return PG_ERR_ARG;
    const int H = (int)(op == 1 ? 0 : width);
    int rc = PG_OK;
    switch (op) {
        case 0:
            if (!ids || n_ids < 1 || dst_idx || (H & 3) || (((uintptr_t)src | (uintptr_t)dst) & 15) || n > dst_rows || src_rows > 0x7fffffffL) return PG_ERR_ARG;
            rc = screen_rows(src_idx, n, n_ids, false);
            break;
        case 1:
            if ((width & 3) || width / 4 > 0x7fffffffL || (((uintptr_t)src | (uintptr_t)dst) & 3)) return PG_ERR_ARG;
            rc = screen_rows(src_idx, n, src_rows, false);
            if (rc == PG_OK) rc = screen_rows(dst_idx, n, dst_rows, true);
            break;
        case 2:
            if (dst_idx || n > dst_rows || ((uintptr_t)src & (src_bf16 ? 1 : 3)) || ((uintptr_t)dst & 3)) return PG_ERR_ARG;
            rc = screen_rows(src_idx, n, src_rows, false);
            break;
        case 3: case 4: case 5:
            if (src_idx || n > src_rows || ((uintptr_t)src & (op == 5 ? 1 : 3)) || ((uintptr_t)dst & (dst_bf16 ? 1 : 3))) return PG_ERR_ARG;
            rc = screen_rows(dst_idx, n, dst_rows, true);
            break;
        default:
            if (!ids || src_idx || dst_idx || first < 0 || stride < 1 || ref < 0 || ref >= src_rows || from < 0 || from > width) return PG_ERR_ARG;
            if ((long)first + (long)(n - 1) * stride >= src_rows || (((uintptr_t)ids | (uintptr_t)dst) & 3)) return PG_ERR_ARG;
            break;
    }
    if (rc != PG_OK) return rc;
    LocalTune lt;
    const hipStream_t s = (hipStream_t)stream;
    switch (op) {
        case 0: launch_embed_gather(s, (const float*)src, ids, src_idx, (float*)dst, n, H, (int)src_rows); break;
        case 1: launch_copy_rows(s, src, src_idx, dst, dst_idx, n, width); break;
        case 2: launch_rows_to_f32(s, src, src_bf16, src_idx, (float*)dst, n, H); break;
        case 3: launch_f32_to_rows(s, (const float*)src, dst, dst_bf16, dst_idx, n, H); break;
        case 4: launch_t_to_rows<float>(s, (const float*)src, dst, dst_bf16, dst_idx, n, H); break;
        case 5: launch_t_to_rows<bf16>(s, (const bf16*)src, dst, dst_bf16, dst_idx, n, H); break;
        default: launch_rows_differ(s, ids, H, first, stride, ref, n, from, (int32_t*)dst); break;
    }
    return finish(s);
}

}  // extern "C"
