#include <cstdlib>
// Language-model side kernels (HBM-bound, wave64): fused split-K-reduce + residual + RMSNorm,
// RoPE + KV append, decode attention with per-lane-group online softmax, SwiGLU gate,
// gen_head activation, fused CFG-mix + argmax / Gumbel-max sampling + next-embedding gather.
// References: SURVEY.md K1-K9, a6.1-a6.4, a7-a9 (third-party transformers Llama formulas).
#include <type_traits>
#include "kernels.h"
#include "attn_decode.h"      // sum_slabs + the fused decode-attention kernel template


// ------------------------------------------------------------------------------- RMSNorm
// One 256-thread block per row.  x += sum_s partial[s]; xn = w * (x * rsqrt(mean(x^2)+eps)).
// LlamaRMSNorm: stats in fp32, normalised value cast to the input dtype (fp32 residual
// stream here) before the weight multiply; the product is rounded once to T.
// Register-resident fast path: H <= NV*1024, thread holds NV float4 (no LDS row buffer), all
// (S+1)*NV loads are independent and issued up front, weights / outputs moved as 8- or 16-byte
// vectors.
template <typename T, int NV, int SB = 4>
__global__ __launch_bounds__(256) void rmsnorm_kernel(float* __restrict__ x, const float* __restrict__ partial,
                                                     int S, long slab, const T* __restrict__ w,
                                                     T* __restrict__ xn, int H, float eps, int32_t* __restrict__ advance) {
    __shared__ float red[4];
    rmsnorm_row<T, NV, false, SB>(blockIdx.x, x, partial, S, slab, w, xn, H, eps, red);
    // the decode step's LAST kernel also advances the device step counter (no kernel of the step reads it after this
    // point; saves the 1-thread advance launch of every step)
    if (advance && blockIdx.x == 0 && threadIdx.x == 0) *advance += 1;
}
// 512 threads per row (H = 2048: one f32x4 per thread and slab): twice the waves issue the row's loads
template <typename T, int SB>
__global__ __launch_bounds__(512) void rmsnorm512_kernel(float* __restrict__ x, const float* __restrict__ partial, const T* __restrict__ w,
                                                        T* __restrict__ xn, int32_t* __restrict__ advance, int S, int slab, int H, float eps) {
    // 5 pointers + 4 x 32 bits = 56 bytes: the whole kernarg block is preloaded into SGPRs at wave launch (see attn_decode.h); slab (elements
    // of one split-K slab, M x N <= 2^31) travels as int for that
    __shared__ float red[8];
    rmsnorm_row<T, 1, false, SB, 512>(blockIdx.x, x, partial, S, (long)slab, w, xn, H, eps, red);
    if (advance && blockIdx.x == 0 && threadIdx.x == 0) *advance += 1;
}
template <typename T>
void launch_rmsnorm(hipStream_t s, float* x, const float* partial, int S, long slab, const T* w, T* xn,
                    int M, int H, float eps, int32_t* advance) {
    if (M <= 0) return;
    // rmsnorm512_kernel carries the slab stride as a 32-bit int (56-byte preloaded kernarg block): a stride that does not fit -- M x H >= 2^31,
    // i.e. >= 2^20 rows at H = 2048, only reachable through pg_op_rmsnorm -- takes the long-stride kernel below
    if (H == 2048 && (S == 0 || slab <= 0x7fffffffL)) {   // every row count (the reduction order must not depend on M: sharded == unsharded tokens); decode loop -8 ms at bs=64, -7 ms at bs=8 vs 256 threads per row
        // S == 0 (prefill: o / down add into the residual stream in their GEMM epilogues, 13 k rows per launch): no slab loads at all -- the
        // branch-free decode form would read every row four more times (-6 us of 34 per launch at the bench's packed batch)
        if (S == 0) hipLaunchKernelGGL((rmsnorm512_kernel<T, 0>), dim3(M), dim3(512), 0, s, x, partial, w, xn, advance, S, (int)slab, H, eps);
        else if (S > 4) hipLaunchKernelGGL((rmsnorm512_kernel<T, 8>), dim3(M), dim3(512), 0, s, x, partial, w, xn, advance, S, (int)slab, H, eps);
        else hipLaunchKernelGGL((rmsnorm512_kernel<T, 4>), dim3(M), dim3(512), 0, s, x, partial, w, xn, advance, S, (int)slab, H, eps);
        return;
    }
    if (H <= 1024) hipLaunchKernelGGL((rmsnorm_kernel<T, 1>), dim3(M), dim3(256), 0, s, x, partial, S, slab, w, xn, H, eps, advance);
    else if (H <= 2048 && S > 4) hipLaunchKernelGGL((rmsnorm_kernel<T, 2, 8>), dim3(M), dim3(256), 0, s, x, partial, S, slab, w, xn, H, eps, advance);   // 5-8 slabs (small row counts): still one round trip
    else if (H <= 2048) hipLaunchKernelGGL((rmsnorm_kernel<T, 2>), dim3(M), dim3(256), 0, s, x, partial, S, slab, w, xn, H, eps, advance);
    else if (H <= 4096) hipLaunchKernelGGL((rmsnorm_kernel<T, 4>), dim3(M), dim3(256), 0, s, x, partial, S, slab, w, xn, H, eps, advance);
    else hipLaunchKernelGGL((rmsnorm_kernel<T, 8>), dim3(M), dim3(256), 0, s, x, partial, S, slab, w, xn, H, eps, advance);
}
// Deferred-1/rms form of the decode norm (round 6; H = 2048, bf16): NO block reduction, no barrier.  Block = 256 threads = half a row, every thread
// one f32x4 of x and of each slab (all loads up front, added in the SAME order as rmsnorm_row: the residual stream keeps its bits), stores the
// updated residual, xw = bf16(x . w) -- the consumer GEMM's A operand WITHOUT the 1/rms -- and each WAVE leaves the sum of squares of its 256
// columns in ssq[row][half * 4 + wave] (8 partials per row, summed in fixed order by the consumer: deterministic, no atomics).  2 M blocks instead
// of M: twice the waves have the row's loads in flight, and the kernel's tail is a store, not a reduction.
template <int SB>
__global__ __launch_bounds__(256) void rmsnorm_defer_kernel(float* __restrict__ x, const float* __restrict__ partial, const bf16* __restrict__ w,
                                                           bf16* __restrict__ xw, float* __restrict__ ssq, int S, int slab, int H) {
    const int tid = threadIdx.x, m = blockIdx.x >> 1, half = blockIdx.x & 1;
    const int i = half * 1024 + tid * 4;
    float* xr = x + (long)m * H + i;
    const u32x2 wv = *(const u32x2*)(w + i);
    f32x4 v = *(const f32x4*)xr;
    f32x4 t[SB];
    const float* pp = partial + (long)m * H + i;
    const int smax = S - 1;
#pragma unroll
    for (int u = 0; u < SB; ++u) t[u] = *(const f32x4*)(pp + (long)(u < smax ? u : smax) * slab);
#pragma unroll
    for (int u = 0; u < SB; ++u) if (u < S) v += t[u];
    float ss = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    *(f32x4*)xr = v;
    u32x2 ov; ov.x = pack_bf16x2(bf16_lo(wv.x) * v.x, bf16_hi(wv.x) * v.y); ov.y = pack_bf16x2(bf16_lo(wv.y) * v.z, bf16_hi(wv.y) * v.w);
    *(u32x2*)(xw + (long)m * H + i) = ov;
    ss = wave_sum(ss);
    if ((tid & 63) == 0) ssq[m * 8 + half * 4 + (tid >> 6)] = ss;
}
void launch_rmsnorm_defer(hipStream_t s, float* x, const float* partial, int S, long slab, const bf16* w, bf16* xw, float* ssq, int M, int H) {
    // contract (checked by the caller through deferred_norm_ok + the engine): H == 2048, 1 <= S <= 8, slab fits 32 bits
    if (S > 4) hipLaunchKernelGGL((rmsnorm_defer_kernel<8>), dim3(2 * M), dim3(256), 0, s, x, partial, w, xw, ssq, S, (int)slab, H);
    else hipLaunchKernelGGL((rmsnorm_defer_kernel<4>), dim3(2 * M), dim3(256), 0, s, x, partial, w, xw, ssq, S, (int)slab, H);
}
template void launch_rmsnorm<float>(hipStream_t, float*, const float*, int, long, const float*, float*, int, int, float, int32_t*);
template void launch_rmsnorm<bf16>(hipStream_t, float*, const float*, int, long, const bf16*, bf16*, int, int, float, int32_t*);

// ------------------------------------------------------------------------------- row movers
// dst[t] = table[ids[src_idx ? src_idx[t] : t]]   (K1; packed left-pad-free gather)
__global__ void embed_gather_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                    const int32_t* __restrict__ src_idx, float* __restrict__ dst, int H, int vocab) {
    const int t = blockIdx.x;
    int id = ids[src_idx ? src_idx[t] : t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const float* src = table + (long)id * H;
    for (int i = threadIdx.x * 4; i < H; i += blockDim.x * 4)
        *(f32x4*)(dst + (long)t * H + i) = *(const f32x4*)(src + i);
}
void launch_embed_gather(hipStream_t s, const float* table, const int32_t* ids, const int32_t* src_idx, float* dst,
                         int n, int H, int vocab) {
    if (n <= 0) return;
    hipLaunchKernelGGL(embed_gather_kernel, dim3(n), dim3(256), 0, s, table, ids, src_idx, dst, H, vocab);
}
// byte-row copy with optional gather (src_idx) / scatter (dst_idx); row_bytes % 4 == 0
__global__ void copy_rows_kernel(const uint32_t* __restrict__ src, const int32_t* __restrict__ src_idx,
                                 uint32_t* __restrict__ dst, const int32_t* __restrict__ dst_idx, int row_words) {
    const int t = blockIdx.x;
    const long rs = src_idx ? src_idx[t] : t, rd = dst_idx ? dst_idx[t] : t;
    for (int i = threadIdx.x; i < row_words; i += blockDim.x) dst[rd * row_words + i] = src[rs * row_words + i];
}
void launch_copy_rows(hipStream_t s, const void* src, const int32_t* src_idx, void* dst, const int32_t* dst_idx,
                      int n, long row_bytes) {
    if (n <= 0) return;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(n), dim3(256), 0, s, (const uint32_t*)src, src_idx, (uint32_t*)dst, dst_idx, (int)(row_bytes / 4));
}

__global__ void rows_to_f32_kernel(const void* __restrict__ src, int src_bf16, const int32_t* __restrict__ src_row,
                                   float* __restrict__ dst, int H) {
    const int t = blockIdx.x;
    const long r = src_row ? src_row[t] : t;
    for (int i = threadIdx.x; i < H; i += blockDim.x) {
        float v = src_bf16 ? ET<bf16>::ld((const bf16*)src + r * H + i) : ((const float*)src)[r * H + i];
        dst[(long)t * H + i] = v;
    }
}
void launch_rows_to_f32(hipStream_t s, const void* src, int src_bf16, const int32_t* src_row, float* dst, int n, int H) {
    if (n <= 0) return;
    hipLaunchKernelGGL(rows_to_f32_kernel, dim3(n), dim3(256), 0, s, src, src_bf16, src_row, dst, H);
}
template <typename TS>
__global__ void t_to_rows_kernel(const TS* __restrict__ src, void* __restrict__ dst, int dst_bf16,
                                 const int32_t* __restrict__ dst_row, int H) {
    const int t = blockIdx.x;
    const long r = dst_row ? dst_row[t] : t;
    for (int i = threadIdx.x; i < H; i += blockDim.x) {
        const float v = ET<TS>::ld(src + (long)t * H + i);
        if (dst_bf16) ET<bf16>::st((bf16*)dst + r * H + i, v); else ((float*)dst)[r * H + i] = v;
    }
}
void launch_f32_to_rows(hipStream_t s, const float* src, void* dst, int dst_bf16, const int32_t* dst_row, int n, int H) {
    if (n <= 0) return;
    hipLaunchKernelGGL(t_to_rows_kernel<float>, dim3(n), dim3(256), 0, s, src, dst, dst_bf16, dst_row, H);
}
template <typename T>
void launch_t_to_rows(hipStream_t s, const T* src, void* dst, int dst_bf16, const int32_t* dst_row, int n, int H) {
    if (n <= 0) return;
    hipLaunchKernelGGL(t_to_rows_kernel<T>, dim3(n), dim3(256), 0, s, src, dst, dst_bf16, dst_row, H);
}
template void launch_t_to_rows<float>(hipStream_t, const float*, void*, int, const int32_t*, int, int);
template void launch_t_to_rows<bf16>(hipStream_t, const bf16*, void*, int, const int32_t*, int, int);

// flag |= any(ids[row][from..L) != ids[ref][from..L)) over rows first, first+stride, ... (n rows): the
// batch-constant negative prompt probe of pg_prefill (plangen_base.py:673-686 builds every uncond row from
// the same neg_prompt; verified, not assumed).
__global__ void rows_differ_kernel(const int32_t* __restrict__ ids, int L, int first, int stride, int ref, int from, int32_t* __restrict__ flag) {
    const int32_t* a = ids + (long)(first + blockIdx.x * stride) * L;
    const int32_t* b = ids + (long)ref * L;
    int diff = 0;
    for (int j = from + threadIdx.x; j < L; j += blockDim.x) diff |= a[j] != b[j];
    if (diff) atomicOr(flag, 1);
}
void launch_rows_differ(hipStream_t s, const int32_t* ids, int L, int first, int stride, int ref, int n, int from, int32_t* flag) {
    if (n <= 0) return;
    hipLaunchKernelGGL(rows_differ_kernel, dim3(n), dim3(256), 0, s, ids, L, first, stride, ref, from, flag);
}

// ------------------------------------------------------------------------------- RoPE + KV append
// grid (M tokens, nh/4), 256 threads = 4 heads x 64 rotation pairs.  rotate_half form
// (half-split, not interleaved): out[j] = x[j]cos - x[j+64]sin, out[j+64] = x[j+64]cos + x[j]sin.
template <typename T>
__global__ __launch_bounds__(256) void rope_kv_kernel(const float* __restrict__ qkv, int S, long slab,
                                                     T* __restrict__ qbuf, T* __restrict__ kc, T* __restrict__ vc,
                                                     const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                     SeqState st, int mode, int nh, int slots, int max_pos) {
    const int m = blockIdx.x, head = blockIdx.y * 4 + (threadIdx.x >> 6), j = threadIdx.x & 63;
    if (head >= nh) return;
    int row, slot;
    if (mode == 0) { row = m; slot = st.len[m] + *st.n_dec; }
    else { row = st.tok_row[m]; slot = st.tok_j[m]; }
    int pos = st.pos_off[row] + slot;
    if (pos >= max_pos) pos = max_pos - 1;
    if (slot >= slots) return;                                     // capacity guard (host checks too)
    const int HD = nh * 128;
    const long base = (long)m * 3 * HD + head * 128 + j;
    float a6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int o6[6] = {0, 64, HD, HD + 64, 2 * HD, 2 * HD + 64};
    sum_slabs<6>(qkv + base, slab, S, o6, a6);
    const float q0 = a6[0], q1 = a6[1], k0 = a6[2], k1 = a6[3], v0 = a6[4], v1 = a6[5];
    const float c = cos_t[(long)pos * 64 + j], sn = sin_t[(long)pos * 64 + j];
    T* qo = qbuf + (long)m * HD + head * 128 + j;
    ET<T>::st(qo, rope_lo(q0, q1, c, sn));
    ET<T>::st(qo + 64, rope_hi(q0, q1, c, sn));
    const long co = (((long)row * nh + head) * slots + slot) * 128 + j;
    ET<T>::st(kc + co, rope_lo(k0, k1, c, sn));
    ET<T>::st(kc + co + 64, rope_hi(k0, k1, c, sn));
    ET<T>::st(vc + co, v0);
    ET<T>::st(vc + co + 64, v1);
}
template <typename T>
void launch_rope_kv(hipStream_t s, const float* qkv, int S, long slab, T* qbuf, T* kc, T* vc,
                    const float* cos_t, const float* sin_t, SeqState st, int mode, int M, int nh,
                    int slots, int max_pos) {
    if (M <= 0) return;
    hipLaunchKernelGGL(rope_kv_kernel<T>, dim3(M, (nh + 3) / 4), dim3(256), 0, s, qkv, S, slab, qbuf, kc, vc,
                       cos_t, sin_t, st, mode, nh, slots, max_pos);
}
template void launch_rope_kv<float>(hipStream_t, const float*, int, long, float*, float*, float*, const float*, const float*, SeqState, int, int, int, int, int);
template void launch_rope_kv<bf16>(hipStream_t, const float*, int, long, bf16*, bf16*, bf16*, const float*, const float*, SeqState, int, int, int, int, int);

// ------------------------------------------------------------------------------- attention
// One 256-thread block per (query, head); head_dim = 128.  HBM-bound streaming of that
// (row, head)'s K and V (contiguous [slot][128]).  Each 16-byte vector load covers EPV
// elements of one key; LPK = 128/EPV lanes cover a key, so one wave load instruction covers
// KPI = 64/LPK keys (bf16: 4 keys, fp32: 2).  Every LPK-lane group runs its OWN online
// softmax over the keys it sees (no cross-lane max exchange inside the loop); the
// 4 waves x KPI groups partial states (m, l, o[128]) are merged once through LDS.
template <typename T, int UN, bool NT>
__global__ __launch_bounds__(256) void attn_kernel(const T* __restrict__ qbuf, T* __restrict__ obuf,
                                                  const T* __restrict__ kc, const T* __restrict__ vc,
                                                  SeqState st, int mode, int nh, int slots, float scale) {
    constexpr int EPV = ET<T>::EPV, LPK = 128 / EPV, KPI = 64 / LPK, NST = 4 * KPI;
    __shared__ float s_o[NST][128];
    __shared__ float s_m[NST], s_l[NST];
    const int qi = blockIdx.x, head = blockIdx.y;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int grp = l / LPK, lk = l % LPK;                // key group in wave, lane within key
    int row, klen;
    if (mode == 0) { row = qi; klen = st.len[qi] + *st.n_dec + 1; }
    else { row = st.tok_row[qi]; klen = st.tok_j[qi] + 1; }
    if (klen > slots) klen = slots;
    const int HD = nh * 128;
    float q[EPV];
    {
        const u32x4 qv = *(const u32x4*)(qbuf + (long)qi * HD + head * 128 + lk * EPV);
        ET<T>::unpack(qv, q);
#pragma unroll
        for (int e = 0; e < EPV; ++e) q[e] *= scale;
    }
    const T* kb = kc + ((long)row * nh + head) * slots * 128 + lk * EPV;
    const T* vb = vc + ((long)row * nh + head) * slots * 128 + lk * EPV;
    float m_run = -INFINITY, l_run = 0.f, o[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) o[e] = 0.f;

    constexpr int KPW = KPI * UN;                          // keys per wave iteration
    for (int base = w * KPW; base < klen; base += 4 * KPW) {
        u32x4 kv[UN], vv[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            int key = base + u * KPI + grp;
            key = key < klen ? key : klen - 1;             // clamp: load stays in bounds
            kv[u] = NT ? __builtin_nontemporal_load((const u32x4*)(kb + (long)key * 128)) : *(const u32x4*)(kb + (long)key * 128);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            int key = base + u * KPI + grp;
            key = key < klen ? key : klen - 1;
            vv[u] = NT ? __builtin_nontemporal_load((const u32x4*)(vb + (long)key * 128)) : *(const u32x4*)(vb + (long)key * 128);
        }
        float sc[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            float kf[EPV]; ET<T>::unpack(kv[u], kf);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < EPV; ++e) d = fmaf(q[e], kf[e], d);
#pragma unroll
            for (int o_ = LPK / 2; o_ > 0; o_ >>= 1) d += __shfl_xor(d, o_, 64);
            sc[u] = (base + u * KPI + grp < klen) ? d : -INFINITY;
        }
        float mx = m_run;
#pragma unroll
        for (int u = 0; u < UN; ++u) mx = fmaxf(mx, sc[u]);
        if (mx > -INFINITY) {
            const float alpha = __expf(m_run - mx);        // m_run=-inf -> 0
            l_run *= alpha;
#pragma unroll
            for (int e = 0; e < EPV; ++e) o[e] *= alpha;
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const float p = __expf(sc[u] - mx);        // -inf -> 0
                l_run += p;
                float vf[EPV]; ET<T>::unpack(vv[u], vf);
#pragma unroll
                for (int e = 0; e < EPV; ++e) o[e] = fmaf(p, vf[e], o[e]);
            }
            m_run = mx;
        }
    }
    const int stt = w * KPI + grp;
#pragma unroll
    for (int e = 0; e < EPV; ++e) s_o[stt][lk * EPV + e] = o[e];
    if (lk == 0) { s_m[stt] = m_run; s_l[stt] = l_run; }
    __syncthreads();
    if (tid < 128) {
        float M = -INFINITY;
#pragma unroll
        for (int i = 0; i < NST; ++i) M = fmaxf(M, s_m[i]);
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const float f = (s_m[i] > -INFINITY) ? __expf(s_m[i] - M) : 0.f;
            num = fmaf(f, s_o[i][tid], num);
            den = fmaf(f, s_l[i], den);
        }
        ET<T>::st(obuf + (long)qi * HD + head * 128 + tid, num / den);
    }
}
template <typename T>
void launch_attn_decode_fused(hipStream_t s, const float* qkv, int S, long slab, T* obuf, T* kc, T* vc,
                              const float* cos_t, const float* sin_t, SeqState st, int M, int nh, int slots,
                              int max_pos, float scale) {
    if (M <= 0) return;
    // The software-pipelined loop (template argument ABL = 16): 8-wave blocks 5 deep when the launch has few (row, head) blocks (small batch:
    // 2x the K/V bytes in flight per CU), 4-wave blocks 6 deep otherwise (7 deep spills in the pipelined form).  Only these two forms are
    // instantiated in libplangen_hip.so; the older non-pipelined kernel and the timing ablations live in libplangen_diag.so (diag_attn.hip),
    // which registers itself in PgTune::diag.
    // (the measurement forms know nothing of group_rows: a grouped launch never goes through them -- they would read the replicas' never-written prompt slots)
    if (st.group_rows <= 0 && pg_tune->diag && pg_tune->diag->attn_decode && pg_tune->diag->attn_decode(s, std::is_same<T, bf16>::value, qkv, S, slab, obuf, kc, vc, cos_t, sin_t, st, M, nh, slots, max_pos, scale)) return;
#define ATT_LAUNCH(U, W, A) hipLaunchKernelGGL((attn_decode_fused_kernel<T, U, W, A>), dim3(nh, M), dim3(64 * W), 0, s, st.row_order, st.len, st.n_dec, kc, vc, nh, slots, st.shared_len, st.shared_row, qkv, slab, obuf, cos_t, sin_t, st.pos_off, S, max_pos, scale)
    // grouped form (SeqState::group_rows > 0, pg_prefill_replicated alias = 1): the same two block shapes, chosen the same way, with the one extra argument
#define ATT_LAUNCH_GRP(U, W, A) hipLaunchKernelGGL((attn_decode_fused_kernel<T, U, W, A, true, int>), dim3(nh, M), dim3(64 * W), 0, s, st.row_order, st.len, st.n_dec, kc, vc, nh, slots, st.shared_len, st.shared_row, qkv, slab, obuf, cos_t, sin_t, st.pos_off, S, max_pos, scale, st.group_rows)
    const bool small = (M * nh <= 512 && pg_tune->attn_waves != 4) || pg_tune->attn_waves == 8;
    if (st.group_rows > 0) {
        if (small) ATT_LAUNCH_GRP(5, 8, 16);
        else ATT_LAUNCH_GRP(6, 4, 16);
    }
    else if (small) ATT_LAUNCH(5, 8, 16);
    else ATT_LAUNCH(6, 4, 16);
#undef ATT_LAUNCH_GRP
#undef ATT_LAUNCH
}
template void launch_attn_decode_fused<float>(hipStream_t, const float*, int, long, float*, float*, float*, const float*, const float*, SeqState, int, int, int, int, float);
template void launch_attn_decode_fused<bf16>(hipStream_t, const float*, int, long, bf16*, bf16*, bf16*, const float*, const float*, SeqState, int, int, int, int, float);

// FP8 KV cache (kv8.h): the same two block forms as launch_attn_decode_fused, chosen the same way.  kvs: interleaved (K, V) scales.
void launch_attn_decode_kv8(hipStream_t s, const float* qkv, int S, long slab, bf16* obuf, uint8_t* kc, uint8_t* vc, float* kvs,
                            const float* cos_t, const float* sin_t, SeqState st, int M, int nh, int slots, int max_pos, float scale) {
    if (M <= 0) return;
#define ATT8_LAUNCH(U, W) hipLaunchKernelGGL((attn_decode_kv8_kernel<U, W>), dim3(nh, M), dim3(64 * W), 0, s, st.row_order, st.len, st.n_dec, kc, vc, nh, slots, st.shared_len, st.shared_row, kvs, qkv, slab, obuf, cos_t, sin_t, st.pos_off, S, max_pos, scale)
#define ATT8_LAUNCH_GRP(U, W) hipLaunchKernelGGL((attn_decode_kv8_kernel<U, W, true, int>), dim3(nh, M), dim3(64 * W), 0, s, st.row_order, st.len, st.n_dec, kc, vc, nh, slots, st.shared_len, st.shared_row, kvs, qkv, slab, obuf, cos_t, sin_t, st.pos_off, S, max_pos, scale, st.group_rows)
    const bool small = (M * nh <= 512 && pg_tune->attn_waves != 4) || pg_tune->attn_waves == 8;
    if (st.group_rows > 0) {
        if (small) ATT8_LAUNCH_GRP(KV8_UN_SMALL, 8);
        else ATT8_LAUNCH_GRP(KV8_UN_BIG, 4);
    }
    else if (small) ATT8_LAUNCH(KV8_UN_SMALL, 8);
    else ATT8_LAUNCH(KV8_UN_BIG, 4);
#undef ATT8_LAUNCH_GRP
#undef ATT8_LAUNCH
}

// pg_prefill_replicated with alias = 0: the owner's prompt K/V -> every replica's own row.  One block per (replica row, head, plane); a plane is
// one layer's K or V block (or one layer's scale block, FP8 cache), rows [R0, R) are the replicas of rows [0, R0): owner = row % R0.  Rows that
// alias the shared uncond prompt (odd, shared_len > 0) hold no prompt of their own and are skipped.  VB = bytes per load / store (16; 8 for
// the FP8 scales, whose [slot][2] fp32 pairs are 8 bytes per slot).
template <int VB>
__global__ __launch_bounds__(256) void kv_replicate_kernel(char* __restrict__ base, long plane_bytes, long rowhead_bytes, int slot_bytes,
                                                           const int32_t* __restrict__ len_p, int R0, int nh, int shared_len) {
    typedef typename std::conditional<VB == 16, u32x4, u32x2>::type V;
    const int head = blockIdx.x, row = R0 + (int)blockIdx.y;
    if (shared_len > 0 && (row & 1)) return;
    const long n = (long)len_p[row] * slot_bytes / VB;
    char* const plane = base + (long)blockIdx.z * plane_bytes;
    const V* src = (const V*)(plane + ((long)(row % R0) * nh + head) * rowhead_bytes);
    V* dst = (V*)(plane + ((long)row * nh + head) * rowhead_bytes);
    for (long i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}
void launch_kv_replicate(hipStream_t s, void* base, long plane_bytes, int planes, long rowhead_bytes, int slot_bytes, const int32_t* len,
                         int R0, int R, int nh, int shared_len) {
    if (R <= R0 || planes <= 0) return;
    const dim3 grid(nh, R - R0, planes);
    if (slot_bytes % 16 == 0)
        hipLaunchKernelGGL(kv_replicate_kernel<16>, grid, dim3(256), 0, s, (char*)base, plane_bytes, rowhead_bytes, slot_bytes, len, R0, nh, shared_len);
    else
        hipLaunchKernelGGL(kv_replicate_kernel<8>, grid, dim3(256), 0, s, (char*)base, plane_bytes, rowhead_bytes, slot_bytes, len, R0, nh, shared_len);
}

// n rows of 128 bf16 -> 128 codes + one scale each (one wave per row)
__global__ __launch_bounds__(256) void kv_quantize_rows_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ codes, float* __restrict__ scale, long n) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    kv8_quant_row(x + i * 128, codes + i * 128, scale + i, threadIdx.x & 63);
}
void launch_kv_quantize_rows(hipStream_t s, const bf16* x, uint8_t* codes, float* scale, long n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(kv_quantize_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, codes, scale, n);
}
// prefill -> FP8 cache: one wave per (packed token, head, K | V) converts that row of the one-layer bf16 scratch [R][nh][slots][128] into
// the layer's codes (same layout) and scale.  Indexed by the packed tokens, so aliased uncond rows and empty slots are never touched.
__global__ __launch_bounds__(256) void kv_quantize_kernel(const bf16* __restrict__ ksrc, const bf16* __restrict__ vsrc, uint8_t* __restrict__ kc,
                                                         uint8_t* __restrict__ vc, float* __restrict__ kvs, const int32_t* __restrict__ tok_row,
                                                         const int32_t* __restrict__ tok_j, long nitems, int nh, int slots) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nitems) return;
    const int isv = (int)(i & 1);
    const long th = i >> 1;
    const int head = (int)(th % nh);
    const long tok = th / nh;
    const int j = tok_j[tok];
    if (j >= slots) return;                                       // capacity guard, as rope_kv_kernel
    const long idx = ((long)tok_row[tok] * nh + head) * slots + j;
    kv8_quant_row((isv ? vsrc : ksrc) + idx * 128, (isv ? vc : kc) + idx * 128, kvs + idx * 2 + isv, threadIdx.x & 63);
}
// debug tap: dst[i] = kvs[2 i + which] (the K or the V scales out of the interleaved array)
__global__ void kv8_scale_plane_kernel(const float* __restrict__ kvs, int which, float* __restrict__ dst, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = kvs[2 * i + which];
}
void launch_kv8_scale_plane(hipStream_t s, const float* kvs, int which, float* dst, long n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(kv8_scale_plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kvs, which, dst, n);
}
void launch_kv_quantize(hipStream_t s, const bf16* ksrc, const bf16* vsrc, uint8_t* kc, uint8_t* vc, float* kvs, const int32_t* tok_row,
                        const int32_t* tok_j, int ntok, int nh, int slots) {
    const long nitems = (long)ntok * nh * 2;
    if (nitems <= 0) return;
    hipLaunchKernelGGL(kv_quantize_kernel, dim3((unsigned)((nitems + 3) / 4)), dim3(256), 0, s, ksrc, vsrc, kc, vc, kvs, tok_row, tok_j, nitems, nh, slots);
}

template <typename T>
void launch_attn(hipStream_t s, const T* qbuf, T* obuf, const T* kc, const T* vc, SeqState st, int mode,
                 int M, int nh, int slots, float scale) {
    if (M <= 0) return;
    dim3 grid(M, nh), block(256);
    // decode (mode 0): 8 keys per lane group in flight, non-temporal K/V loads (read once per step); prefill: cached loads
    if (mode == 0) hipLaunchKernelGGL((attn_kernel<T, 8, true>), grid, block, 0, s, qbuf, obuf, kc, vc, st, mode, nh, slots, scale);
    else hipLaunchKernelGGL((attn_kernel<T, 8, false>), grid, block, 0, s, qbuf, obuf, kc, vc, st, mode, nh, slots, scale);
}
template void launch_attn<float>(hipStream_t, const float*, float*, const float*, const float*, SeqState, int, int, int, int, float);
template void launch_attn<bf16>(hipStream_t, const bf16*, bf16*, const bf16*, const bf16*, SeqState, int, int, int, int, float);

// ------------------------------------------------------------------------------- SwiGLU gate
// gu columns are interleaved in blocks of 8: [8 gate | 8 up] per 16 columns (= one MFMA n-tile).
template <typename T>
__global__ void silu_mul_kernel(const float* __restrict__ gu, int S, long slab, T* __restrict__ h, int I) {
    const int m = blockIdx.y;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= I) return;
    const long cg = (long)m * 2 * I + (n >> 3) * 16 + (n & 7);
    float a2[2] = {0.f, 0.f};
    const int o2[2] = {0, 8};
    sum_slabs<2>(gu + cg, slab, S, o2, a2);
    const float g = a2[0], u = a2[1];
    ET<T>::st(h + (long)m * I + n, (g / (1.f + expf(-g))) * u);
}
template <typename T>
void launch_silu_mul(hipStream_t s, const float* gu, int S, long slab, T* h, int M, int I) {
    if (M <= 0) return;
    hipLaunchKernelGGL(silu_mul_kernel<T>, dim3((I + 255) / 256, M), dim3(256), 0, s, gu, S, slab, h, I);
}
template void launch_silu_mul<float>(hipStream_t, const float*, int, long, float*, int, int);
template void launch_silu_mul<bf16>(hipStream_t, const float*, int, long, bf16*, int, int);

template <typename T>
__global__ void bias_act_kernel(const float* __restrict__ partial, int S, long slab, const float* __restrict__ bias,
                                T* __restrict__ out, int N, int act) {
    const int m = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float a1[1] = {bias ? bias[n] : 0.f};
    const int o1[1] = {0};
    sum_slabs<1>(partial + (long)m * N + n, slab, S, o1, a1);
    float v = a1[0];
    if (act == 1) v = gelu_erf(v);
    ET<T>::st(out + (long)m * N + n, v);
}
template <typename T>
void launch_bias_act(hipStream_t s, const float* partial, int S, long slab, const float* bias, T* out,
                     int M, int N, int act) {
    if (M <= 0) return;
    hipLaunchKernelGGL(bias_act_kernel<T>, dim3((N + 255) / 256, M), dim3(256), 0, s, partial, S, slab, bias, out, N, act);
}
template void launch_bias_act<float>(hipStream_t, const float*, int, long, const float*, float*, int, int, int);
template void launch_bias_act<bf16>(hipStream_t, const float*, int, long, const float*, bf16*, int, int, int);
void launch_bias_f32(hipStream_t s, const float* partial, int S, long slab, const float* bias, float* out, int M, int N) {
    launch_bias_act<float>(s, partial, S, slab, bias, out, M, N, 0);
}

// ------------------------------------------------------------------------------- CFG + sample
// One block per image b (rows 2b = cond, 2b+1 = uncond).  mixed = u + w (c - u)
// (plangen_base.py:587); greedy: first index of the max (torch.argmax tie rule);
// temperature > 0: Gumbel-max == multinomial(softmax(mixed / T)).  Then the chosen (or
// forced) token's precomputed gen_aligner(gen_embed(tok)) row is written to both CFG rows
// of the residual stream (plangen_base.py:602-604).
__device__ __forceinline__ void argmax_combine(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// Stage 1: grid (CFG_CHUNKS, B): each block scans V/CFG_CHUNKS logits of image b and leaves its
// local (value, index) winner; stage 2 (one block per image) combines the winners, applies the
// forcing rules and gathers the next embedding.
#define CFG_CHUNKS 16
// the sampler's perturbed value: Gumbel-max over mixed / T (cfg_scan_kernel and the filtered sampler's cfg_select_kernel
// draw through this one expression, so a filtered draw equals the unfiltered one whenever that one survives the filter)
__device__ __forceinline__ float gumbel_perturb(float mixed, float invT, uint64_t seed, uint64_t stream, int v) {
    const float uu = rng_uniform(seed, stream, v);
    return mixed * invT - __logf(-__logf(uu));
}
// STORE (filtered sampler): also write the CFG-mixed row to mix [B, V] and leave the draw to cfg_select_kernel
// PLAN (pg_request_sample_plan): the block's image reads its own temperature, key and this step's weight from the plan's device arrays, once,
// in front of the loop; everything else is the same code.  The plain instantiations take the plain SampleArgs.
template <bool STORE, bool PLAN = false>
__global__ __launch_bounds__(256) void cfg_scan_kernel(typename std::conditional<PLAN, SampleArgsPlan, SampleArgs>::type a, float* __restrict__ pv,
                                                       int* __restrict__ pi, float* __restrict__ mix) {
    __shared__ float sv[4]; __shared__ int si[4];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    const int bg = b + a.b_off, B = a.B_total;            // global image index (lane-independent results)
    const int per = (a.V + CFG_CHUNKS - 1) / CFG_CHUNKS, v0 = ch * per, v1 = min(a.V, v0 + per);
    const long rc = (long)(2 * b) * a.V, ru = (long)(2 * b + 1) * a.V;
    float best = -INFINITY; int bi = 0x7fffffff;
    float temperature, cfg_weight; uint64_t stream;
    if constexpr (PLAN) {
        const int T = a.p->T;
        temperature = a.plan.temperature[bg];
        cfg_weight = a.plan.w[(long)bg * T + (step < T ? step : T - 1)];
        stream = (uint64_t)a.plan.key[bg] * 1000003ull + step;
    } else {
        temperature = a.p->temperature; cfg_weight = a.p->cfg_weight;
        stream = (uint64_t)(bg + a.p->img_off) * 1000003ull + step;
    }
    const uint64_t seed = a.p->seed;
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    // four vocabulary entries per thread per pass, ALL their loads (bias, cond / uncond row of every slab) issued before the first use
    // (indices clamped into the chunk): one memory round trip per pass instead of one per entry
    constexpr int IT = 4;
    const float* bias0 = a.bias ? a.bias : a.logits_partial + rc;     // no bias: any mapped address, value discarded
    const int ocu[2] = {0, a.V};                                      // cond row, uncond row (adjacent rows)
    for (int vb = v0 + tid; vb < v1; vb += IT * 256) {
        float bb[IT], cu[IT][2];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256, vc = v < v1 ? v : v1 - 1;
            bb[it] = bias0[vc];
        }
        float t[IT][4][2];
        const int smax = a.S > 0 ? a.S - 1 : 0;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256, vc = v < v1 ? v : v1 - 1;
            const float* pp = a.logits_partial + rc + vc;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* q = pp + (long)(u < smax ? u : smax) * a.slab;       // slab index clamped: branch-free loads
                t[it][u][0] = q[0]; t[it][u][1] = q[a.V];
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256, vc = v < v1 ? v : v1 - 1;
            cu[it][0] = a.bias ? bb[it] : 0.f; cu[it][1] = cu[it][0];
#pragma unroll
            for (int u = 0; u < 4; ++u) if (u < a.S) { cu[it][0] += t[it][u][0]; cu[it][1] += t[it][u][1]; }
            if (a.S > 4) sum_slabs<2>(a.logits_partial + rc + vc + 4 * a.slab, a.slab, a.S - 4, ocu, cu[it]);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256;
            if (v < v1) {
                const float c = cu[it][0], u = cu[it][1];
                float mixed = u + cfg_weight * (c - u);
                if (a.logits_out) a.logits_out[((long)step * B + bg) * a.V + v] = mixed;
                if (STORE) { mix[(long)b * a.V + v] = mixed; continue; }
                if (temperature > 0.f) mixed = gumbel_perturb(mixed, invT, seed, stream, v);
                if (mixed > best) { best = mixed; bi = v; }
            }
        }
    }
    if (STORE) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        argmax_combine(best, bi, ov, oi);
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = sv[0]; int i = si[0];
        for (int k = 1; k < 4; ++k) argmax_combine(v, i, sv[k], si[k]);
        pv[b * CFG_CHUNKS + ch] = v; pi[b * CFG_CHUNKS + ch] = i;
    }
}
__global__ __launch_bounds__(256) void cfg_pick_kernel(SampleArgs a, const float* __restrict__ pv, const int* __restrict__ pi) {
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    if (tid == 0) {
        float v = pv[b * CFG_CHUNKS]; int i = pi[b * CFG_CHUNKS];
        for (int k = 1; k < CFG_CHUNKS; ++k) argmax_combine(v, i, pv[b * CFG_CHUNKS + k], pi[b * CFG_CHUNKS + k]);
        i = i < 0 ? 0 : (i >= a.V ? a.V - 1 : i);
        int emit = i, feed = i;
        const long bg = b + a.b_off;
        const int T = a.p->T;
        if (step < T && a.p->has_force) {
            const int f = a.force_tok[bg * T + step];
            if (a.p->has_mask) { if (a.force_mask[bg * T + step] == 0) { emit = f; feed = f; } }
            else feed = f;
        }
        if (step < T) a.out_tok[bg * T + step] = emit;
        feed = feed < 0 ? 0 : (feed >= a.V ? a.V - 1 : feed);
        s_tok = feed;
    }
    __syncthreads();
    const float* src = a.embed_table + (long)s_tok * a.H;
    float* x0 = a.x + (long)(2 * b) * a.H;
    for (int i = tid * 4; i < a.H; i += 1024) {
        const f32x4 v = *(const f32x4*)(src + i);
        *(f32x4*)(x0 + i) = v;
        *(f32x4*)(x0 + a.H + i) = v;
    }
}
__global__ void set_sample_params_kernel(SampleParams* dst, SampleParams v) { *dst = v; }
void launch_set_sample_params(hipStream_t s, SampleParams* dst, SampleParams v) { hipLaunchKernelGGL(set_sample_params_kernel, dim3(1), dim3(1), 0, s, dst, v); }
__global__ void set_text_params_kernel(TextParams* dst, TextParams v) { *dst = v; }
void launch_set_text_params(hipStream_t s, TextParams* dst, TextParams v) { hipLaunchKernelGGL(set_text_params_kernel, dim3(1), dim3(1), 0, s, dst, v); }
void launch_cfg_sample(hipStream_t s, const SampleArgs& a, int B, float* scratch_v, int* scratch_i) {
    hipLaunchKernelGGL(cfg_scan_kernel<false>, dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, (float*)nullptr);
    hipLaunchKernelGGL(cfg_pick_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}

// ------------------------------------------------------------------------------- top-k / top-p sampler
// One 1024-thread block per image over its row x = mixed * invT (kept in LDS as the raw mixed values).
// Keys: order-preserving fp32 -> uint32 (NaN -> -inf, -0 -> +0).  top-k threshold tk = the k-th largest key, by an
// MSB-first radix select (8-bit digits, LDS count histograms, wave-0 prefix over the 256 buckets).  top-p threshold
// tp = the smallest key whose strictly-larger survivors (key >= tk) hold < top_p of their exp-mass: the same radix walk
// over mass histograms.  Masses are w = exp(x - max) in 2^-40 fixed point (64-bit integer sums: the result does not depend
// on the order of the LDS atomics).  Kept: key >= max(tk, tp) and x > -inf.  Then the Gumbel-max of cfg_scan_kernel
// over the kept set (same noise, same tie rule) -> slot 0 of the stage-1 winners cfg_pick_kernel combines.
__device__ __forceinline__ uint32_t sel_key(float mixed, float invT) {
    float x = mixed * invT;
    if (x != x) x = -INFINITY;
    if (x == 0.f) x = 0.f;
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
#define SEL_THREADS 1024
#define SEL_KEY_NEGINF 0x007fffffu                   // sel_key(-inf)
#define SEL_MASS_ONE 1099511627776.f                 // 2^40
__device__ __forceinline__ unsigned long long sel_mass(uint32_t key, float m) {
    const float x = sel_unkey(key);
    const float w = m == INFINITY ? (x == INFINITY ? 1.f : 0.f) : expf(x - m);
    return (unsigned long long)(w * SEL_MASS_ONE);
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// PLAN: image b + b_off takes its temperature, (top_k, top_p) and key from the plan.  A greedy image (temperature <= 0) ignores its filter and is the
// plain first-index argmax of the row, an image with (0, 1) keeps everything: both leave the winner the unfiltered scan would leave (nothing to
// choose from -> the out-of-range index that cfg_pick_kernel clamps, not the filtered form's token 0).
template <bool PLAN>
__global__ __launch_bounds__(SEL_THREADS) void cfg_select_kernel(typename std::conditional<PLAN, FilterArgsPlan, FilterArgs>::type f) {
    __shared__ float vals[SEL_MAXV];
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long mhist[256];
    __shared__ uint32_t s_max, s_digit, s_rem;
    __shared__ unsigned long long s_z, s_above;
    __shared__ float wv[SEL_THREADS / 64]; __shared__ int wi[SEL_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, V = f.V;
    float temperature; int top_k; float top_p;
    if constexpr (PLAN) {
        const int bg = b + f.b_off;
        temperature = f.plan.temperature[bg];
        const bool greedy = !(temperature > 0.f);
        top_k = greedy ? 0 : f.plan.top_k[bg]; top_p = greedy ? 1.f : f.plan.top_p[bg];
    } else {
        temperature = f.p ? f.p->temperature : f.temperature;
        top_k = f.p ? f.p->top_k : f.top_k;
        top_p = f.p ? f.p->top_p : f.top_p;
    }
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const float* row = f.mix + (long)b * V;
    if (tid == 0) { s_max = 0; s_z = 0; }
    uint32_t kmax = 0;
    for (int v = tid; v < V; v += SEL_THREADS) {
        const float m = row[v];
        vals[v] = m;
        const uint32_t k = sel_key(m, invT);
        kmax = k > kmax ? k : kmax;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(kmax, o, 64); kmax = t > kmax ? t : kmax; }
    __syncthreads();
    if (lane == 0) atomicMax(&s_max, kmax);
    // ---- top-k: the key of the k-th largest entry
    uint32_t tk = 0;
    if (top_k > 0 && top_k < V) {
        uint32_t prefix = 0, pmask = 0, rem = (uint32_t)top_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int v = tid; v < V; v += SEL_THREADS) {
                const uint32_t k = sel_key(vals[v], invT);
                if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {          // lane l holds digits 255-4l .. 252-4l (descending): bucket of the rem-th largest
                uint32_t h[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = hist[255 - 4 * lane - j]; sum += h[j]; }
                uint32_t incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                uint32_t before = incl - sum;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (before < rem && before + h[j] >= rem) { s_digit = 255 - 4 * lane - j; s_rem = rem - before; }
                    before += h[j];
                }
            }
            __syncthreads();
            prefix |= s_digit << shift; pmask |= 255u << shift; rem = s_rem;
        }
        tk = prefix;
    }
    __syncthreads();
    const uint32_t kmx = s_max;
    // ---- top-p over the top-k survivors
    uint32_t tp = 0;
    if (top_p < 1.f && kmx > SEL_KEY_NEGINF) {
        const float m = sel_unkey(kmx);
        unsigned long long z = 0;
        for (int v = tid; v < V; v += SEL_THREADS) {
            const uint32_t k = sel_key(vals[v], invT);
            if (k >= tk) z += sel_mass(k, m);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += shfl_xor_u64(z, o);
        if (lane == 0) atomicAdd(&s_z, z);
        __syncthreads();
        const double limit = (double)top_p * (double)s_z;
        uint32_t prefix = 0, pmask = 0;
        unsigned long long above = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) { hist[tid] = 0; mhist[tid] = 0; }
            __syncthreads();
            for (int v = tid; v < V; v += SEL_THREADS) {
                const uint32_t k = sel_key(vals[v], invT);
                if (k >= tk && (k & pmask) == prefix) {
                    const uint32_t d = (k >> shift) & 255u;
                    atomicAdd(&hist[d], 1u);
                    const unsigned long long q = sel_mass(k, m);
                    if (q) atomicAdd(&mhist[d], q);
                }
            }
            __syncthreads();
            if (tid < 64) {          // lowest non-empty bucket whose strictly-larger mass is < limit
                uint32_t c[4]; unsigned long long mm[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * lane - j]; mm[j] = mhist[255 - 4 * lane - j]; sum += mm[j]; }
                unsigned long long incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = shfl_up_u64(incl, o); if (lane >= o) incl += t; }
                unsigned long long cum = above + incl - sum;
                int dj = -1; unsigned long long cj = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (c[j] && (double)cum < limit) { dj = 255 - 4 * lane - j; cj = cum; }
                    cum += mm[j];
                }
                const unsigned long long has = __ballot(dj >= 0);
                if (dj >= 0 && lane == 63 - __clzll(has)) { s_digit = (uint32_t)dj; s_above = cj; }
            }
            __syncthreads();
            prefix |= s_digit << shift; pmask |= 255u << shift; above = s_above;
        }
        tp = prefix;
    }
    uint32_t tau = tk > tp ? tk : tp;
    tau = tau > SEL_KEY_NEGINF + 1 ? tau : SEL_KEY_NEGINF + 1;
    // ---- kept mask (operator) / Gumbel-max over the kept set (sampler)
    float best = -INFINITY; int bi = 0x7fffffff;
    uint64_t seed = 0, stream = 0;
    if (f.pv) {
        const int step = *f.n_dec;
        seed = f.p->seed;
        if constexpr (PLAN) stream = (uint64_t)f.plan.key[b + f.b_off] * 1000003ull + step;
        else stream = (uint64_t)(b + f.b_off + f.p->img_off) * 1000003ull + step;
    }
    for (int v = tid; v < V; v += SEL_THREADS) {
        const float mv = vals[v];
        const bool kept = sel_key(mv, invT) >= tau;
        if (f.keep) f.keep[(long)b * V + v] = kept;
        if (f.pv && kept) {
            const float g = (PLAN && !(temperature > 0.f)) ? mv : gumbel_perturb(mv, invT, seed, stream, v);
            if (g > best) { best = g; bi = v; }
        }
    }
    if (!f.pv) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        argmax_combine(best, bi, ov, oi);
    }
    if (lane == 0) { wv[tid >> 6] = best; wi[tid >> 6] = bi; }
    __syncthreads();
    if (tid < CFG_CHUNKS) {
        float v = -INFINITY; int i = 0x7fffffff;
        if (tid == 0) {
            v = wv[0]; i = wi[0];
            for (int w = 1; w < SEL_THREADS / 64; ++w) argmax_combine(v, i, wv[w], wi[w]);
            if (i == 0x7fffffff && !(PLAN && top_k <= 0 && !(top_p < 1.f))) i = 0;          // nothing kept (every entry -inf / NaN): token 0
        }
        f.pv[b * CFG_CHUNKS + tid] = v; f.pi[b * CFG_CHUNKS + tid] = i;
    }
}
void launch_cfg_sample_filtered(hipStream_t s, const SampleArgs& a, int B, float* scratch_v, int* scratch_i, float* mix) {
    hipLaunchKernelGGL(cfg_scan_kernel<true>, dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix);
    FilterArgs f{};
    f.mix = mix; f.V = a.V; f.p = a.p; f.pv = scratch_v; f.pi = scratch_i; f.n_dec = a.n_dec; f.b_off = a.b_off;
    hipLaunchKernelGGL(cfg_select_kernel<false>, dim3(B), dim3(SEL_THREADS), 0, s, f);
    hipLaunchKernelGGL(cfg_pick_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}
// The planned step.  Filtered route: store scan -> planned select -> pick (the mixed rows are in mix afterwards).  Otherwise: [store scan ->] scan -> pick.
void launch_cfg_sample_plan(hipStream_t s, const SampleArgsPlan& a, int B, bool filtered, bool stored, float* scratch_v, int* scratch_i, float* mix) {
    const SampleArgs& base = a;
    if (filtered || stored) hipLaunchKernelGGL((cfg_scan_kernel<true, true>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix);
    if (filtered) {
        FilterArgsPlan f{};
        f.mix = mix; f.V = a.V; f.p = a.p; f.pv = scratch_v; f.pi = scratch_i; f.n_dec = a.n_dec; f.b_off = a.b_off; f.plan = a.plan;
        hipLaunchKernelGGL(cfg_select_kernel<true>, dim3(B), dim3(SEL_THREADS), 0, s, f);
    } else hipLaunchKernelGGL((cfg_scan_kernel<false, true>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, (float*)nullptr);
    hipLaunchKernelGGL(cfg_pick_kernel, dim3(B), dim3(256), 0, s, base, scratch_v, scratch_i);
}
// the arrays a plan left out <- the call's scalars (key: global image index + img_off); one thread per (image, step)
__global__ __launch_bounds__(256) void plan_fill_kernel(SamplePlanDev d, int mask, int B, int T, float cfg_weight, float temperature, int top_k, float top_p,
                                                        int img_off) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (!(mask & 1) && i < (long)B * T) const_cast<float*>(d.w)[i] = cfg_weight;
    if (i < B) {
        if (!(mask & 2)) const_cast<float*>(d.temperature)[i] = temperature;
        if (!(mask & 4)) const_cast<int32_t*>(d.top_k)[i] = top_k;
        if (!(mask & 8)) const_cast<float*>(d.top_p)[i] = top_p;
        if (!(mask & 16)) const_cast<int32_t*>(d.key)[i] = (int32_t)i + img_off;
    }
}
void launch_plan_fill(hipStream_t s, const SamplePlanDev& d, int mask, int B, int T, float cfg_weight, float temperature, int top_k, float top_p, int img_off) {
    const long n = (long)B * T;
    hipLaunchKernelGGL(plan_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, mask, B, T, cfg_weight, temperature, top_k, top_p, img_off);
}
void launch_sample_filter(hipStream_t s, const float* rows, int B, int V, float temperature, int top_k, float top_p, uint8_t* keep) {
    FilterArgs f{};
    f.mix = rows; f.V = V; f.temperature = temperature; f.top_k = top_k; f.top_p = top_p; f.keep = keep;
    hipLaunchKernelGGL(cfg_select_kernel<false>, dim3(B), dim3(SEL_THREADS), 0, s, f);
}

// text token (HF generate): greedy = argmax over vocab; sampled = Gumbel-max over logits / T (== multinomial(softmax(logits / T)));
// finished rows emit eos, unfinished &= (tok != eos).  Two stages like the image sampler: grid (CFG_CHUNKS, B) scans V/CFG_CHUNKS logits with
// 16-byte loads (split-K slabs summed in slab order), one block per row combines the winners (lowest index on ties =
// torch.argmax), does the EOS bookkeeping and gathers the next embedding.  (One block per row over 102 400 logits with
// scalar loads was 160 us per step at 64 rows; this pair is ~10.)
// MODE: TEXT_GREEDY (the argmax, as before), TEXT_SAMPLE (every logit perturbed by gumbel_perturb with p->temperature / seed / row_off: no extra
// pass), TEXT_STORE (filtered sampler: the reduced row, EOS suppression applied, goes to mix [B, V]; the winners are the chunk MAXIMA of the
// unperturbed row, which text_select_kernel reads as the softmax shift).  TAP: also write the row to logits_out [max_new, B, V].
// DFA (pg_generate_text_constrained; rule: kernels.h TextDfaArgs): the block first folds its row's state into one "allowed" bit per token
// class -- 1024 bits = 32 LDS dwords, one per bank, so the lookups of a wave never conflict whatever classes its tokens have (a byte or
// int16 per class spreads 1024 classes over 8-16 dwords per bank) -- and each 16-byte logit load gets one 8-byte load of the four tokens'
// classes issued beside it (token_class: 200 KiB shared by every row, L2 resident).  A disallowed entry becomes -inf where the EOS ban is
// applied, so the tap, the TEXT_STORE row and text_select_kernel carry it without a change.
enum { TEXT_GREEDY = 0, TEXT_SAMPLE = 1, TEXT_STORE = 2 };
// One body, two kernels (text_scan_body.h is included in each): text_scan_kernel is the kernel it was, text_scan_dfa_kernel takes the
// automaton as well.  A shared __device__ function would do, but it changes the unconstrained kernels' register allocation; this way
// their instruction streams are unchanged (compared with llvm-objdump against the build before the DFA parameter existed).
template <int MODE, bool TAP>
__global__ __launch_bounds__(256) void text_scan_kernel(TextArgs a, float* __restrict__ pv, int* __restrict__ pi, float* __restrict__ mix) {
    constexpr bool DFA = MODE < 0;                      // always false; dependent, so `if constexpr (DFA)` discards its branch
    [[maybe_unused]] const TextDfaArgs* d = nullptr;
#include "text_scan_body.h"
}
template <int MODE, bool TAP>
__global__ __launch_bounds__(256) void text_scan_dfa_kernel(TextArgs a, float* __restrict__ pv, int* __restrict__ pi, float* __restrict__ mix, TextDfaArgs dfa) {
    constexpr bool DFA = MODE >= 0;                     // always true
    const TextDfaArgs* d = &dfa;
#include "text_scan_body.h"
}
__global__ __launch_bounds__(256) void text_argmax_kernel(TextArgs a, const float* __restrict__ pv, const int* __restrict__ pi) {
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    if (tid == 0) {
        const int eos = a.p->eos, max_new = a.p->max_new;
        float v = pv[b * CFG_CHUNKS]; int i = pi[b * CFG_CHUNKS];
        for (int k = 1; k < CFG_CHUNKS; ++k) argmax_combine(v, i, pv[b * CFG_CHUNKS + k], pi[b * CFG_CHUNKS + k]);
        if (i == 0x7fffffff) i = 0;                                   // every logit -inf / NaN: index 0 (torch.argmax)
        const int unf = a.unfinished[b];
        const int tok = unf ? i : eos;
        if (step < max_new) a.out[(long)b * max_new + step] = tok;
        const int still = unf && (tok != eos);
        a.unfinished[b] = still;
        if (still) atomicOr(a.any_unfinished + ((step + 1) & 1023), 1);
        s_tok = tok < 0 ? 0 : (tok >= a.V ? a.V - 1 : tok);
    }
    __syncthreads();
    const float* src = a.embed_table + (long)s_tok * a.H;
    float* x0 = a.x + (long)b * a.H;
    for (int i = tid * 4; i < a.H; i += 1024) *(f32x4*)(x0 + i) = *(const f32x4*)(src + i);
}
// The constrained pick: text_argmax_kernel with two differences.  Nothing kept (every allowed logit -inf / NaN) emits eos and finishes the
// row -- token 0 could lie outside the language -- and an unfinished row's state moves along its token (it stays where it is when nothing
// was kept, and for finished rows).  d.tok != null is the operator form: token and next state out, no loop bookkeeping, no embedding.
__global__ __launch_bounds__(256) void text_pick_dfa_kernel(TextArgs a, TextDfaArgs d, const float* __restrict__ pv, const int* __restrict__ pi) {
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    if (tid == 0) {
        const int eos = a.p->eos, max_new = a.p->max_new;
        float v = pv[b * CFG_CHUNKS]; int i = pi[b * CFG_CHUNKS];
        for (int k = 1; k < CFG_CHUNKS; ++k) argmax_combine(v, i, pv[b * CFG_CHUNKS + k], pi[b * CFG_CHUNKS + k]);
        const bool none = i == 0x7fffffff || i < 0 || i >= a.V;
        const int unf = d.tok ? 1 : a.unfinished[b];
        const int tok = (unf && !none) ? i : eos;
        const int st = d.state[b], ncl = d.hdr->n_classes;
        int ns = st;
        if (unf && !none && st >= 0 && st < d.hdr->n_states) {
            const int nx = d.next_state[(long)st * ncl + ((uint16_t)d.token_class[i] & (TEXT_DFA_MAX_CLASSES - 1))];
            if (nx >= 0) ns = nx;
        }
        d.state_out[b] = ns;
        if (d.tok) { d.tok[b] = tok; s_tok = -1; }
        else {
            if (step < max_new) a.out[(long)b * max_new + step] = tok;
            const int still = unf && (tok != eos);
            a.unfinished[b] = still;
            if (still) atomicOr(a.any_unfinished + ((step + 1) & 1023), 1);
            s_tok = tok < 0 ? 0 : (tok >= a.V ? a.V - 1 : tok);
        }
    }
    __syncthreads();
    if (s_tok < 0) return;
    const float* src = a.embed_table + (long)s_tok * a.H;
    float* x0 = a.x + (long)b * a.H;
    for (int i = tid * 4; i < a.H; i += 1024) *(f32x4*)(x0 + i) = *(const f32x4*)(src + i);
}
__global__ void text_dfa_reset_kernel(int32_t* __restrict__ state, const TextDfaHdr* __restrict__ hdr, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) state[b] = hdr->start_state;
}
void launch_text_dfa_reset(hipStream_t s, int32_t* state, const TextDfaHdr* hdr, int B) {
    hipLaunchKernelGGL(text_dfa_reset_kernel, dim3((B + 255) / 256), dim3(256), 0, s, state, hdr, B);
}
__global__ void set_text_op_params_kernel(TextParams* dst, TextParams v, int32_t* step_dst, int step) { *dst = v; *step_dst = step; }
void launch_set_text_op_params(hipStream_t s, TextParams* dst, TextParams v, int32_t* step_dst, int step) {
    hipLaunchKernelGGL(set_text_op_params_kernel, dim3(1), dim3(1), 0, s, dst, v, step_dst, step);
}
template <int MODE>
static void launch_text_scan(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i, float* mix) {
    if (a.logits_out) hipLaunchKernelGGL((text_scan_kernel<MODE, true>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix);
    else hipLaunchKernelGGL((text_scan_kernel<MODE, false>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix);
}
template <int MODE>
static void launch_text_scan_dfa(hipStream_t s, const TextArgs& a, const TextDfaArgs& d, int B, float* scratch_v, int* scratch_i, float* mix) {
    if (a.logits_out) hipLaunchKernelGGL((text_scan_dfa_kernel<MODE, true>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix, d);
    else hipLaunchKernelGGL((text_scan_dfa_kernel<MODE, false>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix, d);
}
void launch_text_argmax(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i) {
    launch_text_scan<TEXT_GREEDY>(s, a, B, scratch_v, scratch_i, nullptr);
    hipLaunchKernelGGL(text_argmax_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}
void launch_text_sample(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i) {
    launch_text_scan<TEXT_SAMPLE>(s, a, B, scratch_v, scratch_i, nullptr);
    hipLaunchKernelGGL(text_argmax_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}

// ------------------------------------------------------------------------------- top-k / top-p text sampler
// The rule of cfg_select_kernel (same keys, same 2^-40 fixed-point masses, same Gumbel noise) for rows that do not fit in LDS
// (vocab 102 400 = 400 KiB): one 1024-thread block per row over the fp32 row in global memory (written by the scan just before: L2 resident).
//   1. m = row maximum (from the scan's chunk maxima, or one pass), the softmax shift.
//   2. one pass: histogram of the 12 leading key bits (sign, exponent, 3 mantissa bits): counts, and exp-masses when top-p acts alone.
//   3. floor bucket = the bucket that holds the k-th largest entry (top_k on: the top-p threshold lies at or above it too), else the
//      bucket that holds the top-p threshold (exact from the bucket masses: no top-k, so Z is the whole row's mass).
//   4. entries at or above the floor are compacted into LDS (<= TSEL_CAND of them: 50 for top_k = 50, ~14 000 for top_p = 0.9 on a
//      Gaussian row) and text_thresholds -- the 8-bit radix walks of cfg_select_kernel -- runs over them.  More candidates than fit
//      (top_p just below 1 on a flat row): the same walks run over the row in global memory instead.  Both give the same thresholds,
//      which depend on the multiset of values only (compaction order does not matter; all mass sums are 64-bit integers).
//   5. one pass: kept = key >= tau; kept mask (operator) and Gumbel-max over the kept set -> slot 0 of the winners text_argmax_kernel combines.
#define TSEL_BITS 12
#define TSEL_BUCKETS (1 << TSEL_BITS)
#define TSEL_CAND 16384
struct TextWalkShm {
    uint32_t hist[256]; unsigned long long mhist[256];
    uint32_t digit, rem; unsigned long long z, above;
};
// f(v, value) over a row with 16-byte loads when the row allows it (V % 4 == 0 and a 16-byte aligned base)
template <class F>
__device__ __forceinline__ void text_row_each(const float* __restrict__ row, int V, int tid, F f) {
    if (((V & 3) | (int)((uintptr_t)row & 15)) == 0) {
        for (int v = tid * 4; v < V; v += SEL_THREADS * 4) {
            const f32x4 c = *(const f32x4*)(row + v);
            f(v, c[0]); f(v + 1, c[1]); f(v + 2, c[2]); f(v + 3, c[3]);
        }
    } else {
        for (int v = tid; v < V; v += SEL_THREADS) f(v, row[v]);
    }
}
struct TextSrcRow {          // the whole row in global memory
    const float* row; int V;
    template <class F> __device__ __forceinline__ void each(int tid, F f) const { text_row_each(row, V, tid, [&](int, float x) { f(x); }); }
};
struct TextSrcLds {          // the compacted candidates
    const float* p; int n;
    template <class F> __device__ __forceinline__ void each(int tid, F f) const { for (int i = tid; i < n; i += SEL_THREADS) f(p[i]); }
};
// tau = max(top-k threshold, top-p threshold) over the entries of src (cfg_select_kernel's walks).  rem_k: rank of the top-k threshold
// (0: top-k off); have_z: Z is z_in (top-k off: the caller knows the row's whole mass), else it is summed over the top-k survivors.
template <class Src>
__device__ __forceinline__ uint32_t text_thresholds(const Src src, TextWalkShm& w, float invT, uint32_t rem_k, float top_p, uint32_t kmx, bool have_z,
                                    unsigned long long z_in) {
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t tk = 0;
    if (rem_k > 0) {
        uint32_t prefix = 0, pmask = 0, rem = rem_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) w.hist[tid] = 0;
            __syncthreads();
            src.each(tid, [&](float x) {
                const uint32_t k = sel_key(x, invT);
                if ((k & pmask) == prefix) atomicAdd(&w.hist[(k >> shift) & 255u], 1u);
            });
            __syncthreads();
            if (tid < 64) {          // lane l holds digits 255-4l .. 252-4l (descending): bucket of the rem-th largest
                uint32_t h[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = w.hist[255 - 4 * lane - j]; sum += h[j]; }
                uint32_t incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                uint32_t before = incl - sum;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (before < rem && before + h[j] >= rem) { w.digit = 255 - 4 * lane - j; w.rem = rem - before; }
                    before += h[j];
                }
            }
            __syncthreads();
            prefix |= w.digit << shift; pmask |= 255u << shift; rem = w.rem;
        }
        tk = prefix;
    }
    uint32_t tp = 0;
    if (top_p < 1.f && kmx > SEL_KEY_NEGINF) {
        const float m = sel_unkey(kmx);
        if (tid == 0) w.z = have_z ? z_in : 0;
        __syncthreads();
        if (!have_z) {
            unsigned long long z = 0;
            src.each(tid, [&](float x) {
                const uint32_t k = sel_key(x, invT);
                if (k >= tk) z += sel_mass(k, m);
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) z += shfl_xor_u64(z, o);
            if (lane == 0) atomicAdd(&w.z, z);
            __syncthreads();
        }
        const double limit = (double)top_p * (double)w.z;
        uint32_t prefix = 0, pmask = 0;
        unsigned long long above = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) { w.hist[tid] = 0; w.mhist[tid] = 0; }
            __syncthreads();
            src.each(tid, [&](float x) {
                const uint32_t k = sel_key(x, invT);
                if (k >= tk && (k & pmask) == prefix) {
                    const uint32_t d = (k >> shift) & 255u;
                    atomicAdd(&w.hist[d], 1u);
                    const unsigned long long q = sel_mass(k, m);
                    if (q) atomicAdd(&w.mhist[d], q);
                }
            });
            __syncthreads();
            if (tid < 64) {          // lowest non-empty bucket whose strictly-larger mass is < limit
                uint32_t c[4]; unsigned long long mm[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = w.hist[255 - 4 * lane - j]; mm[j] = w.mhist[255 - 4 * lane - j]; sum += mm[j]; }
                unsigned long long incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = shfl_up_u64(incl, o); if (lane >= o) incl += t; }
                unsigned long long cum = above + incl - sum;
                int dj = -1; unsigned long long cj = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (c[j] && (double)cum < limit) { dj = 255 - 4 * lane - j; cj = cum; }
                    cum += mm[j];
                }
                const unsigned long long has = __ballot(dj >= 0);
                if (dj >= 0 && lane == 63 - __clzll(has)) { w.digit = (uint32_t)dj; w.above = cj; }
            }
            __syncthreads();
            prefix |= w.digit << shift; pmask |= 255u << shift; above = w.above;
        }
        tp = prefix;
    }
    __syncthreads();
    uint32_t tau = tk > tp ? tk : tp;
    return tau > SEL_KEY_NEGINF + 1 ? tau : SEL_KEY_NEGINF + 1;
}
__global__ __launch_bounds__(SEL_THREADS) void text_select_kernel(TextSelectArgs f) {
    // phase 2-3: cnt[TSEL_BUCKETS] u32 | mass[TSEL_BUCKETS] u64 (48 KiB); phase 4: cand[TSEL_CAND] fp32 (64 KiB)
    __shared__ __attribute__((aligned(16))) unsigned char buf[TSEL_CAND * 4];
    __shared__ TextWalkShm w;
    __shared__ uint32_t s_max, s_floor, s_nc, s_fill;
    __shared__ uint32_t wcnt[SEL_THREADS / 64]; __shared__ unsigned long long wmass[SEL_THREADS / 64];
    __shared__ float wv[SEL_THREADS / 64]; __shared__ int wi[SEL_THREADS / 64];
    uint32_t* cnt = (uint32_t*)buf;
    unsigned long long* mass = (unsigned long long*)(buf + TSEL_BUCKETS * 4);
    float* cand = (float*)buf;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = f.V;
    const float temperature = f.p ? f.p->temperature : f.temperature;
    const int top_k = f.p ? f.p->top_k : f.top_k;
    const float top_p = f.p ? f.p->top_p : f.top_p;
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const float* row = f.rows + (long)b * V;
    // ---- 1. the row maximum
    if (tid == 0) { s_max = 0; s_floor = TSEL_BUCKETS; s_nc = 0; s_fill = 0; }
    __syncthreads();
    if (f.chunk_max) {
        if (tid < CFG_CHUNKS) atomicMax(&s_max, sel_key(f.chunk_max[b * CFG_CHUNKS + tid], invT));
    } else {
        uint32_t kmax = 0;
        text_row_each(row, V, tid, [&](int, float x) { const uint32_t k = sel_key(x, invT); kmax = k > kmax ? k : kmax; });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(kmax, o, 64); kmax = t > kmax ? t : kmax; }
        if (lane == 0) atomicMax(&s_max, kmax);
    }
    __syncthreads();
    const uint32_t kmx = s_max;
    const bool k_on = top_k > 0 && top_k < V;
    const bool p_on = top_p < 1.f && kmx > SEL_KEY_NEGINF;
    uint32_t tau = SEL_KEY_NEGINF + 1;
    if (k_on || p_on) {
        // ---- 2. first-digit histogram
        const bool need_mass = !k_on;
        const float m = sel_unkey(kmx);
        for (int i = tid; i < TSEL_BUCKETS; i += SEL_THREADS) { cnt[i] = 0; mass[i] = 0; }
        __syncthreads();
        text_row_each(row, V, tid, [&](int, float x) {
            const uint32_t k = sel_key(x, invT), d = k >> (32 - TSEL_BITS);
            atomicAdd(&cnt[d], 1u);
            if (need_mass) { const unsigned long long q = sel_mass(k, m); if (q) atomicAdd(&mass[d], q); }
        });
        __syncthreads();
        // ---- 3. the floor bucket: thread t holds buckets top-4t .. top-4t-3 (descending); block-wide exclusive prefix from the top
        constexpr int top = TSEL_BUCKETS - 1;
        uint32_t h[4], hs = 0; unsigned long long mm[4], ms = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { h[j] = cnt[top - 4 * tid - j]; mm[j] = mass[top - 4 * tid - j]; hs += h[j]; ms += mm[j]; }
        uint32_t hin = hs; unsigned long long min_ = ms;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(hin, o, 64); const unsigned long long u = shfl_up_u64(min_, o);
            if (lane >= o) { hin += t; min_ += u; }
        }
        if (lane == 63) { wcnt[wave] = hin; wmass[wave] = min_; }
        __syncthreads();
        uint32_t before = hin - hs; unsigned long long cum = min_ - ms, ztot = 0;
        for (int i = 0; i < SEL_THREADS / 64; ++i) {
            if (i < wave) { before += wcnt[i]; cum += wmass[i]; }
            ztot += wmass[i];
        }
        if (k_on) {
            uint32_t bf = before;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (bf < (uint32_t)top_k && bf + h[j] >= (uint32_t)top_k) { s_floor = top - 4 * tid - j; s_nc = bf + h[j]; }
                bf += h[j];
            }
        } else {
            const double limit = (double)top_p * (double)ztot;
            int dj = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (h[j] && (double)cum < limit) dj = top - 4 * tid - j;
                cum += mm[j];
            }
            if (dj >= 0) atomicMin(&s_floor, (uint32_t)dj);
        }
        __syncthreads();
        const uint32_t floor_d = s_floor;
        if (!k_on) {          // candidates at or above the floor: the inclusive count at that bucket
            uint32_t bf = before;
#pragma unroll
            for (int j = 0; j < 4; ++j) { bf += h[j]; if ((uint32_t)(top - 4 * tid - j) == floor_d) s_nc = bf; }
        }
        __syncthreads();
        const uint32_t nc = s_nc;
        if (nc <= TSEL_CAND) {
            // ---- 4. compact (one LDS atomic per wave and element slot), then the walks over LDS
            text_row_each(row, V, tid, [&](int, float x) {
                const bool in = (sel_key(x, invT) >> (32 - TSEL_BITS)) >= floor_d;
                const unsigned long long bal = __ballot(in);
                if (bal) {
                    uint32_t base = 0;
                    const int leader = __ffsll((long long)bal) - 1;
                    if (lane == leader) base = atomicAdd(&s_fill, (uint32_t)__popcll(bal));
                    base = __shfl(base, leader, 64);
                    if (in) cand[base + __popcll(bal & ((1ull << lane) - 1ull))] = x;
                }
            });
            __syncthreads();
            tau = text_thresholds(TextSrcLds{cand, (int)nc}, w, invT, k_on ? (uint32_t)top_k : 0u, top_p, kmx, !k_on, ztot);
        } else {
            tau = text_thresholds(TextSrcRow{row, V}, w, invT, k_on ? (uint32_t)top_k : 0u, top_p, kmx, false, 0ull);
        }
    }
    // ---- 5. kept mask (operator) / Gumbel-max over the kept set
    const bool draw = f.pv || f.tok;
    float best = -INFINITY; int bi = 0x7fffffff;
    uint64_t seed = 0, stream = 0;
    if (draw) {
        const int step = f.n_dec ? *f.n_dec : f.step;
        seed = f.p ? f.p->seed : f.seed;
        stream = (uint64_t)(b + (f.p ? f.p->row_off : f.row_off)) * 1000003ull + step;
    }
    uint8_t* keep = f.keep ? f.keep + (long)b * V : nullptr;
    text_row_each(row, V, tid, [&](int v, float x) {
        const bool kept = sel_key(x, invT) >= tau;
        if (keep) keep[v] = kept;
        if (draw && kept) {
            const float g = gumbel_perturb(x, invT, seed, stream, v);
            if (g > best) { best = g; bi = v; }
        }
    });
    if (!draw) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        argmax_combine(best, bi, ov, oi);
    }
    if (lane == 0) { wv[wave] = best; wi[wave] = bi; }
    __syncthreads();
    if (tid < CFG_CHUNKS) {
        float v = -INFINITY; int i = 0x7fffffff;
        if (tid == 0) {
            v = wv[0]; i = wi[0];
            for (int k = 1; k < SEL_THREADS / 64; ++k) argmax_combine(v, i, wv[k], wi[k]);
            if (f.tok) f.tok[b] = i == 0x7fffffff ? 0 : i;          // nothing kept (every entry -inf / NaN): token 0
        }
        if (f.pv) { f.pv[b * CFG_CHUNKS + tid] = v; f.pi[b * CFG_CHUNKS + tid] = i; }
    }
}
void launch_text_select(hipStream_t s, const TextSelectArgs& f, int B) {
    hipLaunchKernelGGL(text_select_kernel, dim3(B), dim3(SEL_THREADS), 0, s, f);
}
void launch_text_sample_filtered(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i, float* mix) {
    launch_text_scan<TEXT_STORE>(s, a, B, scratch_v, scratch_i, mix);
    TextSelectArgs f{};
    f.rows = mix; f.V = a.V; f.chunk_max = scratch_v; f.p = a.p; f.n_dec = a.n_dec; f.pv = scratch_v; f.pi = scratch_i;
    launch_text_select(s, f, B);
    hipLaunchKernelGGL(text_argmax_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}
void launch_text_constrained(hipStream_t s, const TextArgs& a, const TextDfaArgs& d, int B, int mode, float* scratch_v, int* scratch_i, float* mix) {
    if (mode == 2) {
        launch_text_scan_dfa<TEXT_STORE>(s, a, d, B, scratch_v, scratch_i, mix);
        TextSelectArgs f{};
        f.rows = mix; f.V = a.V; f.chunk_max = scratch_v; f.p = a.p; f.n_dec = a.n_dec; f.pv = scratch_v; f.pi = scratch_i; f.keep = d.keep;
        launch_text_select(s, f, B);
    } else if (mode == 1) launch_text_scan_dfa<TEXT_SAMPLE>(s, a, d, B, scratch_v, scratch_i, mix);
    else launch_text_scan_dfa<TEXT_GREEDY>(s, a, d, B, scratch_v, scratch_i, mix);
    hipLaunchKernelGGL(text_pick_dfa_kernel, dim3(B), dim3(256), 0, s, a, d, scratch_v, scratch_i);
}

// ------------------------------------------------------------------------------- token log-probabilities
// logprob = x[tok] - logsumexp(x) of one stored row per block (kernels.h LogprobArgs; the definition is in include/plangen_hip.h).
// Two passes over the row, which the scan of this step has just written (L2 resident; 400 KiB at vocab 102 400): the maximum, then
// sum expf(x - max) -- one accurate expf per entry, nothing rescaled.  Eight 16-byte loads in flight per thread as in text_scan_body.h;
// the row may start at any 4-byte boundary and have any length (scalar head and tail around the aligned vectors).  A thread adds at
// most V / 1024 terms in index order, then a butterfly over the wave and a serial sum of the 16 wave sums: a fixed shape, so the
// bits do not depend on how the block was scheduled.  x == max contributes exactly 1 (this is expf(0), and it keeps a row whose
// maximum is +inf meaningful: the mass sits evenly on the +inf entries).
#define LP_THREADS 1024
enum { LP_OP = 0, LP_IMAGE = 1, LP_TEXT = 2, LP_IMAGE_PLAN = 3 };      // LP_IMAGE_PLAN: LP_IMAGE with the image's own temperature (sample plan)
// the argument struct of a form, by specialisation: an expression over the unnamed enum in the kernel's signature would put the enum's
// compiler-made name into the mangled symbol, and the host and device passes number such names differently
template <int FORM> struct LpArgsOf { using type = LogprobArgs; };
template <> struct LpArgsOf<3> { using type = LogprobArgsPlan; };
template <int FORM>
__global__ __launch_bounds__(LP_THREADS) void token_logprob_kernel(typename LpArgsOf<FORM>::type a) {
    __shared__ float red[LP_THREADS / 64];
    __shared__ float s_m;
    const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
    int tok; float temperature; float* dst;
    if (FORM == LP_OP) { tok = a.tok32[b]; temperature = a.temperature; dst = a.out + b; }
    else if (FORM == LP_IMAGE || FORM == LP_IMAGE_PLAN) {
        const int step = *a.n_dec, T = a.sp->T;
        if (step >= T) return;
        const long at = (long)(b + a.b_off) * T + step;
        tok = a.tok32[at]; dst = a.out + at;
        if constexpr (FORM == LP_IMAGE_PLAN) temperature = a.plan_temperature[b + a.b_off]; else temperature = a.sp->temperature;
    } else {
        const int step = *a.n_dec, max_new = a.tp->max_new;
        if (step >= max_new) return;
        const int64_t* o = a.tok64 + (long)b * max_new;
        dst = a.out + (long)b * max_new + step;
        // a finished row emits eos and a row finishes by emitting eos: the row was finished BEFORE this step iff its previous token is eos
        if (step > 0 && o[step - 1] == (int64_t)a.tp->eos) { if (tid == 0) *dst = 0.f; return; }
        tok = (int)o[step]; temperature = a.tp->temperature;
    }
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const float* row = a.rows + (long)b * V;
    auto xval = [&](float y) -> float { const float x = temperature > 0.f ? __fmul_rn(y, invT) : y; return x != x ? -INFINITY : x; };   // the rounded product, never fused into x - m
    int head = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);
    if (head > V) head = V;
    const int nv = (V - head) >> 2, tail0 = head + nv * 4;
    const f32x4* rv = (const f32x4*)(row + head);
    constexpr int IT = 8;
    auto block_reduce = [&](float v, bool is_max) -> float {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const float ov = __shfl_xor(v, o, 64); v = is_max ? fmaxf(v, ov) : v + ov; }
        __syncthreads();                                   // red / s_m of the previous reduction have been read
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) {
            float r = red[0];
            for (int k = 1; k < LP_THREADS / 64; ++k) r = is_max ? fmaxf(r, red[k]) : r + red[k];
            s_m = r;
        }
        __syncthreads();
        return s_m;
    };
    float m = -INFINITY;
    for (int i0 = tid; i0 < nv; i0 += IT * LP_THREADS) {
        f32x4 c[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) { const int i = i0 + it * LP_THREADS; c[it] = rv[i < nv ? i : nv - 1]; }   // clamped: a repeat does not move a maximum
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fmaxf(m, xval(c[it][j]));
    }
    for (int v = tid; v < head; v += LP_THREADS) m = fmaxf(m, xval(row[v]));
    for (int v = tail0 + tid; v < V; v += LP_THREADS) m = fmaxf(m, xval(row[v]));
    m = block_reduce(m, true);
    auto term = [&](float y) -> float { const float x = xval(y); return x == m ? 1.f : expf(x - m); };
    float sum = 0.f;
    for (int i0 = tid; i0 < nv; i0 += IT * LP_THREADS) {
        f32x4 c[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) { const int i = i0 + it * LP_THREADS; c[it] = rv[i < nv ? i : nv - 1]; }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            if (i0 + it * LP_THREADS < nv) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sum += term(c[it][j]);
            }
        }
    }
    for (int v = tid; v < head; v += LP_THREADS) sum += term(row[v]);
    for (int v = tail0 + tid; v < V; v += LP_THREADS) sum += term(row[v]);
    sum = block_reduce(sum, false);
    if (tid == 0) {
        const float xt = (tok >= 0 && tok < V) ? xval(row[tok]) : -INFINITY;
        float lp = -INFINITY;                              // no finite entry, or the token's own entry is -inf
        if (m > -INFINITY && xt > -INFINITY) lp = (xt == m ? 0.f : xt - m) - logf(sum);
        *dst = lp;
    }
}
void launch_token_logprob_op(hipStream_t s, const float* rows, int B, int V, const int32_t* tok, float temperature, float* out) {
    LogprobArgs l{};
    l.rows = rows; l.V = V; l.temperature = temperature; l.tok32 = tok; l.out = out;
    hipLaunchKernelGGL(token_logprob_kernel<LP_OP>, dim3(B), dim3(LP_THREADS), 0, s, l);
}
void launch_cfg_store(hipStream_t s, const SampleArgs& a, int B, float* mix) {
    hipLaunchKernelGGL(cfg_scan_kernel<true>, dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, (float*)nullptr, (int*)nullptr, mix);
}
void launch_token_logprob_image(hipStream_t s, const SampleArgs& a, int B, const float* mix, float* out) {
    LogprobArgs l{};
    l.rows = mix; l.V = a.V; l.sp = a.p; l.tok32 = a.out_tok; l.n_dec = a.n_dec; l.b_off = a.b_off; l.out = out;
    hipLaunchKernelGGL(token_logprob_kernel<LP_IMAGE>, dim3(B), dim3(LP_THREADS), 0, s, l);
}
void launch_token_logprob_image_plan(hipStream_t s, const SampleArgsPlan& a, int B, const float* mix, float* out) {
    LogprobArgsPlan l{};
    l.rows = mix; l.V = a.V; l.sp = a.p; l.tok32 = a.out_tok; l.n_dec = a.n_dec; l.b_off = a.b_off; l.out = out; l.plan_temperature = a.plan.temperature;
    hipLaunchKernelGGL(token_logprob_kernel<LP_IMAGE_PLAN>, dim3(B), dim3(LP_THREADS), 0, s, l);
}
void launch_text_store(hipStream_t s, const TextArgs& a, const TextDfaArgs* d, int B, float* scratch_v, int* scratch_i, float* mix) {
    if (d) {
        TextDfaArgs dd = *d; dd.keep = nullptr;
        launch_text_scan_dfa<TEXT_STORE>(s, a, dd, B, scratch_v, scratch_i, mix);
    } else launch_text_scan<TEXT_STORE>(s, a, B, scratch_v, scratch_i, mix);
}
void launch_token_logprob_text(hipStream_t s, const TextArgs& a, int B, const float* mix, float* out) {
    LogprobArgs l{};
    l.rows = mix; l.V = a.V; l.tp = a.p; l.tok64 = a.out; l.n_dec = a.n_dec; l.out = out;
    hipLaunchKernelGGL(token_logprob_kernel<LP_TEXT>, dim3(B), dim3(LP_THREADS), 0, s, l);
}

// test tap: the sampler's uniform / Gumbel transform of raw 64-bit RNG outputs: out[i] = u, out[n+i] = -log(-log(u))
__global__ void uniform_from_bits_kernel(const uint64_t* __restrict__ z, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float u = uniform_from_bits(z[i]);
    out[i] = u;
    out[n + i] = -__logf(-__logf(u));
}
void launch_uniform_from_bits(hipStream_t s, const uint64_t* z, float* out, int n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(uniform_from_bits_kernel, dim3((n + 255) / 256), dim3(256), 0, s, z, out, n);
}

__global__ void advance_kernel(int32_t* n) { *n += 1; }
void launch_advance(hipStream_t s, int32_t* n_dec) { hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, s, n_dec); }

// ------------------------------------------------------------------------------- weight conversion
template <typename T>
__global__ void convert_kernel(const void* __restrict__ src, int src_bf16, T* __restrict__ dst, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = src_bf16 ? ET<bf16>::ld((const bf16*)src + i) : ((const float*)src)[i];
        ET<T>::st(dst + i, v);
    }
}
// fp32 -> bf16, 8 elements per thread per pass (two 16-byte loads, one 16-byte store); n % 8 == 0, 16-byte aligned pointers
__global__ __launch_bounds__(256) void convert_f32_bf16_vec_kernel(const float* __restrict__ src, bf16* __restrict__ dst, long n8) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const u32x4 a = *(const u32x4*)(src + i * 8), b = *(const u32x4*)(src + i * 8 + 4);
        float f[8];
        ET<float>::unpack(a, f); ET<float>::unpack(b, f + 4);
        *(u32x4*)(dst + i * 8) = ET<bf16>::pack(f);
    }
}
template <typename T>
void launch_convert(hipStream_t s, const void* src, int src_bf16, T* dst, long n) {
    if (n <= 0) return;
    if constexpr (sizeof(T) == 2) {
        if (!src_bf16 && n % 8 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && n >= 65536) {      // the VQ upsample inputs
            const long n8 = n / 8;
            const int vb = (int)((n8 + 255) / 256 < 8192 ? (n8 + 255) / 256 : 8192);
            hipLaunchKernelGGL(convert_f32_bf16_vec_kernel, dim3(vb), dim3(256), 0, s, (const float*)src, (bf16*)dst, n8);
            return;
        }
    }
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(convert_kernel<T>, dim3(blocks), dim3(256), 0, s, src, src_bf16, dst, n);
}
template void launch_convert<float>(hipStream_t, const void*, int, float*, long);
template void launch_convert<bf16>(hipStream_t, const void*, int, bf16*, long);
void launch_to_f32(hipStream_t s, const void* src, int src_bf16, float* dst, long n) { launch_convert<float>(s, src, src_bf16, dst, n); }

template <typename T>
__global__ void convert_conv_kernel(const void* __restrict__ src, int src_bf16, T* __restrict__ dst, int Cout, int Cin, int kk) {
    const long n = (long)Cout * Cin * kk;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        // dst index i = (co*kk + tap)*Cin + ci ; src index = (co*Cin + ci)*kk + tap
        const int ci = (int)(i % Cin); const long t = i / Cin; const int tap = (int)(t % kk); const long co = t / kk;
        const long si = (co * Cin + ci) * kk + tap;
        const float v = src_bf16 ? ET<bf16>::ld((const bf16*)src + si) : ((const float*)src)[si];
        ET<T>::st(dst + i, v);
    }
}
template <typename T>
void launch_convert_conv(hipStream_t s, const void* src, int src_bf16, T* dst, int Cout, int Cin, int kk) {
    const long n = (long)Cout * Cin * kk;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(convert_conv_kernel<T>, dim3(blocks), dim3(256), 0, s, src, src_bf16, dst, Cout, Cin, kk);
}
template void launch_convert_conv<float>(hipStream_t, const void*, int, float*, int, int, int);
template void launch_convert_conv<bf16>(hipStream_t, const void*, int, bf16*, int, int, int);

template <typename T>
__global__ void convert_il16_kernel(const void* __restrict__ src, int src_bf16, T* __restrict__ dst, int I, int H, int which) {
    const long n = (long)I * H;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / H; const int c = (int)(i % H);
        const long dr = (r >> 3) * 16 + which * 8 + (r & 7);
        const float v = src_bf16 ? ET<bf16>::ld((const bf16*)src + i) : ((const float*)src)[i];
        ET<T>::st(dst + dr * H + c, v);
    }
}
template <typename T>
void launch_convert_interleave16(hipStream_t s, const void* src, int src_bf16, T* dst, int I, int H, int which) {
    const long n = (long)I * H;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(convert_il16_kernel<T>, dim3(blocks), dim3(256), 0, s, src, src_bf16, dst, I, H, which);
}
template void launch_convert_interleave16<float>(hipStream_t, const void*, int, float*, int, int, int);
template void launch_convert_interleave16<bf16>(hipStream_t, const void*, int, bf16*, int, int, int);

__global__ void l2norm_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int D) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    float ss = 0.f;
    for (int d = 0; d < D; ++d) ss += src[(long)r * D + d] * src[(long)r * D + d];
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);                   // F.normalize eps
    for (int d = 0; d < D; ++d) dst[(long)r * D + d] = src[(long)r * D + d] / nrm;
}
void launch_l2norm_rows(hipStream_t s, const float* src, float* dst, int n, int D) {
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n, D);
}
void launch_fill_zero(hipStream_t s, void* p, long bytes) { (void)hipMemsetAsync(p, 0, bytes, s); }
