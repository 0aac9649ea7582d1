// Attention mass of chosen query columns on prompt spans (pg_request_attn_spans / pg_op_attn_span_mass; definition: include/plangen_hip.h,
// DESIGN 4.13):   A[r, i, s] = 1 / nh * sum_h sum_{k in span(r, s), k <= q_i, k real} softmax_k(scale * Q[r, h, q_i] . K[r, h, k]).
//
// The swapped-QK^T flash tile of attn_prefill_flash_kernel with V replaced by a span indicator.  One 256-thread block = 64 consecutive query
// SLOTS of one row (wave w owns 16 of them) and walks ALL heads in ascending order, so the head mean is one fixed-order fp32 sum inside one
// block: no atomics, no partials, two launches give the same bits.  Per head and 64-key tile: K [64][128] is staged in LDS, S^T = K . Q^T by
// v_mfma_f32_16x16x32_bf16 (C layout: lane (lr, g) holds the scores of QUERY lr for keys 16 kt + 4 g + r), scale applied to the fp32 scores,
// running max / sum per query in fp32 as in the attention kernel.  The [key][16 spans] 0/1 matrix E is never stored: lane (lr, g) of the
// P.E MFMA's B operand is SPAN lr for the same 8 keys the lane's P fragment covers, built from the span's bounds by comparisons.  P enters
// that MFMA as hi + lo (two bf16 each, two MFMAs per k-step): E is exact in bf16, so the only rounding of the span sum is the 2^-17 relative
// residue of the split and the fp32 accumulation.  The span accumulator [16 queries][16 spans] is rescaled like the O accumulator when the
// running maximum rises.  Slots and columns: slot = column - pad_len[row]; keys are slots 0 .. len[row) of the row's K.
#include "kernels.h"
#include "gemm_common.h"

#define AS_KROW 272          // bytes per K row in LDS (256 + 16 pad), as the flash kernel's

__global__ __launch_bounds__(256) void attn_span_mass_kernel(const bf16* __restrict__ qbuf, const bf16* __restrict__ kc,
                                                            const int32_t* __restrict__ row_off, const int32_t* __restrict__ len,
                                                            const int32_t* __restrict__ pad_len, const int32_t* __restrict__ span_lo,
                                                            const int32_t* __restrict__ span_hi, int n_spans, int q_col0, int n_q, int nh,
                                                            int slots, float scale, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char sK[64 * AS_KROW];
    const int row = blockIdx.y;
    const int off = row_off[row];
    const int L = len[row];
    const int pad = pad_len[row];
    // requested query slots of this row: columns [q_col0, q_col0 + n_q) that are real tokens
    const int s_lo = max(q_col0 - pad, 0), s_hi = min(q_col0 + n_q - pad, L);
    if (off < 0 || L <= 0 || s_lo >= s_hi) return;             // nothing real requested in this row: the launcher's zeros stay
    const int qt = s_lo / 64 + (int)blockIdx.x;                // only the query tiles that hold a requested slot
    if (qt * 64 >= s_hi) return;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, g = l >> 4, lr = l & 15;
    const int HD = nh * 128;
    const int q0 = qt * 64 + w * 16;                            // first query slot of this wave
    const int myq = q0 + lr;                                    // the query whose softmax state this lane carries
    // this lane's span (B-operand column lr of the P.E MFMA), in slots; lanes past n_spans carry an empty one
    int sp_lo = 0, sp_hi = 0;
    if (lr < n_spans) { sp_lo = span_lo[row * n_spans + lr] - pad; sp_hi = span_hi[row * n_spans + lr] - pad; }
    const int qmax = min(qt * 64 + 63, s_hi - 1);               // last requested query of the block
    const int ntiles = qmax / 64 + 1;                           // causal: keys 0 .. qmax  (qmax < L <= slots)
    float hsum[4] = {0.f, 0.f, 0.f, 0.f};                       // sum over heads of A for (query g*4+r, span lr)
    for (int head = 0; head < nh; ++head) {
        bf16x8 qf[4];                                           // Q fragments (B operand): lane (q = lr, g) holds Q[q][ds*32 + g*8 .. +8], unscaled
        {
            const int qq = myq < L ? myq : L - 1;
            const bf16* qp = qbuf + (long)(off + qq) * HD + head * 128 + g * 8;
#pragma unroll
            for (int ds = 0; ds < 4; ++ds) qf[ds] = *(const bf16x8*)(qp + ds * 32);
        }
        const bf16* kbase = kc + ((long)row * nh + head) * slots * 128;
        f32x4 eacc = (f32x4){0.f, 0.f, 0.f, 0.f};
        float m_run = -INFINITY, l_run = 0.f;
        for (int kt0 = 0; kt0 < ntiles; ++kt0) {
            const int kb = kt0 * 64;
            __syncthreads();                                    // previous tile (or head) fully consumed
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = tid + j * 256, key = v >> 4, cv = v & 15;
                const int ks = (kb + key < L) ? kb + key : L - 1;
                *(u32x4*)(sK + key * AS_KROW + cv * 16) = *(const u32x4*)(kbase + (long)ks * 128 + cv * 8);
            }
            __syncthreads();
            f32x4 sacc[4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                sacc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ds = 0; ds < 4; ++ds) {
                    const bf16x8 ka = *(const bf16x8*)(sK + (kt * 16 + lr) * AS_KROW + (ds * 32 + g * 8) * 2);
                    sacc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[ds], sacc[kt], 0, 0, 0);
                }
            }
            // lane (lr, g): query myq, keys kb + kt*16 + g*4 + r; the scale multiplies the fp32 score
            float mx = m_run;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kb + kt * 16 + g * 4 + r;
                    sacc[kt][r] = (key > myq || key >= L) ? -INFINITY : sacc[kt][r] * scale;      // causal + length mask
                    mx = fmaxf(mx, sacc[kt][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            // key 0 <= every query, so mx is finite from the first tile on
            const float alpha = __expf(m_run - mx);
            float psum = 0.f;
            bf16x8 ph[2], pl[2], ef[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float p[8], ph_f[8], pl_f[8], e[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = __expf(sacc[2 * s][r] - mx);
                    p[4 + r] = __expf(sacc[2 * s + 1][r] - mx);
                    const int k0 = kb + (2 * s) * 16 + g * 4 + r, k1 = k0 + 16;
                    e[r] = (k0 >= sp_lo && k0 < sp_hi) ? 1.f : 0.f;
                    e[4 + r] = (k1 >= sp_lo && k1 < sp_hi) ? 1.f : 0.f;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    psum += p[i];
                    ph_f[i] = bf16_bits_to_f32(f32_to_bf16_bits(p[i]));      // hi = bf16(p), lo = bf16(p - hi): p - hi is exact in fp32
                    pl_f[i] = p[i] - ph_f[i];
                }
                const u32x4 hv = ET<bf16>::pack(ph_f), lv = ET<bf16>::pack(pl_f), ev = ET<bf16>::pack(e);
                ph[s] = *(const bf16x8*)&hv; pl[s] = *(const bf16x8*)&lv; ef[s] = *(const bf16x8*)&ev;
            }
            psum += __shfl_xor(psum, 16, 64);
            psum += __shfl_xor(psum, 32, 64);
            l_run = l_run * alpha + psum;
            m_run = mx;
            // rescale the span sums (row = query g*4+r of this wave) by that query's alpha, then add this tile's P . E
#pragma unroll
            for (int r = 0; r < 4; ++r) eacc[r] *= __shfl(alpha, g * 4 + r, 64);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                eacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph[s], ef[s], eacc, 0, 0, 0);
                eacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl[s], ef[s], eacc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) hsum[r] += eacc[r] / __shfl(l_run, g * 4 + r, 64);
    }
    // ---- head mean and store: query slot q0 + g*4 + r, span lr
    const float inv_nh = 1.f / (float)nh;
    if (lr < n_spans) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + g * 4 + r;
            if (q >= s_lo && q < s_hi) out[((long)row * n_q + (q + pad - q_col0)) * n_spans + lr] = hsum[r] * inv_nh;
        }
    }
}

// out fp32 [R][n_q][n_spans]: zeroed here (pad queries, rows without packed tokens), then every real requested query is written by exactly
// one block.  The caller guarantees len[r] <= slots, n_spans in 1..16 and that q / K hold what row_off / len name.
void launch_attn_span_mass(hipStream_t s, const bf16* qbuf, const bf16* kc, const int32_t* row_off, const int32_t* len, const int32_t* pad_len,
                           const int32_t* span_lo, const int32_t* span_hi, int n_spans, int q_col0, int n_q, int R, int nh, int slots,
                           float scale, float* out) {
    if (R <= 0 || n_q <= 0 || n_spans <= 0) return;
    (void)hipMemsetAsync(out, 0, (size_t)R * n_q * n_spans * 4, s);
    // a row's requested slots are n_q consecutive ones starting anywhere in a 64-slot tile: at most (n_q + 62) / 64 + 1 tiles
    hipLaunchKernelGGL(attn_span_mass_kernel, dim3((n_q + 62) / 64 + 1, R), dim3(256), 0, s, qbuf, kc, row_off, len, pad_len, span_lo, span_hi,
                       n_spans, q_col0, n_q, nh, slots, scale, out);
}
