// Query-offset form of the 128-query flash prefill kernel (attn_prefill.hip: attn_prefill_flash2_kernel) for pg_prefill_extend: the packed
// queries of row r are its n_new[r] NEW tokens, which sit in slots q0 .. q0 + n_new - 1 of a cache that already holds slots 0 .. q0 - 1
// (q0 = len[r] - n_new[r]; len is the row's length AFTER the extension).  New token i sees keys 0 .. q0 + i.
//
// Everything about a key tile is flash2's: 64-key K / V tiles by LDS-DMA straight from the cache [row][head][slot][128], double-buffered per
// operand, each tile retired one barrier before the phase that reads it (two raw s_barrier per tile, counted vmcnt(4)); the same chunk
// swizzles; V through ds_read_b64_tr_b16; swapped QK^T so P stays in registers; tiles walked 0 .. ntiles - 1 with the same online-softmax
// updates.  What differs is where a query sits: query tile qt of a row covers LOCAL queries 128 qt .. 128 qt + 127 (packed rows
// row_off + local), whose slots are q0 + local.  q0 is arbitrary (not a multiple of 64), so
//   * the block walks (q0 + last local query) / 64 + 1 key tiles;
//   * a wave skips tiles that start past its last query's slot, and masks (per element: key > slot of the query, key >= len) only tiles
//     that reach past its FIRST query's slot or past len -- tiles wholly in the past need no mask;
// With q0 = 0 every index above is flash2's, so the two kernels give the same bits on the same inputs (tests/test_gpu_extend_ops.py).
#include "kernels.h"
#include "gemm_common.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
#define FX_TILE 16384
__device__ __forceinline__ u32x2 lds_tr16x(const char* p) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
    return __builtin_bit_cast(u32x2, v);
}
__global__ __launch_bounds__(256, 2) void attn_extend_flash_kernel(const bf16* __restrict__ qbuf, bf16* __restrict__ obuf,
                                                                  const bf16* __restrict__ kc, const bf16* __restrict__ vc,
                                                                  const int32_t* __restrict__ row_off, const int32_t* __restrict__ len,
                                                                  const int32_t* __restrict__ n_new, int nh, int slots, float scale, int nqt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];                    // K[2][16 KiB] | V[2][16 KiB]
    const int qt = nqt - 1 - (int)blockIdx.x, head = blockIdx.y, row = blockIdx.z;
    const int off = row_off[row];
    const int L = len[row];                                                         // keys of the row, the new tokens included
    const int n = n_new[row];
    if (off < 0 || n < 1 || n > L || qt * 128 >= n) return;
    const int q0 = L - n;                                                           // slot of the row's first new token
    const int tid = threadIdx.x, l = tid & 63, g = l >> 4, lr = l & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HD = nh * 128;
    const int i0w = qt * 128 + w * 32;                                              // first LOCAL query of this wave
    const int q0w = q0 + i0w;                                                       // ... and its slot
    bf16x8 qf[2][4];
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
        const int myi = i0w + qg * 16 + lr;
        const int qq = myi < n ? myi : n - 1;
        const bf16* qp = qbuf + (long)(off + qq) * HD + head * 128 + g * 8;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
            const u32x4 v = *(const u32x4*)(qp + ds * 32);
            float f[8]; ET<bf16>::unpack(v, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] *= scale;
            const u32x4 pv = ET<bf16>::pack(f);
            qf[qg][ds] = *(const bf16x8*)&pv;
        }
    }
    const bf16* kbase = kc + ((long)row * nh + head) * slots * 128;
    const bf16* vbase = vc + ((long)row * nh + head) * slots * 128;
    // DMA: wave w, instruction i covers tile rows (w*4 + i)*4 .. +3 (lane: row l >> 4, slot l & 15)
    int rr[4], ksw[4], vsw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (w * 4 + i) * 4 + (l >> 4);
        rr[i] = r; ksw[i] = ((l & 15) ^ (r & 15)) * 8; vsw[i] = ((l & 15) ^ ((r & 3) << 1)) * 8;
    }
    auto issueK = [&](int t) __attribute__((always_inline)) {
        const int kb = t * 64;
        char* kd = smem + (t & 1) * FX_TILE + w * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int key = kb + rr[i];
            key = key < L ? key : L - 1;                                            // clamp: the load stays inside the row's written slots
            glds16(kbase + (long)key * 128 + ksw[i], kd + i * 1024);
        }
    };
    auto issueV = [&](int t) __attribute__((always_inline)) {
        const int kb = t * 64;
        char* vd = smem + 2 * FX_TILE + (t & 1) * FX_TILE + w * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int key = kb + rr[i];
            key = key < L ? key : L - 1;
            glds16(vbase + (long)key * 128 + vsw[i], vd + i * 1024);
        }
    };
    f32x4 oacc[2][8];
#pragma unroll
    for (int qg = 0; qg < 2; ++qg)
#pragma unroll
        for (int i = 0; i < 8; ++i) oacc[qg][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
    const int qlast = q0 + min(qt * 128 + 127, n - 1);                              // slot of the block's last query
    const int ntiles = qlast / 64 + 1;                                             // causal: keys 0 .. qlast
    const int vlane = (4 * g + (lr >> 2)) * 256 + (lr & 1) * 8;
    const int vcb = (lr & 3) >> 1, vsz = (lr >> 2) << 1;
    // Staging protocol of attn_prefill_flash2_kernel, unchanged: a tile is RETIRED (its issuing waves' vmcnt wait + a block barrier) one
    // barrier BEFORE the phase that first reads it.
    //   A(t): retires V(t)   [issued after A(t-1)];  everyone is past PV(t-1)  -> V(t+1) is issued into the slot of V(t-1)
    //   B(t): retires K(t+1) [issued after PV(t-1)]; everyone is past QK^T(t)  -> after PV(t), K(t+2) is issued into the slot of K(t)
    // In flight behind each wait is exactly one younger tile (4 DMA instructions per wave): counted vmcnt(4), vmcnt(0) at the tail.
    issueK(0); issueV(0);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                                // K(0) landed (V(0) may still be in flight)
    __builtin_amdgcn_s_barrier();                                                   // B(-1): retires K(0)
    if (1 < ntiles) issueK(1);
    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");        // V(t) landed; K(t+1) behind it
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                               // A(t)
        if (t + 1 < ntiles) issueV(t + 1);
        const int kb = t * 64;
        const bool skip = kb > q0w + 31;                                            // the whole tile is in the future of this wave's queries
        const char* sK = smem + (t & 1) * FX_TILE;
        const char* sV = sK + 2 * FX_TILE;
        bf16x8 pf[2][2];
        if (!skip) {
        f32x4 sacc[2][4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            sacc[0][kt] = (f32x4){0.f, 0.f, 0.f, 0.f}; sacc[1][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ds = 0; ds < 4; ++ds) {
                const bf16x8 ka = *(const bf16x8*)(sK + (kt * 16 + lr) * 256 + (((ds * 4 + g) ^ lr) << 4));
                sacc[0][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[0][ds], sacc[0][kt], 0, 0, 0);
                sacc[1][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[1][ds], sacc[1][kt], 0, 0, 0);
            }
        }
        const bool need_mask = (kb + 63 > q0w) || (kb + 64 > L);                    // tiles wholly in the wave's past stay unmasked
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {
            const int myq = q0w + qg * 16 + lr;                                     // slot of the query whose softmax state this lane carries
            float mx = m_run[qg];
            if (need_mask) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = kb + kt * 16 + g * 4 + r;
                        if (key > myq || key >= L) sacc[qg][kt][r] = -INFINITY;
                    }
            }
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sacc[qg][kt][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float alpha = __expf(m_run[qg] - mx);                              // key 0 is visible to every query: mx finite from tile 0
            float psum = 0.f;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                float p[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = __expf(sacc[qg][2 * s2][r] - mx);
                    p[4 + r] = __expf(sacc[qg][2 * s2 + 1][r] - mx);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) psum += p[e];
                const u32x4 pv = ET<bf16>::pack(p);
                pf[qg][s2] = *(const bf16x8*)&pv;
            }
            psum += __shfl_xor(psum, 16, 64);
            psum += __shfl_xor(psum, 32, 64);
            l_run[qg] = l_run[qg] * alpha + psum;
            m_run[qg] = mx;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = __shfl(alpha, g * 4 + r, 64);
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) oacc[qg][dt][r] *= a;
            }
        }
        }
        if (t + 1 < ntiles) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");        // K(t+1) landed; V(t+1) behind it
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                               // B(t)
        if (!skip) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            const int co = ((2 * dt + vcb) ^ vsz) << 4;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const char* va = sV + (32 * s2) * 256 + vlane + co;
                const u32x2 lo = lds_tr16x(va), hi = lds_tr16x(va + 16 * 256);
                u32x4 vb; vb.x = lo.x; vb.y = lo.y; vb.z = hi.x; vb.w = hi.y;
                const bf16x8 vf = *(const bf16x8*)&vb;
                oacc[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[0][s2], vf, oacc[0][dt], 0, 0, 0);
                oacc[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[1][s2], vf, oacc[1][dt], 0, 0, 0);
            }
        }
        }
        // issued AFTER PV(t), as in flash2: hipcc drains vmcnt in front of the transpose reads
        if (t + 2 < ntiles) issueK(t + 2);
    }
#pragma unroll
    for (int qg = 0; qg < 2; ++qg)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float lq = __shfl(l_run[qg], g * 4 + r, 64);
            const int i = i0w + qg * 16 + g * 4 + r;                                // local query of accumulator row r
            if (i < n) {
                const float inv = 1.f / lq;
                bf16* op = obuf + (long)(off + i) * HD + head * 128 + lr;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) ET<bf16>::st(op + dt * 16, oacc[qg][dt][r] * inv);
            }
        }
}

// len [R]: the rows' lengths after the extension (<= slots); n_new [R]: new tokens of the row (1 .. len); row_off [R]: first packed token of
// the row, -1 = none; max_new = max n_new over the rows.
void launch_attn_extend_flash(hipStream_t s, const bf16* qbuf, bf16* obuf, const bf16* kc, const bf16* vc, const int32_t* row_off,
                              const int32_t* len, const int32_t* n_new, int R, int max_new, int nh, int slots, float scale) {
    if (R <= 0 || max_new <= 0) return;
    (void)PG_DYN_LDS(attn_extend_flash_kernel, 4 * FX_TILE);
    const int nqt = (max_new + 127) / 128;
    hipLaunchKernelGGL(attn_extend_flash_kernel, dim3(nqt, nh, R), dim3(256), 4 * FX_TILE, s, qbuf, obuf, kc, vc, row_off, len, n_new, nh, slots, scale, nqt);
}
