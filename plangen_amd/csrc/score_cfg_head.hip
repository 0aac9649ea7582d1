// Fused CFG-mixed gen_head layer 2 + log-softmax at a target (pg_score_image_tokens / pg_op_cfg_head_logprob): score_head.hip's kernel with
// a classifier-free-guidance mix between the accumulators and the fold.  Per scored position i (c = cond_idx[i], u = uncond_idx[i], t = target[i]):
//
//   yc_v = sum_k X[c][k] * W[v][k] + bias[v],   yu_v likewise with X[u]     (bf16 operands, fp32 accumulation on the MFMA units; bias fp32 or absent)
//   y_v  = yu_v + cfg_weight * (yc_v - yu_v)                                (fp32, the expression of cfg_scan_kernel in llm_kernels.hip)
//   x_v  = y_v * (1 / temperature)  when temperature > 0, else y_v          (the rounded fp32 product)
//   out[i] = (x_t - m) - logf(sum_v expf(x_v - m)),  m = max_v x_v;   t outside [0, V) gives -inf
//
// Neither the two [n, V] logit tensors nor the mixed one leave registers.  NaN / inf operands are NOT covered, as in score_head.hip.
//
// Everything but the fold is head_logprob_kernel's (tiles of 256 rows x 256 columns, K step 64, the glds16 staging stream, the swizzle, the
// two-phase schedule and its counted waits, column-tile groups, the XCD remap, [G][n][2] partials merged by head_combine_kernel); the
// geometry is head_logprob_geom(2 n, V, K): a row tile holds CH_PAIRS = 128 pairs.  What differs:
// * Pair placement.  The A tile is gathered through BOTH index lists so that pair p of a tile (p = wave row * 64 + q * 16 + lane row) has
//   its cond row at accumulator row mt = 2q and its uncond row at mt = 2q + 1 of the lane that holds it: tile rows wr*128 + mt*16 + lr.  A
//   pair never straddles a tile or a lane.  Pairs >= n of the last row tile re-read pair n - 1 (results dropped).
// * Fold.  A lane loads its 16 bias values of the column tile, adds them to both rows, mixes in registers and runs the online (m, s) update
//   on 4 mixed rows instead of 8 raw ones: no shuffle and no LDS for the mix.
// * Merge: 4 lanes of a pair (shuffles, fixed order), the 4 column waves (LDS, ascending), the G groups (combine kernel, ascending): every
//   reduction has a fixed shape, so a position's bits are a function of its two X rows, W, bias, its target, cfg_weight, the temperature
//   and (n, V, K) -- not of its slot nor of the other positions.
#include "score_head.h"

#define CH_PAIRS (SH_BM / 2)

size_t cfg_head_logprob_ws_bytes(long n, int V, int K) {
    const HeadGeom g = head_logprob_geom(2 * n, V, K);
    return (((size_t)2 * 4 * g.G * (size_t)n) + 255) & ~(size_t)255;
}

__global__ __launch_bounds__(512) void cfg_head_logprob_kernel(const bf16* __restrict__ X, const bf16* __restrict__ W, const float* __restrict__ bias,
                                                               const int32_t* __restrict__ cond_idx, const int32_t* __restrict__ uncond_idx,
                                                               const int32_t* __restrict__ target, int n, int V, int K, int ntm, int ntn, int cpt, int G,
                                                               float cfg_weight, float temperature, float* __restrict__ part, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = K / SH_BK;

    // block -> (row tile, group): an XCD's share of the grid is 4 row tiles x all groups, so its L2 holds 4 A panels while the W tiles stream
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int per = 4 * G, mg = t / per, rem = t - mg * per, gm = min(4, ntm - mg * 4);
    const int p0 = (mg * 4 + rem % gm) * CH_PAIRS, grp = rem / gm;      // first pair of the row tile
    const int c0 = grp * cpt, c1 = min(ntn, c0 + cpt);

    const int srow = w * 8 + (l >> 3);                           // + i*64
    const int sc = ((l & 7) ^ (((w & 1) << 2) + (l >> 4))) * 8;  // swizzled SOURCE chunk (elements)
    char* const swave = smem + w * 1024;
    const int wr = w >> 2, wc = w & 3, g = l >> 4, lr = l & 15;
    const int swz = (lr >> 1) & 7;
    const int aoff0 = (wr * 64 + lr) * 128 + ((g ^ swz) << 4), aoff1 = aoff0 ^ 64;
    const int boff0 = 2 * SH_AH + (wc * 32 + lr) * 128 + ((g ^ swz) << 4), boff1 = boff0 ^ 64;

    const bf16* arow[4];
    const bf16* wrow[4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = i * 64 + srow;                         // LDS row of the half-tile -> (wave row r>>6, row r&63)
            // wave row r>>6, accumulator row mt = h*4 + ((r&63)>>4), lane row r&15: pair (wave row)*64 + (mt>>1)*16 + (r&15), cond when mt is even
            const int mt = h * 4 + ((r & 63) >> 4);
            const int p = p0 + (r >> 6) * 64 + (mt >> 1) * 16 + (r & 15), pc = p < n ? p : n - 1;
            arow[h * 2 + i] = X + (long)((mt & 1) ? uncond_idx[pc] : cond_idx[pc]) * K;
        }
    int n0 = 0;
    auto setup = [&](int ct) __attribute__((always_inline)) {
        n0 = ct * SH_BN;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = i * 64 + srow;
                const int v = n0 + (r >> 5) * 64 + h * 32 + (r & 31);
                wrow[h * 2 + i] = W + (long)(v < V ? v : V - 1) * K;
            }
    };
    auto stage_A = [&](int h, int T) __attribute__((always_inline)) {
        const int k0 = (T < nk ? T : nk - 1) * SH_BK;
        char* d = swave + (T & 1) * SH_BUF + h * SH_AH;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(arow[h * 2 + i] + k0 + sc, d + i * 8192);
    };
    auto stage_B = [&](int h, int T) __attribute__((always_inline)) {
        const int k0 = (T < nk ? T : nk - 1) * SH_BK;
        char* d = swave + (T & 1) * SH_BUF + 2 * SH_AH + h * SH_BH;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(wrow[h * 2 + i] + k0 + sc, d + i * 8192);
    };
    auto prologue = [&]() __attribute__((always_inline)) { stage_A(0, 0); stage_B(0, 0); stage_B(1, 0); stage_A(1, 0); stage_A(0, 1); stage_B(0, 1); };

    f32x4 acc[8][4];
    bf16x8 a[4][2], b0[2][2], b1[2][2];
    float mrun[4], srun[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { mrun[i] = -INFINITY; srun[i] = 0.f; }
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const bool scaled = temperature > 0.f;

#define SH_MFMA_SECTION(MH, BFA, NHA, BFB, NHB)                                                            \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      /* WAR: fragments in registers BEFORE the barrier (gemm256.hip) */ \
    sh_barrier();                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    __builtin_amdgcn_s_setprio(1);                                                                          \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                        \
        _Pragma("unroll") for (int mt = 0; mt < 4; ++mt)                                                    \
            _Pragma("unroll") for (int nt = 0; nt < 2; ++nt) {                                              \
                acc[MH * 4 + mt][NHA * 2 + nt] =                                                            \
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(BFA[nt][ks], a[mt][ks], acc[MH * 4 + mt][NHA * 2 + nt], 0, 0, 0); \
                acc[MH * 4 + mt][NHB * 2 + nt] =                                                            \
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(BFB[nt][ks], a[mt][ks], acc[MH * 4 + mt][NHB * 2 + nt], 0, 0, 0); \
            }                                                                                               \
    __builtin_amdgcn_s_setprio(0);                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    sh_barrier();

    setup(c0);
    prologue();
    for (int ct = c0; ct < c1; ++ct) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // HB1(0) landed (younger: HA1(0) HA0(1) HB0(1))
        sh_barrier();
        if (wr >= 1) sh_barrier();                            // second wave group runs one barrier behind

        for (int kt = 0; kt < nk; ++kt) {
            const char* buf = smem + (kt & 1) * SH_BUF;
            // ---- phase A: quadrants (0,0) (0,1): fragments of HB0, HA0, HB1; stage HB1(kt+1), HA1(kt+1)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                b0[nt][0] = *(const bf16x8*)(buf + boff0 + nt * 2048);
                b0[nt][1] = *(const bf16x8*)(buf + boff1 + nt * 2048);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                a[mt][0] = *(const bf16x8*)(buf + aoff0 + mt * 2048);
                a[mt][1] = *(const bf16x8*)(buf + aoff1 + mt * 2048);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                b1[nt][0] = *(const bf16x8*)(buf + SH_BH + boff0 + nt * 2048);
                b1[nt][1] = *(const bf16x8*)(buf + SH_BH + boff1 + nt * 2048);
            }
            stage_B(1, kt + 1);
            stage_A(1, kt + 1);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");      // HA1(kt) landed (younger: HA0 HB0 HB1 HA1 of kt+1)
            __builtin_amdgcn_sched_barrier(0);
            SH_MFMA_SECTION(0, b0, 0, b1, 1)
            // ---- phase B: quadrants (1,1) (1,0): fragments of HA1; stage HA0(kt+2), HB0(kt+2)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                a[mt][0] = *(const bf16x8*)(buf + SH_AH + aoff0 + mt * 2048);
                a[mt][1] = *(const bf16x8*)(buf + SH_AH + aoff1 + mt * 2048);
            }
            stage_A(0, kt + 2);
            stage_B(0, kt + 2);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // HB1(kt+1) (and the older HA0 / HB0(kt+1)) landed
            __builtin_amdgcn_sched_barrier(0);
            SH_MFMA_SECTION(1, b1, 1, b0, 0)
        }
        if (wr < 1) sh_barrier();
        // every wave is past its last ds_read: the next column tile's first loads go out before this tile's fold
        const int ecol = n0 + wc * 64 + g * 4;                // the lane's first column; n-tile nt, element j -> ecol + nt*16 + j
        if (ct + 1 < c1) { setup(ct + 1); prologue(); }
        const int lim = V - ecol;                             // columns nt*16 + j >= lim are past the vocabulary
        float bv[16];                                         // the lane's 16 bias values of this column tile (columns past V: clamped, folded as -inf)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = ecol + nt * 16 + j;
                bv[nt * 4 + j] = bias ? bias[v < V ? v : V - 1] : 0.f;
            }
        int tcol[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = p0 + wr * 64 + q * 16 + lr;
            const int tg = target[p < n ? p : n - 1];
            tcol[q] = (p < n && tg >= 0 && tg < V) ? tg - ecol : -1;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {                         // pair q: cond in accumulator row 2q, uncond in 2q + 1 -- the mix never leaves the lane
            float xs[16];
            float mx = -INFINITY, xt = 0.f;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float c = acc[2 * q][nt][j] + bv[nt * 4 + j], u = acc[2 * q + 1][nt][j] + bv[nt * 4 + j];
                    const float y = u + cfg_weight * (c - u);     // the expression of cfg_scan_kernel
                    float x = scaled ? __fmul_rn(y, invT) : y;
                    if (nt * 16 + j >= lim) x = -INFINITY;
                    if (nt * 16 + j == tcol[q]) xt = x;
                    xs[nt * 4 + j] = x;
                    mx = fmaxf(mx, x);
                }
            const float mn = fmaxf(mrun[q], mx), mref = mn == -INFINITY ? 0.f : mn;
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sum += expf(xs[i] - mref);
            srun[q] = srun[q] * expf(mrun[q] - mref) + sum;
            mrun[q] = mn;
            const int tc = tcol[q];
            if (tc >= 0 && tc < 64 && (tc & 15) < 4) out[p0 + wr * 64 + q * 16 + lr] = xt;      // the one lane that holds column t of this pair
        }
    }
#undef SH_MFMA_SECTION
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // clamped tail stages must not outlive the block's LDS
    // ---- merge: the row's four lanes (g = 0..3), then the four column waves in ascending order
    float2* red = (float2*)(smem + 2 * SH_BUF);           // [wc][CH_PAIRS]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float m = mrun[q], s = srun[q];
        sh_merge(m, s, __shfl_xor(m, 16, 64), __shfl_xor(s, 16, 64));
        sh_merge(m, s, __shfl_xor(m, 32, 64), __shfl_xor(s, 32, 64));
        if (g == 0) red[wc * CH_PAIRS + wr * 64 + q * 16 + lr] = make_float2(m, s);
    }
    __syncthreads();
    if (tid < CH_PAIRS && p0 + tid < n) {
        float2 p = red[tid];
        float m = p.x, s = p.y;
#pragma unroll
        for (int c = 1; c < 4; ++c) { p = red[c * CH_PAIRS + tid]; sh_merge(m, s, p.x, p.y); }
        *(float2*)(part + ((long)grp * n + p0 + tid) * 2) = make_float2(m, s);
    }
}

bool launch_cfg_head_logprob(hipStream_t s, const bf16* X, const bf16* W, const float* bias, const int32_t* cond_idx, const int32_t* uncond_idx,
                             const int32_t* target, long n, int V, int K, float cfg_weight, float temperature, float* part, float* out) {
    if (n < 1 || V < 1 || K < SH_BK || K % SH_BK || n > (1L << 29)) return false;
    const HeadGeom g = head_logprob_geom(2 * n, V, K);
    if ((long)g.ntm * g.G > 0x7fffffffL) return false;
    auto kfn = cfg_head_logprob_kernel;
    if (!PG_DYN_LDS(kfn, SH_LDS)) return false;
    hipLaunchKernelGGL(kfn, dim3(g.ntm * g.G), dim3(512), SH_LDS, s, X, W, bias, cond_idx, uncond_idx, target, (int)n, V, K, g.ntm, g.ntn, g.cpt, g.G,
                       cfg_weight, temperature, part, out);
    launch_head_combine(s, part, target, n, V, g.G, out);
    return true;
}

// fp32 engines (parity mode): logits [2 cn, V] of one chunk, cond rows first -- row i <- the mixed row of pair i (bias included), in place
__global__ __launch_bounds__(256) void cfg_mix_rows_kernel(float* __restrict__ logits, const float* __restrict__ bias, int cn, int V, float cfg_weight) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)cn * V) return;
    const float b = bias ? bias[i % V] : 0.f;
    const float c = logits[i] + b, u = logits[(long)cn * V + i] + b;
    logits[i] = u + cfg_weight * (c - u);
}
void launch_cfg_mix_rows(hipStream_t s, float* logits, const float* bias, int cn, int V, float cfg_weight) {
    hipLaunchKernelGGL(cfg_mix_rows_kernel, dim3((unsigned)(((long)cn * V + 255) / 256)), dim3(256), 0, s, logits, bias, cn, V, cfg_weight);
}
