// Fused lm_head + log-softmax at a target (pg_score_tokens / pg_op_head_logprob): the flash-attention idea over the vocabulary.
//
//   y_v    = sum_k X[row_idx[i]][k] * W[v][k]                       (bf16 operands, fp32 accumulation on the MFMA units)
//   x_v    = y_v * (1 / temperature)  when temperature > 0, else y_v (the rounded fp32 product, as token_logprob_kernel)
//   out[i] = (x_t - m) - logf(sum_v expf(x_v - m)),  m = max_v x_v,  t = target[i];   t outside [0, V) gives -inf
//
// The [n, V] logits never leave registers.  NaN / inf operands are NOT covered (a NaN logit poisons its row; token_logprob_kernel's
// NaN-as--inf rule is not reproduced).
//
// Geometry (fixed; G is a function of (n, V, K) alone -- head_logprob_geom, mirrored by plangen_amd.engine.head_logprob_geometry):
// * SH_BM = 256 scored rows x SH_BN = 256 vocabulary columns per tile, K step SH_BK = 64 (K % 64 == 0), eight waves, each owning 128 x 64 of
//   the tile as 8 x 4 MFMA tiles (mfma_f32_16x16x32_bf16): the staging stream, the swizzled LDS layout, the two-phase schedule and its counted
//   waits are those of gemm256.hip's 256x256 two-phase form (the invariants are written down there); the A rows are gathered through row_idx.
// * A block owns ONE row tile and a contiguous group of `cpt` column tiles (G = ceil(ntn / cpt) groups) and walks them with the K loop per
//   tile; the next tile's first loads go out before the current tile's fold, as gemm256 does before its stores.
// * Fold after each column tile: a lane holds, for each of its 8 rows, 16 columns of the tile (4 n-tiles x 4).  It keeps a running (m, s)
//   per row for ITS columns: m' = max(m, max of the 16), s = s * expf(m - m') + sum expf(x - m') -- 17 accurate expf per row and tile.  The
//   lane that holds the target column stores x_t to out[i]: exactly one lane of one block does (plain store, no atomics).
// * End of block: the four lanes of a row (shuffles, fixed order), then the four column waves (LDS, ascending) merge into one (m, s) per row,
//   written to the partials workspace [G][n][2] fp32.  head_combine_kernel merges the G groups in ascending order and finishes out[i].
// * Every reduction has a fixed shape that does not depend on the row's slot in the batch or on other rows: a row's bits are a function of
//   its X row, W, its target, the temperature and (n, V, K).
// * Rows >= n of the last row tile re-read row n - 1 (results dropped); columns >= V re-read W row V - 1 and are folded as -inf.
// * LDS: 128 KiB of staging + 8 KiB for the end-of-block merge (its own region: the clamped tail stages of the last K tile may still be
//   landing in the staging buffers) = 136 KiB, one block per CU, like gemm256 (MI355X: 160 KiB per CU).
#include "gemm_common.h"

#define SH_BM 256
#define SH_BN 256
#define SH_BK 64
#define SH_AH (2 * 64 * 128)                 // bytes per A half-tile (2 wave rows x 64 rows x 128 B)
#define SH_BH (4 * 32 * 128)                 // bytes per W half-tile (4 wave columns x 32 rows x 128 B)
#define SH_BUF (2 * SH_AH + 2 * SH_BH)       // one K tile: [HA0 | HA1 | HB0 | HB1]
#define SH_LDS (2 * SH_BUF + 4 * SH_BM * 8)
#define SH_TARGET_BLOCKS 256                 // blocks per round the group count is sized for (one per CU of an MI355X; a constant, so G never depends on the device)

HeadGeom head_logprob_geom(long n, int V, int K) {
    HeadGeom g{};
    g.ntm = (int)((n + SH_BM - 1) / SH_BM); g.ntn = (V + SH_BN - 1) / SH_BN;
    // cost of a choice = rounds of SH_TARGET_BLOCKS blocks x (column tiles per block + 1 for the pipeline fill and the merge); ties keep fewer groups
    long best = -1;
    for (int cpt = g.ntn; cpt >= 1; --cpt) {
        const int G = (g.ntn + cpt - 1) / cpt;
        const long cost = (((long)g.ntm * G + SH_TARGET_BLOCKS - 1) / SH_TARGET_BLOCKS) * (cpt + 1);
        if (best < 0 || cost < best) { best = cost; g.cpt = cpt; g.G = G; }
    }
    return g;
}
size_t head_logprob_ws_bytes(long n, int V, int K) {
    const HeadGeom g = head_logprob_geom(n, V, K);
    return (((size_t)2 * 4 * g.G * (size_t)n) + 255) & ~(size_t)255;
}

__device__ __forceinline__ void sh_barrier() { asm volatile("s_barrier" ::: "memory"); }
// (m, s) <- (m, s) (+) (mo, so) with both sums rescaled to the common maximum; an empty side is (-inf, 0)
__device__ __forceinline__ void sh_merge(float& m, float& s, float mo, float so) {
    const float mn = fmaxf(m, mo), mref = mn == -INFINITY ? 0.f : mn;
    s = s * expf(m - mref) + so * expf(mo - mref);
    m = mn;
}

__global__ __launch_bounds__(512) void head_logprob_kernel(const bf16* __restrict__ X, const bf16* __restrict__ W, const int32_t* __restrict__ row_idx,
                                                           const int32_t* __restrict__ target, int n, int V, int K, int ntm, int ntn, int cpt, int G,
                                                           float temperature, float* __restrict__ part, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = K / SH_BK;

    // block -> (row tile, group): an XCD's share of the grid is 4 row tiles x all groups, so its L2 holds 4 A panels while the W tiles stream
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int per = 4 * G, mg = t / per, rem = t - mg * per, gm = min(4, ntm - mg * 4);
    const int m0 = (mg * 4 + rem % gm) * SH_BM, grp = rem / gm;
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
            const int m = m0 + (r >> 6) * 128 + h * 64 + (r & 63), mc = m < n ? m : n - 1;
            arow[h * 2 + i] = X + (long)(row_idx ? row_idx[mc] : mc) * K;
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
    float mrun[8], srun[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { mrun[i] = -INFINITY; srun[i] = 0.f; }
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
        int tcol[8];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int m = m0 + wr * 128 + mt * 16 + lr;
            const int tg = target[m < n ? m : n - 1];
            tcol[mt] = (m < n && tg >= 0 && tg < V) ? tg - ecol : -1;
        }
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            float xs[16];
            float mx = -INFINITY, xt = 0.f;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float y = acc[mt][nt][j];
                    float x = scaled ? __fmul_rn(y, invT) : y;
                    if (nt * 16 + j >= lim) x = -INFINITY;
                    if (nt * 16 + j == tcol[mt]) xt = x;
                    xs[nt * 4 + j] = x;
                    mx = fmaxf(mx, x);
                }
            const float mn = fmaxf(mrun[mt], mx), mref = mn == -INFINITY ? 0.f : mn;
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sum += expf(xs[i] - mref);
            srun[mt] = srun[mt] * expf(mrun[mt] - mref) + sum;
            mrun[mt] = mn;
            const int tc = tcol[mt];
            if (tc >= 0 && tc < 64 && (tc & 15) < 4) out[m0 + wr * 128 + mt * 16 + lr] = xt;      // the one lane that holds column t of this row
        }
    }
#undef SH_MFMA_SECTION
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // clamped tail stages must not outlive the block's LDS
    // ---- merge: the row's four lanes (g = 0..3), then the four column waves in ascending order
    float2* red = (float2*)(smem + 2 * SH_BUF);           // [wc][SH_BM]
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        float m = mrun[mt], s = srun[mt];
        sh_merge(m, s, __shfl_xor(m, 16, 64), __shfl_xor(s, 16, 64));
        sh_merge(m, s, __shfl_xor(m, 32, 64), __shfl_xor(s, 32, 64));
        if (g == 0) red[wc * SH_BM + wr * 128 + mt * 16 + lr] = make_float2(m, s);
    }
    __syncthreads();
    if (tid < SH_BM && m0 + tid < n) {
        float2 p = red[tid];
        float m = p.x, s = p.y;
#pragma unroll
        for (int c = 1; c < 4; ++c) { p = red[c * SH_BM + tid]; sh_merge(m, s, p.x, p.y); }
        *(float2*)(part + ((long)grp * n + m0 + tid) * 2) = make_float2(m, s);
    }
}

// out[i] holds x_t (written by the one block that met column t; untouched when t is outside [0, V)): merge the G groups' (m, s) in ascending
// group order and finish the log-probability
__global__ __launch_bounds__(256) void head_combine_kernel(const float* __restrict__ part, const int32_t* __restrict__ target, int n, int V, int G,
                                                           float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = target[i];
    float m = -INFINITY;
    for (int g = 0; g < G; ++g) m = fmaxf(m, part[((long)g * n + i) * 2]);
    float s = 0.f;
    for (int g = 0; g < G; ++g) { const float2 p = *(const float2*)(part + ((long)g * n + i) * 2); s += p.y * expf(p.x - m); }
    out[i] = (t >= 0 && t < V) ? (out[i] - m) - logf(s) : -INFINITY;
}

bool launch_head_logprob(hipStream_t s, const bf16* X, const bf16* W, const int32_t* row_idx, const int32_t* target, long n, int V, int K,
                         float temperature, float* part, float* out) {
    if (n < 1 || V < 1 || K < SH_BK || K % SH_BK || n > (1L << 30)) return false;
    const HeadGeom g = head_logprob_geom(n, V, K);
    if ((long)g.ntm * g.G > 0x7fffffffL) return false;
    auto kfn = head_logprob_kernel;
    if (!PG_DYN_LDS(kfn, SH_LDS)) return false;
    hipLaunchKernelGGL(kfn, dim3(g.ntm * g.G), dim3(512), SH_LDS, s, X, W, row_idx, target, (int)n, V, K, g.ntm, g.ntn, g.cpt, g.G, temperature, part, out);
    hipLaunchKernelGGL(head_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)part, target, (int)n, V, g.G, out);
    return true;
}
