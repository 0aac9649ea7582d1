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
// * SH_BM = 256 scored rows x SH_BN = 256 vocabulary columns per tile, K step 64 (K % 64 == 0): one tile of tile256.h's two-phase pipeline
//   (eight waves, each owning 128 x 64 of the tile as 8 x 4 MFMA tiles); the A rows are gathered through row_idx.
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
#include "score_head.h"

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

__global__ __launch_bounds__(512) void head_logprob_kernel(const bf16* __restrict__ X, const bf16* __restrict__ W, const int32_t* __restrict__ row_idx,
                                                           const int32_t* __restrict__ target, int n, int V, int K, int ntm, int ntn, int cpt, int G,
                                                           float temperature, float* __restrict__ part, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HeadBlock b = sh_block(ntm, ntn, cpt, G);
    const int m0 = b.tile * SH_BM;
    GatherLoader al;
    Tile256<GatherLoader> T(al, smem, K);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int m = m0 + T.slot_wr(s) * 128 + T.slot_row(s), mc = m < n ? m : n - 1;
        al.init(s, X + (long)(row_idx ? row_idx[mc] : mc) * K);
    }

    f32x4 acc[8][4];
    float mrun[8], srun[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { mrun[i] = -INFINITY; srun[i] = 0.f; }
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const bool scaled = temperature > 0.f;
    const int row0 = m0 + T.wr * 128 + T.lr;                  // the lane's rows: row0 + mt*16

    T.set_W(W, K, b.c0 * SH_BN, V);
    T.prologue();
    for (int ct = b.c0; ct < b.c1; ++ct) {
        T.run(acc);
        // every wave is past its last ds_read: the next column tile's first loads go out before this tile's fold
        const int ecol = ct * SH_BN + T.wc * 64 + T.g * 4;    // the lane's first column; n-tile nt, element j -> ecol + nt*16 + j
        if (ct + 1 < b.c1) { T.set_W(W, K, (ct + 1) * SH_BN, V); T.prologue(); }
        int tcol[8];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) tcol[mt] = sh_target_col(target, row0 + mt * 16, n, V, ecol);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
            sh_fold16([&](int nt, int j) { return acc[mt][nt][j]; }, V - ecol, tcol[mt], scaled, invT, mrun[mt], srun[mt], out, row0 + mt * 16);
    }
    T.drain();
    sh_block_merge<8>(T, (float2*)(smem + T256_STAGING), mrun, srun, m0, n, b.grp, part);
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

void launch_head_combine(hipStream_t s, const float* part, const int32_t* target, long n, int V, int G, float* out) {
    hipLaunchKernelGGL(head_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, target, (int)n, V, G, out);
}

bool launch_head_logprob(hipStream_t s, const bf16* X, const bf16* W, const int32_t* row_idx, const int32_t* target, long n, int V, int K,
                         float temperature, float* part, float* out) {
    HeadGeom g;
    if (!sh_launch_geom(n, V, K, g)) return false;
    auto kfn = head_logprob_kernel;
    if (!PG_DYN_LDS(kfn, SH_LDS)) return false;
    hipLaunchKernelGGL(kfn, dim3(g.ntm * g.G), dim3(512), SH_LDS, s, X, W, row_idx, target, (int)n, V, K, g.ntm, g.ntn, g.cpt, g.G, temperature, part, out);
    launch_head_combine(s, part, target, n, V, g.G, out);
    return true;
}
