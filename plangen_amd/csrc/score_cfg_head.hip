// Fused CFG-mixed gen_head layer 2 + log-softmax at a target (pg_score_image_tokens / pg_op_cfg_head_logprob): score_head.hip's kernel with
// a classifier-free-guidance mix between the accumulators and the fold.  Per scored position i (c = cond_idx[i], u = uncond_idx[i], t = target[i]):
//
//   yc_v = sum_k X[c][k] * W[v][k] + bias[v],   yu_v likewise with X[u]     (bf16 operands, fp32 accumulation on the MFMA units; bias fp32 or absent)
//   y_v  = yu_v + cfg_weight * (yc_v - yu_v)                                (fp32, the expression of cfg_scan_kernel in sampler.hip)
//   x_v  = y_v * (1 / temperature)  when temperature > 0, else y_v          (the rounded fp32 product)
//   out[i] = (x_t - m) - logf(sum_v expf(x_v - m)),  m = max_v x_v;   t outside [0, V) gives -inf
//
// Neither the two [n, V] logit tensors nor the mixed one leave registers.  NaN / inf operands are NOT covered, as in score_head.hip.
//
// Same structure as head_logprob_kernel (tile256.h's 256 x 256 two-phase tile per column tile, column-tile groups, the XCD remap, [G][n][2]
// partials merged by head_combine_kernel; the shared pieces are score_head.h's); the geometry is head_logprob_geom(2 n, V, K): a row tile
// holds CH_PAIRS = 128 pairs.  What differs:
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
    const HeadBlock b = sh_block(ntm, ntn, cpt, G);
    const int p0 = b.tile * CH_PAIRS;                         // first pair of the row tile
    GatherLoader al;
    Tile256<GatherLoader> T(al, smem, K);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        // tile row = accumulator row mt (16 rows each) x lane row: pair (wave row)*64 + (mt>>1)*16 + lane row, cond when mt is even
        const int r = T.slot_row(s), mt = r >> 4;
        const int p = p0 + T.slot_wr(s) * 64 + (mt >> 1) * 16 + (r & 15), pc = p < n ? p : n - 1;
        al.init(s, X + (long)((mt & 1) ? uncond_idx[pc] : cond_idx[pc]) * K);
    }

    f32x4 acc[8][4];
    float mrun[4], srun[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { mrun[i] = -INFINITY; srun[i] = 0.f; }
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const bool scaled = temperature > 0.f;
    const int pair0 = p0 + T.wr * 64 + T.lr;                  // the lane's pairs: pair0 + q*16

    T.set_W(W, K, b.c0 * SH_BN, V);
    T.prologue();
    for (int ct = b.c0; ct < b.c1; ++ct) {
        T.run(acc);
        // every wave is past its last ds_read: the next column tile's first loads go out before this tile's fold
        const int ecol = ct * SH_BN + T.wc * 64 + T.g * 4;    // the lane's first column; n-tile nt, element j -> ecol + nt*16 + j
        if (ct + 1 < b.c1) { T.set_W(W, K, (ct + 1) * SH_BN, V); T.prologue(); }
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
        for (int q = 0; q < 4; ++q) tcol[q] = sh_target_col(target, pair0 + q * 16, n, V, ecol);
#pragma unroll
        for (int q = 0; q < 4; ++q)                           // pair q: cond in accumulator row 2q, uncond in 2q + 1 -- the mix never leaves the lane
            sh_fold16([&](int nt, int j) {
                const float c = acc[2 * q][nt][j] + bv[nt * 4 + j], u = acc[2 * q + 1][nt][j] + bv[nt * 4 + j];
                return u + cfg_weight * (c - u);              // the expression of cfg_scan_kernel
            }, V - ecol, tcol[q], scaled, invT, mrun[q], srun[q], out, pair0 + q * 16);
    }
    T.drain();
    sh_block_merge<4>(T, (float2*)(smem + T256_STAGING), mrun, srun, p0, n, b.grp, part);
}

bool launch_cfg_head_logprob(hipStream_t s, const bf16* X, const bf16* W, const float* bias, const int32_t* cond_idx, const int32_t* uncond_idx,
                             const int32_t* target, long n, int V, int K, float cfg_weight, float temperature, float* part, float* out) {
    HeadGeom g;
    if (!sh_launch_geom(2 * n, V, K, g)) return false;
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
