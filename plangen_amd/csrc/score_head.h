// What the two fused scoring heads share (score_head.hip: lm_head; score_cfg_head.hip: the CFG-mixed gen_head).  Both walk column tiles on
// tile256.h's two-phase pipeline; this header holds everything around it that is not the gather or the fold's input: the block mapping, the
// online (max, sum) update, the end-of-block merge and the launch checks.  The geometry (head_logprob_geom) and the combine kernel's
// launcher are declared in kernels.h.
#pragma once
#include "tile256.h"

#define SH_BM 256
#define SH_BN 256
#define SH_LDS (T256_STAGING + 4 * SH_BM * 8)     // + the merge's own region: the clamped tail stages of the last K tile may still be landing in the staging buffers
#define SH_TARGET_BLOCKS 256                 // blocks per round the group count is sized for (one per CU of an MI355X; a constant, so G never depends on the device)

// block -> (row tile, group of column tiles [c0, c1)): an XCD's share of the grid is 4 row tiles x all groups, so its L2 holds 4 A panels
// while the W tiles stream
struct HeadBlock { int tile, grp, c0, c1; };
__device__ __forceinline__ HeadBlock sh_block(int ntm, int ntn, int cpt, int G) {
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int per = 4 * G, mg = t / per, rem = t - mg * per, gm = min(4, ntm - mg * 4);
    HeadBlock b;
    b.tile = mg * 4 + rem % gm; b.grp = rem / gm;
    b.c0 = b.grp * cpt; b.c1 = min(ntn, b.c0 + cpt);
    return b;
}

// (m, s) <- (m, s) (+) (mo, so) with both sums rescaled to the common maximum; an empty side is (-inf, 0)
__device__ __forceinline__ void sh_merge(float& m, float& s, float mo, float so) {
    const float mn = fmaxf(m, mo), mref = mn == -INFINITY ? 0.f : mn;
    s = s * expf(m - mref) + so * expf(mo - mref);
    m = mn;
}

// the target's column relative to the lane's first column ecol, -1 when the row is padding or the target is outside [0, V)
__device__ __forceinline__ int sh_target_col(const int32_t* __restrict__ target, int row, int n, int V, int ecol) {
    const int tg = target[row < n ? row : n - 1];
    return (row < n && tg >= 0 && tg < V) ? tg - ecol : -1;
}

// Online update of one row's running (m, s) with the lane's 16 logits of a column tile, y(nt, j) = column nt*16 + j behind the lane's first:
// x = y / temperature when scaled; columns >= lim are past the vocabulary and fold as -inf; m' = max(m, max of the 16),
// s = s * expf(m - m') + sum expf(x - m') -- 17 accurate expf.  The lane that holds the target column (tcol) stores x_t to out[row].
template <class F>
__device__ __forceinline__ void sh_fold16(F y, int lim, int tcol, bool scaled, float invT, float& mrun, float& srun, float* __restrict__ out, int row) {
    float xs[16];
    float mx = -INFINITY, xt = 0.f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float yv = y(nt, j);
            float x = scaled ? __fmul_rn(yv, invT) : yv;
            if (nt * 16 + j >= lim) x = -INFINITY;
            if (nt * 16 + j == tcol) xt = x;
            xs[nt * 4 + j] = x;
            mx = fmaxf(mx, x);
        }
    const float mn = fmaxf(mrun, mx), mref = mn == -INFINITY ? 0.f : mn;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += expf(xs[i] - mref);
    srun = srun * expf(mrun - mref) + sum;
    mrun = mn;
    if (tcol >= 0 && tcol < 64 && (tcol & 15) < 4) out[row] = xt;      // the one lane that holds column t of this row
}

// End of a block: a lane holds RPL running (m, s), entry i for scored row wr*16*RPL + i*16 + lr of the block's 32 RPL rows (RPL = 8: 256 raw
// rows; 4: 128 CFG pairs).  The row's four lanes (g = 0..3, shuffles), then the four column waves (LDS `red`, ascending) merge in a fixed
// order; row0 + r < n goes to part[grp][row0 + r].
template <int RPL, class TILE>
__device__ __forceinline__ void sh_block_merge(const TILE& T, float2* red, const float (&mrun)[RPL], const float (&srun)[RPL], int row0, int n, int grp,
                                               float* __restrict__ part) {
    constexpr int ROWS = 32 * RPL;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        float m = mrun[i], s = srun[i];
        sh_merge(m, s, __shfl_xor(m, 16, 64), __shfl_xor(s, 16, 64));
        sh_merge(m, s, __shfl_xor(m, 32, 64), __shfl_xor(s, 32, 64));
        if (T.g == 0) red[T.wc * ROWS + T.wr * (16 * RPL) + i * 16 + T.lr] = make_float2(m, s);
    }
    __syncthreads();
    if (tid < ROWS && row0 + tid < n) {
        float2 p = red[tid];
        float m = p.x, s = p.y;
#pragma unroll
        for (int c = 1; c < 4; ++c) { p = red[c * ROWS + tid]; sh_merge(m, s, p.x, p.y); }
        *(float2*)(part + ((long)grp * n + row0 + tid) * 2) = make_float2(m, s);
    }
}

// launch-time checks of a head over `rows` A rows (n, or 2 n for CFG pairs) and its geometry
static inline bool sh_launch_geom(long rows, int V, int K, HeadGeom& g) {
    if (rows < 1 || V < 1 || K < T256_BK || K % T256_BK || rows > (1L << 30)) return false;
    g = head_logprob_geom(rows, V, K);
    return (long)g.ntm * g.G <= 0x7fffffffL;
}
