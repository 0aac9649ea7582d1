// What the two fused scoring heads share (score_head.hip: lm_head; score_cfg_head.hip: the CFG-mixed gen_head): the tile constants, the
// barrier and the (max, sum) merge.  The geometry (head_logprob_geom) and the combine kernel's launcher are declared in kernels.h.
#pragma once
#include "gemm_common.h"

#define SH_BM 256
#define SH_BN 256
#define SH_BK 64
#define SH_AH (2 * 64 * 128)                 // bytes per A half-tile (2 wave rows x 64 rows x 128 B)
#define SH_BH (4 * 32 * 128)                 // bytes per W half-tile (4 wave columns x 32 rows x 128 B)
#define SH_BUF (2 * SH_AH + 2 * SH_BH)       // one K tile: [HA0 | HA1 | HB0 | HB1]
#define SH_LDS (2 * SH_BUF + 4 * SH_BM * 8)
#define SH_TARGET_BLOCKS 256                 // blocks per round the group count is sized for (one per CU of an MI355X; a constant, so G never depends on the device)

__device__ __forceinline__ void sh_barrier() { asm volatile("s_barrier" ::: "memory"); }
// (m, s) <- (m, s) (+) (mo, so) with both sums rescaled to the common maximum; an empty side is (-inf, 0)
__device__ __forceinline__ void sh_merge(float& m, float& s, float mo, float so) {
    const float mn = fmaxf(m, mo), mref = mn == -INFINITY ? 0.f : mn;
    s = s * expf(m - mref) + so * expf(mo - mref);
    m = mn;
}

