// LoRA merge at load time: W[o][i] <- T((float)W[o][i] + scale * sum_k B[o][k] A[k][i]), in place, in the layout the weight slot already has
// (pg_merge_lora).  The arithmetic per element is a CONTRACT that tests/lora_ref.py reproduces bit for bit on the host:
//
//     acc = 0.0f;  for k = 0 .. r - 1 ascending:  acc = acc (+) (B[o][k] (*) A[k][i])        (*) and (+): fp32, round to nearest even, never fused
//     m = (float)W[o][i] (+) (scale (*) acc);     W[o][i] = T(m)                              bf16: round to nearest even (common.h)
//
// One thread carries one element's accumulator through every k-chunk in order, so the result does not depend on the tile, the grid or the thread that
// computes it.  Plain fp32 VALU work (an MFMA's internal summation order is not the contract): rank 256 on 2048 x 2048 is ~1 G multiplies and ~1 G adds.
//
// Tile: LM_OT = 32 rows of `out` x LM_IT = 128 columns of `in` per 256-thread block, k in chunks of LM_KC = 32 staged through LDS.  Thread (ty, tx) =
// (tid / 16, tid % 16) owns rows ty and ty + 16 and the 8 consecutive columns 8 tx .. 8 tx + 7: its 8 values of A are two ds_read_b128 (16 lanes cover one
// 512-byte row of the A tile, the four ty of a wave read the same addresses: a broadcast), its two values of B are broadcast reads of sB[row][k] whose row
// pitch of LM_KC + 1 words keeps the four rows of a wave on different banks.  W is read and written 16 bytes at a time where the 8 elements are inside the
// row and their address is 16-byte aligned (every row when `in` * sizeof(T) is a multiple of 16 and the base is aligned; some rows otherwise), else
// element by element with a bounds check -- the ragged tail of `in` takes that path.  A is staged the same way (16 bytes or element-wise), B element-wise.
#include "kernels.h"

#define LM_OT 32
#define LM_IT 128
#define LM_KC 32

namespace {

// fp32 multiply and add that the compiler may not contract into an FMA (the build's default lets it fuse a * b + c)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// destination row of row o: which < 0 row-major; which = 0 / 1 the gate / up half of the [8 gate | 8 up] interleave (convert_il16_kernel)
__device__ __forceinline__ long dst_row(int o, int which) { return which < 0 ? (long)o : ((long)(o >> 3) * 16 + which * 8 + (o & 7)); }

template <typename T>
__global__ __launch_bounds__(256) void lora_merge_kernel(T* __restrict__ W, int which, int out, int in, const float* __restrict__ A,
                                                         const float* __restrict__ B, int r, float scale) {
    __shared__ __attribute__((aligned(16))) float sA[LM_KC][LM_IT];
    __shared__ float sB[LM_OT][LM_KC + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.x * LM_IT, o0 = blockIdx.y * LM_OT;
    const int c0 = i0 + tx * 8;                                 // this thread's first column
    float acc[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] = 0.0f;

    for (int k0 = 0; k0 < r; k0 += LM_KC) {
        const int kc = r - k0 < LM_KC ? r - k0 : LM_KC;
        // A[k0 .. k0 + kc)[i0 .. i0 + 128): 32 x 32 vectors of 4, 4 per thread; columns past `in` read as 0 (they are never stored)
#pragma unroll
        for (int p = 0; p < (LM_KC * LM_IT / 4) / 256; ++p) {
            const int v = p * 256 + tid, kk = v >> 5, c = i0 + (v & 31) * 4;
            f32x4 q = {0.f, 0.f, 0.f, 0.f};
            if (kk < kc) {
                const float* src = A + (long)(k0 + kk) * in + c;
                if (c + 4 <= in && ((uintptr_t)src & 15) == 0) q = *(const f32x4*)src;
                else {
                    if (c < in) q.x = src[0];
                    if (c + 1 < in) q.y = src[1];
                    if (c + 2 < in) q.z = src[2];
                    if (c + 3 < in) q.w = src[3];
                }
            }
            *(f32x4*)&sA[kk][(v & 31) * 4] = q;
        }
        // B[o0 .. o0 + 32)[k0 .. k0 + kc): 1024 elements, 4 per thread, a wave reads two 128-byte row segments
#pragma unroll
        for (int p = 0; p < (LM_OT * LM_KC) / 256; ++p) {
            const int e = p * 256 + tid, row = e / LM_KC, kk = e % LM_KC;
            sB[row][kk] = (o0 + row < out && kk < kc) ? B[(long)(o0 + row) * r + k0 + kk] : 0.f;
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
            const f32x4 a0 = *(const f32x4*)&sA[kk][tx * 8], a1 = *(const f32x4*)&sA[kk][tx * 8 + 4];
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float b0 = sB[ty][kk], b1 = sB[ty + 16][kk];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[0][j] = add_rn(acc[0][j], mul_rn(b0, a[j]));
                acc[1][j] = add_rn(acc[1][j], mul_rn(b1, a[j]));
            }
        }
        __syncthreads();
    }

    if (c0 >= in) return;
    constexpr int EPV = ET<T>::EPV;                             // 8 (bf16: one 16-byte vector per thread and row) or 4 (fp32: two)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int o = o0 + ty + 16 * h;
        if (o >= out) continue;
        T* w = W + dst_row(o, which) * in + c0;
        if (c0 + 8 <= in && ((uintptr_t)w & 15) == 0) {
#pragma unroll
            for (int v = 0; v < 8 / EPV; ++v) {
                float f[EPV];
                ET<T>::unpack(*(const u32x4*)(w + v * EPV), f);
#pragma unroll
                for (int j = 0; j < EPV; ++j) f[j] = add_rn(f[j], mul_rn(scale, acc[h][v * EPV + j]));
                *(u32x4*)(w + v * EPV) = ET<T>::pack(f);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < in) ET<T>::st(w + j, add_rn(ET<T>::ld(w + j), mul_rn(scale, acc[h][j])));
        }
    }
}

}  // namespace

template <typename T>
bool launch_lora_merge(hipStream_t s, T* W, int layout, int out, int in, const float* A, const float* B, int r, float scale) {
    const long gx = ((long)in + LM_IT - 1) / LM_IT, gy = ((long)out + LM_OT - 1) / LM_OT;
    if (out < 1 || in < 1 || r < 1 || (layout != LORA_K_T && layout != LORA_K_IL16_G && layout != LORA_K_IL16_U) || gy > 65535) return false;
    if (layout != LORA_K_T && (out & 7)) return false;           // the last block of 8 rows would fall behind row 2 out - 1
    const int which = layout == LORA_K_T ? -1 : layout == LORA_K_IL16_U;
    hipLaunchKernelGGL(lora_merge_kernel<T>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, W, which, out, in, A, B, r, scale);
    return true;
}
template bool launch_lora_merge<float>(hipStream_t, float*, int, int, int, const float*, const float*, int, float);
template bool launch_lora_merge<bf16>(hipStream_t, bf16*, int, int, int, const float*, const float*, int, float);
