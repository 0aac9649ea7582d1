// FP8 KV cache (pg_config.kv_dtype = PG_FP8_E4M3): the storage format and its device quantiser, shared by the decode-attention append
// (attn_decode.h), kv_quantize_kernel and pg_op_kv_quantize (llm_kernels.hip).  The contract (include/plangen_hip.h): every 128-element
// K or V row of a (row, head, slot) is stored as 128 OCP e4m3fn codes plus ONE power-of-two scale 2^e, e the smallest integer with
// amax * 2^-e <= 448 clamped to [-100, 100] (amax == 0: e = 0); code = e4m3_rne(x * 2^-e).  x * 2^-e and code * 2^e are exact in fp32,
// so the CPU reference (tests/kv8_ref.py) and the device agree bit for bit, and the scaled value never reaches the saturation point.
// Scales live interleaved per slot: float [rows][heads][slots][2] = (K scale, V scale).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(2))) float f32x2;

__device__ __forceinline__ int kv8_exponent(float amax) {
    const uint32_t b = __float_as_uint(amax) & 0x7fffffffu;
    if (b == 0) return 0;
    // amax = 1.f * 2^(E - 127) and 448 = 1.75 * 2^8: e = E - 127 - 8 while the mantissa is <= 1.75, one more above it
    const int e = (int)(b >> 23) - 135 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}
__device__ __forceinline__ float kv8_pow2(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }      // |e| <= 100: a normal fp32
// two / four scaled values -> e4m3fn codes (v_cvt_pk_fp8_f32: round to nearest even), lowest byte first
__device__ __forceinline__ uint32_t kv8_pack2(float a, float b, float inv) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, 0, false) & 0xffffu;
}
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d, float inv) {
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c * inv, d * inv, r, true);
    return (uint32_t)r;
}
// 16 codes (one 16-byte load) -> 16 floats (v_cvt_pk_f32_fp8), unscaled
__device__ __forceinline__ void kv8_unpack16(const u32x4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        f[4 * i] = lo.x; f[4 * i + 1] = lo.y; f[4 * i + 2] = hi.x; f[4 * i + 3] = hi.y;
    }
}
// One wave quantises one 128-element bf16 row (2 elements per lane): codes to dst[0..128), the scale to *sc.
__device__ __forceinline__ void kv8_quant_row(const bf16* __restrict__ src, uint8_t* __restrict__ dst, float* __restrict__ sc, int l) {
    const uint32_t pk = *(const uint32_t*)(src + 2 * l);
    const float a = bf16_lo(pk), b = bf16_hi(pk);
    const float amax = wave_max(fmaxf(fabsf(a), fabsf(b)));
    const int e = kv8_exponent(amax);
    *(uint16_t*)(dst + 2 * l) = (uint16_t)kv8_pack2(a, b, kv8_pow2(-e));
    if (l == 0) *sc = kv8_pow2(e);
}
