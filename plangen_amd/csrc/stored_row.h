// The stored-row route's reader, shared by its two reducers: token_logprob_kernel (sampler.hip) and token_stats_kernel (token_stats.hip).
// One SR_THREADS-thread block per row y the step's scan has just stored (L2 resident; 400 KiB at vocab 102 400).  Both kernels find their
// position -- the emitted token, the temperature, the index of their outputs -- with sr_locate and walk x = y * (1 / temperature) with
// StoredRow::each, so a thread of either visits the same entries in the same order: aligned 16-byte vectors in index order (eight loads
// in flight, as in text_scan_body.h), then the scalar head, then the tail -- the row may start at any 4-byte boundary and have any
// length.  With the kernels' reduction shape (xor butterfly over the wave, serial sum of the 16 wave values) that order fixes the bits of
// sum expf(x - max): token_stats_kernel's logprob has token_logprob_kernel's bits because both sums are formed here.
#pragma once
#include "kernels.h"

#define SR_THREADS 1024
#define SR_WAVES (SR_THREADS / 64)

struct StoredRowArgs {
    const float* rows; int V;                                     // [gridDim, V] fp32
    const SampleParams* sp;                                       // image loop: temperature and T from device memory
    const TextParams* tp;                                         // text loop: temperature, max_new and eos from device memory
    float temperature;                                            // operator: from the host
    const int32_t* tok32;                                         // operator: [gridDim]; image loop: out_tok [B, T]
    const int64_t* tok64;                                         // text loop: out [B, max_new]
    const int32_t* n_dec; int b_off;                              // loops: device step counter, first image of this launch
};
struct LogprobArgs : StoredRowArgs { float* out; };               // operator: [gridDim]; loops: [B, T] / [B, max_new] library-owned
struct LogprobArgsPlan : LogprobArgs { const float* plan_temperature; };      // [B_total]: the image loop under a sample plan
struct StatsArgs : StoredRowArgs { TokenStatsOut o; };
struct StatsArgsPlan : StatsArgs { const float* plan_temperature; };

enum { SR_OP = 0, SR_IMAGE = 1, SR_TEXT = 2, SR_IMAGE_PLAN = 3 };      // SR_IMAGE_PLAN: SR_IMAGE with the image's own temperature (sample plan)
// the argument struct of a form, by specialisation: an expression over the unnamed enum in the kernel's signature would put the enum's
// compiler-made name into the mangled symbol, and the host and device passes number such names differently
template <int FORM, class Plain, class Plan> struct SrArgsOf { using type = Plain; };
template <class Plain, class Plan> struct SrArgsOf<3, Plain, Plan> { using type = Plan; };

// Where block b stands: the emitted token, the temperature and the index of this position's outputs ([gridDim], [B, T] or [B, max_new]).
enum { SR_LIVE = 0, SR_PAST = 1, SR_FINISHED = 2 };               // SR_PAST: the loop is past its last step, nothing to write;
                                                                   // SR_FINISHED: a text row finished before this step (the kernel writes its own constants at `at`)
template <int FORM, class A>
__device__ __forceinline__ int sr_locate(const A& a, int b, int& tok, float& temperature, long& at) {
    tok = 0; temperature = 0.f; at = b;
    if (FORM == SR_OP) { tok = a.tok32[b]; temperature = a.temperature; }
    else if (FORM == SR_IMAGE || FORM == SR_IMAGE_PLAN) {
        const int step = *a.n_dec, T = a.sp->T;
        if (step >= T) return SR_PAST;
        at = (long)(b + a.b_off) * T + step;
        tok = a.tok32[at];
        if constexpr (FORM == SR_IMAGE_PLAN) temperature = a.plan_temperature[b + a.b_off]; else temperature = a.sp->temperature;
    } else {
        const int step = *a.n_dec, max_new = a.tp->max_new;
        if (step >= max_new) return SR_PAST;
        const int64_t* o = a.tok64 + (long)b * max_new;
        at = (long)b * max_new + step;
        // a finished row emits eos and a row finishes by emitting eos: the row was finished BEFORE this step iff its previous token is eos
        if (step > 0 && o[step - 1] == (int64_t)a.tp->eos) return SR_FINISHED;
        tok = (int)o[step]; temperature = a.tp->temperature;
    }
    return SR_LIVE;
}

struct StoredRow {
    const float* row; const f32x4* rv;                            // the row; its 16-byte aligned vectors
    int V, head, nv, tail0;                                       // [0, head) scalar head, nv vectors, [tail0, V) scalar tail
    float temperature, invT;
    __device__ __forceinline__ StoredRow(const float* row_, int V_, float temperature_)
        : row(row_), V(V_), temperature(temperature_), invT(temperature_ > 0.f ? 1.f / temperature_ : 1.f) {
        head = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);
        if (head > V) head = V;
        nv = (V - head) >> 2; tail0 = head + nv * 4;
        rv = (const f32x4*)(row + head);
    }
    __device__ __forceinline__ float xval(float y) const {       // the rounded product, never fused into x - m
        const float x = temperature > 0.f ? __fmul_rn(y, invT) : y;
        return x != x ? -INFINITY : x;
    }
    // f(y, v, fresh) over this thread's entries.  CLAMPED: a vector index past the end loads the last vector again and f sees those
    // repeats with fresh = false (they do not move a maximum); otherwise every entry exactly once, fresh = true (sums, counts).
    template <bool CLAMPED, class F>
    __device__ __forceinline__ void each(int tid, F f) const {
        constexpr int IT = 8;
        for (int i0 = tid; i0 < nv; i0 += IT * SR_THREADS) {
            f32x4 c[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) { const int i = i0 + it * SR_THREADS; c[it] = rv[i < nv ? i : nv - 1]; }
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int i = i0 + it * SR_THREADS;
                if (CLAMPED || i < nv) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) f(c[it][j], head + i * 4 + j, i < nv);
                }
            }
        }
        for (int v = tid; v < head; v += SR_THREADS) f(row[v], v, true);
        for (int v = tail0 + tid; v < V; v += SR_THREADS) f(row[v], v, true);
    }
};
