// The token samplers (one place for everything that turns a logit row into a token and scores it): the CFG-mix + argmax / Gumbel-max image
// sampler and its top-k / top-p form, the text scan / select / pick kernels with the grammar automaton, the token log-probability
// reducer of the stored-row route (its sibling token_stats_kernel is in token_stats.hip; both read rows through stored_row.h) and the RNG
// tap.  sel_thresholds and sel_draw are the one threshold walk and the one draw of both filtered samplers.
#include <type_traits>
#include "kernels.h"
#include "attn_decode.h"      // sum_slabs
#include "stored_row.h"

// ------------------------------------------------------------------------------- CFG + sample
// One block per image b over its NR adjacent rows of the logits.
//   NR = 2 (pg_decode_image_tokens): rows 2b = cond, 2b + 1 = uncond; mixed = u + w (c - u) (plangen_base.py:587), w = p->cfg_weight or the
//       plan's w[bg][step].
//   NR = 3 (pg_decode_image_tokens_dual; definition: include/plangen_hip.h): rows 3b = f (caption + layout), 3b + 1 = p (caption only),
//       3b + 2 = u (negative); mixed = (u + w_caption (p - u)) + w_layout (f - p), the two weights from device memory (DualWeights), like
//       every per-call value; p->cfg_weight is not read.
// Greedy: first index of the max (torch.argmax tie rule); temperature > 0: Gumbel-max == multinomial(softmax(mixed / T)).  Then the chosen
// (or forced) token's precomputed gen_aligner(gen_embed(tok)) row is written to all NR rows of the residual stream (plangen_base.py:602-604).
// Everything but the guidance source and the mixing expression is one body: the chunking, the load discipline, the slab sum (bias first, then
// slabs in index order: a row of a triple has the bits the pair scan gives that row), the tap, the store, the perturbation, the winner
// reduction and the forcing rules.
__device__ __forceinline__ void argmax_combine(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// Stage 1: grid (CFG_CHUNKS, B): each block scans V/CFG_CHUNKS logits of image b and leaves its
// local (value, index) winner; stage 2 (one block per image) combines the winners, applies the
// forcing rules and gathers the next embedding.
#define CFG_CHUNKS 16
// the sampler's perturbed value: Gumbel-max over mixed / T (cfg_scan_kernel and the filtered sampler's cfg_select_kernel
// draw through this one expression, so a filtered draw equals the unfiltered one whenever that one survives the filter)
__device__ __forceinline__ float gumbel_perturb(float mixed, float invT, uint64_t seed, uint64_t stream, int v) {
    const float uu = rng_uniform(seed, stream, v);
    return mixed * invT - __logf(-__logf(uu));
}
// The scan's argument struct: the plain SampleArgs, with the plan's arrays (PLAN) or the dual weights' address (NR = 3) behind it.
template <int NR, bool PLAN> struct CfgScanArgs { using type = typename std::conditional<PLAN, SampleArgsPlan, SampleArgs>::type; };
template <> struct CfgScanArgs<3, false> { using type = SampleArgsDual; };
// STORE (filtered sampler, stored-row route): write the mixed row to mix [B, V] and nothing else but the tap; the draw is left to cfg_select_kernel
// or to the scan that follows.  PLAN (pg_request_sample_plan, NR = 2): the block's image reads its own temperature, key and this step's weight
// from the plan's device arrays, once, in front of the loop.
template <int NR, bool STORE, bool PLAN = false>
__global__ __launch_bounds__(256) void cfg_scan_kernel(typename CfgScanArgs<NR, PLAN>::type a, float* __restrict__ pv, int* __restrict__ pi,
                                                       float* __restrict__ mix) {
    static_assert(NR == 2 || (NR == 3 && !PLAN), "pairs (plain or planned) and plain triples");
    __shared__ float sv[4]; __shared__ int si[4];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    const int bg = b + a.b_off, B = a.B_total;            // global image index (lane-independent results)
    const int per = (a.V + CFG_CHUNKS - 1) / CFG_CHUNKS, v0 = ch * per, v1 = min(a.V, v0 + per);
    const long r0 = (long)(NR * b) * a.V;
    float best = -INFINITY; int bi = 0x7fffffff;
    float temperature, cfg_weight = 0.f, w_c = 0.f, w_l = 0.f; uint64_t stream;
    if constexpr (PLAN) {
        const int T = a.p->T;
        temperature = a.plan.temperature[bg];
        cfg_weight = a.plan.w[(long)bg * T + (step < T ? step : T - 1)];
        stream = (uint64_t)a.plan.key[bg] * 1000003ull + step;
    } else {
        temperature = a.p->temperature;
        if constexpr (NR == 3) { w_c = a.dw->w_caption; w_l = a.dw->w_layout; } else cfg_weight = a.p->cfg_weight;
        stream = (uint64_t)(bg + a.p->img_off) * 1000003ull + step;
    }
    const uint64_t seed = a.p->seed;
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    // four vocabulary entries per thread per pass, ALL their loads (bias, the NR rows of every slab) issued before the first use
    // (indices clamped into the chunk): one memory round trip per pass instead of one per entry
    constexpr int IT = 4;
    const float* bias0 = a.bias ? a.bias : a.logits_partial + r0;     // no bias: any mapped address, value discarded
    int off[NR];                                                      // the image's rows are adjacent
#pragma unroll
    for (int r = 0; r < NR; ++r) off[r] = r * a.V;
    for (int vb = v0 + tid; vb < v1; vb += IT * 256) {
        float bb[IT], row[IT][NR];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256, vc = v < v1 ? v : v1 - 1;
            bb[it] = bias0[vc];
        }
        float t[IT][4][NR];
        const int smax = a.S > 0 ? a.S - 1 : 0;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256, vc = v < v1 ? v : v1 - 1;
            const float* pp = a.logits_partial + r0 + vc;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* q = pp + (long)(u < smax ? u : smax) * a.slab;       // slab index clamped: branch-free loads
#pragma unroll
                for (int r = 0; r < NR; ++r) t[it][u][r] = q[r * a.V];
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256, vc = v < v1 ? v : v1 - 1;
#pragma unroll
            for (int r = 0; r < NR; ++r) row[it][r] = a.bias ? bb[it] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < a.S) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) row[it][r] += t[it][u][r];
                }
            if (a.S > 4) sum_slabs<NR>(a.logits_partial + r0 + vc + 4 * a.slab, a.slab, a.S - 4, off, row[it]);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = vb + it * 256;
            if (v < v1) {
                float mixed;
                if constexpr (NR == 3) {
                    const float f = row[it][0], p = row[it][1], u = row[it][2];
                    mixed = (u + w_c * (p - u)) + w_l * (f - p);
                } else {
                    const float c = row[it][0], u = row[it][1];
                    mixed = u + cfg_weight * (c - u);
                }
                if (a.logits_out) a.logits_out[((long)step * B + bg) * a.V + v] = mixed;
                if (STORE) { mix[(long)b * a.V + v] = mixed; continue; }
                if (temperature > 0.f) mixed = gumbel_perturb(mixed, invT, seed, stream, v);
                if (mixed > best) { best = mixed; bi = v; }
            }
        }
    }
    if (STORE) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        argmax_combine(best, bi, ov, oi);
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = sv[0]; int i = si[0];
        for (int k = 1; k < 4; ++k) argmax_combine(v, i, sv[k], si[k]);
        pv[b * CFG_CHUNKS + ch] = v; pi[b * CFG_CHUNKS + ch] = i;
    }
}
template <int NR>
__global__ __launch_bounds__(256) void cfg_pick_kernel(SampleArgs a, const float* __restrict__ pv, const int* __restrict__ pi) {
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    if (tid == 0) {
        float v = pv[b * CFG_CHUNKS]; int i = pi[b * CFG_CHUNKS];
        for (int k = 1; k < CFG_CHUNKS; ++k) argmax_combine(v, i, pv[b * CFG_CHUNKS + k], pi[b * CFG_CHUNKS + k]);
        i = i < 0 ? 0 : (i >= a.V ? a.V - 1 : i);
        int emit = i, feed = i;
        const long bg = b + a.b_off;
        const int T = a.p->T;
        if (step < T && a.p->has_force) {
            const int f = a.force_tok[bg * T + step];
            if (a.p->has_mask) { if (a.force_mask[bg * T + step] == 0) { emit = f; feed = f; } }
            else feed = f;
        }
        if (step < T) a.out_tok[bg * T + step] = emit;
        feed = feed < 0 ? 0 : (feed >= a.V ? a.V - 1 : feed);
        s_tok = feed;
    }
    __syncthreads();
    const float* src = a.embed_table + (long)s_tok * a.H;
    float* x0 = a.x + (long)(NR * b) * a.H;
    for (int i = tid * 4; i < a.H; i += 1024) {
        const f32x4 v = *(const f32x4*)(src + i);
#pragma unroll
        for (int r = 0; r < NR; ++r) *(f32x4*)(x0 + r * a.H + i) = v;
    }
}
__global__ void set_sample_params_kernel(SampleParams* dst, SampleParams v) { *dst = v; }
void launch_set_sample_params(hipStream_t s, SampleParams* dst, SampleParams v) { hipLaunchKernelGGL(set_sample_params_kernel, dim3(1), dim3(1), 0, s, dst, v); }
__global__ void set_text_params_kernel(TextParams* dst, TextParams v) { *dst = v; }
void launch_set_text_params(hipStream_t s, TextParams* dst, TextParams v) { hipLaunchKernelGGL(set_text_params_kernel, dim3(1), dim3(1), 0, s, dst, v); }

// ------------------------------------------------------------------------------- top-k / top-p sampler
// One 1024-thread block per image over its row x = mixed * invT (kept in LDS as the raw mixed values).
// Keys: order-preserving fp32 -> uint32 (NaN -> -inf, -0 -> +0).  top-k threshold tk = the k-th largest key, by an
// MSB-first radix select (8-bit digits, LDS count histograms, wave-0 prefix over the 256 buckets).  top-p threshold
// tp = the smallest key whose strictly-larger survivors (key >= tk) hold < top_p of their exp-mass: the same radix walk
// over mass histograms.  Masses are w = exp(x - max) in 2^-40 fixed point (64-bit integer sums: the result does not depend
// on the order of the LDS atomics).  Kept: key >= max(tk, tp) and x > -inf.  Then the Gumbel-max of cfg_scan_kernel
// over the kept set (same noise, same tie rule) -> slot 0 of the stage-1 winners cfg_pick_kernel combines.
// text_select_kernel (below) applies the same rule to rows that do not fit in LDS: both kernels get their threshold from
// sel_thresholds and their token from sel_draw.
__device__ __forceinline__ uint32_t sel_key(float mixed, float invT) {
    float x = mixed * invT;
    if (x != x) x = -INFINITY;
    if (x == 0.f) x = 0.f;
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
#define SEL_THREADS 1024
#define SEL_KEY_NEGINF 0x007fffffu                   // sel_key(-inf)
#define SEL_MASS_ONE 1099511627776.f                 // 2^40
__device__ __forceinline__ unsigned long long sel_mass(uint32_t key, float m) {
    const float x = sel_unkey(key);
    const float w = m == INFINITY ? (x == INFINITY ? 1.f : 0.f) : expf(x - m);
    return (unsigned long long)(w * SEL_MASS_ONE);
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
struct SelWalkShm {
    uint32_t hist[256]; unsigned long long mhist[256];
    uint32_t digit, rem; unsigned long long z, above;
};
// f(v, value) over a row with 16-byte loads when the row allows it (V % 4 == 0 and a 16-byte aligned base)
template <class F>
__device__ __forceinline__ void sel_row_each(const float* __restrict__ row, int V, int tid, F f) {
    if (((V & 3) | (int)((uintptr_t)row & 15)) == 0) {
        for (int v = tid * 4; v < V; v += SEL_THREADS * 4) {
            const f32x4 c = *(const f32x4*)(row + v);
            f(v, c[0]); f(v + 1, c[1]); f(v + 2, c[2]); f(v + 3, c[3]);
        }
    } else {
        for (int v = tid; v < V; v += SEL_THREADS) f(v, row[v]);
    }
}
struct SelSrcRow {          // the whole row in global memory
    const float* row; int V;
    template <class F> __device__ __forceinline__ void each(int tid, F f) const { sel_row_each(row, V, tid, [&](int, float x) { f(x); }); }
};
struct SelSrcLds {          // the compacted candidates
    const float* p; int n;
    template <class F> __device__ __forceinline__ void each(int tid, F f) const { for (int i = tid; i < n; i += SEL_THREADS) f(p[i]); }
};
// tau = max(top-k threshold, top-p threshold, the key above -inf) over the entries of src: the two radix walks of the header.  kmx: the
// largest key; rem_k: rank of the top-k threshold (0: top-k off); have_z: Z is z_in (top-k off: the caller knows the row's whole mass),
// else it is summed over the top-k survivors into w.z, which the caller has zeroed in front of a barrier.  Called by every thread of
// the block; w is not written after the last barrier inside, so the caller needs none behind it.
template <class Src>
__device__ __forceinline__ uint32_t sel_thresholds(const Src src, SelWalkShm& w, float invT, uint32_t rem_k, float top_p, uint32_t kmx, bool have_z,
                                    unsigned long long z_in) {
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t tk = 0;
    if (rem_k > 0) {
        uint32_t prefix = 0, pmask = 0, rem = rem_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) w.hist[tid] = 0;
            __syncthreads();
            src.each(tid, [&](float x) {
                const uint32_t k = sel_key(x, invT);
                if ((k & pmask) == prefix) atomicAdd(&w.hist[(k >> shift) & 255u], 1u);
            });
            __syncthreads();
            if (tid < 64) {          // lane l holds digits 255-4l .. 252-4l (descending): bucket of the rem-th largest
                uint32_t h[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = w.hist[255 - 4 * lane - j]; sum += h[j]; }
                uint32_t incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                uint32_t before = incl - sum;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (before < rem && before + h[j] >= rem) { w.digit = 255 - 4 * lane - j; w.rem = rem - before; }
                    before += h[j];
                }
            }
            __syncthreads();
            prefix |= w.digit << shift; pmask |= 255u << shift; rem = w.rem;
        }
        tk = prefix;
    }
    uint32_t tp = 0;
    if (top_p < 1.f && kmx > SEL_KEY_NEGINF) {
        const float m = sel_unkey(kmx);
        if (!have_z) {
            unsigned long long z = 0;
            src.each(tid, [&](float x) {
                const uint32_t k = sel_key(x, invT);
                if (k >= tk) z += sel_mass(k, m);
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) z += shfl_xor_u64(z, o);
            if (lane == 0) atomicAdd(&w.z, z);
            __syncthreads();
        }
        const double limit = (double)top_p * (double)(have_z ? z_in : w.z);
        uint32_t prefix = 0, pmask = 0;
        unsigned long long above = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) { w.hist[tid] = 0; w.mhist[tid] = 0; }
            __syncthreads();
            src.each(tid, [&](float x) {
                const uint32_t k = sel_key(x, invT);
                if (k >= tk && (k & pmask) == prefix) {
                    const uint32_t d = (k >> shift) & 255u;
                    atomicAdd(&w.hist[d], 1u);
                    const unsigned long long q = sel_mass(k, m);
                    if (q) atomicAdd(&w.mhist[d], q);
                }
            });
            __syncthreads();
            if (tid < 64) {          // lowest non-empty bucket whose strictly-larger mass is < limit
                uint32_t c[4]; unsigned long long mm[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = w.hist[255 - 4 * lane - j]; mm[j] = w.mhist[255 - 4 * lane - j]; sum += mm[j]; }
                unsigned long long incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = shfl_up_u64(incl, o); if (lane >= o) incl += t; }
                unsigned long long cum = above + incl - sum;
                int dj = -1; unsigned long long cj = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (c[j] && (double)cum < limit) { dj = 255 - 4 * lane - j; cj = cum; }
                    cum += mm[j];
                }
                const unsigned long long has = __ballot(dj >= 0);
                if (dj >= 0 && lane == 63 - __clzll(has)) { w.digit = (uint32_t)dj; w.above = cj; }
            }
            __syncthreads();
            prefix |= w.digit << shift; pmask |= 255u << shift; above = w.above;
        }
        tp = prefix;
    }
    uint32_t tau = tk > tp ? tk : tp;
    return tau > SEL_KEY_NEGINF + 1 ? tau : SEL_KEY_NEGINF + 1;
}
// The draw over the kept set.  each(g) calls g(v, value) for this thread's entries of the row; kept = key >= tau goes to keep[v] (keep: the
// row's mask or null).  draw: Gumbel-max of cfg_scan_kernel over the kept entries (greedy: the kept values themselves, a planned greedy
// image), lowest index on ties, reduced over the block; thread 0 returns the winner in (best, bi) -- (-inf, 0x7fffffff) when nothing
// was kept.  Without draw nothing is reduced (no barrier).
template <class Each>
__device__ __forceinline__ void sel_draw(Each each, uint32_t tau, float invT, uint64_t seed, uint64_t stream, uint8_t* keep, bool draw, bool greedy,
                                         float& best, int& bi) {
    __shared__ float wv[SEL_THREADS / 64]; __shared__ int wi[SEL_THREADS / 64];
    const int tid = threadIdx.x;
    best = -INFINITY; bi = 0x7fffffff;
    each([&](int v, float x) {
        const bool kept = sel_key(x, invT) >= tau;
        if (keep) keep[v] = kept;
        if (draw && kept) {
            const float g = greedy ? x : gumbel_perturb(x, invT, seed, stream, v);
            if (g > best) { best = g; bi = v; }
        }
    });
    if (!draw) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        argmax_combine(best, bi, ov, oi);
    }
    if ((tid & 63) == 0) { wv[tid >> 6] = best; wi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        best = wv[0]; bi = wi[0];
        for (int k = 1; k < SEL_THREADS / 64; ++k) argmax_combine(best, bi, wv[k], wi[k]);
    }
}
// PLAN: image b + b_off takes its temperature, (top_k, top_p) and key from the plan.  A greedy image (temperature <= 0) ignores its filter and is the
// plain first-index argmax of the row, an image with (0, 1) keeps everything: both leave the winner the unfiltered scan would leave (nothing to
// choose from -> the out-of-range index that cfg_pick_kernel clamps, not the filtered form's token 0).
template <bool PLAN>
__global__ __launch_bounds__(SEL_THREADS) void cfg_select_kernel(typename std::conditional<PLAN, FilterArgsPlan, FilterArgs>::type f) {
    __shared__ float vals[SEL_MAXV];
    __shared__ __attribute__((aligned(16))) SelWalkShm w;          // 16-byte aligned: the walks read four buckets with one LDS load
    __shared__ uint32_t s_max;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, V = f.V;
    float temperature; int top_k; float top_p;
    if constexpr (PLAN) {
        const int bg = b + f.b_off;
        temperature = f.plan.temperature[bg];
        const bool greedy = !(temperature > 0.f);
        top_k = greedy ? 0 : f.plan.top_k[bg]; top_p = greedy ? 1.f : f.plan.top_p[bg];
    } else {
        temperature = f.p ? f.p->temperature : f.temperature;
        top_k = f.p ? f.p->top_k : f.top_k;
        top_p = f.p ? f.p->top_p : f.top_p;
    }
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const float* row = f.mix + (long)b * V;
    if (tid == 0) { s_max = 0; w.z = 0; }
    uint32_t kmax = 0;
    for (int v = tid; v < V; v += SEL_THREADS) {
        const float m = row[v];
        vals[v] = m;
        const uint32_t k = sel_key(m, invT);
        kmax = k > kmax ? k : kmax;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(kmax, o, 64); kmax = t > kmax ? t : kmax; }
    __syncthreads();
    if (lane == 0) atomicMax(&s_max, kmax);
    __syncthreads();
    // Z is summed over the top-k survivors (have_z = false)
    const bool k_on = top_k > 0 && top_k < V;
    const uint32_t tau = sel_thresholds(SelSrcLds{vals, V}, w, invT, k_on ? (uint32_t)top_k : 0u, top_p, s_max, false, 0ull);
    // ---- kept mask (operator) / Gumbel-max over the kept set (sampler)
    uint64_t seed = 0, stream = 0;
    if (f.pv) {
        const int step = *f.n_dec;
        seed = f.p->seed;
        if constexpr (PLAN) stream = (uint64_t)f.plan.key[b + f.b_off] * 1000003ull + step;
        else stream = (uint64_t)(b + f.b_off + f.p->img_off) * 1000003ull + step;
    }
    float best; int bi;
    sel_draw([&](auto g) { for (int v = tid; v < V; v += SEL_THREADS) g(v, vals[v]); }, tau, invT, seed, stream,
             f.keep ? f.keep + (long)b * V : nullptr, f.pv != nullptr, PLAN && !(temperature > 0.f), best, bi);
    if (!f.pv) return;
    if (tid < CFG_CHUNKS) {
        float v = -INFINITY; int i = 0x7fffffff;
        if (tid == 0) {
            v = best; i = bi;
            if (i == 0x7fffffff && !(PLAN && top_k <= 0 && !(top_p < 1.f))) i = 0;          // nothing kept (every entry -inf / NaN): token 0
        }
        f.pv[b * CFG_CHUNKS + tid] = v; f.pi[b * CFG_CHUNKS + tid] = i;
    }
}
// One step of the image sampler.  filtered: store scan -> select (it reads mix and leaves the winner in slot 0) -> pick, never a second scan.
// Otherwise [stored: store scan ->] scan -> pick.  The store scan writes no winner slots.
template <int NR, bool PLAN, class A>
static void cfg_step(hipStream_t s, const A& a, int B, bool filtered, bool stored, float* scratch_v, int* scratch_i, float* mix) {
    const dim3 grid(CFG_CHUNKS, B);
    if (filtered || stored) hipLaunchKernelGGL((cfg_scan_kernel<NR, true, PLAN>), grid, dim3(256), 0, s, a, (float*)nullptr, (int*)nullptr, mix);
    if (filtered) {
        typename std::conditional<PLAN, FilterArgsPlan, FilterArgs>::type f{};
        f.mix = mix; f.V = a.V; f.p = a.p; f.pv = scratch_v; f.pi = scratch_i; f.n_dec = a.n_dec; f.b_off = a.b_off;
        if constexpr (PLAN) f.plan = a.plan;
        hipLaunchKernelGGL(cfg_select_kernel<PLAN>, dim3(B), dim3(SEL_THREADS), 0, s, f);
    } else hipLaunchKernelGGL((cfg_scan_kernel<NR, false, PLAN>), grid, dim3(256), 0, s, a, scratch_v, scratch_i, (float*)nullptr);
    hipLaunchKernelGGL(cfg_pick_kernel<NR>, dim3(B), dim3(256), 0, s, static_cast<const SampleArgs&>(a), scratch_v, scratch_i);
}
void launch_cfg_step(hipStream_t s, const SampleArgs& a, const SamplePlanDev* plan, const DualWeights* dw, int rows_per_image, int B, bool filtered,
                     bool stored, float* scratch_v, int* scratch_i, float* mix) {
    if (rows_per_image == 3) { SampleArgsDual d{}; static_cast<SampleArgs&>(d) = a; d.dw = dw; cfg_step<3, false>(s, d, B, filtered, stored, scratch_v, scratch_i, mix); }
    else if (plan) { SampleArgsPlan p{}; static_cast<SampleArgs&>(p) = a; p.plan = *plan; cfg_step<2, true>(s, p, B, filtered, stored, scratch_v, scratch_i, mix); }
    else cfg_step<2, false>(s, a, B, filtered, stored, scratch_v, scratch_i, mix);
}
// the arrays a plan left out <- the call's scalars (key: global image index + img_off); one thread per (image, step)
__global__ __launch_bounds__(256) void plan_fill_kernel(SamplePlanDev d, int mask, int B, int T, float cfg_weight, float temperature, int top_k, float top_p,
                                                        int img_off) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (!(mask & 1) && i < (long)B * T) const_cast<float*>(d.w)[i] = cfg_weight;
    if (i < B) {
        if (!(mask & 2)) const_cast<float*>(d.temperature)[i] = temperature;
        if (!(mask & 4)) const_cast<int32_t*>(d.top_k)[i] = top_k;
        if (!(mask & 8)) const_cast<float*>(d.top_p)[i] = top_p;
        if (!(mask & 16)) const_cast<int32_t*>(d.key)[i] = (int32_t)i + img_off;
    }
}
void launch_plan_fill(hipStream_t s, const SamplePlanDev& d, int mask, int B, int T, float cfg_weight, float temperature, int top_k, float top_p, int img_off) {
    const long n = (long)B * T;
    hipLaunchKernelGGL(plan_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, mask, B, T, cfg_weight, temperature, top_k, top_p, img_off);
}
void launch_sample_filter(hipStream_t s, const float* rows, int B, int V, float temperature, int top_k, float top_p, uint8_t* keep) {
    FilterArgs f{};
    f.mix = rows; f.V = V; f.temperature = temperature; f.top_k = top_k; f.top_p = top_p; f.keep = keep;
    hipLaunchKernelGGL(cfg_select_kernel<false>, dim3(B), dim3(SEL_THREADS), 0, s, f);
}

__global__ void set_dual_weights_kernel(DualWeights* dst, DualWeights v) { *dst = v; }
void launch_set_dual_weights(hipStream_t s, DualWeights* dst, DualWeights v) { hipLaunchKernelGGL(set_dual_weights_kernel, dim3(1), dim3(1), 0, s, dst, v); }

// text token (HF generate): greedy = argmax over vocab; sampled = Gumbel-max over logits / T (== multinomial(softmax(logits / T)));
// finished rows emit eos, unfinished &= (tok != eos).  Two stages like the image sampler: grid (CFG_CHUNKS, B) scans V/CFG_CHUNKS logits with
// 16-byte loads (split-K slabs summed in slab order), one block per row combines the winners (lowest index on ties =
// torch.argmax), does the EOS bookkeeping and gathers the next embedding.  (One block per row over 102 400 logits with
// scalar loads was 160 us per step at 64 rows; this pair is ~10.)
// MODE: TEXT_GREEDY (the argmax, as before), TEXT_SAMPLE (every logit perturbed by gumbel_perturb with p->temperature / seed / row_off: no extra
// pass), TEXT_STORE (filtered sampler: the reduced row, EOS suppression applied, goes to mix [B, V]; the winners are the chunk MAXIMA of the
// unperturbed row, which text_select_kernel reads as the softmax shift).  TAP: also write the row to logits_out [max_new, B, V].
// DFA (pg_generate_text_constrained; rule: kernels.h TextDfaArgs): the block first folds its row's state into one "allowed" bit per token
// class -- 1024 bits = 32 LDS dwords, one per bank, so the lookups of a wave never conflict whatever classes its tokens have (a byte or
// int16 per class spreads 1024 classes over 8-16 dwords per bank) -- and each 16-byte logit load gets one 8-byte load of the four tokens'
// classes issued beside it (token_class: 200 KiB shared by every row, L2 resident).  A disallowed entry becomes -inf where the EOS ban is
// applied, so the tap, the TEXT_STORE row and text_select_kernel carry it without a change.
enum { TEXT_GREEDY = 0, TEXT_SAMPLE = 1, TEXT_STORE = 2 };
// One body, two kernels (text_scan_body.h is included in each): text_scan_kernel is the kernel it was, text_scan_dfa_kernel takes the
// automaton as well.  A shared __device__ function would do, but it changes the unconstrained kernels' register allocation; this way
// their instruction streams are unchanged (compared with llvm-objdump against the build before the DFA parameter existed).
template <int MODE, bool TAP>
__global__ __launch_bounds__(256) void text_scan_kernel(TextArgs a, float* __restrict__ pv, int* __restrict__ pi, float* __restrict__ mix) {
    constexpr bool DFA = MODE < 0;                      // always false; dependent, so `if constexpr (DFA)` discards its branch
    [[maybe_unused]] const TextDfaArgs* d = nullptr;
#include "text_scan_body.h"
}
template <int MODE, bool TAP>
__global__ __launch_bounds__(256) void text_scan_dfa_kernel(TextArgs a, float* __restrict__ pv, int* __restrict__ pi, float* __restrict__ mix, TextDfaArgs dfa) {
    constexpr bool DFA = MODE >= 0;                     // always true
    const TextDfaArgs* d = &dfa;
#include "text_scan_body.h"
}
__global__ __launch_bounds__(256) void text_argmax_kernel(TextArgs a, const float* __restrict__ pv, const int* __restrict__ pi) {
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    if (tid == 0) {
        const int eos = a.p->eos, max_new = a.p->max_new;
        float v = pv[b * CFG_CHUNKS]; int i = pi[b * CFG_CHUNKS];
        for (int k = 1; k < CFG_CHUNKS; ++k) argmax_combine(v, i, pv[b * CFG_CHUNKS + k], pi[b * CFG_CHUNKS + k]);
        if (i == 0x7fffffff) i = 0;                                   // every logit -inf / NaN: index 0 (torch.argmax)
        const int unf = a.unfinished[b];
        const int tok = unf ? i : eos;
        if (step < max_new) a.out[(long)b * max_new + step] = tok;
        const int still = unf && (tok != eos);
        a.unfinished[b] = still;
        if (still) atomicOr(a.any_unfinished + ((step + 1) & 1023), 1);
        s_tok = tok < 0 ? 0 : (tok >= a.V ? a.V - 1 : tok);
    }
    __syncthreads();
    const float* src = a.embed_table + (long)s_tok * a.H;
    float* x0 = a.x + (long)b * a.H;
    for (int i = tid * 4; i < a.H; i += 1024) *(f32x4*)(x0 + i) = *(const f32x4*)(src + i);
}
// The constrained pick: text_argmax_kernel with two differences.  Nothing kept (every allowed logit -inf / NaN) emits eos and finishes the
// row -- token 0 could lie outside the language -- and an unfinished row's state moves along its token (it stays where it is when nothing
// was kept, and for finished rows).  d.tok != null is the operator form: token and next state out, no loop bookkeeping, no embedding.
__global__ __launch_bounds__(256) void text_pick_dfa_kernel(TextArgs a, TextDfaArgs d, const float* __restrict__ pv, const int* __restrict__ pi) {
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, step = *a.n_dec;
    if (tid == 0) {
        const int eos = a.p->eos, max_new = a.p->max_new;
        float v = pv[b * CFG_CHUNKS]; int i = pi[b * CFG_CHUNKS];
        for (int k = 1; k < CFG_CHUNKS; ++k) argmax_combine(v, i, pv[b * CFG_CHUNKS + k], pi[b * CFG_CHUNKS + k]);
        const bool none = i == 0x7fffffff || i < 0 || i >= a.V;
        const int unf = d.tok ? 1 : a.unfinished[b];
        const int tok = (unf && !none) ? i : eos;
        const int st = d.state[b], ncl = d.hdr->n_classes;
        int ns = st;
        if (unf && !none && st >= 0 && st < d.hdr->n_states) {
            const int nx = d.next_state[(long)st * ncl + ((uint16_t)d.token_class[i] & (TEXT_DFA_MAX_CLASSES - 1))];
            if (nx >= 0) ns = nx;
        }
        d.state_out[b] = ns;
        if (d.tok) { d.tok[b] = tok; s_tok = -1; }
        else {
            if (step < max_new) a.out[(long)b * max_new + step] = tok;
            const int still = unf && (tok != eos);
            a.unfinished[b] = still;
            if (still) atomicOr(a.any_unfinished + ((step + 1) & 1023), 1);
            s_tok = tok < 0 ? 0 : (tok >= a.V ? a.V - 1 : tok);
        }
    }
    __syncthreads();
    if (s_tok < 0) return;
    const float* src = a.embed_table + (long)s_tok * a.H;
    float* x0 = a.x + (long)b * a.H;
    for (int i = tid * 4; i < a.H; i += 1024) *(f32x4*)(x0 + i) = *(const f32x4*)(src + i);
}
__global__ void text_dfa_reset_kernel(int32_t* __restrict__ state, const TextDfaHdr* __restrict__ hdr, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) state[b] = hdr->start_state;
}
void launch_text_dfa_reset(hipStream_t s, int32_t* state, const TextDfaHdr* hdr, int B) {
    hipLaunchKernelGGL(text_dfa_reset_kernel, dim3((B + 255) / 256), dim3(256), 0, s, state, hdr, B);
}
__global__ void set_text_op_params_kernel(TextParams* dst, TextParams v, int32_t* step_dst, int step) { *dst = v; *step_dst = step; }
void launch_set_text_op_params(hipStream_t s, TextParams* dst, TextParams v, int32_t* step_dst, int step) {
    hipLaunchKernelGGL(set_text_op_params_kernel, dim3(1), dim3(1), 0, s, dst, v, step_dst, step);
}
template <int MODE>
static void launch_text_scan(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i, float* mix) {
    if (a.logits_out) hipLaunchKernelGGL((text_scan_kernel<MODE, true>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix);
    else hipLaunchKernelGGL((text_scan_kernel<MODE, false>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix);
}
template <int MODE>
static void launch_text_scan_dfa(hipStream_t s, const TextArgs& a, const TextDfaArgs& d, int B, float* scratch_v, int* scratch_i, float* mix) {
    if (a.logits_out) hipLaunchKernelGGL((text_scan_dfa_kernel<MODE, true>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix, d);
    else hipLaunchKernelGGL((text_scan_dfa_kernel<MODE, false>), dim3(CFG_CHUNKS, B), dim3(256), 0, s, a, scratch_v, scratch_i, mix, d);
}
void launch_text_argmax(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i) {
    launch_text_scan<TEXT_GREEDY>(s, a, B, scratch_v, scratch_i, nullptr);
    hipLaunchKernelGGL(text_argmax_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}
void launch_text_sample(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i) {
    launch_text_scan<TEXT_SAMPLE>(s, a, B, scratch_v, scratch_i, nullptr);
    hipLaunchKernelGGL(text_argmax_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}

// ------------------------------------------------------------------------------- top-k / top-p text sampler
// The rule of cfg_select_kernel (its sel_thresholds over the same keys and 2^-40 fixed-point masses, its sel_draw) for rows that do not fit in LDS
// (vocab 102 400 = 400 KiB): one 1024-thread block per row over the fp32 row in global memory (written by the scan just before: L2 resident).
//   1. m = row maximum (from the scan's chunk maxima, or one pass), the softmax shift.
//   2. one pass: histogram of the 12 leading key bits (sign, exponent, 3 mantissa bits): counts, and exp-masses when top-p acts alone.
//   3. floor bucket = the bucket that holds the k-th largest entry (top_k on: the top-p threshold lies at or above it too), else the
//      bucket that holds the top-p threshold (exact from the bucket masses: no top-k, so Z is the whole row's mass).
//   4. entries at or above the floor are compacted into LDS (<= TSEL_CAND of them: 50 for top_k = 50, ~14 000 for top_p = 0.9 on a
//      Gaussian row) and sel_thresholds -- the 8-bit radix walks -- runs over them.  More candidates than fit
//      (top_p just below 1 on a flat row): the same walks run over the row in global memory instead.  Both give the same thresholds,
//      which depend on the multiset of values only (compaction order does not matter; all mass sums are 64-bit integers).
//   5. one pass (sel_draw): kept = key >= tau; kept mask (operator) and Gumbel-max over the kept set -> slot 0 of the winners text_argmax_kernel combines.
#define TSEL_BITS 12
#define TSEL_BUCKETS (1 << TSEL_BITS)
#define TSEL_CAND 16384
__global__ __launch_bounds__(SEL_THREADS) void text_select_kernel(TextSelectArgs f) {
    // phase 2-3: cnt[TSEL_BUCKETS] u32 | mass[TSEL_BUCKETS] u64 (48 KiB); phase 4: cand[TSEL_CAND] fp32 (64 KiB)
    __shared__ __attribute__((aligned(16))) unsigned char buf[TSEL_CAND * 4];
    __shared__ __attribute__((aligned(16))) SelWalkShm w;          // 16-byte aligned: the walks read four buckets with one LDS load
    __shared__ uint32_t s_max, s_floor, s_nc, s_fill;
    __shared__ uint32_t wcnt[SEL_THREADS / 64]; __shared__ unsigned long long wmass[SEL_THREADS / 64];
    uint32_t* cnt = (uint32_t*)buf;
    unsigned long long* mass = (unsigned long long*)(buf + TSEL_BUCKETS * 4);
    float* cand = (float*)buf;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = f.V;
    const float temperature = f.p ? f.p->temperature : f.temperature;
    const int top_k = f.p ? f.p->top_k : f.top_k;
    const float top_p = f.p ? f.p->top_p : f.top_p;
    const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
    const float* row = f.rows + (long)b * V;
    // ---- 1. the row maximum
    if (tid == 0) { s_max = 0; s_floor = TSEL_BUCKETS; s_nc = 0; s_fill = 0; w.z = 0; }
    __syncthreads();
    if (f.chunk_max) {
        if (tid < CFG_CHUNKS) atomicMax(&s_max, sel_key(f.chunk_max[b * CFG_CHUNKS + tid], invT));
    } else {
        uint32_t kmax = 0;
        sel_row_each(row, V, tid, [&](int, float x) { const uint32_t k = sel_key(x, invT); kmax = k > kmax ? k : kmax; });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(kmax, o, 64); kmax = t > kmax ? t : kmax; }
        if (lane == 0) atomicMax(&s_max, kmax);
    }
    __syncthreads();
    const uint32_t kmx = s_max;
    const bool k_on = top_k > 0 && top_k < V;
    const bool p_on = top_p < 1.f && kmx > SEL_KEY_NEGINF;
    uint32_t tau = SEL_KEY_NEGINF + 1;
    if (k_on || p_on) {
        // ---- 2. first-digit histogram
        const bool need_mass = !k_on;
        const float m = sel_unkey(kmx);
        for (int i = tid; i < TSEL_BUCKETS; i += SEL_THREADS) { cnt[i] = 0; mass[i] = 0; }
        __syncthreads();
        sel_row_each(row, V, tid, [&](int, float x) {
            const uint32_t k = sel_key(x, invT), d = k >> (32 - TSEL_BITS);
            atomicAdd(&cnt[d], 1u);
            if (need_mass) { const unsigned long long q = sel_mass(k, m); if (q) atomicAdd(&mass[d], q); }
        });
        __syncthreads();
        // ---- 3. the floor bucket: thread t holds buckets top-4t .. top-4t-3 (descending); block-wide exclusive prefix from the top
        constexpr int top = TSEL_BUCKETS - 1;
        uint32_t h[4], hs = 0; unsigned long long mm[4], ms = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { h[j] = cnt[top - 4 * tid - j]; mm[j] = mass[top - 4 * tid - j]; hs += h[j]; ms += mm[j]; }
        uint32_t hin = hs; unsigned long long min_ = ms;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(hin, o, 64); const unsigned long long u = shfl_up_u64(min_, o);
            if (lane >= o) { hin += t; min_ += u; }
        }
        if (lane == 63) { wcnt[wave] = hin; wmass[wave] = min_; }
        __syncthreads();
        uint32_t before = hin - hs; unsigned long long cum = min_ - ms, ztot = 0;
        for (int i = 0; i < SEL_THREADS / 64; ++i) {
            if (i < wave) { before += wcnt[i]; cum += wmass[i]; }
            ztot += wmass[i];
        }
        if (k_on) {
            uint32_t bf = before;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (bf < (uint32_t)top_k && bf + h[j] >= (uint32_t)top_k) { s_floor = top - 4 * tid - j; s_nc = bf + h[j]; }
                bf += h[j];
            }
        } else {
            const double limit = (double)top_p * (double)ztot;
            int dj = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (h[j] && (double)cum < limit) dj = top - 4 * tid - j;
                cum += mm[j];
            }
            if (dj >= 0) atomicMin(&s_floor, (uint32_t)dj);
        }
        __syncthreads();
        const uint32_t floor_d = s_floor;
        if (!k_on) {          // candidates at or above the floor: the inclusive count at that bucket
            uint32_t bf = before;
#pragma unroll
            for (int j = 0; j < 4; ++j) { bf += h[j]; if ((uint32_t)(top - 4 * tid - j) == floor_d) s_nc = bf; }
        }
        __syncthreads();
        const uint32_t nc = s_nc;
        if (nc <= TSEL_CAND) {
            // ---- 4. compact (one LDS atomic per wave and element slot), then the walks over LDS
            sel_row_each(row, V, tid, [&](int, float x) {
                const bool in = (sel_key(x, invT) >> (32 - TSEL_BITS)) >= floor_d;
                const unsigned long long bal = __ballot(in);
                if (bal) {
                    uint32_t base = 0;
                    const int leader = __ffsll((long long)bal) - 1;
                    if (lane == leader) base = atomicAdd(&s_fill, (uint32_t)__popcll(bal));
                    base = __shfl(base, leader, 64);
                    if (in) cand[base + __popcll(bal & ((1ull << lane) - 1ull))] = x;
                }
            });
            __syncthreads();
            tau = sel_thresholds(SelSrcLds{cand, (int)nc}, w, invT, k_on ? (uint32_t)top_k : 0u, top_p, kmx, !k_on, ztot);
        } else {
            tau = sel_thresholds(SelSrcRow{row, V}, w, invT, k_on ? (uint32_t)top_k : 0u, top_p, kmx, false, 0ull);
        }
    }
    // ---- 5. kept mask (operator) / Gumbel-max over the kept set
    const bool draw = f.pv || f.tok;
    uint64_t seed = 0, stream = 0;
    if (draw) {
        const int step = f.n_dec ? *f.n_dec : f.step;
        seed = f.p ? f.p->seed : f.seed;
        stream = (uint64_t)(b + (f.p ? f.p->row_off : f.row_off)) * 1000003ull + step;
    }
    float best; int bi;
    sel_draw([&](auto g) { sel_row_each(row, V, tid, g); }, tau, invT, seed, stream, f.keep ? f.keep + (long)b * V : nullptr, draw, false, best, bi);
    if (!draw) return;
    if (tid < CFG_CHUNKS) {
        float v = -INFINITY; int i = 0x7fffffff;
        if (tid == 0) {
            v = best; i = bi;
            if (f.tok) f.tok[b] = i == 0x7fffffff ? 0 : i;          // nothing kept (every entry -inf / NaN): token 0
        }
        if (f.pv) { f.pv[b * CFG_CHUNKS + tid] = v; f.pi[b * CFG_CHUNKS + tid] = i; }
    }
}
void launch_text_select(hipStream_t s, const TextSelectArgs& f, int B) {
    hipLaunchKernelGGL(text_select_kernel, dim3(B), dim3(SEL_THREADS), 0, s, f);
}
void launch_text_sample_filtered(hipStream_t s, const TextArgs& a, int B, float* scratch_v, int* scratch_i, float* mix) {
    launch_text_scan<TEXT_STORE>(s, a, B, scratch_v, scratch_i, mix);
    TextSelectArgs f{};
    f.rows = mix; f.V = a.V; f.chunk_max = scratch_v; f.p = a.p; f.n_dec = a.n_dec; f.pv = scratch_v; f.pi = scratch_i;
    launch_text_select(s, f, B);
    hipLaunchKernelGGL(text_argmax_kernel, dim3(B), dim3(256), 0, s, a, scratch_v, scratch_i);
}
void launch_text_constrained(hipStream_t s, const TextArgs& a, const TextDfaArgs& d, int B, int mode, float* scratch_v, int* scratch_i, float* mix) {
    if (mode == 2) {
        launch_text_scan_dfa<TEXT_STORE>(s, a, d, B, scratch_v, scratch_i, mix);
        TextSelectArgs f{};
        f.rows = mix; f.V = a.V; f.chunk_max = scratch_v; f.p = a.p; f.n_dec = a.n_dec; f.pv = scratch_v; f.pi = scratch_i; f.keep = d.keep;
        launch_text_select(s, f, B);
    } else if (mode == 1) launch_text_scan_dfa<TEXT_SAMPLE>(s, a, d, B, scratch_v, scratch_i, mix);
    else launch_text_scan_dfa<TEXT_GREEDY>(s, a, d, B, scratch_v, scratch_i, mix);
    hipLaunchKernelGGL(text_pick_dfa_kernel, dim3(B), dim3(256), 0, s, a, d, scratch_v, scratch_i);
}

// ------------------------------------------------------------------------------- token log-probabilities
// logprob = x[tok] - logsumexp(x) of one stored row per block (stored_row.h LogprobArgs; the definition is in include/plangen_hip.h).
// Two passes over the row in the order of StoredRow::each: the maximum, then sum expf(x - max) -- one accurate expf per entry, nothing
// rescaled.  A thread adds at most V / 1024 terms, then a butterfly over the wave and a serial sum of the 16 wave sums: a fixed shape,
// so the bits do not depend on how the block was scheduled.  x == max contributes exactly 1 (this is expf(0), and it keeps a row whose
// maximum is +inf meaningful: the mass sits evenly on the +inf entries).
template <int FORM>
__global__ __launch_bounds__(SR_THREADS) void token_logprob_kernel(typename SrArgsOf<FORM, LogprobArgs, LogprobArgsPlan>::type a) {
    __shared__ float red[SR_WAVES];
    __shared__ float s_m;
    const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
    int tok; float temperature; long at;
    const int where = sr_locate<FORM>(a, b, tok, temperature, at);
    if (where == SR_FINISHED && tid == 0) a.out[at] = 0.f;
    if (where != SR_LIVE) return;
    const StoredRow sr(a.rows + (long)b * V, V, temperature);
    auto block_reduce = [&](float v, bool is_max) -> float {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const float ov = __shfl_xor(v, o, 64); v = is_max ? fmaxf(v, ov) : v + ov; }
        __syncthreads();                                   // red / s_m of the previous reduction have been read
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) {
            float t = red[0];
            for (int k = 1; k < SR_WAVES; ++k) t = is_max ? fmaxf(t, red[k]) : t + red[k];
            s_m = t;
        }
        __syncthreads();
        return s_m;
    };
    float m = -INFINITY;
    sr.template each<true>(tid, [&](float y, int, bool) { m = fmaxf(m, sr.xval(y)); });
    m = block_reduce(m, true);
    float sum = 0.f;
    sr.template each<false>(tid, [&](float y, int, bool) { const float x = sr.xval(y); sum += x == m ? 1.f : expf(x - m); });
    sum = block_reduce(sum, false);
    if (tid == 0) {
        const float xt = (tok >= 0 && tok < V) ? sr.xval(sr.row[tok]) : -INFINITY;
        float lp = -INFINITY;                              // no finite entry, or the token's own entry is -inf
        if (m > -INFINITY && xt > -INFINITY) lp = (xt == m ? 0.f : xt - m) - logf(sum);
        a.out[at] = lp;
    }
}
void launch_token_logprob_op(hipStream_t s, const float* rows, int B, int V, const int32_t* tok, float temperature, float* out) {
    LogprobArgs l{};
    l.rows = rows; l.V = V; l.temperature = temperature; l.tok32 = tok; l.out = out;
    hipLaunchKernelGGL(token_logprob_kernel<SR_OP>, dim3(B), dim3(SR_THREADS), 0, s, l);
}
void launch_token_logprob_image(hipStream_t s, const SampleArgs& a, int B, const float* mix, float* out) {
    LogprobArgs l{};
    l.rows = mix; l.V = a.V; l.sp = a.p; l.tok32 = a.out_tok; l.n_dec = a.n_dec; l.b_off = a.b_off; l.out = out;
    hipLaunchKernelGGL(token_logprob_kernel<SR_IMAGE>, dim3(B), dim3(SR_THREADS), 0, s, l);
}
void launch_token_logprob_image_plan(hipStream_t s, const SampleArgsPlan& a, int B, const float* mix, float* out) {
    LogprobArgsPlan l{};
    l.rows = mix; l.V = a.V; l.sp = a.p; l.tok32 = a.out_tok; l.n_dec = a.n_dec; l.b_off = a.b_off; l.out = out; l.plan_temperature = a.plan.temperature;
    hipLaunchKernelGGL(token_logprob_kernel<SR_IMAGE_PLAN>, dim3(B), dim3(SR_THREADS), 0, s, l);
}
void launch_text_store(hipStream_t s, const TextArgs& a, const TextDfaArgs* d, int B, float* scratch_v, int* scratch_i, float* mix) {
    if (d) {
        TextDfaArgs dd = *d; dd.keep = nullptr;
        launch_text_scan_dfa<TEXT_STORE>(s, a, dd, B, scratch_v, scratch_i, mix);
    } else launch_text_scan<TEXT_STORE>(s, a, B, scratch_v, scratch_i, mix);
}
void launch_token_logprob_text(hipStream_t s, const TextArgs& a, int B, const float* mix, float* out) {
    LogprobArgs l{};
    l.rows = mix; l.V = a.V; l.tp = a.p; l.tok64 = a.out; l.n_dec = a.n_dec; l.out = out;
    hipLaunchKernelGGL(token_logprob_kernel<SR_TEXT>, dim3(B), dim3(SR_THREADS), 0, s, l);
}

// test tap: the sampler's uniform / Gumbel transform of raw 64-bit RNG outputs: out[i] = u, out[n+i] = -log(-log(u))
__global__ void uniform_from_bits_kernel(const uint64_t* __restrict__ z, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float u = uniform_from_bits(z[i]);
    out[i] = u;
    out[n + i] = -__logf(-__logf(u));
}
void launch_uniform_from_bits(hipStream_t s, const uint64_t* z, float* out, int n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(uniform_from_bits_kernel, dim3((n + 255) / 256), dim3(256), 0, s, z, out, n);
}
