// Per-token uncertainty of one stored row per block (stored_row.h StatsArgs; the definition is in include/plangen_hip.h, pg_request_token_stats):
// the emitted token's log-probability, the entropy of the row's softmax, the token's rank and the N largest entries with their
// log-probabilities.  The second reducer on the stored-row route: it finds its position and reads its row through stored_row.h, as
// token_logprob_kernel (sampler.hip) does, one 1024-thread block per row.
// Pass 1: the maximum m and, when alternatives are asked for, every thread's 8 best (value desc, index asc) in a sorted register list;
//         the lists are merged per wave by 8 rounds of "butterfly for the best head, its owner pops it", the 16 wave lists go through
//         LDS and wave 0 merges them the same way.  Indices are unique, so the order is total and the result does not depend on timing.
// Pass 2: s = sum expf(x - m) with the term order of token_logprob_kernel (StoredRow::each; xor butterfly over the wave; serial sum of
//         the 16 wave sums), so logprob has that kernel's bits; t = sum expf(x - m) (x - m)
//         and the count of x_v > x_tok are reduced in the same fixed shape.  x = -inf adds 0 to s and t; x == m adds exactly 1 and 0.
// H = logf(s) - t / s.  m = +inf: only the +inf entries count (s = k, t = 0, H = logf(k)).  No finite entry: H = 0, rank = V.
#include <type_traits>
#include "kernels.h"
#include "stored_row.h"

#define TS_THREADS SR_THREADS
#define TS_WAVES SR_WAVES
#define TS_NALT 8
#define TS_NOIDX 0x7fffffff

__device__ __forceinline__ bool ts_better(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// sorted insert into a thread's list; every index is static, so the list stays in registers
__device__ __forceinline__ void ts_insert(float (&v)[TS_NALT], int (&i)[TS_NALT], float x, int idx) {
    if (!(x > -INFINITY) || !ts_better(x, idx, v[TS_NALT - 1], i[TS_NALT - 1])) return;
#pragma unroll
    for (int k = TS_NALT - 1; k >= 1; --k) {
        const bool above = ts_better(x, idx, v[k - 1], i[k - 1]);         // the new entry goes above slot k - 1: that one moves down
        const bool here = ts_better(x, idx, v[k], i[k]);
        v[k] = above ? v[k - 1] : (here ? x : v[k]);
        i[k] = above ? i[k - 1] : (here ? idx : i[k]);
    }
    if (ts_better(x, idx, v[0], i[0])) { v[0] = x; i[0] = idx; }
}

// the 8 best of the 64 lanes' sorted lists, in every lane; the lists are consumed
__device__ __forceinline__ void ts_wave_merge(float (&v)[TS_NALT], int (&i)[TS_NALT], float (&ov)[TS_NALT], int (&oi)[TS_NALT]) {
#pragma unroll
    for (int r = 0; r < TS_NALT; ++r) {
        float bv = v[0]; int bi = i[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float pv = __shfl_xor(bv, o, 64); const int pi = __shfl_xor(bi, o, 64);
            if (ts_better(pv, pi, bv, bi)) { bv = pv; bi = pi; }
        }
        ov[r] = bv; oi[r] = bi;
        if (i[0] == bi && bi != TS_NOIDX) {                               // this lane owned the winner: pop it
#pragma unroll
            for (int k = 0; k < TS_NALT - 1; ++k) { v[k] = v[k + 1]; i[k] = i[k + 1]; }
            v[TS_NALT - 1] = -INFINITY; i[TS_NALT - 1] = TS_NOIDX;
        }
    }
}

template <int FORM, bool ALT>
__global__ __launch_bounds__(TS_THREADS) void token_stats_kernel(typename SrArgsOf<FORM, StatsArgs, StatsArgsPlan>::type a) {
    __shared__ float red[TS_WAVES];
    __shared__ float red_t[TS_WAVES];
    __shared__ int red_c[TS_WAVES];
    __shared__ float s_m;
    __shared__ float s_tv[TS_WAVES][TS_NALT];
    __shared__ int s_ti[TS_WAVES][TS_NALT];
    const int b = blockIdx.x, tid = threadIdx.x, V = a.V, n_alt = a.o.n_alt;
    int tok; float temperature; long at;
    const int where = sr_locate<FORM>(a, b, tok, temperature, at);
    if (where == SR_FINISHED) {
        if (tid == 0) {
            if (a.o.logprob) a.o.logprob[at] = 0.f;
            if (a.o.entropy) a.o.entropy[at] = 0.f;
            if (a.o.rank) a.o.rank[at] = 0;
        }
        if (tid < n_alt) {
            if (a.o.alt_tok) a.o.alt_tok[at * n_alt + tid] = -1;
            if (a.o.alt_logprob) a.o.alt_logprob[at * n_alt + tid] = 0.f;
        }
    }
    if (where != SR_LIVE) return;
    const StoredRow sr(a.rows + (long)b * V, V, temperature);

    // ---- pass 1: the maximum and the 8 best
    float lv[TS_NALT]; int li[TS_NALT];
#pragma unroll
    for (int k = 0; k < TS_NALT; ++k) { lv[k] = -INFINITY; li[k] = TS_NOIDX; }
    float m = -INFINITY;
    sr.template each<true>(tid, [&](float y, int v, bool fresh) {
        const float x = sr.xval(y);
        m = fmaxf(m, x);
        if (ALT && fresh) ts_insert(lv, li, x, v);                          // a repeat must not enter the list twice
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float fv[TS_NALT]; int fi[TS_NALT];                                    // the block's 8 best: valid in wave 0 after the merge
    if (ALT) {
        ts_wave_merge(lv, li, fv, fi);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < TS_NALT; ++k) { s_tv[tid >> 6][k] = fv[k]; s_ti[tid >> 6][k] = fi[k]; }
        }
    }
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        float r = red[0];
        for (int k = 1; k < TS_WAVES; ++k) r = fmaxf(r, red[k]);
        s_m = r;
    }
    if (ALT && tid < 64) {                                                 // wave 0: lane w takes wave w's list
#pragma unroll
        for (int k = 0; k < TS_NALT; ++k) { lv[k] = tid < TS_WAVES ? s_tv[tid][k] : -INFINITY; li[k] = tid < TS_WAVES ? s_ti[tid][k] : TS_NOIDX; }
        ts_wave_merge(lv, li, fv, fi);
    }
    __syncthreads();
    m = s_m;

    // ---- pass 2: s (the term order of token_logprob_kernel), t and the rank count
    const float xt = (tok >= 0 && tok < V) ? sr.xval(sr.row[tok]) : -INFINITY;
    float sum = 0.f, tsum = 0.f; int cnt = 0;
    sr.template each<false>(tid, [&](float y, int, bool) {
        const float x = sr.xval(y);
        const float d = x - m;
        const float e = x == m ? 1.f : expf(d);
        sum += e;
        if (x != m && e > 0.f) tsum += e * d;                              // x == m: d counts as 0 (also when m is infinite); e == 0: nothing
        cnt += x > xt ? 1 : 0;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); tsum += __shfl_xor(tsum, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6] = sum; red_t[tid >> 6] = tsum; red_c[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        float s = red[0], t = red_t[0]; int c = red_c[0];
        for (int k = 1; k < TS_WAVES; ++k) { s += red[k]; t += red_t[k]; c += red_c[k]; }
        const float ls = logf(s);
        const bool any = m > -INFINITY;
        if (a.o.logprob) {
            float lp = -INFINITY;                                          // no finite entry, or the token's own entry is -inf
            if (any && xt > -INFINITY) lp = (xt == m ? 0.f : xt - m) - ls;
            a.o.logprob[at] = lp;
        }
        if (a.o.entropy) a.o.entropy[at] = any ? ls - t / s : 0.f;
        if (a.o.rank) a.o.rank[at] = xt > -INFINITY ? c : V;
        if (ALT) {
            for (int k = 0; k < n_alt; ++k) {
                const bool have = fv[k] > -INFINITY;                       // V < n_alt, or only -inf entries left: not an alternative
                if (a.o.alt_tok) a.o.alt_tok[at * n_alt + k] = have ? fi[k] : -1;
                if (a.o.alt_logprob) a.o.alt_logprob[at * n_alt + k] = have ? (fv[k] == m ? 0.f : fv[k] - m) - ls : -INFINITY;
            }
        }
    }
}

template <int FORM, class A>
static void ts_launch(hipStream_t s, int B, const A& l) {
    if (l.o.n_alt > 0) hipLaunchKernelGGL((token_stats_kernel<FORM, true>), dim3(B), dim3(TS_THREADS), 0, s, l);
    else hipLaunchKernelGGL((token_stats_kernel<FORM, false>), dim3(B), dim3(TS_THREADS), 0, s, l);
}
void launch_token_stats_op(hipStream_t s, const float* rows, int B, int V, const int32_t* tok, float temperature, const TokenStatsOut& o) {
    StatsArgs l{};
    l.rows = rows; l.V = V; l.temperature = temperature; l.tok32 = tok; l.o = o;
    ts_launch<SR_OP>(s, B, l);
}
void launch_token_stats_image(hipStream_t s, const SampleArgs& a, int B, const float* mix, const TokenStatsOut& o) {
    StatsArgs l{};
    l.rows = mix; l.V = a.V; l.sp = a.p; l.tok32 = a.out_tok; l.n_dec = a.n_dec; l.b_off = a.b_off; l.o = o;
    ts_launch<SR_IMAGE>(s, B, l);
}
void launch_token_stats_image_plan(hipStream_t s, const SampleArgsPlan& a, int B, const float* mix, const TokenStatsOut& o) {
    StatsArgsPlan l{};
    l.rows = mix; l.V = a.V; l.sp = a.p; l.tok32 = a.out_tok; l.n_dec = a.n_dec; l.b_off = a.b_off; l.o = o; l.plan_temperature = a.plan.temperature;
    ts_launch<SR_IMAGE_PLAN>(s, B, l);
}
void launch_token_stats_text(hipStream_t s, const TextArgs& a, int B, const float* mix, const TokenStatsOut& o) {
    StatsArgs l{};
    l.rows = mix; l.V = a.V; l.tp = a.p; l.tok64 = a.out; l.n_dec = a.n_dec; l.o = o;
    ts_launch<SR_TEXT>(s, B, l);
}
