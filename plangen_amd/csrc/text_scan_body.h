// Body of text_scan_kernel / text_scan_dfa_kernel (sampler.hip): included once in each, NOT a header to include elsewhere.
// In scope: TextArgs a; pv, pi, mix; MODE, TAP; constexpr bool DFA; const TextDfaArgs* d (null when DFA is off).
    __shared__ float sv[4]; __shared__ int si[4];
    const int ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, step = *a.n_dec;
    const int ban = step < a.p->min_new ? a.p->eos : -1;
    const int chunk = ((a.V + CFG_CHUNKS * 4 - 1) / (CFG_CHUNKS * 4)) * 4;
    const int v0 = ch * chunk, v1 = v0 + chunk < a.V ? v0 + chunk : a.V;
    const float* lp = a.logits_partial + (long)b * a.V;
    float best = -INFINITY; int bi = 0x7fffffff;
    float invT = 1.f; uint64_t seed = 0, stream = 0;
    if (MODE == TEXT_SAMPLE) {
        invT = 1.f / a.p->temperature; seed = a.p->seed;
        stream = (uint64_t)(b + a.p->row_off) * 1000003ull + step;
    }
    float* tap = TAP ? a.logits_out + ((long)step * gridDim.y + b) * a.V : nullptr;
    float* mrow = MODE == TEXT_STORE ? mix + (long)b * a.V : nullptr;
    const uint32_t* allow = nullptr; const int16_t* tc = nullptr; uint8_t* keep = nullptr;
    if constexpr (DFA) {
        __shared__ uint32_t s_allow[TEXT_DFA_MAX_CLASSES / 32];
        const int st = d->state[b], nst = d->hdr->n_states, ncl = d->hdr->n_classes, budget = a.p->max_new - step - 1;
        const bool live = st >= 0 && st < nst;              // a state outside the table allows nothing (the pick then emits eos)
#pragma unroll
        for (int c0 = 0; c0 < TEXT_DFA_MAX_CLASSES; c0 += 256) {
            const int c = c0 + tid;
            bool ok = false;
            if (live && c < ncl) {
                const int nx = d->next_state[(long)st * ncl + c];
                ok = nx >= 0 && d->dist[nx] <= budget;
            }
            const unsigned long long m = __ballot(ok);
            if ((tid & 63) == 0) { s_allow[c >> 5] = (uint32_t)m; s_allow[(c >> 5) + 1] = (uint32_t)(m >> 32); }
        }
        __syncthreads();
        allow = s_allow; tc = d->token_class;
        if (MODE != TEXT_STORE && d->keep) keep = d->keep + (long)b * a.V;
    }
    auto allowed = [&](uint32_t c) -> bool { c &= TEXT_DFA_MAX_CLASSES - 1; return (allow[c >> 5] >> (c & 31)) & 1u; };
    if (((a.V | (int)(a.slab & 3)) & 3) == 0) {
        // eight independent 16-byte loads per slab in flight per thread (addresses clamped into the chunk, validity applied to the
        // compare): a plain `for v` / `for s` nest is one dependent round trip per vector and slab
        constexpr int IT = 8;
        for (int vb = v0 + tid * 4; vb < v1; vb += IT * 1024) {
            f32x4 c[IT];
            uint2 k[DFA ? IT : 1];
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int v = vb + it * 1024;
                c[it] = *(const f32x4*)(lp + (v < v1 ? v : v1 - 4));
                if constexpr (DFA) k[it] = *(const uint2*)(tc + (v < v1 ? v : v1 - 4));
            }
            for (int s = 1; s < a.S; ++s) {
                f32x4 t[IT];
#pragma unroll
                for (int it = 0; it < IT; ++it) {
                    const int v = vb + it * 1024;
                    t[it] = *(const f32x4*)(lp + (long)s * a.slab + (v < v1 ? v : v1 - 4));
                }
#pragma unroll
                for (int it = 0; it < IT; ++it) c[it] += t[it];
            }
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int v = vb + it * 1024;
                [[maybe_unused]] bool off[4];
                if constexpr (DFA) {
                    off[0] = !allowed(k[it].x & 0xffffu); off[1] = !allowed(k[it].x >> 16);
                    off[2] = !allowed(k[it].y & 0xffffu); off[3] = !allowed(k[it].y >> 16);
                    if (keep && v < v1) {
                        uint32_t kb = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) kb |= (uint32_t)(!off[j] && v + j != ban && c[it][j] > -INFINITY) << (8 * j);
                        *(uint32_t*)(keep + v) = kb;
                    }
                }
                if (MODE == TEXT_STORE || TAP) {
                    if (v < v1) {                                  // V % 4 == 0: a vector is wholly inside the chunk or wholly outside
                        f32x4 w = c[it];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (v + j == ban) w[j] = -INFINITY;
                            if constexpr (DFA) { if (off[j]) w[j] = -INFINITY; }
                        }
                        if (TAP) *(f32x4*)(tap + v) = w;
                        if (MODE == TEXT_STORE) *(f32x4*)(mrow + v) = w;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float cj = (v + j == ban || v >= v1) ? -INFINITY : c[it][j];
                    if constexpr (DFA) { if (off[j]) cj = -INFINITY; }
                    if (MODE == TEXT_SAMPLE && v < v1) cj = gumbel_perturb(cj, invT, seed, stream, v + j);
                    if (cj > best) { best = cj; bi = v + j; }
                }
            }
        }
    } else {
        for (int v = v0 + tid; v < v1; v += 256) {
            float c = 0.f;
            for (int s = 0; s < a.S; ++s) c += lp[(long)s * a.slab + v];
            if (v == ban) c = -INFINITY;
            if constexpr (DFA) {
                if (!allowed((uint16_t)tc[v])) c = -INFINITY;
                if (keep) keep[v] = c > -INFINITY;
            }
            if (TAP) tap[v] = c;
            if (MODE == TEXT_STORE) mrow[v] = c;
            if (MODE == TEXT_SAMPLE) c = gumbel_perturb(c, invT, seed, stream, v);
            if (c > best) { best = c; bi = v; }
        }
    }
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
