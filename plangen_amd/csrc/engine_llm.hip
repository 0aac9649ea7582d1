// pg_engine: the language-model side of the path -- packed prefill, the 576-step CFG decode loop (System.sample_image,
// plangen_base.py:567-607), single steps behind language_model.model(...), gen_head, greedy text decode (System.x2t, :513-523).
#include "engine.h"

// =============================================================================== LLM
// C = a . W^T into the view's fp32 split-K slabs ``part`` [S_last][M][N].
template <typename T>
void pg_engine::gemm_llm(hipStream_t s, DecodeView& v, const T* a, const T* W, int M, int N, int K, bool allow_skinny, const void* Wt) {
    v.slab_last = (long)M * N;
    if constexpr (std::is_same<T, bf16>::value) {
        if (allow_skinny && M <= 512 && K % 128 == 0) {
            const int S = skinny_pick_splits(N, K, M);
            if ((long)S * M * N <= part_elems) {
                launch_gemm_skinny(s, a, W, v.part, M, N, K, S, (const bf16*)Wt);
                v.S_last = S;
                return;
            }
        }
    }
    GemmA ga; ga.ptr = a; ga.lda = K;
    GemmEpi e; e.out = v.part; e.out_f32 = 1; e.ldc = N;
    launch_gemm<T>(s, ga, W, K, 0, e, M, N, K, 1);
    v.S_last = 1;
}

// Prefill form of the two projections that end a residual branch: x[M,N] (fp32 residual stream) += a . W^T in the GEMM's own epilogue
// (every element is read and written by the same lane), so the norm kernel that follows has no slab to fold in (S_last = 0): it reads x
// and writes xn only -- 220 MB less traffic per norm at the bench's 13.4 k packed tokens.  Same fp32 sum as the slab form (x + acc), bit for bit.
template <typename T>
void pg_engine::gemm_residual(hipStream_t s, DecodeView& v, const T* a, const T* W, int M, int N, int K) {
    GemmA ga; ga.ptr = a; ga.lda = K;
    GemmEpi e; e.out = v.x; e.out_f32 = 1; e.ldc = N; e.residual = v.x; e.res_f32 = 1;
    launch_gemm<T>(s, ga, W, K, 0, e, M, N, K, 1);
    v.S_last = 0; v.slab_last = (long)M * N;
}

// The layer stack on M token rows.  mode 0: decode (row m = batch row, slot len+n_dec);
// mode 1: prefill (packed prompt tokens).  Residual stream x fp32 [M,H]; ends with the final
// RMSNorm written to final_out (T).  Every GEMM leaves fp32 split-K slabs in ``part``; the
// next elementwise kernel folds the reduction in (deterministic, no atomics).
template <typename T>
void pg_engine::run_layers(hipStream_t s, DecodeView& v, int M, int mode, T* final_out, int32_t* advance) {
    const int Hh = H(), I = cfg.inter, HDm = HD();
    const bool sk = mode == 0;
    int S_pend = 0; long slab_pend = 0;
    const float scale = 1.0f / sqrtf(128.0f);
    tc_on = time_attn && mode == 0 && (n_dec_host % (time_stride > 0 ? time_stride : 1)) == 0;
    const double wb = (double)esz;                                  // weight bytes per element
    auto norm_bytes = [&](int S) { return (double)M * Hh * (4.0 * (S + 2) + wb); };   // x + S slabs read, x written (S > 0), xn written
    for (int li = 0; li < cfg.n_layers; ++li) {
        const Layer& ly = layers[li];
        tic(s); toc(s, TC_EMPTY, 0.0);          // an event pair around nothing: what the instrumentation itself adds to every timed launch
        tic(s);
        // Deferred 1/rms (round 6; decode at 65..128 rows, bf16): the norm launch becomes a barrier-free elementwise pass (residual + xw = bf16(x . w) +
        // 8 partial sums of squares per row) and the consumer GEMM scales its fp32 result by the row's 1/rms (kernels.h).  PG_F32 and every other
        // row count keep rmsnorm512_kernel; layer 0 of a step has no slabs to fold in (S_pend = 0) and keeps it too.
        bool d1 = false, d2 = false;
        int Sq = 0;
        if constexpr (std::is_same<T, bf16>::value) {
            if (sk && defer_norm && Hh == 2048 && S_pend > 0 && S_pend <= 8 && slab_pend <= 0x7fffffffL && ly.wqkv_t) {
                Sq = skinny_pick_splits(3 * HDm, Hh, M);
                d1 = deferred_norm_ok(M, 3 * HDm, Hh, Sq) && (long)Sq * M * 3 * HDm <= part_elems;
            }
            if (d1) launch_rmsnorm_defer(s, v.x, v.part, S_pend, slab_pend, (const bf16*)ly.ln1, (bf16*)v.xn, ssq_part, M, Hh);
        }
        if (!d1) launch_rmsnorm<T>(s, v.x, v.part, S_pend, slab_pend, (const T*)ly.ln1, (T*)v.xn, M, Hh, cfg.rms_eps);
        toc(s, TC_NORM, norm_bytes(S_pend));
        tic(s);
        bool qkv_fused = false;
        if constexpr (std::is_same<T, bf16>::value) {
            // prefill: RoPE(q), RoPE(k) and the KV-cache write in the QKV GEMM's own epilogue when the packed batch is big enough
            // for the 256x256 kernel; smaller batches keep GEMM -> fp32 q|k|v -> rope_kv_kernel on the un-interleaved weights
            if (mode == 1 && prefill_rope_epi && ly.wqkv_p) {
                GemmA ga; ga.ptr = v.xn; ga.lda = Hh;
                GemmEpi ge; ge.act = 3; ge.out = v.qbuf; ge.out_f32 = 0; ge.ldc = 3 * HDm;
                ge.rope.qbuf = v.qbuf; ge.rope.kc = kc(v, li); ge.rope.vc = vc(v, li); ge.rope.cos_t = cos_t; ge.rope.sin_t = sin_t;
                ge.rope.tok_row = d_tok_row; ge.rope.tok_j = d_tok_j; ge.rope.pos_off = v.d_pos_off;
                ge.rope.nh = cfg.n_heads; ge.rope.slots = slots; ge.rope.max_pos = max_pos;
                qkv_fused = gemm256_try(s, ga, (const bf16*)ly.wqkv_p, Hh, 0, ge, M, 3 * HDm, Hh, 1, 1, 0);
            }
        }
        if constexpr (std::is_same<T, bf16>::value) {
            if (d1) {
                d1 = launch_gemm_skinny_deferred(s, (const bf16*)v.xn, (const bf16*)ly.wqkv_t, v.part, M, 3 * HDm, Hh, Sq, ssq_part, cfg.rms_eps);
                if (d1) { v.S_last = Sq; v.slab_last = (long)M * 3 * HDm; qkv_fused = true; }
                else launch_rmsnorm<T>(s, v.x, v.part, 0, 0, (const T*)ly.ln1, (T*)v.xn, M, Hh, cfg.rms_eps);   // cannot happen (one predicate); the residual is already updated: normalise it the ordinary way
            }
        }
        if (!qkv_fused) gemm_llm<T>(s, v, (const T*)v.xn, (const T*)ly.wqkv, M, 3 * HDm, Hh, sk, ly.wqkv_t);
        toc(s, TC_QKV, 3.0 * HDm * Hh * wb);
        if (mode == 0 && skip_attn) {
            // nothing: the GEMM + norm phase alone (outputs are garbage by construction)
        } else if (mode == 0 && fuse_rope) {
            tic(s);
            if (kv8)
                launch_attn_decode_kv8(s, v.part, v.S_last, v.slab_last, (bf16*)v.obuf, kc8(li), vc8(li), kvs(li), cos_t, sin_t, seq(v), M, cfg.n_heads,
                                       slots, max_pos, scale);
            else
            launch_attn_decode_fused<T>(s, v.part, v.S_last, v.slab_last, (T*)v.obuf, (T*)kc(v, li), (T*)vc(v, li), cos_t, sin_t, seq(v), M,
                                        cfg.n_heads, slots, max_pos, scale);
        } else {
            if (!qkv_fused)
                launch_rope_kv<T>(s, v.part, v.S_last, v.slab_last, (T*)v.qbuf, (T*)kc(v, li), (T*)vc(v, li), cos_t, sin_t, seq(v), mode, M,
                                  cfg.n_heads, slots, max_pos);
            tic(s);
            bool done = false;
            if constexpr (std::is_same<T, bf16>::value) {
                if (mode == 1 && flash_prefill && ext_nnew) {       // pg_prefill_extend: the packed tokens are the rows' new tokens, behind cached slots
                    launch_attn_extend_flash(s, (const bf16*)v.qbuf, (bf16*)v.obuf, (const bf16*)kc(v, li), (const bf16*)vc(v, li), d_row_off, v.d_len,
                                             ext_nnew, v.rows, ext_max_new, cfg.n_heads, slots, scale);
                    done = true;
                } else if (mode == 1 && flash_prefill) {
                    launch_attn_prefill_flash(s, (const bf16*)v.qbuf, (bf16*)v.obuf, (const bf16*)kc(v, li), (const bf16*)vc(v, li), d_row_off, v.d_len,
                                              v.rows, max_len_host, cfg.n_heads, slots, scale);
                    done = true;
                }
            }
            if (!done)
                launch_attn<T>(s, (const T*)v.qbuf, (T*)v.obuf, (const T*)kc(v, li), (const T*)vc(v, li), seq(v), mode, M, cfg.n_heads, slots, scale);
            // pg_request_attn_spans: this layer's RoPE'd Q and K are both still in place (FP8 cache: the bf16 scratch, before it is quantised)
            if constexpr (std::is_same<T, bf16>::value) {
                if (mode == 1 && as_run && ((as_run->mask >> li) & 1)) {
                    const AttnSpanRun& a = *as_run;
                    const int nth = __builtin_popcountll(a.mask & ((1ull << li) - 1));          // layers ascending
                    launch_attn_span_mass(s, (const bf16*)v.qbuf, (const bf16*)kc(v, li), d_row_off, v.d_len, a.d_pad, a.d_lo, a.d_hi, a.n_spans,
                                          a.q_col0, a.n_q, v.rows, cfg.n_heads, slots, scale, a.out + nth * a.layer_floats);
                }
            }
            // FP8 KV cache: this layer's K/V of the packed tokens, bf16 scratch -> codes + scales (prefill only: decode never takes this branch)
            if (kv8 && mode == 1)
                launch_kv_quantize(s, (const bf16*)kc(v, li), (const bf16*)vc(v, li), kc8(li), vc8(li), kvs(li), d_tok_row, d_tok_j, M, cfg.n_heads, slots);
        }
        if (tc_on && !(mode == 0 && skip_attn)) {
            double keys = shared_len;       // the shared uncond prompt is read from HBM once per launch
            for (int r = 0; r < v.rows; ++r) {
                keys += (double)(h_len[v.r0 + r] + n_dec_host + 1) - ((shared_len > 0 && (r & 1)) ? shared_len : 0);
                // grouped form: a replica's prompt is its owner's -- counted once, with the owner
                if (group_rows > 0 && r >= group_rows && !(shared_len > 0 && (r & 1))) keys -= (double)h_len[v.r0 + r];
            }
            toc(s, TC_ATTN, keys * cfg.n_heads * 2 * (kv8 ? 128.0 + 4.0 : 128.0 * (double)esz));      // FP8 cache: 128 codes + one fp32 scale per key, K and V
        }
        tic(s);
        if (!sk && prefill_res_epi) gemm_residual<T>(s, v, (const T*)v.obuf, (const T*)ly.wo, M, Hh, HDm);      // prefill: x += o . Wo^T in the GEMM's epilogue
        else gemm_llm<T>(s, v, (const T*)v.obuf, (const T*)ly.wo, M, Hh, HDm, sk, ly.wo_t);
        toc(s, TC_O, (double)Hh * HDm * wb);
        tic(s);
        if constexpr (std::is_same<T, bf16>::value) {
            if (sk && defer_norm && Hh == 2048 && v.S_last > 0 && v.S_last <= 8 && v.slab_last <= 0x7fffffffL && ly.wgu_t)
                d2 = deferred_norm_ok(M, 2 * I, Hh, 1) && (force_swiglu || skinny_pick_splits(2 * I, Hh, M) == 1);
            if (d2) launch_rmsnorm_defer(s, v.x, v.part, v.S_last, v.slab_last, (const bf16*)ly.ln2, (bf16*)v.xn, ssq_part, M, Hh);
        }
        if (!d2) launch_rmsnorm<T>(s, v.x, v.part, v.S_last, v.slab_last, (const T*)ly.ln2, (T*)v.xn, M, Hh, cfg.rms_eps);
        toc(s, TC_NORM, norm_bytes(v.S_last));
        bool fused = false;
        tic(s);
        if constexpr (std::is_same<T, bf16>::value) {
            if (d2) {
                fused = launch_gemm_skinny_swiglu_deferred(s, (const bf16*)v.xn, (const bf16*)ly.wgu_t, (bf16*)v.hbuf, M, 2 * I, Hh, ssq_part, cfg.rms_eps);
                if (!fused) launch_rmsnorm<T>(s, v.x, v.part, 0, 0, (const T*)ly.ln2, (T*)v.xn, M, Hh, cfg.rms_eps);   // cannot happen (one predicate); see the QKV site
            }
            // decode: SwiGLU gate fused into the gate|up GEMM epilogue (S = 1, no slab, no extra kernel)
            if (!fused && sk && M <= 512 && Hh % 128 == 0 && (force_swiglu || skinny_pick_splits(2 * I, Hh, M) == 1))   // fused wins at every M (B=4/8/16: -2..3 % loop time)
                fused = launch_gemm_skinny_swiglu(s, (const bf16*)v.xn, (const bf16*)ly.wgu, (bf16*)v.hbuf, M, 2 * I, Hh, (const bf16*)ly.wgu_t);
        }
        if constexpr (std::is_same<T, bf16>::value) {
            // prefill: SwiGLU in the 256x256 GEMM's epilogue (h written as bf16, no fp32 gate|up tensor, no extra pass)
            if (!fused && !sk && (I % 4) == 0) {
                GemmA ga; ga.ptr = v.xn; ga.lda = Hh;
                GemmEpi ge; ge.out = v.hbuf; ge.out_f32 = 0; ge.ldc = I; ge.act = 2;
                fused = gemm256_try(s, ga, (const bf16*)ly.wgu, Hh, 0, ge, M, 2 * I, Hh, 1, 1, 0);
            }
        }
        if (!fused) {
            gemm_llm<T>(s, v, (const T*)v.xn, (const T*)ly.wgu, M, 2 * I, Hh, sk, ly.wgu_t);
            launch_silu_mul<T>(s, v.part, v.S_last, v.slab_last, (T*)v.hbuf, M, I);
        }
        toc(s, TC_GU, 2.0 * I * Hh * wb);
        tic(s);
        if (!sk && prefill_res_epi) gemm_residual<T>(s, v, (const T*)v.hbuf, (const T*)ly.wd, M, Hh, I);         // prefill: x += h . Wd^T
        else gemm_llm<T>(s, v, (const T*)v.hbuf, (const T*)ly.wd, M, Hh, I, sk, ly.wd_t);
        toc(s, TC_DOWN, (double)Hh * I * wb);
        S_pend = v.S_last; slab_pend = v.slab_last;
    }
    tic(s);
    launch_rmsnorm<T>(s, v.x, v.part, S_pend, slab_pend, (const T*)norm_w, final_out, M, Hh, cfg.rms_eps, advance);
    toc(s, TC_NORM, norm_bytes(S_pend));
    tc_on = false;
}

int pg_engine::prefill(const int32_t* ids_dev, const void* emb_dev, int emb_dtype, const int32_t* pad_len, int R0, int L_,
                       int pmode, void* hidden_out, int hidden_dtype, hipStream_t s, int replicas, int alias, bool replicated_api) {
    // one-shot: the hint describes the ids of THIS call only -- consumed before anything can fail, so that a rejected call
    // cannot leave it armed for the next batch
    const int hint = uncond_hint; uncond_hint = -1;
    const bool as = as_pending; as_pending = false;      // pg_request_attn_spans: one-shot in the same way
    if (!finalized) FAIL(PG_ERR_STATE, "pg_finalize_weights not called");
    if (as) {       // nothing is launched when the request does not fit this call
        const pg_attn_spans& q = as_req;
        if (replicated_api) FAIL(PG_ERR_ARG, "pg_request_attn_spans: pg_prefill_replicated packs owner rows only and cannot serve it");
        if (!bf) FAIL(PG_ERR_ARG, "pg_request_attn_spans: the span kernel is bf16; a PG_F32 handle cannot serve it");
        if (q.rows != R0) FAIL(PG_ERR_ARG, "pg_request_attn_spans: requested for %d rows, the prefill has %d", q.rows, R0);
        if (q.q_col0 < 0 || q.n_q < 1 || (long)q.q_col0 + q.n_q > L_) FAIL(PG_ERR_ARG, "pg_request_attn_spans: query columns [%d, %d + %d) leave the %d columns of the prefill", q.q_col0, q.q_col0, q.n_q, L_);
        for (size_t i = 0; i < as_lo.size(); ++i)
            if (as_lo[i] < 0 || as_lo[i] > L_ || as_hi[i] < 0 || as_hi[i] > L_) FAIL(PG_ERR_ARG, "pg_request_attn_spans: span %d of row %d, [%d, %d), leaves [0, %d]", (int)(i % q.n_spans), (int)(i / q.n_spans), as_lo[i], as_hi[i], L_);
        if (q.capacity_floats < (int64_t)__builtin_popcountll(q.layer_mask) * R0 * q.n_q * q.n_spans)
            FAIL(PG_ERR_CAPACITY, "pg_request_attn_spans: capacity_floats %lld < %d layers x %d rows x %d queries x %d spans", (long long)q.capacity_floats, __builtin_popcountll(q.layer_mask), R0, q.n_q, q.n_spans);
    }
    // Replicated batch (pg_prefill_replicated): R_ = R0 * replicas VIRTUAL rows, row t * R0 + r = replica t of row r (the reference's [all pairs] x p,
    // plangen_base.py:547).  Everything below is decided on the virtual rows exactly as a plain prefill of the replicated ids would decide it; only the
    // rows that own their prompt (owner(row) == row) are packed and run through the layer stack.
    if (replicated_api) {          // pg_prefill_replicated's own argument rules (behind the one-shot hint's consumption, like every other rejection)
        if (replicas < 1 || R0 < 1 || (alias != 0 && alias != 1)) FAIL(PG_ERR_ARG, "pg_prefill_replicated: R0=%d and replicas=%d must be >= 1 and alias=%d 0 or 1", R0, replicas, alias);
        if ((long)R0 * replicas > cfg.max_rows) FAIL(PG_ERR_CAPACITY, "%d rows x %d replicas > max_rows %d", R0, replicas, cfg.max_rows);
    }
    if (replicas > 1 && !fuse_rope) FAIL(PG_ERR_ARG, "pg_prefill_replicated needs the fused decode attention (fuse_rope)");
    const int R_ = R0 * replicas;
    auto pad_of = [&](int r) { return pad_len[r % R0]; };
    if (R_ <= 0 || R_ > cfg.max_rows) FAIL(PG_ERR_CAPACITY, "rows %d > max_rows %d", R_, cfg.max_rows);
    if (L_ + cfg.max_new + 1 > max_pos) FAIL(PG_ERR_CAPACITY, "padded length %d too long for the RoPE table (%d)", L_, max_pos);
    if (!ids_dev && !emb_dev) FAIL(PG_ERR_ARG, "ids or embeds required");
    HIPCHK(hipSetDevice(dev));
    for (int r = 0; r < R0; ++r) {                 // validate every row BEFORE pad_len is used as an offset anywhere
        const int pad = pad_len[r];
        if (pad < 0 || pad >= L_) FAIL(PG_ERR_ARG, "row %d: pad_len %d not in [0,%d)", r, pad, L_);
        if (L_ - pad > cfg.max_prompt) FAIL(PG_ERR_CAPACITY, "row %d: %d prompt tokens > max_prompt %d", r, L_ - pad, cfg.max_prompt);
    }
    // Shared negative prompt (the uncond prompt is batch-constant for non-edit
    // data): when every odd row carries the same ids and padding, its prompt is prefilled and
    // its K/V stored ONCE (row 1); the other uncond rows alias it.  Verified per batch, never
    // assumed: the ids are compared ON THE DEVICE and one 4-byte flag comes back (the only
    // host<->device round trip of pg_prefill: the packed-token count, hence every GEMM shape of
    // the prefill, depends on the answer).  Only on the fused path (no per-position hidden output).
    shared_len = 0;
    // (replicated: the odd virtual rows are the odd rows of every replica -- R0 must be even for that -- and the probe compares the distinct ones)
    // (a pending span request needs every row's own Q and K: no sharing)
    if (share_uncond && fuse_rope && ids_dev && !hidden_out && pmode == 0 && R_ >= 4 && (R0 % 2) == 0 && !as) {
        bool same = true;
        for (int r = 3; r < R_ && same; r += 2) same = pad_of(r) == pad_len[1];
        if (same && hint == 1) shared_len = L_ - pad_len[1];      // the caller compared the ids on the host (its collate built them): no probe, no sync
        else if (same && hint != 0) {
            HIPCHK(hipMemsetAsync(d_flag, 0, 4, s));
            launch_rows_differ(s, ids_dev, L_, /*first*/ 3, /*stride*/ 2, /*ref row*/ 1, (R0 - 2) / 2, pad_len[1], d_flag);
            HIPCHK(hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (*h_flag == 0) shared_len = L_ - pad_len[1];
        }
    }
    // pinned staging is double-buffered: the copies of call n are still in flight while call n+1 fills
    // the other buffer; a buffer is reused only after the event recorded behind its copies has fired
    // (two calls back: in practice never waits), so pg_prefill itself does not synchronise the stream.
    stage_sel ^= 1;
    int32_t* const hs = h_stage2[stage_sel];
    if (stage_used[stage_sel]) HIPCHK(hipEventSynchronize(ev_stage[stage_sel]));
    int ntok = 0;
    h_len.assign(R_, 0); h_pos_off.assign(R_, 0);
    int32_t* s_len = hs; int32_t* s_off = hs + cfg.max_rows; int32_t* s_last = hs + 2 * cfg.max_rows;
    int32_t* s_roff = hs + 3 * cfg.max_rows; int32_t* s_ord = hs + 4 * cfg.max_rows; max_len_host = 0;
    int32_t* s_row = hs + 5 * cfg.max_rows; int32_t* s_j = s_row + max_tok; int32_t* s_src = s_j + max_tok;
    // owner rule: the shared uncond prompt's row for odd rows when it is shared, else the row's first replica
    auto owner = [&](int r) { return (shared_len > 0 && (r & 1)) ? 1 : r % R0; };
    for (int r = 0; r < R_; ++r) {
        const int pad = pad_of(r);
        const int len = L_ - pad;
        h_len[r] = len; s_len[r] = len; s_off[r] = pmode == 0 ? pad : 0; h_pos_off[r] = s_off[r];
        if (owner(r) != r) { s_last[r] = s_last[owner(r)]; s_roff[r] = -1; continue; }   // aliases its owner's prompt (owner(r) < r)
        s_roff[r] = ntok; if (len > max_len_host) max_len_host = len;
        for (int j = 0; j < len; ++j) { s_row[ntok] = r; s_j[ntok] = j; s_src[ntok] = r * L_ + pad + j; ++ntok; }
        s_last[r] = ntok - 1;
    }
    R = R_; L = L_; n_dec_host = 0;
    replicas_n = replicas; group_rows = (replicas > 1 && alias == 1) ? R0 : 0;
    {   // longest-first row order for the decode attention launch (private keys per row)
        for (int r = 0; r < R_; ++r) s_ord[r] = r;
        // grouped form: a replica walks its owner's prompt (from L2, one hopes) -- same key as its owner, and ties go by owner, so the replicas of one
        // owner sit next to each other in the launch (same head -> same XCD, close in time)
        const int G = group_rows;
        std::stable_sort(s_ord, s_ord + R_, [&](int a, int b) {
            const int ka = h_len[a] - ((shared_len > 0 && (a & 1)) ? shared_len : 0), kb = h_len[b] - ((shared_len > 0 && (b & 1)) ? shared_len : 0);
            if (G > 0 && ka == kb) return a % G < b % G;
            return ka > kb; });
        order_valid = true; order_rows = R_;
    }
    HIPCHK(hipEventRecord(ev_p0, s));
    HIPCHK(hipMemcpyAsync(d_row_order, s_ord, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_len, s_len, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pos_off, s_off, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_last, s_last, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_row_off, s_roff, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tok_row, s_row, (size_t)ntok * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tok_j, s_j, (size_t)ntok * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tok_src, s_src, (size_t)ntok * 4, hipMemcpyHostToDevice, s));
    AttnSpanRun asr{};
    if (as) {       // pad_len and the spans ride in the same pinned staging buffer, behind the token lists
        const int n = as_req.rows * as_req.n_spans;
        int32_t* s_as = hs + 5 * cfg.max_rows + 3 * max_tok + 16;
        for (int r = 0; r < R_; ++r) s_as[r] = pad_of(r);
        std::copy(as_lo.begin(), as_lo.end(), s_as + cfg.max_rows);
        std::copy(as_hi.begin(), as_hi.end(), s_as + 17 * cfg.max_rows);
        HIPCHK(hipMemcpyAsync(d_as, s_as, (size_t)R_ * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_as + cfg.max_rows, s_as + cfg.max_rows, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_as + 17 * cfg.max_rows, s_as + 17 * cfg.max_rows, (size_t)n * 4, hipMemcpyHostToDevice, s));
        asr = AttnSpanRun{d_as, d_as + cfg.max_rows, d_as + 17 * cfg.max_rows, as_req.n_spans, as_req.q_col0, as_req.n_q, as_req.layer_mask,
                          as_req.out_dev, (long)R_ * as_req.n_q * as_req.n_spans};
    }
    HIPCHK(hipEventRecord(ev_stage[stage_sel], s));
    stage_used[stage_sel] = true;
    HIPCHK(hipMemsetAsync(d_ndec, 0, 64, s));
    HIPCHK(hipMemsetAsync(d_ndec2, 0, 64, s));
    if (ids_dev) launch_embed_gather(s, embed, ids_dev, d_tok_src, x, ntok, H(), cfg.vocab);
    else launch_rows_to_f32(s, emb_dev, emb_dtype == PG_BF16, d_tok_src, x, ntok, H());
    DecodeView v = view(0, R, 0);
    as_run = as ? &asr : nullptr;
    if (bf) run_layers<bf16>(s, v, ntok, 1, (bf16*)xn); else run_layers<float>(s, v, ntok, 1, (float*)xn);
    as_run = nullptr;
    // last real token of every row -> hfin (input of gen_head / lm_head for the first sample)
    launch_copy_rows(s, xn, d_last, hfin, nullptr, R, (long)H() * esz);
    if (replicas > 1 && alias == 0) {     // the equality-tested fallback: every replica gets a private copy of its owner's prompt K/V, decode runs today's kernels
        const size_t cb = kv8 ? 1 : esz;
        launch_kv_replicate(s, kv, (long)(kv_layer_elems() * cb), 2 * cfg.n_layers, (long)slots * 128 * (long)cb, (int)(128 * cb), d_len, R0, R, cfg.n_heads, shared_len);
        if (kv8) launch_kv_replicate(s, kv_scale, (long)(2 * kv_layer_slots() * 4), cfg.n_layers, (long)slots * 8, 8, d_len, R0, R, cfg.n_heads, shared_len);
    }
    if (hidden_out) {
        const size_t ob = (size_t)R * L * H() * (hidden_dtype == PG_BF16 ? 2 : 4);
        HIPCHK(hipMemsetAsync(hidden_out, 0, ob, s));
        if (bf) launch_t_to_rows<bf16>(s, (const bf16*)xn, hidden_out, hidden_dtype == PG_BF16, d_tok_src, ntok, H());
        else launch_t_to_rows<float>(s, (const float*)xn, hidden_out, hidden_dtype == PG_BF16, d_tok_src, ntok, H());
    }
    HIPCHK(hipEventRecord(ev_p1, s));
    have_prefill_t = true;
    HIPCHK(hipGetLastError());
    prefilled = true; hfin_stale = false;
    return PG_OK;
}

// ---- pg_prefill_extend / pg_rewind: continue or shorten the cached sequences.  cur[r] = h_len[r] + n_dec_host is what row r holds: its prompt
// plus the decode steps run since (the token a loop emitted last was never fed back and has no slot).
int pg_engine::check_extendable(const char* who) {
    if (!prefilled) FAIL(PG_ERR_STATE, "%s before pg_prefill", who);
    if (replicas_n > 1) FAIL(PG_ERR_STATE, "%s after pg_prefill_replicated with replicas > 1: replicas alias their owner's prompt slots", who);
    if (shared_len > 0)
        FAIL(PG_ERR_STATE, "%s: the batch shares its negative prompt (it lives in row 1's slots, which the prefill attention kernels do not follow); "
                           "prefill with the one-shot pg_set_option(\"uncond_shared_hint\", 0)", who);
    if (kv8) FAIL(PG_ERR_ARG, "%s: an FP8 KV cache keeps past keys as codes only and prefill attention needs bf16", who);
    return PG_OK;
}
// The rows' new lengths (s_len, pinned staging) become the row-set geometry: h_len, max_len_host, the longest-first order of the decode attention
// (into s_ord, same staging buffer) and step counters at zero.  Small copies and memsets only; the caller records the staging event behind them.
int pg_engine::set_lengths(const int32_t* s_len, int32_t* s_ord, hipStream_t s) {
    max_len_host = 0;
    for (int r = 0; r < R; ++r) { h_len[r] = s_len[r]; s_ord[r] = r; if (h_len[r] > max_len_host) max_len_host = h_len[r]; }
    std::stable_sort(s_ord, s_ord + R, [&](int a, int b) { return h_len[a] > h_len[b]; });      // shared_len = 0 and no replica groups here
    order_valid = true; order_rows = R; n_dec_host = 0;
    HIPCHK(hipMemcpyAsync(d_row_order, s_ord, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_len, s_len, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_ndec, 0, 64, s));
    HIPCHK(hipMemsetAsync(d_ndec2, 0, 64, s));
    return PG_OK;
}

int pg_engine::prefill_extend(const int32_t* ids_dev, const void* emb_dev, int emb_dtype, const int32_t* n_new, int Lx, void* hidden_out,
                              int hidden_dtype, hipStream_t s) {
    const bool as = as_pending; as_pending = false;      // one-shot: consumed before anything can fail; this call cannot serve it
    if (as) FAIL(PG_ERR_ARG, "pg_request_attn_spans: pg_prefill_extend cannot serve it (only pg_prefill / pg_prefill_embeds pack whole rows)");
    TRY(check_extendable("pg_prefill_extend"));
    if ((ids_dev == nullptr) == (emb_dev == nullptr)) FAIL(PG_ERR_ARG, "pg_prefill_extend: exactly one of ids_dev / embeds_dev must be given");
    if (emb_dev && emb_dtype != PG_F32 && emb_dtype != PG_BF16) FAIL(PG_ERR_ARG, "pg_prefill_extend: embeds_dtype %d is neither PG_F32 nor PG_BF16", emb_dtype);
    if (hidden_out && hidden_dtype != PG_F32 && hidden_dtype != PG_BF16) FAIL(PG_ERR_ARG, "pg_prefill_extend: hidden_dtype %d is neither PG_F32 nor PG_BF16", hidden_dtype);
    if (!n_new || Lx < 1) FAIL(PG_ERR_ARG, "pg_prefill_extend: n_new_host is NULL or Lx=%d < 1", Lx);
    for (int r = 0; r < R; ++r)
        if (n_new[r] < 1 || n_new[r] > Lx) FAIL(PG_ERR_ARG, "pg_prefill_extend: row %d: n_new %d not in [1, Lx=%d]", r, n_new[r], Lx);
    long total = 0;
    for (int r = 0; r < R; ++r) {
        const long end = (long)h_len[r] + n_dec_host + n_new[r];
        if (end > slots) FAIL(PG_ERR_CAPACITY, "pg_prefill_extend: row %d: %d cached + %d new tokens exceed the %d KV slots", r, h_len[r] + n_dec_host, n_new[r], slots);
        if (h_pos_off[r] + end > max_pos) FAIL(PG_ERR_CAPACITY, "pg_prefill_extend: row %d: position %ld exceeds the RoPE table (%d)", r, h_pos_off[r] + end - 1, max_pos);
        total += n_new[r];
    }
    if (total > max_tok) FAIL(PG_ERR_CAPACITY, "pg_prefill_extend: %ld new tokens exceed the packed-token capacity %ld", total, max_tok);
    HIPCHK(hipSetDevice(dev));
    stage_sel ^= 1;                                       // pinned staging as in prefill: double-buffered, guarded by an event
    int32_t* const hs = h_stage2[stage_sel];
    if (stage_used[stage_sel]) HIPCHK(hipEventSynchronize(ev_stage[stage_sel]));
    int32_t* s_len = hs; int32_t* s_last = hs + 2 * cfg.max_rows; int32_t* s_roff = hs + 3 * cfg.max_rows; int32_t* s_ord = hs + 4 * cfg.max_rows;
    int32_t* s_row = hs + 5 * cfg.max_rows; int32_t* s_j = s_row + max_tok; int32_t* s_src = s_j + max_tok;
    int32_t* s_nnew = hs + 5 * cfg.max_rows + 3 * max_tok + 16;      // the span request's place: no request runs here
    int ntok = 0, mx = 0;
    for (int r = 0; r < R; ++r) {
        const int cur = h_len[r] + n_dec_host, n = n_new[r];
        s_len[r] = cur + n; s_roff[r] = ntok; s_nnew[r] = n; if (n > mx) mx = n;
        for (int i = 0; i < n; ++i) { s_row[ntok] = r; s_j[ntok] = cur + i; s_src[ntok] = r * Lx + i; ++ntok; }
        s_last[r] = ntok - 1;
    }
    TRY(set_lengths(s_len, s_ord, s));
    HIPCHK(hipMemcpyAsync(d_last, s_last, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_row_off, s_roff, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_nnew, s_nnew, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tok_row, s_row, (size_t)ntok * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tok_j, s_j, (size_t)ntok * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tok_src, s_src, (size_t)ntok * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ev_stage[stage_sel], s));
    stage_used[stage_sel] = true;
    if (ids_dev) launch_embed_gather(s, embed, ids_dev, d_tok_src, x, ntok, H(), cfg.vocab);
    else launch_rows_to_f32(s, emb_dev, emb_dtype == PG_BF16, d_tok_src, x, ntok, H());
    // only the new tokens go through the GEMMs: packed, tok_j = cur + i, the prefill path of run_layers (RoPE epilogue included); the attention
    // reads the cached slots in front of them
    DecodeView v = view(0, R, 0);
    ext_nnew = d_nnew; ext_max_new = mx;
    if (bf) run_layers<bf16>(s, v, ntok, 1, (bf16*)xn); else run_layers<float>(s, v, ntok, 1, (float*)xn);
    ext_nnew = nullptr; ext_max_new = 0;
    launch_copy_rows(s, xn, d_last, hfin, nullptr, R, (long)H() * esz);      // each row's last new token -> hfin
    hfin_stale = false;
    if (hidden_out) {
        HIPCHK(hipMemsetAsync(hidden_out, 0, (size_t)R * Lx * H() * (hidden_dtype == PG_BF16 ? 2 : 4), s));
        if (bf) launch_t_to_rows<bf16>(s, (const bf16*)xn, hidden_out, hidden_dtype == PG_BF16, d_tok_src, ntok, H());
        else launch_t_to_rows<float>(s, (const float*)xn, hidden_out, hidden_dtype == PG_BF16, d_tok_src, ntok, H());
    }
    HIPCHK(hipGetLastError());
    return PG_OK;
}

// Row r keeps its first len_host[r] slots.  The slots behind them keep their stale keys and are never read (every attention kernel bounds its reads
// by the lengths on the device); hfin is NOT recomputed -- it belongs to whatever ran last -- so a pg_prefill_extend follows before anything samples (hfin_stale: the
// decode loops answer PG_ERR_STATE until then; pg_step, which takes its input from the caller, is allowed).
int pg_engine::rewind(const int32_t* len_host, hipStream_t s) {
    TRY(check_extendable("pg_rewind"));
    if (!len_host) FAIL(PG_ERR_ARG, "pg_rewind: len_host is NULL");
    for (int r = 0; r < R; ++r)
        if (len_host[r] < 1 || len_host[r] > h_len[r] + n_dec_host) FAIL(PG_ERR_ARG, "pg_rewind: row %d: length %d not in [1, %d]", r, len_host[r], h_len[r] + n_dec_host);
    HIPCHK(hipSetDevice(dev));
    stage_sel ^= 1;
    int32_t* const hs = h_stage2[stage_sel];
    if (stage_used[stage_sel]) HIPCHK(hipEventSynchronize(ev_stage[stage_sel]));
    std::copy(len_host, len_host + R, hs);
    TRY(set_lengths(hs, hs + 4 * cfg.max_rows, s));
    hfin_stale = true;
    HIPCHK(hipEventRecord(ev_stage[stage_sel], s));
    stage_used[stage_sel] = true;
    return PG_OK;
}

// pg_request_attn_spans: what can be checked without the prefill is checked here; the host arrays are copied
int pg_engine::request_attn_spans(const pg_attn_spans* q) {
    if (!q) { as_pending = false; return PG_OK; }
    as_pending = false;                                   // a refused request leaves nothing pending either
    if (!q->span_lo_host || !q->span_hi_host || !q->out_dev) FAIL(PG_ERR_ARG, "pg_request_attn_spans: null pointer");
    if (q->rows < 1 || q->rows > cfg.max_rows) FAIL(PG_ERR_ARG, "pg_request_attn_spans: rows=%d not in [1, max_rows=%d]", q->rows, cfg.max_rows);
    if (q->n_spans < 1 || q->n_spans > 16) FAIL(PG_ERR_ARG, "pg_request_attn_spans: n_spans=%d not in [1, 16]", q->n_spans);
    if (q->q_col0 < 0 || q->n_q < 1) FAIL(PG_ERR_ARG, "pg_request_attn_spans: q_col0=%d must be >= 0 and n_q=%d >= 1", q->q_col0, q->n_q);
    if (q->layer_mask == 0 || (cfg.n_layers < 64 && (q->layer_mask >> cfg.n_layers) != 0))
        FAIL(PG_ERR_ARG, "pg_request_attn_spans: layer_mask must be non-zero and name layers below %d", cfg.n_layers);
    if (q->capacity_floats < 1) FAIL(PG_ERR_ARG, "pg_request_attn_spans: capacity_floats must be >= 1");
    if (!d_as) { HIPCHK(hipSetDevice(dev)); TRY(dalloc(&d_as, (size_t)33 * cfg.max_rows * 4)); }
    as_lo.assign(q->span_lo_host, q->span_lo_host + (size_t)q->rows * q->n_spans);
    as_hi.assign(q->span_hi_host, q->span_hi_host + (size_t)q->rows * q->n_spans);
    as_req = *q; as_req.span_lo_host = nullptr; as_req.span_hi_host = nullptr;
    as_pending = true;
    return PG_OK;
}
// pg_op_attn_span_mass: the kernel alone on the caller's device arrays
int pg_engine::op_attn_span_mass(const void* q, const void* k, const int32_t* row_off, const int32_t* len, const int32_t* pad_len, const int32_t* lo,
                                 const int32_t* hi, int R_, int nh, int slots_, int n_spans, int q_col0, int n_q, float scale, float* out, hipStream_t s) {
    if (!q || !k || !row_off || !len || !pad_len || !lo || !hi || !out) FAIL(PG_ERR_ARG, "pg_op_attn_span_mass: null pointer");
    if (!bf) FAIL(PG_ERR_ARG, "pg_op_attn_span_mass: the span kernel is bf16; a PG_F32 handle cannot run it");
    if (R_ < 1 || R_ > 65535 || nh < 1 || slots_ < 1 || n_spans < 1 || n_spans > 16 || q_col0 < 0 || n_q < 1)
        FAIL(PG_ERR_ARG, "pg_op_attn_span_mass: needs 1 <= R <= 65535, nh >= 1, slots >= 1, n_spans in [1, 16], q_col0 >= 0, n_q >= 1");
    HIPCHK(hipSetDevice(dev));
    launch_attn_span_mass(s, (const bf16*)q, (const bf16*)k, row_off, len, pad_len, lo, hi, n_spans, q_col0, n_q, R_, nh, slots_, scale, out);
    HIPCHK(hipGetLastError());
    return PG_OK;
}

// gen_head: Linear+b -> GELU(erf) -> Linear (second bias folded into the consumer)
template <typename T>
void pg_engine::head_logits(hipStream_t s, DecodeView& v, const T* in, int M) {
    const int Hh = H(), G = cfg.gen_head_dim, V = cfg.img_vocab;
    gemm_llm<T>(s, v, in, (const T*)gh_w1, M, G, Hh, true, gh_w1_t);
    launch_bias_act<T>(s, v.part, v.S_last, v.slab_last, gh_b1, (T*)v.gh_mid, M, G, 1);
    gemm_llm<T>(s, v, (const T*)v.gh_mid, (const T*)gh_w2, M, V, G, true, gh_w2_t);
}

void pg_engine::forward_decode(hipStream_t s, DecodeView& v) {
    // the final RMSNorm launch also advances the view's device step counter
    if (bf) run_layers<bf16>(s, v, v.rows, 0, (bf16*)v.hfin, v.d_ndec); else run_layers<float>(s, v, v.rows, 0, (float*)v.hfin, v.d_ndec);
}

// ---- what the two decode loops share
int pg_engine::reserve_requests(const TokenRequests& q) {      // the library-owned result buffers, allocated by the first request of each kind
    if (q.lp_out && !d_logprob) TRY(dalloc(&d_logprob, (size_t)cfg.max_rows * (cfg.max_new + 1) * 4, false));
    if (q.stats && !d_stats) TRY(dalloc(&d_stats, (size_t)cfg.max_rows * (cfg.max_new + 1) * 19 * 4, false));
    return PG_OK;
}
// graphs cannot be captured on the legacy default stream, and a second lane needs a stream to fork from: hop to istream behind the caller's work ...
int pg_engine::hop_in(hipStream_t s) { HIPCHK(hipEventRecord(ev_in, s)); HIPCHK(hipStreamWaitEvent(istream, ev_in, 0)); return PG_OK; }
// ... and put the caller's stream behind ours (nothing to do when the loop ran on the caller's stream)
int pg_engine::hop_out(hipStream_t ws, hipStream_t s) { if (ws != s) { HIPCHK(hipEventRecord(ev_out, ws)); HIPCHK(hipStreamWaitEvent(s, ev_out, 0)); } return PG_OK; }
// One replay of the step graph ``exec`` on s.  When ``key`` is not the cached one, record() -- which issues one step on s -- is captured first; a
// recording that fails ends the capture before its error is returned.
template <typename F>
int pg_engine::graph_step(hipGraphExec_t& exec, std::vector<int64_t>& cached, const std::vector<int64_t>& key, hipStream_t s, F&& record) {
    if (!exec || key != cached) {
        if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = record();
        hipError_t ce = hipStreamEndCapture(s, &g);
        if (rc != PG_OK) return rc;
        HIPCHK(ce);
        HIPCHK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        cached = key;
    }
    HIPCHK(hipGraphLaunch(exec, s));
    return PG_OK;
}

// pg_request_sample_plan: validate on the host, then stage the given arrays through pinned memory into their places in d_plan (no stream
// synchronisation: the staging buffer is guarded by an event).  Anything refused leaves nothing pending.
int pg_engine::request_sample_plan(const pg_sample_plan* pl, hipStream_t s) {
    plan_req.pending = false;
    if (!pl) return PG_OK;
    const int B = pl->B, T = pl->T;
    if (B < 1 || T < 1) FAIL(PG_ERR_ARG, "pg_request_sample_plan: B=%d and T=%d must be >= 1", B, T);
    if (!pl->cfg_weight_host && !pl->temperature_host && !pl->top_k_host && !pl->top_p_host && !pl->image_key_host)
        FAIL(PG_ERR_ARG, "pg_request_sample_plan: all five arrays are NULL");
    if (B > cfg.max_rows / 2 || T > cfg.max_new) FAIL(PG_ERR_CAPACITY, "pg_request_sample_plan: B=%d > max_rows / 2 = %d or T=%d > max_new=%d", B, cfg.max_rows / 2, T, cfg.max_new);
    if (pl->cfg_weight_host)
        for (long i = 0; i < (long)B * T; ++i)
            if (!std::isfinite(pl->cfg_weight_host[i])) FAIL(PG_ERR_ARG, "pg_request_sample_plan: cfg_weight[%ld][%ld] is not finite", i / T, i % T);
    for (int b = 0; b < B; ++b) {
        if (pl->temperature_host && !std::isfinite(pl->temperature_host[b])) FAIL(PG_ERR_ARG, "pg_request_sample_plan: temperature[%d] is not finite", b);
        if (pl->top_k_host && pl->top_k_host[b] < 0) FAIL(PG_ERR_ARG, "pg_request_sample_plan: top_k[%d]=%d must be >= 0", b, pl->top_k_host[b]);
        if (pl->top_p_host && !(pl->top_p_host[b] > 0.f && pl->top_p_host[b] <= 1.f)) FAIL(PG_ERR_ARG, "pg_request_sample_plan: top_p[%d]=%g must be in (0, 1]", b, (double)pl->top_p_host[b]);
        if (pl->image_key_host && pl->image_key_host[b] < 0) FAIL(PG_ERR_ARG, "pg_request_sample_plan: image_key[%d]=%d must be >= 0", b, pl->image_key_host[b]);
    }
    HIPCHK(hipSetDevice(dev));
    const size_t Bm = (size_t)cfg.max_rows / 2, total = (Bm * cfg.max_new + 4 * Bm) * 4;
    if (!ev_plan) {          // first request: the event is created last, so a failure part-way is retried from the start by the next call
        if (!d_plan) TRY(dalloc(&d_plan, total, false));     // no zero fill (and so no synchronisation): every array is copied here or filled by the consuming call before it is read
        if (!h_plan) HIPCHK(hipHostMalloc((void**)&h_plan, total));
        HIPCHK(hipEventCreateWithFlags(&ev_plan, hipEventDisableTiming));
    }
    if (plan_staged) HIPCHK(hipEventSynchronize(ev_plan));
    const SamplePlanDev d = plan_dev();
    const void* dst[5] = {d.w, d.temperature, d.top_k, d.top_p, d.key};
    const void* src[5] = {pl->cfg_weight_host, pl->temperature_host, pl->top_k_host, pl->top_p_host, pl->image_key_host};
    int mask = 0;
    for (int i = 0; i < 5; ++i) {
        if (!src[i]) continue;
        const size_t off = (const char*)dst[i] - (const char*)d_plan, n = (i == 0 ? (size_t)B * T : (size_t)B) * 4;
        memcpy(h_plan + off, src[i], n);
        HIPCHK(hipMemcpyAsync(const_cast<void*>(dst[i]), h_plan + off, n, hipMemcpyHostToDevice, s));
        mask |= 1 << i;
    }
    HIPCHK(hipEventRecord(ev_plan, s));
    plan_staged = true;
    plan_req.B = B; plan_req.T = T; plan_req.mask = mask;
    plan_req.temp.assign(pl->temperature_host ? pl->temperature_host : nullptr, pl->temperature_host ? pl->temperature_host + B : nullptr);
    plan_req.top_k.assign(pl->top_k_host ? pl->top_k_host : nullptr, pl->top_k_host ? pl->top_k_host + B : nullptr);
    plan_req.top_p.assign(pl->top_p_host ? pl->top_p_host : nullptr, pl->top_p_host ? pl->top_p_host + B : nullptr);
    plan_req.pending = true;
    return PG_OK;
}

// The image decode loop of both entry points: rows_per_image rows per image through the stack, one sampler step per token.  Everything around
// the sampler step is row-agnostic; the spec says what the entry point allows and whose name the messages carry.
int pg_engine::image_loop(const ImageLoopSpec& sp, int T, float temp, int top_k, float top_p, uint64_t seed, const int32_t* force_tok,
                          const uint8_t* force_mask, int32_t* out_tok, float* logits_out, hipStream_t s) {
    const int rpi = sp.rows_per_image;
    const bool dual = rpi == 3;
    const TokenRequests q = take_requests();      // the one-shot log-prob and stats requests: consumed whatever this call answers
    const bool score = q.lp_out != nullptr, stats = q.stats;
    const bool plan = plan_req.pending; plan_req.pending = false;      // pg_request_sample_plan: one-shot in the same way (consumed, then refused, where no plan is taken)
    if (top_k < 0 || !(top_p > 0.f && top_p <= 1.f)) FAIL(PG_ERR_ARG, "top_k=%d must be >= 0 and top_p=%g in (0, 1]", top_k, (double)top_p);
    if (dual && (!std::isfinite(sp.w) || !std::isfinite(sp.w_layout))) FAIL(PG_ERR_ARG, "%s: w_caption and w_layout must be finite", sp.name);
    if (!prefilled) FAIL(PG_ERR_STATE, "%s before pg_prefill", sp.name);
    if (plan && !sp.takes_plan) FAIL(PG_ERR_ARG, "%s does not take a sample plan (pg_request_sample_plan); the plan is dropped", sp.name);
    if (kv8 && !fuse_rope) FAIL(PG_ERR_ARG, "the FP8 KV cache needs the fused decode attention (fuse_rope)");
    if (lanes_opt == 2 && !sp.two_lanes) FAIL(PG_ERR_ARG, "%s does not support lanes = 2", sp.name);
    if (kv8 && lanes_opt == 2) FAIL(PG_ERR_ARG, "the FP8 KV cache does not support lanes = 2");
    if (group_rows > 0 && !sp.aliased_replicas) FAIL(PG_ERR_STATE, "%s does not support replicas that alias their owner's prompt (pg_prefill_replicated, alias = 1)", sp.name);
    if (group_rows > 0 && lanes_opt == 2) FAIL(PG_ERR_ARG, "replicas that alias their owner's prompt (pg_prefill_replicated, alias = 1) do not support lanes = 2");
    if (group_rows > 0 && !fuse_rope) FAIL(PG_ERR_ARG, "replicas that alias their owner's prompt need the fused decode attention (fuse_rope)");
    if (R % rpi) {
        if (dual) FAIL(PG_ERR_ARG, "dual-guidance decode needs a multiple of three rows (got %d)", R);
        FAIL(PG_ERR_ARG, "CFG decode needs an even number of rows (got %d)", R);
    }
    if (shared_len > 0 && !sp.shared_negative)
        FAIL(PG_ERR_STATE, "%s: the prefill shared the negative prompt across odd rows, which are not the negative rows of "
                           "triples; prefill with uncond_shared=False (the one-shot pg_set_option(\"uncond_shared_hint\", 0))", sp.name);
    if (n_dec_host != 0) FAIL(PG_ERR_STATE, "decode loop needs a fresh prefill");
    if (T < 1 || T - 1 > cfg.max_new) FAIL(PG_ERR_CAPACITY, "T=%d exceeds max_new=%d", T, cfg.max_new);
    if (max_len_host + T - 1 > slots) FAIL(PG_ERR_CAPACITY, "T=%d behind %d cached tokens (pg_prefill_extend) exceeds the %d KV slots", T, max_len_host, slots);
    if (max_pos_end() + T - 1 > max_pos) FAIL(PG_ERR_CAPACITY, "T=%d from position %d (pg_prefill_extend) exceeds the RoPE table (%d)", T, max_pos_end(), max_pos);
    if (hfin_stale) FAIL(PG_ERR_STATE, "%s after pg_rewind: a pg_prefill_extend must follow before anything samples", sp.name);
    const int B = R / rpi;
    if (score && q.lp_cap < (int64_t)B * T) FAIL(PG_ERR_ARG, "token log-probs: capacity %lld floats is below B * T = %lld", (long long)q.lp_cap, (long long)B * T);
    if (score && lanes_opt == 2) FAIL(PG_ERR_ARG, "token log-probs do not support lanes = 2");
    if (stats && q.ts.capacity < (int64_t)B * T) FAIL(PG_ERR_ARG, "token stats: capacity %lld positions is below B * T = %lld", (long long)q.ts.capacity, (long long)B * T);
    if (stats && lanes_opt == 2) FAIL(PG_ERR_ARG, "token stats do not support lanes = 2");
    if (plan && (plan_req.B != B || plan_req.T != T)) FAIL(PG_ERR_ARG, "sample plan: requested for B=%d, T=%d, the call has B=%d, T=%d", plan_req.B, plan_req.T, B, T);
    if (plan && lanes_opt == 2) FAIL(PG_ERR_ARG, "sample plans do not support lanes = 2");
    HIPCHK(hipSetDevice(dev));
    // the route of a planned call, from the host copies: filtered when any image is sampled with an active top-k / top-p
    bool plan_filtered = false;
    if (plan) {
        for (int b = 0; b < B; ++b) {
            const float tb = plan_req.temp.empty() ? temp : plan_req.temp[b];
            const int kb = plan_req.top_k.empty() ? top_k : plan_req.top_k[b];
            const float pb = plan_req.top_p.empty() ? top_p : plan_req.top_p[b];
            plan_filtered |= tb > 0.f && (kb > 0 || pb < 1.f);
        }
        if (plan_filtered && cfg.img_vocab > SEL_MAXV) FAIL(PG_ERR_ARG, "sample plan: a filtered image needs img_vocab <= %d (got %d)", SEL_MAXV, cfg.img_vocab);
    }
    TRY(reserve_requests(q));
    const bool stored = score || stats;                                   // the step also leaves the row the draw is made from in the row workspace
    // Lanes: at large batch the rows are split into two independent chains on two streams so one
    // half's latency-bound GEMM / norm kernels overlap the other half's bandwidth-bound attention.
    // CFG pairs never straddle lanes; results are lane-independent (global image index in the RNG).
    // Measured on MI355X at B=64: two lanes are 6 % SLOWER (kernels of both streams each fill the chip, the
    // weights are read twice) -> one lane unless asked for (pg_set_option "lanes").
    int nl = lanes_opt > 0 ? lanes_opt : 1;
    if (R % 4 || (long)decode_part_elems <= 0) nl = 1;
    const bool graph = use_graph && !time_attn && T > 2;
    // top-k / top-p only act on sampled draws (greedy ignores them, as HF's warpers do)
    const bool filtered = plan ? plan_filtered : temp > 0.f && (top_k > 0 || top_p < 1.f);
    if (filtered && !plan) {
        if (cfg.img_vocab > SEL_MAXV) FAIL(PG_ERR_CAPACITY, "top-k / top-p sampler supports img_vocab <= %d (got %d)", SEL_MAXV, cfg.img_vocab);
    }
    // cfg_mix is sized for max_rows / 2 images, which covers max_rows / 3
    if ((filtered || stored) && !cfg_mix) TRY(dalloc(&cfg_mix, (size_t)(cfg.max_rows / 2) * cfg.img_vocab * 4, false));
    // a lane is a view of its row range, built once: the loop writes no engine member (a second view is built, and unused, with one lane)
    DecodeView lane[2] = {view(0, nl == 2 ? R / 2 : R, 0), view(R / 2, R / 2, 1)};
    const int Hh = H(), G = cfg.gen_head_dim;
    if (force_mask && !force_tok) FAIL(PG_ERR_ARG, "force_mask needs force_tok");
    SampleArgs sa{};
    sa.bias = gh_b2; sa.V = cfg.img_vocab; sa.p = d_sparams;
    sa.force_tok = d_force_tok; sa.force_mask = d_force_mask; sa.out_tok = d_out_tok; sa.logits_out = logits_out;
    sa.embed_table = gen_table; sa.H = Hh; sa.B_total = B;
    const SamplePlanDev pd = plan ? plan_dev() : SamplePlanDev{};
    auto sample = [&](hipStream_t st, DecodeView& v) {
        tc_on = time_attn && (n_dec_host % (time_stride > 0 ? time_stride : 1)) == 0;
        tic(st);
        if (bf) head_logits<bf16>(st, v, (const bf16*)v.hfin, v.rows); else head_logits<float>(st, v, (const float*)v.hfin, v.rows);
        toc(st, TC_HEAD, ((double)G * Hh + (double)cfg.img_vocab * G) * (double)esz);
        sa.logits_partial = v.part; sa.S = v.S_last; sa.slab = v.slab_last; sa.x = v.x; sa.n_dec = v.d_ndec; sa.b_off = v.r0 / rpi;
        const int Bv = v.rows / rpi;
        tic(st);
        launch_cfg_step(st, sa, plan ? &pd : nullptr, d_dual, rpi, Bv, filtered, stored, v.cfg_pv, v.cfg_pi, v.cfg_mix);
        // the two reducers read the row, the token, T and the temperature (the plan's, with a plan): nothing pair-shaped
        if (plan) {
            SampleArgsPlan pa{}; static_cast<SampleArgs&>(pa) = sa; pa.plan = pd;
            if (score) launch_token_logprob_image_plan(st, pa, Bv, v.cfg_mix, d_logprob);
            if (stats) launch_token_stats_image_plan(st, pa, Bv, v.cfg_mix, stats_out(q.ts.n_alt));
        } else {
            if (score) launch_token_logprob_image(st, sa, Bv, v.cfg_mix, d_logprob);
            if (stats) launch_token_stats_image(st, sa, Bv, v.cfg_mix, stats_out(q.ts.n_alt));
        }
        toc(st, TC_SAMPLE, (double)v.S_last * v.rows * cfg.img_vocab * 4.0);
        tc_on = false;
    };
    if (time_attn) { tc_used = 0; tc_meta.clear(); }
    hipStream_t ws = s;
    if (graph || nl == 2) { TRY(hop_in(s)); ws = istream; }
    // one loop iteration for every lane: sample token i from hfin (step index = n_dec), then
    // (with_forward) run the stack on its embedding (appends KV slot len+n_dec) and advance n_dec.
    // In time_attn mode the lanes run back to back on one stream so the per-launch events are clean.
    const bool two_streams = nl == 2 && !time_attn;
    auto iteration = [&](bool with_forward) -> int {
        if (two_streams) { HIPCHK(hipEventRecord(ev_fork, ws)); HIPCHK(hipStreamWaitEvent(istream2, ev_fork, 0)); }
        for (int li = 0; li < nl; ++li) {
            hipStream_t st = (two_streams && li == 1) ? istream2 : ws;
            sample(st, lane[li]);
            if (with_forward) forward_decode(st, lane[li]);
        }
        if (two_streams) { HIPCHK(hipEventRecord(ev_join, istream2)); HIPCHK(hipStreamWaitEvent(ws, ev_join, 0)); }
        return PG_OK;
    };
    HIPCHK(hipEventRecord(ev_t0, ws));
    {   // per-call parameters and the caller's forcing tensors -> library-owned device memory (what the graph reads)
        SampleParams p{}; p.cfg_weight = sp.w; p.temperature = temp; p.seed = seed; p.T = T;
        p.has_force = force_tok != nullptr; p.has_mask = force_mask != nullptr; p.img_off = rng_image_offset;
        p.top_k = top_k; p.top_p = top_p;
        launch_set_sample_params(ws, d_sparams, p);
        if (dual) launch_set_dual_weights(ws, d_dual, DualWeights{sp.w, sp.w_layout});
        if (plan) HIPCHK(hipStreamWaitEvent(ws, ev_plan, 0));      // the request may have staged its arrays on another stream
        if (plan) launch_plan_fill(ws, pd, plan_req.mask, B, T, sp.w, temp, top_k, top_p, rng_image_offset);      // the arrays the plan left out
        if (force_tok) HIPCHK(hipMemcpyAsync(d_force_tok, force_tok, (size_t)B * T * 4, hipMemcpyDeviceToDevice, ws));
        if (force_mask) HIPCHK(hipMemcpyAsync(d_force_mask, force_mask, (size_t)B * T, hipMemcpyDeviceToDevice, ws));
    }
    TRY(iteration(T > 1));
    if (T > 1) n_dec_host++;
    int i = 1;
    if (graph) {
        // shapes and kernel selection only: seeds, temperatures, weights, T and the caller's buffers reach the kernels through
        // device memory, so a bench / serving loop replays ONE instantiated graph across calls
        std::vector<int64_t> key = {rpi,                         // pairs or triples: the same R never replays the other loop's step
                                    R, (int64_t)bf, (int64_t)logits_out, (int64_t)shared_len, (int64_t)fuse_rope, (int64_t)nl,
                                    (int64_t)(lpt_order && order_valid), (int64_t)tune_epoch, (int64_t)skip_attn, (int64_t)filtered,
                                    (int64_t)group_rows,         // replica geometry: never replay a graph across different aliasing
                                    (int64_t)score,              // the scored step holds two more launches
                                    (int64_t)(stats ? 1 + q.ts.n_alt : 0),       // the stats step one more (and the store, if score did not bring it)
                                    (int64_t)plan};              // a plan is present: the planned instantiations (its values come from device memory)
        for (; i < T - 1; ++i) { TRY(graph_step(gexec, gkey, key, ws, [&] { return iteration(true); })); n_dec_host++; }
    } else {
        for (; i < T - 1; ++i) { TRY(iteration(true)); n_dec_host++; }
    }
    if (T > 1) TRY(iteration(false));
    HIPCHK(hipMemcpyAsync(out_tok, d_out_tok, (size_t)B * T * 4, hipMemcpyDeviceToDevice, ws));
    if (score) HIPCHK(hipMemcpyAsync(q.lp_out, d_logprob, (size_t)B * T * 4, hipMemcpyDeviceToDevice, ws));
    if (stats) TRY(stats_copy_out(q.ts, B, T, T, ws));
    HIPCHK(hipEventRecord(ev_t1, ws));
    TRY(hop_out(ws, s));
    have_decode_t = true;
    HIPCHK(hipGetLastError());
    return PG_OK;
}
int pg_engine::decode_image(int T, float cfgw, float temp, int top_k, float top_p, uint64_t seed, const int32_t* force_tok,
                            const uint8_t* force_mask, int32_t* out_tok, float* logits_out, hipStream_t s) {
    return image_loop(ImageLoopSpec{"pg_decode_image_tokens", 2, cfgw, 0.f, true, true, true, true}, T, temp, top_k, top_p, seed, force_tok, force_mask,
                      out_tok, logits_out, s);
}
// pg_decode_image_tokens_dual: triples of rows (3b = caption + layout, 3b + 1 = caption only, 3b + 2 = negative); one lane, no plan, no shared or
// replicated prompts
int pg_engine::decode_image_dual(int T, float w_caption, float w_layout, float temp, int top_k, float top_p, uint64_t seed, const int32_t* force_tok,
                                 const uint8_t* force_mask, int32_t* out_tok, float* logits_out, hipStream_t s) {
    return image_loop(ImageLoopSpec{"pg_decode_image_tokens_dual", 3, w_caption, w_layout, false, false, false, false}, T, temp, top_k, top_p, seed,
                      force_tok, force_mask, out_tok, logits_out, s);
}

int pg_engine::step(const void* emb, int emb_dtype, void* hidden_out, int hidden_dtype, hipStream_t s) {
    if (!prefilled) FAIL(PG_ERR_STATE, "pg_step before pg_prefill");
    if (kv8 && !fuse_rope) FAIL(PG_ERR_ARG, "the FP8 KV cache needs the fused decode attention (fuse_rope)");
    if (group_rows > 0 && !fuse_rope) FAIL(PG_ERR_ARG, "replicas that alias their owner's prompt need the fused decode attention (fuse_rope)");
    if (n_dec_host + 1 > cfg.max_new) FAIL(PG_ERR_CAPACITY, "decode capacity max_new=%d exhausted", cfg.max_new);
    if (max_len_host + n_dec_host + 1 > slots) FAIL(PG_ERR_CAPACITY, "the %d KV slots are exhausted (%d cached tokens, pg_prefill_extend)", slots, max_len_host + n_dec_host);
    if (max_pos_end() + n_dec_host + 1 > max_pos) FAIL(PG_ERR_CAPACITY, "position %d (pg_prefill_extend) exceeds the RoPE table (%d)", max_pos_end() + n_dec_host, max_pos);
    HIPCHK(hipSetDevice(dev));
    DecodeView v = view(0, R, 0);
    launch_rows_to_f32(s, emb, emb_dtype == PG_BF16, nullptr, v.x, R, H());
    forward_decode(s, v);
    n_dec_host++;
    if (hidden_out) {
        if (bf) launch_t_to_rows<bf16>(s, (const bf16*)hfin, hidden_out, hidden_dtype == PG_BF16, nullptr, R, H());
        else launch_t_to_rows<float>(s, (const float*)hfin, hidden_out, hidden_dtype == PG_BF16, nullptr, R, H());
    }
    HIPCHK(hipGetLastError());
    return PG_OK;
}

int pg_engine::gen_head(const void* h_dev, int h_dtype, float* logits, int R_, hipStream_t s) {
    if (!finalized) FAIL(PG_ERR_STATE, "pg_finalize_weights not called");
    if (R_ < 1 || R_ > cfg.max_rows) FAIL(PG_ERR_CAPACITY, "rows %d > max_rows %d", R_, cfg.max_rows);
    HIPCHK(hipSetDevice(dev));
    DecodeView v = view(0, R_, 0);
    // bring h into the compute dtype
    if (bf) {
        if (h_dtype == PG_BF16) HIPCHK(hipMemcpyAsync(gh_in, h_dev, (size_t)R_ * H() * 2, hipMemcpyDeviceToDevice, s));
        else launch_t_to_rows<float>(s, (const float*)h_dev, gh_in, 1, nullptr, R_, H());
        head_logits<bf16>(s, v, (const bf16*)gh_in, R_);
    } else {
        launch_rows_to_f32(s, h_dev, h_dtype == PG_BF16, nullptr, (float*)gh_in, R_, H());
        head_logits<float>(s, v, (const float*)gh_in, R_);
    }
    launch_bias_f32(s, v.part, v.S_last, v.slab_last, gh_b2, logits, R_, cfg.img_vocab);
    HIPCHK(hipGetLastError());
    return PG_OK;
}

// pg_set_text_dfa: validate on the host, then stage the tables through pinned memory (no stream synchronisation: the staging buffer is
// guarded by an event, and refilled only after the previous upload's copies have left it).
int pg_engine::set_text_dfa(const pg_text_dfa* dfa, hipStream_t s) {
    if (!dfa) { dfa_set = false; return PG_OK; }
    const int ns = dfa->n_states, nc = dfa->n_classes, V = cfg.vocab;
    if (!dfa->token_class_host || !dfa->next_state_host || !dfa->dist_host) FAIL(PG_ERR_ARG, "pg_set_text_dfa: null table");
    if (ns < 1 || ns > TEXT_DFA_MAX_STATES || nc < 1 || nc > TEXT_DFA_MAX_CLASSES)
        FAIL(PG_ERR_ARG, "pg_set_text_dfa: n_states=%d / n_classes=%d outside 1..%d / 1..%d", ns, nc, TEXT_DFA_MAX_STATES, TEXT_DFA_MAX_CLASSES);
    if (dfa->start_state < 0 || dfa->start_state >= ns) FAIL(PG_ERR_ARG, "pg_set_text_dfa: start_state=%d outside [0, %d)", dfa->start_state, ns);
    std::vector<char> used(nc, 0);
    for (int v = 0; v < V; ++v) {
        const int c = dfa->token_class_host[v];
        if (c < 0 || c >= nc) FAIL(PG_ERR_ARG, "pg_set_text_dfa: token %d has class %d outside [0, %d)", v, c, nc);
        used[c] = 1;
    }
    for (int st = 0; st < ns; ++st) {
        // the builder's promise behind the budget rule: a state that can finish in dist tokens has a token that leads to dist - 1
        const int32_t dd = dfa->dist_host[st];
        if (dd < 0) FAIL(PG_ERR_ARG, "pg_set_text_dfa: dist[%d]=%d is negative", st, dd);
        bool down = dd == 0 || dd >= TEXT_DFA_INF;
        for (int c = 0; c < nc; ++c) {
            const int nx = dfa->next_state_host[(size_t)st * nc + c];
            if (nx < -1 || nx >= ns) FAIL(PG_ERR_ARG, "pg_set_text_dfa: next_state[%d][%d]=%d outside [-1, %d)", st, c, nx, ns);
            if (nx >= 0 && used[c] && dfa->dist_host[nx] <= dd - 1) down = true;
        }
        if (!down) FAIL(PG_ERR_ARG, "pg_set_text_dfa: dist[%d]=%d but no token leads to a state with dist <= %d", st, dd, dd - 1);
    }
    HIPCHK(hipSetDevice(dev));
    if (!ev_dfa) {           // first upload: the event is created last, so a failure part-way is retried from the start by the next call
        if (!d_dfa_class) TRY(dalloc(&d_dfa_class, (size_t)V * 2 + 16));
        if (!d_dfa_next) TRY(dalloc(&d_dfa_next, (size_t)TEXT_DFA_MAX_STATES * TEXT_DFA_MAX_CLASSES * 2));
        if (!d_dfa_dist) TRY(dalloc(&d_dfa_dist, (size_t)TEXT_DFA_MAX_STATES * 4));
        if (!d_dfa_hdr) TRY(dalloc(&d_dfa_hdr, 64));
        if (!d_dfa_state) TRY(dalloc(&d_dfa_state, (size_t)cfg.max_rows * 4));
        if (!d_op_tparams) TRY(dalloc(&d_op_tparams, 64));
        if (!d_op_step) TRY(dalloc(&d_op_step, 64));
        HIPCHK(hipStreamSynchronize(nullptr));               // dalloc's zero fills run on the NULL stream (this first call only)
        HIPCHK(hipEventCreateWithFlags(&ev_dfa, hipEventDisableTiming));
    }
    const size_t b_cls = ((size_t)V * 2 + 15) & ~(size_t)15, b_next = (((size_t)ns * nc * 2) + 15) & ~(size_t)15, b_dist = (size_t)ns * 4;
    const size_t need = b_cls + b_next + b_dist + sizeof(TextDfaHdr);
    if (dfa_staged) HIPCHK(hipEventSynchronize(ev_dfa));
    if (need > h_dfa_bytes) {
        if (h_dfa) { (void)hipHostFree(h_dfa); h_dfa = nullptr; h_dfa_bytes = 0; }
        HIPCHK(hipHostMalloc((void**)&h_dfa, need));
        h_dfa_bytes = need;
    }
    TextDfaHdr hd{ns, nc, dfa->start_state, 0};
    memcpy(h_dfa, dfa->token_class_host, (size_t)V * 2);
    memcpy(h_dfa + b_cls, dfa->next_state_host, (size_t)ns * nc * 2);
    memcpy(h_dfa + b_cls + b_next, dfa->dist_host, b_dist);
    memcpy(h_dfa + b_cls + b_next + b_dist, &hd, sizeof hd);
    HIPCHK(hipMemcpyAsync(d_dfa_class, h_dfa, (size_t)V * 2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_dfa_next, h_dfa + b_cls, (size_t)ns * nc * 2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_dfa_dist, h_dfa + b_cls + b_next, b_dist, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_dfa_hdr, h_dfa + b_cls + b_next + b_dist, sizeof hd, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ev_dfa, s));
    dfa_staged = true; dfa_set = true; dfa_dist_start = dfa->dist_host[dfa->start_state];
    return PG_OK;
}

// pg_op_text_constrain: the scan + pick pair of the constrained loop on caller-given rows and states
int pg_engine::text_constrain(const float* logits, int B, int V, const int32_t* state, int remaining, int eos, float temp, int top_k, float top_p,
                              uint64_t seed, int row_offset, int step, uint8_t* keep, int32_t* tok, int32_t* next_state, hipStream_t s) {
    if (!dfa_set) FAIL(PG_ERR_STATE, "pg_op_text_constrain: no automaton (pg_set_text_dfa)");
    if (B < 1 || B > cfg.max_rows || V < 1 || V > cfg.vocab) FAIL(PG_ERR_ARG, "pg_op_text_constrain: needs 1 <= B <= max_rows and 1 <= V <= vocab");
    if (top_k < 0 || !(top_p > 0.f && top_p <= 1.f) || remaining < 0 || step < 0)
        FAIL(PG_ERR_ARG, "pg_op_text_constrain: needs top_k >= 0, top_p in (0, 1], remaining >= 0, step >= 0");
    if (((uintptr_t)logits & 15) || ((uintptr_t)keep & 3)) FAIL(PG_ERR_ARG, "pg_op_text_constrain: logits_dev must be 16-byte and keep_dev 4-byte aligned");
    HIPCHK(hipSetDevice(dev));
    const int mode = !(temp > 0.f) ? 0 : ((top_k > 0 || top_p < 1.f) ? 2 : 1);
    if (mode == 2 && !txt_mix) { TRY(dalloc(&txt_mix, (size_t)cfg.max_rows * cfg.vocab * 4, false)); }
    TextParams tp{}; tp.eos = eos; tp.min_new = 0; tp.max_new = remaining + step;
    tp.temperature = temp; tp.top_k = top_k; tp.top_p = top_p; tp.seed = seed; tp.row_off = row_offset;
    launch_set_text_op_params(s, d_op_tparams, tp, d_op_step, step);
    TextArgs ta{};
    ta.logits_partial = logits; ta.S = 1; ta.slab = V; ta.V = V; ta.p = d_op_tparams; ta.n_dec = d_op_step;
    TextDfaArgs da{};
    da.token_class = d_dfa_class; da.next_state = d_dfa_next; da.dist = d_dfa_dist; da.hdr = d_dfa_hdr;
    da.state = state; da.state_out = next_state; da.keep = keep; da.tok = tok;
    const DecodeView v = view(0, B, 0);
    launch_text_constrained(s, ta, da, B, mode, v.cfg_pv, v.cfg_pi, txt_mix);
    HIPCHK(hipGetLastError());
    return PG_OK;
}

// pg_op_token_logprob: the loops' scoring kernel on caller-given rows and tokens
int pg_engine::token_logprob(const float* x, int B, int V, const int32_t* tok, float temp, float* out, hipStream_t s) {
    if (B < 1 || V < 1) FAIL(PG_ERR_ARG, "pg_op_token_logprob: needs B >= 1 and V >= 1 (got %d, %d)", B, V);
    if (((uintptr_t)x & 3) || ((uintptr_t)tok & 3) || ((uintptr_t)out & 3)) FAIL(PG_ERR_ARG, "pg_op_token_logprob: pointers must be 4-byte aligned");
    HIPCHK(hipSetDevice(dev));
    launch_token_logprob_op(s, x, B, V, tok, temp, out);
    HIPCHK(hipGetLastError());
    return PG_OK;
}

// pg_request_token_stats / pg_op_token_stats: what both refuse
const char* pg_engine::check_stats_request(const pg_token_stats* r) const {
    if (r->n_alt < 0 || r->n_alt > 8) return "n_alt must be in 0..8";
    if (r->capacity < 1) return "capacity must be >= 1";
    if (r->n_alt > 0 && (r->alt_tok_dev == nullptr) != (r->alt_logprob_dev == nullptr)) return "n_alt > 0 needs both alt_tok_dev and alt_logprob_dev, or neither";
    const bool alts = r->n_alt > 0 && r->alt_tok_dev;
    if (!r->logprob_dev && !r->entropy_dev && !r->rank_dev && !alts) return "no output requested";
    if (((uintptr_t)r->logprob_dev | (uintptr_t)r->entropy_dev | (uintptr_t)r->rank_dev | (uintptr_t)r->alt_tok_dev | (uintptr_t)r->alt_logprob_dev) & 3)
        return "pointers must be 4-byte aligned";
    return nullptr;
}

// the loop's library-owned results -> the caller's arrays: the first cols columns of every [B, pitch_cols] array (alternatives: x n_alt)
int pg_engine::stats_copy_out(const pg_token_stats& r, int B, int cols, int pitch_cols, hipStream_t s) {
    const TokenStatsOut o = stats_out(r.n_alt);
    auto copy = [&](void* dst, const void* src, size_t per) -> hipError_t {
        return hipMemcpy2DAsync(dst, (size_t)pitch_cols * per, src, (size_t)pitch_cols * per, (size_t)cols * per, B, hipMemcpyDeviceToDevice, s);
    };
    if (cols < 1) return PG_OK;
    if (r.logprob_dev) HIPCHK(copy(r.logprob_dev, o.logprob, 4));
    if (r.entropy_dev) HIPCHK(copy(r.entropy_dev, o.entropy, 4));
    if (r.rank_dev) HIPCHK(copy(r.rank_dev, o.rank, 4));
    if (r.n_alt > 0 && r.alt_tok_dev) {
        HIPCHK(copy(r.alt_tok_dev, o.alt_tok, (size_t)r.n_alt * 4));
        HIPCHK(copy(r.alt_logprob_dev, o.alt_logprob, (size_t)r.n_alt * 4));
    }
    return PG_OK;
}

// pg_op_token_stats: the loops' second reducer on caller-given rows and tokens
int pg_engine::token_stats(const float* x, int B, int V, const int32_t* tok, float temp, const pg_token_stats* out, hipStream_t s) {
    if (B < 1 || V < 1) FAIL(PG_ERR_ARG, "pg_op_token_stats: needs B >= 1 and V >= 1 (got %d, %d)", B, V);
    if (((uintptr_t)x & 3) || ((uintptr_t)tok & 3)) FAIL(PG_ERR_ARG, "pg_op_token_stats: pointers must be 4-byte aligned");
    if (const char* why = check_stats_request(out)) FAIL(PG_ERR_ARG, "pg_op_token_stats: %s", why);
    if (out->capacity < B) FAIL(PG_ERR_ARG, "pg_op_token_stats: capacity %lld is below B = %d", (long long)out->capacity, B);
    HIPCHK(hipSetDevice(dev));
    const bool alts = out->n_alt > 0 && out->alt_tok_dev;
    launch_token_stats_op(s, x, B, V, tok, temp, TokenStatsOut{out->logprob_dev, out->entropy_dev, out->rank_dev, out->alt_tok_dev, out->alt_logprob_dev, alts ? out->n_alt : 0});
    HIPCHK(hipGetLastError());
    return PG_OK;
}

// pg_score_tokens / pg_op_head_logprob: log softmax(x . w^T)[target] for n chosen rows.  bf16: the fused head (score_head.hip), only its
// (max, sum) partials touch HBM.  f32 (parity mode): the f32 GEMM + token_logprob_kernel over row chunks whose logits stay <= 64 MB.
int pg_engine::head_logprob(const char* who, const void* x, int64_t rows, const void* w, int V, int K, const int32_t* row_idx, const int32_t* target,
                            int64_t n, float temp, float* out, hipStream_t s) {
    if (!x || !w || !target || !out) FAIL(PG_ERR_ARG, "%s: null pointer", who);
    if (n < 1 || rows < 1 || V < 1 || n > (1L << 30)) FAIL(PG_ERR_ARG, "%s: needs 1 <= n <= 2^30, rows >= 1, V >= 1 (got n=%lld rows=%lld V=%d)", who, (long long)n, (long long)rows, V);
    if (K < 64 || K % 64) FAIL(PG_ERR_ARG, "%s: K=%d must be a positive multiple of 64 (the kernel's K step)", who, K);
    if (!row_idx && n > rows) FAIL(PG_ERR_ARG, "%s: n=%lld > rows=%lld without row_idx", who, (long long)n, (long long)rows);
    HIPCHK(hipSetDevice(dev));
    const long chunk = bf ? 0 : std::min<long>((long)n, std::max<long>(1, (64L << 20) / (4L * V)));
    const long need = bf ? (long)head_logprob_ws_bytes((long)n, V, K) : (((chunk * V * 4 + 255) & ~255L) + chunk * K * 4);
    sh_mid_bytes = 0;
    TRY(sh_reserve(need));
    if (bf) {
        if (!launch_head_logprob(s, (const bf16*)x, (const bf16*)w, row_idx, target, (long)n, V, K, temp, (float*)sh_ws, out)) FAIL(PG_ERR_ARG, "%s: shape not supported (n=%lld V=%d K=%d)", who, (long long)n, V, K);
    } else {
        float* logits = (float*)sh_ws;
        float* xg = (float*)((char*)sh_ws + ((chunk * V * 4 + 255) & ~255L));
        for (long r0 = 0; r0 < (long)n; r0 += chunk) {
            const int cn = (int)std::min<long>(chunk, (long)n - r0);
            const float* a = (const float*)x + r0 * K;
            if (row_idx) { launch_copy_rows(s, x, row_idx + r0, xg, nullptr, cn, (long)K * 4); a = xg; }
            GemmA ga; ga.ptr = a; ga.lda = K;
            GemmEpi e; e.out = logits; e.out_f32 = 1; e.ldc = V;
            launch_gemm<float>(s, ga, (const float*)w, K, 0, e, cn, V, K, 1);
            launch_token_logprob_op(s, logits, cn, V, target + r0, temp, out + r0);
        }
    }
    HIPCHK(hipGetLastError());
    return PG_OK;
}

// ---- scoring given images: the CFG-mixed gen_head (pg_score_image_tokens / pg_op_cfg_head_logprob)
// the scoring workspace holds at least ``need`` bytes afterwards (grown: the old one is freed; hipFree waits for the work that still reads it)
int pg_engine::sh_reserve(long need) {
    if (need <= sh_ws_bytes) return PG_OK;
    if (sh_ws) { HIPCHK(hipFree(sh_ws)); bytes -= sh_ws_bytes; sh_ws = nullptr; sh_ws_bytes = 0; }
    HIPCHK(hipMalloc(&sh_ws, (size_t)need));
    sh_ws_bytes = need; bytes += need;
    return PG_OK;
}
// bf16: the fused head's (max, sum) partials.  f32: one chunk of pairs -- its 2 * chunk logit rows (<= 64 MB) + its 2 * chunk gathered X rows
static long cfg_head_chunk(int64_t n, int V) { return std::min<long>((long)n, std::max<long>(1, (64L << 20) / (8L * V))); }
long pg_engine::cfg_head_need(int64_t n, int V, int K) const {
    if (bf) return (long)cfg_head_logprob_ws_bytes((long)n, V, K);
    const long chunk = cfg_head_chunk(n, V);
    return ((2 * chunk * V * 4 + 255) & ~255L) + 2 * chunk * K * 4;
}
// the head on operands already validated, in workspace ``ws`` (>= cfg_head_need bytes).  bf16: score_cfg_head.hip.  f32 (parity mode), per
// chunk of pairs: gather [cond rows | uncond rows] -> f32 GEMM -> cfg_mix_rows_kernel (bias + mix, in place) -> token_logprob_kernel
int pg_engine::cfg_head_run(const char* who, const void* x, const void* w, int V, int K, const float* bias, const int32_t* cond_idx, const int32_t* uncond_idx,
                            const int32_t* target, int64_t n, float cfgw, float temp, float* out, hipStream_t s, char* ws) {
    if (bf) {
        if (!launch_cfg_head_logprob(s, (const bf16*)x, (const bf16*)w, bias, cond_idx, uncond_idx, target, (long)n, V, K, cfgw, temp, (float*)ws, out))
            FAIL(PG_ERR_ARG, "%s: shape not supported (n=%lld V=%d K=%d)", who, (long long)n, V, K);
    } else {
        const long chunk = cfg_head_chunk(n, V);
        float* logits = (float*)ws;
        float* xg = (float*)(ws + ((2 * chunk * V * 4 + 255) & ~255L));
        for (long r0 = 0; r0 < (long)n; r0 += chunk) {
            const int cn = (int)std::min<long>(chunk, (long)n - r0);
            launch_copy_rows(s, x, cond_idx + r0, xg, nullptr, cn, (long)K * 4);
            launch_copy_rows(s, x, uncond_idx + r0, xg + (long)cn * K, nullptr, cn, (long)K * 4);
            GemmA ga; ga.ptr = xg; ga.lda = K;
            GemmEpi e; e.out = logits; e.out_f32 = 1; e.ldc = V;
            launch_gemm<float>(s, ga, (const float*)w, K, 0, e, 2 * cn, V, K, 1);
            launch_cfg_mix_rows(s, logits, bias, cn, V, cfgw);
            launch_token_logprob_op(s, logits, cn, V, target + r0, temp, out + r0);
        }
    }
    HIPCHK(hipGetLastError());
    return PG_OK;
}
static const char* cfg_head_args(const void* x, const void* w, const int32_t* ci, const int32_t* ui, const int32_t* t, const float* out, int64_t n, int64_t rows,
                                 int V, int K) {
    if (!x || !w || !ci || !ui || !t || !out) return "null pointer";
    if (n < 1 || rows < 1 || V < 1 || n > (1L << 29)) return "needs 1 <= n <= 2^29, rows >= 1, V >= 1";
    if (K < 64 || K % 64) return "K must be a positive multiple of 64 (the kernel's K step)";
    return nullptr;
}
int pg_engine::cfg_head_logprob(const char* who, const void* x, int64_t rows, const void* w, int V, int K, const float* bias, const int32_t* cond_idx,
                                const int32_t* uncond_idx, const int32_t* target, int64_t n, float cfgw, float temp, float* out, hipStream_t s) {
    if (const char* why = cfg_head_args(x, w, cond_idx, uncond_idx, target, out, n, rows, V, K))
        FAIL(PG_ERR_ARG, "%s: %s (got n=%lld rows=%lld V=%d K=%d)", who, why, (long long)n, (long long)rows, V, K);
    HIPCHK(hipSetDevice(dev));
    sh_mid_bytes = 0;
    TRY(sh_reserve(cfg_head_need(n, V, K)));
    return cfg_head_run(who, x, w, V, K, bias, cond_idx, uncond_idx, target, n, cfgw, temp, out, s, (char*)sh_ws);
}
// gen_head layer 1 (Linear + b1 -> GELU(erf), both in the large-M GEMM's epilogue; output in the compute dtype, as head_logits leaves it) over
// ALL ``rows`` of hidden -- no compaction: the index lists address the layer-1 output as they address hidden -- then the head on gh_w2 / gh_b2
int pg_engine::score_image_tokens(const void* hidden, int64_t rows, const int32_t* cond_idx, const int32_t* uncond_idx, const int32_t* target, int64_t n,
                                  float cfgw, float temp, float* out, hipStream_t s) {
    const char* who = "pg_score_image_tokens";
    const int Hh = H(), G = cfg.gen_head_dim, V = cfg.img_vocab;
    if (const char* why = cfg_head_args(hidden, gh_w2, cond_idx, uncond_idx, target, out, n, rows, V, G))
        FAIL(PG_ERR_ARG, "%s: %s (got n=%lld rows=%lld V=%d K=%d)", who, why, (long long)n, (long long)rows, V, G);
    if (rows > 0x7fffffffL / std::max(Hh, G)) FAIL(PG_ERR_ARG, "%s: rows=%lld x max(hidden, gen_head_dim) must stay below 2^31 elements", who, (long long)rows);
    HIPCHK(hipSetDevice(dev));
    const long mid_bytes = ((long)rows * G * (long)esz + 255) & ~255L;
    sh_mid_bytes = 0;
    TRY(sh_reserve(mid_bytes + cfg_head_need(n, V, G)));
    sh_mid_bytes = (long)rows * G * (long)esz;
    GemmA ga; ga.ptr = hidden; ga.lda = Hh;
    GemmEpi e; e.out = sh_ws; e.out_f32 = 0; e.ldc = G; e.bias_n = gh_b1; e.act = 1;
    if (bf) launch_gemm<bf16>(s, ga, (const bf16*)gh_w1, Hh, 0, e, (int)rows, G, Hh, 1);
    else launch_gemm<float>(s, ga, (const float*)gh_w1, Hh, 0, e, (int)rows, G, Hh, 1);
    return cfg_head_run(who, sh_ws, gh_w2, V, G, gh_b2, cond_idx, uncond_idx, target, n, cfgw, temp, out, s, (char*)sh_ws + mid_bytes);
}

int pg_engine::text_generate(int max_new, int min_new, int eos, float temp, int top_k, float top_p, uint64_t seed, int64_t* out, int* out_len,
                             float* logits_out, hipStream_t s, bool constrained, int32_t* state_out) {
    const TokenRequests q = take_requests();      // the one-shot log-prob and stats requests: consumed whatever this call answers
    const bool score = q.lp_out != nullptr, stats = q.stats;
    if (top_k < 0 || !(top_p > 0.f && top_p <= 1.f)) FAIL(PG_ERR_ARG, "top_k=%d must be >= 0 and top_p=%g in (0, 1]", top_k, (double)top_p);
    if (!prefilled) FAIL(PG_ERR_STATE, "text decode before pg_prefill");
    if (replicas_n > 1) FAIL(PG_ERR_STATE, "text decode after pg_prefill_replicated (position_mode 0, image sampling only)");
    if (kv8 && !fuse_rope) FAIL(PG_ERR_ARG, "the FP8 KV cache needs the fused decode attention (fuse_rope)");
    if (!cfg.with_lm_head) FAIL(PG_ERR_STATE, "engine created without lm_head");
    if (n_dec_host != 0) FAIL(PG_ERR_STATE, "text decode needs a fresh prefill");
    if (max_new < 1 || max_new > cfg.max_new || max_new > 1000) FAIL(PG_ERR_CAPACITY, "max_new=%d exceeds capacity %d", max_new, cfg.max_new);
    if (max_len_host + max_new - 1 > slots) FAIL(PG_ERR_CAPACITY, "max_new=%d behind %d cached tokens (pg_prefill_extend) exceeds the %d KV slots", max_new, max_len_host, slots);
    if (max_pos_end() + max_new - 1 > max_pos) FAIL(PG_ERR_CAPACITY, "max_new=%d from position %d (pg_prefill_extend) exceeds the RoPE table (%d)", max_new, max_pos_end(), max_pos);
    if (hfin_stale) FAIL(PG_ERR_STATE, "text decode after pg_rewind: a pg_prefill_extend must follow before anything samples");
    if (constrained) {
        if (!dfa_set) FAIL(PG_ERR_STATE, "constrained text decode without an automaton (pg_set_text_dfa)");
        if (dfa_dist_start > max_new) FAIL(PG_ERR_ARG, "max_new=%d is below dist[start_state]=%d: no row could finish", max_new, dfa_dist_start);
    }
    if (score && q.lp_cap < (int64_t)R * max_new) FAIL(PG_ERR_ARG, "token log-probs: capacity %lld floats is below B * max_new = %lld", (long long)q.lp_cap, (long long)R * max_new);
    if (stats && q.ts.capacity < (int64_t)R * max_new) FAIL(PG_ERR_ARG, "token stats: capacity %lld positions is below B * max_new = %lld", (long long)q.ts.capacity, (long long)R * max_new);
    HIPCHK(hipSetDevice(dev));
    const int B = R;
    TRY(reserve_requests(q));
    const bool stored = score || stats;                                   // the step also leaves the row the draw is made from in the row workspace
    // launch structure: greedy argmax (temperature <= 0 ignores the filters, as HF's warpers do) / Gumbel-max folded into the scan /
    // scan -> workspace -> select.  Everything else about sampling is a value in TextParams.
    const int mode = !(temp > 0.f) ? 0 : ((top_k > 0 || top_p < 1.f) ? 2 : 1);
    if ((mode == 2 || stored) && !txt_mix) TRY(dalloc(&txt_mix, (size_t)cfg.max_rows * cfg.vocab * 4, false));
    std::vector<int32_t> ones(B, 1);
    HIPCHK(hipMemcpyAsync(d_unf, ones.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_anyunf, 0, 1024 * 4, s));
    HIPCHK(hipStreamSynchronize(s));
    DecodeView v = view(0, R, 0);
    TextArgs ta{};
    ta.V = cfg.vocab; ta.p = d_tparams; ta.out = d_text_out; ta.unfinished = d_unf;
    ta.any_unfinished = d_anyunf; ta.embed_table = embed; ta.x = v.x; ta.H = H(); ta.n_dec = v.d_ndec; ta.logits_out = logits_out;
    std::vector<int32_t> flags(1024);
    int checked = 0, done_len = -1;
    // one step = lm_head GEMM -> argmax or draw / EOS bookkeeping (device step counter) -> the stack on the new
    // token's embedding.  Like the image loop it is captured once and replayed; every 8th step the
    // any-unfinished flags come back to the host (HF generate stops when every row has emitted EOS).
    hipStream_t ws = s;
    if (use_graph) { TRY(hop_in(s)); ws = istream; }
    {
        TextParams tp{}; tp.eos = eos; tp.min_new = min_new; tp.max_new = max_new;
        tp.temperature = temp; tp.top_k = top_k; tp.top_p = top_p; tp.seed = seed; tp.row_off = rng_image_offset;
        launch_set_text_params(ws, d_tparams, tp);
    }
    TextDfaArgs da{};
    if (constrained) {
        da.token_class = d_dfa_class; da.next_state = d_dfa_next; da.dist = d_dfa_dist; da.hdr = d_dfa_hdr;
        da.state = d_dfa_state; da.state_out = d_dfa_state;
        launch_text_dfa_reset(ws, d_dfa_state, d_dfa_hdr, B);
    }
    auto iteration = [&](bool with_forward) {
        if (bf) gemm_llm<bf16>(ws, v, (const bf16*)v.hfin, (const bf16*)lm_head, B, cfg.vocab, H(), true, lm_head_t);
        else gemm_llm<float>(ws, v, (const float*)v.hfin, (const float*)lm_head, B, cfg.vocab, H(), true);
        ta.logits_partial = v.part; ta.S = v.S_last; ta.slab = v.slab_last;
        // scored greedy / Gumbel-in-the-scan steps: the row goes to txt_mix first (mode 2 leaves it there anyway); the step's own scan follows
        if (stored && mode != 2) launch_text_store(ws, ta, constrained ? &da : nullptr, B, v.cfg_pv, v.cfg_pi, txt_mix);
        if (constrained) launch_text_constrained(ws, ta, da, B, mode, v.cfg_pv, v.cfg_pi, txt_mix);
        else if (mode == 2) launch_text_sample_filtered(ws, ta, B, v.cfg_pv, v.cfg_pi, txt_mix);
        else if (mode == 1) launch_text_sample(ws, ta, B, v.cfg_pv, v.cfg_pi);
        else launch_text_argmax(ws, ta, B, v.cfg_pv, v.cfg_pi);
        if (score) launch_token_logprob_text(ws, ta, B, txt_mix, d_logprob);
        if (stats) launch_token_stats_text(ws, ta, B, txt_mix, stats_out(q.ts.n_alt));
        if (with_forward) forward_decode(ws, v);
        return PG_OK;
    };
    for (int step_i = 0; step_i < max_new; ++step_i) {
        const bool last = step_i == max_new - 1;
        if (use_graph && !last && step_i > 0) {
            // shapes and kernel selection only: temperature, top_k, top_p, seed and the row offset reach the kernels through TextParams
            std::vector<int64_t> key = {R, (int64_t)bf, (int64_t)fuse_rope, (int64_t)shared_len, (int64_t)(lpt_order && order_valid), (int64_t)tune_epoch,
                                        (int64_t)mode, (int64_t)logits_out, (int64_t)constrained, (int64_t)score, (int64_t)(stats ? 1 + q.ts.n_alt : 0)};
            TRY(graph_step(gexec_txt, gkey_txt, key, ws, [&] { return iteration(true); }));
        } else {
            iteration(!last);
        }
        if (!last) n_dec_host++;
        if (last || (step_i & 7) == 7) {
            HIPCHK(hipMemcpyAsync(flags.data(), d_anyunf, 1024 * 4, hipMemcpyDeviceToHost, ws));
            HIPCHK(hipStreamSynchronize(ws));
            for (; checked <= step_i; ++checked)
                if (flags[(checked + 1) & 1023] == 0) { done_len = checked + 1; break; }
            if (done_len >= 0) break;
        }
    }
    if (done_len < 0) done_len = max_new;
    // only the columns this call produced; the caller's buffer keeps its own fill beyond them
    HIPCHK(hipMemcpy2DAsync(out, (size_t)max_new * 8, d_text_out, (size_t)max_new * 8, (size_t)done_len * 8, B, hipMemcpyDeviceToDevice, ws));
    if (score) HIPCHK(hipMemcpy2DAsync(q.lp_out, (size_t)max_new * 4, d_logprob, (size_t)max_new * 4, (size_t)done_len * 4, B, hipMemcpyDeviceToDevice, ws));
    if (stats) TRY(stats_copy_out(q.ts, B, done_len, max_new, ws));
    if (constrained && state_out) HIPCHK(hipMemcpyAsync(state_out, d_dfa_state, (size_t)B * 4, hipMemcpyDeviceToDevice, ws));
    TRY(hop_out(ws, s));
    if (out_len) *out_len = done_len;
    HIPCHK(hipGetLastError());
    return PG_OK;
}

