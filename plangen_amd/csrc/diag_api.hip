// libplangen_diag.so only: the switches that do NOT belong in the product library -- measurement modes whose results are garbage by
// construction (skip_attn, attn_variant 101-107), kernel-form selectors of the sweeps (attn_variant 100, attn_waves, split_target_small
// / _mid), and A/B switches of settled questions (fuse_rope, force_swiglu, lpt_order).  libplangen_diag.so is a
// SUPERSET build: the same object files as libplangen_hip.so plus diag_*.o / bench_kernels.o / chain.o, so a handle created through it
// runs exactly the product's code until one of these is set.  tools/, bench.py's instrumented pass and the hazard-screen tests use it.
#include "engine.h"
#include "diag.h"

extern "C" {

int pg_diag_set_option(pg_handle h, const char* key, int64_t value) {
    if (!h || !key) return PG_ERR_ARG;
    h->tune.diag = diag_hooks();
    if (!strcmp(key, "skip_attn")) { h->skip_attn = value != 0; return PG_OK; }          // MEASUREMENT ONLY: decode steps without their attention launches
    if (!strcmp(key, "attn_variant")) { h->tune.attn_variant = (int)value; h->tune_epoch++; return PG_OK; }
    if (!strcmp(key, "attn_waves")) { h->tune.attn_waves = (int)value; h->tune_epoch++; return PG_OK; }
    if (!strcmp(key, "split_target_small")) { h->tune.split_small = (int)value; h->tune_epoch++; return PG_OK; }
    if (!strcmp(key, "split_target_mid")) { h->tune.split_mid = (int)value; h->tune_epoch++; return PG_OK; }
    if (!strcmp(key, "gn_epilogue256")) { h->tune.gn_epilogue256 = value != 0; return PG_OK; }      // GroupNorm partials from the 256x256 conv epilogue (measured slower, profiles/r06_c)
    if (!strcmp(key, "defer_norm")) { h->defer_norm = value != 0; h->tune_epoch++; return PG_OK; }      // 0: rmsnorm512 + plain GEMMs at 65..128 rows too (round-5 arithmetic; bf16 rounding differs)
    if (!strcmp(key, "fuse_rope")) { h->fuse_rope = value != 0; h->tune_epoch++; return PG_OK; }
    if (!strcmp(key, "force_swiglu")) { h->force_swiglu = value != 0; h->tune_epoch++; return PG_OK; }
    if (!strcmp(key, "lpt_order")) { h->lpt_order = value != 0; h->tune_epoch++; return PG_OK; }
    h->err = std::string("unknown diagnostics option ") + key;
    return PG_ERR_ARG;
}

// Copy one weight buffer of a handle, in its DEVICE layout, into dst_dev (device to device, at most max_bytes; synchronous).  info_out[3] = {elements, bytes per
// element, kind}.  name is
//   * a state-dict name the handle accepts (without the vl_gpt. prefix): that slot's own destination range -- q / k / v_proj are the thirds of wqkv, a K_CONV slot
//     is [Cout][tap][Cin]; kind = its SlotKind (K_T 0, K_F32 1, K_IL16_G 2, K_IL16_U 3, K_CONV 4).  gate_proj and up_proj share ONE interleaved destination: both
//     names give the whole [2 I][H] buffer (elements = 2 I H);
//   * a buffer pg_finalize_weights derives (kind 100): "layers.<i>.wqkv_t" / ".wo_t" / ".wgu_t" / ".wd_t" (the decode-tiled copies) and "layers.<i>.wqkv_p" (the
//     [8 | 8] rotary interleave of the prefill epilogue), "gh_w1_t", "gh_w2_t", "lm_head_t", all bf16; "cos_t" / "sin_t", fp32 [max_pos][64].
// (gen_table and pq_table: pg_debug_read.)  PG_ERR_NAME: no such name.  PG_ERR_STATE: a derived buffer this handle does not hold -- an fp32 handle has no tiled
// copies, tile_one skips a shape it cannot tile, wqkv_p exists only when the handle's capacity can reach the fused prefill epilogue, and before the first
// pg_finalize_weights nothing is derived (cos_t / sin_t exist from creation and read as zeros until then); info_out is filled (elements as if it existed) and nothing is copied.
int pg_diag_read_weight(pg_handle h, const char* name, void* dst_dev, int64_t max_bytes, int64_t* info_out) {
    if (!h || !name || !dst_dev || !info_out || max_bytes < 0) return PG_ERR_ARG;
    const std::string nm = name;
    const void* src = nullptr; int64_t n = 0, es = 0, kind = 100;
    const int Hh = h->H(), I = h->cfg.inter, HDm = h->HD();
    auto it = h->slots_map.find(nm);
    if (it != h->slots_map.end()) {
        const Slot& sl = it->second;
        src = sl.dst; kind = sl.kind; es = sl.kind == K_F32 ? 4 : (int64_t)h->esz;
        n = sl.kind == K_IL16_G || sl.kind == K_IL16_U ? 2 * sl.n : sl.n;
    } else if (nm.rfind("layers.", 0) == 0) {
        char* end = nullptr;
        const long li = strtol(nm.c_str() + 7, &end, 10);
        if (end == nm.c_str() + 7 || *end != '.' || li < 0 || li >= (long)h->layers.size()) { h->err = "pg_diag_read_weight: unknown buffer " + nm; return PG_ERR_NAME; }
        const pg_engine::Layer& ly = h->layers[li];
        const std::string f = end + 1;
        es = 2;
        if (f == "wqkv_t") { src = ly.wqkv_t; n = 3L * HDm * Hh; }
        else if (f == "wo_t") { src = ly.wo_t; n = (int64_t)Hh * HDm; }
        else if (f == "wgu_t") { src = ly.wgu_t; n = 2L * I * Hh; }
        else if (f == "wd_t") { src = ly.wd_t; n = (int64_t)Hh * I; }
        else if (f == "wqkv_p") { src = ly.wqkv_p; n = 3L * HDm * Hh; }
        else { h->err = "pg_diag_read_weight: unknown buffer " + nm; return PG_ERR_NAME; }
    }
    else if (nm == "gh_w1_t") { src = h->gh_w1_t; n = (int64_t)h->cfg.gen_head_dim * Hh; es = 2; }
    else if (nm == "gh_w2_t") { src = h->gh_w2_t; n = (int64_t)h->cfg.img_vocab * h->cfg.gen_head_dim; es = 2; }
    else if (nm == "lm_head_t") { src = h->lm_head_t; n = (int64_t)h->cfg.vocab * Hh; es = 2; }
    else if (nm == "cos_t") { src = h->cos_t; n = (int64_t)h->max_pos * 64; es = 4; }
    else if (nm == "sin_t") { src = h->sin_t; n = (int64_t)h->max_pos * 64; es = 4; }
    else { h->err = "pg_diag_read_weight: unknown buffer " + nm; return PG_ERR_NAME; }
    info_out[0] = n; info_out[1] = es; info_out[2] = kind;
    if (!src) { h->err = "pg_diag_read_weight: this handle holds no " + nm; return PG_ERR_STATE; }
    int64_t bytes = n * es;
    if (bytes > max_bytes) bytes = max_bytes;
    if (hipSetDevice(h->dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(dst_dev, src, (size_t)bytes, hipMemcpyDeviceToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        h->err = "pg_diag_read_weight: copy failed"; return PG_ERR_HIP;
    }
    return PG_OK;
}

}  // extern "C"
