// On-device image pre-processing behind pg_preprocess_images (include/plangen_hip.h states the contract): the reference's
// VLMImageProcessor (image_processing_vlm.py:41-52,127-192) -- Pillow's 8-bit fixed-point bicubic resize to the target size, paste into
// a square canvas of the background colour, rescale and normalise through a caller-filled lookup table.  Integer arithmetic throughout,
// so the result equals Pillow + transformers bit for bit.
//
//   imgproc_coef_kernel    Pillow's precompute_coeffs + normalize_coeffs_8bpc per image and axis, one thread per output index, in fp64
//                          with contraction off (add / multiply / divide / truncate are IEEE on gfx950: the doubles are the ones x86 computes)
//   imgproc_h_kernel       horizontal pass: a block owns IP_RB source rows x <= IP_TX output pixels, stages the source span it needs in LDS
//                          with dword loads, one thread per output byte (pixel, channel)        -> uint8 [h][ow][3]
//   imgproc_v_kernel       vertical pass: a thread owns 4 consecutive bytes of IP_RY output rows (one dword load per tap; the tap
//                          coefficients are uniform across the block)                           -> uint8 [oh][ow][3]
//   imgproc_finish_kernel  every element of [B, 3, S, S]: canvas or resized pixel -> lut[c][v] -> fp32 / bf16
// The intermediate between the passes is uint8 as in Pillow (ImagingResampleHorizontal_8bpc / Vertical_8bpc): its rounding and
// clamping are part of the result.  A pass whose size does not change is skipped (its blocks return), as Pillow skips it.
#include "engine.h"

#pragma clang fp contract(off)

#define IP_PREC 22                      // Pillow's PRECISION_BITS for 8-bit images
#define IP_TX 64                        // output pixels per block of the horizontal pass (fewer when the source span would not fit)
#define IP_RB 4                         // source rows per block of the horizontal pass
#define IP_SPAN 8192                    // bytes of one source-row span in LDS
#define IP_RY 4                         // output rows per block of the vertical pass
#define IP_MAX_RATIO 64.0               // down-scaling limit per axis: caps the taps per output at 2 * 128 + 1
#define IP_MAX_OUT 16384

struct ImgDesc {
    const uint8_t* pix; int64_t stride;         // source: uint8 HWC, rows `stride` bytes apart
    int32_t h, w, oh, ow;                       // source and resized size
    int32_t px, py;                             // where the resized image sits in the S x S canvas
    int32_t ksx, ksy;                           // table row length (Pillow's ksize) per axis; 0: pass skipped
    int32_t tx;                                 // output pixels per horizontal block
    int32_t rs;                                 // row stride of both uint8 intermediates (ow * 3 rounded up to 4)
    int64_t cx, cy;                             // int32 offsets of the axis tables: bounds [out][2] = (xmin, n), then coefficients [out][ks]
    int64_t t1, t2;                             // byte offsets of the intermediates in the workspace (multiples of 16)
};

__device__ __forceinline__ double ip_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// grid (ceil(S / 64), 2 axes, images)
__global__ __launch_bounds__(64) void imgproc_coef_kernel(const ImgDesc* __restrict__ descs, int32_t* __restrict__ tab, int b0) {
    const ImgDesc d = descs[b0 + blockIdx.z];
    const int axis = blockIdx.y;
    const int in = axis ? d.h : d.w, out = axis ? d.oh : d.ow, ks = axis ? d.ksy : d.ksx;
    const int xx = blockIdx.x * 64 + threadIdx.x;
    if (ks == 0 || xx >= out) return;
    int32_t* bounds = tab + (axis ? d.cy : d.cx);
    int32_t* k = bounds + 2 * (long)out + (long)xx * ks;
    const double scale = (double)in / (double)out;
    double fs = scale;
    if (fs < 1.0) fs = 1.0;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double c = (xx + 0.5) * scale;
    int xmin = (int)(c - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(c + support + 0.5);
    if (xmax > in) xmax = in;
    int n = xmax - xmin;
    if (n > ks) n = ks;                         // cannot happen (ks = ceil(support) * 2 + 1); keeps the stores inside the row
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += ip_bicubic((x + xmin - c + 0.5) * ss);
    for (int x = 0; x < n; ++x) {
        double w = ip_bicubic((x + xmin - c + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << IP_PREC)) : (int)(0.5 + w * (double)(1 << IP_PREC));
    }
    bounds[2 * xx] = xmin; bounds[2 * xx + 1] = n;
}

__device__ __forceinline__ uint32_t ip_clip8(int acc) {
    const int v = acc >> IP_PREC;               // arithmetic shift
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
// four bytes at p, of which only those inside [lo, hi) are read (the others come back as 0)
__device__ __forceinline__ uint32_t ip_load4(const uint8_t* p, const uint8_t* lo, const uint8_t* hi, bool word_ok) {
    if (word_ok && p >= lo && p + 4 <= hi) return *(const uint32_t*)p;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (p + i >= lo && p + i < hi) v |= (uint32_t)p[i] << (8 * i);
    return v;
}

// grid (row groups, x chunks, images)
__global__ __launch_bounds__(256) void imgproc_h_kernel(const ImgDesc* __restrict__ descs, const int32_t* __restrict__ tab, uint8_t* __restrict__ ws, int b0) {
    __shared__ uint32_t span[IP_RB][IP_SPAN / 4 + 2];
    const ImgDesc d = descs[b0 + blockIdx.z];
    if (d.ksx == 0) return;
    const int r0 = blockIdx.x * IP_RB, x0 = blockIdx.y * d.tx;
    if (r0 >= d.h || x0 >= d.ow) return;
    const int x1 = min(x0 + d.tx, d.ow), tid = threadIdx.x;
    const int32_t* bounds = tab + d.cx;
    const int32_t* coef = bounds + 2 * (long)d.ow;
    // xmin and xmin + n never decrease with the output index: the chunk reads source pixels [lo, hi)
    const int lo = bounds[2 * x0], hi = bounds[2 * (x1 - 1)] + bounds[2 * (x1 - 1) + 1];
    const int nbytes = (hi - lo) * 3;
    if (nbytes > IP_SPAN) return;               // the host sizes tx so that this cannot happen
    int sh[IP_RB];
#pragma unroll
    for (int r = 0; r < IP_RB; ++r) {
        sh[r] = 0;
        if (r0 + r >= d.h) continue;
        const uint8_t* row = d.pix + (int64_t)(r0 + r) * d.stride;
        const uint8_t* a = row + (long)lo * 3;
        sh[r] = (int)((uintptr_t)a & 3);
        const uint8_t* al = a - sh[r];          // dword-aligned; bytes outside the row are never read
        const int nd = (sh[r] + nbytes + 3) >> 2;
        for (int i = tid; i < nd; i += 256) span[r][i] = ip_load4(al + 4 * i, row, row + (long)d.w * 3, true);
    }
    __syncthreads();
    if (tid >= (x1 - x0) * 3) return;
    const int xx = x0 + tid / 3, ch = tid % 3;
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const int32_t* k = coef + (long)xx * d.ksx;
    int acc[IP_RB];
    const uint8_t* sp[IP_RB];
#pragma unroll
    for (int r = 0; r < IP_RB; ++r) { acc[r] = 1 << (IP_PREC - 1); sp[r] = (const uint8_t*)span[r] + sh[r] + (xmin - lo) * 3 + ch; }
    for (int t = 0; t < n; ++t) {
        const int kv = k[t];
#pragma unroll
        for (int r = 0; r < IP_RB; ++r) acc[r] += (int)sp[r][3 * t] * kv;
    }
    uint8_t* o = ws + d.t1 + (long)r0 * d.rs + (long)xx * 3 + ch;
#pragma unroll
    for (int r = 0; r < IP_RB; ++r) if (r0 + r < d.h) o[(long)r * d.rs] = (uint8_t)ip_clip8(acc[r]);
}

// grid (ceil(rs / 1024), ceil(oh / IP_RY), images)
__global__ __launch_bounds__(256) void imgproc_v_kernel(const ImgDesc* __restrict__ descs, const int32_t* __restrict__ tab, uint8_t* __restrict__ ws, int b0) {
    const ImgDesc d = descs[b0 + blockIdx.z];
    if (d.ksy == 0) return;
    const int y0 = blockIdx.y * IP_RY, j = (blockIdx.x * 256 + threadIdx.x) * 4, rowbytes = d.ow * 3;
    if (y0 >= d.oh || j >= rowbytes) return;
    // source: the horizontal pass's output, or the image itself when that pass was skipped (ow == w)
    const bool from_ws = d.ksx != 0;
    const uint8_t* base = from_ws ? ws + d.t1 : d.pix;
    const int64_t sstride = from_ws ? d.rs : d.stride;
    const bool word_ok = (((uintptr_t)base | (uintptr_t)sstride) & 3) == 0;
    const int32_t* bounds = tab + d.cy;
    const int32_t* coef = bounds + 2 * (long)d.oh;
    for (int yy = y0; yy < min(y0 + IP_RY, d.oh); ++yy) {
        const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
        const int32_t* k = coef + (long)yy * d.ksy;
        int acc[4] = {1 << (IP_PREC - 1), 1 << (IP_PREC - 1), 1 << (IP_PREC - 1), 1 << (IP_PREC - 1)};
        for (int t = 0; t < n; ++t) {
            const uint8_t* row = base + (int64_t)(ymin + t) * sstride;
            const uint32_t v = ip_load4(row + j, row, row + rowbytes, word_ok);
            const int kv = k[t];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] += (int)((v >> (8 * i)) & 255u) * kv;
        }
        uint8_t* o = ws + d.t2 + (long)yy * d.rs + j;           // rs is a multiple of 4: the whole dword lies inside the row's slot
        *(uint32_t*)o = ip_clip8(acc[0]) | (ip_clip8(acc[1]) << 8) | (ip_clip8(acc[2]) << 16) | (ip_clip8(acc[3]) << 24);
    }
}

// grid (ceil(S / 256), S, images): one thread per canvas pixel, three planes
__global__ __launch_bounds__(256) void imgproc_finish_kernel(const ImgDesc* __restrict__ descs, const uint8_t* __restrict__ ws, const float* __restrict__ lut,
                                                            const uint8_t* __restrict__ bg, void* __restrict__ out, int S, int out_bf16, int b0) {
    __shared__ float s_lut[768];
    for (int i = threadIdx.x; i < 768; i += 256) s_lut[i] = lut[i];
    __syncthreads();
    const int b = b0 + blockIdx.z;
    const ImgDesc d = descs[b];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= S) return;
    uint32_t v[3] = {bg[0], bg[1], bg[2]};
    const int ix = x - d.px, iy = y - d.py;
    if (ix >= 0 && ix < d.ow && iy >= 0 && iy < d.oh) {
        const uint8_t* p = d.ksy ? ws + d.t2 + (long)iy * d.rs : d.ksx ? ws + d.t1 + (long)iy * d.rs : d.pix + (int64_t)iy * d.stride;
        p += (long)ix * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = s_lut[c * 256 + v[c]];
        const long o = (((long)b * 3 + c) * S + y) * S + x;
        if (out_bf16) ((uint16_t*)out)[o] = (uint16_t)f32_to_bf16_bits(f);
        else ((float*)out)[o] = f;
    }
}

static inline long ip_up(long v, long a) { return (v + a - 1) / a * a; }

int pg_engine::preprocess_images(const pg_image_u8* images, int B, int S, int min_size, const uint8_t* background, const float* lut_host,
                                 void* out_dev, int out_dtype, hipStream_t s) {
    if (!images || !background || !lut_host || !out_dev) FAIL(PG_ERR_ARG, "pg_preprocess_images: null argument");
    if (B < 1) FAIL(PG_ERR_ARG, "pg_preprocess_images: B = %d < 1", B);
    if (min_size < 1 || S < min_size || S > IP_MAX_OUT) FAIL(PG_ERR_ARG, "pg_preprocess_images: needs 1 <= min_size <= out_size <= %d", IP_MAX_OUT);
    if (out_dtype != PG_F32 && out_dtype != PG_BF16) FAIL(PG_ERR_ARG, "pg_preprocess_images: out_dtype must be PG_F32 or PG_BF16");
    // ---- plan every image on the host (nothing is launched before the whole batch is known to be valid)
    const long head_bytes = ip_up((long)B * (long)sizeof(ImgDesc), 16) + 768 * 4 + 16;
    std::vector<ImgDesc> ds((size_t)B);
    long tab_n = 0, ws_n = 0;
    int g_rows = 1, g_chunks = 1, g_v = 1, g_oh = 1; bool any_h = false, any_v = false;
    for (int b = 0; b < B; ++b) {
        const pg_image_u8& im = images[b];
        ImgDesc& d = ds[b];
        if (!im.pix_dev) FAIL(PG_ERR_ARG, "pg_preprocess_images: image %d has a null pointer", b);
        if (im.height < 1 || im.width < 1) FAIL(PG_ERR_ARG, "pg_preprocess_images: image %d is %d x %d", b, im.height, im.width);
        d.pix = im.pix_dev; d.stride = im.row_stride; d.h = im.height; d.w = im.width;
        // VLMImageProcessor.resize (image_processing_vlm.py:137-143): divide, multiply, truncate, in double
        const int m = std::max(d.h, d.w);
        d.oh = std::max((int)((double)d.h / (double)m * (double)S), min_size);
        d.ow = std::max((int)((double)d.w / (double)m * (double)S), min_size);
        const double sx = (double)d.w / (double)d.ow, sy = (double)d.h / (double)d.oh;
        if (sx > IP_MAX_RATIO || sy > IP_MAX_RATIO)
            FAIL(PG_ERR_ARG, "pg_preprocess_images: image %d (%d x %d -> %d x %d) is scaled down by more than %d on an axis", b, d.h, d.w, d.oh, d.ow, (int)IP_MAX_RATIO);
        // expand2square (:41-52): the longer side is S (h / m is exactly 1 there), the shorter one is centred with the odd pixel after it
        d.px = d.ow < d.oh ? (S - d.ow) / 2 : 0; d.py = d.oh < d.ow ? (S - d.oh) / 2 : 0;
        d.ksx = d.ow != d.w ? (int)ceil(2.0 * std::max(sx, 1.0)) * 2 + 1 : 0;
        d.ksy = d.oh != d.h ? (int)ceil(2.0 * std::max(sy, 1.0)) * 2 + 1 : 0;
        // a chunk of tx outputs reads at most (tx - 1) * scale + 2 * support + 1 source pixels
        const double room = IP_SPAN / 3 - 4.0 * std::max(sx, 1.0) - 2.0;
        d.tx = (int)std::min((double)IP_TX, std::max(1.0, floor(room / sx) + 1.0));
        d.rs = (int)ip_up((long)d.ow * 3, 4);
        d.cx = tab_n; if (d.ksx) tab_n += (long)d.ow * (2 + d.ksx);
        d.cy = tab_n; if (d.ksy) tab_n += (long)d.oh * (2 + d.ksy);
        d.t1 = ws_n; if (d.ksx) ws_n += ip_up((long)d.h * d.rs, 16);
        d.t2 = ws_n; if (d.ksy) ws_n += ip_up((long)d.oh * d.rs, 16);
        if (d.ksx) { any_h = true; g_rows = std::max(g_rows, (d.h + IP_RB - 1) / IP_RB); g_chunks = std::max(g_chunks, (d.ow + d.tx - 1) / d.tx); }
        if (d.ksy) { any_v = true; g_v = std::max(g_v, (d.rs + 1023) / 1024); g_oh = std::max(g_oh, (d.oh + IP_RY - 1) / IP_RY); }
    }
    (void)hipSetDevice(dev);
    // ---- library-owned device workspace: [descriptors | lut | background] [coefficient tables] [uint8 intermediates]; grows when needed
    const long tab_off = ip_up(head_bytes, 256), ws_off = tab_off + ip_up(tab_n * 4, 256), need = ws_off + ip_up(ws_n, 256);
    if (need > ip_dev_bytes) {
        if (ip_dev) { HIPCHK(hipFree(ip_dev)); bytes -= ip_dev_bytes; ip_dev = nullptr; ip_dev_bytes = 0; }   // hipFree waits for the work that still reads it
        HIPCHK(hipMalloc(&ip_dev, (size_t)need));
        ip_dev_bytes = need; bytes += need;
    }
    // ---- descriptors, table and background travel through pinned staging, double-buffered like pg_prefill's row metadata
    ip_sel ^= 1;
    if (ip_used[ip_sel]) HIPCHK(hipEventSynchronize(ip_ev[ip_sel]));
    if (!ip_ev[ip_sel]) HIPCHK(hipEventCreateWithFlags(&ip_ev[ip_sel], hipEventDisableTiming));
    if (head_bytes > ip_host_bytes[ip_sel]) {
        if (ip_host[ip_sel]) { HIPCHK(hipHostFree(ip_host[ip_sel])); ip_host[ip_sel] = nullptr; ip_host_bytes[ip_sel] = 0; }
        HIPCHK(hipHostMalloc((void**)&ip_host[ip_sel], (size_t)head_bytes));
        ip_host_bytes[ip_sel] = head_bytes;
    }
    uint8_t* hs = ip_host[ip_sel];
    const long lut_off = ip_up((long)B * (long)sizeof(ImgDesc), 16), bg_off = lut_off + 768 * 4;
    memcpy(hs, ds.data(), (size_t)B * sizeof(ImgDesc));
    memcpy(hs + lut_off, lut_host, 768 * 4);
    memset(hs + bg_off, 0, 16); memcpy(hs + bg_off, background, 3);
    HIPCHK(hipMemcpyAsync(ip_dev, hs, (size_t)head_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ip_ev[ip_sel], s));
    ip_used[ip_sel] = true;
    const ImgDesc* dd = (const ImgDesc*)ip_dev;
    int32_t* tab = (int32_t*)((char*)ip_dev + tab_off);
    uint8_t* ws = (uint8_t*)ip_dev + ws_off;
    for (int b0 = 0; b0 < B; b0 += 32768) {         // gridDim.z
        const int nb = std::min(B - b0, 32768);
        if (any_h || any_v) hipLaunchKernelGGL(imgproc_coef_kernel, dim3((S + 63) / 64, 2, nb), dim3(64), 0, s, dd, tab, b0);
        if (any_h) hipLaunchKernelGGL(imgproc_h_kernel, dim3(g_rows, g_chunks, nb), dim3(256), 0, s, dd, (const int32_t*)tab, ws, b0);
        if (any_v) hipLaunchKernelGGL(imgproc_v_kernel, dim3(g_v, g_oh, nb), dim3(256), 0, s, dd, (const int32_t*)tab, ws, b0);
        hipLaunchKernelGGL(imgproc_finish_kernel, dim3((S + 255) / 256, S, nb), dim3(256), 0, s, dd, (const uint8_t*)ws, (const float*)((char*)ip_dev + lut_off),
                           (const uint8_t*)ip_dev + bg_off, out_dev, S, out_dtype == PG_BF16 ? 1 : 0, b0);
    }
    if (hipGetLastError() != hipSuccess) FAIL(PG_ERR_HIP, "pg_preprocess_images: kernel launch failed");
    return PG_OK;
}
