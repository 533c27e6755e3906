// PIL's 8-bit antialiased resize (Pillow src/libImaging/Resample.c: ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc), a crop window and a
// per-channel affine in ONE launch: image file bytes -> the `pixel_values` of the CLIP towers and the VAE.  What it replaces: open_clip's preprocess_train
// (Resize(224, BICUBIC), CenterCrop, ToTensor, Normalize: eegdatasets_leaveone.py:62-74's ImageEncoder input), transformers' CLIPImageProcessor (the
// IP-Adapter's feature_extractor, GIT's processor) and the low-level script's Resize((512, 512)) in front of the VAE.
//
//   resize_coeffs (host only)   PIL's precompute_coeffs + normalize_coeffs_8bpc in double for output indices first .. first + count - 1 of one axis: bounds
//                               (xmin, n) and ksize int32 fixed-point coefficients (22 fractional bits) per output index.  Only the rows / columns of the crop
//                               window are computed: that is the crop.
//   resize_crop_normalize       grid (column tiles, row tiles, B), 256 threads, one TH x TW output tile of one image per workgroup:
//       1. the tile's coefficient rows and bounds -> LDS (bounds clamped into the image, so that no table can make the kernel read outside it);
//       2. horizontal pass over every input row the tile's vertical taps span (first row's ymin .. last row's ymin + n): source bytes from global memory,
//          lanes along the tile's columns (neighbouring lanes read neighbouring bytes of one row), t = clip8((2^21 + sum k p) >> 22) as uint8 into the LDS
//          strip [row][channel][column];
//       3. vertical pass over the strip, the same arithmetic, then q * scale[c] + shift[c] in fp32 (two roundings, no fma: -ffp-contract=off), one rounding to
//          the output type; lanes along the output row.
//   The intermediate never reaches HBM; no atomics, no memset, results do not depend on the tiling.  int32 sums: 2^21 + 255 sum|k| <= 2^21 + 255 * 1.25 * 2^22
//   + ksize rounding units < 1.35e9 for both filters at every scale (the bicubic's |w| sums to at most 1.25 after normalisation).
//
//   Tile: 16 rows x 64 columns; smaller (down to 4 x 16) while there are fewer workgroups than CUs (the loop in the launcher).  The horizontal pass of a
//   tile covers TH scale + 2 support rows, (1 + 2 support / (TH scale)) times the rows it owns: for the bicubic at any scale >= 1 (support = 2 scale) 1.25 x
//   at TH = 16, 1.5 x at 8, 1.125 x at 32.  500 x 500 -> 224 x 224 gives 4 x 14 = 56 workgroups per image at 16 rows and 28 at 32, against 256 CUs: 16 keeps the
//   redundancy at a quarter and fills the machine from B = 5; measured (profiles/preprocess_bench.json).
//   LDS per workgroup = 4 (TW (kh + 2) + TH (kv + 2)) + 3 TW (ceil(TH scale_v + 2 support_v) + 2) bytes, at most 64 KiB: the host halves TW while it is at least
//   twice the window's width, then TH down to 1, then TW down to 8.  The smallest tile (1 x 8) fits up to scale 240 on both axes with the bicubic filter
//   (264 scale + 84 bytes); beyond that the launcher returns EEGCLIP_EINVAL.
#include "half16.h"

#include <cmath>
#include <vector>

namespace eeg {

constexpr int RS_BITS = 22;                                   // PIL's PRECISION_BITS = 32 - 8 - 2
constexpr int RS_LDS_MAX = 64 * 1024;
constexpr int RS_CUS = 256;                                    // MI355X
constexpr int RS_SRC_U8 = EEGCLIP_SRC_U8_HWC;

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int clip8(int v) {                 // PIL's clip8: arithmetic shift, then clamp to 0..255
    v >>= RS_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// SRC: 0 bf16 / 1 fp16 / 2 fp32 planes (B, 3, H, W): p = (uint8) rint(min(max(x a + b, 0), 1) 255) in fp32, unfused, round-half-even (diffusers'
// postprocess(output_type="pil"): (x / 2 + 0.5).clamp(0, 1), then (.. * 255).round().astype(uint8)); 3: uint8 (B, H, W, 3)
template <int SRC>
__device__ __forceinline__ int load_px(const void* src, long long i, float a, float b) {
    if (SRC == RS_SRC_U8) return static_cast<const unsigned char*>(src)[i];
    float x = SRC == 2 ? static_cast<const float*>(src)[i] : to_f32<SRC == 1>(static_cast<const unsigned short*>(src)[i]);
    x = x * a;
    x = x + b;
    x = fminf(fmaxf(x, 0.0f), 1.0f);
    return (int)rintf(x * 255.0f);
}

template <int OUT>
__device__ __forceinline__ void store_px(void* out, long long i, float v) {
    if (OUT == 2) static_cast<float*>(out)[i] = v;
    else static_cast<unsigned short*>(out)[i] = to_h<OUT == 1>(v);
}

template <int SRC, int OUT>
__global__ __launch_bounds__(256) void resize_crop_normalize_kernel(const void* __restrict__ src, float a, float b, int H, int W, int ch, int cw,
                                                                     const int* __restrict__ hb, const int* __restrict__ hk, int kh,
                                                                     const int* __restrict__ vb, const int* __restrict__ vk, int kv,
                                                                     const float* __restrict__ scale, const float* __restrict__ shift, void* __restrict__ out,
                                                                     int TH, int TW, int max_rows) {
    EEG_LDS_BASE(int, lds);
    int* hk_s = lds;                                          // [TW][kh]
    int* vk_s = hk_s + TW * kh;                               // [TH][kv]
    int* hb_s = vk_s + TH * kv;                               // [TW][2]
    int* vb_s = hb_s + 2 * TW;                                // [TH][2]
    unsigned char* strip = reinterpret_cast<unsigned char*>(vb_s + 2 * TH);      // [rows][3][TW]
    const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, img = blockIdx.z;
    const int tw = imin(TW, cw - x0), th = imin(TH, ch - y0);  // the part of the tile inside the window (>= 1 each: the grid is ceil(cw / TW) x ceil(ch / TH))

    // 1. coefficient rows and bounds of the tile.  A bound is clamped into the image and into the table's row: whatever the tables hold, reads stay inside.
    for (int i = tid; i < tw; i += 256) {
        int lo = hb[2 * (x0 + i)], n = hb[2 * (x0 + i) + 1];
        lo = imax(0, imin(lo, W - 1));
        hb_s[2 * i] = lo;
        hb_s[2 * i + 1] = imax(0, imin(n, imin(kh, W - lo)));
    }
    for (int i = tid; i < th; i += 256) {
        int lo = vb[2 * (y0 + i)], n = vb[2 * (y0 + i) + 1];
        lo = imax(0, imin(lo, H - 1));
        vb_s[2 * i] = lo;
        vb_s[2 * i + 1] = imax(0, imin(n, imin(kv, H - lo)));
    }
    for (int i = tid; i < tw * kh; i += 256) hk_s[i] = hk[(long long)x0 * kh + i];
    for (int i = tid; i < th * kv; i += 256) vk_s[i] = vk[(long long)y0 * kv + i];
    __syncthreads();

    // the input rows the tile's vertical taps span
    int r0 = vb_s[0], r1 = r0;
    for (int i = 0; i < th; ++i) {
        r0 = imin(r0, vb_s[2 * i]);
        r1 = imax(r1, vb_s[2 * i] + vb_s[2 * i + 1]);
    }
    const int rows = imin(r1 - r0, max_rows);

    // 2. horizontal pass: strip[r][c][x] for r < rows, c < 3, x < tw
    for (int idx = tid; idx < rows * 3 * TW; idx += 256) {
        const int x = idx % TW, rc = idx / TW, c = rc % 3, r = rc / 3;
        if (x >= tw) continue;
        const int lo = hb_s[2 * x], n = hb_s[2 * x + 1];
        const int* k = hk_s + x * kh;
        int ss = 1 << (RS_BITS - 1);
        if (SRC == RS_SRC_U8) {
            const long long base = (((long long)img * H + r0 + r) * W + lo) * 3 + c;
            for (int j = 0; j < n; ++j) ss += k[j] * load_px<SRC>(src, base + 3 * j, a, b);
        } else {
            const long long base = (((long long)img * 3 + c) * H + r0 + r) * W + lo;
            for (int j = 0; j < n; ++j) ss += k[j] * load_px<SRC>(src, base + j, a, b);
        }
        strip[idx] = (unsigned char)clip8(ss);
    }
    __syncthreads();

    // 3. vertical pass + affine
    for (int idx = tid; idx < th * 3 * TW; idx += 256) {
        const int x = idx % TW, yc = idx / TW, c = yc % 3, y = yc / 3;
        if (x >= tw) continue;
        const int lo = vb_s[2 * y] - r0, n = imin(vb_s[2 * y + 1], rows - lo);
        const int* k = vk_s + y * kv;
        int ss = 1 << (RS_BITS - 1);
        for (int j = 0; j < n; ++j) ss += k[j] * (int)strip[((lo + j) * 3 + c) * TW + x];
        float v = (float)clip8(ss);
        if (scale) {
            v = v * scale[c];
            v = v + shift[c];
        }
        store_px<OUT>(out, (((long long)img * 3 + c) * ch + y0 + y) * cw + x0 + x, v);
    }
}

static double rs_bicubic(double x) {                          // Pillow's bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static double rs_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
static bool rs_filter_ok(int filter) { return filter == EEGCLIP_RESIZE_BILINEAR || filter == EEGCLIP_RESIZE_BICUBIC; }
static double rs_support(int filter, int in_size, int out_size) {
    const double scale = (double)in_size / out_size, fs = scale < 1.0 ? 1.0 : scale;
    return (filter == EEGCLIP_RESIZE_BICUBIC ? 2.0 : 1.0) * fs;
}
static int rs_ksize(int filter, int in_size, int out_size) { return (int)ceil(rs_support(filter, in_size, out_size)) * 2 + 1; }

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_resize_coeffs(int in_size, int out_size, int first, int count, int filter, int* bounds, int* coeffs, int ksize) {
    if (in_size < 1 || out_size < 1 || !rs_filter_ok(filter) || in_size > (1 << 24) || out_size > (1 << 24)) return EEGCLIP_EINVAL;
    const int need = rs_ksize(filter, in_size, out_size);
    if (!bounds && !coeffs) return need;                      // the query form
    if (!bounds || !coeffs || first < 0 || count < 1 || first > out_size - count || ksize < need) return EEGCLIP_EINVAL;
    const double scale = (double)in_size / out_size, fs = scale < 1.0 ? 1.0 : scale, support = rs_support(filter, in_size, out_size), ss = 1.0 / fs;
    std::vector<double> w((size_t)need);
    for (int i = 0; i < count; ++i) {
        const int xx = first + i;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            const double v = filter == EEGCLIP_RESIZE_BICUBIC ? rs_bicubic((x + xmin - center + 0.5) * ss) : rs_bilinear((x + xmin - center + 0.5) * ss);
            w[x] = v;
            ww += v;
        }
        int* k = coeffs + (long long)i * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < n) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << RS_BITS)) : (int)(0.5 + v * (1 << RS_BITS));
        }
        bounds[2 * i] = xmin;
        bounds[2 * i + 1] = n;
    }
    return need;
}

namespace {

struct RsArgs {
    const void* src; float a, b; int H, W, ch, cw; const int *hb, *hk; int kh; const int *vb, *vk; int kv; const float *scale, *shift; void* out;
    int TH, TW, max_rows; dim3 grid; size_t lds; void* stream;
};

template <int SRC, int OUT>
void rs_launch(const RsArgs& r) {
    EEG_LAUNCH((resize_crop_normalize_kernel<SRC, OUT>), r.grid, dim3(256), r.lds, r.stream, r.src, r.a, r.b, r.H, r.W, r.ch, r.cw, r.hb, r.hk, r.kh, r.vb, r.vk,
               r.kv, r.scale, r.shift, r.out, r.TH, r.TW, r.max_rows);
}
template <int SRC>
void rs_launch_out(int dtype, const RsArgs& r) {
    if (dtype == EEGCLIP_DT_F32) rs_launch<SRC, 2>(r);
    else if (dtype == EEGCLIP_DT_F16) rs_launch<SRC, 1>(r);
    else rs_launch<SRC, 0>(r);
}

}  // namespace

extern "C" int eegclip_resize_crop_normalize(const void* src, int src_kind, float a, float b, int B, int H, int W, int rh, int rw, int top, int left, int ch,
                                             int cw, int filter, const int* hbounds, const int* hcoeffs, int kh, const int* vbounds, const int* vcoeffs, int kv,
                                             const float* scale, const float* shift, void* out, int dtype, void* stream) {
    if (!src || !out || !hbounds || !hcoeffs || !vbounds || !vcoeffs || B < 1 || B > 65535 || H < 1 || W < 1 || rh < 1 || rw < 1 || ch < 1 || cw < 1 ||
        H > (1 << 24) || W > (1 << 24) || rh > (1 << 24) || rw > (1 << 24) || top < 0 || left < 0 || top > rh - ch || left > rw - cw || !rs_filter_ok(filter) ||
        (scale == nullptr) != (shift == nullptr) || (dtype != EEGCLIP_DT_F32 && !half_dtype_ok(dtype)) ||
        (src_kind != EEGCLIP_SRC_U8_HWC && src_kind != EEGCLIP_DT_F32 && !half_dtype_ok(src_kind)))
        return EEGCLIP_EINVAL;
    if (kh < rs_ksize(filter, W, rw) || kv < rs_ksize(filter, H, rh) || kh > (1 << 14) || kv > (1 << 14)) return EEGCLIP_EINVAL;
    if ((long long)B * 3 * H * W > (1LL << 40) || (long long)B * 3 * ch * cw > (1LL << 40)) return EEGCLIP_EINVAL;
    const uintptr_t src_mask = src_kind == EEGCLIP_SRC_U8_HWC ? 0u : (src_kind == EEGCLIP_DT_F32 ? 3u : 1u), out_mask = dtype == EEGCLIP_DT_F32 ? 3u : 1u;
    if ((reinterpret_cast<uintptr_t>(src) & src_mask) || (reinterpret_cast<uintptr_t>(out) & out_mask) ||
        ((reinterpret_cast<uintptr_t>(hbounds) | reinterpret_cast<uintptr_t>(hcoeffs) | reinterpret_cast<uintptr_t>(vbounds) | reinterpret_cast<uintptr_t>(vcoeffs)) & 3u) ||
        (scale && ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 3u)))
        return EEGCLIP_EALIGN;
    // the tile (see the head of the file): rows of the strip from the vertical scale and support, in double as the coefficient builder computes them
    const double vscale = (double)H / rh, vsupport = rs_support(filter, H, rh);
    int TH = 16, TW = 64, max_rows = 0;
    size_t lds = 0;
    for (;;) {
        max_rows = (int)ceil(TH * vscale + 2.0 * vsupport) + 2;
        if (max_rows > H) max_rows = H;
        lds = 4u * ((size_t)TW * (kh + 2) + (size_t)TH * (kv + 2)) + 3u * (size_t)TW * max_rows;
        if (TW >= 2 * cw && TW > 8) TW /= 2;                  // columns nobody owns cost LDS and lanes
        else if (lds <= (size_t)RS_LDS_MAX) {
            // few images: a workgroup's time is its serial tap loops, so smaller tiles until every CU has one -- narrower first (no redundant work), then lower
            // (B = 1 at 500 -> 224: 8 x 16 tiles, 392 workgroups, 1.5 x the rows instead of 56 workgroups at 1.25 x)
            const long long wgs = (long long)B * ((cw + TW - 1) / TW) * ((ch + TH - 1) / TH);
            if (wgs >= RS_CUS) break;
            if (TW > 16) TW /= 2;
            else if (TH > 4) TH /= 2;
            else break;
        }
        else if (TH > 1) TH /= 2;
        else if (TW > 8) TW /= 2;
        else return EEGCLIP_EINVAL;                           // the scale is beyond what one workgroup's LDS holds
    }
    const long long gy = (ch + TH - 1) / TH;
    if (gy > 65535) return EEGCLIP_EINVAL;
    RsArgs r{src, a, b, H, W, ch, cw, hbounds, hcoeffs, kh, vbounds, vcoeffs, kv, scale, shift, out, TH, TW, max_rows,
             dim3((unsigned)((cw + TW - 1) / TW), (unsigned)gy, (unsigned)B), (lds + 15) / 16 * 16, stream};
    if (src_kind == EEGCLIP_SRC_U8_HWC) rs_launch_out<3>(dtype, r);
    else if (src_kind == EEGCLIP_DT_F32) rs_launch_out<2>(dtype, r);
    else if (src_kind == EEGCLIP_DT_F16) rs_launch_out<1>(dtype, r);
    else rs_launch_out<0>(dtype, r);
    return (int)hipGetLastError();
}
