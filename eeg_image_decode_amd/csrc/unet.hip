// The SDXL UNet's layers that neither csrc/vae.hip nor csrc/gemm16.hip covers (Generation/custom_pipeline.py:456-492 loads UNet2DConditionModel from
// stabilityai/sdxl-turbo; the module is diffusers 0.30.0's, not vendored by the reference), 16-bit in and out, fp32 arithmetic:
//   layernorm16  BasicTransformerBlock's norm1 / norm2 / norm3 (LayerNorm(C, eps 1e-5), affine) over 16-bit token rows: one wave per row, the row kept in
//                registers (16-byte reads), mean and variance in two passes over the registers
//   geglu16      the feed-forward's GEGLU: a * gelu_erf(g) for the [value | gate] halves of ff.net.0.proj's output row
//   concat16     the up blocks' skip concatenation cat([h, skip], channel) of two padded NHWC frames, interior pixels only (the frame pool relies on borders
//                that no launch writes: vae.py)
#include "half16.h"

namespace eeg {

constexpr int LN16_MAXV = 8;                                  // 8-channel vectors per lane: C <= 64 * 8 * 8 = 4096

template <bool F16>
__global__ __launch_bounds__(256) void layernorm16_kernel(const unsigned short* __restrict__ x, long long ldx, const unsigned short* __restrict__ gamma,
                                                           const unsigned short* __restrict__ beta, unsigned short* __restrict__ y, long long ldy, int rows,
                                                           int C, float eps) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                    // (wave-uniform: no barrier below)
    const unsigned short* xr = x + (long long)r * ldx;
    const int nv = C / 8;
    u16x8 v[LN16_MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN16_MAXV; ++i) {
        const int c8 = lane + 64 * i;
        if (c8 < nv) {
            v[i] = *reinterpret_cast<const u16x8*>(xr + 8 * c8);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += to_f32<F16>(v[i][e]);
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN16_MAXV; ++i)
        if (lane + 64 * i < nv) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = to_f32<F16>(v[i][e]) - mean;
                q += d * d;
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    unsigned short* yr = y + (long long)r * ldy;
#pragma unroll
    for (int i = 0; i < LN16_MAXV; ++i) {
        const int c8 = lane + 64 * i;
        if (c8 < nv) {
            const u16x8 g = *reinterpret_cast<const u16x8*>(gamma + 8 * c8), b = *reinterpret_cast<const u16x8*>(beta + 8 * c8);
            u16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = to_h<F16>((to_f32<F16>(v[i][e]) - mean) * rstd * to_f32<F16>(g[e]) + to_f32<F16>(b[e]));
            *reinterpret_cast<u16x8*>(yr + 8 * c8) = o;
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void geglu16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y, int M, int D) {
    const int d8 = D / 8;
    const long long total = (long long)M * d8;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const long long m = q / d8;
        const int j = 8 * (int)(q - m * d8);
        const u16x8 a = *reinterpret_cast<const u16x8*>(x + m * 2 * D + j), g = *reinterpret_cast<const u16x8*>(x + m * 2 * D + D + j);
        u16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = to_h<F16>(to_f32<F16>(a[e]) * gelu_erf(to_f32<F16>(g[e])));
        *reinterpret_cast<u16x8*>(y + m * D + j) = o;
    }
}

__global__ __launch_bounds__(256) void concat16_kernel(const unsigned short* __restrict__ a, const unsigned short* __restrict__ b, unsigned short* __restrict__ out,
                                                        int N, int H, int W, int pad, int Ca, int Cb, int opad) {
    const int ca8 = Ca / 8, c8 = (Ca + Cb) / 8, Wp = W + 2 * pad, Hp = H + 2 * pad, Wop = W + 2 * opad, Hop = H + 2 * opad;
    const long long hw = (long long)H * W, total = (long long)N * hw * c8;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const long long pq = q / c8;
        const int k = (int)(q - pq * c8);
        const int n_ = (int)(pq / hw), p = (int)(pq - (long long)n_ * hw), yy = p / W, xx = p - yy * W;
        const long long ipix = ((long long)n_ * Hp + yy + pad) * Wp + xx + pad, opix = ((long long)n_ * Hop + yy + opad) * Wop + xx + opad;
        const u16x8 v = k < ca8 ? *reinterpret_cast<const u16x8*>(a + ipix * Ca + 8 * k) : *reinterpret_cast<const u16x8*>(b + ipix * Cb + 8 * (k - ca8));
        *reinterpret_cast<u16x8*>(out + opix * (Ca + Cb) + 8 * k) = v;
    }
}

}  // namespace eeg

using namespace eeg;

static bool un_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" int eegclip_layernorm16(const void* x, long long ldx, const void* gamma, const void* beta, void* y, long long ldy, int rows, int C, float eps, int dtype,
                                   void* stream) {
    if (!x || !gamma || !beta || !y || rows < 1 || C < 8 || C % 8 || C > 64 * 8 * LN16_MAXV || ldx < C || ldy < C || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if (!un_a16(x) || !un_a16(gamma) || !un_a16(beta) || !un_a16(y) || ldx % 8 || ldy % 8) return EEGCLIP_EALIGN;
    const dim3 g((unsigned)((rows + 3) / 4));
    if (dtype == EEGCLIP_DT_F16)
        EEG_LAUNCH((layernorm16_kernel<true>), g, dim3(256), 0, stream, static_cast<const unsigned short*>(x), ldx, static_cast<const unsigned short*>(gamma),
                   static_cast<const unsigned short*>(beta), static_cast<unsigned short*>(y), ldy, rows, C, eps);
    else
        EEG_LAUNCH((layernorm16_kernel<false>), g, dim3(256), 0, stream, static_cast<const unsigned short*>(x), ldx, static_cast<const unsigned short*>(gamma),
                   static_cast<const unsigned short*>(beta), static_cast<unsigned short*>(y), ldy, rows, C, eps);
    return (int)hipGetLastError();
}

extern "C" int eegclip_geglu16(const void* x, void* y, int M, int D, int dtype, void* stream) {
    if (!x || !y || M < 1 || D < 8 || D % 8 || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if (!un_a16(x) || !un_a16(y)) return EEGCLIP_EALIGN;
    long long g = ((long long)M * (D / 8) + 255) / 256;
    if (g > 16384) g = 16384;
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((geglu16_kernel<true>), dim3((unsigned)g), dim3(256), 0, stream, static_cast<const unsigned short*>(x), static_cast<unsigned short*>(y), M, D);
    else                         EEG_LAUNCH((geglu16_kernel<false>), dim3((unsigned)g), dim3(256), 0, stream, static_cast<const unsigned short*>(x), static_cast<unsigned short*>(y), M, D);
    return (int)hipGetLastError();
}

extern "C" int eegclip_concat16(const void* a, const void* b, void* out, int N, int H, int W, int pad, int Ca, int Cb, int out_pad, int dtype, void* stream) {
    if (!a || !b || !out || N < 1 || H < 1 || W < 1 || pad < 0 || pad > 1 || out_pad < 0 || out_pad > 1 || Ca < 8 || Cb < 8 || Ca % 8 || Cb % 8 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if (!un_a16(a) || !un_a16(b) || !un_a16(out)) return EEGCLIP_EALIGN;
    long long g = ((long long)N * H * W * ((Ca + Cb) / 8) + 255) / 256;
    if (g > 16384) g = 16384;
    EEG_LAUNCH(concat16_kernel, dim3((unsigned)g), dim3(256), 0, stream, static_cast<const unsigned short*>(a), static_cast<const unsigned short*>(b),
               static_cast<unsigned short*>(out), N, H, W, pad, Ca, Cb, out_pad);
    return (int)hipGetLastError();
}
