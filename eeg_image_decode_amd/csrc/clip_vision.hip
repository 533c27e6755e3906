// The front end of CLIP's vision towers (transformers' CLIPVisionEmbeddings + pre_layrnorm: ViT-H/14 = the IP-Adapter's models/image_encoder, whose image_embeds
// are the `image_embeds` of Generation/custom_pipeline.py:365-373 and the data sets' cached features; ViT-L/14 = GIT's git.image_encoder, whose tokens
// Generation/modeling_git.py:1970-1973 takes as an input), 16-bit out, fp32 arithmetic.  Three launches from the pixels to hidden_states[0]:
//   patch_rows16   NCHW pixels (fp32, fp16 or bf16) -> the A operand of the patch convolution as a GEMM: B (1 + P) rows of Kpad = ceil64(3 patch^2) columns.
//                  Row b (1 + P) is zero (the class token's slot: its "patch embedding" is 0), row b (1 + P) + 1 + p holds patch p = (py, px) in (c, i, j)
//                  order -- the flatten order of patch_embedding.weight (C, 3, patch, patch) -- zero-padded to Kpad.  Optional per-channel scale / shift
//                  (x * scale[c] + shift[c] in fp32, one rounding): 0..255 pixels are normalised with CLIP's mean / std in the same pass.  Without them a
//                  16-bit pixel of the output's dtype is copied bit for bit.  One 16-byte store per thread.
//   (csrc/gemm16.hip against the weight packed once to (C, Kpad): no bias, CLIP's patch convolution has none)
//   embed_ln16     y[r] = LayerNorm(x[r] + pos[r % T]) * gamma + beta: the position embedding (row 0 = position 0 + the class embedding, packed once on the
//                  host) added to the GEMM's output, the sum kept in fp32, then pre_layrnorm -- csrc/unet.hip's layernorm16 with one more operand: one wave
//                  per row, the row in registers, mean and variance in two passes over the registers.  y may be x.
#include "half16.h"

namespace eeg {

constexpr int EL16_MAXV = 8;                                  // 8-channel vectors per lane: C <= 64 * 8 * 8 = 4096

// PIX: 0 bf16, 1 fp16, 2 fp32 (the dtype codes of include/eegclip.h)
template <int PIX>
__device__ __forceinline__ float pixel_f32(const void* px, long long i) {
    if (PIX == 2) return static_cast<const float*>(px)[i];
    return to_f32<PIX == 1>(static_cast<const unsigned short*>(px)[i]);
}

template <bool F16, int PIX>
__global__ __launch_bounds__(256) void patch_rows16_kernel(const void* __restrict__ px, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            unsigned short* __restrict__ out, int B, int H, int W, int patch, int Kpad) {
    const int gw = W / patch, P = (H / patch) * gw, T = 1 + P, pp = patch * patch, K = 3 * pp, k8 = Kpad / 8;
    const long long total = (long long)B * T * k8;
    constexpr bool COPY = PIX == (F16 ? 1 : 0);               // same 16-bit format in and out: without scale / shift a bit copy
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const long long row = q / k8;
        const int col0 = 8 * (int)(q - row * k8), b = (int)(row / T), t = (int)(row - (long long)b * T);
        u16x8 o = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (t > 0 && col0 < K) {
            const int p = t - 1, py = p / gw, pxx = p - py * gw;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int col = col0 + e;
                if (col < K) {
                    const int c = col / pp, ij = col - c * pp, i = ij / patch, j = ij - i * patch;
                    const long long src = (((long long)b * 3 + c) * H + py * patch + i) * W + pxx * patch + j;      // c < 3, row < H, column < W
                    if (COPY && !scale) {
                        o[e] = static_cast<const unsigned short*>(px)[src];
                    } else {
                        float v = pixel_f32<PIX>(px, src);
                        if (scale) v = v * scale[c] + shift[c];
                        o[e] = to_h<F16>(v);
                    }
                }
            }
        }
        *reinterpret_cast<u16x8*>(out + row * Kpad + col0) = o;
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void embed_ln16_kernel(const unsigned short* x, long long ldx, const unsigned short* __restrict__ pos, int T,
                                                          const unsigned short* __restrict__ gamma, const unsigned short* __restrict__ beta, unsigned short* y,
                                                          long long ldy, int rows, int C, float eps) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                    // (wave-uniform: no barrier below)
    const unsigned short* xr = x + (long long)r * ldx;
    const unsigned short* pr = pos + (long long)(r % T) * C;
    const int nv = C / 8;
    float v[EL16_MAXV][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < EL16_MAXV; ++i) {
        const int c8 = lane + 64 * i;
        if (c8 < nv) {
            const u16x8 a = *reinterpret_cast<const u16x8*>(xr + 8 * c8), p = *reinterpret_cast<const u16x8*>(pr + 8 * c8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[i][e] = to_f32<F16>(a[e]) + to_f32<F16>(p[e]);
                s += v[i][e];
            }
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < EL16_MAXV; ++i)
        if (lane + 64 * i < nv) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[i][e] - mean;
                q += d * d;
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    unsigned short* yr = y + (long long)r * ldy;
#pragma unroll
    for (int i = 0; i < EL16_MAXV; ++i) {
        const int c8 = lane + 64 * i;
        if (c8 < nv) {
            const u16x8 g = *reinterpret_cast<const u16x8*>(gamma + 8 * c8), b = *reinterpret_cast<const u16x8*>(beta + 8 * c8);
            u16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = to_h<F16>((v[i][e] - mean) * rstd * to_f32<F16>(g[e]) + to_f32<F16>(b[e]));
            *reinterpret_cast<u16x8*>(yr + 8 * c8) = o;
        }
    }
}

}  // namespace eeg

using namespace eeg;

static bool cv_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <bool F16>
static void patch_rows16_launch(int pix_dtype, unsigned g, void* stream, const void* px, const float* scale, const float* shift, unsigned short* out, int B, int H,
                                int W, int patch, int Kpad) {
    if (pix_dtype == EEGCLIP_DT_F32) EEG_LAUNCH((patch_rows16_kernel<F16, 2>), dim3(g), dim3(256), 0, stream, px, scale, shift, out, B, H, W, patch, Kpad);
    else if (pix_dtype == EEGCLIP_DT_F16) EEG_LAUNCH((patch_rows16_kernel<F16, 1>), dim3(g), dim3(256), 0, stream, px, scale, shift, out, B, H, W, patch, Kpad);
    else EEG_LAUNCH((patch_rows16_kernel<F16, 0>), dim3(g), dim3(256), 0, stream, px, scale, shift, out, B, H, W, patch, Kpad);
}

extern "C" int eegclip_patch_rows16(const void* pixels, int pix_dtype, const float* scale, const float* shift, void* out, int B, int H, int W, int patch, int dtype,
                                    void* stream) {
    if (!pixels || !out || B < 1 || patch < 1 || H < patch || W < patch || H % patch || W % patch || (scale == nullptr) != (shift == nullptr) ||
        !half_dtype_ok(dtype) || (pix_dtype != EEGCLIP_DT_F32 && !half_dtype_ok(pix_dtype)))
        return EEGCLIP_EINVAL;
    const long long K = 3LL * patch * patch, Kpad = (K + 63) / 64 * 64, rows = (long long)B * (1 + (long long)(H / patch) * (W / patch));
    if (Kpad > (1 << 20) || rows > 0x7fffffffLL || (long long)B * 3 * H * W > (1LL << 40)) return EEGCLIP_EINVAL;
    if (!cv_a16(out) || (reinterpret_cast<uintptr_t>(pixels) & (pix_dtype == EEGCLIP_DT_F32 ? 3u : 1u)) || (scale && ((reinterpret_cast<uintptr_t>(scale) |
        reinterpret_cast<uintptr_t>(shift)) & 3u)))
        return EEGCLIP_EALIGN;
    long long g = (rows * (Kpad / 8) + 255) / 256;
    if (g > 16384) g = 16384;
    unsigned short* o = static_cast<unsigned short*>(out);
    if (dtype == EEGCLIP_DT_F16) patch_rows16_launch<true>(pix_dtype, (unsigned)g, stream, pixels, scale, shift, o, B, H, W, patch, (int)Kpad);
    else                         patch_rows16_launch<false>(pix_dtype, (unsigned)g, stream, pixels, scale, shift, o, B, H, W, patch, (int)Kpad);
    return (int)hipGetLastError();
}

extern "C" int eegclip_embed_ln16(const void* x, long long ldx, const void* pos, int T, const void* gamma, const void* beta, void* y, long long ldy, int rows, int C,
                                  float eps, int dtype, void* stream) {
    if (!x || !pos || !gamma || !beta || !y || T < 1 || rows < 1 || C < 8 || C % 8 || C > 64 * 8 * EL16_MAXV || ldx < C || ldy < C || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if (!cv_a16(x) || !cv_a16(pos) || !cv_a16(gamma) || !cv_a16(beta) || !cv_a16(y) || ldx % 8 || ldy % 8) return EEGCLIP_EALIGN;
    const dim3 g((unsigned)((rows + 3) / 4));
    if (dtype == EEGCLIP_DT_F16)
        EEG_LAUNCH((embed_ln16_kernel<true>), g, dim3(256), 0, stream, static_cast<const unsigned short*>(x), ldx, static_cast<const unsigned short*>(pos), T,
                   static_cast<const unsigned short*>(gamma), static_cast<const unsigned short*>(beta), static_cast<unsigned short*>(y), ldy, rows, C, eps);
    else
        EEG_LAUNCH((embed_ln16_kernel<false>), g, dim3(256), 0, stream, static_cast<const unsigned short*>(x), ldx, static_cast<const unsigned short*>(pos), T,
                   static_cast<const unsigned short*>(gamma), static_cast<const unsigned short*>(beta), static_cast<unsigned short*>(y), ldy, rows, C, eps);
    return (int)hipGetLastError();
}
