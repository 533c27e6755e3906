// The middle of EfficientNet's MBConv block (torchvision/models/efficientnet.py; the EffNet-B row of the reference's metrics table): depthwise k x k convolution +
// eval-mode BatchNorm + SiLU with the squeeze's pooled sums from the same launch, the squeeze-and-excitation gate, and the gate multiply.  The 1 x 1 expansion and
// projection around them are csrc/metric_nets.hip's eegclip_convbnact16.  16-bit activations in that file's NHWC frames, fp32 arithmetic, one rounding per store.
//
// Depthwise: memory- and vector-ALU-bound (k^2 multiply-adds per 2 bytes stored; no matrix core applies).  A thread owns 8 consecutive channels -- one 16-byte
// access per pixel -- and DW_PX = 4 consecutive output pixels of a row, so the k + 3 stride columns of a window row are each loaded and converted once and feed
// up to k of the 4 x k taps from registers; the k weights of a row are 16-byte loads of [ky][kx][C].  The frame's zero border IS the padding: the only test is
// the run's right end, where a run of 4 may pass the last pixel of a row.  A workgroup is 8 channel groups (64 channels: 128 contiguous bytes per pixel) x 32
// runs, counted along the image's rows, so a slab index s names 128 output pixels of one image (the last slab: what is left).
//
// The squeeze: each thread adds what it STORED (the rounded values, so the mean is that of the tensor the gate multiplies), the 32 runs of a workgroup are added
// through LDS in their order, and workgroup s writes pooled[n][s][c]: a slab per workgroup as in csrc/head_gemm.hip, every element written once, no atomics and
// no memset; eegclip_se_gate16 adds the S slabs in a fixed order.  Runs are bit-identical.
#include "silu16.h"

namespace eeg {

constexpr int DW_PX = 4, DW_RUNS = 32, DW_CG = 8;            // 256 threads: thread t owns channel group t & 7 and run t >> 3 of its workgroup

template <bool F16, int K, int ST>
__global__ __launch_bounds__(256, K == 3 ? 4 : 2) void dwconv16_kernel(const unsigned short* __restrict__ in, const unsigned short* __restrict__ W, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, unsigned short* __restrict__ out, float* __restrict__ pooled, int H, int Wi,
                                                       int C, int Ho, int Wo, int S) {
    EEG_LDS_BASE(float, red);                                 // [DW_RUNS][64]
    constexpr int P = K / 2, WIN = K + (DW_PX - 1) * ST;
    const int t = threadIdx.x, cg = t & (DW_CG - 1), rl = t >> 3;
    const int s = (int)blockIdx.x, n_ = (int)blockIdx.z;
    const int c = 64 * (int)blockIdx.y + 8 * cg;
    const int rpr = (Wo + DW_PX - 1) / DW_PX;                 // runs per output row
    const int run = s * DW_RUNS + rl;
    const int Hp = H + 2 * P, Wp = Wi + 2 * P;
    float psum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < C && run < Ho * rpr) {
        const int y = run / rpr, x0 = (run - y * rpr) * DW_PX;
        const int ncols = Wp - x0 * ST < WIN ? Wp - x0 * ST : WIN;       // the frame columns this run's windows have (all WIN, except at a row's right end)
        const unsigned short* src = in + (((long long)n_ * Hp + y * ST) * Wp + x0 * ST) * C + c;
        float acc[DW_PX][8];
#pragma unroll
        for (int px = 0; px < DW_PX; ++px)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[px][e] = 0.f;
#pragma unroll 1
        for (int ky = 0; ky < K; ++ky) {                      // (not unrolled: a row's k weights and its k + 3 stride columns are what the registers hold)
            float w[K][8];
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const u16x8 wv = *reinterpret_cast<const u16x8*>(W + (long long)(ky * K + kx) * C + c);
#pragma unroll
                for (int e = 0; e < 8; ++e) w[kx][e] = to_f32<F16>(wv[e]);
            }
#pragma unroll
            for (int col = 0; col < WIN; ++col) {
                u16x8 v{0, 0, 0, 0, 0, 0, 0, 0};
                if (col < ncols) v = *reinterpret_cast<const u16x8*>(src + ((long long)ky * Wp + col) * C);
                float xv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) xv[e] = to_f32<F16>(v[e]);
#pragma unroll
                for (int px = 0; px < DW_PX; ++px) {
                    const int kx = col - px * ST;             // (a constant after unrolling: pixel px takes this column as tap kx, or not at all)
                    if (kx >= 0 && kx < K) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[px][e] += xv[e] * w[kx][e];
                    }
                }
            }
        }
        const f32x4 sc0 = *reinterpret_cast<const f32x4*>(scale + c), sc1 = *reinterpret_cast<const f32x4*>(scale + c + 4);
        const f32x4 sh0 = *reinterpret_cast<const f32x4*>(shift + c), sh1 = *reinterpret_cast<const f32x4*>(shift + c + 4);
        unsigned short* dst = out + (((long long)n_ * Ho + y) * Wo + x0) * C + c;
#pragma unroll
        for (int px = 0; px < DW_PX; ++px) {
            if (x0 + px >= Wo) break;
            u16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = acc[px][e] * (e < 4 ? sc0[e & 3] : sc1[e & 3]) + (e < 4 ? sh0[e & 3] : sh1[e & 3]);
                o[e] = to_h<F16>(silu_exp2(v));
                psum[e] += to_f32<F16>(o[e]);
            }
            *reinterpret_cast<u16x8*>(dst + (long long)px * C) = o;
        }
    }
    // ---- the squeeze's partial sums: the workgroup's 32 runs in their order, one fp32 per channel
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl * 64 + 8 * cg + e] = psum[e];
    __syncthreads();
    if (t < 64 && 64 * (int)blockIdx.y + t < C) {
        float sum = 0.f;
        for (int r = 0; r < DW_RUNS; ++r) sum += red[r * 64 + t];
        pooled[((long long)n_ * S + s) * C + 64 * (int)blockIdx.y + t] = sum;
    }
}

// ---- the squeeze-and-excitation gate of one image per workgroup: the slabs added in a fixed order and divided by the pixel count, fc1 + SiLU with a wave per
// hidden unit (lanes stride over the channels, a shuffle tree), fc2 + sigmoid with a thread per channel.  Where the channels leave threads idle (C <= 128: the
// early stages, whose large images have the most slabs) G = 4 or 2 groups of threads each add a contiguous quarter or half of the slabs in increasing s and the
// G partial sums are added in their order; otherwise one thread adds a channel's S slabs in increasing s.
template <bool F16>
__global__ __launch_bounds__(256) void se_gate16_kernel(const float* __restrict__ pooled, const unsigned short* __restrict__ W1, const unsigned short* __restrict__ b1,
                                                        const unsigned short* __restrict__ W2, const unsigned short* __restrict__ b2, float* __restrict__ gate, int S,
                                                        int HW, int C, int sq) {
    EEG_LDS_BASE(float, mean);                                // [C], then hid[sq], then part[G][C] where G > 1
    float* hid = mean + C;
    float* part = hid + sq;
    const int t = threadIdx.x, lane = t & 63, wave = wave_uniform(t >> 6);
    const long long n_ = blockIdx.x;
    const float cnt = (float)HW;
    const int cw = C <= 64 ? 64 : 128, G = C <= 128 ? 256 / cw : 1;
    if (G == 1) {
        for (int c = t; c < C; c += 256) {
            float s = 0.f;
            for (int si = 0; si < S; ++si) s += pooled[(n_ * S + si) * C + c];
            mean[c] = s / cnt;
        }
    } else {
        const int grp = t / cw, c = t - grp * cw, per = (S + G - 1) / G;
        const int s0 = grp * per, s1 = s0 + per < S ? s0 + per : S;
        if (c < C) {
            float s = 0.f;
            for (int si = s0; si < s1; ++si) s += pooled[(n_ * S + si) * C + c];
            part[grp * C + c] = s;
        }
        __syncthreads();
        if (t < C) {
            float s = part[t];
            for (int g = 1; g < G; ++g) s += part[g * C + t];
            mean[t] = s / cnt;
        }
    }
    __syncthreads();
    for (int j = wave; j < sq; j += 4) {
        float p = 0.f;
        for (int c = lane; c < C; c += 64) p += to_f32<F16>(W1[(long long)j * C + c]) * mean[c];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) p += __shfl_xor(p, m, 64);
        if (lane == 0) hid[j] = silu(p + to_f32<F16>(b1[j]));
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        float g = to_f32<F16>(b2[c]);
        for (int j = 0; j < sq; ++j) g += to_f32<F16>(W2[(long long)c * sq + j]) * hid[j];
        gate[n_ * C + c] = 1.0f / (1.0f + expf(-g));
    }
}

// ---- y *= gate, in place: thread = (pixel, 8 consecutive channels), one 16-byte load and store.  The product is an fp32 VALUE (rounded to fp32) before it is
// rounded to 16 bits, as torch's (y.float() * gate).to(dtype): left alone, hipcc fuses fp16 x fp32 -> fp16 into v_fma_mixlo_f16, whose results differed from that
// in about one element of 10^4 on the MI355X; the empty asm keeps the multiply a v_mul_f32 and the conversion a v_cvt.
__device__ __forceinline__ float f32_value(float v) {
#if !defined(EEG_EMU)
    asm("" : "+v"(v));
#endif
    return v;
}

template <bool F16>
__global__ __launch_bounds__(256) void gate_mul16_kernel(unsigned short* __restrict__ y, const float* __restrict__ gate, int N, int HW, int C) {
    const int c8n = C / 8;
    const long long total = (long long)N * HW * c8n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 8 * (int)(q % c8n);
        const long long pq = q / c8n, n_ = pq / HW;
        const float* g = gate + n_ * C + c;
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(g), g1 = *reinterpret_cast<const f32x4*>(g + 4);
        u16x8* p = reinterpret_cast<u16x8*>(y + pq * C + c);
        u16x8 v = *p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = to_h<F16>(f32_value(to_f32<F16>(v[e]) * (e < 4 ? g0[e & 3] : g1[e & 3])));
        *p = v;
    }
}

static bool dw_shape_ok(int H, int W, int k, int stride) { return H >= 1 && W >= 1 && (k == 3 || k == 5) && (stride == 1 || stride == 2); }

static int dw_slabs(int H, int W, int k, int stride) {
    const int Ho = (H + 2 * (k / 2) - k) / stride + 1, Wo = (W + 2 * (k / 2) - k) / stride + 1;
    const long long runs = (long long)Ho * ((Wo + DW_PX - 1) / DW_PX);
    const long long S = (runs + DW_RUNS - 1) / DW_RUNS;
    return S > 0x7fffffffLL ? EEGCLIP_EINVAL : (int)S;
}

template <bool F16, int K, int ST>
static void dw_launch(const unsigned short* in, const unsigned short* W, const float* scale, const float* shift, unsigned short* out, float* pooled, int N, int H,
                      int Wi, int C, int S, void* stream) {
    const int Ho = (H + 2 * (K / 2) - K) / ST + 1, Wo = (Wi + 2 * (K / 2) - K) / ST + 1;
    const dim3 grid((unsigned)S, (unsigned)((C + 63) / 64), (unsigned)N);
    EEG_LAUNCH((dwconv16_kernel<F16, K, ST>), grid, dim3(256), DW_RUNS * 64 * sizeof(float), stream, in, W, scale, shift, out, pooled, H, Wi, C, Ho, Wo, S);
}

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_dwconv16_slabs(int H, int W, int k, int stride) { return dw_shape_ok(H, W, k, stride) ? dw_slabs(H, W, k, stride) : EEGCLIP_EINVAL; }

extern "C" int eegclip_dwconv16(const void* in, const void* W, const float* scale, const float* shift, void* out, float* pooled, int N, int H, int Wi, int C, int k,
                                int stride, int dtype, void* stream) {
    if (!in || !W || !scale || !shift || !out || !pooled || N < 1 || N > 65535 || !dw_shape_ok(H, Wi, k, stride) || C < 8 || C % 8 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    const int S = dw_slabs(H, Wi, k, stride);
    if (S < 1) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(scale) |
         reinterpret_cast<uintptr_t>(shift)) & 15u)
        return EEGCLIP_EALIGN;
    if (reinterpret_cast<uintptr_t>(pooled) & 3u) return EEGCLIP_EALIGN;
    const unsigned short* i16 = static_cast<const unsigned short*>(in);
    const unsigned short* w16 = static_cast<const unsigned short*>(W);
    unsigned short* o16 = static_cast<unsigned short*>(out);
    const bool f16 = dtype == EEGCLIP_DT_F16;
#define DW_CASE(K, ST)                                                                                \
    if (k == K && stride == ST) {                                                                     \
        if (f16) dw_launch<true, K, ST>(i16, w16, scale, shift, o16, pooled, N, H, Wi, C, S, stream); \
        else     dw_launch<false, K, ST>(i16, w16, scale, shift, o16, pooled, N, H, Wi, C, S, stream); \
    }
    DW_CASE(3, 1)
    DW_CASE(3, 2)
    DW_CASE(5, 1)
    DW_CASE(5, 2)
#undef DW_CASE
    return (int)hipGetLastError();
}

extern "C" int eegclip_se_gate16(const float* pooled, const void* W1, const void* b1, const void* W2, const void* b2, float* gate, int N, int S, int HW, int C, int sq,
                                 int dtype, void* stream) {
    if (!pooled || !W1 || !b1 || !W2 || !b2 || !gate || N < 1 || S < 1 || HW < 1 || C < 1 || C > 8192 || sq < 1 || sq > 4096 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(pooled) | reinterpret_cast<uintptr_t>(gate)) & 3u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(W1) | reinterpret_cast<uintptr_t>(b1) | reinterpret_cast<uintptr_t>(W2) | reinterpret_cast<uintptr_t>(b2)) & 1u) return EEGCLIP_EALIGN;
    const size_t lds = (size_t)(C + sq + (C <= 64 ? 4 * C : C <= 128 ? 2 * C : 0)) * sizeof(float);
    const unsigned short *w1 = static_cast<const unsigned short*>(W1), *c1 = static_cast<const unsigned short*>(b1);
    const unsigned short *w2 = static_cast<const unsigned short*>(W2), *c2 = static_cast<const unsigned short*>(b2);
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((se_gate16_kernel<true>), dim3((unsigned)N), dim3(256), lds, stream, pooled, w1, c1, w2, c2, gate, S, HW, C, sq);
    else                         EEG_LAUNCH((se_gate16_kernel<false>), dim3((unsigned)N), dim3(256), lds, stream, pooled, w1, c1, w2, c2, gate, S, HW, C, sq);
    return (int)hipGetLastError();
}

extern "C" int eegclip_gate_mul16(void* y, const float* gate, int N, int HW, int C, int dtype, void* stream) {
    if (!y || !gate || N < 1 || HW < 1 || C < 8 || C % 8 || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gate)) & 15u) return EEGCLIP_EALIGN;
    long long g = ((long long)N * HW * (C / 8) + 255) / 256;
    if (g > 16384) g = 16384;
    unsigned short* y16 = static_cast<unsigned short*>(y);
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((gate_mul16_kernel<true>), dim3((unsigned)g), dim3(256), 0, stream, y16, gate, N, HW, C);
    else                         EEG_LAUNCH((gate_mul16_kernel<false>), dim3((unsigned)g), dim3(256), 0, stream, y16, gate, N, HW, C);
    return (int)hipGetLastError();
}
