// ConvTranspose2d(kernel 4, stride 2, padding 1) on 16-bit padded NHWC frames: the layers of the reference's low-level EEG -> VAE-latent encoder
// (Generation/train_vae_latent_512_low_level_no_average.py:219-260, encoder_low_level.upsampler).  H x W -> 2H x 2W; fp16 / bf16 in and out, fp32 accumulation.
//
//   sub-pixel phases   out[2m + py][2n + px] is a 2 x 2 convolution of the input.  Per axis, output o = 2 i - 1 + k: an even phase takes weight taps k = 1
//     (source m) and k = 3 (source m - 1), an odd phase k = 2 (source m) and k = 0 (source m + 1).  Tap t = 2 ty + tx; ty = 0 is the source row m itself,
//     ty = 1 the neighbour (m - 1 for py = 0, m + 1 for py = 1), likewise tx.  The frame's zero border serves the neighbours outside the image: no
//     boundary case.  Per phase an implicit GEMM with M = N Hi Wi pixels, N = Cout, K = 4 Cin.
//   packed weight      [phase 2 py + px][Cout][tap][Cin] (K contiguous), repacked once on the host from torch's (Cin, Cout, 4, 4).
//   tap mask           bit 4 phase + tap set = the tap is read.  A tap whose source lies in the zero border for EVERY pixel of the launch (ty = 1 with
//     Hi = 1, tx = 1 with Wi = 1) may be cleared: at 1 x 1 three of four taps, i.e. three quarters of the weight, are never read.  A host-side decision
//     in the descriptor, not a data-dependent branch; a mask that clears a tap some pixel needs is rejected.
//   convt16_kernel     Cout % 16 == 0.  A weight-streaming kernel in the manner of gemm16_skinny (csrc/caption.hip): a workgroup owns 16 output channels
//     of one phase and 16 MT pixels; its WAVES split K in chunks of 64 (chunk i of the 4 Cin / 64 slots goes to wave i % WAVES whatever the mask, so
//     clearing dead taps changes no summation order: same bits).  v_mfma_f32_16x16x32 with W as the A operand (two 16-byte loads per lane and chunk
//     straight into VGPRs) and the pixels, zero-padded to 16 rows in registers, as B: D[co][pixel].  The WAVES partial tiles meet in LDS and are added
//     in wave order: bit-reproducible, no atomics, no memset.  MT = 1 for few pixels (the weight is the traffic), MT = 4 reuses a weight fragment for
//     64 pixels where M is large and the weight small.
//   convt_small16_kernel   Cout < 16 (the last layer, 64 -> 4): thread = one output element, packed weights in LDS, fp32 accumulation, output UNPADDED
//     NCHW (N, Cout, 2H, 2W): the layout of the pipeline's low_level_latent.
//   epilogue           y = acc * scale[co] + shift[co] (fp32; eval-mode BatchNorm folded with the bias; scale NULL: 1, shift NULL: 0), optional ReLU, one
//     rounding to 16 bit.  Interior pixels only: the output frame's border is never written.
#include "half16.h"

namespace eeg {

struct ct_args {
    const unsigned short *in, *W;
    unsigned short* out;
    const float *scale, *shift;
    int N, Hi, Wi, Cin, Cout, M, relu, mask;
};

// source offset (rows, columns) of tap half `t` (0: the pixel itself, 1: the neighbour) in phase half `p`
__device__ __forceinline__ int ct_delta(int p, int t) { return t ? (p ? 1 : -1) : 0; }

template <bool F16, int WAVES, int MT, int U>
__global__ __launch_bounds__(64 * WAVES) void convt16_kernel(const ct_args a) {
    EEG_LDS_BASE(float, red);                                               // [WAVES][MT][pixel 16][co 16]
    const int lane = threadIdx.x & 63, wave = wave_uniform((int)(threadIdx.x >> 6));
    const int fr = lane & 15, g = lane >> 4;
    const int phase = blockIdx.z, py = phase >> 1, px = phase & 1;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16 * MT;
    const int nch = a.Cin / 64, nib = (a.mask >> (4 * phase)) & 15;
    const int Hp = a.Hi + 2, Wp = a.Wi + 2, hw = a.Hi * a.Wi;
    const int last = nib & 8 ? 4 : nib & 4 ? 3 : nib & 2 ? 2 : 1;           // chunk slots past the last live tap are never visited
    const unsigned short* wp = a.W + ((long long)(phase * a.Cout + n0 + fr) * 4) * a.Cin + 16 * g;
    const unsigned short* xp[MT];
    bool live[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int q = m0 + 16 * j + fr;
        live[j] = q < a.M;                                                 // pixels past M: zeros, never read
        const int qq = live[j] ? q : 0;
        const int n_ = qq / hw, rem = qq - n_ * hw, y = rem / a.Wi, x = rem - y * a.Wi;
        xp[j] = a.in + (((long long)n_ * Hp + y + 1) * Wp + x + 1) * a.Cin + 16 * g;
    }
    const bf16x8 zero{0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int slots = last * nch;
    for (int i0 = wave; i0 < slots; i0 += WAVES * U) {
        bf16x8 w[U][2], x[U][MT][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * WAVES;
            const int tap = i / nch, c = i - tap * nch;                    // (wave-uniform)
            w[u][0] = w[u][1] = zero;
#pragma unroll
            for (int j = 0; j < MT; ++j) x[u][j][0] = x[u][j][1] = zero;
            if (i < slots && ((nib >> tap) & 1)) {
                const long long toff = ((long long)ct_delta(py, tap >> 1) * Wp + ct_delta(px, tap & 1)) * a.Cin + 64 * c;
                const unsigned short* wq = wp + (long long)tap * a.Cin + 64 * c;
                w[u][0] = *reinterpret_cast<const bf16x8*>(wq);
                w[u][1] = *reinterpret_cast<const bf16x8*>(wq + 8);
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    if (live[j]) {
                        x[u][j][0] = *reinterpret_cast<const bf16x8*>(xp[j] + toff);
                        x[u][j][1] = *reinterpret_cast<const bf16x8*>(xp[j] + toff + 8);
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)                                        // (a dead or absent slot multiplies zeros)
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                acc[j] = mma<F16>(w[u][0], x[u][j][0], acc[j]);            // D[co = 4g + r][pixel = fr]
                acc[j] = mma<F16>(w[u][1], x[u][j][1], acc[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) *reinterpret_cast<f32x4*>(red + (wave * MT + j) * 256 + fr * 16 + 4 * g) = acc[j];
    __syncthreads();
    const int Hop = 2 * a.Hi + 2, Wop = 2 * a.Wi + 2;
    for (int idx = threadIdx.x; idx < MT * 256; idx += 64 * WAVES) {
        const int j = idx >> 8, r = idx & 255, q = m0 + 16 * j + (r >> 4), co = n0 + (r & 15);
        if (q >= a.M) continue;
        float v = red[j * 256 + r];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += red[(w * MT + j) * 256 + r];
        if (a.scale) v *= a.scale[co];
        if (a.shift) v += a.shift[co];
        if (a.relu) v = fmaxf(v, 0.f);
        const int n_ = q / hw, rem = q - n_ * hw, y = rem / a.Wi, x = rem - y * a.Wi;
        a.out[(((long long)n_ * Hop + 2 * y + py + 1) * Wop + 2 * x + px + 1) * a.Cout + co] = to_h<F16>(v);
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void convt_small16_kernel(const ct_args a) {
    EEG_LDS_BASE(unsigned short, wl);                                       // [phase][Cout][tap][Cin]
    const int wn8 = 2 * a.Cout * a.Cin;                                     // 16 Cout Cin elements in vectors of 8
    for (int i = threadIdx.x; i < wn8; i += 256) reinterpret_cast<u16x8*>(wl)[i] = reinterpret_cast<const u16x8*>(a.W)[i];
    __syncthreads();
    const int Ho = 2 * a.Hi, Wo = 2 * a.Wi, Hp = a.Hi + 2, Wp = a.Wi + 2;
    const long long total = (long long)a.N * a.Cout * Ho * Wo;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int ox = (int)(q % Wo);
        const long long q1 = q / Wo;
        const int oy = (int)(q1 % Ho);
        const long long q2 = q1 / Ho;
        const int co = (int)(q2 % a.Cout), n_ = (int)(q2 / a.Cout);
        const int py = oy & 1, px = ox & 1, y = oy >> 1, x = ox >> 1, phase = 2 * py + px;
        float acc = 0.f;
        for (int tap = 0; tap < 4; ++tap) {
            if (!((a.mask >> (4 * phase + tap)) & 1)) continue;
            const unsigned short* p = a.in + (((long long)n_ * Hp + y + 1 + ct_delta(py, tap >> 1)) * Wp + x + 1 + ct_delta(px, tap & 1)) * a.Cin;
            const unsigned short* w = wl + ((phase * a.Cout + co) * 4 + tap) * a.Cin;
            for (int ci = 0; ci < a.Cin; ci += 8) {
                const u16x8 pv = *reinterpret_cast<const u16x8*>(p + ci), wv = *reinterpret_cast<const u16x8*>(w + ci);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += to_f32<F16>(pv[e]) * to_f32<F16>(wv[e]);
            }
        }
        if (a.scale) acc *= a.scale[co];
        if (a.shift) acc += a.shift[co];
        if (a.relu) acc = fmaxf(acc, 0.f);
        a.out[q] = to_h<F16>(acc);
    }
}

}  // namespace eeg

using namespace eeg;

constexpr int CT_SMALL_LDS = 64 * 1024;     // the direct form's packed weights: 16 Cout Cin 16-bit elements

static int ct_check(const eegclip_convt16_desc* d) {
    if (!d || !d->in || !d->W || !d->out || d->N < 1 || d->Hi < 1 || d->Wi < 1 || d->Cin < 64 || d->Cin % 64 || d->Cout < 1 || d->KS != 4 || d->stride != 2 ||
        d->pad != 1 || (d->relu != 0 && d->relu != 1) || !half_dtype_ok(d->dtype))
        return EEGCLIP_EINVAL;
    if (d->Hi > 16384 || d->Wi > 16384 || d->Ho != 2 * d->Hi || d->Wo != 2 * d->Wi) return EEGCLIP_EINVAL;
    if (d->Cout >= 16 ? d->Cout % 16 != 0 : (long long)32 * d->Cout * d->Cin > CT_SMALL_LDS) return EEGCLIP_EINVAL;
    if ((long long)d->N * d->Hi * d->Wi > 0x7fffffffLL / 4) return EEGCLIP_EINVAL;
    // the mask names taps of the 4 phases only and keeps every tap that some pixel of the launch needs
    int need = 0;
    for (int phase = 0; phase < 4; ++phase)
        for (int tap = 0; tap < 4; ++tap)
            if (!((tap >> 1) && d->Hi == 1) && !((tap & 1) && d->Wi == 1)) need |= 1 << (4 * phase + tap);
    if ((d->tap_mask & ~0xffff) || (d->tap_mask & need) != need) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->out) & 1u) || ((reinterpret_cast<uintptr_t>(d->scale) | reinterpret_cast<uintptr_t>(d->shift)) & 3u)) return EEGCLIP_EALIGN;
    return 0;
}

template <bool F16>
static int ct_launch(const ct_args& a, void* stream) {
    if (a.Cout < 16) {
        long long g = ((long long)a.N * a.Cout * 4 * a.Hi * a.Wi + 255) / 256;
        if (g > 16384) g = 16384;
        EEG_LAUNCH((convt_small16_kernel<F16>), dim3((unsigned)g), dim3(256), (size_t)32 * a.Cout * a.Cin, stream, a);
        return 0;
    }
    // few pixels: the weight is the traffic, 16 K-splitting waves keep its loads in flight; many pixels: a weight fragment serves 64 of them
    const bool wide = a.M > 64;
    const int mt = (a.M + (wide ? 63 : 15)) / (wide ? 64 : 16);
    if (mt > 65535) return EEGCLIP_EINVAL;
    const dim3 grid((unsigned)(a.Cout / 16), (unsigned)mt, 4);
    if (wide) EEG_LAUNCH((convt16_kernel<F16, 8, 4, 2>), grid, dim3(512), 8 * 4 * 1024, stream, a);
    else      EEG_LAUNCH((convt16_kernel<F16, 16, 1, 4>), grid, dim3(1024), 16 * 1024, stream, a);
    return 0;
}

extern "C" int eegclip_convt16(const eegclip_convt16_desc* d, void* stream) {
    if (const int rc = ct_check(d)) return rc;
    const ct_args a{static_cast<const unsigned short*>(d->in), static_cast<const unsigned short*>(d->W), static_cast<unsigned short*>(d->out), d->scale, d->shift,
                    d->N, d->Hi, d->Wi, d->Cin, d->Cout, d->N * d->Hi * d->Wi, d->relu, d->tap_mask};
    const int rc = d->dtype == EEGCLIP_DT_F16 ? ct_launch<true>(a, stream) : ct_launch<false>(a, stream);
    return rc ? rc : (int)hipGetLastError();
}
