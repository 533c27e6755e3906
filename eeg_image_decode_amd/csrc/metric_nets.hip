// The feature nets of the reference's metrics table (its notebooks under Generation/, which copy MindEye's Reconstruction_Metrics: the AlexNet(2) / AlexNet(5)
// rows are two-way identification on torchvision AlexNet's `features.4` / `features.11`): convolution + bias + ReLU, MaxPool2d(3, 2) and the NCHW -> frame
// pack, on 16-bit activations with fp32 accumulation.
//
// Layout: csrc/vae.hip's PADDED NHWC frames -- [image][H + 2 pad][W + 2 pad][C], 16-bit, the border zero and never written -- with the border as wide as the
// next layer's padding (2 in front of the 5 x 5 layer, 1 in front of a 3 x 3 layer, 0 in front of a pool), so a tap is a constant pixel offset.
// The convolution is vae.hip's implicit GEMM (M = pixels, N = Cout, K = taps x channels; 128 pixels per workgroup, 64-k tiles by LDS-DMA into XOR-swizzled
// rows, two stages, four producer waves that issue every DMA and four MFMA waves on v_mfma_f32_32x32x16_{f16,bf16}) with two differences: the N tile is 128
// or 64 wide (Cout = 64 and 192 are whole 64-wide tiles: no masked columns), and the k order is general -- (ky, kx, 64-channel run) for the layers with
// Cin % 64 == 0, and for the 3-channel 11 x 11 stride-4 layer ONE k-tile per ky: its input frame has 4 channels per pixel (the fourth is zero), so the 11 taps
// of a row are 44 contiguous elements and the k-tile is the 16 pixels (64 elements) from the window's left edge; the packed weight is [Cout][11][64] with
// k = 4 kx + c and zeros at c = 3 and kx >= 11.  The frame's rows are wide enough for the last window's 16 pixels (eegclip_convrelu16_in_width), so what the
// zero weights meet is always a frame element: zero, or a pixel -- which must be finite: an Inf or NaN within 5 pixels right of a window reaches that window's
// outputs as NaN (0 x Inf), where a convolution proper would not read it.
#include "half16.h"

namespace eeg {

constexpr int MN_T = 128, MN_K = 64;
constexpr int MN_ROWB = 2 * MN_K;                            // bytes per LDS row
constexpr int MN_A_B = MN_T * MN_ROWB;                       // the pixel tile of a stage; the weight tile (64 NJ rows) follows it

struct mn_args {
    const unsigned short* in;          // input frame, pixel (0, 0) of image 0
    const unsigned short* W;           // [Cout][KH * KW * kc]
    const unsigned short* bias;        // [Cout]
    unsigned short* out;               // output frame, pixel (0, 0) of image 0
    int Ho, Wo, Hp, Wp, pix;           // output size; input frame and its elements per pixel
    int Hop, Wop, opad, Cout;
    int KH, KW, kc, stride;            // k-tile kt = ((ky KW + kx) kc + c0) / 64 reads 64 elements from frame pixel (y stride + ky, x stride + kx), element c0
    int M, tiles_n, ntiles, chunk;
};

// NJ: 32-column blocks per MFMA wave along N; the N tile is 64 NJ wide
template <bool F16, int NJ>
__global__ __launch_bounds__(512) void convrelu16_kernel(const mn_args a) {
    EEG_LDS_BASE(unsigned char, lds);
    constexpr int TN = 64 * NJ, STAGE_B = MN_A_B + TN * MN_ROWB;
    const int logical = (int)(blockIdx.x & 7) * a.chunk + (int)(blockIdx.x >> 3);
    if (logical >= a.ntiles) return;
    const int m0 = (logical / a.tiles_n) * MN_T, n0 = (logical % a.tiles_n) * TN;
    const int t = threadIdx.x, lane = t & 63, wave_ = wave_uniform(t >> 6);
    const int wave = wave_ & 3;                               // index among the MFMA waves / among the DMA waves
    const int hw = a.Ho * a.Wo;
    const int ktiles = a.KH * a.KW * (a.kc / MN_K);
    auto swz = [](int row) { return (row >> 1) & 7; };
    if (wave_ >= 4) {
        // ---- producers: DMA wave w deposits pixel rows 32 w .. 32 w + 31 and weight rows 16 NJ w .. of every stage, 8 rows (1 KB) per instruction
        const int drow = lane >> 3, dpos = lane & 7;
        int pbase[4];
        const unsigned short* wsrc[2 * NJ];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 32 * wave + 8 * i + drow;
            const int m = m0 + row < a.M ? m0 + row : a.M - 1;      // rows beyond M: a clamped copy that nobody stores
            const int n_ = m / hw, rem = m - n_ * hw, y = rem / a.Wo, x = rem - y * a.Wo;
            pbase[i] = ((n_ * a.Hp + y * a.stride) * a.Wp + x * a.stride) * a.pix + 8 * (dpos ^ swz(row));
        }
#pragma unroll
        for (int i = 0; i < 2 * NJ; ++i) {
            const int row = 16 * NJ * wave + 8 * i + drow;
            wsrc[i] = a.W + (long long)(n0 + row) * ktiles * MN_K + 8 * (dpos ^ swz(row));
        }
        int t_ky = 0, t_kx = 0, t_c0 = 0;                     // the k-tile the next issue() fetches
        auto issue = [&](int kt) {
            unsigned char* st = lds + (kt & 1) * STAGE_B;
            const int off = (t_ky * a.Wp + t_kx) * a.pix + t_c0;
#pragma unroll
            for (int i = 0; i < 4; ++i) lds_dma16(st + (32 * wave + 8 * i) * MN_ROWB, a.in + pbase[i] + off);
#pragma unroll
            for (int i = 0; i < 2 * NJ; ++i) lds_dma16(st + MN_A_B + (16 * NJ * wave + 8 * i) * MN_ROWB, wsrc[i] + (long long)kt * MN_K);
            t_c0 += MN_K;
            if (t_c0 == a.kc) {
                t_c0 = 0;
                if (++t_kx == a.KW) { t_kx = 0; ++t_ky; }
            }
        };
        issue(0);
        for (int kt = 0; kt < ktiles; ++kt) {
            wait_vmcnt<0>();
            raw_barrier();                                    // tile kt is in LDS; every MFMA wave has read tile kt - 1, whose stage the next issue overwrites
            if (kt + 1 < ktiles) issue(kt + 1);
        }
        return;                                               // (the epilogue has no barrier)
    }
    const int wm = wave >> 1, wn = wave & 1;
    const int r32 = lane & 31, h = lane >> 5;
    f32x16 acc[NJ][2];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
    int fom[4][2], fon[4][NJ];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rm = wm * 64 + 32 * i + r32;
            fom[s][i] = rm * MN_ROWB + (((2 * s + h) ^ swz(rm)) & 7) * 16;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int rn = wn * 32 * NJ + 32 * j + r32;
            fon[s][j] = MN_A_B + rn * MN_ROWB + (((2 * s + h) ^ swz(rn)) & 7) * 16;
        }
    }
    for (int kt = 0; kt < ktiles; ++kt) {
        raw_barrier();
        const unsigned char* st = lds + (kt & 1) * STAGE_B;
        bf16x8 am[2][2], wf[2][NJ];
        // (what a step's first MFMA takes is read last and the next step's reads go out behind that MFMA: csrc/vae.hip)
        auto read_step = [&](int s, int set) {
#pragma unroll
            for (int i = 1; i >= 0; --i) am[set][i] = *reinterpret_cast<const bf16x8*>(st + fom[s][i]);
#pragma unroll
            for (int j = NJ - 1; j >= 0; --j) wf[set][j] = *reinterpret_cast<const bf16x8*>(st + fon[s][j]);
        };
        read_step(0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sched_fence();
            const int set = s & 1;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    acc[j][i] = mma32<F16>(wf[set][j], am[set][i], acc[j][i]);
                    if (j == 0 && i == 0 && s + 1 < 4) {
                        sched_fence();
                        read_step(s + 1, (s + 1) & 1);
                        sched_fence();
                    }
                }
            sched_fence();
        }
    }
    // ---- epilogue: lane (r32, h) owns pixel m = m0 + 64 wm + 32 i + r32; registers 4 eq .. 4 eq + 3 of n block j are channels n0 + 32 NJ wn + 32 j + 8 eq + 4 h ..
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + 32 * i + r32;
        if (m >= a.M) continue;
        const int n_ = m / hw, rem = m - n_ * hw, y = rem / a.Wo, x = rem - y * a.Wo;
        const long long opix = (((long long)n_ * a.Hop + y + a.opad) * a.Wop + x + a.opad) * a.Cout;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int eq = 0; eq < 4; ++eq) {
                const int n = n0 + wn * 32 * NJ + 32 * j + 8 * eq + 4 * h;
                const u16x4 bv = *reinterpret_cast<const u16x4*>(a.bias + n);
                u16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = acc[j][i][4 * eq + e] + to_f32<F16>(bv[e]);
                    o[e] = to_h<F16>(v < 0.f ? 0.f : v);      // ReLU (a NaN stays a NaN)
                }
                *reinterpret_cast<u16x4*>(a.out + opix + n) = o;
            }
    }
}

// ---- MaxPool2d(3, 2), floor mode, no padding: thread = (output pixel, 8 consecutive channels), 16-byte reads and one 16-byte store.  The running maximum
// starts from the first tap (the input may be negative everywhere); a NaN tap wins, as in torch.
template <bool F16>
__global__ __launch_bounds__(256) void maxpool16_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int N, int H, int W, int C,
                                                        int ipad, int opad, int Ho, int Wo) {
    const int c8n = C / 8, Hp = H + 2 * ipad, Wp = W + 2 * ipad, Hop = Ho + 2 * opad, Wop = Wo + 2 * opad;
    const long long total = (long long)N * Ho * Wo * c8n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 8 * (int)(q % c8n);
        const long long pq = q / c8n;
        const int x = (int)(pq % Wo), y = (int)((pq / Wo) % Ho), n_ = (int)(pq / ((long long)Wo * Ho));
        const unsigned short* src = in + (((long long)n_ * Hp + 2 * y + ipad) * Wp + 2 * x + ipad) * C + c;
        u16x8 best = *reinterpret_cast<const u16x8*>(src);
#pragma unroll
        for (int tap = 1; tap < 9; ++tap) {
            const u16x8 v = *reinterpret_cast<const u16x8*>(src + ((long long)(tap / 3) * Wp + tap % 3) * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = to_f32<F16>(v[e]), b = to_f32<F16>(best[e]);
                if (f > b || f != f) best[e] = v[e];
            }
        }
        *reinterpret_cast<u16x8*>(out + (((long long)n_ * Hop + y + opad) * Wop + x + opad) * C + c) = best;
    }
}

// ---- (N, 3, H, W) planes -> the first layer's frame [N][H + 4][Wf][4]: pixel (y, x) at frame (y + 2, x + 2) as {c0, c1, c2, 0}; a copy of 16-bit patterns
__global__ __launch_bounds__(256) void pack_nchw16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ frame, int N, int H, int W, int Wf) {
    const long long hw = (long long)H * W, total = N * hw;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const long long n_ = q / hw, p = q - n_ * hw;
        const int y = (int)(p / W), xx = (int)(p - (long long)y * W);
        const unsigned short* s = x + n_ * 3 * hw + p;
        const u16x4 v{s[0], s[hw], s[2 * hw], 0};
        *reinterpret_cast<u16x4*>(frame + ((n_ * (H + 4) + y + 2) * Wf + xx + 2) * 4) = v;
    }
}

// torchvision AlexNet's five convolutions (torchvision/models/alexnet.py): the only shapes eegclip_convrelu16 takes
struct mn_layer { int KS, stride, pad, Cin, Cout; };
static const mn_layer MN_LAYERS[5] = {{11, 4, 2, 3, 64}, {5, 1, 2, 64, 192}, {3, 1, 1, 192, 384}, {3, 1, 1, 384, 256}, {3, 1, 1, 256, 256}};

static int mn_in_width(int Wi) {
    const int Wo = (Wi + 4 - 11) / 4 + 1;
    int w = 4 * (Wo - 1) + 16;                               // the last window's k-tile: 16 pixels from its left edge
    if (w < Wi + 4) w = Wi + 4;
    return (w + 1) & ~1;                                     // even: every row starts at a 16-byte boundary
}

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_convrelu16_in_width(int Wi) { return Wi < 7 ? EEGCLIP_EINVAL : mn_in_width(Wi); }

extern "C" int eegclip_convrelu16(const eegclip_convrelu16_desc* d, void* stream) {
    if (!d || !d->in || !d->W || !d->bias || !d->out || d->N < 1 || d->Hi < 1 || d->Wi < 1 || d->out_pad < 0 || d->out_pad > 2 || !half_dtype_ok(d->dtype))
        return EEGCLIP_EINVAL;
    const mn_layer* L = nullptr;
    for (const mn_layer& l : MN_LAYERS)
        if (l.KS == d->KS && l.stride == d->stride && l.pad == d->pad && l.Cin == d->Cin && l.Cout == d->Cout) L = &l;
    if (!L || d->Hi + 2 * L->pad < L->KS || d->Wi + 2 * L->pad < L->KS) return EEGCLIP_EINVAL;
    const int Ho = (d->Hi + 2 * L->pad - L->KS) / L->stride + 1, Wo = (d->Wi + 2 * L->pad - L->KS) / L->stride + 1;
    const bool first = L->Cin == 3;
    mn_args a;
    a.in = static_cast<const unsigned short*>(d->in);
    a.W = static_cast<const unsigned short*>(d->W);
    a.bias = static_cast<const unsigned short*>(d->bias);
    a.out = static_cast<unsigned short*>(d->out);
    a.Ho = Ho; a.Wo = Wo;
    a.Hp = d->Hi + 2 * L->pad;                               // (the frame's border IS the layer's padding: every tap of every window is a frame pixel)
    a.Wp = first ? mn_in_width(d->Wi) : d->Wi + 2 * L->pad;
    a.pix = first ? 4 : L->Cin;
    a.Hop = Ho + 2 * d->out_pad; a.Wop = Wo + 2 * d->out_pad; a.opad = d->out_pad; a.Cout = L->Cout;
    a.KH = L->KS; a.KW = first ? 1 : L->KS; a.kc = first ? MN_K : L->Cin; a.stride = L->stride;
    const long long M = (long long)d->N * Ho * Wo;
    // (the kernel's element offsets into the input frame are 32-bit)
    if (M > 0x7fffffffLL || (long long)d->N * a.Hp * a.Wp * a.pix > 0x7fffffffLL) return EEGCLIP_EINVAL;
    a.M = (int)M;
    if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->bias)) & 7u) return EEGCLIP_EALIGN;
    const int nj = L->Cout % 128 == 0 ? 2 : 1;
    a.tiles_n = L->Cout / (64 * nj);
    a.ntiles = a.tiles_n * ((a.M + MN_T - 1) / MN_T);
    a.chunk = (a.ntiles + 7) / 8;
    const size_t lds = 2 * (size_t)(MN_A_B + 64 * nj * MN_ROWB);
    const dim3 grid((unsigned)(8 * a.chunk)), block(512);
    const bool f16 = d->dtype == EEGCLIP_DT_F16;
    if (nj == 2) {
        if (f16) EEG_LAUNCH((convrelu16_kernel<true, 2>), grid, block, lds, stream, a);
        else     EEG_LAUNCH((convrelu16_kernel<false, 2>), grid, block, lds, stream, a);
    } else {
        if (f16) EEG_LAUNCH((convrelu16_kernel<true, 1>), grid, block, lds, stream, a);
        else     EEG_LAUNCH((convrelu16_kernel<false, 1>), grid, block, lds, stream, a);
    }
    return (int)hipGetLastError();
}

extern "C" int eegclip_maxpool16(const void* in, void* out, int N, int H, int W, int C, int in_pad, int out_pad, int dtype, void* stream) {
    if (!in || !out || N < 1 || H < 3 || W < 3 || C < 8 || C % 8 || in_pad < 0 || in_pad > 2 || out_pad < 0 || out_pad > 2 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) return EEGCLIP_EALIGN;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    long long g = ((long long)N * Ho * Wo * (C / 8) + 255) / 256;
    if (g > 16384) g = 16384;
    const unsigned short* i16 = static_cast<const unsigned short*>(in);
    unsigned short* o16 = static_cast<unsigned short*>(out);
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((maxpool16_kernel<true>), dim3((unsigned)g), dim3(256), 0, stream, i16, o16, N, H, W, C, in_pad, out_pad, Ho, Wo);
    else                         EEG_LAUNCH((maxpool16_kernel<false>), dim3((unsigned)g), dim3(256), 0, stream, i16, o16, N, H, W, C, in_pad, out_pad, Ho, Wo);
    return (int)hipGetLastError();
}

extern "C" int eegclip_pack_nchw16(const void* x, void* frame, int N, int H, int W, int dtype, void* stream) {
    if (!x || !frame || N < 1 || H < 7 || W < 7 || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) & 1u) || (reinterpret_cast<uintptr_t>(frame) & 15u)) return EEGCLIP_EALIGN;
    long long g = ((long long)N * H * W + 255) / 256;
    if (g > 16384) g = 16384;
    EEG_LAUNCH(pack_nchw16_kernel, dim3((unsigned)g), dim3(256), 0, stream, static_cast<const unsigned short*>(x), static_cast<unsigned short*>(frame), N, H, W,
               mn_in_width(W));
    return (int)hipGetLastError();
}
