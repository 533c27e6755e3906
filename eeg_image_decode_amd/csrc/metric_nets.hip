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
//
// The SwAV row's ResNet-50 trunk (torchvision's Bottleneck ResNet v1.5 up to `avgpool`) runs on the same convolution kernel with a second epilogue
// (eegclip_convbn16: eval-mode BatchNorm as fp32 scale / shift, the block's residual added in fp32, ReLU or not) for 1 x 1 and 3 x 3 layers at stride 1 or 2 and
// the 3-channel 7 x 7 stride-2 stem in the form above (a 3-pixel border, [64][7][64] weights; the 9 pixels right of a window must be finite), with
// MaxPool2d(3, 2, 1), the average pool to fp32 (N, C) and scipy's correlation distance per pair of feature rows.
//
// The EffNet-B row's EfficientNet-B1 trunk takes its dense layers from a third epilogue of the same kernel (eegclip_convbnact16: scale / shift, then none | ReLU |
// SiLU in fp32, THEN the residual): the 1 x 1 expansions, projections and head at Cin, Cout % 64 == 0 -- the host pads 16, 24, 40 .. channels with zeros -- and
// the 3-channel 3 x 3 stride-2 stem in the first-layer form (a 1-pixel border, [64][3][64] weights of which EfficientNet fills 32 rows).  The depthwise layers,
// the squeeze-and-excitation gate and the gate multiply are csrc/mbconv.hip.
//
// The Inception row's InceptionV3 trunk (torchvision's Inception3 up to `avgpool`) is a fourth epilogue (eegclip_convbncat16: scale / shift / ReLU written into
// channels oc0 .. oc0 + Cout - 1 of a frame with `ostride` channels per pixel): a block's branches write their slices of ONE output frame, so nothing is
// concatenated.  The tile loop is the same -- it walks KH and KW separately, so 1 x 7, 7 x 1, 1 x 3 and 3 x 1 layers and per-axis padding are host geometry: the
// frame walk starts at pixel (in_pad - pad_h, in_pad - pad_w) -- and the N tiles cover pad64(Cout) weight rows, of which the epilogue stores the groups below Cout.
// With it: the 3 x 3 stride-1 average pool of every block, MaxPool2d(3, 2) as a branch of a concatenation, and the pack with transform_input's affine.
//
// The host half is shared by the four rows: one mn_geometry fills the tile loop's arguments for every convolution entry point (each keeps its own whitelist of
// shapes and its alignment rules), the four 3-channel first layers are one table (MN_FIRST), MaxPool2d(3, 2) is one kernel on a channel slice (a whole frame is
// the widest slice), the four packs are one kernel with a runtime border and an optional affine, and MN_ELEMENTWISE picks an elementwise kernel's f16 / bf16
// instantiation.  convrelu16_kernel and its four argument types are NOT part of that folding: each row has a type of its own so that the earlier rows'
// instantiations stay instruction for instruction what they were.
#include "silu16.h"

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
    static constexpr bool BN = false;  // the epilogue: bias + ReLU
    static constexpr bool ACT = false; // (eegclip_convbnact16's epilogue)
    static constexpr bool CAT = false; // (eegclip_convbncat16's epilogue)
};

// eegclip_convbn16's arguments: the same tile loop with the epilogue act(scale[co] acc + shift[co] + residual).  A type of its own, so the kernel argument
// block of the bias + ReLU instantiations stays what it was.
struct mn_bn_args : mn_args {
    const float* scale;                // [Cout]
    const float* shift;                // [Cout]
    const unsigned short* residual;    // NULL, or a frame in the output's own layout
    int relu;
    static constexpr bool BN = true;
};

// eegclip_convbnact16's arguments (the EfficientNet row): act(scale[co] acc + shift[co]) + residual, act = 0 none | 1 ReLU | 2 SiLU.  Again a type of its own:
// the two epilogues above keep their instantiations.
struct mn_act_args : mn_args {
    const float* scale;                // [Cout]
    const float* shift;                // [Cout]
    const unsigned short* residual;    // NULL, or a frame in the output's own layout
    int act;
    static constexpr bool BN = true, ACT = true;
};

// eegclip_convbncat16's arguments (the Inception row): relu?(scale[co] acc + shift[co]) written into channels oc0 .. oc0 + Cout - 1 of a frame whose pixels are
// `ostride` elements apart -- one branch's slice of a block's concatenated output.  `Cout` is the layer's own count (a multiple of 8); the N tiles cover
// pad64(Cout) weight rows and the epilogue skips the store groups at or past Cout.  A type of its own once more: the three epilogues above keep theirs.
struct mn_cat_args : mn_args {
    const float* scale;                // [pad64(Cout)]
    const float* shift;                // [pad64(Cout)]
    int relu, ostride, oc0;
    static constexpr bool BN = true, CAT = true;
};

// NJ: 32-column blocks per MFMA wave along N; the N tile is 64 NJ wide
template <bool F16, int NJ, class ARGS>
__global__ __launch_bounds__(512) void convrelu16_kernel(const ARGS a) {
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
        long long opix = ((long long)n_ * a.Hop + y + a.opad) * a.Wop + x + a.opad;
        if constexpr (ARGS::CAT) opix = opix * a.ostride + a.oc0;
        else opix *= a.Cout;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int eq = 0; eq < 4; ++eq) {
                const int n = n0 + wn * 32 * NJ + 32 * j + 8 * eq + 4 * h;
                u16x4 o;
                if constexpr (ARGS::CAT) {
                    // the slice's mask: Cout % 8 == 0, so the two 4-channel groups of an 8-channel run (h = 0, 1) are inside or outside together and the
                    // test is the same in every lane of the wave; nothing outside the slice is stored
                    if (n - 4 * h >= a.Cout) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[j][i][4 * eq + e] * a.scale[n + e] + a.shift[n + e];
                        o[e] = to_h<F16>(a.relu && v < 0.f ? 0.f : v);
                    }
                } else if constexpr (ARGS::ACT) {
                    // eval-mode BatchNorm as fp32 scale / shift, the activation in fp32, THEN the residual (MBConv's projection has none of the former, its
                    // expansion none of the latter), one rounding at the store
                    u16x4 rv{0, 0, 0, 0};
                    if (a.residual) rv = *reinterpret_cast<const u16x4*>(a.residual + opix + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = acc[j][i][4 * eq + e] * a.scale[n + e] + a.shift[n + e];
                        if (a.act == 2) v = silu_exp2(v);
                        else if (a.act == 1) v = v < 0.f ? 0.f : v;
                        if (a.residual) v += to_f32<F16>(rv[e]);
                        o[e] = to_h<F16>(v);
                    }
                } else if constexpr (ARGS::BN) {
                    // eval-mode BatchNorm as fp32 scale / shift, the residual added in fp32, one rounding at the store
                    u16x4 rv{0, 0, 0, 0};
                    if (a.residual) rv = *reinterpret_cast<const u16x4*>(a.residual + opix + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = acc[j][i][4 * eq + e] * a.scale[n + e] + a.shift[n + e];
                        if (a.residual) v += to_f32<F16>(rv[e]);
                        o[e] = to_h<F16>(a.relu && v < 0.f ? 0.f : v);
                    }
                } else {
                    const u16x4 bv = *reinterpret_cast<const u16x4*>(a.bias + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[j][i][4 * eq + e] + to_f32<F16>(bv[e]);
                        o[e] = to_h<F16>(v < 0.f ? 0.f : v);      // ReLU (a NaN stays a NaN)
                    }
                }
                *reinterpret_cast<u16x4*>(a.out + opix + n) = o;
            }
    }
}

// ---- MaxPool2d(3, 2), floor mode, no padding, on a channel slice: it reads the first C channels of a frame whose pixels are `istride` elements apart and
// writes channels oc0 .. oc0 + C - 1 of the interior of a frame with `ostride` elements per pixel; nothing else is written.  A whole frame is the slice
// istride = ostride = C, oc0 = 0 (eegclip_maxpool16); Inception's Mixed_6a / Mixed_7a pool the block's input into their branch of the concatenation
// (eegclip_maxpool16_cat).  thread = (output pixel, 8 consecutive channels), 16-byte reads and one 16-byte store.  The running maximum starts from the first
// tap (the input may be negative everywhere); a NaN tap wins, as in torch.
template <bool F16>
__global__ __launch_bounds__(256) void maxpool16_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int N, int H, int W, int C,
                                                        int istride, int ipad, int ostride, int oc0, int opad, int Ho, int Wo) {
    const int c8n = C / 8, Hp = H + 2 * ipad, Wp = W + 2 * ipad, Hop = Ho + 2 * opad, Wop = Wo + 2 * opad;
    const long long total = (long long)N * Ho * Wo * c8n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 8 * (int)(q % c8n);
        const long long pq = q / c8n;
        const int x = (int)(pq % Wo), y = (int)((pq / Wo) % Ho), n_ = (int)(pq / ((long long)Wo * Ho));
        const unsigned short* src = in + (((long long)n_ * Hp + 2 * y + ipad) * Wp + 2 * x + ipad) * istride + c;
        u16x8 best = *reinterpret_cast<const u16x8*>(src);
#pragma unroll
        for (int tap = 1; tap < 9; ++tap) {
            const u16x8 v = *reinterpret_cast<const u16x8*>(src + ((long long)(tap / 3) * Wp + tap % 3) * istride);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = to_f32<F16>(v[e]), b = to_f32<F16>(best[e]);
                if (f > b || f != f) best[e] = v[e];
            }
        }
        *reinterpret_cast<u16x8*>(out + (((long long)n_ * Hop + y + opad) * Wop + x + opad) * ostride + oc0 + c) = best;
    }
}

// ---- F.avg_pool2d(x, 3, 1, 1) with count_include_pad=True (the pooled branch of every Inception block): the frame's zero border (ipad >= 1) is read, not
// tested for; the nine taps are added in fp32 in (ky, kx) order and divided by 9, one rounding at the store into the UNPADDED frame [N][H][W][C].
// thread = (pixel, 8 consecutive channels), 16-byte accesses.
template <bool F16>
__global__ __launch_bounds__(256) void avgpool3x3_16_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int N, int H, int W, int C,
                                                            int ipad) {
    const int c8n = C / 8, Hp = H + 2 * ipad, Wp = W + 2 * ipad;
    const long long total = (long long)N * H * W * c8n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 8 * (int)(q % c8n);
        const long long pq = q / c8n;
        const int x = (int)(pq % W), y = (int)((pq / W) % H), n_ = (int)(pq / ((long long)W * H));
        const unsigned short* src = in + (((long long)n_ * Hp + y + ipad - 1) * Wp + x + ipad - 1) * C + c;
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const u16x8 v = *reinterpret_cast<const u16x8*>(src + ((long long)(tap / 3) * Wp + tap % 3) * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += to_f32<F16>(v[e]);
        }
        u16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = to_h<F16>(s[e] / 9.f);
        *reinterpret_cast<u16x8*>(out + pq * C + c) = o;
    }
}

// ---- MaxPool2d(3, 2, padding=1), floor mode (ResNet's): the same thread shape.  A tap outside the image is skipped, not read (the frame's border, if any,
// holds zeros, which would beat an all-negative window); the centre tap is always inside, so every window has a first tap.  Taps are visited in torch's
// order and a later tap replaces the maximum only when larger (or NaN): the stored pattern is the largest tap's own.
template <bool F16>
__global__ __launch_bounds__(256) void maxpool16_pad_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int N, int H, int W, int C,
                                                            int ipad, int opad, int Ho, int Wo) {
    const int c8n = C / 8, Hp = H + 2 * ipad, Wp = W + 2 * ipad, Hop = Ho + 2 * opad, Wop = Wo + 2 * opad;
    const long long total = (long long)N * Ho * Wo * c8n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 8 * (int)(q % c8n);
        const long long pq = q / c8n;
        const int x = (int)(pq % Wo), y = (int)((pq / Wo) % Ho), n_ = (int)(pq / ((long long)Wo * Ho));
        u16x8 best{0, 0, 0, 0, 0, 0, 0, 0};
        bool have = false;
        for (int tap = 0; tap < 9; ++tap) {
            const int ty = 2 * y - 1 + tap / 3, tx = 2 * x - 1 + tap % 3;
            if (ty < 0 || ty >= H || tx < 0 || tx >= W) continue;
            const u16x8 v = *reinterpret_cast<const u16x8*>(in + (((long long)n_ * Hp + ty + ipad) * Wp + tx + ipad) * C + c);
            if (!have) {
                best = v;
                have = true;
                continue;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = to_f32<F16>(v[e]), b = to_f32<F16>(best[e]);
                if (f > b || f != f) best[e] = v[e];
            }
        }
        *reinterpret_cast<u16x8*>(out + (((long long)n_ * Hop + y + opad) * Wop + x + opad) * C + c) = best;
    }
}

// ---- the mean over the H W pixels of an unpadded frame [N][HW][C] -> fp32 [N][C]: thread = (image, 8 consecutive channels), the pixels added in fp32 in
// their order and divided once.  No atomics: bit-reproducible.
template <bool F16>
__global__ __launch_bounds__(256) void avgpool16_kernel(const unsigned short* __restrict__ in, float* __restrict__ out, int N, int HW, int C) {
    const int c8n = C / 8;
    const long long total = (long long)N * c8n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 8 * (int)(q % c8n);
        const long long n_ = q / c8n;
        const unsigned short* src = in + n_ * HW * C + c;
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < HW; ++p) {
            const u16x8 v = *reinterpret_cast<const u16x8*>(src + (long long)p * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += to_f32<F16>(v[e]);
        }
        const float cnt = (float)HW;
#pragma unroll
        for (int e = 0; e < 8; ++e) out[n_ * C + c + e] = s[e] / cnt;
    }
}

// ---- scipy.spatial.distance.correlation per pair of rows: one 256-thread workgroup per pair, two passes (the means, then the three centred sums), each
// thread's strided partial sums combined by a shuffle tree within the wave and an LDS tree across the four waves: a fixed order, no atomics.
__device__ __forceinline__ float cd_block_sum(float v, float* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                                          // (the previous sum's readers are done with `red`)
    if (lane == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void corr_distance_kernel(const float* __restrict__ a, const float* __restrict__ b, int D, float* __restrict__ out) {
    EEG_LDS_BASE(float, red);                                 // [4]
    const float* pa = a + (long long)blockIdx.x * D;
    const float* pb = b + (long long)blockIdx.x * D;
    const int t = threadIdx.x;
    float sa = 0.f, sb = 0.f;
    for (int i = t; i < D; i += 256) {
        sa += pa[i];
        sb += pb[i];
    }
    const float ma = cd_block_sum(sa, red) / (float)D, mb = cd_block_sum(sb, red) / (float)D;
    float saa = 0.f, sbb = 0.f, sab = 0.f;
    for (int i = t; i < D; i += 256) {
        const float x = pa[i] - ma, y = pb[i] - mb;
        saa += x * x;
        sbb += y * y;
        sab += x * y;
    }
    saa = cd_block_sum(saa, red);
    sbb = cd_block_sum(sbb, red);
    sab = cd_block_sum(sab, red);
    if (t == 0) out[blockIdx.x] = 1.f - sab / (sqrtf(saa) * sqrtf(sbb));          // a constant row: 0 / 0 = NaN, as scipy gives
}

// ---- (N, 3, H, W) planes -> a 3-channel layer's frame [N][H + 2 B][Wf][4]: pixel (y, x) at frame (y + B, x + B) as {c0, c1, c2, 0}.  Without AFFINE it is a
// copy of 16-bit patterns, whatever the dtype (F16 is not looked at).  With it (torchvision Inception3's transform_input) channel c becomes a_c x_c + b_c, the
// product and the sum in fp32, one rounding; a channel with a_c = 1 and b_c = 0 is still copied as a pattern (-0 and NaN payloads included), so the identity is
// the plain pack.
template <bool AFFINE, bool F16>
__global__ __launch_bounds__(256) void pack_nchw16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ frame, const float* __restrict__ a,
                                                          const float* __restrict__ b, int N, int H, int W, int Wf, int B) {
    const long long hw = (long long)H * W, total = N * hw;
    float av[3] = {1.f, 1.f, 1.f}, bv[3] = {0.f, 0.f, 0.f};
    if constexpr (AFFINE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            av[c] = a[c];
            bv[c] = b[c];
        }
    }
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const long long n_ = q / hw, p = q - n_ * hw;
        const int y = (int)(p / W), xx = (int)(p - (long long)y * W);
        const unsigned short* s = x + n_ * 3 * hw + p;
        u16x4 v{s[0], s[hw], s[2 * hw], 0};
        if constexpr (AFFINE) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (av[c] != 1.f || bv[c] != 0.f) v[c] = to_h<F16>(av[c] * to_f32<F16>(v[c]) + bv[c]);
        }
        *reinterpret_cast<u16x4*>(frame + ((n_ * (H + 2 * B) + y + B) * Wf + xx + B) * 4) = v;
    }
}

// a convolution's filter as the tile loop sees it
struct mn_filter { int KH, KW, stride, pad_h, pad_w, Cin, Cout; };
static mn_filter mn_square(int KS, int stride, int pad, int Cin, int Cout) { return {KS, KS, stride, pad, pad, Cin, Cout}; }
static bool mn_same(const mn_filter& a, const mn_filter& b) {
    return a.KH == b.KH && a.KW == b.KW && a.stride == b.stride && a.pad_h == b.pad_h && a.pad_w == b.pad_w && a.Cin == b.Cin && a.Cout == b.Cout;
}

// the 3-channel first layer of each net -- its padding is the border of the frame the pack writes -- and the smallest image side its entry points take
enum { MN_ALEXNET, MN_RESNET, MN_EFFNET, MN_INCEPTION };
struct mn_first { mn_filter F; int min_side; };
static const mn_first MN_FIRST[4] = {
    {{11, 11, 4, 2, 2, 3, 64}, 7},     // torchvision AlexNet's features.0
    {{7, 7, 2, 3, 3, 3, 64}, 1},       // torchvision ResNet's conv1
    {{3, 3, 2, 1, 1, 3, 64}, 1},       // torchvision EfficientNet's features.0 (32 filters; rows 32 .. 63 of the packed weight are zero)
    {{3, 3, 2, 0, 0, 3, 64}, 3},       // torchvision Inception3's Conv2d_1a_3x3 (32 filters; rows 32 .. 63 of the packed weight are zero and never stored)
};
// torchvision AlexNet's other four convolutions: with features.0 the only shapes eegclip_convrelu16 takes
static const mn_filter MN_ALEXNET_BODY[4] = {{5, 5, 1, 2, 2, 64, 192}, {3, 3, 1, 1, 1, 192, 384}, {3, 3, 1, 1, 1, 384, 256}, {3, 3, 1, 1, 1, 256, 256}};

// a 3-channel layer's frame width: at least the image and its border, and the 16 pixels of the last window's k-tile; even, so every row starts at 16 bytes
static int mn_first_width(int Wi, const mn_filter& F) {
    const int Wo = (Wi + 2 * F.pad_w - F.KW) / F.stride + 1;
    int w = F.stride * (Wo - 1) + 16;
    if (w < Wi + 2 * F.pad_w) w = Wi + 2 * F.pad_w;
    return (w + 1) & ~1;
}
static int mn_in_width(int net, int Wi) { return Wi < MN_FIRST[net].min_side ? EEGCLIP_EINVAL : mn_first_width(Wi, MN_FIRST[net].F); }

static const unsigned short* mn_u16(const void* p) { return static_cast<const unsigned short*>(p); }
static unsigned short* mn_u16(void* p) { return static_cast<unsigned short*>(p); }

// what the four convolution entry points share: the tile loop's geometry for filter F on a frame with a border of B >= the padding around Hi x Wi images
// (0, or EEGCLIP_EINVAL past the kernel's 32-bit offsets).  The walk starts at frame pixel (B - pad_h, B - pad_w), so every tap of every window is a frame
// pixel: a 1 x 1 layer skips whatever border it meets, and a 1 x 7 and a 7 x 1 layer read the same border-3 frame.  A 3-channel layer (B = its padding) reads
// 4 elements per pixel, one k-tile per ky.  The N tiles cover pad64(Cout) weight rows, 64 nj at a time.
static int mn_geometry(mn_args& a, const void* in, const mn_filter& F, int N, int Hi, int Wi, int B, int out_pad, int& nj) {
    const int Ho = (Hi + 2 * F.pad_h - F.KH) / F.stride + 1, Wo = (Wi + 2 * F.pad_w - F.KW) / F.stride + 1;
    const bool first = F.Cin == 3;
    a.Ho = Ho; a.Wo = Wo;
    a.Hp = Hi + 2 * B;
    a.Wp = first ? mn_first_width(Wi, F) : Wi + 2 * B;
    a.pix = first ? 4 : F.Cin;
    a.Hop = Ho + 2 * out_pad; a.Wop = Wo + 2 * out_pad; a.opad = out_pad; a.Cout = F.Cout;
    a.KH = F.KH; a.KW = first ? 1 : F.KW; a.kc = first ? MN_K : F.Cin; a.stride = F.stride;
    const long long M = (long long)N * Ho * Wo;
    // (the kernel's element offsets into the input frame are 32-bit)
    if (M > 0x7fffffffLL || (long long)N * a.Hp * a.Wp * a.pix > 0x7fffffffLL) return EEGCLIP_EINVAL;
    a.M = (int)M;
    const int cpad = (F.Cout + 63) / 64 * 64;
    nj = cpad % 128 == 0 ? 2 : 1;
    a.tiles_n = cpad / (64 * nj);
    a.ntiles = a.tiles_n * ((a.M + MN_T - 1) / MN_T);
    a.chunk = (a.ntiles + 7) / 8;
    a.in = mn_u16(in) + ((long long)(B - F.pad_h) * a.Wp + (B - F.pad_w)) * a.pix;
    return 0;
}

// .. and the launch, N tiles of 64 nj channels
template <class ARGS>
static int mn_launch(const ARGS& a, int nj, int dtype, void* stream) {
    const size_t lds = 2 * (size_t)(MN_A_B + 64 * nj * MN_ROWB);
    const dim3 grid((unsigned)(8 * a.chunk)), block(512);
    const bool f16 = dtype == EEGCLIP_DT_F16;
    if (nj == 2) {
        if (f16) EEG_LAUNCH((convrelu16_kernel<true, 2, ARGS>), grid, block, lds, stream, a);
        else     EEG_LAUNCH((convrelu16_kernel<false, 2, ARGS>), grid, block, lds, stream, a);
    } else {
        if (f16) EEG_LAUNCH((convrelu16_kernel<true, 1, ARGS>), grid, block, lds, stream, a);
        else     EEG_LAUNCH((convrelu16_kernel<false, 1, ARGS>), grid, block, lds, stream, a);
    }
    return (int)hipGetLastError();
}

static unsigned mn_grid(long long threads) {
    const long long g = (threads + 255) / 256;
    return (unsigned)(g > 16384 ? 16384 : g);
}

// the launch of an elementwise kernel<F16> over `threads` grid-stride threads, in the dtype's instantiation
#define MN_ELEMENTWISE(kernel, dtype, threads, stream, ...)                                                                        \
    do {                                                                                                                           \
        const dim3 grid_(mn_grid(threads));                                                                                        \
        if ((dtype) == EEGCLIP_DT_F16) EEG_LAUNCH((kernel<true>), grid_, dim3(256), 0, stream, __VA_ARGS__);                       \
        else                           EEG_LAUNCH((kernel<false>), grid_, dim3(256), 0, stream, __VA_ARGS__);                      \
    } while (0)

// the four packs: net's first layer gives the frame's border and width; a, b = NULL without an affine
static int mn_pack(int net, const void* x, void* frame, bool affine, const float* a, const float* b, int N, int H, int W, int dtype, void* stream) {
    const mn_first& L = MN_FIRST[net];
    if (!x || !frame || (affine && (!a || !b)) || N < 1 || H < L.min_side || W < L.min_side || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) & 1u) || (reinterpret_cast<uintptr_t>(frame) & 15u)) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3u) return EEGCLIP_EALIGN;
    const dim3 grid(mn_grid((long long)N * H * W)), block(256);
    const int Wf = mn_first_width(W, L.F), B = L.F.pad_h;
    if (!affine)                         EEG_LAUNCH((pack_nchw16_kernel<false, false>), grid, block, 0, stream, mn_u16(x), mn_u16(frame), a, b, N, H, W, Wf, B);
    else if (dtype == EEGCLIP_DT_F16)    EEG_LAUNCH((pack_nchw16_kernel<true, true>), grid, block, 0, stream, mn_u16(x), mn_u16(frame), a, b, N, H, W, Wf, B);
    else                                 EEG_LAUNCH((pack_nchw16_kernel<true, false>), grid, block, 0, stream, mn_u16(x), mn_u16(frame), a, b, N, H, W, Wf, B);
    return (int)hipGetLastError();
}

// MaxPool2d(3, 2) of a channel slice; the callers have checked their own limits
static int mn_maxpool(const void* in, void* out, int N, int H, int W, int C, int istride, int ipad, int ostride, int oc0, int opad, int dtype, void* stream) {
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) return EEGCLIP_EALIGN;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    MN_ELEMENTWISE(maxpool16_kernel, dtype, (long long)N * Ho * Wo * (C / 8), stream, mn_u16(in), mn_u16(out), N, H, W, C, istride, ipad, ostride, oc0, opad, Ho,
                   Wo);
    return (int)hipGetLastError();
}

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_convrelu16_in_width(int Wi) { return mn_in_width(MN_ALEXNET, Wi); }

extern "C" int eegclip_convrelu16(const eegclip_convrelu16_desc* d, void* stream) {
    if (!d || !d->in || !d->W || !d->bias || !d->out || d->N < 1 || d->Hi < 1 || d->Wi < 1 || d->out_pad < 0 || d->out_pad > 2 || !half_dtype_ok(d->dtype))
        return EEGCLIP_EINVAL;
    const mn_filter F = mn_square(d->KS, d->stride, d->pad, d->Cin, d->Cout);
    bool known = mn_same(F, MN_FIRST[MN_ALEXNET].F);
    for (const mn_filter& l : MN_ALEXNET_BODY) known = known || mn_same(F, l);
    if (!known || d->Hi + 2 * F.pad_h < F.KH || d->Wi + 2 * F.pad_w < F.KW) return EEGCLIP_EINVAL;
    mn_args a;
    int nj;
    a.W = mn_u16(d->W);
    a.bias = mn_u16(d->bias);
    a.out = mn_u16(d->out);
    if (mn_geometry(a, d->in, F, d->N, d->Hi, d->Wi, d->pad, d->out_pad, nj)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->bias)) & 7u) return EEGCLIP_EALIGN;
    return mn_launch(a, nj, d->dtype, stream);
}

extern "C" int eegclip_convbn16_in_width(int Wi) { return mn_in_width(MN_RESNET, Wi); }

extern "C" int eegclip_convbn16(const eegclip_convbn16_desc* d, void* stream) {
    if (!d || !d->in || !d->W || !d->scale || !d->shift || !d->out || d->N < 1 || d->Hi < 1 || d->Wi < 1 || d->out_pad < 0 || d->out_pad > 2 ||
        (d->relu != 0 && d->relu != 1) || !half_dtype_ok(d->dtype))
        return EEGCLIP_EINVAL;
    const mn_filter F = mn_square(d->KS, d->stride, d->pad, d->Cin, d->Cout);
    const bool stem = mn_same(F, MN_FIRST[MN_RESNET].F);
    const bool body = (d->KS == 1 || d->KS == 3) && (d->stride == 1 || d->stride == 2) && d->pad == d->KS / 2 && d->Cin >= 64 && d->Cin % 64 == 0 && d->Cout >= 64 &&
                      d->Cout % 64 == 0;
    if (!stem && !body) return EEGCLIP_EINVAL;
    mn_bn_args a;
    int nj;
    a.W = mn_u16(d->W);
    a.bias = nullptr;
    a.out = mn_u16(d->out);
    a.scale = static_cast<const float*>(d->scale);
    a.shift = static_cast<const float*>(d->shift);
    a.residual = mn_u16(d->residual);
    a.relu = d->relu;
    if (mn_geometry(a, d->in, F, d->N, d->Hi, d->Wi, d->pad, d->out_pad, nj)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->residual)) & 7u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->scale) | reinterpret_cast<uintptr_t>(d->shift)) & 3u) return EEGCLIP_EALIGN;
    return mn_launch(a, nj, d->dtype, stream);
}

extern "C" int eegclip_convbnact16_in_width(int Wi) { return mn_in_width(MN_EFFNET, Wi); }

extern "C" int eegclip_convbnact16(const eegclip_convbnact16_desc* d, void* stream) {
    if (!d || !d->in || !d->W || !d->scale || !d->shift || !d->out || d->N < 1 || d->Hi < 1 || d->Wi < 1 || d->out_pad < 0 || d->out_pad > 2 || d->in_pad < 0 ||
        d->in_pad > 2 || d->act < 0 || d->act > 2 || !half_dtype_ok(d->dtype))
        return EEGCLIP_EINVAL;
    const mn_filter F = mn_square(d->KS, d->stride, d->pad, d->Cin, d->Cout);
    const bool stem = mn_same(F, MN_FIRST[MN_EFFNET].F) && d->in_pad == 0;
    const bool point = d->KS == 1 && d->stride == 1 && d->pad == 0 && d->Cin >= 64 && d->Cin % 64 == 0 && d->Cout >= 64 && d->Cout % 64 == 0;
    if (!stem && !point) return EEGCLIP_EINVAL;
    mn_act_args a;
    int nj;
    a.W = mn_u16(d->W);
    a.bias = nullptr;
    a.out = mn_u16(d->out);
    a.scale = static_cast<const float*>(d->scale);
    a.shift = static_cast<const float*>(d->shift);
    a.residual = mn_u16(d->residual);
    a.act = d->act;
    // a 1 x 1 layer may read the interior of a frame with a border (the depthwise layer in front of it needed one)
    if (mn_geometry(a, d->in, F, d->N, d->Hi, d->Wi, d->pad + d->in_pad, d->out_pad, nj)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->residual)) & 7u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->scale) | reinterpret_cast<uintptr_t>(d->shift)) & 3u) return EEGCLIP_EALIGN;
    return mn_launch(a, nj, d->dtype, stream);
}

extern "C" int eegclip_maxpool16(const void* in, void* out, int N, int H, int W, int C, int in_pad, int out_pad, int dtype, void* stream) {
    if (!in || !out || N < 1 || H < 3 || W < 3 || C < 8 || C % 8 || in_pad < 0 || in_pad > 2 || out_pad < 0 || out_pad > 2 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    return mn_maxpool(in, out, N, H, W, C, C, in_pad, C, 0, out_pad, dtype, stream);
}

extern "C" int eegclip_maxpool16_pad(const void* in, void* out, int N, int H, int W, int C, int in_pad, int out_pad, int dtype, void* stream) {
    if (!in || !out || N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || in_pad < 0 || in_pad > 2 || out_pad < 0 || out_pad > 2 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) return EEGCLIP_EALIGN;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    MN_ELEMENTWISE(maxpool16_pad_kernel, dtype, (long long)N * Ho * Wo * (C / 8), stream, mn_u16(in), mn_u16(out), N, H, W, C, in_pad, out_pad, Ho, Wo);
    return (int)hipGetLastError();
}

extern "C" int eegclip_avgpool16(const void* in, float* out, int N, int H, int W, int C, int dtype, void* stream) {
    if (!in || !out || N < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL || C < 8 || C % 8 || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(in) & 15u) || (reinterpret_cast<uintptr_t>(out) & 3u)) return EEGCLIP_EALIGN;
    MN_ELEMENTWISE(avgpool16_kernel, dtype, (long long)N * (C / 8), stream, mn_u16(in), out, N, H * W, C);
    return (int)hipGetLastError();
}

extern "C" int eegclip_corr_distance(const float* a, const float* b, int N, int D, float* out, void* stream) {
    if (!a || !b || !out || N < 1 || D < 2) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 3u) return EEGCLIP_EALIGN;
    EEG_LAUNCH(corr_distance_kernel, dim3((unsigned)N), dim3(256), 4 * sizeof(float), stream, a, b, D, out);
    return (int)hipGetLastError();
}

extern "C" int eegclip_pack_nchw16(const void* x, void* frame, int N, int H, int W, int dtype, void* stream) {
    return mn_pack(MN_ALEXNET, x, frame, false, nullptr, nullptr, N, H, W, dtype, stream);
}

extern "C" int eegclip_pack_nchw16_stem(const void* x, void* frame, int N, int H, int W, int dtype, void* stream) {
    return mn_pack(MN_RESNET, x, frame, false, nullptr, nullptr, N, H, W, dtype, stream);
}

extern "C" int eegclip_pack_nchw16_pad1(const void* x, void* frame, int N, int H, int W, int dtype, void* stream) {
    return mn_pack(MN_EFFNET, x, frame, false, nullptr, nullptr, N, H, W, dtype, stream);
}

extern "C" int eegclip_pack_nchw16_affine(const void* x, void* frame, const float* a, const float* b, int N, int H, int W, int dtype, void* stream) {
    return mn_pack(MN_INCEPTION, x, frame, true, a, b, N, H, W, dtype, stream);
}

// ---- the Inception row (torchvision/models/inception.py): convolution + BatchNorm + ReLU into a channel slice of a concatenated frame
extern "C" int eegclip_convbncat16_in_width(int Wi) { return mn_in_width(MN_INCEPTION, Wi); }

extern "C" int eegclip_convbncat16(const eegclip_convbncat16_desc* d, void* stream) {
    if (!d || !d->in || !d->W || !d->scale || !d->shift || !d->out || d->N < 1 || d->Hi < 1 || d->Wi < 1 || d->out_pad < 0 || d->out_pad > 3 || d->in_pad < 0 ||
        d->in_pad > 3 || (d->relu != 0 && d->relu != 1) || !half_dtype_ok(d->dtype))
        return EEGCLIP_EINVAL;
    const int KH = d->KH, KW = d->KW, ph = d->pad_h, pw = d->pad_w;
    // the kernel shapes of the net: a square 3 x 3 unpadded (stride 1 or 2) or padded by 1, every other shape with its "same" padding on each axis, stride 1
    bool shape = false;
    if (KH == 3 && KW == 3) shape = (ph == 0 && pw == 0 && (d->stride == 1 || d->stride == 2)) || (ph == 1 && pw == 1 && d->stride == 1);
    else if ((KH == 1 && (KW == 1 || KW == 3 || KW == 7)) || (KW == 1 && (KH == 3 || KH == 7)) || (KH == 5 && KW == 5))
        shape = ph == KH / 2 && pw == KW / 2 && d->stride == 1;
    if (!shape || d->Cout < 8 || d->Cout % 8 || d->out_c0 < 0 || d->out_c0 % 8 || d->out_stride % 8 || (long long)d->out_c0 + d->Cout > d->out_stride)
        return EEGCLIP_EINVAL;
    if (d->Cin == 3 ? !(KH == 3 && d->stride == 2 && d->in_pad == 0 && d->Cout <= 64) : (d->Cin < 64 || d->Cin % 64 || d->in_pad < (ph > pw ? ph : pw)))
        return EEGCLIP_EINVAL;
    if (d->Hi + 2 * ph < KH || d->Wi + 2 * pw < KW) return EEGCLIP_EINVAL;
    mn_cat_args a;
    int nj;
    a.W = mn_u16(d->W);
    a.bias = nullptr;
    a.out = mn_u16(d->out);
    a.scale = static_cast<const float*>(d->scale);
    a.shift = static_cast<const float*>(d->shift);
    a.relu = d->relu; a.ostride = d->out_stride; a.oc0 = d->out_c0;
    // (Cout is the layer's own count: the epilogue stores the channel groups below it)
    if (mn_geometry(a, d->in, {KH, KW, d->stride, ph, pw, d->Cin, d->Cout}, d->N, d->Hi, d->Wi, d->in_pad, d->out_pad, nj)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
    if (reinterpret_cast<uintptr_t>(d->out) & 7u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->scale) | reinterpret_cast<uintptr_t>(d->shift)) & 3u) return EEGCLIP_EALIGN;
    return mn_launch(a, nj, d->dtype, stream);
}

extern "C" int eegclip_avgpool3x3_16(const void* in, void* out, int N, int H, int W, int C, int in_pad, int dtype, void* stream) {
    if (!in || !out || N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || in_pad < 1 || in_pad > 3 || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) return EEGCLIP_EALIGN;
    MN_ELEMENTWISE(avgpool3x3_16_kernel, dtype, (long long)N * H * W * (C / 8), stream, mn_u16(in), mn_u16(out), N, H, W, C, in_pad);
    return (int)hipGetLastError();
}

extern "C" int eegclip_maxpool16_cat(const void* in, void* out, int N, int H, int W, int C, int in_stride, int in_pad, int out_stride, int out_c0, int out_pad,
                                     int dtype, void* stream) {
    if (!in || !out || N < 1 || H < 3 || W < 3 || C < 8 || C % 8 || in_stride < C || in_stride % 8 || out_c0 < 0 || out_c0 % 8 || out_stride % 8 ||
        (long long)out_c0 + C > out_stride || in_pad < 0 || in_pad > 3 || out_pad < 0 || out_pad > 3 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    return mn_maxpool(in, out, N, H, W, C, in_stride, in_pad, out_stride, out_c0, out_pad, dtype, stream);
}
