// The SDXL VAE's arithmetic (low-level reconstruction path: Generation/custom_pipeline_low_level.py:8-31 `vae.encode` of the start image,
// Generation/custom_pipeline.py:421 `vae.decode` of the final latents; the module is diffusers' AutoencoderKL -- 3 x 3 convolutions, GroupNorm(32) + SiLU,
// nearest 2 x upsampling / stride-2 downsampling, one single-head self-attention in the middle) on 16-bit activations, fp32 accumulation.
//
// Layout: activations are PADDED NHWC -- [image][H + 2][W + 2][C], 16-bit, the one-pixel border is zero and never written -- so a 3 x 3 tap is a
// constant pixel offset with no boundary case, and a pixel's channels are one contiguous run: the k-slices of the implicit GEMM
//     out[p][co] = sum_{tap, ci} in[p + off(tap)][ci] W[co][tap][ci]          (M = pixels, N = Cout, K = 9 Cin)
// go global -> LDS by LDS-DMA exactly like the rows of a plain GEMM (csrc/gemm16.hip, whose tile loop this is: 128 pixels x 128 output channels per
// 256-thread workgroup, 64-k tiles, 4 stages with counted vmcnt, XOR-swizzled chunks, v_mfma_f32_32x32x16_{f16,bf16}); only the row ADDRESS differs -- it
// is recomputed per tap from the output pixel (stride 1 or 2; `up`: the source is the nearest-2x upsampled image, i.e. pixel >> 1 -- the Upsample2D +
// conv pair of the decoder never materialises the upsampled tensor).  Epilogue: + bias, + residual (a tensor shaped like the output).
// The few layers with 3 / 4 / 8 channels on one side (conv_in, conv_out, quant convs) run on a direct fp32-accumulate kernel, weights in LDS.
// GroupNorm: one statistics pass (fp32 sums about a pivot per thread, turned into fp64 partial sums per (image, group), atomics onto 64 addresses per image)
// and one apply pass (+ SiLU) that writes the next convolution's padded operand.
#include "half16.h"

#include <stdlib.h>

namespace eeg {

// LDS stages of the implicit-GEMM conv: 2 (64 KB: two workgroups per CU, the other's MFMAs cover this one's barrier and DMA waits) measured 19.9-20.0 ms per
// 1024 x 1024 decode against 20.8-20.9 with 3 or 4 stages (one workgroup per CU), three builds alternated on one box
#ifndef CV_NS_BUILD
#define CV_NS_BUILD 2
#endif
constexpr int CV_T = 128, CV_K = 64, CV_NS = CV_NS_BUILD;
constexpr int CV_ROWB = 2 * CV_K;
constexpr int CV_TILE_B = CV_T * CV_ROWB;
constexpr int CV_STAGE_B = 2 * CV_TILE_B;

struct cv_args {
    const unsigned short* in;          // padded NHWC input, pixel (0, 0) of the padded image 0
    const unsigned short* W;           // [Cout][KS * KS][Cin]
    unsigned short* out;               // output image 0, pixel (0, 0) of ITS (optionally padded) frame
    const unsigned short* bias;        // [Cout] or null
    const unsigned short* R;           // residual in the output's layout, or null
    int N, Ho, Wo;                     // images, output height / width
    int Hp, Wp, Cin;                   // input frame (padded) and channels
    int Hop, Wop, opad, Cout;          // output frame, its padding (0 or 1), channels
    int KS, stride, oy, ox, up;        // source pixel of output (y, x), tap (ky, kx): (y * stride + ky + oy, x * stride + kx + ox), or with `up`
                                       // (((y + ky - 1) >> 1) + 1, ((x + kx - 1) >> 1) + 1) in the padded input frame
    int M, tiles_n, ntiles, chunk;
    const unsigned short* cb;          // (N, Cout) per-image channel bias, or null (EXT forms only)
};

// EXT: the UNet's form (csrc/unet.hip's layers around it; diffusers 0.30.0 UNet2DConditionModel) -- Cout % 64 == 0 with the last 128-wide N tile masked (weight
// rows >= Cout are never read: those DMA lanes fetch row Cout - 1, whose columns nobody stores) and the per-image channel bias `cb` in the epilogue (ResnetBlock2D's
// time-embedding add, folded into conv1).  EXT = false is the VAE's form, unchanged.
// Four extra PRODUCER waves (round 6) issue every LDS-DMA instruction (and do the address arithmetic in front of it); the four MFMA waves only read
// fragments and feed the matrix pipe, and meet the producers at the one barrier per k-tile -- a wave that does both is in order and stalls in every DMA issue
// with its MFMAs unissued behind it (csrc/infonce_fused.hip, NPRD).
template <bool F16, bool EXT>
__global__ __launch_bounds__(512) void conv16_kernel(const cv_args a) {
    EEG_LDS_BASE(unsigned char, lds);
    const int logical = (int)(blockIdx.x & 7) * a.chunk + (int)(blockIdx.x >> 3);
    if (logical >= a.ntiles) return;
    const int m0 = (logical / a.tiles_n) * CV_T, n0 = (logical % a.tiles_n) * CV_T;
    const int t = threadIdx.x, lane = t & 63, wave_ = wave_uniform(t >> 6);
    const bool producer = wave_ >= 4;                         // (wave-uniform)
    const int wave = wave_ & 3;                               // index among the MFMA waves / among the DMA waves
    const int wm = wave >> 1, wn = wave & 1;
    const int r32 = lane & 31, h = lane >> 5;
    auto swz = [](int row) { return (row >> 1) & 7; };
    // DMA roles (csrc/gemm16.hip): DMA wave w deposits rows 32 w .. 32 w + 31 of both tiles, 8 rows (1 KB) per instruction
    const int drow = lane >> 3, dpos = lane & 7;
    int pn[4], py[4], px[4], acol[4], pbase[4];
    const unsigned short* wsrc[4];
    const int hw = a.Ho * a.Wo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 32 * wave + 8 * i + drow;
        const int col = 8 * (dpos ^ swz(row));
        const int m = m0 + row < a.M ? m0 + row : a.M - 1;          // rows beyond M: a clamped copy that nobody stores
        pn[i] = m / hw;
        const int rem = m - pn[i] * hw;
        py[i] = rem / a.Wo;
        px[i] = rem - py[i] * a.Wo;
        acol[i] = col;
        const int wrow = EXT && n0 + row >= a.Cout ? a.Cout - 1 : n0 + row;
        wsrc[i] = a.W + (long long)wrow * a.KS * a.KS * a.Cin + col;
        // pixel index of tap (0, 0) in the padded input frame (plain form) / of the frame row 0 of this image (`up`: the source row depends on the tap's parity)
        pbase[i] = a.up ? pn[i] * a.Hp : (pn[i] * a.Hp + py[i] * a.stride + a.oy) * a.Wp + px[i] * a.stride + a.ox;
    }
    const int cpt = a.Cin / CV_K;                             // k-tiles per tap
    // (tap, channel offset) of the NEXT k-tile to be issued, stepped once per tile: k-tile kt is tap kt / cpt, channels (kt % cpt) CV_K .. -- the first version
    // took those two integer divisions (and the tap's / KS) inside every one of the 8 DMA instructions of a tile: ~65 instructions of address arithmetic per
    // instruction, ~520 per k-tile against the 16 MFMAs they sit between (240 TFLOP/s for the decode); the weights' offset is simply kt CV_K
    int t_ky = 0, t_kx = 0, t_c0 = 0;
    auto advance = [&]() {
        t_c0 += CV_K;
        if (t_c0 == a.Cin) {
            t_c0 = 0;
            if (++t_kx == a.KS) { t_kx = 0; ++t_ky; }
        }
    };
    auto issue_one = [&](int kt, int dnum) {                  // DMA instruction `dnum` of k-tile kt == the tile (t_ky, t_kx, t_c0) describes
        const int o = dnum >> 2, i = dnum & 3;
        unsigned char* st = lds + (kt % CV_NS) * CV_STAGE_B + 32 * wave * CV_ROWB;
        if (o == 0) {
            int pix;
            if (a.up) {
                const int sy = ((py[i] + t_ky - 1) >> 1) + 1, sx = ((px[i] + t_kx - 1) >> 1) + 1;
                pix = (pbase[i] + sy) * a.Wp + sx;
            } else {
                pix = pbase[i] + t_ky * a.Wp + t_kx;
            }
            lds_dma16(st + 8 * i * CV_ROWB, a.in + (long long)pix * a.Cin + t_c0 + acol[i]);
        } else {
            lds_dma16(st + CV_TILE_B + 8 * i * CV_ROWB, wsrc[i] + (long long)kt * CV_K);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][i][e] = 0.f;
    int fom[4][2], fon[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rm = wm * 64 + 32 * i + r32, rn = wn * 64 + 32 * i + r32;
            fom[s][i] = rm * CV_ROWB + (((2 * s + h) ^ swz(rm)) & 7) * 16;
            fon[s][i] = CV_TILE_B + rn * CV_ROWB + (((2 * s + h) ^ swz(rn)) & 7) * 16;
        }
    const int ktiles = a.KS * a.KS * cpt;
    if (producer) {
#pragma unroll
        for (int p = 0; p < CV_NS - 1; ++p)
            if (p < ktiles) {
#pragma unroll
                for (int dnum = 0; dnum < 8; ++dnum) issue_one(p, dnum);
                advance();
            }
        for (int kt = 0; kt < ktiles; ++kt) {
            const int newer = ktiles - 1 - kt < CV_NS - 2 ? ktiles - 1 - kt : CV_NS - 2;
            if (newer >= 2) wait_vmcnt<16>();
            else if (newer == 1) wait_vmcnt<8>();
            else wait_vmcnt<0>();
            raw_barrier();                                    // the one meeting point of the two kinds of waves per k-tile
            if (kt + CV_NS - 1 < ktiles) {
#pragma unroll
                for (int dnum = 0; dnum < 8; ++dnum) issue_one(kt + CV_NS - 1, dnum);
                advance();
            }
        }
        return;                                               // (the epilogue has no barrier)
    }
    for (int kt = 0; kt < ktiles; ++kt) {
        raw_barrier();
        const unsigned char* st = lds + (kt % CV_NS) * CV_STAGE_B;
        bf16x8 am[2][2], wf[2][2];
        // (what a step's first MFMA takes is read last and the next step's reads go out behind that MFMA: csrc/infonce_fused.hip, round 6)
        auto read_step = [&](int s, int set) {
#pragma unroll
            for (int i = 1; i >= 0; --i) {
                am[set][i] = *reinterpret_cast<const bf16x8*>(st + fom[s][i]);
                wf[set][i] = *reinterpret_cast<const bf16x8*>(st + fon[s][i]);
            }
        };
        read_step(0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sched_fence();
            const int set = s & 1;
#pragma unroll
            for (int j = 0; j < 2; ++j)
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
    // ---- epilogue: lane (r32, h) owns pixel m = m0 + 64 wm + 32 i + r32; registers 4 eq .. 4 eq + 3 of n tile j are channels n0 + 64 wn + 32 j + 8 eq + 4 h ..
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + 32 * i + r32;
        if (m >= a.M) continue;
        const int n_ = m / hw, rem = m - n_ * hw, y = rem / a.Wo, x = rem - y * a.Wo;
        const long long opix = (((long long)n_ * a.Hop + y + a.opad) * a.Wop + x + a.opad) * a.Cout;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int eq = 0; eq < 4; ++eq) {
                const int n = n0 + wn * 64 + 32 * j + 8 * eq + 4 * h;
                if (EXT && n >= a.Cout) continue;
                u16x4 bv = u16x4{0, 0, 0, 0}, rv = u16x4{0, 0, 0, 0}, cbv = u16x4{0, 0, 0, 0};
                if (a.bias) bv = *reinterpret_cast<const u16x4*>(a.bias + n);
                if (a.R) rv = *reinterpret_cast<const u16x4*>(a.R + opix + n);
                if (EXT && a.cb) cbv = *reinterpret_cast<const u16x4*>(a.cb + (long long)n_ * a.Cout + n);
                u16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = acc[j][i][4 * eq + e];
                    if (a.bias) v += to_f32<F16>(bv[e]);
                    if (EXT && a.cb) v += to_f32<F16>(cbv[e]);
                    if (a.R) v += to_f32<F16>(rv[e]);
                    o[e] = to_h<F16>(v);
                }
                *reinterpret_cast<u16x4*>(a.out + opix + n) = o;
            }
    }
}

// ---- direct convolution for the layers with 3 / 4 / 8 channels on one side: thread = (pixel, output channel), weights (16-bit) in LDS, fp32 accumulate
template <bool F16>
__global__ __launch_bounds__(256) void conv_small16_kernel(const cv_args a) {
    EEG_LDS_BASE(unsigned short, wl);                        // [Cout][KS*KS][Cin]
    const int kk = a.KS * a.KS, wn = a.Cout * kk * a.Cin;
    for (int i = threadIdx.x; i < wn; i += 256) wl[i] = a.W[i];
    __syncthreads();
    const long long total = (long long)a.M * a.Cout;
    const int hw = a.Ho * a.Wo;
    const bool vec8 = (a.Cin & 7) == 0 && (reinterpret_cast<uintptr_t>(a.in) & 15u) == 0;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int m = (int)(q / a.Cout), co = (int)(q - (long long)m * a.Cout);
        const int n_ = m / hw, rem = m - n_ * hw, y = rem / a.Wo, x = rem - y * a.Wo;
        float acc = a.bias ? to_f32<F16>(a.bias[co]) : 0.f;
        for (int ky = 0; ky < a.KS; ++ky)
            for (int kx = 0; kx < a.KS; ++kx) {
                const int sy = a.up ? (((y + ky - 1) >> 1) + 1) : y * a.stride + ky + a.oy;
                const int sx = a.up ? (((x + kx - 1) >> 1) + 1) : x * a.stride + kx + a.ox;
                const unsigned short* p = a.in + (((long long)n_ * a.Hp + sy) * a.Wp + sx) * a.Cin;
                const unsigned short* w = wl + (co * kk + ky * a.KS + kx) * a.Cin;
                if (vec8) {                                  // 16-byte reads of both operands (conv_out, 128 -> 3 at 1024 x 1024: 6.1 -> ms with 2-byte reads); same summation order
                    for (int ci = 0; ci < a.Cin; ci += 8) {
                        const u16x8 pv = *reinterpret_cast<const u16x8*>(p + ci), wv = *reinterpret_cast<const u16x8*>(w + ci);
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc += to_f32<F16>(pv[e]) * to_f32<F16>(wv[e]);
                    }
                } else {
                    for (int ci = 0; ci < a.Cin; ++ci) acc += to_f32<F16>(p[ci]) * to_f32<F16>(w[ci]);
                }
            }
        const long long opix = (((long long)n_ * a.Hop + y + a.opad) * a.Wop + x + a.opad) * a.Cout;
        if (a.R) acc += to_f32<F16>(a.R[opix + co]);
        a.out[opix + co] = to_h<F16>(acc);
    }
}

// ---- GroupNorm over a padded NHWC tensor (interior pixels only).  Statistics: workgroup = (image, block of GN_PB pixels); thread = (8 consecutive channels, pixel lane):
// 16-byte reads, the pixels of a lane independent of one another (loads in flight), the two 4-channel halves summed apart (a group has >= 4 channels); the sums meet
// per group in LDS, one fp64 atomic pair per (workgroup, group).  (The first version gave a thread one CHANNEL and walked its 64 pixels one 2-byte read after the
// other, an integer division each: 7.5 ms of a 35 ms decode for ~3 GB of reads.)  Channel counts the vector form does not take (C % 8, 256 % (C / 8)) walk as before.
constexpr int GN_PB = 256;
template <bool F16>
__global__ __launch_bounds__(256) void gn_stats16_kernel(const unsigned short* __restrict__ x, int H, int W, int C, int pad, int groups, double* __restrict__ sums) {
    EEG_LDS_BASE(double, part);                              // [256][2 halves](sum x, sum x^2)
    const int n_ = blockIdx.y, t = threadIdx.x, hw = H * W, Wp = W + 2 * pad, Hp = H + 2 * pad;
    const int p0 = blockIdx.x * GN_PB, p1 = p0 + GN_PB < hw ? p0 + GN_PB : hw;
    const int cpg = C / groups, c8n = C / 8;
    if ((C & 7) == 0 && c8n <= 256 && 256 % c8n == 0 && (groups & 1) == 0 && groups <= 256 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0) {
        const int cc = t % c8n, pl = t / c8n, ppi = 256 / c8n;
        // sums of (x - k) and (x - k)^2 about a pivot k per half-chunk, the first value read: fp32 sums of x and x^2 lose the variance of a group whose
        // |mean| is large against its deviation (sum x^2 / n - mean^2 cancels (mean / sd)^2 of their 2^24: an fp16 decode's rstd off by 1 % at mean / sd 160)
        // (the pivots' read is the loop's own first read, not one more round trip in front of it; a lane without a pixel has k = 0 and counts n = 0)
        // The even and the odd channels of a half are summed apart, two floats per instruction (v_pk_add_f32 / v_pk_mul_f32): at 512 channels, 128 x 128, one
        // wave per SIMD, the loop's VALU instructions are the kernel's time
        f32x2_t s0 = {0.f, 0.f}, q0 = {0.f, 0.f}, s1 = {0.f, 0.f}, q1 = {0.f, 0.f};
        int cnt = 0;
        auto load = [&](int p) {
            const int y = p / W, xx = p - y * W;
            return *reinterpret_cast<const u16x8*>(x + (((long long)n_ * Hp + y + pad) * Wp + xx + pad) * C + 8 * cc);
        };
        u16x8 vk = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (p0 + pl < p1) vk = load(p0 + pl);
        const float k0 = to_f32<F16>(vk[0]), k1 = to_f32<F16>(vk[4]);
        const f32x2_t k0v = {k0, k0}, k1v = {k1, k1};
#pragma unroll 4
        for (int p = p0 + pl; p < p1; p += ppi) {
            const u16x8 v = load(p);
            ++cnt;
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                const f32x2_t a = f32x2_t{to_f32<F16>(v[e]), to_f32<F16>(v[e + 1])} - k0v, b = f32x2_t{to_f32<F16>(v[4 + e]), to_f32<F16>(v[5 + e])} - k1v;
                s0 += a; q0 += a * a;
                s1 += b; q1 += b * b;
            }
        }
        // every thread turns its two half-chunks into (sum x, sum x^2) over their n = 4 cnt values in fp64 -- sum x = s + n k, sum x^2 = q + 2 k s + n k^2 -- and
        // leaves them in LDS; fixed-order combine (two decodes of one latent are bit-identical: tests/test_vae_gpu.py): thread g adds group g's entries --
        // half-chunks g cpg / 4 .. of every pixel lane -- in index order
        const double n = 4.0 * cnt, d0 = k0, d1 = k1;
        const double ds0 = (double)s0[0] + (double)s0[1], ds1 = (double)s1[0] + (double)s1[1];
        part[4 * t] = ds0 + n * d0;
        part[4 * t + 1] = (double)q0[0] + (double)q0[1] + 2.0 * d0 * ds0 + n * d0 * d0;
        part[4 * t + 2] = ds1 + n * d1;
        part[4 * t + 3] = (double)q1[0] + (double)q1[1] + 2.0 * d1 * ds1 + n * d1 * d1;
        __syncthreads();
        if (t < groups) {
            const int hpg = cpg / 4;                         // 4-channel half-chunks per group
            double S = 0.0, Q = 0.0;
            for (int l = 0; l < ppi; ++l)
                for (int k = 0; k < hpg; ++k) {
                    const int hc = t * hpg + k;              // half-chunk index along the channels: thread (l, hc >> 1), half hc & 1
                    const double* e = part + 4 * (l * c8n + (hc >> 1)) + 2 * (hc & 1);
                    S += e[0];
                    Q += e[1];
                }
            atomicAdd(sums + ((long long)n_ * groups + t) * 2, S);
            atomicAdd(sums + ((long long)n_ * groups + t) * 2 + 1, Q);
        }
    } else {
        // the same pivot form per channel; the channels of a group meet in LDS as doubles ([2][groups], atomics: no fixed order here), then one fp64 atomic pair
        // per (workgroup, group) as in the vector form
        for (int i = t; i < 2 * groups; i += 256) part[i] = 0.0;
        __syncthreads();
        for (int c = t; c < C; c += 256) {
            const unsigned short* xc = x + c;
            auto at = [&](int p) {
                const int y = p / W, xx = p - y * W;
                return to_f32<F16>(xc[(((long long)n_ * Hp + y + pad) * Wp + xx + pad) * C]);
            };
            const float k = at(p0);
            float s_ = 0.f, q = 0.f;
            for (int p = p0; p < p1; ++p) {
                const float v = at(p) - k;
                s_ += v;
                q += v * v;
            }
            const double n = p1 - p0, kk = k;
            atomicAdd(part + c / cpg, (double)s_ + n * kk);
            atomicAdd(part + groups + c / cpg, (double)q + 2.0 * kk * s_ + n * kk * kk);
        }
        __syncthreads();
        for (int g = t; g < groups; g += 256) {
            atomicAdd(sums + ((long long)n_ * groups + g) * 2, part[g]);
            atomicAdd(sums + ((long long)n_ * groups + g) * 2 + 1, part[groups + g]);
        }
    }
}
// Statistics for the channel counts the vector form above does not take (the UNet's 320 / 640 / 960 / 1280 / 1920 / 2560 channels in 32 groups: 256 % (C / 8)
// != 0, or 2 mod 4 channels per group), in a FIXED order so that two passes over one tensor give bit-identical sums: item (pixel lane pl, 8-channel chunk cc),
// item i = pl * c8n + cc, belongs to thread i % 256 (a thread may own two); the item walks pixels p0 + pl, p0 + pl + ppi, .. and keeps (sum, sum of squares)
// per channel PAIR (a group has an even channel count: both channels of a pair share it).  The pairs meet per group in LDS in index order; one fp64 atomic
// pair per (workgroup, group), as in the vector form.  (The per-channel walk it replaces for these counts added float partials into LDS with atomics: no
// fixed order.)
template <bool F16>
__global__ __launch_bounds__(256) void gn_stats16_pairs_kernel(const unsigned short* __restrict__ x, int H, int W, int C, int pad, int groups,
                                                               double* __restrict__ sums) {
    EEG_LDS_BASE(double, part);                              // [ppi * c8n][4 pairs](sum x, sum x^2)
    const int n_ = blockIdx.y, t = threadIdx.x, hw = H * W, Wp = W + 2 * pad, Hp = H + 2 * pad;
    const int p0 = blockIdx.x * GN_PB, p1 = p0 + GN_PB < hw ? p0 + GN_PB : hw;
    const int c8n = C / 8, ppi = c8n < 256 ? 256 / c8n : 1, items = ppi * c8n, ppg = C / groups / 2;
    for (int i = t; i < items; i += 256) {
        const int pl = i / c8n, cc = i - pl * c8n;
        // (sums about a pivot per pair, the first value the item reads, as in gn_stats16_kernel)
        f32x2_t s[4], q[4], k[4];                            // (the two channels of a pair side by side: two floats per instruction)
        int cnt = 0;
        auto load = [&](int p) {
            const int y = p / W, xx = p - y * W;
            return *reinterpret_cast<const u16x8*>(x + (((long long)n_ * Hp + y + pad) * Wp + xx + pad) * C + 8 * cc);
        };
        u16x8 vk = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (p0 + pl < p1) vk = load(p0 + pl);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = q[j] = f32x2_t{0.f, 0.f};
            k[j] = f32x2_t{to_f32<F16>(vk[2 * j]), to_f32<F16>(vk[2 * j])};
        }
        for (int p = p0 + pl; p < p1; p += ppi) {
            const u16x8 v = load(p);
            ++cnt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2_t a = f32x2_t{to_f32<F16>(v[2 * j]), to_f32<F16>(v[2 * j + 1])} - k[j];
                s[j] += a;
                q[j] += a * a;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {                         // (sum x, sum x^2) = (s + n k, q + 2 k s + n k^2) over the pair's n = 2 cnt values, in fp64
            const double n = 2.0 * cnt, d = k[j][0], ds = (double)s[j][0] + (double)s[j][1];
            part[8 * i + 2 * j] = ds + n * d;
            part[8 * i + 2 * j + 1] = (double)q[j][0] + (double)q[j][1] + 2.0 * d * ds + n * d * d;
        }
    }
    __syncthreads();
    for (int g = t; g < groups; g += 256) {
        double S = 0.0, Q = 0.0;
        for (int l = 0; l < ppi; ++l)
            for (int k = 0; k < ppg; ++k) {
                const int pr = g * ppg + k;                  // channel pair index: chunk pr / 4, pair pr % 4 of it
                const double* e = part + 8 * (l * c8n + (pr >> 2)) + 2 * (pr & 3);
                S += e[0];
                Q += e[1];
            }
        atomicAdd(sums + ((long long)n_ * groups + g) * 2, S);
        atomicAdd(sums + ((long long)n_ * groups + g) * 2 + 1, Q);
    }
}

// apply: y = (x - mean) * rstd * gamma + beta (then SiLU if `silu`), written into another frame (its own padding); 4 consecutive channels per thread.  Every workgroup
// first turns the (image, group) sums into a (mean, 1 / sqrt(var + eps)) table in LDS (the first version redid the fp64 division and square root per 4 channels)
template <bool F16>
__global__ __launch_bounds__(256) void gn_apply16_kernel(const unsigned short* __restrict__ x, int N, int H, int W, int C, int pad, int groups,
                                                          const double* __restrict__ sums, const unsigned short* __restrict__ gamma,
                                                          const unsigned short* __restrict__ beta, float eps, int silu_on, unsigned short* __restrict__ y, int opad) {
    EEG_LDS_BASE(float, tab);                                // [N * groups][2]
    const int c4n = C / 4, hw = H * W, Wp = W + 2 * pad, Hp = H + 2 * pad, Wop = W + 2 * opad, Hop = H + 2 * opad, cpg = C / groups;
    const long long total = (long long)N * hw * c4n;
    const double cnt = (double)hw * cpg;
    for (int i = threadIdx.x; i < N * groups; i += 256) {
        const double mu = sums[2 * (long long)i] / cnt;
        double var = sums[2 * (long long)i + 1] / cnt - mu * mu;
        if (var < 0.0) var = 0.0;
        tab[2 * i] = (float)mu;
        tab[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 4 * (int)(q % c4n);
        const long long pq = q / c4n;
        const int n_ = (int)(pq / hw), p = (int)(pq - (long long)n_ * hw), yy = p / W, xx = p - yy * W;
        const int g = c / cpg;                               // (cpg % 4 == 0: the 4 channels share a group)
        const float mean = tab[2 * (n_ * groups + g)], rstd = tab[2 * (n_ * groups + g) + 1];
        const u16x4 xv = *reinterpret_cast<const u16x4*>(x + (((long long)n_ * Hp + yy + pad) * Wp + xx + pad) * C + c);
        const u16x4 gv = *reinterpret_cast<const u16x4*>(gamma + c), bv = *reinterpret_cast<const u16x4*>(beta + c);
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = (to_f32<F16>(xv[e]) - mean) * rstd * to_f32<F16>(gv[e]) + to_f32<F16>(bv[e]);
            if (silu_on) v = silu(v);
            o[e] = to_h<F16>(v);
        }
        *reinterpret_cast<u16x4*>(y + (((long long)n_ * Hop + yy + opad) * Wop + xx + opad) * C + c) = o;
    }
}

// apply with 2 consecutive channels per thread (C / groups even but not a multiple of 4: both channels of a pair share a group)
template <bool F16>
__global__ __launch_bounds__(256) void gn_apply16_c2_kernel(const unsigned short* __restrict__ x, int N, int H, int W, int C, int pad, int groups,
                                                             const double* __restrict__ sums, const unsigned short* __restrict__ gamma,
                                                             const unsigned short* __restrict__ beta, float eps, int silu_on, unsigned short* __restrict__ y, int opad) {
    EEG_LDS_BASE(float, tab);                                // [N * groups][2]
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const int c2n = C / 2, hw = H * W, Wp = W + 2 * pad, Hp = H + 2 * pad, Wop = W + 2 * opad, Hop = H + 2 * opad, cpg = C / groups;
    const long long total = (long long)N * hw * c2n;
    const double cnt = (double)hw * cpg;
    for (int i = threadIdx.x; i < N * groups; i += 256) {
        const double mu = sums[2 * (long long)i] / cnt;
        double var = sums[2 * (long long)i + 1] / cnt - mu * mu;
        if (var < 0.0) var = 0.0;
        tab[2 * i] = (float)mu;
        tab[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int c = 2 * (int)(q % c2n);
        const long long pq = q / c2n;
        const int n_ = (int)(pq / hw), p = (int)(pq - (long long)n_ * hw), yy = p / W, xx = p - yy * W;
        const int g = c / cpg;
        const float mean = tab[2 * (n_ * groups + g)], rstd = tab[2 * (n_ * groups + g) + 1];
        const u16x2 xv = *reinterpret_cast<const u16x2*>(x + (((long long)n_ * Hp + yy + pad) * Wp + xx + pad) * C + c);
        const u16x2 gv = *reinterpret_cast<const u16x2*>(gamma + c), bv = *reinterpret_cast<const u16x2*>(beta + c);
        u16x2 o;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float v = (to_f32<F16>(xv[e]) - mean) * rstd * to_f32<F16>(gv[e]) + to_f32<F16>(bv[e]);
            if (silu_on) v = silu(v);
            o[e] = to_h<F16>(v);
        }
        *reinterpret_cast<u16x2*>(y + (((long long)n_ * Hop + yy + opad) * Wop + xx + opad) * C + c) = o;
    }
}

// ---- softmax over the rows of a 16-bit matrix, in place, logits scaled by `scale` first (the mid-block attention's (HW, HW) score matrix): one workgroup
// per row, fp32 arithmetic
template <bool F16>
__global__ __launch_bounds__(256) void softmax_rows16_kernel(unsigned short* __restrict__ s, int cols, long long ld, float scale) {
    EEG_LDS_BASE(float, red);                                // [8]
    unsigned short* row = s + (long long)blockIdx.x * ld;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    float mx = -3.0e38f;
    for (int c = t; c < cols; c += 256) mx = fmaxf(mx, scale * to_f32<F16>(row[c]));
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int c = t; c < cols; c += 256) sum += expf(scale * to_f32<F16>(row[c]) - mx);
    sum = wave_sum(sum);
    if (lane == 0) red[4 + w] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[4] + red[5]) + (red[6] + red[7]));
    for (int c = t; c < cols; c += 256) row[c] = to_h<F16>(expf(scale * to_f32<F16>(row[c]) - mx) * inv);
}

// ---- DiagonalGaussianDistribution.sample of the encoder's moments (padded-free NHWC (N, H, W, 2 L): mean | logvar): z = mean + exp(0.5 clamp(logvar)) noise
template <bool F16>
__global__ __launch_bounds__(256) void vae_sample16_kernel(const unsigned short* __restrict__ mom, const unsigned short* __restrict__ noise,
                                                            unsigned short* __restrict__ z, long long pixels, int L) {
    const long long total = pixels * L;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const long long p = q / L;
        const int c = (int)(q - p * L);
        const float mean = to_f32<F16>(mom[p * 2 * L + c]);
        float lv = to_f32<F16>(mom[p * 2 * L + L + c]);
        lv = fminf(fmaxf(lv, -30.f), 20.f);
        const float nz = noise ? to_f32<F16>(noise[q]) : 0.f;
        z[q] = to_h<F16>(mean + expf(0.5f * lv) * nz);
    }
}

}  // namespace eeg

using namespace eeg;

static int cv_check(const eegclip_conv16_desc* d) {
    if (!d || !d->in || !d->W || !d->out || d->N < 1 || d->Ho < 1 || d->Wo < 1 || d->Cin < 1 || d->Cout < 1 || (d->KS != 1 && d->KS != 3) ||
        (d->stride != 1 && d->stride != 2) || d->in_pad < 0 || d->in_pad > 1 || d->out_pad < 0 || d->out_pad > 1 || d->Hi < 1 || d->Wi < 1 || !half_dtype_ok(d->dtype))
        return EEGCLIP_EINVAL;
    if (d->upsample && (d->KS != 3 || d->stride != 1 || d->in_pad != 1 || d->Ho != 2 * d->Hi || d->Wo != 2 * d->Wi)) return EEGCLIP_EINVAL;
    // every tap of every output pixel must land inside the padded input frame
    const int pt = d->pad_top, pl = d->pad_left;
    if (pt < 0 || pl < 0 || pt > d->in_pad || pl > d->in_pad) return EEGCLIP_EINVAL;
    if (!d->upsample) {
        const int ymax = (d->Ho - 1) * d->stride + d->KS - 1 - pt, xmax = (d->Wo - 1) * d->stride + d->KS - 1 - pl;
        if (ymax > d->Hi - 1 + d->in_pad || xmax > d->Wi - 1 + d->in_pad) return EEGCLIP_EINVAL;
    }
    return 0;
}

extern "C" int eegclip_conv16(const eegclip_conv16_desc* d, void* stream) {
    if (const int rc = cv_check(d)) return rc;
    cv_args a;
    a.in = static_cast<const unsigned short*>(d->in);
    a.W = static_cast<const unsigned short*>(d->W);
    a.out = static_cast<unsigned short*>(d->out);
    a.bias = static_cast<const unsigned short*>(d->bias);
    a.R = static_cast<const unsigned short*>(d->residual);
    a.N = d->N; a.Ho = d->Ho; a.Wo = d->Wo;
    a.Hp = d->Hi + 2 * d->in_pad; a.Wp = d->Wi + 2 * d->in_pad; a.Cin = d->Cin;
    a.Hop = d->Ho + 2 * d->out_pad; a.Wop = d->Wo + 2 * d->out_pad; a.opad = d->out_pad; a.Cout = d->Cout;
    a.KS = d->KS; a.stride = d->stride; a.oy = d->in_pad - d->pad_top; a.ox = d->in_pad - d->pad_left; a.up = d->upsample ? 1 : 0;
    const long long M = (long long)d->N * d->Ho * d->Wo;
    if (M > 0x7fffffffLL) return EEGCLIP_EINVAL;
    a.M = (int)M;
    a.cb = static_cast<const unsigned short*>(d->chan_bias);
    const bool f16 = d->dtype == EEGCLIP_DT_F16;
    const bool mfma = d->Cin % CV_K == 0 && d->Cout % CV_T == 0 && !d->chan_bias;
    const size_t wbytes = (size_t)d->Cout * d->KS * d->KS * d->Cin * 2;
    // the UNet's form: Cout % 64 with a channel bias, or with weights beyond what the direct kernel takes (shapes it took before keep it)
    const bool ext = d->Cin % CV_K == 0 && d->Cout % 64 == 0 && !mfma && (d->chan_bias || wbytes > 150 * 1024);
    if (mfma || ext) {
        if ((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
        if ((reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->bias) | reinterpret_cast<uintptr_t>(d->residual) |
             reinterpret_cast<uintptr_t>(d->chan_bias)) & 7u) return EEGCLIP_EALIGN;
        a.tiles_n = (d->Cout + CV_T - 1) / CV_T;
        a.ntiles = a.tiles_n * ((a.M + CV_T - 1) / CV_T);
        a.chunk = (a.ntiles + 7) / 8;
        const size_t lds = (size_t)CV_NS * CV_STAGE_B;
        const dim3 grid((unsigned)(8 * a.chunk)), block(512);       // 4 MFMA + 4 producer (DMA) waves
#define EEG_CV(F, X) EEG_LAUNCH((conv16_kernel<F, X>), grid, block, lds, stream, a)
        if (ext) { if (f16) EEG_CV(true, true); else EEG_CV(false, true); }
        else     { if (f16) EEG_CV(true, false); else EEG_CV(false, false); }
#undef EEG_CV
        return (int)hipGetLastError();
    }
    if (d->chan_bias) return EEGCLIP_EINVAL;                 // (the channel bias is an epilogue of the matrix-core forms only)
    if (wbytes > 150 * 1024) return EEGCLIP_EINVAL;           // (the small-channel layers of the VAE: at most 512 -> 8, 72 KB)
    a.tiles_n = a.ntiles = a.chunk = 0;
    long long g = (M * d->Cout + 255) / 256;
    if (g > 16384) g = 16384;
    if (f16) EEG_LAUNCH((conv_small16_kernel<true>), dim3((unsigned)g), dim3(256), wbytes, stream, a);
    else     EEG_LAUNCH((conv_small16_kernel<false>), dim3((unsigned)g), dim3(256), wbytes, stream, a);
    return (int)hipGetLastError();
}

extern "C" int eegclip_groupnorm16(const void* x, int N, int H, int W, int C, int pad, int groups, const void* gamma, const void* beta, float eps, int silu_on,
                                   void* y, int out_pad, double* sums, int dtype, void* stream) {
    if (!x || !gamma || !beta || !y || !sums || N < 1 || H < 1 || W < 1 || C < 4 || groups < 1 || C % groups || (C / groups) % 2 || pad < 0 || pad > 1 ||
        out_pad < 0 || out_pad > 1 || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) | reinterpret_cast<uintptr_t>(y) |
         reinterpret_cast<uintptr_t>(sums)) & 7u)
        return EEGCLIP_EALIGN;
    const bool f16 = dtype == EEGCLIP_DT_F16;
    const int cpg = C / groups, c8n = C / 8;
    const bool a16 = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
    // statistics: the vector form (the VAE's channel counts; the condition gn_stats16_kernel takes it under) keeps its kernel; other counts with C % 8 == 0
    // and a 16-byte aligned x take the fixed-order pair form; the per-channel walk stays for the rest (4 k channels per group only)
    const bool vec = cpg % 4 == 0 && (C & 7) == 0 && c8n <= 256 && 256 % c8n == 0 && (groups & 1) == 0 && groups <= 256 && a16;
    const bool pairs = !vec && (C & 7) == 0 && a16 && c8n <= 2048;
    if (!vec && !pairs && cpg % 4) return EEGCLIP_EINVAL;
    if ((long long)N * groups > 4096) return EEGCLIP_EINVAL;     // (the apply kernel keeps the (mean, rstd) table of every (image, group) in LDS)
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)N * groups * 2 * sizeof(double), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const dim3 gs((unsigned)((H * W + GN_PB - 1) / GN_PB), (unsigned)N);
    if (pairs) {
        const size_t lds_p = (size_t)(c8n < 256 ? 256 / c8n : 1) * c8n * 8 * sizeof(double);         // (at most 128 KB)
#if !defined(EEG_EMU)
        if (lds_p > 64 * 1024) {                             // C > 8192: more dynamic LDS than the default limit of a launch (csrc/vae_attn.hip)
            e = f16 ? hipFuncSetAttribute((const void*)gn_stats16_pairs_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_p)
                    : hipFuncSetAttribute((const void*)gn_stats16_pairs_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_p);
            if (e != hipSuccess) return (int)e;
        }
#endif
        if (f16) EEG_LAUNCH((gn_stats16_pairs_kernel<true>), gs, dim3(256), lds_p, stream, static_cast<const unsigned short*>(x), H, W, C, pad, groups, sums);
        else     EEG_LAUNCH((gn_stats16_pairs_kernel<false>), gs, dim3(256), lds_p, stream, static_cast<const unsigned short*>(x), H, W, C, pad, groups, sums);
    } else {
        // (vector form: [256][4]; walk: [2][groups], N groups <= 4096: at most 64 KB)
        const size_t lds = (groups <= 512 ? 256 * 4 : 2 * (size_t)groups) * sizeof(double);
        if (f16) EEG_LAUNCH((gn_stats16_kernel<true>), gs, dim3(256), lds, stream, static_cast<const unsigned short*>(x), H, W, C, pad, groups, sums);
        else     EEG_LAUNCH((gn_stats16_kernel<false>), gs, dim3(256), lds, stream, static_cast<const unsigned short*>(x), H, W, C, pad, groups, sums);
    }
    if (cpg % 4) {                                           // (2 mod 4 channels per group: the UNet's 320 / 960 channels)
        long long g2 = ((long long)N * H * W * (C / 2) + 255) / 256;
        if (g2 > 16384) g2 = 16384;
#define EEG_GNA2(F)                                                                                                                                       \
    EEG_LAUNCH((gn_apply16_c2_kernel<F>), dim3((unsigned)g2), dim3(256), (size_t)N * groups * 2 * sizeof(float), stream, static_cast<const unsigned short*>(x), N, H, W, C, pad, \
               groups, sums, static_cast<const unsigned short*>(gamma), static_cast<const unsigned short*>(beta), eps, silu_on, static_cast<unsigned short*>(y), out_pad)
        if (f16) EEG_GNA2(true);
        else     EEG_GNA2(false);
#undef EEG_GNA2
        return (int)hipGetLastError();
    }
    long long g = ((long long)N * H * W * (C / 4) + 255) / 256;
    if (g > 16384) g = 16384;
#define EEG_GNA(F)                                                                                                                                        \
    EEG_LAUNCH((gn_apply16_kernel<F>), dim3((unsigned)g), dim3(256), (size_t)N * groups * 2 * sizeof(float), stream, static_cast<const unsigned short*>(x), N, H, W, C, pad, groups, sums,      \
               static_cast<const unsigned short*>(gamma), static_cast<const unsigned short*>(beta), eps, silu_on, static_cast<unsigned short*>(y), out_pad)
    if (f16) EEG_GNA(true);
    else     EEG_GNA(false);
#undef EEG_GNA
    return (int)hipGetLastError();
}

extern "C" int eegclip_softmax_rows16(void* s, int rows, int cols, long long ld, float scale, int dtype, void* stream) {
    if (!s || rows < 1 || cols < 1 || ld < cols || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((softmax_rows16_kernel<true>), dim3((unsigned)rows), dim3(256), 8 * sizeof(float), stream, static_cast<unsigned short*>(s), cols, ld, scale);
    else                         EEG_LAUNCH((softmax_rows16_kernel<false>), dim3((unsigned)rows), dim3(256), 8 * sizeof(float), stream, static_cast<unsigned short*>(s), cols, ld, scale);
    return (int)hipGetLastError();
}

extern "C" int eegclip_vae_sample16(const void* moments, const void* noise, void* z, long long pixels, int latent_channels, int dtype, void* stream) {
    if (!moments || !z || pixels < 1 || latent_channels < 1 || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    long long g = (pixels * latent_channels + 255) / 256;
    if (g > 4096) g = 4096;
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((vae_sample16_kernel<true>), dim3((unsigned)g), dim3(256), 0, stream, static_cast<const unsigned short*>(moments), static_cast<const unsigned short*>(noise), static_cast<unsigned short*>(z), pixels, latent_channels);
    else                         EEG_LAUNCH((vae_sample16_kernel<false>), dim3((unsigned)g), dim3(256), 0, stream, static_cast<const unsigned short*>(moments), static_cast<const unsigned short*>(noise), static_cast<unsigned short*>(z), pixels, latent_channels);
    return (int)hipGetLastError();
}
