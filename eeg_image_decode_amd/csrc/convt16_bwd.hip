// Backward of ConvTranspose2d(kernel 4, stride 2, padding 1) on the padded 16-bit NHWC frames of csrc/convt16.hip: what training the reference's low-level
// EEG -> VAE-latent encoder needs (Generation/train_vae_latent_512_low_level_no_average.py:219-260 differentiated).  z = the raw convolution output frame
// (N, 2 Hi + 2, 2 Wi + 2, Cout), x = the input frame (N, Hi + 2, Wi + 2, Cin), both with zero borders; fp16 / bf16 operands, fp32 accumulation, no atomics, no
// memset, fixed summation orders: the same bits on every run.
//
//   convt_pack_train_kernel      fp32 master weight (Cin, Cout, 4, 4) -> the forward packing [phase][Cout][tap][Cin] (the bits of ops16.pack_conv_transpose16 of
//     the rounded weight) AND the data-gradient packing [Cin][ky 4 + kx][Cout] (Cout contiguous: K-major for that GEMM) in one pass: a 32 ci x 32 co x 16 tile is
//     rounded on the way into LDS (odd dword strides: both write orders read it conflict-free) and leaves it twice, once ci-fastest, once co-fastest.
//   convt16_bwd_data_kernel      dx[n][y][x][ci] = sum_{ky,kx,co} dz[n][2y - 1 + ky][2x - 1 + kx][co] W[ci][co][ky][kx]: in frame coordinates row 2y + ky, column
//     2x + kx of the padded dz -- a 4 x 4 stride-2 convolution with no boundary case.  Implicit GEMM M = N Hi Wi, N = Cin, K = 16 Cout, the structure of
//     convt16_kernel: a workgroup owns 16 input channels and 16 MT pixels, its WAVES split K in chunks of 64 (chunk i goes to wave i % WAVES whatever the mask),
//     W is the MFMA A operand straight from global memory, the partial tiles meet in LDS and are added in wave order.  tap_mask: bit 4 ky + kx set = the tap is
//     read; ky in {0, 3} only meets the border when Hi == 1, kx in {0, 3} when Wi == 1: at 1 x 1 a quarter of the weight is streamed.
//   convt_small16_bwd_data_kernel    Cout < 16 (the last layer): dz is UNPADDED fp32 NCHW, the layout of the loss gradient; thread = one dx element, the packed
//     weight transposed into LDS ([k][Cin]: consecutive lanes, consecutive 16-bit words), bounds checked per tap.
//   convt16_bwd_weight_kernel    dW[ci][co][ky][kx] = sum_{n,y,x} x[n][y][x][ci] dz[n][2y - 1 + ky][2x - 1 + kx][co].  Both operands are pixel-major, K (pixels) is the
//     slow index: a k-tile of 32 pixels of x (64 channels, 160-byte LDS rows) and of the pixels' 4 x 4 dz windows (16 taps x 16 channels, 544-byte rows; either
//     way the 8 rows x 32 bytes of a half-wave's transpose read cover the 64 banks once) is staged in LDS and the fragments come out through
//     ds_read_b64_tr_b16, as in csrc/wgrad_tok.hip.  Workgroup = (64 ci, 16 co, K slab) with ALL 16 taps; wave w owns ci 16 w .. + 15: a lane ends with the 16
//     taps of one (ci, co), one whole 64-byte line of torch's layout, and 16 lanes write 1 KB runs (a lane holding only the 4 kx of one ky would write 16-byte pieces 64 bytes apart
//     and every line of the first layer's 528 MB gradient four times partially).  db[co] = sum of dz over the interior = the taps ky, kx in {1, 2}
//     summed over the pixels: an all-ones A fragment in wave 0 of the ci-tile-0 workgroups.  slabs == 1: dW is written directly (divided by loss_scale); else
//     slab s goes to the workspace and convt_bwd_weight_reduce_kernel adds the slabs in order.  Dead taps (Hi == 1 / Wi == 1) get exact zeros, nothing read.
//   convt_small16_bwd_weight_kernel  Cout < 16: thread = one (ci, co) with its 16 taps in registers, fp32 dz NCHW, K slabs over workgroups -> workspace -> reduce.
#include "half16.h"

#include <string.h>

namespace eeg {

// ---------------------------------------------------------------------------------------------------------------------------------------- pack
constexpr int CP_T = 32;                        // tile side (ci and co)
constexpr int CP_CO = 18;                       // 16-bit elements per (ci, co) cell: 16 taps + 2 (9 dwords: odd)
constexpr int CP_CI = CP_T * CP_CO + 2;         // ... per ci row: 289 dwords (odd)

template <bool F16>
__global__ __launch_bounds__(256) void convt_pack_train_kernel(const float* __restrict__ W, unsigned short* __restrict__ wf, unsigned short* __restrict__ wb, int Cin,
                                                               int Cout) {
    EEG_LDS_BASE(unsigned short, tile);                                     // [ci 32][co 32][k 16] with the strides above
    const int ci0 = blockIdx.x * CP_T, co0 = blockIdx.y * CP_T;
    const int nco = Cout - co0 < CP_T ? Cout - co0 : CP_T;
    for (int i = threadIdx.x; i < CP_T * CP_T * 4; i += 256) {              // one float4 (4 kx of one ky) per step; a ci row of the tile is contiguous in W
        const int ci = i >> 7, co = (i >> 2) & 31, ky = i & 3;
        unsigned lo = 0, hi = 0;
        if (co < nco) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(W + ((long long)(ci0 + ci) * Cout + co0 + co) * 16 + 4 * ky);
            lo = pack2<F16>(v[0], v[1]);
            hi = pack2<F16>(v[2], v[3]);
        }
        unsigned* d = reinterpret_cast<unsigned*>(tile + ci * CP_CI + co * CP_CO + 4 * ky);
        d[0] = lo;
        d[1] = hi;
    }
    __syncthreads();
    // forward packing [phase][Cout][tap][Cin]: pairs of ci per lane
    for (int i = threadIdx.x; i < 16 * CP_T * (CP_T / 2); i += 256) {
        const int ci = 2 * (i & 15), co = (i >> 4) & 31, pt = i >> 9;
        if (co >= nco) continue;
        const int phase = pt >> 2, tap = pt & 3, py = phase >> 1, px = phase & 1, ty = tap >> 1, tx = tap & 1;
        const int ky = ty ? (py ? 0 : 3) : (py ? 2 : 1), kx = tx ? (px ? 0 : 3) : (px ? 2 : 1);
        const unsigned short* s = tile + ci * CP_CI + co * CP_CO + 4 * ky + kx;
        *reinterpret_cast<unsigned*>(wf + ((long long)(phase * Cout + co0 + co) * 4 + tap) * Cin + ci0 + ci) = (unsigned)s[0] | ((unsigned)s[CP_CI] << 16);
    }
    // data-gradient packing [Cin][16][Cout]: co fastest
    for (int i = threadIdx.x; i < CP_T * 16 * CP_T; i += 256) {
        const int co = i & 31, k = (i >> 5) & 15, ci = i >> 9;
        if (co < nco) wb[((long long)(ci0 + ci) * 16 + k) * Cout + co0 + co] = tile[ci * CP_CI + co * CP_CO + k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------- data gradient
struct cbd_args {
    const unsigned short *dz, *W;
    const float* dzf;
    unsigned short* dx;
    int N, Hi, Wi, Cin, Cout, M, mask;
};

template <bool F16, int WAVES, int MT, int U>
__global__ __launch_bounds__(64 * WAVES) void convt16_bwd_data_kernel(const cbd_args a) {
    EEG_LDS_BASE(float, red);                                               // [WAVES][MT][pixel 16][ci 16]
    const int lane = threadIdx.x & 63, wave = wave_uniform((int)(threadIdx.x >> 6));
    const int fr = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16 * MT;
    const int nch = a.Cout / 64;
    const int Wop = 2 * a.Wi + 2, Hop = 2 * a.Hi + 2, hw = a.Hi * a.Wi;
    const unsigned short* wp = a.W + ((long long)(n0 + fr) * 16) * a.Cout + 16 * g;
    const unsigned short* zp[MT];
    bool live[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int q = m0 + 16 * j + fr;
        live[j] = q < a.M;                                                 // pixels past M: zeros, never read
        const int qq = live[j] ? q : 0;
        const int n_ = qq / hw, rem = qq - n_ * hw, y = rem / a.Wi, x = rem - y * a.Wi;
        zp[j] = a.dz + (((long long)n_ * Hop + 2 * y) * Wop + 2 * x) * a.Cout + 16 * g;      // tap (0, 0) of this pixel's 4 x 4 window
    }
    const bf16x8 zero{0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int slots = 16 * nch;
    for (int i0 = wave; i0 < slots; i0 += WAVES * U) {
        bf16x8 w[U][2], z[U][MT][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * WAVES;
            const int tap = i / nch, c = i - tap * nch;                    // (wave-uniform)
            w[u][0] = w[u][1] = zero;
#pragma unroll
            for (int j = 0; j < MT; ++j) z[u][j][0] = z[u][j][1] = zero;
            if (i < slots && ((a.mask >> tap) & 1)) {
                const long long toff = ((long long)(tap >> 2) * Wop + (tap & 3)) * a.Cout + 64 * c;
                const unsigned short* wq = wp + (long long)tap * a.Cout + 64 * c;
                w[u][0] = *reinterpret_cast<const bf16x8*>(wq);
                w[u][1] = *reinterpret_cast<const bf16x8*>(wq + 8);
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    if (live[j]) {
                        z[u][j][0] = *reinterpret_cast<const bf16x8*>(zp[j] + toff);
                        z[u][j][1] = *reinterpret_cast<const bf16x8*>(zp[j] + toff + 8);
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)                                        // (a dead or absent slot multiplies zeros)
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                acc[j] = mma<F16>(w[u][0], z[u][j][0], acc[j]);            // D[ci = 4g + r][pixel = fr]
                acc[j] = mma<F16>(w[u][1], z[u][j][1], acc[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) *reinterpret_cast<f32x4*>(red + (wave * MT + j) * 256 + fr * 16 + 4 * g) = acc[j];
    __syncthreads();
    const int Hp = a.Hi + 2, Wp = a.Wi + 2;
    for (int idx = threadIdx.x; idx < MT * 256; idx += 64 * WAVES) {
        const int j = idx >> 8, r = idx & 255, q = m0 + 16 * j + (r >> 4), ci = n0 + (r & 15);
        if (q >= a.M) continue;
        float v = red[j * 256 + r];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += red[(w * MT + j) * 256 + r];
        const int n_ = q / hw, rem = q - n_ * hw, y = rem / a.Wi, x = rem - y * a.Wi;
        a.dx[(((long long)n_ * Hp + y + 1) * Wp + x + 1) * a.Cin + ci] = to_h<F16>(v);
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void convt_small16_bwd_data_kernel(const cbd_args a) {
    EEG_LDS_BASE(unsigned short, wl);                                       // [k = (4 ky + kx) Cout + co][Cin]
    const int K = 16 * a.Cout;
    for (int i = threadIdx.x; i < a.Cin * K; i += 256) {
        const int ci = i / K, k = i - ci * K;
        wl[k * a.Cin + ci] = a.W[i];
    }
    __syncthreads();
    const int Ho = 2 * a.Hi, Wo = 2 * a.Wi, Hp = a.Hi + 2, Wp = a.Wi + 2;
    const long long total = (long long)a.M * a.Cin;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int ci = (int)(q % a.Cin);
        const int p = (int)(q / a.Cin);
        const int x = p % a.Wi, p1 = p / a.Wi, y = p1 % a.Hi, n_ = p1 / a.Hi;
        float acc = 0.f;
        for (int ky = 0; ky < 4; ++ky) {
            const int oy = 2 * y - 1 + ky;
            if (oy < 0 || oy >= Ho) continue;
            for (int kx = 0; kx < 4; ++kx) {
                const int ox = 2 * x - 1 + kx;
                if (ox < 0 || ox >= Wo) continue;
                const float* zq = a.dzf + ((long long)n_ * a.Cout * Ho + oy) * Wo + ox;
                const unsigned short* w = wl + (4 * ky + kx) * a.Cout * a.Cin + ci;
                for (int co = 0; co < a.Cout; ++co) acc += zq[(long long)co * Ho * Wo] * to_f32<F16>(w[co * a.Cin]);
            }
        }
        a.dx[(((long long)n_ * Hp + y + 1) * Wp + x + 1) * a.Cin + ci] = to_h<F16>(acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------- weight gradient
constexpr int CW_ROWB = 160;                    // bytes per LDS row of the x tile, 64 channels (128 + 32: rows r .. r + 7 start 40 banks apart -> 8 x 32 B cover 64 banks)
constexpr int CW_ZROWB = 544;                   // ... of the dz tile, 16 taps x 16 channels (512 + 32: rows start 8 banks apart, the same cover)
constexpr int CW_LDS = 32 * (CW_ROWB + CW_ZROWB);

struct cbw_args {
    const unsigned short *x, *dz;
    const float* dzf;
    float *out, *dbp;                           // dW itself (slabs == 1) or the workspace slabs; db partials [slab][Cout]
    int N, Hi, Wi, Cin, Cout, M, slabs, kt_total;
    float inv_scale;
};

template <bool F16>
__global__ __launch_bounds__(256) void convt16_bwd_weight_kernel(const cbw_args a) {
    EEG_LDS_BASE(unsigned char, lds);
    unsigned char* const zs = lds + 32 * CW_ROWB;
    const int t = threadIdx.x, lane = t & 63, wave = wave_uniform(t >> 6), fr = lane & 15, g = lane >> 4;
    const int ci0 = 64 * blockIdx.x, co0 = 16 * blockIdx.y, slab = blockIdx.z;
    const int kt0 = (int)((long long)slab * a.kt_total / a.slabs), kt1 = (int)((long long)(slab + 1) * a.kt_total / a.slabs);
    const int lky = a.Hi == 1 ? 6 : 15, lkx = a.Wi == 1 ? 6 : 15;          // live ky / kx: {0, 3} only meet the border of dz at one row / column
    const bool dob = blockIdx.x == 0 && wave == 0;                          // (wave-uniform)
    const int Hp = a.Hi + 2, Wp = a.Wi + 2, Hop = 2 * a.Hi + 2, Wop = 2 * a.Wi + 2, hw = a.Hi * a.Wi;
    f32x4 acc[16], bacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (short)(F16 ? 0x3C00 : 0x3F80);
    const int srow = t >> 3, sch = t & 7;                                   // x staging: pixel row of the k-tile, 16-byte chunk of its 64 channels
    const int frow = 4 * g + (fr >> 2), fcol = 8 * (fr & 3);                // transpose-read role: row and byte offset within a 16-channel block
    auto frag = [&](const unsigned char* p, int rowb) {
        const s16x4 u = lds_read_tr16(p), v = lds_read_tr16(p + 16 * rowb);
        return bf16x8{u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
    };
    for (int kt = kt0; kt < kt1; ++kt) {
        const bf16x8 zero{0, 0, 0, 0, 0, 0, 0, 0};
        bf16x8 xv = zero, zv[4];
        {
            const int p = 32 * kt + srow;
            if (p < a.M) {
                const int n_ = p / hw, rem = p - n_ * hw, y = rem / a.Wi, x = rem - y * a.Wi;
                xv = *reinterpret_cast<const bf16x8*>(a.x + (((long long)n_ * Hp + y + 1) * Wp + x + 1) * a.Cin + ci0 + 8 * sch);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                       // dz: piece j = (pixel, tap, half of the 16 channels), 1024 pieces of 16 bytes
            const int j = t + 256 * i, p = 32 * kt + (j >> 5), tap = (j >> 1) & 15, ky = tap >> 2, kx = tap & 3;
            zv[i] = zero;
            if (p < a.M && ((lky >> ky) & 1) && ((lkx >> kx) & 1)) {
                const int n_ = p / hw, rem = p - n_ * hw, y = rem / a.Wi, x = rem - y * a.Wi;
                zv[i] = *reinterpret_cast<const bf16x8*>(a.dz + (((long long)n_ * Hop + 2 * y + ky) * Wop + 2 * x + kx) * a.Cout + co0 + 8 * (j & 1));
            }
        }
        __syncthreads();                                                    // every wave's reads of the previous k-tile are complete
        *reinterpret_cast<bf16x8*>(lds + srow * CW_ROWB + 16 * sch) = xv;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = t + 256 * i;
            *reinterpret_cast<bf16x8*>(zs + (j >> 5) * CW_ZROWB + 16 * (j & 31)) = zv[i];
        }
        __syncthreads();
        const bf16x8 af = frag(lds + frow * CW_ROWB + 32 * wave + fcol, CW_ROWB);
#pragma unroll
        for (int tap = 0; tap < 16; ++tap) {
            if (!((lky >> (tap >> 2)) & 1) || !((lkx >> (tap & 3)) & 1)) continue;       // (uniform)
            const bf16x8 bf = frag(zs + frow * CW_ZROWB + 32 * tap + fcol, CW_ZROWB);
            acc[tap] = mma<F16>(af, bf, acc[tap]);                          // D[ci = 4g + r][co = fr]
            if (dob && (tap == 5 || tap == 6 || tap == 9 || tap == 10)) bacc = mma<F16>(ones, bf, bacc);
        }
    }
    const float s = a.slabs == 1 ? a.inv_scale : 1.f;
    float* out = a.out + (a.slabs == 1 ? 0 : (long long)slab * a.Cin * a.Cout * 16);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ci = ci0 + 16 * wave + 4 * g + r, co = co0 + fr;
        float* o = out + ((long long)ci * a.Cout + co) * 16;               // the 16 taps of one (ci, co): one 64-byte line
#pragma unroll
        for (int ky = 0; ky < 4; ++ky)
            *reinterpret_cast<f32x4*>(o + 4 * ky) = f32x4{acc[4 * ky][r] * s, acc[4 * ky + 1][r] * s, acc[4 * ky + 2][r] * s, acc[4 * ky + 3][r] * s};
    }
    if (dob && g == 0) a.dbp[(long long)slab * a.Cout + co0 + fr] = bacc[0];
}

template <bool F16>
__global__ __launch_bounds__(256) void convt_small16_bwd_weight_kernel(const cbw_args a) {
    const int e = blockIdx.y * 256 + threadIdx.x, slab = blockIdx.x;
    if (e >= a.Cin * a.Cout) return;
    const int ci = e % a.Cin, co = e / a.Cin;
    const int p0 = (int)((long long)slab * a.M / a.slabs), p1 = (int)((long long)(slab + 1) * a.M / a.slabs);
    const int Ho = 2 * a.Hi, Wo = 2 * a.Wi, Hp = a.Hi + 2, Wp = a.Wi + 2;
    float acc[16], bsum = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
    for (int p = p0; p < p1; ++p) {                                         // (the pixel is uniform over the workgroup: so is every bounds check)
        const int x = p % a.Wi, q1 = p / a.Wi, y = q1 % a.Hi, n_ = q1 / a.Hi;
        const float xv = to_f32<F16>(a.x[(((long long)n_ * Hp + y + 1) * Wp + x + 1) * a.Cin + ci]);
        const float* zq = a.dzf + ((long long)n_ * a.Cout + co) * Ho * Wo;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const int oy = 2 * y - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const int ox = 2 * x - 1 + kx;
                if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
                    const float zv = zq[(long long)oy * Wo + ox];
                    acc[4 * ky + kx] += xv * zv;
                    if ((ky == 1 || ky == 2) && (kx == 1 || kx == 2)) bsum += zv;      // each interior element of dz exactly once
                }
            }
        }
    }
    float* o = a.out + (long long)slab * a.Cin * a.Cout * 16 + ((long long)ci * a.Cout + co) * 16;
#pragma unroll
    for (int k = 0; k < 16; k += 4) *reinterpret_cast<f32x4*>(o + k) = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
    if (ci == 0) a.dbp[(long long)slab * a.Cout + co] = bsum;
}

// dW = (sum of the slabs in slab order) / loss_scale (from_ws; 4 elements per thread), db = (sum of its partial rows in order) / loss_scale
__global__ __launch_bounds__(256) void convt_bwd_weight_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW, long long n4, int slabs, int from_ws,
                                                                      const float* __restrict__ dbp, float* __restrict__ db, int Cout, int nb, float inv_scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (from_ws && i < n4) {
        f32x4 s = reinterpret_cast<const f32x4*>(ws)[i];
        for (int k = 1; k < slabs; ++k) {
            const f32x4 v = reinterpret_cast<const f32x4*>(ws)[(long long)k * n4 + i];
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += v[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] *= inv_scale;
        reinterpret_cast<f32x4*>(dW)[i] = s;
    }
    if (db && i < Cout) {
        float s = dbp[i];
        for (int k = 1; k < nb; ++k) s += dbp[(long long)k * Cout + i];
        db[i] = s * inv_scale;
    }
}

}  // namespace eeg

using namespace eeg;

constexpr int CB_SMALL_LDS = 64 * 1024;         // the direct forms' packed weights: 16 Cout Cin 16-bit elements

static bool cb_dtype_ok(int dt) { return dt == EEGCLIP_DT_BF16 || dt == EEGCLIP_DT_F16; }

// the shapes both gradients take: Cin a multiple of 64; Cout a multiple of 64 (matrix-core forms) or below 16 with the weight within the direct forms' LDS
static int cb_shape(int N, int Hi, int Wi, int Cin, int Cout) {
    if (N < 1 || Hi < 1 || Wi < 1 || Hi > 16384 || Wi > 16384 || Cin < 64 || Cin % 64 || Cout < 1) return EEGCLIP_EINVAL;
    if (Cout >= 16 ? Cout % 64 != 0 : (long long)32 * Cout * Cin > CB_SMALL_LDS) return EEGCLIP_EINVAL;
    if ((long long)N * Hi * Wi > 0x7fffffffLL / 16) return EEGCLIP_EINVAL;
    return 0;
}

extern "C" int eegclip_convt16_pack_train(const float* W, void* fwd, void* bwd, int Cin, int Cout, int dtype, void* stream) {
    if (!W || !fwd || !bwd || Cin < 64 || Cin % 64 || Cout < 1 || !cb_dtype_ok(dtype) || (Cout >= 16 && Cout % 16)) return EEGCLIP_EINVAL;
    if ((Cout + CP_T - 1) / CP_T > 65535) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(W) & 15u) || ((reinterpret_cast<uintptr_t>(fwd) | reinterpret_cast<uintptr_t>(bwd)) & 3u)) return EEGCLIP_EALIGN;
    const dim3 grid((unsigned)(Cin / CP_T), (unsigned)((Cout + CP_T - 1) / CP_T));
    const size_t lds = (size_t)CP_T * CP_CI * 2;
    if (dtype == EEGCLIP_DT_F16)
        EEG_LAUNCH(convt_pack_train_kernel<true>, grid, dim3(256), lds, stream, W, static_cast<unsigned short*>(fwd), static_cast<unsigned short*>(bwd), Cin, Cout);
    else
        EEG_LAUNCH(convt_pack_train_kernel<false>, grid, dim3(256), lds, stream, W, static_cast<unsigned short*>(fwd), static_cast<unsigned short*>(bwd), Cin, Cout);
    return (int)hipGetLastError();
}

template <bool F16>
static int cbd_launch(const cbd_args& a, void* stream) {
    if (a.Cout < 16) {
        long long g = ((long long)a.M * a.Cin + 1023) / 1024;
        if (g > 4096) g = 4096;
        EEG_LAUNCH((convt_small16_bwd_data_kernel<F16>), dim3((unsigned)g), dim3(256), (size_t)32 * a.Cout * a.Cin, stream, a);
        return 0;
    }
    const bool wide = a.M > 64;
    const int mt = (a.M + (wide ? 63 : 15)) / (wide ? 64 : 16);
    if (mt > 65535) return EEGCLIP_EINVAL;
    const dim3 grid((unsigned)(a.Cin / 16), (unsigned)mt);
    if (wide) EEG_LAUNCH((convt16_bwd_data_kernel<F16, 8, 4, 2>), grid, dim3(512), 8 * 4 * 1024, stream, a);
    else      EEG_LAUNCH((convt16_bwd_data_kernel<F16, 16, 1, 4>), grid, dim3(1024), 16 * 1024, stream, a);
    return 0;
}

extern "C" int eegclip_convt16_bwd_data(const eegclip_convt16_bwd_data_desc* d, void* stream) {
    if (!d || !d->dz || !d->W || !d->dx || !cb_dtype_ok(d->dtype)) return EEGCLIP_EINVAL;
    if (const int rc = cb_shape(d->N, d->Hi, d->Wi, d->Cin, d->Cout)) return rc;
    // the mask names the 16 taps only and keeps every tap that meets the interior of dz for some pixel
    int need = 0;
    for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx)
            if (!((ky == 0 || ky == 3) && d->Hi == 1) && !((kx == 0 || kx == 3) && d->Wi == 1)) need |= 1 << (4 * ky + kx);
    if ((d->tap_mask & ~0xffff) || (d->tap_mask & need) != need) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->dz) | reinterpret_cast<uintptr_t>(d->W)) & 15u) return EEGCLIP_EALIGN;
    if (reinterpret_cast<uintptr_t>(d->dx) & 1u) return EEGCLIP_EALIGN;
    const cbd_args a{static_cast<const unsigned short*>(d->dz), static_cast<const unsigned short*>(d->W), static_cast<const float*>(d->dz),
                     static_cast<unsigned short*>(d->dx), d->N, d->Hi, d->Wi, d->Cin, d->Cout, d->N * d->Hi * d->Wi, d->tap_mask};
    const int rc = d->dtype == EEGCLIP_DT_F16 ? cbd_launch<true>(a, stream) : cbd_launch<false>(a, stream);
    return rc ? rc : (int)hipGetLastError();
}

extern "C" int eegclip_convt16_bwd_weight_slabs(int N, int Hi, int Wi, int Cin, int Cout) {
    if (cb_shape(N, Hi, Wi, Cin, Cout)) return 0;
    const int M = N * Hi * Wi;
    if (Cout < 16) {                                                        // direct form: slabs of at least 64 pixels
        const int s = M / 64;
        return s < 1 ? 1 : s > 256 ? 256 : s;
    }
    const long long tiles = (long long)(Cin / 64) * (Cout / 16);
    const int kt = (M + 31) / 32;
    long long s = 512 / tiles;                                              // two workgroups per CU
    if (s > 32) s = 32;                                                     // (more slabs: their traffic outgrows what the extra workgroups gain)
    if (s > kt / 2) s = kt / 2;                                             // at least two k-tiles per slab
    return s < 1 ? 1 : (int)s;
}

extern "C" long long eegclip_convt16_bwd_weight_workspace_floats(int N, int Hi, int Wi, int Cin, int Cout, int slabs) {
    if (cb_shape(N, Hi, Wi, Cin, Cout) || slabs < 1) return 0;
    const long long n = (long long)Cin * Cout * 16;
    if (Cout < 16) return (long long)slabs * (n + Cout);
    return (slabs > 1 ? (long long)slabs * n : 0) + (long long)slabs * Cout;
}

extern "C" int eegclip_convt16_bwd_weight(const eegclip_convt16_bwd_weight_desc* d, void* stream) {
    if (!d || !d->x || !d->dz || !d->dW || !d->workspace || !cb_dtype_ok(d->dtype) || !(d->loss_scale > 0.f)) return EEGCLIP_EINVAL;
    if (const int rc = cb_shape(d->N, d->Hi, d->Wi, d->Cin, d->Cout)) return rc;
    const int M = d->N * d->Hi * d->Wi, kt = (M + 31) / 32;
    const bool small = d->Cout < 16;
    if (d->slabs < 1 || d->slabs > (small ? M : kt) || d->slabs > 4096) return EEGCLIP_EINVAL;
    if (d->workspace_floats < eegclip_convt16_bwd_weight_workspace_floats(d->N, d->Hi, d->Wi, d->Cin, d->Cout, d->slabs)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->x) | reinterpret_cast<uintptr_t>(d->dz) | reinterpret_cast<uintptr_t>(d->dW) | reinterpret_cast<uintptr_t>(d->workspace)) & 15u)
        return EEGCLIP_EALIGN;
    if (reinterpret_cast<uintptr_t>(d->db) & 3u) return EEGCLIP_EALIGN;
    const long long n = (long long)d->Cin * d->Cout * 16;
    const bool from_ws = small || d->slabs > 1;
    float* dbp = d->workspace + (from_ws ? (long long)d->slabs * n : 0);
    const cbw_args a{static_cast<const unsigned short*>(d->x), static_cast<const unsigned short*>(d->dz), static_cast<const float*>(d->dz),
                     from_ws ? d->workspace : d->dW, dbp, d->N, d->Hi, d->Wi, d->Cin, d->Cout, M, d->slabs, kt, 1.f / d->loss_scale};
    const bool f16 = d->dtype == EEGCLIP_DT_F16;
    if (small) {
        const dim3 grid((unsigned)d->slabs, (unsigned)((d->Cin * d->Cout + 255) / 256));
        if (f16) EEG_LAUNCH(convt_small16_bwd_weight_kernel<true>, grid, dim3(256), 0, stream, a);
        else     EEG_LAUNCH(convt_small16_bwd_weight_kernel<false>, grid, dim3(256), 0, stream, a);
    } else {
        if (d->Cout / 16 > 65535 || d->slabs > 65535) return EEGCLIP_EINVAL;
        const dim3 grid((unsigned)(d->Cin / 64), (unsigned)(d->Cout / 16), (unsigned)d->slabs);
        if (f16) EEG_LAUNCH(convt16_bwd_weight_kernel<true>, grid, dim3(256), CW_LDS, stream, a);
        else     EEG_LAUNCH(convt16_bwd_weight_kernel<false>, grid, dim3(256), CW_LDS, stream, a);
    }
    if (from_ws || d->db) {
        const long long n4 = n / 4, work = from_ws ? n4 : d->Cout;
        EEG_LAUNCH(convt_bwd_weight_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, d->workspace, d->dW, n4, d->slabs, (int)from_ws, dbp, d->db,
                   d->Cout, d->slabs, 1.f / d->loss_scale);
    }
    return (int)hipGetLastError();
}
