// The reference's reconstruction metrics that need no pretrained network (the ..._metrics_sub8.ipynb notebooks under Generation/, Reconstruction_Metrics_ATM.ipynb; MindEye's
// Reconstruction_Metrics): PixCorr, SSIM and two-way identification, on images / features that are already on the GPU.
//
//   pixcorr_ssim   grid (column tiles, row tiles, B), 256 threads, one TH x TW tile of one image pair (B, 3, H, W) per workgroup:
//       1. stage (x, y) = gray - 0.5 (gray = 0.2125 R + 0.7154 G + 0.0721 B, skimage's rgb2gray) of the tile plus a 5-pixel halo of both images in LDS as
//          pairs ([TH + 10][TW + 12] float2; outside the image: 0, only ever used by pixels that are not counted).  Four positions per lane and trip, their 24
//          loads issued before the first use (addresses clamped into the image, the value selected afterwards).  The lanes that hold the tile's OWN pixels
//          add the five raw PixCorr moments (sum a, b, aa, bb, ab over the 3 channels) in fp64 and keep min / max of a and b: each input element is read
//          from HBM once, a halo element comes from a neighbouring tile's lines in cache.
//       2. horizontal 11-tap Gaussian (sigma 1.5, taps normalised in double on the host) of x, y, xx, yy, xy: a lane owns 4 neighbouring columns of a row
//          (8 x 16-byte LDS reads for 14 staged pairs), forms the products once and runs the taps as packed fp32 FMAs on the pairs (x, y) and (xx, yy) plus
//          one scalar FMA for xy -> LDS [TH + 10][TW] as float2, float2, float.
//       3. vertical pass: a lane owns 4 neighbouring rows of a column (lanes along the row: 8- and 4-byte LDS reads without bank conflicts), the same
//          three FMAs per tap, then S in fp32 registers, summed in fp64 over the pixels at least 5 from every border.
//       4. the workgroup's 6 sums + 4 extrema (through LDS: the 4 waves' values added in order, then wave 0's butterflies) -> workspace[(image, tile)][10] (fp64).
//     The moments of the gray images are taken about 0.5: variances and the covariance do not move, the means get the 0.5 back, and E[xx] - mu^2 cancels
//     a tenth of the digits it does on the raw values.  Every S is a fixed expression of its 121 neighbours, so it does not depend on the tiling.
//   pixcorr_ssim_finalize   one wave per image adds the tile rows in a fixed order: ssim = sum S / ((H - 10)(W - 10)); pixcorr = cov / sqrt(var_a var_b) from
//     the fp64 moments, NaN when an image is constant (min == max: what numpy's corrcoef gives for it).
//   No atomics, nothing to clear.  Tile 32 x 32 (smaller, down to 4 x 16, while there are fewer workgroups than CUs): the horizontal pass covers
//   (TH + 10) / TH = 1.31 x the rows it owns, 1.63 x at 16 rows; LDS 4 (2 (TH + 10)(TW + 12) + 5 (TH + 10) TW) = 41664 bytes, three workgroups per CU.
//   The kernel is bound by the vector ALU, not by HBM: 1,309 vector instructions per wave, the VALU active for a third of each of the three waves a SIMD holds
//   (profiles/recon_metrics_pmc.txt); 200 pairs of 425 x 425 take 529 us, 4.9 x the time of their bytes at 8 TB/s (profiles/recon_metrics_bench.json).
//
//   two_way   count[j] = #{ i != j : r[i][j] < r[j][j] }, r = Pearson correlation of row i of G with row j of P, without the N x N matrix in memory:
//       two_way_stats  one workgroup per row j: mean of G[j] and P[j], then the centred sums of squares and the centred cross sum, all in fp64
//                      (16 elements per lane and trip in flight) -> mean, 1 / centred norm (fp32) of both rows and diag[j] = r[j][j];
//       two_way_tile   one workgroup of 16 waves per 16 x 16 tile of r: rows centred in fp32 on load, exact fp32 products on the matrix cores (16x16x4 f32
//                      MFMA), the k range dealt to the waves in steps of 16, four steps' loads in flight, and the waves' accumulators added in LDS in wave
//                      order; r[i][j] = acc ig[i] ip[j] (stored if the caller wants r), compared with diag[j], and the tile's count per column
//                      -> part[row tile][j];
//       two_way_counts count[j] = sum over the row tiles in order.
#include "half16.h"

#include <cmath>

namespace eeg {

constexpr int RM_CUS = 256;                                   // MI355X
constexpr int RM_HALO = 5, RM_TAPS = 11;
constexpr int RM_PART = 10;                                   // doubles per (image, tile): sum S, a, b, aa, bb, ab, min a, max a, min b, max b

constexpr size_t RM_RED_BYTES = 6 * 256 * sizeof(double) + 4 * 256 * sizeof(float);

struct RmTaps { float w[RM_TAPS]; };

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

template <int SRC>
__device__ __forceinline__ float rm_load(const void* p, long long i) {
    return SRC == 2 ? static_cast<const float*>(p)[i] : to_f32<SRC == 1>(static_cast<const unsigned short*>(p)[i]);
}

// sums the four waves' values in wave order; every thread gets the result.  red: 4 doubles of LDS
__device__ __forceinline__ double rm_block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) {        // v_pk_fma_f32
#if defined(EEG_EMU)
    return f32x2{fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1])};
#else
    return __builtin_elementwise_fma(a, b, c);
#endif
}
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// LW = log2(TW)
template <int SRC>
__global__ __launch_bounds__(256) void pixcorr_ssim_kernel(const void* __restrict__ A, const void* __restrict__ Bm, int H, int W, int TH, int LW, RmTaps taps,
                                                            double* __restrict__ ws) {
    EEG_LDS_BASE(float, lds);
    const int TW = 1 << LW, R = TH + 2 * RM_HALO, SW = TW + 12;
    f32x2* G = reinterpret_cast<f32x2*>(lds);                 // [R][SW] (x, y)   staged column s is image column x0 - 5 + s
    f32x2* F01 = G + R * SW;                                  // [R][TW] (mean x, mean y)
    f32x2* F23 = F01 + R * TW;                                // [R][TW] (mean xx, mean yy)
    float* F4 = reinterpret_cast<float*>(F23 + R * TW);       // [R][TW] mean xy
    const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, img = blockIdx.z;
    const long long plane = (long long)H * W, base = (long long)img * 3 * plane;

    // 1. stage + PixCorr moments of the tile's own elements
    double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
    float amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
    const int total = R * SW;
    const float inv_sw = 1.0f / (float)SW;                    // idx / SW as a product: (idx + 0.5) / SW is at least 0.5 / SW from an integer, idx < 2^12
    for (int i0 = tid; i0 < total; i0 += 4 * 256) {
        float a[4][3], b[4][3];
        bool in[4], own[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = i0 + u * 256, r = (int)(((float)idx + 0.5f) * inv_sw), s = idx - r * SW, y = y0 - RM_HALO + r, x = x0 - RM_HALO + s;
            in[u] = idx < total && y >= 0 && y < H && x >= 0 && x < W && s < TW + 2 * RM_HALO;
            own[u] = in[u] && r >= RM_HALO && r < RM_HALO + TH && s >= RM_HALO && s < RM_HALO + TW;
            const long long o = base + (long long)imin(imax(y, 0), H - 1) * W + imin(imax(x, 0), W - 1);      // always inside the image
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a[u][c] = rm_load<SRC>(A, o + c * plane);
                b[u][c] = rm_load<SRC>(Bm, o + c * plane);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = i0 + u * 256;
            const float vx = fmaf(0.0721f, a[u][2], fmaf(0.7154f, a[u][1], 0.2125f * a[u][0])) - 0.5f;
            const float vy = fmaf(0.0721f, b[u][2], fmaf(0.7154f, b[u][1], 0.2125f * b[u][0])) - 0.5f;
            if (idx < total) G[idx] = in[u] ? f32x2{vx, vy} : f32x2{0.f, 0.f};
            if (own[u]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double da = a[u][c], db = b[u][c];
                    sa += da;
                    sb += db;
                    saa = fma(da, da, saa);
                    sbb = fma(db, db, sbb);
                    sab = fma(da, db, sab);
                    amin = fminf(amin, a[u][c]);
                    amax = fmaxf(amax, a[u][c]);
                    bmin = fminf(bmin, b[u][c]);
                    bmax = fmaxf(bmax, b[u][c]);
                }
            }
        }
    }
    __syncthreads();

    // 2. horizontal pass: 4 columns of one row per item
    for (int idx = tid; idx < (R << (LW - 2)); idx += 256) {
        const int r = idx >> (LW - 2), c = (idx - (r << (LW - 2))) * 4;
        f32x2 p[16], q[14];
        float xy[14];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(G + r * SW + c + 2 * k);
            p[2 * k] = f32x2{v[0], v[1]};
            p[2 * k + 1] = f32x2{v[2], v[3]};
        }
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            q[k] = p[k] * p[k];
            xy[k] = p[k][0] * p[k][1];
        }
        f32x2 m01[4], m23[4];
        float m4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m01[e] = m23[e] = f32x2{0.f, 0.f};
            m4[e] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < RM_TAPS; ++j) {
            const f32x2 w2 = {taps.w[j], taps.w[j]};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                m01[e] = fma2(w2, p[e + j], m01[e]);
                m23[e] = fma2(w2, q[e + j], m23[e]);
                m4[e] = fmaf(taps.w[j], xy[e + j], m4[e]);
            }
        }
        *reinterpret_cast<f32x4*>(F01 + r * TW + c) = f32x4{m01[0][0], m01[0][1], m01[1][0], m01[1][1]};
        *reinterpret_cast<f32x4*>(F01 + r * TW + c + 2) = f32x4{m01[2][0], m01[2][1], m01[3][0], m01[3][1]};
        *reinterpret_cast<f32x4*>(F23 + r * TW + c) = f32x4{m23[0][0], m23[0][1], m23[1][0], m23[1][1]};
        *reinterpret_cast<f32x4*>(F23 + r * TW + c + 2) = f32x4{m23[2][0], m23[2][1], m23[3][0], m23[3][1]};
        *reinterpret_cast<f32x4*>(F4 + r * TW + c) = f32x4{m4[0], m4[1], m4[2], m4[3]};
    }
    __syncthreads();

    // 3. vertical pass: 4 rows of one column per item, S, the sum over the counted pixels
    double ss = 0.0;
    for (int idx = tid; idx < ((TH / 4) << LW); idx += 256) {
        const int g = idx >> LW, c = idx - (g << LW), t0 = g * 4;
        f32x2 m01[4], m23[4];
        float m4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m01[e] = m23[e] = f32x2{0.f, 0.f};
            m4[e] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            const f32x2 v01 = F01[(t0 + k) * TW + c], v23 = F23[(t0 + k) * TW + c];
            const float v4 = F4[(t0 + k) * TW + c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (k - e < 0 || k - e >= RM_TAPS) continue;
                const float w = taps.w[k - e];
                m01[e] = fma2(f32x2{w, w}, v01, m01[e]);
                m23[e] = fma2(f32x2{w, w}, v23, m23[e]);
                m4[e] = fmaf(w, v4, m4[e]);
            }
        }
        const int x = x0 + c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int y = y0 + t0 + e;
            if (x < RM_HALO || x >= W - RM_HALO || y < RM_HALO || y >= H - RM_HALO) continue;
            const float mx = m01[e][0], my = m01[e][1];
            const float vx = m23[e][0] - mx * mx, vy = m23[e][1] - my * my, vxy = m4[e] - mx * my;
            const float ux = mx + 0.5f, uy = my + 0.5f;
            const float num = (2.f * ux * uy + 1e-4f) * (2.f * vxy + 9e-4f), den = (ux * ux + uy * uy + 1e-4f) * (vx + vy + 9e-4f);
            ss += (double)(num / den);
        }
    }
    // 4. the workgroup's row of the workspace: every lane's values to LDS, then wave 0 adds the four waves' in order and runs the butterflies alone
    __syncthreads();                                          // (the fields are dead: the LDS is reused)
    double* red = reinterpret_cast<double*>(lds);             // [6][256]
    float* redf = reinterpret_cast<float*>(red + 6 * 256);    // [4][256]
    const double sums[6] = {ss, sa, sb, saa, sbb, sab};
    const float ext[4] = {-amin, amax, -bmin, bmax};
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k * 256 + tid] = sums[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) redf[k * 256 + tid] = ext[k];
    __syncthreads();
    if (tid >= 64) return;
    double* out = ws + ((long long)img * gridDim.y * gridDim.x + (long long)blockIdx.y * gridDim.x + blockIdx.x) * RM_PART;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double v = wave_sum(((red[k * 256 + tid] + red[k * 256 + 64 + tid]) + red[k * 256 + 128 + tid]) + red[k * 256 + 192 + tid]);
        if (tid == 0) out[k] = v;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float v = wave_max(fmaxf(fmaxf(redf[k * 256 + tid], redf[k * 256 + 64 + tid]), fmaxf(redf[k * 256 + 128 + tid], redf[k * 256 + 192 + tid])));
        if (tid == 0) out[6 + k] = (k & 1) ? (double)v : -(double)v;
    }
}

template <int UNUSED>
__global__ __launch_bounds__(64) void pixcorr_ssim_finalize_kernel(const double* __restrict__ ws, int tiles, int H, int W, float* __restrict__ ssim,
                                                                    float* __restrict__ pixcorr) {
    const int lane = threadIdx.x, img = blockIdx.x;
    const double* rows = ws + (long long)img * tiles * RM_PART;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
    for (int t = lane; t < tiles; t += 64) {
        const double* p = rows + (long long)t * RM_PART;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += p[k];
        amin = fmin(amin, p[6]);
        amax = fmax(amax, p[7]);
        bmin = fmin(bmin, p[8]);
        bmax = fmax(bmax, p[9]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = wave_sum(s[k]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        amin = fmin(amin, __shfl_xor(amin, m, 64));
        amax = fmax(amax, __shfl_xor(amax, m, 64));
        bmin = fmin(bmin, __shfl_xor(bmin, m, 64));
        bmax = fmax(bmax, __shfl_xor(bmax, m, 64));
    }
    if (lane == 0) {
        const double n = 3.0 * H * W;
        const double cov = s[5] - s[1] * s[2] / n, va = s[3] - s[1] * s[1] / n, vb = s[4] - s[2] * s[2] / n;
        ssim[img] = (float)(s[0] / ((double)(H - 2 * RM_HALO) * (W - 2 * RM_HALO)));
        pixcorr[img] = (amin == amax || bmin == bmax) ? NAN : (float)(cov / sqrt(va * vb));
    }
}

// ---- two-way identification ----
constexpr int TW_TILE = 16;

constexpr int TW_WAVES = 16, TW_INFLIGHT = 4;

// elements k .. k + 3 of a row of D (`fill` from D on); the address never leaves the row, so the load needs no branch.  VEC: k % 4 == 0, D % 4 == 0, 16-byte rows
template <bool VEC>
__device__ __forceinline__ f32x4 tw_load4(const float* __restrict__ row, int k, int D, float fill) {
    f32x4 v;
    if (VEC) {
        v = *reinterpret_cast<const f32x4*>(row + imin(k, D - 4));
        if (k >= D) v = f32x4{fill, fill, fill, fill};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = row[imin(k + e, D - 1)];
            v[e] = k + e < D ? x : fill;
        }
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void two_way_stats_kernel(const float* __restrict__ G, const float* __restrict__ P, int D, float* __restrict__ stats, int N) {
    EEG_LDS_BASE(double, red);
    const int j = blockIdx.x, tid = threadIdx.x;
    const float *g = G + (long long)j * D, *p = P + (long long)j * D;
    double sg = 0.0, sp = 0.0;
    for (int d0 = 4 * tid; d0 < D; d0 += 1024 * TW_INFLIGHT) {
        f32x4 a[TW_INFLIGHT], b[TW_INFLIGHT];
#pragma unroll
        for (int u = 0; u < TW_INFLIGHT; ++u) {
            a[u] = tw_load4<VEC>(g, d0 + 1024 * u, D, 0.f);
            b[u] = tw_load4<VEC>(p, d0 + 1024 * u, D, 0.f);
        }
#pragma unroll
        for (int u = 0; u < TW_INFLIGHT; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sg += (double)a[u][e];
                sp += (double)b[u][e];
            }
    }
    const double mg = rm_block_sum(sg, red) / D, mp = rm_block_sum(sp, red) / D;
    double gg = 0.0, pp = 0.0, gp = 0.0;
    for (int d0 = 4 * tid; d0 < D; d0 += 1024 * TW_INFLIGHT) {
        f32x4 a[TW_INFLIGHT], b[TW_INFLIGHT];
#pragma unroll
        for (int u = 0; u < TW_INFLIGHT; ++u) {
            a[u] = tw_load4<VEC>(g, d0 + 1024 * u, D, 0.f);
            b[u] = tw_load4<VEC>(p, d0 + 1024 * u, D, 0.f);
        }
#pragma unroll
        for (int u = 0; u < TW_INFLIGHT; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (d0 + 1024 * u + e >= D) continue;
                const double x = (double)a[u][e] - mg, y = (double)b[u][e] - mp;
                gg = fma(x, x, gg);
                pp = fma(y, y, pp);
                gp = fma(x, y, gp);
            }
    }
    gg = rm_block_sum(gg, red);
    pp = rm_block_sum(pp, red);
    gp = rm_block_sum(gp, red);
    if (tid == 0) {
        stats[j] = (float)mg;
        stats[N + j] = (float)(1.0 / sqrt(gg));
        stats[2 * N + j] = (float)mp;
        stats[3 * N + j] = (float)(1.0 / sqrt(pp));
        stats[4 * N + j] = (float)(gp / sqrt(gg * pp));
    }
}

template <bool VEC>
__global__ __launch_bounds__(64 * TW_WAVES) void two_way_tile_kernel(const float* __restrict__ G, const float* __restrict__ P, int N, int D,
                                                                      const float* __restrict__ stats, int* __restrict__ part, float* __restrict__ r_out) {
    EEG_LDS_BASE(float, red);                                 // [TW_WAVES][4][64]
    const int lane = lane_id(), w = wave_uniform(wave_id()), i0 = blockIdx.y * TW_TILE, j0 = blockIdx.x * TW_TILE;
    const int ri = imin(i0 + (lane & 15), N - 1), rj = imin(j0 + (lane & 15), N - 1), kq = 4 * (lane >> 4);     // (rows past N repeat the last one; nobody reads them)
    const float *g = G + (long long)ri * D, *p = P + (long long)rj * D;
    const float mg = stats[ri], mp = stats[2 * N + rj];
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 16 * w; k0 < D; k0 += 16 * TW_WAVES * TW_INFLIGHT) {
        f32x4 a[TW_INFLIGHT], b[TW_INFLIGHT];
#pragma unroll
        for (int u = 0; u < TW_INFLIGHT; ++u) {
            a[u] = tw_load4<VEC>(g, k0 + 16 * TW_WAVES * u + kq, D, mg);
            b[u] = tw_load4<VEC>(p, k0 + 16 * TW_WAVES * u + kq, D, mp);
        }
#pragma unroll
        for (int u = 0; u < TW_INFLIGHT; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u & 1] = mfma_f32_16x16x4(a[u][e] - mg, b[u][e] - mp, acc[u & 1]);      // (0 from D on: the fill is the mean)
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[(w * 4 + e) * 64 + lane] = acc[0][e] + acc[1][e];
    __syncthreads();
    if (w != 0) return;
    const int j = j0 + (lane & 15);
    const float ip = stats[3 * N + rj], dj = stats[4 * N + rj];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = i0 + 4 * (lane >> 4) + e;
        float s = red[e * 64 + lane];
#pragma unroll
        for (int v = 1; v < TW_WAVES; ++v) s += red[(v * 4 + e) * 64 + lane];
        const float r = s * stats[N + imin(i, N - 1)] * ip;
        if (i < N && j < N) {
            if (r_out) r_out[(long long)i * N + j] = r;
            cnt += (i != j && r < dj) ? 1 : 0;
        }
    }
    cnt += __shfl_xor(cnt, 16, 64);
    cnt += __shfl_xor(cnt, 32, 64);
    if (lane < 16 && j < N) part[(long long)blockIdx.y * N + j] = cnt;
}

template <int UNUSED>
__global__ __launch_bounds__(256) void two_way_counts_kernel(const int* __restrict__ part, int row_tiles, int N, int* __restrict__ count) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    int c = 0;
    for (int t = 0; t < row_tiles; ++t) c += part[(long long)t * N + j];
    count[j] = c;
}

}  // namespace eeg

using namespace eeg;

namespace {

struct RmTile { int TH, TW, gx, gy; };

// the tile of a launch: a function of (B, H, W) alone, so the workspace query and the launcher agree
RmTile rm_tile(int B, int H, int W) {
    int TH = EEGCLIP_SSIM_TILE_H, TW = EEGCLIP_SSIM_TILE_W;
    for (;;) {
        if (TW >= 2 * W && TW > 16) TW /= 2;                  // columns nobody owns cost LDS and lanes
        else {
            const long long wgs = (long long)B * ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
            if (wgs >= RM_CUS) break;
            if (TW > 16) TW /= 2;
            else if (TH > 4) TH /= 2;
            else break;
        }
    }
    return RmTile{TH, TW, (W + TW - 1) / TW, (H + TH - 1) / TH};
}

bool rm_shape_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= RM_TAPS && W >= RM_TAPS && H <= (1 << 20) && W <= (1 << 20) && (long long)B * 3 * H * W <= (1LL << 40);
}

template <int SRC>
void rm_launch(const void* a, const void* b, int B, int H, int W, const RmTile& t, const RmTaps& taps, double* ws, void* stream) {
    size_t lds = 4u * ((size_t)2 * (t.TH + 10) * (t.TW + 12) + (size_t)5 * (t.TH + 10) * t.TW);
    if (lds < RM_RED_BYTES) lds = RM_RED_BYTES;               // (the smallest tiles: the reduction's [6][256] doubles + [4][256] floats)
    EEG_LAUNCH((pixcorr_ssim_kernel<SRC>), dim3((unsigned)t.gx, (unsigned)t.gy, (unsigned)B), dim3(256), lds, stream, a, b, H, W, t.TH, t.TW == 32 ? 5 : 4, taps,
               ws);
}

long long tw_row_tiles(int N) { return (N + TW_TILE - 1) / TW_TILE; }
bool tw_shape_ok(int N, int D) { return N >= 2 && N <= (1 << 15) && D >= 2 && (long long)N * D <= (1LL << 40); }

}  // namespace

extern "C" long long eegclip_pixcorr_ssim_workspace_bytes(int B, int H, int W) {
    if (!rm_shape_ok(B, H, W)) return EEGCLIP_EINVAL;
    const RmTile t = rm_tile(B, H, W);
    return (long long)B * t.gx * t.gy * RM_PART * (long long)sizeof(double);
}

extern "C" int eegclip_pixcorr_ssim(const void* a, const void* b, int dtype, int B, int H, int W, float* ssim, float* pixcorr, void* workspace,
                                    long long workspace_bytes, void* stream) {
    if (!a || !b || !ssim || !pixcorr || !workspace || !rm_shape_ok(B, H, W) || (dtype != EEGCLIP_DT_F32 && !half_dtype_ok(dtype))) return EEGCLIP_EINVAL;
    const RmTile t = rm_tile(B, H, W);
    if (t.gy > 65535 || (long long)t.gx * t.gy > (1 << 24) || workspace_bytes < (long long)B * t.gx * t.gy * RM_PART * (long long)sizeof(double)) return EEGCLIP_EINVAL;
    const uintptr_t mask = dtype == EEGCLIP_DT_F32 ? 3u : 1u;
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & mask) || ((reinterpret_cast<uintptr_t>(ssim) | reinterpret_cast<uintptr_t>(pixcorr)) & 3u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return EEGCLIP_EALIGN;
    RmTaps taps;
    double w[RM_TAPS], sum = 0.0;
    for (int i = 0; i < RM_TAPS; ++i) sum += w[i] = exp(-(double)((i - RM_HALO) * (i - RM_HALO)) / (2.0 * 1.5 * 1.5));
    for (int i = 0; i < RM_TAPS; ++i) taps.w[i] = (float)(w[i] / sum);
    double* ws = static_cast<double*>(workspace);
    if (dtype == EEGCLIP_DT_F32) rm_launch<2>(a, b, B, H, W, t, taps, ws, stream);
    else if (dtype == EEGCLIP_DT_F16) rm_launch<1>(a, b, B, H, W, t, taps, ws, stream);
    else rm_launch<0>(a, b, B, H, W, t, taps, ws, stream);
    EEG_LAUNCH((pixcorr_ssim_finalize_kernel<0>), dim3((unsigned)B), dim3(64), 0, stream, (const double*)ws, t.gx * t.gy, H, W, ssim, pixcorr);
    return (int)hipGetLastError();
}

extern "C" long long eegclip_two_way_workspace_bytes(int N, int D) {
    if (!tw_shape_ok(N, D)) return EEGCLIP_EINVAL;
    return 4LL * (5LL * N + tw_row_tiles(N) * N);
}

extern "C" int eegclip_two_way(const float* real, const float* recon, int N, int D, int* count, float* r, void* workspace, long long workspace_bytes,
                               void* stream) {
    if (!real || !recon || !count || !workspace || !tw_shape_ok(N, D) || workspace_bytes < 4LL * (5LL * N + tw_row_tiles(N) * N)) return EEGCLIP_EINVAL;
    if (((reinterpret_cast<uintptr_t>(real) | reinterpret_cast<uintptr_t>(recon) | reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(r) |
          reinterpret_cast<uintptr_t>(workspace)) & 3u))
        return EEGCLIP_EALIGN;
    float* stats = static_cast<float*>(workspace);
    int* part = reinterpret_cast<int*>(stats + 5LL * N);
    const int tiles = (int)tw_row_tiles(N);
    const bool vec = D % 4 == 0 && !((reinterpret_cast<uintptr_t>(real) | reinterpret_cast<uintptr_t>(recon)) & 15u);        // 16-byte loads of the rows
    const size_t red = (size_t)TW_WAVES * 4 * 64 * sizeof(float);
    if (vec) {
        EEG_LAUNCH((two_way_stats_kernel<true>), dim3((unsigned)N), dim3(256), 4 * sizeof(double), stream, real, recon, D, stats, N);
        EEG_LAUNCH((two_way_tile_kernel<true>), dim3((unsigned)tiles, (unsigned)tiles), dim3(64 * TW_WAVES), red, stream, real, recon, N, D, (const float*)stats,
                   part, r);
    } else {
        EEG_LAUNCH((two_way_stats_kernel<false>), dim3((unsigned)N), dim3(256), 4 * sizeof(double), stream, real, recon, D, stats, N);
        EEG_LAUNCH((two_way_tile_kernel<false>), dim3((unsigned)tiles, (unsigned)tiles), dim3(64 * TW_WAVES), red, stream, real, recon, N, D, (const float*)stats,
                   part, r);
    }
    EEG_LAUNCH((two_way_counts_kernel<0>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (const int*)part, tiles, N, count);
    return (int)hipGetLastError();
}
