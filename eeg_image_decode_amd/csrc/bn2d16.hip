// Train-mode BatchNorm2d + ReLU on the padded 16-bit NHWC frames of csrc/convt16.hip, forward and backward: the layers between the transposed convolutions of
// the reference's low-level EEG -> VAE-latent encoder while it is trained (Generation/train_vae_latent_512_low_level_no_average.py:219-260, nn.BatchNorm2d in
// train mode).  z (N, H + 2, W + 2, C) is the raw convolution output, C % 64 == 0; statistics run over the M = N H W interior pixels in fp32.
//
// Every reduction has the same fixed shape, so the same bits come out on every run: no atomics, no memset.  A workgroup of the partial kernels owns 64 channels
// and one slab of pixels; thread (channel octet, pixel group of 32) walks its pixels with 16-byte loads, the 32 groups meet in LDS and are added in group
// order -> one partial row per workgroup; the finalize kernels add the rows in slab order in fp64.
//   forward    bn2d_stats_kernel (sum z, sum z^2) -> bn2d_fwd_finalize_kernel (mean, biased variance, rstd; running_mean / running_var with momentum and the
//              UNBIASED variance, as nn.BatchNorm2d) -> bn2d_fwd_apply_kernel: a = relu((z - mean) rstd gamma + beta), one rounding, interior only.
//   backward   bn2d_bwd_partial_kernel (sum g, sum g xhat; g = da [a > 0], xhat = (z - mean) rstd) -> bn2d_bwd_finalize_kernel (dbeta, dgamma divided by
//              loss_scale; the scaled sums / M stay in the workspace) -> bn2d_bwd_apply_kernel: dz = gamma rstd (g - sum g / M - xhat sum g xhat / M).
#include "half16.h"

#include <string.h>

namespace eeg {

struct bn_args {
    const unsigned short *z, *a, *da;           // frames (a, da: backward only)
    unsigned short* out;                        // a (forward) or dz (backward)
    const float *gamma, *beta, *mean, *rstd;
    float* ws;                                  // [nslab][2][C] partial rows, then [2][C] (backward: the sums / M)
    int N, H, W, C, M, nslab, pix;              // pix = pixels per slab
};

__device__ __forceinline__ long long bn_frame_off(const bn_args& a, int p) {
    const int x = p % a.W, q = p / a.W, y = q % a.H, n_ = q / a.H;
    return (((long long)n_ * (a.H + 2) + y + 1) * (a.W + 2) + x + 1) * a.C;
}

// BWD false: v0 = z, v1 = z^2; BWD true: v0 = g, v1 = g xhat
template <bool F16, bool BWD>
__global__ __launch_bounds__(256) void bn2d_partial_kernel(const bn_args a) {
    EEG_LDS_BASE(float, red);                                               // [32 groups][2][64 channels]
    const int t = threadIdx.x, oc = t & 7, pg = t >> 3, c0 = 64 * blockIdx.x + 8 * oc, slab = blockIdx.y;
    const int p0 = slab * a.pix, p1 = p0 + a.pix < a.M ? p0 + a.pix : a.M;
    float s0[8], s1[8], mu[8], rs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s0[e] = s1[e] = 0.f;
        mu[e] = BWD ? a.mean[c0 + e] : 0.f;
        rs[e] = BWD ? a.rstd[c0 + e] : 0.f;
    }
    for (int p = p0 + pg; p < p1; p += 32) {
        const long long off = bn_frame_off(a, p) + c0;
        const bf16x8 zv = *reinterpret_cast<const bf16x8*>(a.z + off);
        if (BWD) {
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(a.a + off), dv = *reinterpret_cast<const bf16x8*>(a.da + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned short ab = (unsigned short)av[e];
                const float g = (ab & 0x7fff) && !(ab & 0x8000) ? to_f32<F16>((unsigned short)dv[e]) : 0.f;
                const float xh = (to_f32<F16>((unsigned short)zv[e]) - mu[e]) * rs[e];
                s0[e] += g;
                s1[e] += g * xh;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = to_f32<F16>((unsigned short)zv[e]);
                s0[e] += v;
                s1[e] += v * v;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        red[(pg * 2 + 0) * 64 + 8 * oc + e] = s0[e];
        red[(pg * 2 + 1) * 64 + 8 * oc + e] = s1[e];
    }
    __syncthreads();
    if (t < 128) {
        const int which = t >> 6, c = t & 63;
        float s = red[which * 64 + c];
        for (int k = 1; k < 32; ++k) s += red[(k * 2 + which) * 64 + c];
        a.ws[((long long)slab * 2 + which) * a.C + 64 * blockIdx.x + c] = s;
    }
}

__global__ __launch_bounds__(256) void bn2d_fwd_finalize_kernel(const float* __restrict__ ws, int nslab, int C, int M, float eps, float momentum, float* __restrict__ mean,
                                                                float* __restrict__ rstd, float* __restrict__ run_mean, float* __restrict__ run_var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < nslab; ++k) {
        s += (double)ws[((long long)k * 2 + 0) * C + c];
        q += (double)ws[((long long)k * 2 + 1) * C + c];
    }
    const double m = s / M;
    double var = q / M - m * m;
    if (var < 0.0) var = 0.0;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)m;
    if (run_var) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(var * ((double)M / (M - 1)));
}

__global__ __launch_bounds__(256) void bn2d_bwd_finalize_kernel(float* __restrict__ ws, int nslab, int C, int M, float inv_scale, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < nslab; ++k) {
        s += (double)ws[((long long)k * 2 + 0) * C + c];
        q += (double)ws[((long long)k * 2 + 1) * C + c];
    }
    dbeta[c] = (float)s * inv_scale;
    dgamma[c] = (float)q * inv_scale;
    float* m = ws + (long long)nslab * 2 * C;
    m[c] = (float)(s / M);
    m[C + c] = (float)(q / M);
}

// thread = 8 channels of one interior pixel
template <bool F16, bool BWD>
__global__ __launch_bounds__(256) void bn2d_apply_kernel(const bn_args a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c8 = a.C / 8;
    if (i >= (long long)a.M * c8) return;
    const int p = (int)(i / c8), c0 = 8 * (int)(i - (long long)p * c8);
    const long long off = bn_frame_off(a, p) + c0;
    const bf16x8 zv = *reinterpret_cast<const bf16x8*>(a.z + off);
    bf16x8 av{0, 0, 0, 0, 0, 0, 0, 0}, dv{0, 0, 0, 0, 0, 0, 0, 0}, o;
    if (BWD) {
        av = *reinterpret_cast<const bf16x8*>(a.a + off);
        dv = *reinterpret_cast<const bf16x8*>(a.da + off);
    }
    const float* sums = a.ws + (long long)a.nslab * 2 * a.C;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        const float xh = (to_f32<F16>((unsigned short)zv[e]) - a.mean[c]) * a.rstd[c];
        float v;
        if (BWD) {
            const unsigned short ab = (unsigned short)av[e];
            const float g = (ab & 0x7fff) && !(ab & 0x8000) ? to_f32<F16>((unsigned short)dv[e]) : 0.f;
            v = a.gamma[c] * a.rstd[c] * (g - sums[c] - xh * sums[a.C + c]);
        } else {
            v = fmaxf(xh * a.gamma[c] + a.beta[c], 0.f);
        }
        o[e] = (short)to_h<F16>(v);
    }
    *reinterpret_cast<bf16x8*>(a.out + off) = o;
}

}  // namespace eeg

using namespace eeg;

static int bn_slabs(int M, int* pix) {
    int n = (M + 31) / 32;                      // at least one pixel per group
    if (n > 256) n = 256;
    *pix = (M + n - 1) / n;
    return (M + *pix - 1) / *pix;
}

static int bn_shape(int N, int H, int W, int C, int dtype) {
    if (N < 1 || H < 1 || W < 1 || H > 32768 || W > 32768 || C < 64 || C % 64 || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    const long long M = (long long)N * H * W;
    if (M < 2 || M > 0x7fffffffLL / 16) return EEGCLIP_EINVAL;              // one value per channel has no variance (nn.BatchNorm2d raises)
    return 0;
}

extern "C" long long eegclip_bn2d16_workspace_floats(int N, int H, int W, int C) {
    if (bn_shape(N, H, W, C, EEGCLIP_DT_BF16)) return 0;
    int pix;
    return (long long)bn_slabs(N * H * W, &pix) * 2 * C + 2 * C;
}

extern "C" int eegclip_bn2d16_fwd(const eegclip_bn2d16_fwd_desc* d, void* stream) {
    if (!d || !d->z || !d->a || !d->gamma || !d->beta || !d->mean || !d->rstd || !d->workspace || !(d->eps > 0.f) || !(d->momentum >= 0.f && d->momentum <= 1.f))
        return EEGCLIP_EINVAL;
    if (const int rc = bn_shape(d->N, d->H, d->W, d->C, d->dtype)) return rc;
    if (d->workspace_floats < eegclip_bn2d16_workspace_floats(d->N, d->H, d->W, d->C)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->z) | reinterpret_cast<uintptr_t>(d->a)) & 15u) return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->gamma) | reinterpret_cast<uintptr_t>(d->beta) | reinterpret_cast<uintptr_t>(d->mean) | reinterpret_cast<uintptr_t>(d->rstd) |
         reinterpret_cast<uintptr_t>(d->running_mean) | reinterpret_cast<uintptr_t>(d->running_var) | reinterpret_cast<uintptr_t>(d->workspace)) & 3u)
        return EEGCLIP_EALIGN;
    bn_args a{static_cast<const unsigned short*>(d->z), nullptr, nullptr, static_cast<unsigned short*>(d->a), d->gamma, d->beta, d->mean, d->rstd, d->workspace,
              d->N, d->H, d->W, d->C, d->N * d->H * d->W, 0, 0};
    a.nslab = bn_slabs(a.M, &a.pix);
    const bool f16 = d->dtype == EEGCLIP_DT_F16;
    const dim3 pgrid((unsigned)(d->C / 64), (unsigned)a.nslab);
    const unsigned agrid = (unsigned)(((long long)a.M * (d->C / 8) + 255) / 256);
    if (f16) EEG_LAUNCH((bn2d_partial_kernel<true, false>), pgrid, dim3(256), 32 * 2 * 64 * sizeof(float), stream, a);
    else     EEG_LAUNCH((bn2d_partial_kernel<false, false>), pgrid, dim3(256), 32 * 2 * 64 * sizeof(float), stream, a);
    EEG_LAUNCH(bn2d_fwd_finalize_kernel, dim3((unsigned)((d->C + 255) / 256)), dim3(256), 0, stream, d->workspace, a.nslab, d->C, a.M, d->eps, d->momentum, d->mean, d->rstd,
               d->running_mean, d->running_var);
    if (f16) EEG_LAUNCH((bn2d_apply_kernel<true, false>), dim3(agrid), dim3(256), 0, stream, a);
    else     EEG_LAUNCH((bn2d_apply_kernel<false, false>), dim3(agrid), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int eegclip_bn2d16_bwd(const eegclip_bn2d16_bwd_desc* d, void* stream) {
    if (!d || !d->da || !d->a || !d->z || !d->gamma || !d->mean || !d->rstd || !d->dgamma || !d->dbeta || !d->dz || !d->workspace || !(d->loss_scale > 0.f))
        return EEGCLIP_EINVAL;
    if (const int rc = bn_shape(d->N, d->H, d->W, d->C, d->dtype)) return rc;
    if (d->workspace_floats < eegclip_bn2d16_workspace_floats(d->N, d->H, d->W, d->C)) return EEGCLIP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->z) | reinterpret_cast<uintptr_t>(d->a) | reinterpret_cast<uintptr_t>(d->da) | reinterpret_cast<uintptr_t>(d->dz)) & 15u)
        return EEGCLIP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(d->gamma) | reinterpret_cast<uintptr_t>(d->mean) | reinterpret_cast<uintptr_t>(d->rstd) | reinterpret_cast<uintptr_t>(d->dgamma) |
         reinterpret_cast<uintptr_t>(d->dbeta) | reinterpret_cast<uintptr_t>(d->workspace)) & 3u)
        return EEGCLIP_EALIGN;
    bn_args a{static_cast<const unsigned short*>(d->z), static_cast<const unsigned short*>(d->a), static_cast<const unsigned short*>(d->da),
              static_cast<unsigned short*>(d->dz), d->gamma, nullptr, d->mean, d->rstd, d->workspace, d->N, d->H, d->W, d->C, d->N * d->H * d->W, 0, 0};
    a.nslab = bn_slabs(a.M, &a.pix);
    const bool f16 = d->dtype == EEGCLIP_DT_F16;
    const dim3 pgrid((unsigned)(d->C / 64), (unsigned)a.nslab);
    const unsigned agrid = (unsigned)(((long long)a.M * (d->C / 8) + 255) / 256);
    if (f16) EEG_LAUNCH((bn2d_partial_kernel<true, true>), pgrid, dim3(256), 32 * 2 * 64 * sizeof(float), stream, a);
    else     EEG_LAUNCH((bn2d_partial_kernel<false, true>), pgrid, dim3(256), 32 * 2 * 64 * sizeof(float), stream, a);
    EEG_LAUNCH(bn2d_bwd_finalize_kernel, dim3((unsigned)((d->C + 255) / 256)), dim3(256), 0, stream, d->workspace, a.nslab, d->C, a.M, 1.f / d->loss_scale, d->dgamma,
               d->dbeta);
    if (f16) EEG_LAUNCH((bn2d_apply_kernel<true, true>), dim3(agrid), dim3(256), 0, stream, a);
    else     EEG_LAUNCH((bn2d_apply_kernel<false, true>), dim3(agrid), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
