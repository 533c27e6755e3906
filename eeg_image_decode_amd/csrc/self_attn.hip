// Flash-style attention for the SDXL UNet's self-attention (attn1; call site Generation/custom_pipeline.py:365-373, the UNet call; the
// arithmetic is diffusers' AttnProcessor2_0, head_dim 64):
//
//     out[b, i, 64h .. 64h+63] = sum_j softmax_j(scale * q[b,i,h] . k[b,j,h]) v[b,j,h]          i < Tq, j < Tk
//
// A workgroup (4 waves) owns 64 * QT query rows of one (sample, head); a wave owns QT query tiles of 16 with their Q fragments in registers.
// K / V stream through LDS in tiles of 64 keys with an online softmax; no score matrix is ever written.
//   * Scores TRANSPOSED, S^T = K Q^T (v_mfma_f32_16x16x32_{f16,bf16}, as csrc/cross_attn.hip): lane (query fr, group g) holds the scores of
//     keys 16t + 4g + r of its query, the running max / sum are per lane (two xor-shuffles per tile for the max, one reduction at the end for
//     the sum), and the rounded probabilities are already the B operand of O^T = V^T P^T.
//   * V stays row-major in LDS (plain 16-byte stores from the staging registers); the V^T operand of P V comes out of ds_read_b64_tr_b16
//     (two 4-key x 16-column transposed reads per fragment), matching the k-slot permutation of the probabilities (tile pair 2u / 2u+1).
//   * K and V rows padded to 80 halfs (160 B): the ds_read_b128 K reads and the transposed V reads of a 32-lane half hit distinct banks.
//   * Register-staged double buffer: the global loads of tile t+1 are issued before tile t is computed and written to the other LDS buffer
//     after it, one barrier per tile.
// Numerics: fp32 scores; base-2 softmax, exponent (s - m) * scale * log2(e) on the raw scores (scale > 0).  Not one FMA s * c - m * c: at
// |scores| ~ 1e9 (inputs near the fp16 range) the rounding of m * c alone is thousands, and the row maximum's exponent would overflow or vanish;
// s - m is exact near the maximum and never positive.
// probabilities rounded to the I/O dtype before P V; O accumulated in fp32, divided by the fp32 row sum once and rounded once.
// Tail keys are zero-filled in LDS and masked to -inf; tail query rows are clamped on load and never stored.
// CAUSAL (CLIP's text encoders, csrc/clip_text.hip; Tq == Tk): key j reaches query i only if j <= i.  Scores of later keys are set to -inf where the
// tail mask is applied, in the tiles that cross the workgroup's diagonal only, and the key loop ends with the tile that holds the workgroup's last
// query.  Key 0 is visible to every query, so the running maximum is still finite from the first tile on; a tile that is wholly masked for one
// query (the second tile of a 128-query workgroup, for its first 64 queries) leaves that query's m, l and accumulators as they were
// (exp2(-inf) = 0, alpha = exp2(0) = 1).  The non-causal instantiations compile to the code they had without the flag.
// PREFIX-CAUSAL (GIT's caption decoder, eeg_image_decode_amd/git_caption.py: `prefix` image tokens in front of the text): the causal instantiation with a
// runtime bound, key j reaches query i iff j < max(i + 1, prefix) -- the image tokens see each other, everything after them is causal.  prefix = 0 is the
// causal form, bit for bit (the same instructions on the same operands).  A workgroup's key loop ends at max(its last query + 1, prefix) and only the
// tiles that reach past max(its first query + 1, prefix) are masked.
#include "flash16.h"

namespace eeg {

constexpr int SA_D = 64;        // head_dim
constexpr int SA_KT = 64;       // keys per LDS tile
constexpr int SA_LD = SA_D + 16;  // LDS row stride in halfs (160 B), K and V
constexpr int SA_TILE = SA_KT * SA_LD;  // halfs per K (or V) tile buffer

struct sa_args {
    const unsigned short *q, *k, *v;
    unsigned short* out;
    long long ldq, ldk, ldv, ldo;
    int Tq, Tk;
    float scale2;   // scale * log2(e)
    int prefix;     // CAUSAL only: keys < prefix are visible to every query (0: plain causal)
};

// 16-byte pieces of one 64 x 64 tile per thread (256 threads): 2 of K, 2 of V
struct sa_stage {
    uint4 k[2], v[2];
};

__device__ __forceinline__ void sa_issue(sa_stage& r, const sa_args& a, const unsigned short* kb, const unsigned short* vb, int key0) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = t + 256 * j, row = i >> 3, c8 = (i & 7) * 8, key = key0 + row;
        r.k[j] = make_uint4(0, 0, 0, 0);
        r.v[j] = make_uint4(0, 0, 0, 0);
        if (key < a.Tk) {
            r.k[j] = *reinterpret_cast<const uint4*>(kb + key * a.ldk + c8);
            r.v[j] = *reinterpret_cast<const uint4*>(vb + key * a.ldv + c8);
        }
    }
}

__device__ __forceinline__ void sa_commit(const sa_stage& r, unsigned short* Ks, unsigned short* Vs) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = t + 256 * j, row = i >> 3, c8 = (i & 7) * 8;
        *reinterpret_cast<uint4*>(Ks + row * SA_LD + c8) = r.k[j];
        *reinterpret_cast<uint4*>(Vs + row * SA_LD + c8) = r.v[j];
    }
}

template <bool F16, int QT, bool CAUSAL = false>
__global__ __launch_bounds__(256) void self_attn_kernel(const sa_args a) {
    EEG_LDS_BASE(unsigned short, lds);      // [2][K tile | V tile]
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const unsigned short* kb = a.k + (long long)b * a.Tk * a.ldk + h * SA_D;
    const unsigned short* vb = a.v + (long long)b * a.Tk * a.ldv + h * SA_D;
    int nkt = (a.Tk + SA_KT - 1) / SA_KT;
    if (CAUSAL) {                                                          // stop after the tile of the workgroup's last query (Tq == Tk)
        const int qend = (int)(blockIdx.x + 1) * (64 * QT), qlast = (qend < a.Tq ? qend : a.Tq) - 1;
        const int klast = qlast + 1 > a.prefix ? qlast : a.prefix - 1;         // the last key any query of the workgroup sees
        if (klast / SA_KT + 1 < nkt) nkt = klast / SA_KT + 1;
    }

    sa_stage st;
    sa_issue(st, a, kb, vb, 0);
    // Q as the B operand of S^T = K Q^T: lane (query fr, group g) holds Q[q][32 s + 8g .. +7]; query tile p of this wave = (p * 4 + wave)
    bf16x8 bq[QT][2];
#pragma unroll
    for (int p = 0; p < QT; ++p) {
        const int qrow = blockIdx.x * (64 * QT) + (p * 4 + wave) * 16 + fr;
        const unsigned short* qp = a.q + ((long long)b * a.Tq + (qrow < a.Tq ? qrow : a.Tq - 1)) * a.ldq + h * SA_D + 8 * g;
        bq[p][0] = *reinterpret_cast<const bf16x8*>(qp);
        bq[p][1] = *reinterpret_cast<const bf16x8*>(qp + 32);
    }
    f32x4 acc[QT][4];
    float m[QT], l[QT];
#pragma unroll
    for (int p = 0; p < QT; ++p) {
        m[p] = -INFINITY;
        l[p] = 0.f;
#pragma unroll
        for (int dn = 0; dn < 4; ++dn) acc[p][dn] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    sa_commit(st, lds, lds + SA_TILE);
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
        const unsigned short* Ks = lds + (kt & 1) * 2 * SA_TILE;
        const unsigned short* Vs = Ks + SA_TILE;
        if (kt + 1 < nkt) sa_issue(st, a, kb, vb, (kt + 1) * SA_KT);      // in flight while this tile is computed
        // scores of the 4 key tiles of 16
        f32x4 s[QT][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(Ks + (16 * t + fr) * SA_LD + 8 * g);
            const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(Ks + (16 * t + fr) * SA_LD + 32 + 8 * g);
#pragma unroll
            for (int p = 0; p < QT; ++p) s[p][t] = mma<F16>(k1, bq[p][1], mma<F16>(k0, bq[p][0], f32x4{0.f, 0.f, 0.f, 0.f}));
        }
        if ((kt + 1) * SA_KT > a.Tk) {                                     // the last tile, partial: keys >= Tk (zero rows in LDS) -> -inf
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = kt * SA_KT + 16 * t + 4 * g + r < a.Tk;
#pragma unroll
                    for (int p = 0; p < QT; ++p) s[p][t][r] = in ? s[p][t][r] : -INFINITY;
                }
        }
        const int q0 = (int)blockIdx.x * (64 * QT);
        if (CAUSAL && kt * SA_KT + SA_KT - 1 > (q0 + 1 > a.prefix ? q0 : a.prefix - 1)) {   // the tile reaches past what the workgroup's first query sees
#pragma unroll
            for (int p = 0; p < QT; ++p) {
                const int qrow = blockIdx.x * (64 * QT) + (p * 4 + wave) * 16 + fr;
                const int lim = qrow + 1 > a.prefix ? qrow + 1 : a.prefix;   // keys < lim are visible
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[p][t][r] = kt * SA_KT + 16 * t + 4 * g + r < lim ? s[p][t][r] : -INFINITY;
            }
        }
        bf16x8 pa[QT][2];
#pragma unroll
        for (int p = 0; p < QT; ++p) {
            float mx = m[p];
#pragma unroll
            for (int t = 0; t < 4; ++t) mx = fmaxf(fmaxf(fmaxf(s[p][t][0], s[p][t][1]), fmaxf(s[p][t][2], s[p][t][3])), mx);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                        // >= one real key per tile: finite from the first tile on
            const float alpha = fast_exp2((m[p] - mx) * a.scale2);          // 0 on the first tile (m = -inf)
            m[p] = mx;
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = fast_exp2((s[p][t][r] - mx) * a.scale2);    // <= 0 exactly, 0 at the max (see the header)
                    s[p][t][r] = e;
                    sum += e;
                }
            l[p] = fmaf(l[p], alpha, sum);                                 // this lane's keys only: reduced across the 4 groups at the end
#pragma unroll
            for (int dn = 0; dn < 4; ++dn) acc[p][dn] *= alpha;
#pragma unroll
            for (int u = 0; u < 2; ++u) pa[p][u] = flash_pack_p<F16>(s[p][2 * u], s[p][2 * u + 1]);
        }
        // P V: k-step u covers key tiles 2u, 2u+1; lane (query fr, group g) supplies keys {32u+4g+r} U {32u+16+4g+r}; the V^T fragment
        // (d = 16dn + fr, the same keys) is two transposed reads of rows 32u+4g.. / 32u+16+4g.., lane 4q+p addressing row q, columns 4p..
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int dn = 0; dn < 4; ++dn) {
                const unsigned short* vp = Vs + (32 * u + 4 * g + (fr >> 2)) * SA_LD + 16 * dn + 4 * (fr & 3);
                const s16x4 lo = lds_read_tr16(vp), hi = lds_read_tr16(vp + 16 * SA_LD);
                const bf16x8 bv = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int p = 0; p < QT; ++p) acc[p][dn] = mma<F16>(bv, pa[p][u], acc[p][dn]);   // O^T[d = 16dn + 4g + r][query fr]
            }
        if (kt + 1 < nkt) {
            unsigned short* Kn = lds + ((kt + 1) & 1) * 2 * SA_TILE;        // last read in tile kt-1, before the previous barrier
            sa_commit(st, Kn, Kn + SA_TILE);
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < QT; ++p) {
        const float inv = flash_row_inv(l[p]);
        const int qrow = blockIdx.x * (64 * QT) + (p * 4 + wave) * 16 + fr;
        if (qrow < a.Tq) {
            unsigned short* op = a.out + ((long long)b * a.Tq + qrow) * a.ldo + h * SA_D + 4 * g;
#pragma unroll
            for (int dn = 0; dn < 4; ++dn) flash_store4<F16>(op + 16 * dn, acc[p][dn], inv);
        }
    }
}

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_self_attn_supported(int head_dim, long long ldq, long long ldk, long long ldv, long long ldo) {
    if (head_dim != SA_D) return EEGCLIP_EINVAL;
    if (ldq < SA_D || ldk < SA_D || ldv < SA_D || ldo < SA_D) return EEGCLIP_EINVAL;
    if ((ldq | ldk | ldv | ldo) & 7) return EEGCLIP_EALIGN;
    return 0;
}

static int sa_forward(bool causal, int prefix, const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo, int B, int Tq,
                      int Tk, int heads, int head_dim, float scale, int dtype, void* stream) {
    int rc = eegclip_self_attn_supported(head_dim, ldq, ldk, ldv, ldo);
    if (rc) return rc;
    if (heads < 1 || heads > 65535 || (causal && (Tq != Tk || prefix < 0 || prefix > Tk))) return EEGCLIP_EINVAL;
    const long long C = (long long)heads * SA_D;
    if (ldq < C || ldk < C || ldv < C || ldo < C) return EEGCLIP_EINVAL;
    rc = flash_args_ok(q, k, v, out, B, Tq, Tk, scale, dtype);            // (0 = fine)
    if (rc) return rc;
    const sa_args a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (unsigned short*)out, ldq, ldk, ldv, ldo, Tq, Tk,
                    scale * 1.44269504088896340736f, prefix};
    const size_t lds = sizeof(unsigned short) * 4 * SA_TILE;                // 40 KB: two (K, V) tile buffers
    // 128 queries per workgroup, or 64 when that leaves fewer than two workgroups per CU (256 CUs): SDXL's 1024-token stage at one image is
    // 160 workgroups of 128
    const long long wg128 = (long long)B * heads * ((Tq + 127) / 128);
    const bool f16 = dtype == EEGCLIP_DT_F16;
    if (wg128 >= 512) {
        const dim3 grid((Tq + 127) / 128, heads, B);
        if (causal) {
            if (f16) EEG_LAUNCH((self_attn_kernel<true, 2, true>), grid, dim3(256), lds, stream, a);
            else     EEG_LAUNCH((self_attn_kernel<false, 2, true>), grid, dim3(256), lds, stream, a);
        } else {
            if (f16) EEG_LAUNCH((self_attn_kernel<true, 2>), grid, dim3(256), lds, stream, a);
            else     EEG_LAUNCH((self_attn_kernel<false, 2>), grid, dim3(256), lds, stream, a);
        }
    } else {
        const dim3 grid((Tq + 63) / 64, heads, B);
        if (causal) {
            if (f16) EEG_LAUNCH((self_attn_kernel<true, 1, true>), grid, dim3(256), lds, stream, a);
            else     EEG_LAUNCH((self_attn_kernel<false, 1, true>), grid, dim3(256), lds, stream, a);
        } else {
            if (f16) EEG_LAUNCH((self_attn_kernel<true, 1>), grid, dim3(256), lds, stream, a);
            else     EEG_LAUNCH((self_attn_kernel<false, 1>), grid, dim3(256), lds, stream, a);
        }
    }
    return (int)hipGetLastError();
}

extern "C" int eegclip_self_attn_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo,
                                     int B, int Tq, int Tk, int heads, int head_dim, float scale, int dtype, void* stream) {
    return sa_forward(false, 0, q, ldq, k, ldk, v, ldv, out, ldo, B, Tq, Tk, heads, head_dim, scale, dtype, stream);
}

extern "C" int eegclip_self_attn_causal_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo,
                                            int B, int Tq, int Tk, int heads, int head_dim, float scale, int dtype, void* stream) {
    return sa_forward(true, 0, q, ldq, k, ldk, v, ldv, out, ldo, B, Tq, Tk, heads, head_dim, scale, dtype, stream);
}

extern "C" int eegclip_self_attn_prefix_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo,
                                            int B, int T, int prefix, int heads, int head_dim, float scale, int dtype, void* stream) {
    return sa_forward(true, prefix, q, ldq, k, ldk, v, ldv, out, ldo, B, T, T, heads, head_dim, scale, dtype, stream);
}
