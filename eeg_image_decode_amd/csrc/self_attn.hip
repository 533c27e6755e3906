// Flash-style attention at head dims 64 and 80, one kernel template.
// 64: the SDXL UNet's self-attention (attn1; call site Generation/custom_pipeline.py:365-373, the UNet call; the arithmetic is diffusers'
// AttnProcessor2_0), CLIP's text encoders (CAUSAL), GIT's caption decoder (PREFIX-CAUSAL) and GIT's ViT-L/14 image tower.
// 80: CLIP ViT-H/14's image tower (1280 wide, 16 heads; the IP-Adapter's models/image_encoder, transformers' CLIPVisionModelWithProjection -- the
// encoder behind the `image_embeds` of Generation/custom_pipeline.py:365-373 and behind the data sets' cached features); no mask.
//
//     out[b, i, D h .. D h + D - 1] = sum_j softmax_j(scale * q[b,i,h] . k[b,j,h]) v[b,j,h]          i < Tq, j < Tk
//
// A workgroup (4 waves) owns 64 * QT query rows of one (sample, head); a wave owns QT query tiles of 16 with their Q fragments in registers.
// K / V stream through LDS in tiles of 64 keys with an online softmax; no score matrix is ever written.
//   * Scores TRANSPOSED, S^T = K Q^T (v_mfma_f32_16x16x32_{f16,bf16}, as csrc/cross_attn.hip): lane (query fr, group g) holds the scores of
//     keys 16t + 4g + r of its query, the running max / sum are per lane (two xor-shuffles per tile for the max, one reduction at the end for
//     the sum), and the rounded probabilities are already the B operand of O^T = V^T P^T.
//   * V stays row-major in LDS (plain 16-byte stores from the staging registers); the V^T operand of P V comes out of ds_read_b64_tr_b16
//     (two 4-key x 16-column transposed reads per fragment), matching the k-slot permutation of the probabilities (tile pair 2u / 2u+1).
//   * K and V rows of 80 halfs (160 B) at both head dims: the 128-byte rows of head dim 64 are padded to it, at 80 it is the row itself.  160 B = 10
//     sixteen-byte slots, and 10 r mod 16 visits the even slots once per 8 rows.  A ds_read_b128 lane group is 8 rows of lane group g and the other 8
//     rows of g + 1 (one slot further: the odd slots), 16 distinct slots = all 64 banks once.  A 32-lane half of a transposed V read is 8 rows x 32
//     contiguous bytes at bank offsets 40 r mod 64 = {0, 40, 16, 56, 32, 8, 48, 24}: 8 disjoint runs of 8 banks.  Both conflict-free (computed with the
//     bank rule (address / 4) mod 64 of these two instructions; not measured with a counter).  Two (K, V) buffers of 64 x 160 B: 40 KB per workgroup.
//   * Register-staged double buffer (flash_stage, csrc/flash16.h): the global loads of tile t+1 are issued before tile t is computed and written to
//     the other LDS buffer after it, one barrier per tile.  A tile is 64 keys x D / 8 sixteen-byte pieces for 256 threads: 512 at 64, two per thread;
//     640 at 80, two per thread and a third for threads 0..127, and with 10 pieces per 160-byte row piece i sits at byte 16 i: a linear copy.
// What 80 changes, all of it compile-time geometry (KS, DN, sa_frag_exists, flash_stage):
//   * S^T takes KS = 3 k-steps of 32: columns 0..31, 32..63 and 64..95, of which 80..95 (lane groups g = 2, 3 of the third step) do not exist.  Both
//     operands are ZERO there and neither zero comes from memory: those lanes never load -- not from global memory (past column 80 of a head lies the
//     next head, k or v of a fused buffer, the next row or the end of the allocation) and not from LDS (where the next key's row starts) -- their Q
//     and K fragments of the third step are the constant 0 in registers.  0 * 0 adds nothing; a NaN that happened to lie there would.
//   * O^T has DN = 5 tiles of 16 rows, ten MFMAs per key tile and query tile.
//   * 64 queries per workgroup only (QT = 1), no causal form: see sa_forward.
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
// Resources (hipcc -O3 --offload-arch=gfx950, kernel metadata; VGPRs + AGPRs, fp16 and bf16 alike; no spills, no scratch; tests/test_flash_attn_build.py
// holds the occupancies): D = 64, QT = 2: 164 + 32, 2 waves per SIMD; QT = 1: 108 + 16, causal 112 + 16, 4 waves;
// D = 80 (QT = 1): 132 + 20, 3 waves.
#include "flash16.h"

namespace eeg {

constexpr int SA_KT = 64;       // keys per LDS tile
constexpr int SA_LD = 80;       // LDS row stride in halfs (160 B), K and V, both head dims
constexpr int SA_TILE = SA_KT * SA_LD;  // halfs per K (or V) tile buffer

struct sa_args {
    const unsigned short *q, *k, *v;
    unsigned short* out;
    long long ldq, ldk, ldv, ldo;
    int Tq, Tk;
    float scale2;   // scale * log2(e)
    int prefix;     // CAUSAL only: keys < prefix are visible to every query (0: plain causal)
};

// does lane group g hold columns 32 s + 8g .. + 7 of a head of D?  (all of them but groups 2, 3 of the third k-step at D = 80)
template <int D>
__device__ __forceinline__ bool sa_frag_exists(int s, int g) {
    return 32 * s + 32 <= D || 32 * s + 8 * g < D;
}

template <bool F16, int QT, bool CAUSAL, int D>
__global__ __launch_bounds__(256) void self_attn_kernel(const sa_args a) {
    static_assert(D == 64 || D == 80, "head dim");
    constexpr int KS = (D + 31) / 32, DN = D / 16;      // k-steps of S^T (the last one partial at 80), 16-row tiles of O^T
    EEG_LDS_BASE(unsigned short, lds);      // [2][K tile | V tile]
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const unsigned short* kb = a.k + (long long)b * a.Tk * a.ldk + h * D;
    const unsigned short* vb = a.v + (long long)b * a.Tk * a.ldv + h * D;
    int nkt = (a.Tk + SA_KT - 1) / SA_KT;
    if (CAUSAL) {                                                          // stop after the tile of the workgroup's last query (Tq == Tk)
        const int qend = (int)(blockIdx.x + 1) * (64 * QT), qlast = (qend < a.Tq ? qend : a.Tq) - 1;
        const int klast = qlast + 1 > a.prefix ? qlast : a.prefix - 1;         // the last key any query of the workgroup sees
        if (klast / SA_KT + 1 < nkt) nkt = klast / SA_KT + 1;
    }
    const bf16x8 zero8 = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};

    flash_stage<256, SA_KT, D, SA_LD> st;
    st.issue(kb, a.ldk, vb, a.ldv, 0, a.Tk);
    // Q as the B operand of S^T = K Q^T: lane (query fr, group g) holds Q[q][32 s + 8g .. +7], zeros where those columns do not exist; query tile p
    // of this wave = (p * 4 + wave)
    bf16x8 bq[QT][KS];
#pragma unroll
    for (int p = 0; p < QT; ++p) {
        const int qrow = blockIdx.x * (64 * QT) + (p * 4 + wave) * 16 + fr;
        const unsigned short* qp = a.q + ((long long)b * a.Tq + (qrow < a.Tq ? qrow : a.Tq - 1)) * a.ldq + h * D + 8 * g;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            bq[p][s] = zero8;
            if (sa_frag_exists<D>(s, g)) bq[p][s] = *reinterpret_cast<const bf16x8*>(qp + 32 * s);
        }
    }
    f32x4 acc[QT][DN];
    float m[QT], l[QT];
#pragma unroll
    for (int p = 0; p < QT; ++p) {
        m[p] = -INFINITY;
        l[p] = 0.f;
#pragma unroll
        for (int dn = 0; dn < DN; ++dn) acc[p][dn] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    st.commit(lds, lds + SA_TILE);
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
        const unsigned short* Ks = lds + (kt & 1) * 2 * SA_TILE;
        const unsigned short* Vs = Ks + SA_TILE;
        if (kt + 1 < nkt) st.issue(kb, a.ldk, vb, a.ldv, (kt + 1) * SA_KT, a.Tk);   // in flight while this tile is computed
        // scores of the 4 key tiles of 16: the k-steps in order into one accumulator
        f32x4 s[QT][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned short* kr = Ks + (16 * t + fr) * SA_LD + 8 * g;
            bf16x8 kf[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                kf[ks] = zero8;
                if (sa_frag_exists<D>(ks, g)) kf[ks] = *reinterpret_cast<const bf16x8*>(kr + 32 * ks);   // (columns 80 .. 95 would be the next key's row)
            }
#pragma unroll
            for (int p = 0; p < QT; ++p) {
                s[p][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s[p][t] = mma<F16>(kf[ks], bq[p][ks], s[p][t]);
            }
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
            for (int dn = 0; dn < DN; ++dn) acc[p][dn] *= alpha;
#pragma unroll
            for (int u = 0; u < 2; ++u) pa[p][u] = flash_pack_p<F16>(s[p][2 * u], s[p][2 * u + 1]);
        }
        // P V: k-step u covers key tiles 2u, 2u+1; lane (query fr, group g) supplies keys {32u+4g+r} U {32u+16+4g+r}; the V^T fragment
        // (d = 16dn + fr, the same keys) is two transposed reads of rows 32u+4g.. / 32u+16+4g.., lane 4q+p addressing row q, columns 4p..
        // (at most column 16 (DN - 1) + 12 + 3 = D - 1)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int dn = 0; dn < DN; ++dn) {
                const unsigned short* vp = Vs + (32 * u + 4 * g + (fr >> 2)) * SA_LD + 16 * dn + 4 * (fr & 3);
                const s16x4 lo = lds_read_tr16(vp), hi = lds_read_tr16(vp + 16 * SA_LD);
                const bf16x8 bv = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int p = 0; p < QT; ++p) acc[p][dn] = mma<F16>(bv, pa[p][u], acc[p][dn]);   // O^T[d = 16dn + 4g + r][query fr]
            }
        if (kt + 1 < nkt) {
            unsigned short* Kn = lds + ((kt + 1) & 1) * 2 * SA_TILE;        // last read in tile kt-1, before the previous barrier
            st.commit(Kn, Kn + SA_TILE);
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < QT; ++p) {
        const float inv = flash_row_inv(l[p]);
        const int qrow = blockIdx.x * (64 * QT) + (p * 4 + wave) * 16 + fr;
        if (qrow < a.Tq) {
            unsigned short* op = a.out + ((long long)b * a.Tq + qrow) * a.ldo + h * D + 4 * g;
#pragma unroll
            for (int dn = 0; dn < DN; ++dn) flash_store4<F16>(op + 16 * dn, acc[p][dn], inv);   // columns 16dn + 4g .. + 3 <= D - 1
        }
    }
}

// 64 * QT queries per workgroup
template <int QT, bool CAUSAL, int D>
static int sa_launch(const sa_args& a, int B, int heads, bool f16, void* stream) {
    const size_t lds = sizeof(unsigned short) * 4 * SA_TILE;                // 40 KB: two (K, V) tile buffers
    const dim3 grid((a.Tq + 64 * QT - 1) / (64 * QT), heads, B);
    if (f16) EEG_LAUNCH((self_attn_kernel<true, QT, CAUSAL, D>), grid, dim3(256), lds, stream, a);
    else     EEG_LAUNCH((self_attn_kernel<false, QT, CAUSAL, D>), grid, dim3(256), lds, stream, a);
    return (int)hipGetLastError();
}

template <int D>
static int sa_strides_ok(long long ldq, long long ldk, long long ldv, long long ldo) {
    if (ldq < D || ldk < D || ldv < D || ldo < D) return EEGCLIP_EINVAL;
    if ((ldq | ldk | ldv | ldo) & 7) return EEGCLIP_EALIGN;
    return 0;
}

template <int D>
static int sa_forward(bool causal, int prefix, const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo, int B, int Tq,
                      int Tk, int heads, float scale, int dtype, void* stream) {
    int rc = sa_strides_ok<D>(ldq, ldk, ldv, ldo);
    if (rc) return rc;
    if (heads < 1 || heads > 65535 || (causal && (Tq != Tk || prefix < 0 || prefix > Tk))) return EEGCLIP_EINVAL;
    const long long C = (long long)heads * D;
    if (ldq < C || ldk < C || ldv < C || ldo < C) return EEGCLIP_EINVAL;
    rc = flash_args_ok(q, k, v, out, B, Tq, Tk, scale, dtype);            // (0 = fine)
    if (rc) return rc;
    const sa_args a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (unsigned short*)out, ldq, ldk, ldv, ldo, Tq, Tk,
                    scale * 1.44269504088896340736f, prefix};
    const bool f16 = dtype == EEGCLIP_DT_F16;
    if constexpr (D == 80) {
        // 64 queries per workgroup at every size -- not the 64-wide rule below.  Measured on the MI355X (profiles/clip_vision_bench.json, `query_block_ab`: a build with two query tiles per wave at head dim 80, not in the tree) at the
        // towers' T = 257, 16 heads, fp16 (bf16 within 2 % of it), microseconds with 64 | 128 queries per workgroup, median of 7 windows whose spread was under
        // 1 %:  B = 1: 8.8 | 12.2   B = 4: 13.1 | 14.1   B = 8: 20.3 | 19.7   B = 16: 33.5 | 33.5   B = 64: 101.8 | 100.8   B = 256: 388.9 | 420.9.
        // 128 never wins by more than 3 % and loses 38 % at one image and 8 % at 256: 257 queries are 5 blocks of 64 (320 rows, 80 % used) but 3 of 128 (384 rows,
        // 67 % used), which at this length costs what the halved K / V traffic saves, and the 128 form ran at 190 + 40 registers (2 waves per SIMD) against 3 waves.
        // A T of thousands, where the tail no longer matters, was not measured: no caller has one.  Nor has a causal or prefix form a caller: none is built.
        return sa_launch<1, false, D>(a, B, heads, f16, stream);
    } else {
        // 128 queries per workgroup, or 64 when that leaves fewer than two workgroups per CU (256 CUs): SDXL's 1024-token stage at one image is
        // 160 workgroups of 128
        const bool wide = (long long)B * heads * ((Tq + 127) / 128) >= 512;
        if (wide) return causal ? sa_launch<2, true, D>(a, B, heads, f16, stream) : sa_launch<2, false, D>(a, B, heads, f16, stream);
        return causal ? sa_launch<1, true, D>(a, B, heads, f16, stream) : sa_launch<1, false, D>(a, B, heads, f16, stream);
    }
}

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_self_attn_supported(int head_dim, long long ldq, long long ldk, long long ldv, long long ldo) {
    if (head_dim != 64) return EEGCLIP_EINVAL;
    return sa_strides_ok<64>(ldq, ldk, ldv, ldo);
}

extern "C" int eegclip_self_attn_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo,
                                     int B, int Tq, int Tk, int heads, int head_dim, float scale, int dtype, void* stream) {
    if (head_dim != 64) return EEGCLIP_EINVAL;
    return sa_forward<64>(false, 0, q, ldq, k, ldk, v, ldv, out, ldo, B, Tq, Tk, heads, scale, dtype, stream);
}

extern "C" int eegclip_self_attn_causal_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo,
                                            int B, int Tq, int Tk, int heads, int head_dim, float scale, int dtype, void* stream) {
    if (head_dim != 64) return EEGCLIP_EINVAL;
    return sa_forward<64>(true, 0, q, ldq, k, ldk, v, ldv, out, ldo, B, Tq, Tk, heads, scale, dtype, stream);
}

extern "C" int eegclip_self_attn_prefix_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo,
                                            int B, int T, int prefix, int heads, int head_dim, float scale, int dtype, void* stream) {
    if (head_dim != 64) return EEGCLIP_EINVAL;
    return sa_forward<64>(true, prefix, q, ldq, k, ldk, v, ldv, out, ldo, B, T, T, heads, scale, dtype, stream);
}

// head dim 80: eegclip_self_attn_fwd's contract with C = 80 * heads, no head_dim argument
extern "C" int eegclip_attn80_supported(long long ldq, long long ldk, long long ldv, long long ldo) {
    return sa_strides_ok<80>(ldq, ldk, ldv, ldo);
}

extern "C" int eegclip_attn80_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo, int B, int Tq,
                                  int Tk, int heads, float scale, int dtype, void* stream) {
    return sa_forward<80>(false, 0, q, ldq, k, ldk, v, ldv, out, ldo, B, Tq, Tk, heads, scale, dtype, stream);
}
