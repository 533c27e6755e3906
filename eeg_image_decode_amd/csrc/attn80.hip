// Flash-style attention at head dim 80: CLIP ViT-H/14's image tower (1280 wide, 16 heads; the IP-Adapter's models/image_encoder, transformers'
// CLIPVisionModelWithProjection -- the encoder behind the `image_embeds` of Generation/custom_pipeline.py:365-373 and behind the data sets' cached features):
//
//     out[b, i, 80h .. 80h+79] = sum_j softmax_j(scale * q[b,i,h] . k[b,j,h]) v[b,j,h]          i < Tq, j < Tk          (no mask)
//
// The structure, the register layouts and the numerics are csrc/self_attn.hip's (read its header first): a workgroup of 4 waves owns 64 query rows of
// one (sample, head), a wave one query tile of 16, K / V stream through a register-staged double buffer in LDS in tiles of 64 keys, scores are held transposed (S^T = K Q^T), the V^T
// operand of O^T = V^T P^T comes out of ds_read_b64_tr_b16.  What 80 changes:
//   * S^T takes three k-steps of 32: columns 0..31, 32..63 and 64..95, of which 80..95 (lane groups g = 2, 3 of the third step) do not exist.  Both operands
//     are ZERO there and neither zero comes from memory: those lanes never load -- not from global memory (past column 80 of a head lies the next head, k or
//     v of a fused buffer, the next row or the end of the allocation) and not from LDS (where the next key's row starts) -- their Q and K fragments of the
//     third step are the constant 0 in registers.  0 * 0 adds nothing; a NaN that happened to lie there would.
//   * O^T has five 16-row tiles (acc[5]), ten MFMAs per key tile and query tile, and no padding.
//   * A K / V tile is 64 keys x 10 sixteen-byte pieces = 640 pieces for 256 threads: two per thread and a third for threads 0..127.
//   * LDS row stride: 80 halfs = 160 B, the row itself, no padding.  It is the stride csrc/self_attn.hip pads its 128-byte rows TO, for the same reason:
//     160 B = 10 sixteen-byte slots, and 10 r mod 16 visits the even slots once per 8 rows.  A ds_read_b128 lane group is 8 rows of lane group g and the
//     other 8 rows of g + 1 (one slot further: the odd slots), 16 distinct slots = all 64 banks once.  A 32-lane half of a transposed V read is 8 rows x 32
//     contiguous bytes at bank offsets 40 r mod 64 = {0, 40, 16, 56, 32, 8, 48, 24}: 8 disjoint runs of 8 banks.  Both conflict-free (computed with the
//     bank rule (address / 4) mod 64 of these two instructions; not measured with a counter).  With 10 pieces per 160-byte row, piece i of a tile sits at
//     byte 16 i: the commit is a linear copy.  Two (K, V) buffers of 64 x 160 B: 40 KB per workgroup, as the 64-wide kernel.
// Numerics exactly as csrc/self_attn.hip: fp32 scores; base-2 softmax on (s - m) * scale * log2(e); probabilities rounded to the I/O dtype before P V; O in
// fp32, divided by the fp32 row sum once and rounded once.  Tail keys are zero rows in LDS masked to -inf, tail queries are clamped on load, never stored.
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; fp16 and bf16 alike): 130 VGPRs + 20 AGPRs, no spills, no scratch,
// 3 waves per SIMD (a build with 128 queries per workgroup, two query tiles per wave as csrc/self_attn.hip has, was measured and lost -- see eegclip_attn80_fwd --: 190 + 40
// registers, no spills, 2 waves per SIMD; it is not in the tree).
#include "flash16.h"

namespace eeg {

constexpr int A80_D = 80;                  // head_dim
constexpr int A80_KT = 64;                 // keys per LDS tile
constexpr int A80_LD = A80_D;              // LDS row stride in halfs (160 B): see the header
constexpr int A80_TILE = A80_KT * A80_LD;  // halfs per K (or V) tile buffer
constexpr int A80_PIECES = A80_KT * A80_D / 8;   // 16-byte pieces per tile: 640

struct a80_args {
    const unsigned short *q, *k, *v;
    unsigned short* out;
    long long ldq, ldk, ldv, ldo;
    int Tq, Tk;
    float scale2;   // scale * log2(e)
};

// 16-byte pieces of one 64 x 80 tile per thread (256 threads): 2 1/2 of K, 2 1/2 of V (the third of threads 0..127 only)
struct a80_stage {
    uint4 k[3], v[3];
};

__device__ __forceinline__ void a80_issue(a80_stage& r, const a80_args& a, const unsigned short* kb, const unsigned short* vb, int key0) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = t + 256 * j, row = i / 10, c8 = (i - 10 * row) * 8, key = key0 + row;
        r.k[j] = make_uint4(0, 0, 0, 0);
        r.v[j] = make_uint4(0, 0, 0, 0);
        if (i < A80_PIECES && key < a.Tk) {
            r.k[j] = *reinterpret_cast<const uint4*>(kb + key * a.ldk + c8);
            r.v[j] = *reinterpret_cast<const uint4*>(vb + key * a.ldv + c8);
        }
    }
}

__device__ __forceinline__ void a80_commit(const a80_stage& r, unsigned short* Ks, unsigned short* Vs) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = t + 256 * j;                                        // piece i = row i / 10, columns 8 (i % 10): halfs 8 i of the tile
        if (i < A80_PIECES) {
            *reinterpret_cast<uint4*>(Ks + 8 * i) = r.k[j];
            *reinterpret_cast<uint4*>(Vs + 8 * i) = r.v[j];
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(256) void attn80_kernel(const a80_args a) {
    EEG_LDS_BASE(unsigned short, lds);      // [2][K tile | V tile]
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const unsigned short* kb = a.k + (long long)b * a.Tk * a.ldk + h * A80_D;
    const unsigned short* vb = a.v + (long long)b * a.Tk * a.ldv + h * A80_D;
    const int nkt = (a.Tk + A80_KT - 1) / A80_KT;
    const bf16x8 zero8 = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};

    a80_stage st;
    a80_issue(st, a, kb, vb, 0);
    // Q as the B operand of S^T = K Q^T: lane (query fr, group g) holds Q[q][32 s + 8g .. +7]; step 2 covers columns 64 .. 95: groups 2, 3 hold zeros.
    // A wave owns one query tile of 16: the workgroup's 64 queries (why not 128 as csrc/self_attn.hip also has: see eegclip_attn80_fwd)
    const int qrow = blockIdx.x * 64 + wave * 16 + fr;
    const unsigned short* qp = a.q + ((long long)b * a.Tq + (qrow < a.Tq ? qrow : a.Tq - 1)) * a.ldq + h * A80_D + 8 * g;
    const bf16x8 bq0 = *reinterpret_cast<const bf16x8*>(qp);
    const bf16x8 bq1 = *reinterpret_cast<const bf16x8*>(qp + 32);
    bf16x8 bq2 = zero8;
    if (g < 2) bq2 = *reinterpret_cast<const bf16x8*>(qp + 64);
    f32x4 acc[5];
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int dn = 0; dn < 5; ++dn) acc[dn] = f32x4{0.f, 0.f, 0.f, 0.f};
    a80_commit(st, lds, lds + A80_TILE);
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
        const unsigned short* Ks = lds + (kt & 1) * 2 * A80_TILE;
        const unsigned short* Vs = Ks + A80_TILE;
        if (kt + 1 < nkt) a80_issue(st, a, kb, vb, (kt + 1) * A80_KT);    // in flight while this tile is computed
        // scores of the 4 key tiles of 16
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned short* kr = Ks + (16 * t + fr) * A80_LD + 8 * g;
            const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(kr);
            const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(kr + 32);
            bf16x8 k2 = zero8;
            if (g < 2) k2 = *reinterpret_cast<const bf16x8*>(kr + 64);      // (columns 80 .. 95 would be the next key's row)
            s[t] = mma<F16>(k2, bq2, mma<F16>(k1, bq1, mma<F16>(k0, bq0, f32x4{0.f, 0.f, 0.f, 0.f})));
        }
        if ((kt + 1) * A80_KT > a.Tk) {                                    // the last tile, partial: keys >= Tk (zero rows in LDS) -> -inf
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[t][r] = kt * A80_KT + 16 * t + 4 * g + r < a.Tk ? s[t][r] : -INFINITY;
        }
        float mx = m;
#pragma unroll
        for (int t = 0; t < 4; ++t) mx = fmaxf(fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])), mx);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                            // >= one real key per tile: finite from the first tile on
        const float alpha = fast_exp2((m - mx) * a.scale2);                 // 0 on the first tile (m = -inf)
        m = mx;
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = fast_exp2((s[t][r] - mx) * a.scale2);       // <= 0 exactly, 0 at the max
                s[t][r] = e;
                sum += e;
            }
        l = fmaf(l, alpha, sum);                                           // this lane's keys only: reduced across the 4 groups at the end
#pragma unroll
        for (int dn = 0; dn < 5; ++dn) acc[dn] *= alpha;
        bf16x8 pa[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) pa[u] = flash_pack_p<F16>(s[2 * u], s[2 * u + 1]);
        // P V: k-step u covers key tiles 2u, 2u+1; the V^T fragment (d = 16dn + fr) is two transposed reads of rows 32u+4g.. / 32u+16+4g..,
        // lane 4q+p addressing row q, columns 4p.. (at most column 64 + 12 + 3 = 79)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int dn = 0; dn < 5; ++dn) {
                const unsigned short* vp = Vs + (32 * u + 4 * g + (fr >> 2)) * A80_LD + 16 * dn + 4 * (fr & 3);
                const s16x4 lo = lds_read_tr16(vp), hi = lds_read_tr16(vp + 16 * A80_LD);
                const bf16x8 bv = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                acc[dn] = mma<F16>(bv, pa[u], acc[dn]);                    // O^T[d = 16dn + 4g + r][query fr]
            }
        if (kt + 1 < nkt) {
            unsigned short* Kn = lds + ((kt + 1) & 1) * 2 * A80_TILE;       // last read in tile kt-1, before the previous barrier
            a80_commit(st, Kn, Kn + A80_TILE);
        }
        __syncthreads();
    }
    const float inv = flash_row_inv(l);
    if (qrow < a.Tq) {
        unsigned short* op = a.out + ((long long)b * a.Tq + qrow) * a.ldo + h * A80_D + 4 * g;
#pragma unroll
        for (int dn = 0; dn < 5; ++dn) flash_store4<F16>(op + 16 * dn, acc[dn], inv);    // columns 16dn + 4g .. + 3 <= 79
    }
}

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_attn80_supported(long long ldq, long long ldk, long long ldv, long long ldo) {
    if (ldq < A80_D || ldk < A80_D || ldv < A80_D || ldo < A80_D) return EEGCLIP_EINVAL;
    if ((ldq | ldk | ldv | ldo) & 7) return EEGCLIP_EALIGN;
    return 0;
}

extern "C" int eegclip_attn80_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo, int B, int Tq,
                                  int Tk, int heads, float scale, int dtype, void* stream) {
    int rc = eegclip_attn80_supported(ldq, ldk, ldv, ldo);
    if (rc) return rc;
    if (heads < 1 || heads > 65535) return EEGCLIP_EINVAL;
    const long long C = (long long)heads * A80_D;
    if (ldq < C || ldk < C || ldv < C || ldo < C) return EEGCLIP_EINVAL;
    rc = flash_args_ok(q, k, v, out, B, Tq, Tk, scale, dtype);            // (0 = fine)
    if (rc) return rc;
    const a80_args a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (unsigned short*)out, ldq, ldk, ldv, ldo, Tq, Tk,
                     scale * 1.44269504088896340736f};
    const size_t lds = sizeof(unsigned short) * 4 * A80_TILE;              // 40 KB: two (K, V) tile buffers
    // 64 queries per workgroup at every size -- not csrc/self_attn.hip's rule (128 from two workgroups per CU on).  Measured on the MI355X (profiles/clip_vision_bench.json, `query_block_ab`: a second build of this file with two query tiles per wave, not in the tree) at the
    // towers' T = 257, 16 heads, fp16 (bf16 within 2 % of it), microseconds with 64 | 128 queries per workgroup, median of 7 windows whose spread was under
    // 1 %:  B = 1: 8.8 | 12.2   B = 4: 13.1 | 14.1   B = 8: 20.3 | 19.7   B = 16: 33.5 | 33.5   B = 64: 101.8 | 100.8   B = 256: 388.9 | 420.9.
    // 128 never wins by more than 3 % and loses 38 % at one image and 8 % at 256: 257 queries are 5 blocks of 64 (320 rows, 80 % used) but 3 of 128 (384 rows,
    // 67 % used), which at this length costs what the halved K / V traffic saves, and the 128 form runs at 230 registers (2 waves per SIMD) against 150 (3).
    // A T of thousands, where the tail no longer matters, was not measured: no caller has one.
    const dim3 grid((Tq + 63) / 64, heads, B);
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((attn80_kernel<true>), grid, dim3(256), lds, stream, a);
    else                         EEG_LAUNCH((attn80_kernel<false>), grid, dim3(256), lds, stream, a);
    return (int)hipGetLastError();
}
