// Flash-style attention for the SDXL VAE's mid-block attention (Generation/custom_pipeline.py:421 `vae.decode`, custom_pipeline_low_level.py:8-31
// `vae.encode`; the arithmetic is diffusers' Attention with ONE head over the H W positions, head_dim = C = 512 in SDXL's VAE):
//
//     out[b, i, :] = sum_j softmax_j(scale * q[b,i] . k[b,j]) v[b,j]          i, j < T,  head_dim D = 128 NC, NC = 1 .. 4
//
// csrc/self_attn.hip with a wide head: the same transposed scores, online softmax, row-major V read through ds_read_b64_tr_b16 and register-staged
// double buffer (flash_stage, csrc/flash16.h); what changes is the budget.  16 queries x 512 columns of fp32 O are 128 registers per lane, which with the Q fragments (64) and the
// staging registers of a K / V tile leaves one wave per SIMD, the accumulators in the AGPR half of the file and every rescale of O a round trip
// through the vector registers.  So the head is SPLIT IN TWO across waves: a workgroup of 8 waves (two per SIMD, 256 registers each, all of them
// plain VGPRs) owns 64 query rows of one image; wave (query tile qt = wave & 3, half h = wave >> 2) holds columns [h D/2, (h+1) D/2) of its 16
// queries -- Q fragments D / 64 x 4 registers, O^T accumulators D / 32 tiles of 16 x 16 (64 registers at D = 512).
//   * K / V stream through LDS in tiles of 32 keys: two (K, V) buffers of 32 x (D + 16) halfs are 132 KB of the 160 KB at D = 512 (64-key tiles
//     would only fit single-buffered); the staging registers of the tile in flight are D / 16 per lane.
//   * Scores TRANSPOSED, S^T = K Q^T: a wave multiplies its half of the columns, the two halves of a query tile meet in LDS (16 KB of fp32, one
//     extra barrier per tile) and BOTH waves add them (a + b = b + a exactly, so the two run the same softmax on the same numbers).  Lane
//     (query fr, group g) then holds the scores of keys 16t + 4g + r (t = 0, 1) of its query; running max / sum per lane; the rounded
//     probabilities are the B operand of O^T = V^T P^T as they stand (one k-step of 32 keys per tile).  A wave's k-steps go in pairs into four
//     accumulators (tile t, even / odd step): four independent MFMA chains.
//   * K and V fragments are read one group of 4 ahead of the MFMAs that use them and the scheduler is held to that order (left alone it hoists
//     every read of the tile and spills).
//   * Rows padded to D + 16 halfs: D / 8 + 2 sixteen-byte slots, = 2 mod 16, puts the 16 lanes of a ds_read_b128 group (K rows fr, slot g) on 16
//     distinct slots, and D / 2 + 8 dwords, = 8 mod 64, puts the 8 rows x 32 bytes of a transposed V read's 32-lane half on distinct banks.
//   * The 8 waves together read the K and the V tile four times (256 KB per tile at D = 512 against 256 B / clk / CU): about as long as a SIMD's
//     64 MFMAs of the tile, so the kernel is bound by the LDS near half the matrix rate (DESIGN.md section 4 has the measurement).
// Numerics as csrc/self_attn.hip: fp32 scores; base-2 softmax on (s - m) * scale * log2(e) (scale > 0), never s * c - m * c; probabilities rounded
// to the I/O dtype before P V; O in fp32, divided by the fp32 row sum once and rounded once.  Tail keys are zero-filled in LDS and masked to -inf
// (every tile holds at least one real key, so the running maximum is finite from the first tile on); tail query rows are clamped on load and
// never stored.  No score buffer exists outside the registers and those 16 KB of LDS.
#include "flash16.h"

namespace eeg {

constexpr int VA_KT = 32;        // keys per LDS tile
constexpr int VA_PAD = 16;       // halfs added to every LDS row (see the header)
constexpr int VA_XCH = 8 * 2 * 64 * 16;   // bytes of the score exchange: [wave][key tile of 16][lane] f32x4

struct va_args {
    const unsigned short *q, *k, *v;
    unsigned short* out;
    long long ldq, ldk, ldv, ldo;
    int T;
    float scale2;   // scale * log2(e)
};

template <bool F16, int NC>
__global__ __launch_bounds__(512) void vae_attn_kernel(const va_args a) {
    constexpr int D = 128 * NC, DH = D / 2, LD = D + VA_PAD, TILE = VA_KT * LD;      // TILE: halfs per K (or V) tile buffer
    constexpr int DN = DH / 16;                                                       // 16-column tiles of this wave's half of O: 4 NC
    EEG_LDS_BASE(unsigned short, lds);      // [2][K tile | V tile], then the score exchange
    f32x4* xch = reinterpret_cast<f32x4*>(lds + 4 * TILE);
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, g = lane >> 4, qt = wave & 3, h = wave >> 2;
    const unsigned short* kb = a.k + (long long)b * a.T * a.ldk;
    const unsigned short* vb = a.v + (long long)b * a.T * a.ldv;
    const int nkt = (a.T - 1) / VA_KT + 1;

    flash_stage<512, VA_KT, D, LD> st;       // NC pieces of K and of V per thread
    st.issue(kb, a.ldk, vb, a.ldv, 0, a.T);
    // Q as the B operand of S^T = K Q^T: lane (query fr, group g) holds Q[q][DH h + 32 s + 8g .. +7], s < 2 NC
    const int qrow = blockIdx.x * 64 + qt * 16 + fr;
    bf16x8 bq[2 * NC];
    {
        const unsigned short* qp = a.q + ((long long)b * a.T + (qrow < a.T ? qrow : a.T - 1)) * a.ldq + DH * h + 8 * g;
#pragma unroll
        for (int s = 0; s < 2 * NC; ++s) bq[s] = *reinterpret_cast<const bf16x8*>(qp + 32 * s);
    }
    f32x4 acc[DN];
#pragma unroll
    for (int dn = 0; dn < DN; ++dn) acc[dn] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    st.commit(lds, lds + TILE);
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
        const unsigned short* Ks = lds + (kt & 1) * 2 * TILE;
        const unsigned short* Vs = Ks + TILE;
        if (kt + 1 < nkt) st.issue(kb, a.ldk, vb, a.ldv, (kt + 1) * VA_KT, a.T);   // in flight while this tile is computed
        // this wave's half of the scores of the 2 key tiles of 16: fragment i of group p is (tile t = i & 1, k-step 2p + (i >> 1)), so that
        // consecutive MFMAs go round the four accumulators sc[t][step & 1]; the reads of group p + 1 are issued ahead of the MFMAs of group p
        f32x4 sc[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) sc[t][0] = sc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const unsigned short* kp = Ks + fr * LD + DH * h + 8 * g;
            bf16x8 kf[2][4];
            auto read_k = [&](int p, int set) {
#pragma unroll
                for (int i = 0; i < 4; ++i) kf[set][i] = *reinterpret_cast<const bf16x8*>(kp + (i & 1) * 16 * LD + 32 * (2 * p + (i >> 1)));
            };
            read_k(0, 0);
#pragma unroll
            for (int p = 0; p < NC; ++p) {
                if (p + 1 < NC) read_k(p + 1, (p + 1) & 1);
                sched_fence();
#pragma unroll
                for (int i = 0; i < 4; ++i) sc[i & 1][i >> 1] = mma<F16>(kf[p & 1][i], bq[2 * p + (i >> 1)], sc[i & 1][i >> 1]);
                sched_fence();
            }
        }
        // the two halves of a query tile meet: [wave][t][lane]
        f32x4 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            s[t] = sc[t][0] + sc[t][1];
            xch[(wave * 2 + t) * 64 + lane] = s[t];
        }
        __syncthreads();
        // P V is one k-step of 32 keys: lane (query fr, group g) supplies keys {4g + r} U {16 + 4g + r}; the V^T fragment (d = DH h + 16dn + fr,
        // the same keys) is two transposed reads of rows 4g.. / 16 + 4g.., lane 4q+p addressing row q, columns 4p..  Fragments in groups of 4
        // column tiles, read one group ahead like the K fragments; the first group's reads are in flight under the softmax.
        const unsigned short* vp = Vs + (4 * g + (fr >> 2)) * LD + DH * h + 4 * (fr & 3);
        bf16x8 fv[2][4];
        auto read_v = [&](int grp, int set) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const s16x4 lo = lds_read_tr16(vp + 16 * (4 * grp + i)), hi = lds_read_tr16(vp + 16 * (4 * grp + i) + 16 * LD);
                fv[set][i] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
        };
#pragma unroll
        for (int t = 0; t < 2; ++t) s[t] += xch[((wave ^ 4) * 2 + t) * 64 + lane];
        read_v(0, 0);
        if (a.T - kt * VA_KT < VA_KT) {                                    // the last tile, partial: keys >= T (zero rows in LDS) -> -inf
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[t][r] = kt * VA_KT + 16 * t + 4 * g + r < a.T ? s[t][r] : -INFINITY;
        }
        float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])), fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
        mx = fmaxf(mx, m);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                            // >= one real key per tile: finite from the first tile on
        const float alpha = fast_exp2((m - mx) * a.scale2);                // 0 on the first tile (m = -inf)
        m = mx;
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = fast_exp2((s[t][r] - mx) * a.scale2);       // <= 0 exactly, 0 at the max (see the header)
                s[t][r] = e;
                sum += e;
            }
        l = fmaf(l, alpha, sum);                                           // this lane's keys only: reduced across the 4 groups at the end
#pragma unroll
        for (int dn = 0; dn < DN; ++dn) acc[dn] *= alpha;
        const bf16x8 pa = flash_pack_p<F16>(s[0], s[1]);
#pragma unroll
        for (int grp = 0; grp < NC; ++grp) {
            if (grp + 1 < NC) read_v(grp + 1, (grp + 1) & 1);
            sched_fence();
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[4 * grp + i] = mma<F16>(fv[grp & 1][i], pa, acc[4 * grp + i]);   // O^T[d = DH h + 16dn + 4g + r][query fr]
            sched_fence();
        }
        if (kt + 1 < nkt) {
            unsigned short* Kn = lds + ((kt + 1) & 1) * 2 * TILE;           // last read in tile kt-1, before the previous barrier
            st.commit(Kn, Kn + TILE);
        }
        __syncthreads();                                                   // (also: the exchange is read before it is written again)
    }
    const float inv = flash_row_inv(l);
    if (qrow < a.T) {
        unsigned short* op = a.out + ((long long)b * a.T + qrow) * a.ldo + DH * h + 4 * g;
#pragma unroll
        for (int dn = 0; dn < DN; ++dn) flash_store4<F16>(op + 16 * dn, acc[dn], inv);
    }
}

template <bool F16, int NC>
static int va_launch(const va_args& a, int B, void* stream) {
    constexpr size_t lds = sizeof(unsigned short) * 4 * VA_KT * (128 * NC + VA_PAD) + VA_XCH;       // 52 .. 148 KB
#if !defined(EEG_EMU)
    if (lds > 64 * 1024) {                                                 // more dynamic LDS than the default limit of a launch
        const hipError_t e = hipFuncSetAttribute((const void*)vae_attn_kernel<F16, NC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
#endif
    const dim3 grid((unsigned)((a.T - 1) / 64 + 1), (unsigned)B);
    EEG_LAUNCH((vae_attn_kernel<F16, NC>), grid, dim3(512), lds, stream, a);
    return (int)hipGetLastError();
}

}  // namespace eeg

using namespace eeg;

extern "C" int eegclip_vae_attn_supported(int head_dim, long long ldq, long long ldk, long long ldv, long long ldo) {
    if (head_dim < 128 || head_dim > 512 || head_dim % 128) return EEGCLIP_EINVAL;
    if (ldq < head_dim || ldk < head_dim || ldv < head_dim || ldo < head_dim) return EEGCLIP_EINVAL;
    if ((ldq | ldk | ldv | ldo) & 7) return EEGCLIP_EALIGN;
    return 0;
}

extern "C" int eegclip_vae_attn_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv, void* out, long long ldo, int B,
                                    int T, int head_dim, float scale, int dtype, void* stream) {
    int rc = eegclip_vae_attn_supported(head_dim, ldq, ldk, ldv, ldo);
    if (rc) return rc;
    if (T > 0x7fffff00) return EEGCLIP_EINVAL;
    rc = flash_args_ok(q, k, v, out, B, T, T, scale, dtype);              // (0 = fine)
    if (rc) return rc;
    const va_args a{(const unsigned short*)q, (const unsigned short*)k, (const unsigned short*)v, (unsigned short*)out, ldq, ldk, ldv, ldo, T,
                    scale * 1.44269504088896340736f};
    const bool f16 = dtype == EEGCLIP_DT_F16;
    switch (head_dim / 128) {
        case 1: return f16 ? va_launch<true, 1>(a, B, stream) : va_launch<false, 1>(a, B, stream);
        case 2: return f16 ? va_launch<true, 2>(a, B, stream) : va_launch<false, 2>(a, B, stream);
        case 3: return f16 ? va_launch<true, 3>(a, B, stream) : va_launch<false, 3>(a, B, stream);
        default: return f16 ? va_launch<true, 4>(a, B, stream) : va_launch<false, 4>(a, B, stream);
    }
}
