// The per-token kernels of the GIT caption decoder (Generation/modeling_git.py, GitForCausalLMClipEmb: Hugging Face's GitForCausalLM with the visual tokens handed
// in; a 6-layer post-LN BERT stack, hidden 768, 12 heads of 64).  Autoregressive decoding runs every GEMM at M = the batch (1 - 16) and every attention at one
// query row per sample; 16-bit in and out (fp16 / bf16), fp32 arithmetic.  The prefill's kernels are csrc/gemm16.hip, csrc/unet.hip (layernorm16),
// csrc/clip_text.hip and the prefix-causal form of csrc/self_attn.hip.
//
//   gemm16_skinny   C[m][n] = sum_k A[m][k] W[n][k] (+ bias[n]) (+ R[m][n]),  M <= 16, K % 64 == 0, any N.  A weight-streaming kernel: the work is reading W once.
//     * a workgroup owns 16 rows of W (N / 16 workgroups: 48 for N = 768, 1908 for the LM head's 30522) and its WAVES (4, 8 or 16: more where N leaves few
//       workgroups) split K in chunks of 64: wave w takes chunks w, w + WAVES, ...
//     * v_mfma_f32_16x16x32 with W as the A operand and the activations, zero-padded to 16 rows in registers, as B: D[n][m].  Lane (row fr, group g) loads
//       W[n0 + fr][64c + 16g .. +15] as two 16-byte loads straight into VGPRs (a row's 128 contiguous bytes per chunk over its 4 lanes; no LDS round trip for an
//       operand that is read once) and the matching 32 bytes of A[fr] (a few KB: cache hits); the two MFMAs of a chunk take the k-slots 16g .. 16g+7 and
//       16g+8 .. 16g+15 of both operands.  4 chunks (16 loads of 16 bytes per lane) are issued before the first MFMA.
//     * the WAVES partial 16 x 16 tiles meet in LDS and are added in wave order (bit-reproducible; no atomics, no memset, no second launch); thread (m, n)
//       adds bias and residual and stores fp32 (c_f32: the LM head's logits, read by topk_rows) or the 16-bit dtype, row stride ldc >= N (the k | v
//       projection of a new token goes straight into the cache row of each sample).  Rows of W past N are clamped on load and never stored.
//   decode_attn16   out[b, 64h ..] = sum_j softmax_j(scale q[b,h] . k[b,j,h]) v[b,j,h] over the first Tk rows of a cache (B, Tmax, [k | v]); one query row per
//     sample, every key visible.  One workgroup per (sample, head); 8 lanes hold one key row (16 bytes each), a wave takes 8 keys per step and the 4 waves
//     interleave steps.  Each 8-lane group runs its own online softmax (running max, sum, 8 accumulator columns per lane); the groups are merged with xor
//     shuffles and the waves in LDS.  Rows >= Tk are never read.  fp32 probabilities (no 16-bit rounding before P V here: there is no matrix core operand).
#include "half16.h"

namespace eeg {

struct sk_args {
    const unsigned short *A, *W, *bias, *R;
    void* C;
    long long lda, ldw, ldc, ldr;
    int M, N, K, c_f32;
};

constexpr int SK_U = 4;     // chunks of 64 k in flight per wave

template <bool F16, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void gemm16_skinny_kernel(const sk_args a) {
    EEG_LDS_BASE(float, red);                                               // [WAVES][m 16][n 16]
    const int lane = threadIdx.x & 63, wave = wave_uniform((int)(threadIdx.x >> 6));
    const int fr = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int wrow = n0 + fr < a.N ? n0 + fr : a.N - 1;                     // rows past N: clamped, never stored
    const bool mrow = fr < a.M;                                            // rows of A past M: zeros, never read
    const unsigned short* wp = a.W + (long long)wrow * a.ldw + 16 * g;
    const unsigned short* xp = a.A + (long long)(mrow ? fr : 0) * a.lda + 16 * g;
    const int nch = a.K / 64;
    const bf16x8 zero{0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc{0.f, 0.f, 0.f, 0.f};
    for (int c0 = wave; c0 < nch; c0 += WAVES * SK_U) {
        bf16x8 w[SK_U][2], x[SK_U][2];
#pragma unroll
        for (int u = 0; u < SK_U; ++u) {
            const int c = c0 + u * WAVES;
            w[u][0] = w[u][1] = x[u][0] = x[u][1] = zero;
            if (c < nch) {                                                 // (wave-uniform)
                w[u][0] = *reinterpret_cast<const bf16x8*>(wp + 64 * c);
                w[u][1] = *reinterpret_cast<const bf16x8*>(wp + 64 * c + 8);
                if (mrow) {
                    x[u][0] = *reinterpret_cast<const bf16x8*>(xp + 64 * c);
                    x[u][1] = *reinterpret_cast<const bf16x8*>(xp + 64 * c + 8);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SK_U; ++u) {                                   // (a chunk past K multiplies zeros)
            acc = mma<F16>(w[u][0], x[u][0], acc);                         // D[n = 4g + r][m = fr]
            acc = mma<F16>(w[u][1], x[u][1], acc);
        }
    }
    *reinterpret_cast<f32x4*>(red + wave * 256 + fr * 16 + 4 * g) = acc;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 256) {
        const int m = t >> 4, n = n0 + (t & 15);
        if (m < a.M && n < a.N) {
            float v = red[t];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) v += red[w * 256 + t];
            if (a.bias) v += to_f32<F16>(a.bias[n]);
            if (a.R) v += to_f32<F16>(a.R[(long long)m * a.ldr + n]);
            if (a.c_f32) static_cast<float*>(a.C)[(long long)m * a.ldc + n] = v;
            else         static_cast<unsigned short*>(a.C)[(long long)m * a.ldc + n] = to_h<F16>(v);
        }
    }
}

struct da_args {
    const unsigned short *q, *kv;
    unsigned short* out;
    long long ldq, ld_row, sample_stride, ldo;
    int Tk, heads;
    float scale2;   // scale * log2(e)
};

template <bool F16>
__global__ __launch_bounds__(256) void decode_attn16_kernel(const da_args a) {
    EEG_LDS_BASE(float, red);                                               // [4] max | [4] sum | [4][64] accumulators
    const int h = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = wave_uniform((int)(threadIdx.x >> 6));
    const int part = lane & 7, slot = lane >> 3;                            // columns 8 part .. +7 of key (step + slot)
    const long long C = (long long)a.heads * 64;
    float qf[8], acc[8];
    {
        const u16x8 qv = *reinterpret_cast<const u16x8*>(a.q + (long long)b * a.ldq + h * 64 + 8 * part);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            qf[e] = to_f32<F16>(qv[e]);
            acc[e] = 0.f;
        }
    }
    const unsigned short* kb = a.kv + (long long)b * a.sample_stride + h * 64 + 8 * part;
    float m = -INFINITY, l = 0.f;
    for (int j0 = wave * 8; j0 < a.Tk; j0 += 32) {                          // (wave-uniform trip count)
        const int j = j0 + slot;
        const bool in = j < a.Tk;
        u16x8 kk{0, 0, 0, 0, 0, 0, 0, 0}, vv{0, 0, 0, 0, 0, 0, 0, 0};
        if (in) {
            kk = *reinterpret_cast<const u16x8*>(kb + (long long)j * a.ld_row);
            vv = *reinterpret_cast<const u16x8*>(kb + (long long)j * a.ld_row + C);
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += qf[e] * to_f32<F16>(kk[e]);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (in) {
            const float mn = fmaxf(m, s);
            const float alpha = fast_exp2((m - mn) * a.scale2);             // 0 at this group's first key (m = -inf)
            const float p = fast_exp2((s - mn) * a.scale2);
            l = l * alpha + p;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = acc[e] * alpha + p * to_f32<F16>(vv[e]);
            m = mn;
        }
    }
    // the 8 key slots of the wave: a slot that saw no key has m = -inf, l = 0 and weight 0
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
        const float mo = __shfl_xor(m, off, 64), lo = __shfl_xor(l, off, 64);
        const float mn = fmaxf(m, mo);
        const float fa = m == -INFINITY ? 0.f : fast_exp2((m - mn) * a.scale2);
        const float fb = mo == -INFINITY ? 0.f : fast_exp2((mo - mn) * a.scale2);
        l = l * fa + lo * fb;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float ao = __shfl_xor(acc[e], off, 64);
            acc[e] = acc[e] * fa + ao * fb;
        }
        m = mn;
    }
    if (slot == 0) {
        if (part == 0) {
            red[wave] = m;
            red[4 + wave] = l;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[8 + wave * 64 + 8 * part + e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < 64) {                                                 // wave 0 holds key 0: the maximum is finite and the sum positive
        const int d = threadIdx.x;
        const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float sum = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float f = red[w] == -INFINITY ? 0.f : fast_exp2((red[w] - mx) * a.scale2);
            sum += red[4 + w] * f;
            o += red[8 + w * 64 + d] * f;
        }
        a.out[(long long)b * a.ldo + h * 64 + d] = to_h<F16>(o / sum);
    }
}

}  // namespace eeg

using namespace eeg;

static bool cp_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <bool F16>
static void sk_launch(const sk_args& a, void* stream) {
    // more K-splitting waves where N leaves few workgroups for 256 CUs; never more waves than chunks of 64
    const int tiles = (a.N + 15) / 16, nch = a.K / 64;
    const int waves = (tiles >= 1024 || nch <= 4) ? 4 : (tiles >= 512 || nch <= 8) ? 8 : 16;
    const dim3 grid((unsigned)tiles);
    if (waves == 4)      EEG_LAUNCH((gemm16_skinny_kernel<F16, 4>), grid, dim3(256), 4 * 1024, stream, a);
    else if (waves == 8) EEG_LAUNCH((gemm16_skinny_kernel<F16, 8>), grid, dim3(512), 8 * 1024, stream, a);
    else                 EEG_LAUNCH((gemm16_skinny_kernel<F16, 16>), grid, dim3(1024), 16 * 1024, stream, a);
}

extern "C" int eegclip_gemm16_skinny(const void* A, long long lda, const void* W, long long ldw, void* C, long long ldc, const void* bias, const void* R,
                                     long long ldr, int M, int N, int K, int c_f32, int dtype, void* stream) {
    if (!A || !W || !C || M < 1 || M > 16 || N < 1 || K < 64 || K % 64 || lda < K || ldw < K || ldc < N || (R && ldr < N) || (c_f32 != 0 && c_f32 != 1) || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if (!cp_a16(A) || !cp_a16(W) || lda % 8 || ldw % 8 || (reinterpret_cast<uintptr_t>(C) & (c_f32 ? 3u : 1u)) ||
        (bias && (reinterpret_cast<uintptr_t>(bias) & 1u)) || (R && (reinterpret_cast<uintptr_t>(R) & 1u)))
        return EEGCLIP_EALIGN;
    const sk_args a{static_cast<const unsigned short*>(A), static_cast<const unsigned short*>(W), static_cast<const unsigned short*>(bias),
                    static_cast<const unsigned short*>(R), C, lda, ldw, ldc, ldr, M, N, K, c_f32};
    if (dtype == EEGCLIP_DT_F16) sk_launch<true>(a, stream);
    else                         sk_launch<false>(a, stream);
    return (int)hipGetLastError();
}

extern "C" int eegclip_decode_attn16(const void* q, long long ldq, const void* kv, long long ld_row, long long sample_stride, void* out, long long ldo, int B, int Tk,
                                     int heads, int head_dim, float scale, int dtype, void* stream) {
    if (!q || !kv || !out || B < 1 || B > 65535 || Tk < 1 || heads < 1 || heads > 65535 || head_dim != 64 || !(scale > 0.f) || !(scale < INFINITY) || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    const long long C = (long long)heads * 64;
    if (ldq < C || ldo < C || ld_row < 2 * C || sample_stride < (long long)Tk * ld_row) return EEGCLIP_EINVAL;
    if (!cp_a16(q) || !cp_a16(kv) || !cp_a16(out) || ldq % 8 || ld_row % 8 || sample_stride % 8 || ldo % 8) return EEGCLIP_EALIGN;
    const da_args a{static_cast<const unsigned short*>(q), static_cast<const unsigned short*>(kv), static_cast<unsigned short*>(out), ldq, ld_row, sample_stride, ldo,
                    Tk, heads, scale * 1.44269504088896340736f};
    const size_t lds = sizeof(float) * (8 + 4 * 64);
    if (dtype == EEGCLIP_DT_F16) EEG_LAUNCH((decode_attn16_kernel<true>), dim3(heads, B), dim3(256), lds, stream, a);
    else                         EEG_LAUNCH((decode_attn16_kernel<false>), dim3(heads, B), dim3(256), lds, stream, a);
    return (int)hipGetLastError();
}
