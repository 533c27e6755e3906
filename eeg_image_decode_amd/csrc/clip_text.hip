// The layers of SDXL's two CLIP text encoders that csrc/gemm16.hip, csrc/unet.hip (layernorm16) and csrc/self_attn.hip (the causal form) do not cover
// (Generation/custom_pipeline.py:456-492 loads them with stabilityai/sdxl-turbo, :296-316 is encode_prompt; the modules are transformers' CLIPTextModel and
// CLIPTextModelWithProjection), 16-bit in and out, fp32 arithmetic:
//   gather_rows16  out[r] = table[idx[r]] (+ add[r % add_rows]): the embedding token_embedding[ids] + position_embedding[t] (add_rows = 77) and the pooling
//                  (row b * 77 + argmax_t ids[b] of the final LayerNorm's output).  One 16-byte piece per thread; an index outside the table is clamped into
//                  it (the host module rejects such ids before the launch: the clamp keeps a stray index from being read through).
//   act16          the MLP's activation between fc1 and fc2: kind 0 = x * sigmoid(1.702 x) (transformers' quick_gelu, the first encoder), kind 1 = the exact
//                  erf GELU (the second encoder; the form geglu16 uses).  In place allowed.
#include "half16.h"

namespace eeg {

template <bool F16, bool IDX64>
__global__ __launch_bounds__(256) void gather_rows16_kernel(const unsigned short* __restrict__ table, long long table_rows, const void* __restrict__ idx,
                                                             const unsigned short* __restrict__ add, int add_rows, unsigned short* __restrict__ out, int rows,
                                                             int C) {
    const int c8 = C / 8;
    const long long total = (long long)rows * c8;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const int r = (int)(q / c8), j = 8 * (int)(q - (long long)r * c8);
        long long i = IDX64 ? static_cast<const long long*>(idx)[r] : (long long)static_cast<const int*>(idx)[r];
        i = i < 0 ? 0 : (i >= table_rows ? table_rows - 1 : i);
        u16x8 v = *reinterpret_cast<const u16x8*>(table + i * C + j);
        if (add) {
            const u16x8 p = *reinterpret_cast<const u16x8*>(add + (long long)(r % add_rows) * C + j);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = to_h<F16>(to_f32<F16>(v[e]) + to_f32<F16>(p[e]));
        }
        *reinterpret_cast<u16x8*>(out + (long long)r * C + j) = v;
    }
}

__device__ __forceinline__ float quick_gelu(float x) { return x / (1.0f + expf(-1.702f * x)); }

template <bool F16, int KIND>
__global__ __launch_bounds__(256) void act16_kernel(const unsigned short* x, long long ldx, unsigned short* y, long long ldy, int M, int D) {
    const int d8 = D / 8;
    const long long total = (long long)M * d8;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += 256LL * gridDim.x) {
        const long long m = q / d8;
        const int j = 8 * (int)(q - m * d8);
        const u16x8 v = *reinterpret_cast<const u16x8*>(x + m * ldx + j);
        u16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = to_f32<F16>(v[e]);
            o[e] = to_h<F16>(KIND == 0 ? quick_gelu(f) : gelu_erf(f));
        }
        *reinterpret_cast<u16x8*>(y + m * ldy + j) = o;
    }
}

}  // namespace eeg

using namespace eeg;

static bool ct_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" int eegclip_gather_rows16(const void* table, long long table_rows, const void* idx, int idx64, const void* add, int add_rows, void* out, int rows, int C,
                                     int dtype, void* stream) {
    if (!table || !idx || !out || table_rows < 1 || rows < 1 || C < 8 || C % 8 || (add && add_rows < 1) || (idx64 != 0 && idx64 != 1) || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if (!ct_a16(table) || !ct_a16(out) || (add && !ct_a16(add)) || (reinterpret_cast<uintptr_t>(idx) & (idx64 ? 7u : 3u))) return EEGCLIP_EALIGN;
    long long g = ((long long)rows * (C / 8) + 255) / 256;
    if (g > 16384) g = 16384;
    const unsigned short* t = static_cast<const unsigned short*>(table);
    const unsigned short* a = static_cast<const unsigned short*>(add);
    unsigned short* o = static_cast<unsigned short*>(out);
    // (the addition is the only arithmetic: without it the kernel copies bit patterns and the dtype does not matter)
    if (dtype == EEGCLIP_DT_F16) {
        if (idx64) EEG_LAUNCH((gather_rows16_kernel<true, true>), dim3((unsigned)g), dim3(256), 0, stream, t, table_rows, idx, a, add_rows, o, rows, C);
        else       EEG_LAUNCH((gather_rows16_kernel<true, false>), dim3((unsigned)g), dim3(256), 0, stream, t, table_rows, idx, a, add_rows, o, rows, C);
    } else {
        if (idx64) EEG_LAUNCH((gather_rows16_kernel<false, true>), dim3((unsigned)g), dim3(256), 0, stream, t, table_rows, idx, a, add_rows, o, rows, C);
        else       EEG_LAUNCH((gather_rows16_kernel<false, false>), dim3((unsigned)g), dim3(256), 0, stream, t, table_rows, idx, a, add_rows, o, rows, C);
    }
    return (int)hipGetLastError();
}

extern "C" int eegclip_act16(const void* x, long long ldx, void* y, long long ldy, int M, int D, int kind, int dtype, void* stream) {
    if (!x || !y || M < 1 || D < 8 || D % 8 || ldx < D || ldy < D || (kind != 0 && kind != 1) || !half_dtype_ok(dtype))
        return EEGCLIP_EINVAL;
    if (!ct_a16(x) || !ct_a16(y) || ldx % 8 || ldy % 8) return EEGCLIP_EALIGN;
    long long g = ((long long)M * (D / 8) + 255) / 256;
    if (g > 16384) g = 16384;
    const unsigned short* xs = static_cast<const unsigned short*>(x);
    unsigned short* ys = static_cast<unsigned short*>(y);
    if (dtype == EEGCLIP_DT_F16) {
        if (kind == 0) EEG_LAUNCH((act16_kernel<true, 0>), dim3((unsigned)g), dim3(256), 0, stream, xs, ldx, ys, ldy, M, D);
        else           EEG_LAUNCH((act16_kernel<true, 1>), dim3((unsigned)g), dim3(256), 0, stream, xs, ldx, ys, ldy, M, D);
    } else {
        if (kind == 0) EEG_LAUNCH((act16_kernel<false, 0>), dim3((unsigned)g), dim3(256), 0, stream, xs, ldx, ys, ldy, M, D);
        else           EEG_LAUNCH((act16_kernel<false, 1>), dim3((unsigned)g), dim3(256), 0, stream, xs, ldx, ys, ldy, M, D);
    }
    return (int)hipGetLastError();
}
