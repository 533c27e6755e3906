// 16-bit attention helpers shared by csrc/cross_attn.hip and csrc/self_attn.hip: the f16 form of the 16x16x32 MFMA (the bf16 form is in
// eeg_common.h), fp32 -> 16-bit rounding, and the base-2 exponent of the softmax.
#pragma once

#include "eeg_common.h"

namespace eeg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mfma_f16_16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
#if defined(EEG_EMU)
    struct AB { bf16x8 a, b; } in{a, b};
    auto all = hipemu::wave_allgather(&in, sizeof(in));
    const int l = hipemu::cur->lane, col = l & 15, rb = (l >> 4) * 4;
    f32x4 d = c;
    for (int r = 0; r < 4; ++r) {
        float acc = c[r];
        for (int q = 0; q < 4; ++q) {
            AB ra, rbv;
            memcpy(&ra, all[(rb + r) + 16 * q], sizeof(AB));
            memcpy(&rbv, all[col + 16 * q], sizeof(AB));
            for (int e = 0; e < 8; ++e) {
                _Float16 x, y;
                short sx = ra.a[e], sy = rbv.b[e];
                memcpy(&x, &sx, 2);
                memcpy(&y, &sy, 2);
                acc += (float)x * (float)y;
            }
        }
        d[r] = acc;
    }
    return d;
#else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
#endif
}

template <bool F16>
__device__ __forceinline__ unsigned short to_h(float v) {
    if (F16) {
        _Float16 h = (_Float16)v;
        unsigned short u;
        memcpy(&u, &h, 2);
        return u;
    }
    return f32_to_bf16_bits(v);
}
// two fp32 -> one dword of two 16-bit floats (round to nearest even): one v_cvt_pk_{f16,bf16}_f32 on gfx950
template <bool F16>
__device__ __forceinline__ unsigned pack2(float a, float b) {
#if defined(EEG_EMU)
    return (unsigned)to_h<F16>(a) | ((unsigned)to_h<F16>(b) << 16);
#else
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef _Float16 h16x2_ __attribute__((ext_vector_type(2)));
    typedef __bf16 b16x2_ __attribute__((ext_vector_type(2)));
    const f32x2_ v{a, b};
    if (F16) return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h16x2_));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, b16x2_));
#endif
}
__device__ __forceinline__ float fast_exp2(float x) {
#if defined(EEG_EMU)
    return exp2f(x);
#else
    return __builtin_amdgcn_exp2f(x);        // v_exp_f32
#endif
}
template <bool F16>
__device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) {
    return F16 ? mfma_f16_16x16x32(a, b, c) : mfma_bf16_16x16x32(a, b, c);
}

}  // namespace eeg
