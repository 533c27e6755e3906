// The 16-bit (fp16 / bf16 I/O) device layer, one definition each, shared by every 16-bit kernel file (gemm16, vae, unet, clip_text, caption, convt16,
// convt16_bwd, bn2d16, cross_attn, self_attn at both head dims, vae_attn): the vector types, 16-bit <-> fp32 conversion selected by the template flag F16, the f16 forms
// of the 16x16x32 and 32x32x16 MFMAs (the bf16 forms are in eeg_common.h) with their selectors, the base-2 exponent of the softmax, and the host-side
// dtype check.  The transposed LDS read (lds_read_tr16, s16x4) and sched_fence() come with eeg_common.h.
#pragma once

#include "eeg_common.h"

namespace eeg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

inline bool half_dtype_ok(int dtype) { return dtype == EEGCLIP_DT_BF16 || dtype == EEGCLIP_DT_F16; }

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

// 32x32x16 f16: the fragment layout of mfma_bf16_32x32x16 (eeg_common.h)
__device__ __forceinline__ f32x16 mfma_f16_32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
#if defined(EEG_EMU)
    struct AB { bf16x8 a, b; } in{a, b};
    auto all = hipemu::wave_allgather(&in, sizeof(in));
    const int l = hipemu::cur->lane, col = l & 31, hb = 4 * (l >> 5);
    f32x16 d = c;
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + hb;
        float acc = c[r];
        for (int h = 0; h < 2; ++h) {
            AB ra, rbv;
            memcpy(&ra, all[row + 32 * h], sizeof(AB));
            memcpy(&rbv, all[col + 32 * h], sizeof(AB));
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
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
#endif
}

template <bool F16>
__device__ __forceinline__ float to_f32(unsigned short u) {
    if (F16) {
        _Float16 h;
        memcpy(&h, &u, 2);
        return (float)h;
    }
    return bf16_bits_to_f32(u);
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
template <bool F16>
__device__ __forceinline__ f32x16 mma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return F16 ? mfma_f16_32x32x16(a, b, c) : mfma_bf16_32x32x16(a, b, c);
}

}  // namespace eeg
