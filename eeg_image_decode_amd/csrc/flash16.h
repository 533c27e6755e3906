// What the two flash kernels with transposed scores (csrc/self_attn.hip, csrc/vae_attn.hip) share: lane (query fr, group g) of a wave holds the scores of
// keys 16t + 4g + r of ITS query in s[t][r], so the online softmax is per lane plus two xor-shuffles, and the rounded probabilities of two score tiles are
// one B operand of O^T = V^T P^T as they stand.  K / V staging, masking, the MFMA schedule and the online-softmax update itself stay with each kernel:
// the helpers here take their tiles BY VALUE -- a helper that takes a reference into a kernel's score or accumulator array (the softmax step over NT
// tiles, the store of DN tiles) keeps that array in memory until it is inlined and the kernels come out with another register allocation.
#pragma once

#include "half16.h"

namespace eeg {

// the probabilities of score tiles 2u (lo4) and 2u + 1 (hi4), rounded to the I/O dtype: k slots 4g + r and 16 + 4g + r of a 32-key step
template <bool F16>
__device__ __forceinline__ bf16x8 flash_pack_p(f32x4 lo4, f32x4 hi4) {
    const u32x4 pw{pack2<F16>(lo4[0], lo4[1]), pack2<F16>(lo4[2], lo4[3]), pack2<F16>(hi4[0], hi4[1]), pack2<F16>(hi4[2], hi4[3])};
    return __builtin_bit_cast(bf16x8, pw);
}

// 1 / (the row sum): a lane's l covers its own keys only, the 4 lane groups of a query are added here
__device__ __forceinline__ float flash_row_inv(float l) {
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    return 1.0f / l;
}

// one lane's piece of an O^T tile, divided by the row sum and rounded once: an 8-byte store of 4 consecutive d
template <bool F16>
__device__ __forceinline__ void flash_store4(unsigned short* op, f32x4 acc, float inv) {
    uint2 w;
    w.x = pack2<F16>(acc[0] * inv, acc[1] * inv);
    w.y = pack2<F16>(acc[2] * inv, acc[3] * inv);
    *reinterpret_cast<uint2*>(op) = w;
}

// the argument checks both entry points make.  Despite the name (the one these checks go by) it returns an error CODE, like every entry point: 0 when the
// arguments are fine, else EEGCLIP_EINVAL or EEGCLIP_EALIGN (every EINVAL condition is tested before the alignment)
static inline int flash_args_ok(const void* q, const void* k, const void* v, const void* out, int B, int Tq, int Tk, float scale, int dtype) {
    if (!q || !k || !v || !out || B < 1 || Tq < 1 || Tk < 1 || B > 65535 || !(scale > 0.f) || !(scale < INFINITY) || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) != 0) return EEGCLIP_EALIGN;
    return 0;
}

}  // namespace eeg
