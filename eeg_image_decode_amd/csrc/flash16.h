// What the flash kernels with transposed scores (csrc/self_attn.hip at head dims 64 and 80, csrc/vae_attn.hip at 128 .. 512) share: lane (query fr, group g)
// of a wave holds the scores of keys 16t + 4g + r of ITS query in s[t][r], so the online softmax is per lane plus two xor-shuffles, and the rounded
// probabilities of two score tiles are one B operand of O^T = V^T P^T as they stand.  The register staging of a K / V tile is here (flash_stage); masking,
// the MFMA schedule and the online-softmax update itself stay with each kernel:
// the helpers here take their tiles BY VALUE -- a helper that takes a reference into a kernel's score or accumulator array (the softmax step over NT
// tiles, the store of DN tiles) keeps that array in memory until it is inlined and the kernels come out with another register allocation.
#pragma once

#include "half16.h"

namespace eeg {

// One K and one V tile of KT keys x D columns on their way from global memory to LDS, in the registers of a workgroup of NTHR threads: 16-byte piece i of a
// tile is row i / (D / 8), columns 8 (i % (D / 8)), thread t holds pieces t, t + NTHR, ... (where NTHR does not divide the piece count, the last one
// exists for the first threads only).  issue() starts the global loads -- keys >= Tk are zero rows -- and commit() writes the tile to LDS rows of LD halfs;
// a kernel issues tile t + 1 before it computes tile t and commits it after (one barrier per tile).  With LD == D piece i sits at halfs 8 i of the tile.
template <int NTHR, int KT, int D, int LD>
struct flash_stage {
    static constexpr int PPR = D / 8, PIECES = KT * PPR, N = (PIECES + NTHR - 1) / NTHR;
    static constexpr bool FULL = PIECES % NTHR == 0;
    uint4 k[N], v[N];

    __device__ __forceinline__ void issue(const unsigned short* kb, long long ldk, const unsigned short* vb, long long ldv, int key0, int Tk) {
        const int t = threadIdx.x;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int i = t + NTHR * j, row = i / PPR, c8 = (i % PPR) * 8, key = key0 + row;
            k[j] = make_uint4(0, 0, 0, 0);
            v[j] = make_uint4(0, 0, 0, 0);
            if ((FULL || i < PIECES) && key < Tk) {
                k[j] = *reinterpret_cast<const uint4*>(kb + key * ldk + c8);
                v[j] = *reinterpret_cast<const uint4*>(vb + key * ldv + c8);
            }
        }
    }

    __device__ __forceinline__ void commit(unsigned short* Ks, unsigned short* Vs) const {
        const int t = threadIdx.x;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int i = t + NTHR * j, row = i / PPR, c8 = (i % PPR) * 8;
            if (FULL || i < PIECES) {
                *reinterpret_cast<uint4*>(LD == D ? Ks + 8 * i : Ks + row * LD + c8) = k[j];
                *reinterpret_cast<uint4*>(LD == D ? Vs + 8 * i : Vs + row * LD + c8) = v[j];
            }
        }
    }
};

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

// the argument checks every entry point makes.  Despite the name (the one these checks go by) it returns an error CODE, like every entry point: 0 when the
// arguments are fine, else EEGCLIP_EINVAL or EEGCLIP_EALIGN (every EINVAL condition is tested before the alignment)
static inline int flash_args_ok(const void* q, const void* k, const void* v, const void* out, int B, int Tq, int Tk, float scale, int dtype) {
    if (!q || !k || !v || !out || B < 1 || Tq < 1 || Tk < 1 || B > 65535 || !(scale > 0.f) || !(scale < INFINITY) || !half_dtype_ok(dtype)) return EEGCLIP_EINVAL;
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) != 0) return EEGCLIP_EALIGN;
    return 0;
}

}  // namespace eeg
