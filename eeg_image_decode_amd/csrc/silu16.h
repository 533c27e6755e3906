// SiLU for the 16-bit epilogues of the EfficientNet row (csrc/metric_nets.hip's eegclip_convbnact16, csrc/mbconv.hip's eegclip_dwconv16).
#pragma once

#include "half16.h"

namespace eeg {

// x sigmoid(x) in fp32 with the exponential on v_exp_f32 (the 16-bit epilogues of the EfficientNet row: one per stored element, so libm's expf would
// make memory-bound launches VALU-bound).  -x log2(e) is rounded once: the relative error of the exponential is |x| 2^-24 besides the instruction's own
// ulp, which moves x sigmoid(x) by x^2 s (1 - s) 2^-24 < 2^-24 absolutely.  x -> -inf gives x / inf = -0, x -> +inf gives x.
__device__ __forceinline__ float silu_exp2(float x) { return x / (1.0f + fast_exp2(-1.44269504f * x)); }

}  // namespace eeg
