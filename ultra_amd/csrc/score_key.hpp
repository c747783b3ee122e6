// The order key of a served score, shared by the selections that rank candidates (topk_kernels.hip, above_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace ultra {

// fp32 bits -> 32 bits whose unsigned order is the answer order of the scores: NaN (any sign, any payload) on top, then
// +inf ... +0 == -0 ... -inf.  Never 0 (-inf maps to 0x007fffff).
__device__ __forceinline__ unsigned ordered_score(unsigned u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace ultra
