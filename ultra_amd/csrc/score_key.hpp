// The order key of a served score, shared by the selections that rank candidates (topk_kernels.hip, above_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ultra {

// fp32 bits -> 32 bits whose unsigned order is the answer order of the scores: NaN (any sign, any payload) on top, then
// +inf ... +0 == -0 ... -inf.  Never 0 (-inf maps to 0x007fffff).
__device__ __forceinline__ unsigned ordered_score(unsigned u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// RETIRED ids (the ultra_filtered_*_alive entries): bit v & 31 of word v >> 5 of a device bitmap says that id v
// is absent from every selection.  NULL: no id is (the parents and the _live twins).  The callers ask only for ids below the
// live count, which the bitmap covers.
__device__ __forceinline__ bool is_retired(const uint32_t *__restrict__ retired_bits, long long v) {
    return retired_bits && ((retired_bits[v >> 5] >> (unsigned)(v & 31)) & 1u) != 0u;
}

// The mask words of a thread's SLOTS candidates of the chunk [lo, lo + n), candidate j being tid + j * THREADS: words[j] holds
// the candidate's bit at tid & 31 (lo and THREADS are multiples of 32); 0 where nothing is retired or the candidate lies beyond
// n.  The callers load them BEFORE the scores and look at them (slot_retired) AFTER, so that the mask words and the scores are
// in flight together -- a bit looked at inside this branch would be waited for before the first score load is issued, a second
// memory round trip.
template <int SLOTS, int THREADS>
__device__ __forceinline__ void retired_slots(const uint32_t *__restrict__ retired_bits, long long lo, int n,
                                              unsigned (&words)[SLOTS]) {
    static_assert(THREADS % 32 == 0, "a thread's candidates share their bit position");
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) words[j] = 0u;
    if (retired_bits) {     // (the same in every thread)
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int i = (int)threadIdx.x + j * THREADS;
            if (i < n) words[j] = retired_bits[(lo + i) >> 5];
        }
    }
}

__device__ __forceinline__ bool slot_retired(unsigned word) { return ((word >> (threadIdx.x & 31u)) & 1u) != 0u; }

// The number of retired ids below the live count, as the counts take it: *n_retired clamped to [0, live]; NULL: 0.  Never an
// index.
__device__ __forceinline__ long long retired_count(const int64_t *__restrict__ n_retired, long long live) {
    if (!n_retired) return 0;
    const long long v = *n_retired;
    return v < 0 ? 0 : (v < live ? v : live);
}

}  // namespace ultra
