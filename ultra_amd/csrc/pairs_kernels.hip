// The best k (query, id, score) records over many queries (include/ultra_nbfnet.h: ultra_topk_pairs_merge): the
// row-wise answers of one batch -- what an ultra_filtered_topk* entry wrote -- folded into the running list of a whole call.
//
//   order: score descending, then query ascending, then id ascending, every NaN above every number, -0.0 == +0.0: the stable
//   descending torch.sort of the call's row lists laid end to end in query order.
//
// The inputs are sorted lists already: the running list in (score, query, id) order, every row in (score, id) order, the rows
// ascending and every one of them a later query than any in the running list.  So among equal scores the POSITION in
// [running list ; row 0 ; row 1 ; ...] is the (query, id) order, and one 64-bit key carries everything:
// ordered_score << 32 | ~position.  Keys are distinct, a larger key is an earlier record, 0 is "absent" (an empty slot, a
// pad of a short row, a slot that is no member, a row at or beyond *n_rows -- which is never loaded).
//
// One workgroup streams the k + rows * k_row positions through select_topk, TOPK_CHUNK a trip, the survivors so far in the
// extra held slot (merge_partial_lists' loop over keys that are computed rather than loaded).
//
// IN PLACE: the running list is an input of the selection AND of the gather that follows it (a survivor's query, id and stored
// score bits come from the running list or from the batch, by position) and it is the output.  Every thread gathers its
// survivor into registers, then ONE barrier, then slots [0, m) are written, [m, k) are padded and the count is stored: nothing is
// written before every survivor has been read.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"
#include "score_key.hpp"
#include "topk_select.hpp"      // select_topk

namespace ultra {

constexpr long long PAIRS_MAX_BATCH = 65535;
// (the low word of a key holds ~position)
static_assert((PAIRS_MAX_BATCH + 1) * (long long)TOPK_MAX < (1ll << 32), "a position fits 32 bits");

// (the running list is read and written: no __restrict__ on it)
__global__ void __launch_bounds__(TOPK_THREADS) topk_pairs_merge_kernel(const int64_t *__restrict__ ids,
                                                                        const unsigned *__restrict__ scores, long long batch,
                                                                        int k_row, const int64_t *__restrict__ query_base,
                                                                        const int64_t *__restrict__ n_rows,
                                                                        const float *__restrict__ min_score, int64_t *best_query,
                                                                        int64_t *best_id, unsigned *best_score,
                                                                        int64_t *best_count, int k) {
    __shared__ u64 sorted[TOPK_MAX];
    __shared__ TopkScratch s;
    const int tid = threadIdx.x;
    long long rows = batch;
    if (n_rows) {
        const long long v = *n_rows;
        rows = v < 0 ? 0 : (v < batch ? v : batch);
    }
    const long long c = *best_count;
    const int old = (int)(c < 0 ? 0 : (c < k ? c : k));      // the records of the running list
    const bool has_floor = min_score != nullptr;
    const float low = has_floor ? *min_score : 0.0f;
    // positions [0, k): the running list's slots (present below `old`); from k on: the slots of rows [0, rows)
    const long long total = (long long)k + rows * k_row;
    int m = 0;
    for (long long pos = 0; pos < total; pos += TOPK_CHUNK) {
        u64 held[TOPK_HELD];
#pragma unroll
        for (int j = 0; j < TOPK_SLOTS; ++j) {      // (all of a thread's loads in flight at once)
            const long long i = pos + tid + j * TOPK_THREADS;
            bool present = false;
            unsigned bits = 0;
            if (i < k) {
                if (i < old) present = true, bits = best_score[i];
            } else if (i < total) {
                present = ids[i - k] >= 0;
                bits = scores[i - k];
            }
            // a strict fp32 `>`: false for a NaN
            if (has_floor) present = present && __uint_as_float(bits) > low;
            held[j] = present ? ((u64)ordered_score(bits) << 32) | (u64)(~(unsigned)i) : 0;
        }
        held[TOPK_SLOTS] = tid < m ? sorted[tid] : 0;      // the survivors so far
        __syncthreads();       // (sorted[] is rewritten by the selection)
        m = select_topk(held, k, 8, s, sorted);
    }
    // the survivors' records into registers, whichever list they come from
    int64_t query = -1, id = -1;
    unsigned bits = 0xff800000u;
    if (tid < m) {
        const long long at = (long long)(~(unsigned)sorted[tid]);
        if (at < k) {
            query = best_query[at];
            id = best_id[at];
            bits = best_score[at];
        } else {
            query = *query_base + (at - k) / k_row;
            id = ids[at - k];
            bits = scores[at - k];
        }
    }
    __syncthreads();        // every survivor has been read: the running list may be overwritten
    if (tid < k) {
        best_query[tid] = query;
        best_id[tid] = id;
        best_score[tid] = bits;
    }
    if (tid == 0) *best_count = m;
}

}  // namespace ultra

extern "C" int32_t ultra_topk_pairs_merge(const int64_t *ids, const void *scores, int64_t batch, int32_t k_row,
                                          const int64_t *query_base, const int64_t *n_rows, const float *min_score,
                                          int64_t *best_query, int64_t *best_id, void *best_score, int64_t *best_count, int32_t k,
                                          void *stream) {
    if (k < 1 || k > ULTRA_TOPK_MAX || k_row < 1 || k_row > ULTRA_TOPK_MAX || batch < 0 || batch > ultra::PAIRS_MAX_BATCH) {
        ultra::set_error("ultra_topk_pairs_merge: k and k_row must lie in [1, " + std::to_string(ULTRA_TOPK_MAX) +
                         "] and batch in [0, " + std::to_string(ultra::PAIRS_MAX_BATCH) + "]");
        return ULTRA_ERR_UNSUPPORTED;       // (before any pointer is looked at)
    }
    if (!ids || !scores || !query_base || !best_query || !best_id || !best_score || !best_count) {
        ultra::set_error("ultra_topk_pairs_merge: NULL ids, scores, query_base or running list");
        return ULTRA_ERR_INVALID;
    }
    if (batch == 0) return ULTRA_OK;
    ULTRA_DEVICE_SCOPE(stream, best_count);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    hipLaunchKernelGGL(ultra::topk_pairs_merge_kernel, dim3(1), dim3(ultra::TOPK_THREADS), 0, s, ids, (const unsigned *)scores,
                       (long long)batch, (int)k_row, query_base, n_rows, min_score, best_query, best_id, (unsigned *)best_score,
                       best_count, (int)k);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("topk_pairs_merge_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}
