// Filtered top-k answers of a batch of link-prediction queries (include/ultra_nbfnet.h: ultra_filtered_topk).
//
//   candidates of row b = ids not in known(b), ordered by score descending, equal scores by ascending id, every NaN above
//   every number (NaNs tie), -0.0 == +0.0: the stable descending torch.sort.  Exact and reproducible.
//
// One 64-bit key per candidate carries the whole order: an order-preserving map of the canonicalised score in the high word,
// ~id in the low word.  Keys of a row are distinct, a larger key is an earlier answer, and 0 is free for "absent" -- a
// filtered candidate is REMOVED (key 0), never rescored, so a genuine -inf stays a candidate.
//
// Two launches, the kernel boundary the only synchronisation between them:
//   1. topk_chunk_kernel: one workgroup per (row, chunk of ULTRA_TOPK_CHUNK candidates) loads the chunk's keys, knocks out
//      (through LDS) the slice of known(b) that falls into the chunk (binary search for its start in the sorted list), selects the k
//      largest keys (select_topk: a floor from the threads' maxima, a radix select where that leaves too many), sorts them and
//      writes at most k keys to the workspace (0-padded);
//   2. topk_merge_kernel: one workgroup per row streams the row's partial lists through the same selection, any number of them,
//      and writes ids, the STORED bits of the scores (gathered from the score matrix: -0.0 and NaN payloads survive) and the count.
// A row of one chunk is finished by the first launch alone.  LDS atomics only count (histograms, the compaction cursor); the
// survivors are sorted afterwards and their keys are distinct, so no output depends on the order atomics land in.
//
// A LIVE COUNT (ultra_filtered_topk_live): the row stride stays n_cand, the number of SLOTS, while only the ids
// below *n_live -- read on the device, clamped to [0, n_cand] -- are candidates.  A dead id is never loaded, so whatever its
// slot holds (a NaN, +inf) cannot reach a key; a chunk workgroup wholly beyond the live count still writes its empty partial
// list, so the merge reads no stale workspace.  The grid and the workspace depend on (batch, n_cand) alone.  n_live == NULL
// (ultra_filtered_topk) means n_cand: the same kernels, the same bits.
//
// RETIRED IDS (ultra_filtered_topk_alive): a device bitmap names ids below the live count that are absent.  A
// chunk starts at a multiple of TOPK_CHUNK, so its candidates' mask words are whole words; they are loaded next to the scores
// (ahead of them in program order, looked at after them: score_key.hpp) and the key of a retired candidate is zeroed before the
// knock-out and the selection -- its score is loaded but reaches no key.  count_out is taken from live - retired - known, the retired count read on the device and clamped to [0, live].
// retired_bits == NULL: the _live twin and the parent, the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"
#include "score_key.hpp"
#include "topk_select.hpp"      // select_topk, write_answers, live_count, merge_partial_lists

namespace ultra {

__global__ void __launch_bounds__(TOPK_THREADS) topk_chunk_kernel(const float *__restrict__ score, const int64_t *__restrict__ known_ptr,
                                                                  const int64_t *__restrict__ known_index, long long n_cand,
                                                                  long long n_chunk, int k, u64 *__restrict__ partial,
                                                                  int64_t *ids_out, unsigned *scores_out, int64_t *count_out,
                                                                  const int64_t *__restrict__ n_live,
                                                                  const uint32_t *__restrict__ retired_bits,
                                                                  const int64_t *__restrict__ n_retired) {
    __shared__ unsigned ord[TOPK_CHUNK];
    __shared__ u64 sorted[TOPK_MAX];
    __shared__ TopkScratch s;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / n_chunk, c = blockIdx.x % n_chunk;
    const float *row = score + b * n_cand;
    const long long lo = c * TOPK_CHUNK;
    const long long live = live_count(n_live, n_cand);
    // (a chunk beyond the live count holds no candidate: n == 0, nothing is loaded, an empty list is written)
    const int n = (int)(live - lo < TOPK_CHUNK ? (live > lo ? live - lo : 0) : TOPK_CHUNK);
    // all of a thread's scores in flight at once, its mask words ahead of them and the search for the chunk's slice of known(b)
    // beside them; a retired candidate is absent before anything looks at its key
    unsigned mask[TOPK_SLOTS];
    retired_slots<TOPK_SLOTS, TOPK_THREADS>(retired_bits, lo, n, mask);
    unsigned bits[TOPK_SLOTS];
#pragma unroll
    for (int j = 0; j < TOPK_SLOTS; ++j) {
        const int i = tid + j * TOPK_THREADS;
        bits[j] = i < n ? ordered_score(__float_as_uint(row[lo + i])) : 0u;
    }
#pragma unroll
    for (int j = 0; j < TOPK_SLOTS; ++j) bits[j] = slot_retired(mask[j]) ? 0u : bits[j];
    long long n_known = 0, a = 0, k1 = 0;
    bool any_known = false;      // (the same in every thread)
    if (known_ptr) {
        const long long k0 = known_ptr[b];
        k1 = known_ptr[b + 1];
        n_known = k1 - k0;
        long long z = k1;       // first entry >= lo
        a = k0;
        while (a < z) {
            const long long mid = a + ((z - a) >> 1);
            if (known_index[mid] < lo) a = mid + 1; else z = mid;
        }
        any_known = a < k1 && known_index[a] < lo + n;
    }
    if (any_known) {        // the knock-out goes by id: through LDS
#pragma unroll
        for (int j = 0; j < TOPK_SLOTS; ++j) {
            const int i = tid + j * TOPK_THREADS;
            if (i < n) ord[i] = bits[j];
        }
        __syncthreads();
        for (long long j = a + tid; j < k1; j += TOPK_THREADS) {
            const long long id = known_index[j];
            if (id >= lo + n) break;        // ascending: the rest of this thread's entries lie beyond the chunk too
            if (id >= lo) ord[id - lo] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TOPK_SLOTS; ++j) {
            const int i = tid + j * TOPK_THREADS;
            bits[j] = i < n ? ord[i] : 0u;
        }
    }
    // inside a chunk the local index orders the ids: 32 + TOPK_CHUNK_BITS bits of key, two radix passes fewer
    u64 held[TOPK_HELD];
#pragma unroll
    for (int j = 0; j < TOPK_SLOTS; ++j)
        held[j] = bits[j] ? ((u64)bits[j] << TOPK_CHUNK_BITS) | (u64)(TOPK_CHUNK - 1 - (tid + j * TOPK_THREADS)) : 0;
    held[TOPK_SLOTS] = 0;
    const int m = select_topk(held, k, (32 + TOPK_CHUNK_BITS + 7) / 8, s, sorted);
    if (tid < m) {
        const u64 key = sorted[tid];
        const unsigned id = (unsigned)(lo + (TOPK_CHUNK - 1 - (int)(key & (TOPK_CHUNK - 1))));
        sorted[tid] = ((key >> TOPK_CHUNK_BITS) << 32) | (u64)(~id);       // (each thread rewrites its own slot)
    }
    __syncthreads();
    if (n_chunk == 1) {
        write_answers(row, live - retired_count(n_retired, live), n_known, k, m, sorted, ids_out + b * k, scores_out + b * k,
                      count_out + b);
    } else if (tid < k) {
        partial[((long long)blockIdx.x) * k + tid] = tid < m ? sorted[tid] : 0;
    }
}

__global__ void __launch_bounds__(TOPK_THREADS) topk_merge_kernel(const float *__restrict__ score, const int64_t *__restrict__ known_ptr,
                                                                  long long n_cand, long long n_chunk, int k,
                                                                  const u64 *__restrict__ partial, int64_t *ids_out,
                                                                  unsigned *scores_out, int64_t *count_out,
                                                                  const int64_t *__restrict__ n_live,
                                                                  const int64_t *__restrict__ n_retired) {
    __shared__ u64 sorted[TOPK_MAX];
    __shared__ TopkScratch s;
    const long long b = blockIdx.x;
    const int m = merge_partial_lists(partial + b * n_chunk * k, n_chunk * k, k, s, sorted);
    const long long n_known = known_ptr ? known_ptr[b + 1] - known_ptr[b] : 0;
    const long long live = live_count(n_live, n_cand);
    write_answers(score + b * n_cand, live - retired_count(n_retired, live), n_known, k, m, sorted, ids_out + b * k,
                  scores_out + b * k, count_out + b);
}

}  // namespace ultra

extern "C" int64_t ultra_filtered_topk_workspace(int64_t batch, int64_t n_cand, int32_t k) {
    if (batch < 0 || n_cand < 0 || k < 1 || k > ULTRA_TOPK_MAX) return -1;
    const int64_t n_chunk = (n_cand + ULTRA_TOPK_CHUNK - 1) / ULTRA_TOPK_CHUNK;
    return batch * n_chunk * (int64_t)k * (int64_t)sizeof(uint64_t);
}

// The three entries: `who` names the caller in the messages; n_live == NULL: every slot is a candidate; retired_bits == NULL: no
// id is retired.
static int32_t filtered_topk_impl(const char *who_, const void *score, const int64_t *known_ptr, const int64_t *known_index,
                                  int64_t batch, int64_t n_cand, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out,
                                  void *workspace, int64_t workspace_bytes, const int64_t *n_live, const uint32_t *retired_bits,
                                  const int64_t *n_retired, void *stream) {
    const std::string who(who_);
    if (k < 1 || k > ULTRA_TOPK_MAX || n_cand >= (int64_t)1 << 31) {      // (before any pointer is looked at)
        ultra::set_error(who + ": k must lie in [1, " + std::to_string(ULTRA_TOPK_MAX) + "] and n_cand below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (!score || !ids_out || !scores_out || !count_out || batch < 0 || n_cand <= 0) {
        ultra::set_error(who + ": NULL operand or empty candidate set");
        return ULTRA_ERR_INVALID;
    }
    const int64_t n_chunk = (n_cand + ULTRA_TOPK_CHUNK - 1) / ULTRA_TOPK_CHUNK;
    const int64_t need = ultra_filtered_topk_workspace(batch, n_cand, k);
    if (workspace_bytes < need || (need > 0 && !workspace) || ((uintptr_t)workspace & 7u) != 0) {
        ultra::set_error(who + ": workspace of " + std::to_string(workspace_bytes) + " bytes, needs " +
                         std::to_string(need) + " (8-byte aligned)");
        return ULTRA_ERR_INVALID;
    }
    if (batch * n_chunk >= (int64_t)1 << 31) {
        ultra::set_error(who + ": batch * chunks per row must stay below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch == 0) return ULTRA_OK;
    ULTRA_DEVICE_SCOPE(stream, score);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    hipLaunchKernelGGL(ultra::topk_chunk_kernel, dim3((unsigned)(batch * n_chunk)), dim3(ultra::TOPK_THREADS), 0, s,
                       (const float *)score, known_ptr, known_index, (long long)n_cand, (long long)n_chunk, (int)k,
                       (ultra::u64 *)workspace, ids_out, (unsigned *)scores_out, count_out, n_live, retired_bits, n_retired);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("topk_chunk_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    if (n_chunk > 1) {
        hipLaunchKernelGGL(ultra::topk_merge_kernel, dim3((unsigned)batch), dim3(ultra::TOPK_THREADS), 0, s, (const float *)score,
                           known_ptr, (long long)n_cand, (long long)n_chunk, (int)k, (const ultra::u64 *)workspace, ids_out,
                           (unsigned *)scores_out, count_out, n_live, n_retired);
        if (hipGetLastError() != hipSuccess) {
            ultra::set_error("topk_merge_kernel launch failed");
            return ULTRA_ERR_HIP;
        }
    }
    return ULTRA_OK;
}

extern "C" int32_t ultra_filtered_topk(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                       int64_t n_cand, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out,
                                       void *workspace, int64_t workspace_bytes, void *stream) {
    return filtered_topk_impl("ultra_filtered_topk", score, known_ptr, known_index, batch, n_cand, k, ids_out, scores_out, count_out,
                              workspace, workspace_bytes, nullptr, nullptr, nullptr, stream);
}

extern "C" int32_t ultra_filtered_topk_live(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                            int64_t n_cand, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out,
                                            void *workspace, int64_t workspace_bytes, const int64_t *n_live, void *stream) {
    if (!n_live && k >= 1 && k <= ULTRA_TOPK_MAX && n_cand < (int64_t)1 << 31) {      // (the parent's UNSUPPORTED cases come first)
        ultra::set_error("ultra_filtered_topk_live: n_live is NULL");
        return ULTRA_ERR_INVALID;
    }
    return filtered_topk_impl("ultra_filtered_topk_live", score, known_ptr, known_index, batch, n_cand, k, ids_out, scores_out,
                              count_out, workspace, workspace_bytes, n_live, nullptr, nullptr, stream);
}

extern "C" int32_t ultra_filtered_topk_alive(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                             int64_t n_cand, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out,
                                             void *workspace, int64_t workspace_bytes, const int64_t *n_live,
                                             const uint32_t *retired_bits, const int64_t *n_retired, void *stream) {
    // (the parent's UNSUPPORTED cases come first)
    if ((!retired_bits || !n_retired) && k >= 1 && k <= ULTRA_TOPK_MAX && n_cand < (int64_t)1 << 31) {
        ultra::set_error("ultra_filtered_topk_alive: retired_bits or n_retired is NULL");
        return ULTRA_ERR_INVALID;
    }
    return filtered_topk_impl("ultra_filtered_topk_alive", score, known_ptr, known_index, batch, n_cand, k, ids_out, scores_out,
                              count_out, workspace, workspace_bytes, n_live, retired_bits, n_retired, stream);
}
