// The selections AMONG a candidate list per row (include/ultra_nbfnet.h: ultra_filtered_topk_among, ultra_filtered_above_among,
// ultra_filtered_rank_among): the dual of the known lists -- an ALLOW list.
//
//   candidates of row b = among_index[among_span[b][0] : among_span[b][1]], ids ascending and distinct (the known-list
//   contract), the span cut to among_capacity on the device.  An id v of the list is ELIGIBLE iff 0 <= v < live and its retired
//   bit is clear; any other id is absent: its score slot is never loaded, it is never counted, it is never an index.
//
// The order, the keys and the selection are those of the parents (topk_select.hpp: select_topk, merge_partial_lists,
// write_answers, sort_and_write_run; above_kernels.hip's scan and merge kernels through launch_above_scan / _merges).  What
// differs is where a chunk's candidates come from: a workgroup owns ULTRA_TOPK_CHUNK LIST POSITIONS of a row, a thread loads its
// TOPK_SLOTS ids first and then GATHERS their scores and their retired words, both in flight before either is looked at (the
// rule of score_key.hpp; a thread's ids share no bit position, so each id has its own word).  The list is ascending, so the
// local index still orders the ids inside a chunk: the short in-chunk key of topk_chunk_kernel carries over.
//
// The known knock-out: the chunk's id range [first, last] is bracketed in known(b) by two binary searches (the same in every
// thread); every eligible candidate then searches that slice -- staged in LDS where it holds at most AMONG_KNOWN_LDS ids, else
// in place.
//
// What is COUNTED: count / size / num_negative cannot be had from live - retired - |known| here; every chunk counts its own
// eligible candidates -- top-k: the survivors beside its partial list, added up by the merge; above: the two counts of
// above_count_kernel; rank: two integer atomics per wave, on rank and num_negative, both zeroed by a kernel.
//
// The grids, the workspaces and the number of launches depend on (batch, among_capacity) alone; the spans, the lists, the live
// count and the retired bitmap are read by the kernels: a recorded call serves any later values within the capacity.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"
#include "score_key.hpp"
#include "topk_select.hpp"

namespace ultra {

constexpr int AMONG_THREADS = TOPK_THREADS;
constexpr int AMONG_SLOTS = TOPK_SLOTS;
constexpr int AMONG_KNOWN_LDS = 2048;      // the ids of known(b) inside a chunk's id range that are staged in LDS
static_assert(ABOVE_THREADS == AMONG_THREADS && ABOVE_CHUNK == TOPK_CHUNK, "one chunk shape for the three selections");

// The list positions of chunk [lo, lo + TOPK_CHUNK) of row b: the span cut to `capacity`, an inverted or negative span empty.
// begin: the span's start (read only where the result is positive).
__device__ __forceinline__ int among_in_chunk(const int64_t *__restrict__ span, long long b, long long capacity, long long lo,
                                              long long &begin) {
    const long long s0 = span[2 * b], s1 = span[2 * b + 1];
    begin = s0;
    if (s0 < 0 || s1 <= s0) return 0;
    long long len = s1 - s0;
    len = len < capacity ? len : capacity;
    return (int)(len - lo < TOPK_CHUNK ? (len > lo ? len - lo : 0) : TOPK_CHUNK);
}

// The bit mask of a thread's candidates id[j] (-1: absent) that the ascending slice[0 .. m) lists: a binary search each.  A wave
// none of whose lanes holds candidate j skips its search.
__device__ __forceinline__ unsigned among_known_mask(const int64_t *slice, long long m, const int (&id)[TOPK_SLOTS]) {
    unsigned known = 0u;
#pragma unroll
    for (int j = 0; j < TOPK_SLOTS; ++j) {
        if (id[j] < 0) continue;
        long long x = 0, y = m;
        while (x < y) {
            const long long mid = x + ((y - x) >> 1);
            if (slice[mid] < (long long)id[j]) x = mid + 1; else y = mid;
        }
        if (x < m && slice[x] == (long long)id[j]) known |= 1u << j;
    }
    return known;
}

// The chunk's candidates, candidate j of a thread at list[tid + j * AMONG_THREADS] (list: the chunk's first position, n of them):
// id[j] = the id where it is eligible, else -1; f[j] = its score (0 where absent: never loaded).  Returns the bit mask of the
// thread's candidates that known(b) lists.  known_lds: AMONG_KNOWN_LDS words.  Every thread of the workgroup calls it.
__device__ __forceinline__ unsigned among_load(const float *__restrict__ row, const int64_t *__restrict__ list, int n, long long live,
                                               const uint32_t *__restrict__ retired_bits, const int64_t *__restrict__ known_ptr,
                                               const int64_t *__restrict__ known_index, long long b, int64_t *known_lds,
                                               int (&id)[AMONG_SLOTS], float (&f)[AMONG_SLOTS]) {
    const int tid = threadIdx.x;
    long long v[AMONG_SLOTS];
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j) {
        const int i = tid + j * AMONG_THREADS;
        v[j] = i < n ? list[i] : -1;
    }
    // the gathers: a candidate's score and its retired word, issued together, looked at below
    unsigned word[AMONG_SLOTS];
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j) {
        const bool ok = v[j] >= 0 && v[j] < live;
        id[j] = ok ? (int)v[j] : -1;
        word[j] = (ok && retired_bits) ? retired_bits[v[j] >> 5] : 0u;
        f[j] = ok ? row[v[j]] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j)
        if ((word[j] >> (unsigned)(id[j] & 31)) & 1u) id[j] = -1;      // (an absent candidate's word is 0)
    if (!known_ptr || n == 0) return 0u;        // (the same in every thread)
    const long long k0 = known_ptr[b], k1 = known_ptr[b + 1];
    const long long first = list[0], last = list[n - 1];
    long long a = k0, z = k1;       // first entry >= first
    while (a < z) {
        const long long mid = a + ((z - a) >> 1);
        if (known_index[mid] < first) a = mid + 1; else z = mid;
    }
    long long e = a;
    z = k1;                         // first entry > last
    while (e < z) {
        const long long mid = e + ((z - e) >> 1);
        if (known_index[mid] <= last) e = mid + 1; else z = mid;
    }
    const long long m = e - a;      // (the same in every thread)
    if (m <= 0) return 0u;
    if (m <= AMONG_KNOWN_LDS) {
        for (int i = tid; i < (int)m; i += AMONG_THREADS) known_lds[i] = known_index[a + i];
        __syncthreads();
        return among_known_mask(known_lds, m, id);      // (called on the array itself: LDS reads, not flat ones)
    }
    return among_known_mask(known_index + a, m, id);
}

// The sum of `v` over the workgroup, in every thread.  part: one word per wave.  Ends with a barrier.
__device__ __forceinline__ int block_sum(int v, int *part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < AMONG_THREADS / 64; ++w) total += part[w];
    __syncthreads();
    return total;
}

// partial: (batch * n_chunk, k) keys; counts: (batch * n_chunk) survivor counts behind them.
__global__ void __launch_bounds__(AMONG_THREADS) among_topk_chunk_kernel(
        const float *__restrict__ score, const int64_t *__restrict__ known_ptr, const int64_t *__restrict__ known_index,
        const int64_t *__restrict__ span, const int64_t *__restrict__ among_index, long long n_cand, long long capacity,
        long long n_chunk, int k, u64 *__restrict__ partial, long long *__restrict__ counts, int64_t *ids_out, unsigned *scores_out,
        int64_t *count_out, const int64_t *__restrict__ n_live, const uint32_t *__restrict__ retired_bits) {
    __shared__ int64_t known_lds[AMONG_KNOWN_LDS];
    __shared__ u64 sorted[TOPK_MAX];
    __shared__ TopkScratch s;
    __shared__ int part[AMONG_THREADS / 64];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / n_chunk, c = blockIdx.x % n_chunk;
    const float *row = score + b * n_cand;
    const long long lo = c * TOPK_CHUNK;
    long long begin;
    const int n = among_in_chunk(span, b, capacity, lo, begin);
    const int64_t *list = among_index + begin + lo;     // (dereferenced below n only)
    int id[AMONG_SLOTS];
    float f[AMONG_SLOTS];
    const unsigned known = among_load(row, list, n, live_count(n_live, n_cand), retired_bits, known_ptr, known_index, b, known_lds, id, f);
    // inside a chunk the local index orders the ids (the list is ascending): the in-chunk key of topk_chunk_kernel
    u64 held[TOPK_HELD];
    int stay = 0;
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j) {
        const bool present = id[j] >= 0 && ((known >> j) & 1u) == 0u;
        const unsigned bits = present ? ordered_score(__float_as_uint(f[j])) : 0u;
        held[j] = present ? ((u64)bits << TOPK_CHUNK_BITS) | (u64)(TOPK_CHUNK - 1 - (tid + j * AMONG_THREADS)) : 0;
        stay += present ? 1 : 0;
    }
    held[AMONG_SLOTS] = 0;
    const int survivors = block_sum(stay, part);       // the chunk's eligible candidates that are not known
    const int m = select_topk(held, k, (32 + TOPK_CHUNK_BITS + 7) / 8, s, sorted);
    if (tid < m) {
        const u64 key = sorted[tid];
        const unsigned v = (unsigned)list[TOPK_CHUNK - 1 - (int)(key & (TOPK_CHUNK - 1))];
        sorted[tid] = ((key >> TOPK_CHUNK_BITS) << 32) | (u64)(~v);       // (each thread rewrites its own slot)
    }
    __syncthreads();
    if (n_chunk == 1) {
        write_answers(row, survivors, 0, k, m, sorted, ids_out + b * k, scores_out + b * k, count_out + b);
    } else {
        if (tid < k) partial[((long long)blockIdx.x) * k + tid] = tid < m ? sorted[tid] : 0;
        if (tid == 0) counts[blockIdx.x] = survivors;
    }
}

__global__ void __launch_bounds__(AMONG_THREADS) among_topk_merge_kernel(const float *__restrict__ score, long long n_cand,
                                                                         long long n_chunk, int k, const u64 *__restrict__ partial,
                                                                         const long long *__restrict__ counts, int64_t *ids_out,
                                                                         unsigned *scores_out, int64_t *count_out) {
    __shared__ u64 sorted[TOPK_MAX];
    __shared__ TopkScratch s;
    __shared__ long long part[AMONG_THREADS / 64];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const int m = merge_partial_lists(partial + b * n_chunk * k, n_chunk * k, k, s, sorted);
    long long total = 0;
    for (long long c = tid; c < n_chunk; c += AMONG_THREADS) total += counts[b * n_chunk + c];
    for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off);
    if ((tid & 63) == 0) part[tid >> 6] = total;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < AMONG_THREADS / 64; ++w) total += part[w];
    write_answers(score + b * n_cand, total, 0, k, m, sorted, ids_out + b * k, scores_out + b * k, count_out + b);
}

// A thread's members of the answer set: bits[j] = ordered_score of candidate j where it is a member that known(b) does not
// list, else 0.  Returns the thread's number of members (before the filter).
__device__ __forceinline__ int among_members(const int (&id)[AMONG_SLOTS], const float (&f)[AMONG_SLOTS], unsigned known,
                                             float threshold, unsigned (&bits)[AMONG_SLOTS]) {
    int members = 0;
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j) {
        const bool member = id[j] >= 0 && f[j] > threshold;
        members += member ? 1 : 0;
        bits[j] = (member && ((known >> j) & 1u) == 0u) ? ordered_score(__float_as_uint(f[j])) : 0u;
    }
    return members;
}

// counts (batch * n_chunk, 2): the layout of above_count_kernel -- members, members kept.
__global__ void __launch_bounds__(AMONG_THREADS) among_above_count_kernel(
        const float *__restrict__ score, const int64_t *__restrict__ known_ptr, const int64_t *__restrict__ known_index,
        const int64_t *__restrict__ span, const int64_t *__restrict__ among_index, long long n_cand, long long capacity,
        long long n_chunk, float threshold, int *__restrict__ counts, const int64_t *__restrict__ n_live,
        const uint32_t *__restrict__ retired_bits) {
    __shared__ int64_t known_lds[AMONG_KNOWN_LDS];
    __shared__ int part[AMONG_THREADS / 64];
    const long long b = blockIdx.x / n_chunk, c = blockIdx.x % n_chunk;
    const long long lo = c * TOPK_CHUNK;
    long long begin;
    const int n = among_in_chunk(span, b, capacity, lo, begin);
    int id[AMONG_SLOTS];
    float f[AMONG_SLOTS];
    const unsigned known = among_load(score + b * n_cand, among_index + begin + lo, n, live_count(n_live, n_cand), retired_bits,
                                      known_ptr, known_index, b, known_lds, id, f);
    unsigned bits[AMONG_SLOTS];
    int members = among_members(id, f, known, threshold, bits);
    int kept = 0;
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j) kept += bits[j] != 0u ? 1 : 0;
    members = block_sum(members, part);
    kept = block_sum(kept, part);
    if (threadIdx.x == 0) {
        counts[2 * (long long)blockIdx.x] = members;
        counts[2 * (long long)blockIdx.x + 1] = kept;
    }
}

__global__ void __launch_bounds__(AMONG_THREADS) among_above_fill_kernel(
        const float *__restrict__ score, const int64_t *__restrict__ known_ptr, const int64_t *__restrict__ known_index,
        const int64_t *__restrict__ span, const int64_t *__restrict__ among_index, long long n_cand, long long capacity,
        long long n_chunk, float threshold, const long long *__restrict__ offs, u64 *__restrict__ keys_out,
        int64_t *__restrict__ ids_out, unsigned *__restrict__ scores_out, const int64_t *__restrict__ n_live,
        const uint32_t *__restrict__ retired_bits) {
    __shared__ int64_t known_lds[AMONG_KNOWN_LDS];
    __shared__ u64 keys[ABOVE_CHUNK];
    __shared__ unsigned cursor;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / n_chunk, c = blockIdx.x % n_chunk;
    const float *row = score + b * n_cand;
    const long long lo = c * TOPK_CHUNK;
    long long begin;
    const int n = among_in_chunk(span, b, capacity, lo, begin);
    if (tid == 0) cursor = 0;
    int id[AMONG_SLOTS];
    float f[AMONG_SLOTS];
    const unsigned known = among_load(row, among_index + begin + lo, n, live_count(n_live, n_cand), retired_bits, known_ptr,
                                      known_index, b, known_lds, id, f);
    unsigned bits[AMONG_SLOTS];
    among_members(id, f, known, threshold, bits);
    int stay = 0;
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j) stay += bits[j] != 0u ? 1 : 0;
    __syncthreads();
    unsigned at = stay ? atomicAdd(&cursor, (unsigned)stay) : 0u;       // (the order is settled by the sort below)
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j)
        if (bits[j] != 0u) keys[at++] = ((u64)bits[j] << 32) | (u64)(~(unsigned)id[j]);
    __syncthreads();
    // (cursor: the chunk's kept count, what among_above_count_kernel wrote)
    sort_and_write_run(keys, (int)cursor, row, offs[blockIdx.x], n_chunk == 1, keys_out, ids_out, scores_out);
}

// rank and num_negative = 0 ahead of the atomics: a kernel, never a memset node (rank_kernels.hip: rank_zero_kernel).
__global__ void __launch_bounds__(256) among_rank_zero_kernel(unsigned long long *rank, unsigned long long *num_negative,
                                                              long long batch) {
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < batch; q += (long long)gridDim.x * 256) rank[q] = 0, num_negative[q] = 0;
}

__global__ void __launch_bounds__(AMONG_THREADS) among_rank_kernel(
        const float *__restrict__ score, const int64_t *__restrict__ pos, const int64_t *__restrict__ known_ptr,
        const int64_t *__restrict__ known_index, const int64_t *__restrict__ span, const int64_t *__restrict__ among_index,
        long long n_cand, long long capacity, long long n_chunk, unsigned long long *rank, unsigned long long *num_negative,
        const int64_t *__restrict__ n_live, const uint32_t *__restrict__ retired_bits) {
    __shared__ int64_t known_lds[AMONG_KNOWN_LDS];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x / n_chunk, c = blockIdx.x % n_chunk;
    const float *row = score + q * n_cand;
    const float pos_score = row[pos[q]];
    const long long lo = c * TOPK_CHUNK;
    long long begin;
    const int n = among_in_chunk(span, q, capacity, lo, begin);
    int id[AMONG_SLOTS];
    float f[AMONG_SLOTS];
    const unsigned known = among_load(row, among_index + begin + lo, n, live_count(n_live, n_cand), retired_bits, known_ptr,
                                      known_index, q, known_lds, id, f);
    int count = (c == 0 && tid == 0) ? 1 : 0;       // the leading "+ 1" of the rank
    int negative = 0;
#pragma unroll
    for (int j = 0; j < AMONG_SLOTS; ++j) {
        const bool present = id[j] >= 0 && ((known >> j) & 1u) == 0u;
        negative += present ? 1 : 0;
        count += (present && pos_score <= f[j]) ? 1 : 0;
    }
    // wave reduce, then one atomic per wave and counter (integer: order independent)
    count = wave_sum(count);
    negative = wave_sum(negative);
    if ((tid & 63) == 0) {
        if (count) atomicAdd(rank + q, (unsigned long long)count);
        if (negative) atomicAdd(num_negative + q, (unsigned long long)negative);
    }
}

static int64_t among_chunks(int64_t among_capacity) { return (among_capacity + ULTRA_TOPK_CHUNK - 1) / ULTRA_TOPK_CHUNK; }

}  // namespace ultra

// Layout: partial lists (batch * chunks, k) uint64 | survivor counts (batch * chunks) int64.
extern "C" int64_t ultra_filtered_topk_among_workspace(int64_t batch, int64_t among_capacity, int32_t k) {
    if (batch < 0 || among_capacity < 0 || among_capacity >= (int64_t)1 << 31 || k < 1 || k > ULTRA_TOPK_MAX) return -1;
    return batch * ultra::among_chunks(among_capacity) * ((int64_t)k + 1) * (int64_t)sizeof(uint64_t);
}

extern "C" int32_t ultra_filtered_topk_among(const void *score, const int64_t *known_ptr, const int64_t *known_index,
                                             const int64_t *among_span, const int64_t *among_index, int64_t batch, int64_t n_cand,
                                             int64_t among_capacity, int32_t k, int64_t *ids_out, void *scores_out,
                                             int64_t *count_out, void *workspace, int64_t workspace_bytes, const int64_t *n_live,
                                             const uint32_t *retired_bits, const int64_t *n_retired, void *stream) {
    const std::string who("ultra_filtered_topk_among");
    (void)n_retired;        // (part of the optional operands of every selection; the counts here are counted, not derived)
    if (k < 1 || k > ULTRA_TOPK_MAX || n_cand >= (int64_t)1 << 31) {      // (before any pointer is looked at)
        ultra::set_error(who + ": k must lie in [1, " + std::to_string(ULTRA_TOPK_MAX) + "] and n_cand below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (!score || !among_span || !among_index || !ids_out || !scores_out || !count_out || batch < 0 || n_cand <= 0 ||
        among_capacity <= 0 || among_capacity >= (int64_t)1 << 31) {
        ultra::set_error(who + ": NULL operand, empty candidate set or among_capacity outside [1, 2^31)");
        return ULTRA_ERR_INVALID;
    }
    const int64_t n_chunk = ultra::among_chunks(among_capacity);
    const int64_t need = ultra_filtered_topk_among_workspace(batch, among_capacity, k);
    if (workspace_bytes < need || (need > 0 && !workspace) || ((uintptr_t)workspace & 7u) != 0) {
        ultra::set_error(who + ": workspace of " + std::to_string(workspace_bytes) + " bytes, needs " + std::to_string(need) +
                         " (8-byte aligned)");
        return ULTRA_ERR_INVALID;
    }
    if (batch * n_chunk >= (int64_t)1 << 31) {
        ultra::set_error(who + ": batch * chunks per list must stay below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch == 0) return ULTRA_OK;
    ULTRA_DEVICE_SCOPE(stream, score);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    ultra::u64 *partial = (ultra::u64 *)workspace;
    long long *counts = (long long *)(partial + batch * n_chunk * k);
    hipLaunchKernelGGL(ultra::among_topk_chunk_kernel, dim3((unsigned)(batch * n_chunk)), dim3(ultra::AMONG_THREADS), 0, s,
                       (const float *)score, known_ptr, known_index, among_span, among_index, (long long)n_cand,
                       (long long)among_capacity, (long long)n_chunk, (int)k, partial, counts, ids_out, (unsigned *)scores_out,
                       count_out, n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("among_topk_chunk_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    if (n_chunk > 1) {
        hipLaunchKernelGGL(ultra::among_topk_merge_kernel, dim3((unsigned)batch), dim3(ultra::AMONG_THREADS), 0, s,
                           (const float *)score, (long long)n_cand, (long long)n_chunk, (int)k, (const ultra::u64 *)partial,
                           (const long long *)counts, ids_out, (unsigned *)scores_out, count_out);
        if (hipGetLastError() != hipSuccess) {
            ultra::set_error("among_topk_merge_kernel launch failed");
            return ULTRA_ERR_HIP;
        }
    }
    return ULTRA_OK;
}

// The layout of ultra_filtered_above_workspace over rows of among_capacity list positions.
extern "C" int64_t ultra_filtered_above_among_workspace(int64_t batch, int64_t among_capacity) {
    return ultra_filtered_above_workspace(batch, among_capacity);
}

extern "C" int32_t ultra_filtered_above_among(const void *score, const int64_t *known_ptr, const int64_t *known_index,
                                              const int64_t *among_span, const int64_t *among_index, int64_t batch, int64_t n_cand,
                                              int64_t among_capacity, float threshold, int64_t *ptr_out, int64_t *ids_out,
                                              void *scores_out, int64_t capacity, int64_t *size_out, void *workspace,
                                              int64_t workspace_bytes, const int64_t *n_live, const uint32_t *retired_bits,
                                              const int64_t *n_retired, void *stream) {
    const std::string who("ultra_filtered_above_among");
    (void)n_retired;        // (the answer sets have no count that needs it: above_kernels.hip)
    if (n_cand >= (int64_t)1 << 31 || std::isnan(threshold) || (std::isinf(threshold) && threshold > 0)) {      // (before any pointer is looked at)
        ultra::set_error(who + ": n_cand must stay below 2^31 and the threshold be finite or -inf");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (!score || !among_span || !among_index || !ptr_out || !ids_out || !scores_out || !size_out || n_cand <= 0 || batch < 0 ||
        batch > ultra::ABOVE_MAX_BATCH || among_capacity <= 0 || among_capacity >= (int64_t)1 << 31) {
        ultra::set_error(who + ": NULL operand, empty candidate set, batch outside [0, 65535] or among_capacity outside [1, 2^31)");
        return ULTRA_ERR_INVALID;
    }
    if (capacity < batch * among_capacity) {
        ultra::set_error(who + ": capacity " + std::to_string(capacity) + " is below batch * among_capacity = " +
                         std::to_string(batch * among_capacity));
        return ULTRA_ERR_INVALID;
    }
    const int64_t need = ultra_filtered_above_among_workspace(batch, among_capacity);
    if (need < 0 || workspace_bytes < need || !workspace || ((uintptr_t)workspace & 7u) != 0) {
        ultra::set_error(who + ": workspace of " + std::to_string(workspace_bytes) + " bytes, needs " + std::to_string(need) +
                         " (8-byte aligned)");
        return ULTRA_ERR_INVALID;
    }
    const int64_t n_chunk = ultra::among_chunks(among_capacity);
    const int64_t slots = batch * n_chunk;
    if (slots * ultra::ABOVE_TILES_PER_CHUNK >= (int64_t)1 << 31) {
        ultra::set_error(who + ": batch * chunks per list must stay below 2^30");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch == 0) return ULTRA_OK;
    long long *offs = (long long *)workspace;
    ultra::u64 *keys0 = (ultra::u64 *)(offs + slots + 1), *keys1 = keys0 + batch * among_capacity;
    int *counts = (int *)(keys1 + batch * among_capacity);
    ULTRA_DEVICE_SCOPE(stream, score);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    const dim3 threads(ultra::AMONG_THREADS);
    hipLaunchKernelGGL(ultra::among_above_count_kernel, dim3((unsigned)slots), threads, 0, s, (const float *)score, known_ptr,
                       known_index, among_span, among_index, (long long)n_cand, (long long)among_capacity, (long long)n_chunk,
                       threshold, counts, n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("among_above_count_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    if (ultra::launch_above_scan(counts, batch, n_chunk, offs, ptr_out, size_out, s) != hipSuccess) {
        ultra::set_error("above_scan_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    hipLaunchKernelGGL(ultra::among_above_fill_kernel, dim3((unsigned)slots), threads, 0, s, (const float *)score, known_ptr,
                       known_index, among_span, among_index, (long long)n_cand, (long long)among_capacity, (long long)n_chunk,
                       threshold, (const long long *)offs, keys0, ids_out, (unsigned *)scores_out, n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("among_above_fill_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    if (ultra::launch_above_merges((const float *)score, n_cand, batch, n_chunk, offs, keys0, keys1, ids_out, (unsigned *)scores_out,
                                   s) != hipSuccess) {
        ultra::set_error("above_merge_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

extern "C" int32_t ultra_filtered_rank_among(const void *score, const int64_t *pos_index, const int64_t *known_ptr,
                                             const int64_t *known_index, const int64_t *among_span, const int64_t *among_index,
                                             int64_t batch, int64_t n_cand, int64_t among_capacity, int64_t *rank_out,
                                             int64_t *num_negative_out, const int64_t *n_live, const uint32_t *retired_bits,
                                             const int64_t *n_retired, void *stream) {
    const std::string who("ultra_filtered_rank_among");
    (void)n_retired;        // (num_negative is counted, not derived)
    if (n_cand >= (int64_t)1 << 31) {      // (before any pointer is looked at)
        ultra::set_error(who + ": n_cand must stay below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (!score || !pos_index || !known_ptr || !among_span || !among_index || !rank_out || !num_negative_out || batch < 0 ||
        n_cand <= 0 || among_capacity <= 0 || among_capacity >= (int64_t)1 << 31) {
        ultra::set_error(who + ": NULL operand, empty candidate set or among_capacity outside [1, 2^31)");
        return ULTRA_ERR_INVALID;
    }
    const int64_t n_chunk = ultra::among_chunks(among_capacity);
    if (batch * n_chunk >= (int64_t)1 << 31) {
        ultra::set_error(who + ": batch * chunks per list must stay below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch == 0) return ULTRA_OK;
    ULTRA_DEVICE_SCOPE(stream, score);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    const unsigned blocks = (unsigned)(batch < 256 * 1024 ? (batch + 255) / 256 : 1024);
    hipLaunchKernelGGL(ultra::among_rank_zero_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<unsigned long long *>(rank_out),
                       reinterpret_cast<unsigned long long *>(num_negative_out), (long long)batch);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error(who + ": among_rank_zero_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    hipLaunchKernelGGL(ultra::among_rank_kernel, dim3((unsigned)(batch * n_chunk)), dim3(ultra::AMONG_THREADS), 0, s,
                       (const float *)score, pos_index, known_ptr, known_index, among_span, among_index, (long long)n_cand,
                       (long long)among_capacity, (long long)n_chunk, reinterpret_cast<unsigned long long *>(rank_out),
                       reinterpret_cast<unsigned long long *>(num_negative_out), n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("among_rank_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}
