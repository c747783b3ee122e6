// What the selections over a row's slots (topk_kernels.hip, above_kernels.hip) and the selections among a row's candidate list
// (among_kernels.hip) share: the selection of the k largest keys of a workgroup, the merge of partial lists, the
// output of the answers, the sort of a chunk's run of keys, and the host side of the answer sets' scan and merge launches.
// Moved here from the two files, text unchanged: the parents' kernels keep their code and their bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ultra_nbfnet.h"
#include "score_key.hpp"

namespace ultra {

constexpr int TOPK_THREADS = 256;
constexpr int TOPK_CHUNK = ULTRA_TOPK_CHUNK;
constexpr int TOPK_MAX = ULTRA_TOPK_MAX;
constexpr int TOPK_CHUNK_BITS = 12;
static_assert(TOPK_CHUNK == 1 << TOPK_CHUNK_BITS, "the in-chunk key packs the local index into TOPK_CHUNK_BITS bits");
static_assert(TOPK_THREADS == 256 && TOPK_MAX <= TOPK_THREADS, "one thread per histogram bin and per survivor");

typedef unsigned long long u64;

constexpr int TOPK_SLOTS = TOPK_CHUNK / TOPK_THREADS;      // fresh keys a thread holds; one more slot takes a survivor (merge)
constexpr int TOPK_HELD = TOPK_SLOTS + 1;

struct TopkScratch {
    unsigned hist[256];
    u64 surv[TOPK_MAX];
    u64 top[TOPK_THREADS];      // every thread's largest key
    u64 prefix, low;
    unsigned remaining, done, count, cursor;
};

// surv[0 .. m) -> sorted[0 .. min(m, k)), descending: rank by counting, the keys are distinct.  m <= TOPK_THREADS.
__device__ __forceinline__ void rank_sort(const u64 *surv, int m, int k, u64 *sorted) {
    const int tid = threadIdx.x;
    if (tid < m) {
        const u64 key = surv[tid];
        int r = 0;
        for (int j = 0; j < m; ++j) r += surv[j] > key ? 1 : 0;
        if (r < k) sorted[r] = key;
    }
}

// The keys of a workgroup, TOPK_HELD in the registers of every thread: 0 = absent, the others distinct and below 2^(8 bytes).
// Leaves the m = min(k, #present) largest in sorted[0 .. m) (LDS), descending, and returns m (the same in every thread).  Ends
// with a barrier.
//
// Most keys never reach the selection proper: every thread publishes its largest key; the k-th largest of those 256 maxima is
// a floor under the k-th largest key (k keys, the maxima above it, are at least as large), so only keys at or above the floor
// stay.  For scores in no particular order that is little more than k keys, which are ranked by counting.  When more than
// TOPK_MAX stay (the winners crowd into few threads, or k is close to the number of threads) a radix select, a byte per pass
// from the top, finds the k-th largest among them first.
__device__ int select_topk(u64 (&held)[TOPK_HELD], int k, int bytes, TopkScratch &s, u64 *sorted) {
    const int tid = threadIdx.x;
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < TOPK_HELD; ++j) best = held[j] > best ? held[j] : best;
    s.top[tid] = best;
    if (tid == 0) s.low = 1, s.cursor = 0, s.count = 0;      // (fewer than k threads hold a key: everything present stays)
    __syncthreads();
    {
        int r = 0;
        for (int j = 0; j < TOPK_THREADS; ++j) r += s.top[j] > best ? 1 : 0;
        if (best != 0 && r == k - 1) s.low = best;
    }
    __syncthreads();
    const u64 low = s.low;
    int stay = 0;
#pragma unroll
    for (int j = 0; j < TOPK_HELD; ++j) {
        held[j] = held[j] >= low ? held[j] : 0;     // (an absent key, 0, is below any floor)
        stay += held[j] != 0 ? 1 : 0;
    }
    unsigned at = stay ? atomicAdd(&s.cursor, (unsigned)stay) : 0u;       // (the order is settled by the sort below)
    __syncthreads();
    const int n = (int)s.cursor;
    if (n <= TOPK_MAX) {
#pragma unroll
        for (int j = 0; j < TOPK_HELD; ++j)
            if (held[j] != 0) s.surv[at++] = held[j];
        __syncthreads();
        rank_sort(s.surv, n, k, sorted);
        __syncthreads();
        return n < k ? n : k;
    }
    // more than TOPK_MAX >= k keys are left: radix select of the k-th largest
    u64 prefix = 0;
    unsigned remaining = (unsigned)k;
    int p = bytes - 1;
    for (;; --p) {
        s.hist[tid] = 0;
        __syncthreads();
        const int above_shift = 8 * (p + 1);
#pragma unroll
        for (int j = 0; j < TOPK_HELD; ++j) {
            const u64 key = held[j];
            const bool match = above_shift >= 64 ? true : (key >> above_shift) == prefix;
            if (key != 0 && match) atomicAdd(&s.hist[(unsigned)(key >> (8 * p)) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {     // (the whole first wave) lane l owns bins 4 l .. 4 l + 3; suffix sums from the top bin down
            const unsigned c = s.hist[4 * tid] + s.hist[4 * tid + 1] + s.hist[4 * tid + 2] + s.hist[4 * tid + 3];
            unsigned incl = c;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_down(incl, off);
                if (tid + off < 64) incl += v;
            }
            const unsigned above = incl - c;
            if (incl >= remaining && above < remaining) {      // exactly one lane
                unsigned acc = above, h = 0;
                int d = 3;
                for (; d > 0; --d) {
                    h = s.hist[4 * tid + d];
                    if (acc + h >= remaining) break;
                    acc += h;
                }
                if (d == 0) h = s.hist[4 * tid];
                s.prefix = (prefix << 8) | (u64)(4 * tid + d);
                s.remaining = remaining - acc;
                s.done = (acc + h == remaining) ? 1u : 0u;      // the bins from here up hold exactly what is wanted
            }
        }
        __syncthreads();
        prefix = s.prefix;
        remaining = s.remaining;
        if (s.done || p == 0) break;
    }
    const u64 threshold = prefix << (8 * p);
#pragma unroll
    for (int j = 0; j < TOPK_HELD; ++j) {
        if (held[j] != 0 && held[j] >= threshold) {
            const unsigned slot = atomicAdd(&s.count, 1u);
            if (slot < (unsigned)TOPK_MAX) s.surv[slot] = held[j];
        }
    }
    __syncthreads();
    const int m = (int)s.count < k ? (int)s.count : k;
    rank_sort(s.surv, m, k, sorted);
    __syncthreads();
    return m;
}

// (n_cand: the row's LIVE candidates that are not retired, of which the known ids are a part)
__device__ void write_answers(const float *row, long long n_cand, long long n_known, int k, int m, const u64 *sorted,
                              int64_t *ids_out, unsigned *scores_out, int64_t *count_out) {
    const int tid = threadIdx.x;
    if (tid < k) {
        if (tid < m) {
            const unsigned id = ~(unsigned)sorted[tid];
            ids_out[tid] = (int64_t)id;
            scores_out[tid] = __float_as_uint(row[id]);
        } else {
            ids_out[tid] = -1;
            scores_out[tid] = 0xff800000u;
        }
    }
    if (tid == 0) {
        const long long left = n_cand - n_known;
        *count_out = left < 0 ? 0 : (left < k ? left : k);
    }
}

// The number of live candidates of a row of n_cand slots: *n_live clamped to [0, n_cand]; NULL: every slot.
__device__ __forceinline__ long long live_count(const int64_t *__restrict__ n_live, long long n_cand) {
    if (!n_live) return n_cand;
    const long long v = *n_live;
    return v < 0 ? 0 : (v < n_cand ? v : n_cand);
}

// The `total` keys of a row's partial lists at src (0 = absent) streamed through select_topk, any number of them: leaves the
// m = min(k, #present) largest in sorted[0 .. m), descending, and returns m.  Every thread of the workgroup calls it.
__device__ __forceinline__ int merge_partial_lists(const u64 *__restrict__ src, long long total, int k, TopkScratch &s,
                                                   u64 *sorted) {
    const int tid = threadIdx.x;
    int m = 0;
    for (long long pos = 0; pos < total; pos += TOPK_CHUNK) {
        u64 held[TOPK_HELD];
#pragma unroll
        for (int j = 0; j < TOPK_SLOTS; ++j) {      // the next stretch of partial lists (all loads in flight at once) ...
            const long long i = pos + tid + j * TOPK_THREADS;
            held[j] = i < total ? src[i] : 0;
        }
        held[TOPK_SLOTS] = tid < m ? sorted[tid] : 0;      // ... and the survivors so far
        __syncthreads();       // (sorted[] is rewritten by the selection)
        m = select_topk(held, k, 8, s, sorted);
    }
    return m;
}

// ---- the answer sets (above_kernels.hip) ----
constexpr int ABOVE_THREADS = 256;
constexpr int ABOVE_CHUNK = ULTRA_TOPK_CHUNK;
constexpr int ABOVE_SLOTS = ABOVE_CHUNK / ABOVE_THREADS;      // candidates a thread holds
constexpr int ABOVE_TILE = 2048;                              // merged keys one workgroup of a merge level produces
constexpr int ABOVE_ITEMS = ABOVE_TILE / ABOVE_THREADS;
constexpr int ABOVE_TILES_PER_CHUNK = ABOVE_CHUNK / ABOVE_TILE;
constexpr long long ABOVE_MAX_BATCH = 65535;
static_assert(ABOVE_CHUNK % ABOVE_TILE == 0 && ABOVE_TILE % ABOVE_THREADS == 0, "tiles cut chunks evenly");
static_assert((ABOVE_CHUNK & (ABOVE_CHUNK - 1)) == 0, "the bitonic sort runs over powers of two up to a chunk");

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;       // (lane 0 holds the sum)
}

// keys[0 .. m) (LDS, ABOVE_CHUNK words, distinct) sorted descending (bitonic, over the next power of two of m) and written at
// position at_out of the output: ids and the STORED bits of their scores where the row has one chunk (`finished`), else keys.
// Every thread of the workgroup calls it, after the barrier that follows the last write of keys[].
__device__ __forceinline__ void sort_and_write_run(u64 *keys, int m, const float *__restrict__ row, long long at_out, bool finished,
                                                   u64 *__restrict__ keys_out, int64_t *__restrict__ ids_out,
                                                   unsigned *__restrict__ scores_out) {
    const int tid = threadIdx.x;
    if (m == 0) return;
    int p = 1;
    while (p < m) p <<= 1;
    for (int i = m + tid; i < p; i += ABOVE_THREADS) keys[i] = 0;      // absent keys sort last
    __syncthreads();
    for (int k = 2; k <= p; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (p >> 1); t += ABOVE_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool descending = (i & k) == 0;
                const u64 x = keys[i], y = keys[l];
                if ((x < y) == descending) keys[i] = y, keys[l] = x;
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < m; t += ABOVE_THREADS) {
        const u64 key = keys[t];
        if (finished) {
            const unsigned id = ~(unsigned)key;
            ids_out[at_out + t] = (int64_t)id;
            scores_out[at_out + t] = __float_as_uint(row[id]);
        } else {
            keys_out[at_out + t] = key;
        }
    }
}

// The host side of the launches that follow the per-chunk counts and the per-chunk fill (above_kernels.hip): n_chunk chunks a
// row, whatever a chunk is a chunk of.  counts (batch * n_chunk, 2) int32; offs (batch * n_chunk + 1); keys0 holds the filled
// runs, keys1 is the other buffer; n_cand is the row stride of score.  hipSuccess, or the launch's error.
hipError_t launch_above_scan(const int *counts, long long batch, long long n_chunk, long long *offs, int64_t *ptr_out,
                             int64_t *size_out, hipStream_t s);
hipError_t launch_above_merges(const float *score, long long n_cand, long long batch, long long n_chunk, const long long *offs,
                               u64 *keys0, u64 *keys1, int64_t *ids_out, unsigned *scores_out, hipStream_t s);

}  // namespace ultra
