// Answer sets of a batch of queries: every candidate above a threshold, ranked (include/ultra_nbfnet.h: ultra_filtered_above;
// DESIGN.md §16).
//
//   members of row b = ids v with score[b, v] > threshold (fp32, strict: a NaN is never a member); size[b] counts them all;
//   the list of row b = the members not in known(b), in the order of ultra_filtered_topk: score descending, equal scores by
//   ascending id, -0.0 == +0.0.  Its length is decided by the data; the lists lie back to back at ptr_out.
//
// The 64-bit key of topk_kernels.hip carries the order (ordered_score in the high word, ~id in the low word: distinct within
// a row, a larger key is an earlier answer, 0 is free for "absent").  Launches, the kernel boundary the only synchronisation
// between them, their number a function of (batch, n_cand) alone:
//   1. above_count_kernel: one workgroup per (row, chunk of ULTRA_TOPK_CHUNK candidates) evaluates the predicate, knocks out
//      the chunk's slice of known(b) exactly as topk_chunk_kernel does, and writes two counts: members, members kept;
//   2. above_scan_kernel: one workgroup scans the kept counts in (row, chunk) order into the position of every chunk's run in
//      the output (the runs of a row are adjacent, the rows too) and writes ptr_out and size_out;
//   3. above_fill_kernel: (row, chunk) again -- the same predicate and knock-out, the survivors' keys sorted descending in LDS
//      (bitonic, over the next power of two of their number) and written at the chunk's position; a row of one chunk is
//      finished here;
//   4. ceil(log2(chunks)) launches of above_merge_kernel: at width w neighbouring runs of w chunks are merged from one key
//      buffer into the other -- the grid covers the upper bound of every pair's merged length in tiles of ABOVE_TILE keys, a
//      workgroup finds its tile's split on the merge path, merges in LDS and leaves at once when its tile lies beyond the
//      pair's true length; an unpaired last run is a merge with an empty partner (a copy).  The last level writes ids and the
//      STORED bits of the scores (gathered from the score matrix: -0.0 stays -0.0) instead of keys.
// The key buffers are indexed by output position, so a pair's merged run lies exactly where its two runs lay.  LDS atomics
// only hand out compaction slots before the sort; the keys are distinct, so no output depends on the order they land in.
//
// A LIVE COUNT (ultra_filtered_above_live): the row stride, the grid, the workspace layout and the number of
// launches stay those of n_cand SLOTS; only the ids below *n_live -- read on the device, clamped to [0, n_cand] -- are looked at.
// A dead id is never loaded (a NaN or +inf in its slot is no member and reaches no key), a chunk wholly beyond the live count
// writes its two zero counts and an empty run, so the scan and every merge level see what they see for an empty chunk.
// n_live == NULL (ultra_filtered_above) means n_cand: the same kernels, the same bits.
//
// RETIRED IDS (ultra_filtered_above_alive): a device bitmap names ids below the live count that are absent.  Both
// passes over a chunk zero a retired candidate's key next to the predicate -- before the members are counted, so size_out never
// counts it, and before the knock-out and the sort.  The retired count is not needed here.  retired_bits == NULL: the _live twin
// and the parent, the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"
#include "score_key.hpp"
#include "topk_select.hpp"      // the ABOVE_ constants, wave_sum, sort_and_write_run, the scan and merge launches

namespace ultra {

// The candidates of chunk [lo, lo + ABOVE_CHUNK) of a row of n_cand slots of which the ids below *n_live (clamped to
// [0, n_cand]; NULL: all) are live: 0 for a chunk beyond the live count.
__device__ __forceinline__ int live_in_chunk(const int64_t *__restrict__ n_live, long long n_cand, long long lo) {
    long long live = n_cand;
    if (n_live) {
        const long long v = *n_live;
        live = v < 0 ? 0 : (v < n_cand ? v : n_cand);
    }
    return (int)(live - lo < ABOVE_CHUNK ? (live > lo ? live - lo : 0) : ABOVE_CHUNK);
}

// The chunk [lo, lo + n) of `row`: bits[j] = ordered_score of candidate tid + j * ABOVE_THREADS when it is a member that
// known(b) does not list, else 0.  Returns this thread's number of members (before the filter).  A candidate whose bit is set
// in retired_bits (NULL: none) is no member.  ord: ABOVE_CHUNK words of LDS, touched only when the chunk's slice of known(b) is
// non-empty.  Every thread of the workgroup calls it.
__device__ __forceinline__ int chunk_survivors(const float *__restrict__ row, long long lo, int n, float threshold,
                                               const int64_t *__restrict__ known_ptr, const int64_t *__restrict__ known_index,
                                               long long b, unsigned *ord, unsigned (&bits)[ABOVE_SLOTS],
                                               const uint32_t *__restrict__ retired_bits) {
    const int tid = threadIdx.x;
    unsigned mask[ABOVE_SLOTS];
    retired_slots<ABOVE_SLOTS, ABOVE_THREADS>(retired_bits, lo, n, mask);      // (in flight with the scores)
    float v[ABOVE_SLOTS];
#pragma unroll
    for (int j = 0; j < ABOVE_SLOTS; ++j) {
        const int i = tid + j * ABOVE_THREADS;
        v[j] = i < n ? row[lo + i] : 0.f;
    }
    int members = 0;
#pragma unroll
    for (int j = 0; j < ABOVE_SLOTS; ++j) {
        const int i = tid + j * ABOVE_THREADS;
        bits[j] = (i < n && v[j] > threshold && !slot_retired(mask[j])) ? ordered_score(__float_as_uint(v[j])) : 0u;
        members += bits[j] != 0u ? 1 : 0;
    }
    if (!known_ptr) return members;
    const long long k0 = known_ptr[b], k1 = known_ptr[b + 1];
    long long a = k0, z = k1;       // first entry >= lo
    while (a < z) {
        const long long mid = a + ((z - a) >> 1);
        if (known_index[mid] < lo) a = mid + 1; else z = mid;
    }
    if (!(a < k1 && known_index[a] < lo + n)) return members;      // (the same in every thread)
    // the knock-out goes by id: through LDS
#pragma unroll
    for (int j = 0; j < ABOVE_SLOTS; ++j) {
        const int i = tid + j * ABOVE_THREADS;
        if (i < n) ord[i] = bits[j];
    }
    __syncthreads();
    for (long long j = a + tid; j < k1; j += ABOVE_THREADS) {
        const long long id = known_index[j];
        if (id >= lo + n) break;        // ascending: the rest of this thread's entries lie beyond the chunk too
        if (id >= lo) ord[id - lo] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ABOVE_SLOTS; ++j) {
        const int i = tid + j * ABOVE_THREADS;
        bits[j] = i < n ? ord[i] : 0u;
    }
    return members;
}

__global__ void __launch_bounds__(ABOVE_THREADS) above_count_kernel(const float *__restrict__ score, const int64_t *__restrict__ known_ptr,
                                                                    const int64_t *__restrict__ known_index, long long n_cand,
                                                                    long long n_chunk, float threshold, int *__restrict__ counts,
                                                                    const int64_t *__restrict__ n_live,
                                                                    const uint32_t *__restrict__ retired_bits) {
    __shared__ unsigned ord[ABOVE_CHUNK];
    __shared__ int part[2][ABOVE_THREADS / 64];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / n_chunk, c = blockIdx.x % n_chunk;
    const long long lo = c * ABOVE_CHUNK;
    const int n = live_in_chunk(n_live, n_cand, lo);
    unsigned bits[ABOVE_SLOTS];
    int members = chunk_survivors(score + b * n_cand, lo, n, threshold, known_ptr, known_index, b, ord, bits, retired_bits);
    int kept = 0;
#pragma unroll
    for (int j = 0; j < ABOVE_SLOTS; ++j) kept += bits[j] != 0u ? 1 : 0;
    members = wave_sum(members);
    kept = wave_sum(kept);
    if ((tid & 63) == 0) part[0][tid >> 6] = members, part[1][tid >> 6] = kept;
    __syncthreads();
    if (tid < 2) {
        int total = 0;
        for (int w = 0; w < ABOVE_THREADS / 64; ++w) total += part[tid][w];
        counts[2 * (long long)blockIdx.x + tid] = total;
    }
}

// offs[i], i = b * n_chunk + c: the output position of chunk c of row b; offs[batch * n_chunk]: the total.
__global__ void __launch_bounds__(ABOVE_THREADS) above_scan_kernel(const int *__restrict__ counts, long long batch, long long n_chunk,
                                                                   long long *__restrict__ offs, int64_t *__restrict__ ptr_out,
                                                                   int64_t *__restrict__ size_out) {
    __shared__ long long wave_total[ABOVE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m = batch * n_chunk;
    long long carry = 0;
    for (long long base = 0; base < m; base += ABOVE_THREADS) {
        const long long i = base + tid;
        const int v = i < m ? counts[2 * i + 1] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        long long before = carry, tile = 0;
        for (int w = 0; w < ABOVE_THREADS / 64; ++w) {
            before += w < wave ? wave_total[w] : 0;
            tile += wave_total[w];
        }
        if (i < m) {
            const long long at = before + (long long)(incl - v);
            offs[i] = at;
            if (i % n_chunk == 0) ptr_out[i / n_chunk] = at;
        }
        carry += tile;
        __syncthreads();       // (wave_total is rewritten by the next tile)
    }
    if (tid == 0) {
        offs[m] = carry;
        ptr_out[batch] = carry;
    }
    // size: the members of a row, over its chunks -- a wave per row where a row has many chunks, a thread per row otherwise
    if (n_chunk >= 64) {
        for (long long b = wave; b < batch; b += ABOVE_THREADS / 64) {
            long long total = 0;
            for (long long c = lane; c < n_chunk; c += 64) total += counts[2 * (b * n_chunk + c)];
            for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off);
            if (lane == 0) size_out[b] = total;
        }
    } else {
        for (long long b = tid; b < batch; b += ABOVE_THREADS) {
            long long total = 0;
            for (long long c = 0; c < n_chunk; ++c) total += counts[2 * (b * n_chunk + c)];
            size_out[b] = total;
        }
    }
}

__global__ void __launch_bounds__(ABOVE_THREADS) above_fill_kernel(const float *__restrict__ score, const int64_t *__restrict__ known_ptr,
                                                                   const int64_t *__restrict__ known_index, long long n_cand,
                                                                   long long n_chunk, float threshold, const long long *__restrict__ offs,
                                                                   u64 *__restrict__ keys_out, int64_t *__restrict__ ids_out,
                                                                   unsigned *__restrict__ scores_out,
                                                                   const int64_t *__restrict__ n_live,
                                                                   const uint32_t *__restrict__ retired_bits) {
    __shared__ unsigned ord[ABOVE_CHUNK];
    __shared__ u64 keys[ABOVE_CHUNK];
    __shared__ unsigned cursor;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / n_chunk, c = blockIdx.x % n_chunk;
    const float *row = score + b * n_cand;
    const long long lo = c * ABOVE_CHUNK;
    const int n = live_in_chunk(n_live, n_cand, lo);
    if (tid == 0) cursor = 0;
    unsigned bits[ABOVE_SLOTS];
    chunk_survivors(row, lo, n, threshold, known_ptr, known_index, b, ord, bits, retired_bits);
    int stay = 0;
#pragma unroll
    for (int j = 0; j < ABOVE_SLOTS; ++j) stay += bits[j] != 0u ? 1 : 0;
    __syncthreads();
    unsigned at = stay ? atomicAdd(&cursor, (unsigned)stay) : 0u;       // (the order is settled by the sort below)
#pragma unroll
    for (int j = 0; j < ABOVE_SLOTS; ++j) {
        const unsigned id = (unsigned)(lo + tid + j * ABOVE_THREADS);
        if (bits[j] != 0u) keys[at++] = ((u64)bits[j] << 32) | (u64)(~id);
    }
    __syncthreads();
    // (cursor: the chunk's kept count, what above_count_kernel wrote)
    sort_and_write_run(keys, (int)cursor, row, offs[blockIdx.x], n_chunk == 1, keys_out, ids_out, scores_out);
}

// How many of the first d keys of the descending merge of x[0 .. nx) and y[0 .. ny) come from x.  The keys are distinct.
template <typename Index>
__device__ __forceinline__ Index merge_path(const u64 *x, Index nx, const u64 *y, Index ny, Index d) {
    Index lo = d > ny ? d - ny : 0, hi = d < nx ? d : nx;
    while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        if (x[mid] > y[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(ABOVE_THREADS) above_merge_kernel(const float *__restrict__ score, long long n_cand, long long n_chunk,
                                                                    long long width, const long long *__restrict__ offs,
                                                                    const u64 *__restrict__ src, u64 *__restrict__ dst,
                                                                    int64_t *__restrict__ ids_out, unsigned *__restrict__ scores_out,
                                                                    int last) {
    __shared__ u64 in[ABOVE_TILE];
    __shared__ u64 out[ABOVE_TILE];
    __shared__ long long split[2];
    const int tid = threadIdx.x;
    const long long tiles_per_row = n_chunk * ABOVE_TILES_PER_CHUNK;
    const long long b = blockIdx.x / tiles_per_row, t = blockIdx.x % tiles_per_row;
    const long long span = 2 * width * ABOVE_TILES_PER_CHUNK;      // tiles over the upper bound of a pair's merged length
    const long long pair = t / span, tile = t % span;
    const long long c0 = 2 * pair * width;       // (below n_chunk: t < tiles_per_row)
    const long long cm = c0 + width < n_chunk ? c0 + width : n_chunk;
    const long long c1 = c0 + 2 * width < n_chunk ? c0 + 2 * width : n_chunk;
    const long long start_x = offs[b * n_chunk + c0], start_y = offs[b * n_chunk + cm], end = offs[b * n_chunk + c1];
    const long long nx = start_y - start_x, ny = end - start_y;
    const long long d0 = tile * ABOVE_TILE;
    if (d0 >= nx + ny) return;      // (the whole workgroup: beyond the pair's true length)
    const long long d1 = d0 + ABOVE_TILE < nx + ny ? d0 + ABOVE_TILE : nx + ny;
    const u64 *x = src + start_x, *y = src + start_y;
    if (tid < 2) split[tid] = merge_path<long long>(x, nx, y, ny, tid == 0 ? d0 : d1);
    __syncthreads();
    const long long x0 = split[0], y0 = d0 - x0;
    const int mx = (int)(split[1] - x0), count = (int)(d1 - d0), my = count - mx;
    for (int i = tid; i < mx; i += ABOVE_THREADS) in[i] = x[x0 + i];
    for (int i = tid; i < my; i += ABOVE_THREADS) in[mx + i] = y[y0 + i];
    __syncthreads();
    {
        const int d = tid * ABOVE_ITEMS < count ? tid * ABOVE_ITEMS : count;
        const int stop = d + ABOVE_ITEMS < count ? d + ABOVE_ITEMS : count;
        int ix = merge_path<int>(in, mx, in + mx, my, d);
        int iy = d - ix;
        for (int o = d; o < stop; ++o) {
            const bool from_x = iy >= my || (ix < mx && in[ix] > in[mx + iy]);
            out[o] = from_x ? in[ix++] : in[mx + iy++];
        }
    }
    __syncthreads();
    const long long at_out = start_x + d0;
    for (int i = tid; i < count; i += ABOVE_THREADS) {
        const u64 key = out[i];
        if (last) {
            const unsigned id = ~(unsigned)key;
            ids_out[at_out + i] = (int64_t)id;
            scores_out[at_out + i] = __float_as_uint(score[b * n_cand + id]);
        } else {
            dst[at_out + i] = key;
        }
    }
}

static int64_t above_chunks(int64_t n_cand) { return (n_cand + ULTRA_TOPK_CHUNK - 1) / ULTRA_TOPK_CHUNK; }

hipError_t launch_above_scan(const int *counts, long long batch, long long n_chunk, long long *offs, int64_t *ptr_out,
                             int64_t *size_out, hipStream_t s) {
    hipLaunchKernelGGL(above_scan_kernel, dim3(1), dim3(ABOVE_THREADS), 0, s, counts, batch, n_chunk, offs, ptr_out, size_out);
    return hipGetLastError();
}

hipError_t launch_above_merges(const float *score, long long n_cand, long long batch, long long n_chunk, const long long *offs,
                               u64 *keys0, u64 *keys1, int64_t *ids_out, unsigned *scores_out, hipStream_t s) {
    u64 *src = keys0, *dst = keys1;
    for (long long width = 1; width < n_chunk; width <<= 1) {
        const int last = 2 * width >= n_chunk ? 1 : 0;
        hipLaunchKernelGGL(above_merge_kernel, dim3((unsigned)(batch * n_chunk * ABOVE_TILES_PER_CHUNK)), dim3(ABOVE_THREADS), 0, s,
                           score, n_cand, n_chunk, width, offs, (const u64 *)src, dst, ids_out, scores_out, last);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
        u64 *swap = src;
        src = dst;
        dst = swap;
    }
    return hipSuccess;
}

}  // namespace ultra

// Layout: offsets (batch * chunks + 1) int64 | key buffer 0, key buffer 1 (batch * n_cand) uint64 each | counts (batch * chunks, 2) int32.
extern "C" int64_t ultra_filtered_above_workspace(int64_t batch, int64_t n_cand) {
    if (batch < 0 || batch > ultra::ABOVE_MAX_BATCH || n_cand < 0 || n_cand >= (int64_t)1 << 31) return -1;
    const int64_t slots = batch * ultra::above_chunks(n_cand);
    return (slots + 1) * 8 + 2 * batch * n_cand * 8 + slots * 8;
}

// The three entries: `who` names the caller in the messages; n_live == NULL: every slot is a candidate; retired_bits == NULL: no
// id is retired.
static int32_t filtered_above_impl(const char *who_, const void *score, const int64_t *known_ptr, const int64_t *known_index,
                                   int64_t batch, int64_t n_cand, float threshold, int64_t *ptr_out, int64_t *ids_out,
                                   void *scores_out, int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes,
                                   const int64_t *n_live, const uint32_t *retired_bits, void *stream) {
    const std::string who(who_);
    if (n_cand >= (int64_t)1 << 31 || std::isnan(threshold) || (std::isinf(threshold) && threshold > 0)) {      // (before any pointer is looked at)
        ultra::set_error(who + ": n_cand must stay below 2^31 and the threshold be finite or -inf");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (!score || !ptr_out || !ids_out || !scores_out || !size_out || n_cand <= 0 || batch < 0 || batch > ultra::ABOVE_MAX_BATCH) {
        ultra::set_error(who + ": NULL operand, empty candidate set or batch outside [0, 65535]");
        return ULTRA_ERR_INVALID;
    }
    if (capacity < batch * n_cand) {
        ultra::set_error(who + ": capacity " + std::to_string(capacity) + " is below batch * n_cand = " +
                         std::to_string(batch * n_cand));
        return ULTRA_ERR_INVALID;
    }
    const int64_t need = ultra_filtered_above_workspace(batch, n_cand);
    if (workspace_bytes < need || !workspace || ((uintptr_t)workspace & 7u) != 0) {
        ultra::set_error(who + ": workspace of " + std::to_string(workspace_bytes) + " bytes, needs " +
                         std::to_string(need) + " (8-byte aligned)");
        return ULTRA_ERR_INVALID;
    }
    const int64_t n_chunk = ultra::above_chunks(n_cand);
    const int64_t slots = batch * n_chunk;
    if (slots * ultra::ABOVE_TILES_PER_CHUNK >= (int64_t)1 << 31) {
        ultra::set_error(who + ": batch * chunks per row must stay below 2^30");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch == 0) return ULTRA_OK;
    long long *offs = (long long *)workspace;
    ultra::u64 *keys0 = (ultra::u64 *)(offs + slots + 1), *keys1 = keys0 + batch * n_cand;
    int *counts = (int *)(keys1 + batch * n_cand);
    ULTRA_DEVICE_SCOPE(stream, score);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    const dim3 threads(ultra::ABOVE_THREADS);
    hipLaunchKernelGGL(ultra::above_count_kernel, dim3((unsigned)slots), threads, 0, s, (const float *)score, known_ptr, known_index,
                       (long long)n_cand, (long long)n_chunk, threshold, counts, n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("above_count_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    if (ultra::launch_above_scan(counts, batch, n_chunk, offs, ptr_out, size_out, s) != hipSuccess) {
        ultra::set_error("above_scan_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    hipLaunchKernelGGL(ultra::above_fill_kernel, dim3((unsigned)slots), threads, 0, s, (const float *)score, known_ptr, known_index,
                       (long long)n_cand, (long long)n_chunk, threshold, (const long long *)offs, keys0, ids_out,
                       (unsigned *)scores_out, n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("above_fill_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    if (ultra::launch_above_merges((const float *)score, n_cand, batch, n_chunk, offs, keys0, keys1, ids_out, (unsigned *)scores_out,
                                   s) != hipSuccess) {
        ultra::set_error("above_merge_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

extern "C" int32_t ultra_filtered_above(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                        int64_t n_cand, float threshold, int64_t *ptr_out, int64_t *ids_out, void *scores_out,
                                        int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes,
                                        void *stream) {
    return filtered_above_impl("ultra_filtered_above", score, known_ptr, known_index, batch, n_cand, threshold, ptr_out, ids_out,
                               scores_out, capacity, size_out, workspace, workspace_bytes, nullptr, nullptr, stream);
}

extern "C" int32_t ultra_filtered_above_live(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                             int64_t n_cand, float threshold, int64_t *ptr_out, int64_t *ids_out, void *scores_out,
                                             int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes,
                                             const int64_t *n_live, void *stream) {
    // (the parent's UNSUPPORTED cases come first)
    if (!n_live && n_cand < (int64_t)1 << 31 && !std::isnan(threshold) && !(std::isinf(threshold) && threshold > 0)) {
        ultra::set_error("ultra_filtered_above_live: n_live is NULL");
        return ULTRA_ERR_INVALID;
    }
    return filtered_above_impl("ultra_filtered_above_live", score, known_ptr, known_index, batch, n_cand, threshold, ptr_out, ids_out,
                               scores_out, capacity, size_out, workspace, workspace_bytes, n_live, nullptr, stream);
}

// (n_retired is part of the contract of the three _alive entries; the answer sets have no count that needs it)
extern "C" int32_t ultra_filtered_above_alive(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                              int64_t n_cand, float threshold, int64_t *ptr_out, int64_t *ids_out, void *scores_out,
                                              int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes,
                                              const int64_t *n_live, const uint32_t *retired_bits, const int64_t *n_retired,
                                              void *stream) {
    // (the parent's UNSUPPORTED cases come first)
    if ((!retired_bits || !n_retired) && n_cand < (int64_t)1 << 31 && !std::isnan(threshold) &&
        !(std::isinf(threshold) && threshold > 0)) {
        ultra::set_error("ultra_filtered_above_alive: retired_bits or n_retired is NULL");
        return ULTRA_ERR_INVALID;
    }
    return filtered_above_impl("ultra_filtered_above_alive", score, known_ptr, known_index, batch, n_cand, threshold, ptr_out,
                               ids_out, scores_out, capacity, size_out, workspace, workspace_bytes, n_live, retired_bits, stream);
}
