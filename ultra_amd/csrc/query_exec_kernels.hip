// Compiled execution of complex logical queries (include/ultra_nbfnet.h: ultra_query_segment, ultra_nonzero_lists,
// ultra_nonzero_lists_live, ultra_nonzero_lists_alive).
//
// ultra_query_segment: what a batch of UltraQuery stack machines does between two projection calls, as ONE launch.  The host
// has compiled the batch's postfix queries into a program (ultra_amd/query_exec.py): per sample the depth of its stack on
// entry, a row of the previous projection's output to push first, a list of micro-ops (push the one-hot set of an entity,
// AND, OR, NOT) and a row of the next projection's input to pop the top into.  The stacks are two fuzzy sets deep, so both
// values of a sample live in registers across its whole micro-program: every element of a live slot is read once and every
// element of a changed slot is written once, whatever the number of micro-ops.  Element-wise: one workgroup column per
// sample (blockIdx.y), the micro-ops uniform per workgroup, 16-byte accesses where the rows allow, no LDS, no atomics.
// blockIdx.z selects the neural or the symbolic stack: both run the same program.
//
// The arithmetic follows the torch expressions of ultraquery._LOGICS operation for operation (no contraction), so the
// compiled route gives the bits of the interpreter.
//
// ultra_nonzero_lists: the non-zero ids of every row of a matrix as ragged ascending lists -- the known-answer layout of
// ultra_filtered_topk, built from the final symbolic sets without a host round trip.  Two launches: counts per row; then per
// row a sum of the counts before it and an ordered compaction (block scan per tile of the row).  No atomics.
//
// ultra_nonzero_lists_live: the same two kernels over the LIVE prefix of rows of n slots -- a graph served with
// reserved rows, whose dead slots hold 1.0 after a negation and must not be listed as entailed answers.
//   Work split     one workgroup of 256 threads per row in both kernels, as in the parent: the grid, `counts` and `ptr_out`
//                  depend on (batch, n) alone, so a recorded launch serves every later live count.
//   Live count     one uniform 8-byte load of *n_live per workgroup (a scalar load: the pointer is a kernel argument), clamped
//                  to [0, n]; it replaces n as the bound of the count loop, of the tile loop and of the per-id test.  The row
//                  stride stays n.  The clamped value bounds loops only and is never an index; an id at or beyond it is never
//                  loaded, so whatever a dead slot holds (1.0, NaN) reaches neither a count nor a list.
//   Memory         every live element is read twice (count, fill), 4-byte loads coalesced across the workgroup (count) or 16
//                  consecutive bytes per thread (fill); each listed id is one 8-byte store.  At serving sizes (16 x 14,541
//                  fp32 = 0.9 MB) both launches are latency-bound, not bandwidth-bound.
//   LDS / sync     four wave totals (32 B) and four wave counts (16 B); two barriers per tile.  No atomics, no memset node:
//                  for batch == 0 a one-thread kernel writes ptr_out[0] (a captured memset replays wrongly between eager
//                  work).
//   Registers      count 11 VGPRs / 20 SGPRs, fill 32 VGPRs / 48 SGPRs (four hit flags, two 64-bit cursors), no scratch, 8 waves a
//                  SIMD allowed: occupancy is bounded by the grid (one workgroup a row), not by registers.
// The parent passes n_live == NULL -- every slot is live -- and keeps its results bit for bit.
//
// ultra_nonzero_lists_alive: the same two kernels with one more operand, the RETIRED bitmap of a graph that took
// entities out (id v is bit v & 31 of word v >> 5: live.retired_words, the words the ultra_filtered_*_alive entries read).  An id
// whose bit is set is left out of the count and of the list, whatever its slot holds (1.0 after a negation, NaN, +inf).
//   Work split     unchanged: one workgroup of 256 threads per row; the grid, `counts` and `ptr_out` depend on (batch, n) alone
//                  and the bitmap is read at run time, so a recorded launch serves every later retirement.
//   Mask word      count: the thread that tests id i loads word i >> 5 -- 32 neighbouring lanes read the same 4 bytes, two
//                  words a wave.  fill: a thread's four ids start at a multiple of 4 and lie in one word, so one word load per
//                  thread per tile (a tile starts at a multiple of 1024 and covers 32 whole words; eight lanes share a word).
//                  The word load is issued BESIDE the value loads -- ahead of them in program order, looked at after them,
//                  unconditional inside a loop body that is chosen once per workgroup (retired_bits != NULL is the same in
//                  every thread) -- not inside a branch of the loop: there the compiler waited for the word before it issued
//                  the value load (§28 measured that at twice the cost).  Plain loads.  A word is loaded only by a thread
//                  whose first id lies below the clamped live count, and the bit of an id at or beyond it is never looked at
//                  (the per-id bound comes first).  retired_bits == NULL: the loop bodies of before, word 0 folded away --
//                  the twin and the parent, the same bits.
//   Retired slot   its value may be loaded but reaches neither a count nor a list: the bit is ANDed in after the comparison.
//   LDS / sync     as above: 32 B + 16 B, two barriers per tile; no atomics, no memset node (batch == 0: the one-thread kernel).
//   Registers      the compiler's resource report of the gfx950 build, both loop bodies in each kernel: count 13 VGPRs / 24
//                  SGPRs, fill 40 VGPRs / 60 SGPRs (the report's totals, VCC and the reserved pairs included; they replace
//                  the figures above, which were those of the kernels with one body), 0 bytes of scratch and no spill in
//                  either, 8 waves a SIMD allowed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"

#pragma clang fp contract(off)

namespace ultra {

constexpr int QSEG_THREADS = 256;
constexpr int QSEG_GRID_CAP = 256;      // workgroups per row; longer rows go round the grid-stride loop
constexpr int QOP_AND = -1, QOP_OR = -2, QOP_NOT = -3;

struct QuerySegmentArgs {
    const int32_t *entry_depth, *push_row, *pop_row, *op_ptr, *ops;
    long long num_node, push_rows, pop_rows;
    float *stack[2];
    const float *push_src[2];
    float *pop_dst[2];
};

// torch.min / torch.max and clamp hand a NaN on from either operand
template <int LOGIC> __device__ __forceinline__ float fuzzy_and(float x, float y) {
    if (LOGIC == 0) return x * y;
    if (LOGIC == 1) return (x != x || y != y) ? x + y : (y < x ? y : x);
    const float t = (x + y) - 1.0f;
    return t < 0.0f ? 0.0f : t;
}

template <int LOGIC> __device__ __forceinline__ float fuzzy_or(float x, float y) {
    if (LOGIC == 0) {
        const float s = x + y, p = x * y;
        return s - p;
    }
    if (LOGIC == 1) return (x != x || y != y) ? x + y : (y > x ? y : x);
    const float t = x + y;
    return t > 1.0f ? 1.0f : t;
}

template <int W> struct Lanes {
    float v[W];
};

template <int W> __device__ __forceinline__ Lanes<W> load_lanes(const float *p) {
    Lanes<W> r;
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int W> __device__ __forceinline__ void store_lanes(float *p, const Lanes<W> &r) {
    if constexpr (W == 4)
        *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else
        *p = r.v[0];
}

// W = 4: num_node % 4 == 0 and every base pointer 16-byte aligned (decided on the host), else W = 1.
template <int LOGIC, int W> __global__ void __launch_bounds__(QSEG_THREADS) query_segment_kernel(QuerySegmentArgs a) {
    const long long b = blockIdx.y;
    const int z = blockIdx.z;
    // (all of these are the same in every thread of the workgroup)
    const int d0 = a.entry_depth[b];
    long long push_row = a.push_row[b], pop_row = a.pop_row[b];
    const int o0 = a.op_ptr[b], o1 = a.op_ptr[b + 1];
    const float *push_src = a.push_src[z];
    float *pop_dst = a.pop_dst[z];
    if (!push_src || push_row >= a.push_rows) push_row = -1;        // (a program the host compiler made never gets here)
    if (!pop_dst || pop_row >= a.pop_rows) pop_row = -1;
    if ((push_row < 0 && o0 == o1 && pop_row < 0) || d0 < 0 || d0 > 2) return;
    const long long n = a.num_node;
    float *slot0 = a.stack[z] + b * 2 * n, *slot1 = slot0 + n;
    const long long stride = (long long)gridDim.x * QSEG_THREADS * W;
    for (long long i = ((long long)blockIdx.x * QSEG_THREADS + threadIdx.x) * W; i < n; i += stride) {
        Lanes<W> s0, s1;
#pragma unroll
        for (int j = 0; j < W; ++j) s0.v[j] = s1.v[j] = 0.0f;
        int d = d0;
        unsigned dirty = 0;
        if (d0 >= 1) s0 = load_lanes<W>(slot0 + i);
        if (d0 >= 2) s1 = load_lanes<W>(slot1 + i);
        if (push_row >= 0 && d < 2) {
            const Lanes<W> v = load_lanes<W>(push_src + push_row * n + i);
            if (d == 0) s0 = v; else s1 = v;
            dirty |= 1u << d;
            ++d;
        }
        for (int o = o0; o < o1; ++o) {
            const int op = a.ops[o];
            if (op >= 0) {
                if (d < 2) {
                    Lanes<W> v;
#pragma unroll
                    for (int j = 0; j < W; ++j) v.v[j] = (i + j == (long long)op) ? 1.0f : 0.0f;
                    if (d == 0) s0 = v; else s1 = v;
                    dirty |= 1u << d;
                    ++d;
                }
            } else if (op == QOP_NOT) {
                if (d == 1) {
#pragma unroll
                    for (int j = 0; j < W; ++j) s0.v[j] = 1.0f - s0.v[j];
                    dirty |= 1u;
                } else if (d == 2) {
#pragma unroll
                    for (int j = 0; j < W; ++j) s1.v[j] = 1.0f - s1.v[j];
                    dirty |= 2u;
                }
            } else if (d == 2 && (op == QOP_AND || op == QOP_OR)) {
                if (op == QOP_AND) {
#pragma unroll
                    for (int j = 0; j < W; ++j) s0.v[j] = fuzzy_and<LOGIC>(s0.v[j], s1.v[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < W; ++j) s0.v[j] = fuzzy_or<LOGIC>(s0.v[j], s1.v[j]);
                }
                dirty |= 1u;
                d = 1;
            }
        }
        if (pop_row >= 0 && d >= 1) {
            store_lanes<W>(pop_dst + pop_row * n + i, d == 1 ? s0 : s1);
            --d;
        }
        if (d >= 1 && (dirty & 1u)) store_lanes<W>(slot0 + i, s0);
        if (d >= 2 && (dirty & 2u)) store_lanes<W>(slot1 + i, s1);
    }
}

template <int LOGIC> static void launch_query_segment(const QuerySegmentArgs &a, bool vec, dim3 grid, hipStream_t s) {
    if (vec)
        hipLaunchKernelGGL((query_segment_kernel<LOGIC, 4>), grid, dim3(QSEG_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((query_segment_kernel<LOGIC, 1>), grid, dim3(QSEG_THREADS), 0, s, a);
}

constexpr int NZ_THREADS = 256;
constexpr int NZ_PER_THREAD = 4;
constexpr int NZ_TILE = NZ_THREADS * NZ_PER_THREAD;

// NaN != 0 holds, -0.0 != 0 does not: the rule of ultra_traversal_dropout
__device__ __forceinline__ bool is_nonzero(float v) { return v != 0.0f; }

// the sum of v over the workgroup, in every thread; ends with a barrier
__device__ __forceinline__ long long block_sum(long long v, long long *wave_total) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_total[wave] = v;
    __syncthreads();
    long long total = 0;
    for (int w = 0; w < NZ_THREADS / 64; ++w) total += wave_total[w];
    __syncthreads();
    return total;
}

// The live ids of a row of n slots: *n_live clamped to [0, n]; NULL: every slot (the rule of csrc/topk_kernels.hip).
__device__ __forceinline__ long long nonzero_live(const int64_t *__restrict__ n_live, long long n) {
    if (!n_live) return n;
    const long long v = *n_live;
    return v < 0 ? 0 : (v < n ? v : n);
}

// Is the bit of id v (v & 31) clear in the mask word that covers it?  (word 0: nothing is retired)
__device__ __forceinline__ bool nonzero_alive(unsigned word, long long v) { return ((word >> (unsigned)(v & 31)) & 1u) == 0u; }

// The non-zero ids of one row below `live` that this thread tests: i = tid, tid + 256, ...  MASKED: the mask word of id i ahead
// of its value in program order and looked at after it -- both loads unconditional, so they are in flight together.  The branch
// on retired_bits is taken once, outside the loop (inside it the word was waited for before the value load was issued).
template <bool MASKED> __device__ __forceinline__ long long nonzero_count_row(const float *__restrict__ row, long long live,
                                                                             const uint32_t *__restrict__ retired_bits) {
    long long c = 0;
    for (long long i = threadIdx.x; i < live; i += NZ_THREADS) {
        unsigned word = 0u;
        if (MASKED) word = retired_bits[i >> 5];        // (i < live <= n: a word of the bitmap)
        const float v = row[i];
        c += is_nonzero(v) && nonzero_alive(word, i) ? 1 : 0;
    }
    return c;
}

__global__ void __launch_bounds__(NZ_THREADS) nonzero_count_kernel(const float *__restrict__ x, long long n, int64_t *__restrict__ counts,
                                                                   const int64_t *__restrict__ n_live,
                                                                   const uint32_t *__restrict__ retired_bits) {
    __shared__ long long wave_total[NZ_THREADS / 64];
    const float *row = x + (long long)blockIdx.x * n;
    const long long live = nonzero_live(n_live, n);
    long long c = retired_bits ? nonzero_count_row<true>(row, live, retired_bits) : nonzero_count_row<false>(row, live, nullptr);
    c = block_sum(c, wave_total);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// The ordered compaction of one row's live ids into index_out from `at` on, tile by tile.  MASKED: one mask word per thread per
// tile -- its four ids start at a multiple of 4 and lie in one word -- issued ahead of the values and looked at after them; a
// thread whose first id is not live loads none.
template <bool MASKED> __device__ __forceinline__ void nonzero_fill_row(const float *__restrict__ row, long long live, long long at,
                                                                        int64_t *__restrict__ index_out,
                                                                        const uint32_t *__restrict__ retired_bits, int *wave_count) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long lo = 0; lo < live; lo += NZ_TILE) {
        // thread t owns NZ_PER_THREAD consecutive ids: the order of the ids is the order of (thread, slot)
        const long long first = lo + (long long)tid * NZ_PER_THREAD;
        unsigned word = 0u;
        if (MASKED && first < live) word = retired_bits[first >> 5];
        bool hit[NZ_PER_THREAD];
        int mine = 0;
#pragma unroll
        for (int j = 0; j < NZ_PER_THREAD; ++j) {
            hit[j] = first + j < live && is_nonzero(row[first + j]) && nonzero_alive(word, first + j);
            mine += hit[j] ? 1 : 0;
        }
        int incl = mine;
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_count[wave] = incl;
        __syncthreads();
        int wave_before = 0, tile_total = 0;
        for (int w = 0; w < NZ_THREADS / 64; ++w) {
            wave_before += w < wave ? wave_count[w] : 0;
            tile_total += wave_count[w];
        }
        long long out = at + wave_before + (incl - mine);
#pragma unroll
        for (int j = 0; j < NZ_PER_THREAD; ++j)
            if (hit[j]) index_out[out++] = first + j;
        at += tile_total;
        __syncthreads();        // (wave_count is rewritten by the next tile)
    }
}

__global__ void __launch_bounds__(NZ_THREADS) nonzero_fill_kernel(const float *__restrict__ x, long long n, const int64_t *__restrict__ counts,
                                                                  int64_t *__restrict__ ptr_out, int64_t *__restrict__ index_out,
                                                                  const int64_t *__restrict__ n_live,
                                                                  const uint32_t *__restrict__ retired_bits) {
    __shared__ long long wave_total[NZ_THREADS / 64];
    __shared__ int wave_count[NZ_THREADS / 64];
    const long long b = blockIdx.x;
    const long long live = nonzero_live(n_live, n);
    const int tid = threadIdx.x;
    long long before = 0;
    for (long long r = tid; r < b; r += NZ_THREADS) before += counts[r];
    const long long at = block_sum(before, wave_total);       // where this row's list starts
    if (tid == 0) {
        if (b == 0) ptr_out[0] = 0;
        ptr_out[b + 1] = at + counts[b];
    }
    const float *row = x + b * n;
    if (retired_bits)       // (the same in every thread)
        nonzero_fill_row<true>(row, live, at, index_out, retired_bits, wave_count);
    else
        nonzero_fill_row<false>(row, live, at, index_out, nullptr, wave_count);
}

// ptr_out of an empty batch, without a memset node
__global__ void nonzero_empty_kernel(int64_t *__restrict__ ptr_out) { ptr_out[0] = 0; }

}  // namespace ultra

extern "C" int32_t ultra_query_segment(const int32_t *entry_depth, const int32_t *push_row, const int32_t *pop_row,
                                       const int32_t *op_ptr, const int32_t *ops, int64_t batch, int64_t num_node,
                                       int32_t stack_depth, int32_t dtype, int32_t logic, void *stack, const void *push_src,
                                       int64_t push_rows, void *pop_dst, int64_t pop_rows, void *sym_stack,
                                       const void *sym_push_src, void *sym_pop_dst, void *stream) {
    if (stack_depth != 2 || dtype != 0 || num_node >= (int64_t)1 << 31) {      // (before any pointer is looked at)
        ultra::set_error("ultra_query_segment: stacks of depth 2, fp32 and num_node below 2^31 only");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch < 0 || batch > 65535 || num_node <= 0 || logic < 0 || logic > 2) {
        ultra::set_error("ultra_query_segment: batch must lie in [0, 65535], num_node be positive and logic in [0, 2]");
        return ULTRA_ERR_INVALID;
    }
    if (!entry_depth || !push_row || !pop_row || !op_ptr || !ops || !stack) {
        ultra::set_error("ultra_query_segment: NULL program array or stack");
        return ULTRA_ERR_INVALID;
    }
    if ((push_src != nullptr) != (push_rows > 0) || (pop_dst != nullptr) != (pop_rows > 0)) {
        ultra::set_error("ultra_query_segment: push_src / pop_dst and their row counts disagree");
        return ULTRA_ERR_INVALID;
    }
    if (sym_stack ? ((sym_push_src != nullptr) != (push_src != nullptr) || (sym_pop_dst != nullptr) != (pop_dst != nullptr))
                  : (sym_push_src != nullptr || sym_pop_dst != nullptr)) {
        ultra::set_error("ultra_query_segment: the symbolic stack takes the same buffers as the neural one, or none");
        return ULTRA_ERR_INVALID;
    }
    if (batch == 0) return ULTRA_OK;
    ULTRA_DEVICE_SCOPE(stream, stack);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ultra::QuerySegmentArgs a;
    a.entry_depth = entry_depth, a.push_row = push_row, a.pop_row = pop_row, a.op_ptr = op_ptr, a.ops = ops;
    a.num_node = num_node, a.push_rows = push_rows, a.pop_rows = pop_rows;
    a.stack[0] = (float *)stack, a.stack[1] = (float *)sym_stack;
    a.push_src[0] = (const float *)push_src, a.push_src[1] = (const float *)sym_push_src;
    a.pop_dst[0] = (float *)pop_dst, a.pop_dst[1] = (float *)sym_pop_dst;
    uintptr_t low = 0;
    for (int z = 0; z < 2; ++z) low |= (uintptr_t)a.stack[z] | (uintptr_t)a.push_src[z] | (uintptr_t)a.pop_dst[z];
    const bool vec = num_node % 4 == 0 && (low & 15u) == 0;
    const int64_t per_block = (int64_t)ultra::QSEG_THREADS * (vec ? 4 : 1);
    int64_t gx = (num_node + per_block - 1) / per_block;
    if (gx > ultra::QSEG_GRID_CAP) gx = ultra::QSEG_GRID_CAP;
    const dim3 grid((unsigned)gx, (unsigned)batch, sym_stack ? 2u : 1u);
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    if (logic == 0) ultra::launch_query_segment<0>(a, vec, grid, s);
    else if (logic == 1) ultra::launch_query_segment<1>(a, vec, grid, s);
    else ultra::launch_query_segment<2>(a, vec, grid, s);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("query_segment_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

// The three entries: `who` names the caller in the messages; n_live == NULL: every slot is live (the parent, and _alive on a
// graph without a reserve); retired_bits == NULL: no id is retired (the parent and the _live twin).
enum { NZ_PARENT = 0, NZ_LIVE = 1, NZ_ALIVE = 2 };
static int32_t nonzero_lists_impl(const char *who, int entry, const void *x, int64_t batch, int64_t n, int64_t *counts,
                                  int64_t *ptr_out, int64_t *index_out, int64_t capacity, const int64_t *n_live,
                                  const uint32_t *retired_bits, void *stream) {
    const std::string name(who);
    if (n >= (int64_t)1 << 31 || batch >= (int64_t)1 << 31) {
        ultra::set_error(name + ": batch and n must stay below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (entry == NZ_LIVE && !n_live) {
        ultra::set_error(name + ": n_live is NULL");
        return ULTRA_ERR_INVALID;
    }
    if (entry == NZ_ALIVE && !retired_bits) {
        ultra::set_error(name + ": retired_bits is NULL");
        return ULTRA_ERR_INVALID;
    }
    if (!ptr_out || batch < 0 || n < 0 || (batch > 0 && (!counts || (n > 0 && (!x || !index_out))))) {
        ultra::set_error(name + ": NULL operand or negative size");
        return ULTRA_ERR_INVALID;
    }
    if (capacity < batch * n) {
        ultra::set_error(name + ": index_out holds " + std::to_string(capacity) + " ids, a full matrix has " +
                         std::to_string(batch * n));
        return ULTRA_ERR_INVALID;
    }
    ULTRA_DEVICE_SCOPE(stream, ptr_out);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (batch == 0) {       // ptr_out = [0]
        if (entry != NZ_PARENT) {
            hipLaunchKernelGGL(ultra::nonzero_empty_kernel, dim3(1), dim3(1), 0, s, ptr_out);
            if (hipGetLastError() != hipSuccess) {
                ultra::set_error("nonzero_empty_kernel launch failed");
                return ULTRA_ERR_HIP;
            }
        } else if (hipMemsetAsync(ptr_out, 0, sizeof(int64_t), s) != hipSuccess) {
            ultra::set_error(name + ": could not clear ptr_out");
            return ULTRA_ERR_HIP;
        }
        return ULTRA_OK;
    }
    hipLaunchKernelGGL(ultra::nonzero_count_kernel, dim3((unsigned)batch), dim3(ultra::NZ_THREADS), 0, s, (const float *)x,
                       (long long)n, counts, n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("nonzero_count_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    hipLaunchKernelGGL(ultra::nonzero_fill_kernel, dim3((unsigned)batch), dim3(ultra::NZ_THREADS), 0, s, (const float *)x,
                       (long long)n, (const int64_t *)counts, ptr_out, index_out, n_live, retired_bits);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("nonzero_fill_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

extern "C" int32_t ultra_nonzero_lists(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out,
                                       int64_t *index_out, int64_t capacity, void *stream) {
    return nonzero_lists_impl("ultra_nonzero_lists", NZ_PARENT, x, batch, n, counts, ptr_out, index_out, capacity, nullptr, nullptr,
                              stream);
}

extern "C" int32_t ultra_nonzero_lists_live(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out,
                                            int64_t *index_out, int64_t capacity, const int64_t *n_live, void *stream) {
    return nonzero_lists_impl("ultra_nonzero_lists_live", NZ_LIVE, x, batch, n, counts, ptr_out, index_out, capacity, n_live,
                              nullptr, stream);
}

extern "C" int32_t ultra_nonzero_lists_alive(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out,
                                             int64_t *index_out, int64_t capacity, const int64_t *n_live,
                                             const uint32_t *retired_bits, void *stream) {
    return nonzero_lists_impl("ultra_nonzero_lists_alive", NZ_ALIVE, x, batch, n, counts, ptr_out, index_out, capacity, n_live,
                              retired_bits, stream);
}
