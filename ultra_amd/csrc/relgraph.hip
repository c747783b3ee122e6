// Relation graph of a knowledge graph on the GPU (reference: /root/reference/ultra/tasks.py:144-199).
//
// Nodes of the relation graph are the relation ids; an edge r1 -> r2 of type hh / tt / ht / th exists iff some entity is
// a head (h) or tail (t) of an r1 edge and of an r2 edge respectively.  The reference forms four sparse products
// E^T E over (entity, relation) incidence matrices and keeps only their sparsity pattern (tasks.py:186-189) -- 5.9 s on
// the CPU at FB15k237 shape.  Here the pattern is built as bit matrices:
//   1. incidence_bits_kernel : H[n] / T[n] = bit set of the relations entity n is head / tail of        (one atomicOr per edge)
//   2. pair_mark_kernel      : for every entity, every relation r1 in H[n]: A_hh[r1] |= H[n], A_ht[r1] |= T[n];
//                              every r1 in T[n]: A_tt[r1] |= T[n], A_th[r1] |= H[n]                       (word-wide ORs, skipped
//                              when the row already holds the bits)
//   3. row_count_kernel / emit_edges_kernel : popcounts per (type, row), then the edge list in the reference's order --
//      the hh, tt, ht, th blocks one after the other, each sorted by (row, col) -- so that the result equals the
//      reference's relation_graph.edge_index / edge_type element for element;
//   4. dense_order_adjacency_kernel : the same bit matrices as the byte adjacency of the reference-order layer kernel
//      (dense_order_layer.hip, plan.hpp `a_ex`): plan format straight from the device, no edge list in between.
//   5. add_edges_*_kernel : the bit sets of 1. and 2. kept RESIDENT and brought up to date for appended edges -- the relation graph
//      is monotone under additions -- at the cost of those edges and their endpoints' bit sets (ultra_relation_graph_add_edges).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "plan.hpp"
#include "device_scope.hpp"

namespace ultra {

// KEEP: only the edges with keep[e] != 0 count (the relation graph of a graph whose other edges are dropped)
template <bool KEEP>
__global__ void __launch_bounds__(256) incidence_bits_kernel(const int64_t *__restrict__ edge_index, const int64_t *__restrict__ edge_type,
                                                             long long num_edge, int words, uint32_t *__restrict__ hbits,
                                                             uint32_t *__restrict__ tbits, const float *__restrict__ keep) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < num_edge; e += (long long)gridDim.x * blockDim.x) {
        if (KEEP && keep[e] == 0.f) continue;
        const long long h = edge_index[e], t = edge_index[num_edge + e], r = edge_type[e];
        const uint32_t bit = 1u << (r & 31);
        uint32_t *hw = hbits + h * words + (r >> 5), *tw = tbits + t * words + (r >> 5);
        if (!(*hw & bit)) atomicOr(hw, bit);
        if (!(*tw & bit)) atomicOr(tw, bit);
    }
}

// row word |= bits, skipped where the row already holds them.  TRACK: did this lane add a bit -- read off the atomic's old value,
// so a bit another wave set first is not counted
template <bool TRACK>
__device__ __forceinline__ bool or_into(uint32_t *word, uint32_t bits) {
    if (!(bits & ~*word)) return false;
    if (!TRACK) {
        atomicOr(word, bits);
        return false;
    }
    return (bits & ~atomicOr(word, bits)) != 0;
}

// the whole pair marking of entity n by one wave; lane w owns word w (+ 64, ...) of the relation bit sets.  TRACK: returns whether
// this lane added a bit to adj
template <bool TRACK>
__device__ __forceinline__ bool mark_entity_pairs(const uint32_t *__restrict__ hbits, const uint32_t *__restrict__ tbits, long long n,
                                                  int lane, int words, size_t mat, uint32_t *__restrict__ adj) {
    bool added = false;
    for (int w0 = 0; w0 < words; w0 += 64) {           // the words this lane ORs into the rows
        const int w = w0 + lane;
        const uint32_t hv = w < words ? hbits[n * words + w] : 0u, tv = w < words ? tbits[n * words + w] : 0u;
        for (int s = 0; s < words; ++s) {              // the relations (rows) of this entity, word by word (wave-uniform)
            uint32_t hs = hbits[n * words + s], ts = tbits[n * words + s];
            while (hs) {
                const int r1 = 32 * s + __builtin_ctz(hs);
                hs &= hs - 1;
                if (w < words) {
                    uint32_t *a = adj + 0 * mat + (size_t)r1 * words + w, *b = adj + 2 * mat + (size_t)r1 * words + w;
                    added |= or_into<TRACK>(a, hv);     // hh
                    added |= or_into<TRACK>(b, tv);     // ht
                }
            }
            while (ts) {
                const int r1 = 32 * s + __builtin_ctz(ts);
                ts &= ts - 1;
                if (w < words) {
                    uint32_t *a = adj + 1 * mat + (size_t)r1 * words + w, *b = adj + 3 * mat + (size_t)r1 * words + w;
                    added |= or_into<TRACK>(a, tv);     // tt
                    added |= or_into<TRACK>(b, hv);     // th
                }
            }
        }
    }
    return added;
}

// one wave per entity
__global__ void __launch_bounds__(256) pair_mark_kernel(const uint32_t *__restrict__ hbits, const uint32_t *__restrict__ tbits,
                                                        long long num_node, int num_rel, int words, uint32_t *__restrict__ adj) {
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6, nwave = ((long long)gridDim.x * blockDim.x) >> 6;
    const size_t mat = (size_t)num_rel * words;    // words per type matrix; adj = [hh | tt | ht | th]
    for (long long n = wave; n < num_node; n += nwave) mark_entity_pairs<false>(hbits, tbits, n, lane, words, mat, adj);
}

// ---- edges added to resident bit sets (ultra_relation_graph_add_edges) ----
// status word: bit 0 = a bit was added to adj, bit 1 = an index lies outside the graph (then nothing is marked)
constexpr int32_t ADD_CHANGED = 1, ADD_OUT_OF_RANGE = 2;

// one block: every index is looked at before anything is marked, and the status word is written whole (no zeroing by the caller)
__global__ void __launch_bounds__(1024) add_edges_check_kernel(const int64_t *__restrict__ edge_index, const int64_t *__restrict__ edge_type,
                                                               long long num_edge, long long num_node, long long num_rel,
                                                               int32_t *__restrict__ status) {
    int bad = 0;
    for (long long e = threadIdx.x; e < num_edge; e += blockDim.x) {
        const long long h = edge_index[e], t = edge_index[num_edge + e], r = edge_type[e];
        bad |= h < 0 || h >= num_node || t < 0 || t >= num_node || r < 0 || r >= num_rel;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) *status = bad ? ADD_OUT_OF_RANGE : 0;
}

// incidence_bits_kernel for the added edges, behind the check
__global__ void __launch_bounds__(256) add_edges_incidence_kernel(const int64_t *__restrict__ edge_index, const int64_t *__restrict__ edge_type,
                                                                  long long num_edge, int words, uint32_t *__restrict__ hbits,
                                                                  uint32_t *__restrict__ tbits, const int32_t *__restrict__ status) {
    if (*status & ADD_OUT_OF_RANGE) return;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < num_edge; e += (long long)gridDim.x * blockDim.x) {
        const long long h = edge_index[e], t = edge_index[num_edge + e], r = edge_type[e];
        const uint32_t bit = 1u << (r & 31);
        uint32_t *hw = hbits + h * words + (r >> 5), *tw = tbits + t * words + (r >> 5);
        if (!(*hw & bit)) atomicOr(hw, bit);
        if (!(*tw & bit)) atomicOr(tw, bit);
    }
}

// one wave per listed endpoint (the 2 num_edge entries of edge_index): the pair marking of pair_mark_kernel for that entity.  A
// repeated endpoint repeats idempotent ORs.  `status` is read for bit 1 only, which no wave of this launch writes.
__global__ void __launch_bounds__(256) add_edges_pair_kernel(const int64_t *__restrict__ edge_index, long long num_endpoint,
                                                             const uint32_t *__restrict__ hbits, const uint32_t *__restrict__ tbits,
                                                             int num_rel, int words, uint32_t *__restrict__ adj, int32_t *status) {
    if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ADD_OUT_OF_RANGE) return;
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6, nwave = ((long long)gridDim.x * blockDim.x) >> 6;
    const size_t mat = (size_t)num_rel * words;
    bool added = false;
    for (long long i = wave; i < num_endpoint; i += nwave)
        added |= mark_entity_pairs<true>(hbits, tbits, edge_index[i], lane, words, mat, adj);
    if (added) atomicOr(status, ADD_CHANGED);
}

__global__ void __launch_bounds__(256) row_count_kernel(const uint32_t *__restrict__ adj, int rows_total, int words,
                                                        int64_t *__restrict__ counts) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;     // (type, row) flattened
    if (r >= rows_total) return;
    long long c = 0;
    for (int w = 0; w < words; ++w) c += __builtin_popcount(adj[(size_t)r * words + w]);
    counts[r] = c;
}

// one 64-lane wave per (type, row): columns in ascending order
__global__ void __launch_bounds__(256) emit_edges_kernel(const uint32_t *__restrict__ adj, const int64_t *__restrict__ offsets,
                                                         int num_rel, int words, long long total, int64_t *__restrict__ edge_index,
                                                         int64_t *__restrict__ edge_type) {
    const int lane = threadIdx.x & 63;
    const int row_flat = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (row_flat >= 4 * num_rel) return;
    const int type = row_flat / num_rel, r1 = row_flat - type * num_rel;
    long long out = offsets[row_flat];
    for (int w0 = 0; w0 < words; w0 += 64) {
        const int w = w0 + lane;
        uint32_t v = w < words ? adj[(size_t)row_flat * words + w] : 0u;
        int c = __builtin_popcount(v), pre = c;     // inclusive prefix over the wave's 64 words
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(pre, off);
            if (lane >= off) pre += up;
        }
        long long pos = out + pre - c;
        while (v) {
            const int r2 = 32 * w + __builtin_ctz(v);
            v &= v - 1;
            edge_index[pos] = r1;
            edge_index[total + pos] = r2;
            edge_type[pos] = type;
            ++pos;
        }
        out += __shfl(pre, 63);
    }
}

// a_ex[row_tile16][col_chunk16][lane = (row % 16) + 16 type][col % 16]  (plan.hpp), one thread per 16-byte lane record
__global__ void __launch_bounds__(256) dense_order_adjacency_kernel(const uint32_t *__restrict__ adj, int num_rel, int words,
                                                                    uint4 *__restrict__ a_ex) {
    const int njc = (num_rel + 15) / 16, nrt = (num_rel + 15) / 16;
    const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (idx >= (long long)nrt * njc * 64) return;
    const int lane = (int)(idx & 63), jc = (int)((idx >> 6) % njc), rt = (int)((idx >> 6) / njc);
    const int row = 16 * rt + (lane & 15), type = lane >> 4;
    uint32_t half = 0;     // bits of columns 16 jc .. 16 jc + 15
    if (row < num_rel) half = (adj[((size_t)type * num_rel + row) * words + (jc >> 1)] >> (16 * (jc & 1))) & 0xffffu;
    uint32_t out[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        uint32_t wv = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) wv |= ((half >> (4 * q4 + b)) & 1u) << (8 * b);
        out[q4] = wv;
    }
    a_ex[idx] = make_uint4(out[0], out[1], out[2], out[3]);
}

// keep[i] = bit r2 of row r1 of matrix type[i], for the edges (r1, r2, type) of a relation graph: which of them a relation graph
// built from a subset of the entity edges still holds (it can only lose edges)
__global__ void __launch_bounds__(256) relation_edge_keep_kernel(const uint32_t *__restrict__ adj, int num_rel, int words,
                                                                 const int64_t *__restrict__ rel_edge_index,
                                                                 const int64_t *__restrict__ rel_edge_type, long long num_rel_edge,
                                                                 float *__restrict__ keep) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= num_rel_edge) return;
    const long long r1 = rel_edge_index[i], r2 = rel_edge_index[num_rel_edge + i], type = rel_edge_type[i];
    bool on = false;
    if (r1 >= 0 && r1 < num_rel && r2 >= 0 && r2 < num_rel && type >= 0 && type < 4)
        on = (adj[((size_t)type * num_rel + r1) * words + (r2 >> 5)] >> (r2 & 31)) & 1u;
    keep[i] = on ? 1.f : 0.f;
}

}  // namespace ultra

using namespace ultra;

static int32_t relation_graph_bits(const int64_t *edge_index_dev, const int64_t *edge_type_dev, const float *keep_dev, int64_t num_edge,
                                   int64_t num_node, int64_t num_relation, void *hbits_dev, void *tbits_dev, void *adj_dev,
                                   int64_t *row_counts_dev, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, edge_index_dev);
    if (num_edge < 0 || num_node < 0 || num_relation <= 0 || (num_edge > 0 && (!edge_index_dev || !edge_type_dev)) || !hbits_dev ||
        !tbits_dev || !adj_dev || !row_counts_dev) {
        set_error(keep_dev ? "ultra_relation_graph_bits_keep: bad argument" : "ultra_relation_graph_bits: bad argument");
        return ULTRA_ERR_INVALID;
    }
    if (num_relation > (1 << 20)) {
        set_error("ultra_relation_graph_bits: more than 2^20 relations are not supported");
        return ULTRA_ERR_UNSUPPORTED;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int words = (int)((num_relation + 31) / 32);
    (void)hipGetLastError();
    const dim3 grid((unsigned)std::min<int64_t>((num_edge + 255) / 256, 4096));
    if (num_edge > 0 && keep_dev)
        hipLaunchKernelGGL(incidence_bits_kernel<true>, grid, dim3(256), 0, s, edge_index_dev, edge_type_dev, (long long)num_edge, words,
                           (uint32_t *)hbits_dev, (uint32_t *)tbits_dev, keep_dev);
    else if (num_edge > 0)
        hipLaunchKernelGGL(incidence_bits_kernel<false>, grid, dim3(256), 0, s, edge_index_dev, edge_type_dev, (long long)num_edge, words,
                           (uint32_t *)hbits_dev, (uint32_t *)tbits_dev, nullptr);
    if (num_node > 0)
        hipLaunchKernelGGL(pair_mark_kernel, dim3((unsigned)std::min<int64_t>((num_node + 3) / 4, 8192)), dim3(256), 0, s,
                           (const uint32_t *)hbits_dev, (const uint32_t *)tbits_dev, (long long)num_node, (int)num_relation, words,
                           (uint32_t *)adj_dev);
    const int rows_total = (int)(4 * num_relation);
    hipLaunchKernelGGL(row_count_kernel, dim3((rows_total + 255) / 256), dim3(256), 0, s, (const uint32_t *)adj_dev, rows_total, words,
                       row_counts_dev);
    if (hipGetLastError() != hipSuccess) {
        set_error("relation-graph kernels: launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

extern "C" {

int32_t ultra_relation_graph_bits(const int64_t *edge_index_dev, const int64_t *edge_type_dev, int64_t num_edge, int64_t num_node,
                                  int64_t num_relation, void *hbits_dev, void *tbits_dev, void *adj_dev, int64_t *row_counts_dev,
                                  void *stream) {
    return relation_graph_bits(edge_index_dev, edge_type_dev, nullptr, num_edge, num_node, num_relation, hbits_dev, tbits_dev, adj_dev,
                               row_counts_dev, stream);
}

int32_t ultra_relation_graph_bits_keep(const int64_t *edge_index_dev, const int64_t *edge_type_dev, const float *keep_dev,
                                       int64_t num_edge, int64_t num_node, int64_t num_relation, void *hbits_dev, void *tbits_dev,
                                       void *adj_dev, int64_t *row_counts_dev, void *stream) {
    if (num_edge > 0 && !keep_dev) {
        set_error("ultra_relation_graph_bits_keep: NULL keep vector");
        return ULTRA_ERR_INVALID;
    }
    return relation_graph_bits(edge_index_dev, edge_type_dev, keep_dev, num_edge, num_node, num_relation, hbits_dev, tbits_dev, adj_dev,
                               row_counts_dev, stream);
}

int32_t ultra_relation_graph_add_edges(const int64_t *edge_index_dev, const int64_t *edge_type_dev, int64_t num_edge, int64_t num_node,
                                       int64_t num_relation, void *hbits_dev, void *tbits_dev, void *adj_dev, int64_t *row_counts_dev,
                                       int32_t *changed_dev, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, adj_dev);
    if (num_edge < 0 || num_node <= 0 || num_relation <= 0 || num_relation > (1 << 20) || (num_edge > 0 && (!edge_index_dev || !edge_type_dev)) ||
        !hbits_dev || !tbits_dev || !adj_dev || !row_counts_dev || !changed_dev) {
        set_error("ultra_relation_graph_add_edges: bad argument");
        return ULTRA_ERR_INVALID;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int words = (int)((num_relation + 31) / 32);
    (void)hipGetLastError();
    hipLaunchKernelGGL(add_edges_check_kernel, dim3(1), dim3(1024), 0, s, edge_index_dev, edge_type_dev, (long long)num_edge,
                       (long long)num_node, (long long)num_relation, changed_dev);
    if (num_edge > 0) {
        hipLaunchKernelGGL(add_edges_incidence_kernel, dim3((unsigned)std::min<int64_t>((num_edge + 255) / 256, 4096)), dim3(256), 0, s,
                           edge_index_dev, edge_type_dev, (long long)num_edge, words, (uint32_t *)hbits_dev, (uint32_t *)tbits_dev,
                           (const int32_t *)changed_dev);
        hipLaunchKernelGGL(add_edges_pair_kernel, dim3((unsigned)std::min<int64_t>((2 * num_edge + 3) / 4, 8192)), dim3(256), 0, s,
                           edge_index_dev, (long long)(2 * num_edge), (const uint32_t *)hbits_dev, (const uint32_t *)tbits_dev,
                           (int)num_relation, words, (uint32_t *)adj_dev, changed_dev);
    }
    const int rows_total = (int)(4 * num_relation);
    hipLaunchKernelGGL(row_count_kernel, dim3((rows_total + 255) / 256), dim3(256), 0, s, (const uint32_t *)adj_dev, rows_total, words,
                       row_counts_dev);
    if (hipGetLastError() != hipSuccess) {
        set_error("ultra_relation_graph_add_edges: launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

int32_t ultra_relation_graph_emit(const void *adj_dev, const int64_t *row_offsets_dev, int64_t num_relation, int64_t total_edges,
                                  int64_t *edge_index_out_dev, int64_t *edge_type_out_dev, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, adj_dev);
    if (!adj_dev || !row_offsets_dev || num_relation <= 0 || total_edges < 0 || (total_edges > 0 && (!edge_index_out_dev || !edge_type_out_dev))) {
        set_error("ultra_relation_graph_emit: bad argument");
        return ULTRA_ERR_INVALID;
    }
    if (total_edges == 0) return ULTRA_OK;
    const int words = (int)((num_relation + 31) / 32);
    const long long waves = 4 * num_relation;
    (void)hipGetLastError();
    hipLaunchKernelGGL(emit_edges_kernel, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const uint32_t *)adj_dev, row_offsets_dev, (int)num_relation, words, (long long)total_edges, edge_index_out_dev,
                       edge_type_out_dev);
    if (hipGetLastError() != hipSuccess) {
        set_error("emit_edges_kernel: launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

int32_t ultra_relation_graph_dense_adjacency(const void *adj_dev, int64_t num_relation, void *a_ex_out_dev, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, adj_dev);
    if (!adj_dev || !a_ex_out_dev || num_relation <= 0) {
        set_error("ultra_relation_graph_dense_adjacency: bad argument");
        return ULTRA_ERR_INVALID;
    }
    const int words = (int)((num_relation + 31) / 32);
    const long long nt = (num_relation + 15) / 16;
    const long long total = nt * nt * 64;
    (void)hipGetLastError();
    hipLaunchKernelGGL(dense_order_adjacency_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), (const uint32_t *)adj_dev, (int)num_relation, words, (uint4 *)a_ex_out_dev);
    if (hipGetLastError() != hipSuccess) {
        set_error("dense_order_adjacency_kernel: launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

int32_t ultra_relation_graph_edge_keep(const void *adj_dev, int64_t num_relation, const int64_t *rel_edge_index_dev,
                                       const int64_t *rel_edge_type_dev, int64_t num_rel_edge, float *keep_out_dev, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, adj_dev);
    if (!adj_dev || num_relation <= 0 || num_relation > (1 << 20) || num_rel_edge < 0 ||
        (num_rel_edge > 0 && (!rel_edge_index_dev || !rel_edge_type_dev || !keep_out_dev))) {
        set_error("ultra_relation_graph_edge_keep: bad argument");
        return ULTRA_ERR_INVALID;
    }
    if (num_rel_edge == 0) return ULTRA_OK;
    const int words = (int)((num_relation + 31) / 32);
    (void)hipGetLastError();
    hipLaunchKernelGGL(relation_edge_keep_kernel, dim3((unsigned)((num_rel_edge + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), (const uint32_t *)adj_dev, (int)num_relation, words, rel_edge_index_dev,
                       rel_edge_type_dev, (long long)num_rel_edge, keep_out_dev);
    if (hipGetLastError() != hipSuccess) {
        set_error("relation_edge_keep_kernel: launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

}  // extern "C"
