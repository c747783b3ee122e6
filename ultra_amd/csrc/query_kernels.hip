// Complex logical queries (UltraQuery): symbolic traversal and answer ranking.
//
// ultra_symbolic_traversal -- SymbolicTraversal.forward (reference: ultra/ultraquery.py:280-298 with torch_scatter's
//   scatter_max, which leaves a row without entries at 0):
//     t[b, v] = max(0, max{ h[b, u] : edge u -> v of type r[b] })
//   over a CSR keyed by (tail, relation): row v holds the in-edges of v sorted by relation, so the edges of relation r[b]
//   into v are one contiguous segment, found by binary search.  One thread per (query, row) scans short segments; a
//   segment longer than TRAVERSAL_LANE_MAX (hub rows) is scanned by the whole wave, one such segment at a time.  Max is
//   exact and order-free, so any scan order gives the same bits.
//
// ultra_answer_ranking -- batch_evaluate (reference: ultra/query_utils.py:284-325) under the stable descending order:
//   u is ahead of v  iff  p_u > p_v, or p_u == p_v and u < v  (a NaN score is above every number, as in torch's sort).
//   One workgroup per query.  Its answers (easy, then hard, each by ascending id) are sorted by that order (bitonic), in LDS
//   when they fit and in a global workspace otherwise.  pred's row is then streamed once: every node u lands in bin
//   k(u) = #{sorted answers ahead of u} (binary search), an integer histogram.  With s_0, s_1, ... the sorted answers,
//     pos(s_i)         = #{u ahead of s_i} = (bins 0..i summed) - 1              (0-based unfiltered position)
//     filtered(s_i)    = 1 + #{non-answers ahead of s_i} = pos(s_i) - i + 1      (the answers ahead are s_0 .. s_{i-1})
//   All counts are integers: the result does not depend on the order of the atomics.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"

namespace ultra {

constexpr int TRAVERSAL_THREADS = 256;
constexpr int TRAVERSAL_LANE_MAX = 16;       // longest segment one lane scans alone
constexpr int RANKING_THREADS = 256;
constexpr int RANKING_LDS_ANSWERS = ULTRA_RANKING_LDS_ANSWERS;

// KEEP (training, traversal dropout): slots with keep_slot[s] == 0 are absent edges
template <typename T, bool KEEP = false>
__global__ void __launch_bounds__(TRAVERSAL_THREADS) symbolic_traversal_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ csr_src, const int32_t *__restrict__ csr_type,
    const int64_t *__restrict__ r_index, const T *__restrict__ h, long long num_node, T *__restrict__ t,
    const float *__restrict__ keep_slot) {
    const long long b = blockIdx.y;
    const long long v = (long long)blockIdx.x * TRAVERSAL_THREADS + threadIdx.x;
    const int32_t r = (int32_t)r_index[b];
    const T *hb = h + b * num_node;
    long long lo = 0, hi = 0;
    if (v < num_node) {
        // [lo, hi): the slots of row v whose relation is r (the row is sorted by relation)
        long long a = row_ptr[v], e = row_ptr[v + 1];
        long long l = a, u = e;
        while (l < u) {
            const long long m = (l + u) >> 1;
            if (csr_type[m] < r) l = m + 1; else u = m;
        }
        lo = l;
        u = e;
        while (l < u) {
            const long long m = (l + u) >> 1;
            if (csr_type[m] <= r) l = m + 1; else u = m;
        }
        hi = l;
    }
    T best = T(0);      // max(0, ...): the reference's clamp(min=0) and torch_scatter's zero for an empty row
    const bool alone = hi - lo <= TRAVERSAL_LANE_MAX;
    if (alone)
        for (long long s = lo; s < hi; ++s) {
            if (KEEP && keep_slot[s] == 0.f) continue;
            const T x = hb[csr_src[s]];
            best = x > best ? x : best;
        }
    // long segments: the whole wave scans one at a time
    unsigned long long todo = __ballot(!alone);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long slo = __shfl(lo, owner), shi = __shfl(hi, owner);
        T m = T(0);
        for (long long s = slo + lane; s < shi; s += 64) {
            if (KEEP && keep_slot[s] == 0.f) continue;
            const T x = hb[csr_src[s]];
            m = x > m ? x : m;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const T o = __shfl_down(m, off);
            m = o > m ? o : m;
        }
        m = __shfl(m, 0);
        if (lane == owner) best = m;
    }
    if (v < num_node) t[b * num_node + v] = best;
}

// NaN ranks above every number, as in torch's descending sort, so the order stays total
__device__ __forceinline__ bool ahead(float va, int32_t ia, float vb, int32_t ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && (!nb || ia < ib);
    return va > vb || (va == vb && ia < ib);
}

// One query per workgroup.  kv / kid / korig (P entries, P a power of two >= A) and hist (A entries) live in LDS or in this
// query's slice of the global workspace.
__device__ void rank_one_query(const float *__restrict__ row, const uint8_t *__restrict__ keep, const int64_t *__restrict__ ans,
                               long long A, long long num_easy, long long P, long long num_node, float *kv, int32_t *kid,
                               int32_t *korig, uint32_t *hist, int64_t *answer_ranking, int64_t *ranking) {
    const int tid = threadIdx.x;
    const float NEG_INF = -__builtin_inff();
    for (long long i = tid; i < P; i += RANKING_THREADS) {
        if (i < A) {
            const int32_t id = (int32_t)ans[i];
            kv[i] = (keep && !keep[id]) ? NEG_INF : row[id];
            kid[i] = id;
            korig[i] = (int32_t)i;
        } else {            // padding: behind every real key (a real -inf has an id below INT32_MAX)
            kv[i] = NEG_INF;
            kid[i] = 0x7fffffff;
            korig[i] = -1;
        }
    }
    for (long long i = tid; i < A; i += RANKING_THREADS) hist[i] = 0u;
    __syncthreads();
    // bitonic sort into the ahead() order
    for (long long k = 2; k <= P; k <<= 1) {
        for (long long j = k >> 1; j > 0; j >>= 1) {
            for (long long i = tid; i < P; i += RANKING_THREADS) {
                const long long p = i ^ j;
                if (p > i) {
                    const bool up = (i & k) == 0;
                    const float vi = kv[i], vp = kv[p];
                    const int32_t ii = kid[i], ip = kid[p];
                    // up: i must end ahead of p
                    if (up ? ahead(vp, ip, vi, ii) : ahead(vi, ii, vp, ip)) {
                        kv[i] = vp, kv[p] = vi;
                        kid[i] = ip, kid[p] = ii;
                        const int32_t o = korig[i];
                        korig[i] = korig[p], korig[p] = o;
                    }
                }
            }
            __syncthreads();
        }
    }
    // stream the row once: bin k(u) = #{answers ahead of u}; bin A is never read, bin 0 is counted per thread
    uint32_t first = 0u;
    for (long long u = tid; u < num_node; u += RANKING_THREADS) {
        const float p = (keep && !keep[u]) ? NEG_INF : row[u];
        long long l = 0, r = A;
        while (l < r) {
            const long long m = (l + r) >> 1;
            if (ahead(kv[m], kid[m], p, (int32_t)u)) l = m + 1; else r = m;
        }
        if (l == 0) ++first;
        else if (l < A) atomicAdd(hist + l, 1u);
    }
    for (int off = 32; off > 0; off >>= 1) first += __shfl_down(first, off);
    if ((tid & 63) == 0 && first) atomicAdd(hist, first);
    __syncthreads();
    // inclusive prefix sum of hist[0, A), 256 entries at a time
    __shared__ uint32_t carry_lds[RANKING_THREADS / 64 + 1];
    uint32_t carry = 0u;
    for (long long base = 0; base < A; base += RANKING_THREADS) {
        const long long i = base + tid;
        uint32_t x = i < A ? hist[i] : 0u;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if ((tid & 63) >= off) x += y;
        }
        if ((tid & 63) == 63) carry_lds[tid >> 6] = x;
        __syncthreads();
        uint32_t before = carry;
        for (int w = 0; w < (tid >> 6); ++w) before += carry_lds[w];
        uint32_t total = carry;
        for (int w = 0; w < RANKING_THREADS / 64; ++w) total += carry_lds[w];
        if (i < A) {
            const long long pos = (long long)(x + before) - 1;
            const int32_t o = korig[i];
            if (o >= 0) {       // (always: the padding sorts behind every answer)
                answer_ranking[o] = pos;
                if (o >= num_easy) ranking[o - num_easy] = pos - i + 1;
            }
        }
        carry = total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(RANKING_THREADS) answer_ranking_kernel(
    const float *__restrict__ pred, const uint8_t *__restrict__ keep, const int64_t *__restrict__ ans,
    const int64_t *__restrict__ ans_ptr, const int64_t *__restrict__ hard_ptr, const int64_t *__restrict__ num_easy,
    const int64_t *__restrict__ ws_off, void *ws, long long num_node, int64_t *answer_ranking, int64_t *ranking) {
    __shared__ float lds_v[RANKING_LDS_ANSWERS];
    __shared__ int32_t lds_id[RANKING_LDS_ANSWERS];
    __shared__ int32_t lds_orig[RANKING_LDS_ANSWERS];
    __shared__ uint32_t lds_hist[RANKING_LDS_ANSWERS];
    const long long b = blockIdx.x;
    const long long a0 = ans_ptr[b], A = ans_ptr[b + 1] - a0;
    if (A == 0) return;
    long long P = 1;
    while (P < A) P <<= 1;
    const float *row = pred + b * num_node;
    if (P <= RANKING_LDS_ANSWERS) {
        rank_one_query(row, keep, ans + a0, A, num_easy[b], P, num_node, lds_v, lds_id, lds_orig, lds_hist,
                       answer_ranking + a0, ranking + hard_ptr[b]);
    } else {
        // this query's slice of the workspace: P floats, P ids, P list positions, P bins (ws_off counts 4-byte words)
        uint32_t *w = reinterpret_cast<uint32_t *>(ws) + ws_off[b];
        rank_one_query(row, keep, ans + a0, A, num_easy[b], P, num_node, reinterpret_cast<float *>(w),
                       reinterpret_cast<int32_t *>(w + P), reinterpret_cast<int32_t *>(w + 2 * P), w + 3 * P,
                       answer_ranking + a0, ranking + hard_ptr[b]);
    }
}

}  // namespace ultra

extern "C" int32_t ultra_symbolic_traversal(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                            int64_t num_node, const int64_t *r_index, int64_t batch, int32_t dtype,
                                            const void *h, void *t, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, h);
    if (!row_ptr || !r_index || !h || !t || num_node <= 0 || batch < 0 || batch > 65535 || num_node >= (1LL << 31)) {
        ultra::set_error("ultra_symbolic_traversal: NULL operand or batch / num_node out of range");
        return ULTRA_ERR_INVALID;
    }
    if (dtype != 0 && dtype != 1) {
        ultra::set_error("ultra_symbolic_traversal: dtype must be fp32 (0) or fp64 (1)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch == 0) return ULTRA_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((num_node + ultra::TRAVERSAL_THREADS - 1) / ultra::TRAVERSAL_THREADS), (unsigned)batch);
    (void)hipGetLastError();
    if (dtype == 0)
        hipLaunchKernelGGL(ultra::symbolic_traversal_kernel<float>, grid, dim3(ultra::TRAVERSAL_THREADS), 0, s, row_ptr,
                           csr_src, csr_type, r_index, (const float *)h, (long long)num_node, (float *)t, nullptr);
    else
        hipLaunchKernelGGL(ultra::symbolic_traversal_kernel<double>, grid, dim3(ultra::TRAVERSAL_THREADS), 0, s, row_ptr,
                           csr_src, csr_type, r_index, (const double *)h, (long long)num_node, (double *)t, nullptr);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("symbolic_traversal_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

// the same on the graph without its dropped edges: keep_slot (num_edge) fp32 in CSR slot order, 0 = absent (training)
extern "C" int32_t ultra_symbolic_traversal_keep(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                                 const float *keep_slot, int64_t num_node, const int64_t *r_index, int64_t batch,
                                                 int32_t dtype, const void *h, void *t, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, h);
    if (!row_ptr || !keep_slot || !r_index || !h || !t || num_node <= 0 || batch < 0 || batch > 65535 || num_node >= (1LL << 31)) {
        ultra::set_error("ultra_symbolic_traversal_keep: NULL operand or batch / num_node out of range");
        return ULTRA_ERR_INVALID;
    }
    if (dtype != 0 && dtype != 1) {
        ultra::set_error("ultra_symbolic_traversal_keep: dtype must be fp32 (0) or fp64 (1)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (batch == 0) return ULTRA_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((num_node + ultra::TRAVERSAL_THREADS - 1) / ultra::TRAVERSAL_THREADS), (unsigned)batch);
    (void)hipGetLastError();
    if (dtype == 0)
        hipLaunchKernelGGL((ultra::symbolic_traversal_kernel<float, true>), grid, dim3(ultra::TRAVERSAL_THREADS), 0, s, row_ptr,
                           csr_src, csr_type, r_index, (const float *)h, (long long)num_node, (float *)t, keep_slot);
    else
        hipLaunchKernelGGL((ultra::symbolic_traversal_kernel<double, true>), grid, dim3(ultra::TRAVERSAL_THREADS), 0, s, row_ptr,
                           csr_src, csr_type, r_index, (const double *)h, (long long)num_node, (double *)t, keep_slot);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("symbolic_traversal_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

extern "C" int32_t ultra_answer_ranking(const void *pred, const uint8_t *keep, const int64_t *answers, const int64_t *ans_ptr,
                                        const int64_t *hard_ptr, const int64_t *num_easy, const int64_t *ws_off, void *ws,
                                        int64_t batch, int64_t num_node, int64_t *answer_ranking, int64_t *ranking,
                                        void *stream) {
    ULTRA_DEVICE_SCOPE(stream, pred);
    if (!pred || !answers || !ans_ptr || !hard_ptr || !num_easy || !ws_off || !answer_ranking || !ranking || batch < 0 ||
        num_node <= 0 || num_node >= (1LL << 31)) {
        ultra::set_error("ultra_answer_ranking: NULL operand or batch / num_node out of range");
        return ULTRA_ERR_INVALID;
    }
    if (batch == 0) return ULTRA_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(ultra::answer_ranking_kernel, dim3((unsigned)batch), dim3(ultra::RANKING_THREADS), 0, s,
                       (const float *)pred, keep, answers, ans_ptr, hard_ptr, num_easy, ws_off, ws, (long long)num_node,
                       answer_ranking, ranking);
    if (hipGetLastError() != hipSuccess) {
        ultra::set_error("answer_ranking_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}
