// The symbolic traversal of a CHANGING graph: ultra_symbolic_traversal_edit_rows.
//
// ultra_symbolic_traversal (csrc/query_kernels.hip) walks a CSR keyed by (tail, relation) that a device sort over all E edges
// builds once per graph.  Facts added to or retracted from the served graph (rspmm.GraphDelta) change t[b, v] for exactly the
// tails v an added or a removed edge points into, so the cached CSR stays and ONE launch after the base launch recomputes
// those rows:
//     t[b, v] = max(0, max{h[b, u] : live base edge u -> v of type r[b]}, max{h[b, u] : added edge u -> v of type r[b]})
// A base edge (u, v, r) is dead iff (u, r) is among the tail's dead keys (every duplicate goes); the keys never apply to the
// added edges.  Max is exact and order-free: the bits are those of ultra_symbolic_traversal on the materialised graph.
//
// One WAVE per (touched tail, sample).  A uniformly drawn fact points into a hub, and the rspmm fix-up of DESIGN.md 18 showed what a
// hub row walked as one dependent chain costs; a max has no order to keep, so here the relation's segment (the base kernel's two
// binary searches) is scanned 64 slots a trip, one independent gather per lane, and combined by lane shuffles.  Within a tail
// both the added edges and the dead keys are sorted by (relation, source): the relation's keys are one contiguous sorted range
// (two binary searches, wave-uniform), in which every lane binary-searches its own edge's source -- a hub row costs
// segment / 64 trips of log2(keys) compares, not `segment` dependent loads.
//
// The grid is sized by (capacity_rows, batch); the live row count is read on the device and a wave at or beyond it ends at once,
// so a launch recorded into a hipGraph serves whatever the buffers hold at replay.  No atomics, no allocation, no memset, no host
// synchronisation.  Every ptr value is clamped to its capacity, a key is only compared, a touched tail outside [0, num_node) is
// not written and a source outside [0, num_node) is never dereferenced.
//
// Facts ASSUMED per query: ultra_symbolic_traversal_edit_rows_owned, the template flag OWNED.  An int32
// owner per added edge names the one sample that sees it (-1: every sample; any other value outside [0, batch): none); an owner is
// only compared.  The dead keys still apply to base edges only, so a retracted base fact that one sample assumes again is live
// for that sample.  The added range is scanned FIRST, one strided pass that takes the edges live for b and notes whether there
// was one; a (tail, sample) wave with no dead key of its relation and no live added edge ends there, before the base segment is
// read, and writes nothing -- the base launch already wrote the right bits.  A hub tail touched by one query's hypothesis is so
// scanned by one wave, not by `batch` waves.  Without the flag nothing changes: every touched pair is written.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"

namespace ultra {

constexpr int TRAVERSAL_EDIT_THREADS = 256;
constexpr int TRAVERSAL_EDIT_WAVES = TRAVERSAL_EDIT_THREADS / 64;      // (touched tail, sample) pairs per workgroup

// [first index in [a, e) whose type is >= r, first whose type is > r): `type` ascends over [a, e)
template <typename I>
__device__ __forceinline__ void type_range(const int32_t *__restrict__ type, I a, I e, int32_t r, I &lo, I &hi) {
    I l = a, u = e;
    while (l < u) {
        const I m = l + ((u - l) >> 1);
        if (type[m] < r) l = m + 1; else u = m;
    }
    lo = l;
    u = e;
    while (l < u) {
        const I m = l + ((u - l) >> 1);
        if (type[m] <= r) l = m + 1; else u = m;
    }
    hi = l;
}

__device__ __forceinline__ int32_t clamp_ptr(int32_t p, int32_t lo, long long capacity) {
    const int32_t cap = capacity > 0x7fffffffLL ? 0x7fffffff : (int32_t)capacity;
    return p < lo ? lo : (p > cap ? cap : p);
}

template <typename T, bool OWNED = false>
__global__ void __launch_bounds__(TRAVERSAL_EDIT_THREADS) symbolic_traversal_edit_rows_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ csr_src, const int32_t *__restrict__ csr_type,
    long long num_node, const int32_t *__restrict__ rows, const int32_t *__restrict__ count,
    const int32_t *__restrict__ add_ptr, const int32_t *__restrict__ add_src, const int32_t *__restrict__ add_type,
    const int32_t *__restrict__ owner, const int32_t *__restrict__ dead_ptr, const int32_t *__restrict__ dead_src,
    const int32_t *__restrict__ dead_type, long long capacity_rows, long long capacity_edges, long long capacity_keys, const int64_t *__restrict__ r_index,
    const T *__restrict__ h, T *__restrict__ t) {
    // (wave-uniform by construction: the searches below run once per wave)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long slot = (long long)blockIdx.x * TRAVERSAL_EDIT_WAVES + wave;
    const long long b = blockIdx.y;
    long long live = count[0];
    live = live < capacity_rows ? live : capacity_rows;
    if (slot >= live) return;
    const long long v = rows[slot];
    if (v < 0 || v >= num_node) return;
    const int32_t r = (int32_t)r_index[b];
    const T *hb = h + b * num_node;

    // the relation's dead keys of this tail: one sorted range of sources
    int32_t klo = 0, khi = 0;
    if (dead_ptr != nullptr) {
        const int32_t k0 = clamp_ptr(dead_ptr[slot], 0, capacity_keys);
        const int32_t k1 = clamp_ptr(dead_ptr[slot + 1], k0, capacity_keys);
        type_range<int32_t>(dead_type, k0, k1, r, klo, khi);
    }

    T best = T(0);      // max(0, ...), as in the base kernel
    // added edges of relation r into v
    const int32_t a0 = clamp_ptr(add_ptr[slot], 0, capacity_edges);
    const int32_t a1 = clamp_ptr(add_ptr[slot + 1], a0, capacity_edges);
    int32_t alo, ahi;
    type_range<int32_t>(add_type, a0, a1, r, alo, ahi);
    if constexpr (OWNED) {
        // ... those live for sample b: this pass comes first, it decides whether the wave has anything to write
        bool mine = false;
        for (int32_t s = alo + lane; s < ahi; s += 64) {
            const int32_t o = owner[s];
            if (o == -1 || o == (int32_t)b) {
                mine = true;
                const int32_t u = add_src[s];
                if (u >= 0 && u < num_node) {
                    const T x = hb[u];
                    best = x > best ? x : best;
                }
            }
        }
        if (klo == khi && __ballot(mine) == 0) return;      // (wave-uniform) the base launch's bits stand
    }
    // live base edges of relation r into v
    long long lo, hi;
    type_range<long long>(csr_type, row_ptr[v], row_ptr[v + 1], r, lo, hi);
    for (long long s = lo + lane; s < hi; s += 64) {
        const int32_t u = csr_src[s];
        int32_t l = klo, e = khi;
        while (l < e) {
            const int32_t m = l + ((e - l) >> 1);
            if (dead_src[m] < u) l = m + 1; else e = m;
        }
        const bool dead = l < khi && dead_src[l] == u;
        if (!dead && u >= 0 && u < num_node) {
            const T x = hb[u];
            best = x > best ? x : best;
        }
    }
    if constexpr (!OWNED) {
        for (int32_t s = alo + lane; s < ahi; s += 64) {
            const int32_t u = add_src[s];
            if (u >= 0 && u < num_node) {
                const T x = hb[u];
                best = x > best ? x : best;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_down(best, off);
        best = o > best ? o : best;
    }
    if (lane == 0) t[b * num_node + v] = best;
}

}  // namespace ultra

namespace ultra {

// Both entries: `name` prefixes the messages; owner_dev non-NULL selects the OWNED instantiation.
static int32_t traversal_edit_rows(const char *name, const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                   int64_t num_node, const ultra_traversal_edits *edits, const int32_t *owner_dev, bool owned,
                                   const int64_t *r_index, int64_t batch, int32_t dtype, const void *h, void *t, void *stream) {
    // (every argument is judged before the first GPU call)
    const std::string who(name);
    if (!row_ptr || !csr_src || !csr_type || !edits || !r_index || !h || !t || num_node <= 0 || num_node >= (1LL << 31) ||
        batch < 0 || batch > 65535) {
        set_error(who + ": NULL operand or batch / num_node out of range");
        return ULTRA_ERR_INVALID;
    }
    if (owned && !owner_dev) {
        set_error(who + ": owner_dev is NULL (one int32 owner per added edge)");
        return ULTRA_ERR_INVALID;
    }
    if (dtype != 0 && dtype != 1) {
        set_error(who + ": dtype must be fp32 (0) or fp64 (1)");
        return ULTRA_ERR_INVALID;
    }
    if (edits->capacity_rows < 0 || edits->capacity_edges < 0 || edits->capacity_keys < 0 ||
        edits->capacity_rows >= (1LL << 31) - TRAVERSAL_EDIT_WAVES) {
        set_error(who + ": capacities out of range");
        return ULTRA_ERR_INVALID;
    }
    if (!edits->row_dev || !edits->count_dev || !edits->add_ptr_dev || !edits->add_src_dev || !edits->add_type_dev ||
        (edits->dead_ptr_dev && (!edits->dead_src_dev || !edits->dead_type_dev))) {
        set_error(who + ": NULL array in the edits (only dead_ptr_dev may be NULL)");
        return ULTRA_ERR_INVALID;
    }
    if (edits->capacity_rows == 0 || batch == 0) return ULTRA_OK;
    ULTRA_DEVICE_SCOPE(stream, h);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((edits->capacity_rows + TRAVERSAL_EDIT_WAVES - 1) / TRAVERSAL_EDIT_WAVES), (unsigned)batch);
    (void)hipGetLastError();
#define ULTRA_TRAVERSAL_EDIT_LAUNCH(T, OWNED)                                                                                   \
    hipLaunchKernelGGL((symbolic_traversal_edit_rows_kernel<T, OWNED>), grid, dim3(TRAVERSAL_EDIT_THREADS), 0, s, row_ptr,     \
                       csr_src, csr_type, (long long)num_node, edits->row_dev, edits->count_dev, edits->add_ptr_dev,            \
                       edits->add_src_dev, edits->add_type_dev, owner_dev, edits->dead_ptr_dev, edits->dead_src_dev,            \
                       edits->dead_type_dev, (long long)edits->capacity_rows, (long long)edits->capacity_edges,                 \
                       (long long)edits->capacity_keys, r_index, (const T *)h, (T *)t)
    if (owned) {
        if (dtype == 0) ULTRA_TRAVERSAL_EDIT_LAUNCH(float, true); else ULTRA_TRAVERSAL_EDIT_LAUNCH(double, true);
    } else {
        if (dtype == 0) ULTRA_TRAVERSAL_EDIT_LAUNCH(float, false); else ULTRA_TRAVERSAL_EDIT_LAUNCH(double, false);
    }
#undef ULTRA_TRAVERSAL_EDIT_LAUNCH
    if (hipGetLastError() != hipSuccess) {
        set_error("symbolic_traversal_edit_rows_kernel launch failed");
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

}  // namespace ultra

extern "C" int32_t ultra_symbolic_traversal_edit_rows(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                                      int64_t num_node, const ultra_traversal_edits *edits,
                                                      const int64_t *r_index, int64_t batch, int32_t dtype, const void *h,
                                                      void *t, void *stream) {
    return ultra::traversal_edit_rows("ultra_symbolic_traversal_edit_rows", row_ptr, csr_src, csr_type, num_node, edits, nullptr,
                                      false, r_index, batch, dtype, h, t, stream);
}

extern "C" int32_t ultra_symbolic_traversal_edit_rows_owned(const int64_t *row_ptr, const int32_t *csr_src,
                                                            const int32_t *csr_type, int64_t num_node,
                                                            const ultra_traversal_edits *edits, const int32_t *owner_dev,
                                                            const int64_t *r_index, int64_t batch, int32_t dtype, const void *h,
                                                            void *t, void *stream) {
    return ultra::traversal_edit_rows("ultra_symbolic_traversal_edit_rows_owned", row_ptr, csr_src, csr_type, num_node, edits,
                                      owner_dev, true, r_index, batch, dtype, h, t, stream);
}
