// Edits as a DELTA on the cached plan of a served graph: ONE walk of the edited rows with two optional cursors
// (ultra_rspmm_delta_rows / _edit_rows / _edit_rows_samples, include/ultra_rspmm.h).
//
// The plan of the base graph stays as it is.  After a layer's aggregate (ultra_rspmm_forward / _forward_point on the base
// plan) ONE launch recomputes the output rows that an edit points into -- the only rows whose value differs on the edited
// graph -- and overwrites them.  Per (touched row, outer slice) one 16-lane group walks the row's base edges (the plan's device
// CSR: row_ptr / col / type, sorted by (row, col, edge id)) and the row's delta edges (sorted by (row, col, insertion id)) as a
// two-way merge on col, base edges first at equal col: the sorted (row, col, edge id) order of a plan of the concatenated edge
// list, where the delta edges carry the highest ids.  Messages and the sequential reduction are those of the reference-order
// kernels for unit edge weights (rspmm_kernels.hpp: binary / nary), the epilogue is the boundary epilogue of
// rspmm_order_kernels.hpp: with -ffp-contract=off the rows equal those of a fresh reference-order plan of the materialised
// graph bit for bit.
//
// The grid is sized by the delta's CAPACITY; the live number of touched rows is read from device memory and the groups
// beyond it end at once, so a launch recorded into a hipGraph serves every later content of the same buffers.  No atomics,
// no allocation, no memset, no host synchronisation.
//
// A hub row (longer than the plan's seg_len, a chain row of the base walk) is walked by these three kernels by ONE group as one
// dependent chain: loads are issued DELTA_BATCH edges ahead, the additions stay in order.  ultra_rspmm_edit_rows_split
// (the *_split_kernel shells, hub_row_walk below) hands such a row to a workgroup instead.
//
// The walk (edit_rows_walk) is written once; three kernels instantiate it:
//   rspmm_delta_rows_kernel         <TOMBS = false, KEYS = false>   ADDED facts alone: every base edge and every
//                                                                   delta edge of the row takes part.
//   rspmm_edit_rows_kernel          <TOMBS = true,  KEYS = false>   plus RETRACTED facts, TOMBSTONES on the same plan.
//   rspmm_edit_rows_samples_kernel  <TOMBS = true,  KEYS = true>    plus PER-SLICE dead keys.
//
// and the split launch has one more shell of its own:
//   rspmm_edit_rows_owned_kernel    <TOMBS = true,  KEYS = false, OWNED = true>   delta edges that are live in ONE outer slice each
//                                                                   (what-if facts assumed per query) beside those live in all.
//
// TOMBS: a removed edge changes the one row it points into, so the touched rows are the union of both kinds and the base cursor
// gets one more cursor beside it: per touched row the distinct dead (col, type) keys, sorted; a base edge whose (col, type) is
// among them takes no part (base edges of one col come in edge-id order, not type order: the keys of that col are scanned).  A
// subsequence of a sorted row is still sorted, so the bit-equality argument is the same one.  A row left with NO edge holds what
// the reference-order walk writes for an edge-less row: the reduction's start value (0; the largest / lowest finite number under
// min / max, NaryOp::zero of the reference, never an infinity) met by the boundary epilogue -- the boundary row under a dense
// or an on-row point boundary, 0 under an off-row point boundary with min / max, nothing without a boundary.
//
// KEYS: leave-one-out verification on a graph that holds edits.  Outer slice s must not see a few (row, col, type) edges -- its
// stated fact and the inverse -- whether they are base edges or delta edges, so both cursors also skip an edge that one of the
// slice's keys names (type < 0: any type).  A group keeps the keys of its own row in registers (at most eight); the rows no edit
// points into are the business of the per-sample keep masks of the base walk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "device_scope.hpp"
#include "rspmm_kernels.hpp"

namespace ultra {

constexpr int DELTA_BATCH = 8;        // source / relation rows requested ahead of the ordered additions
constexpr int DELTA_THREADS = 256;    // sixteen 16-lane groups a workgroup
constexpr int SAMPLE_KEYS_MAX = 8;

struct DeltaParams {
    const int32_t *row_ptr, *col, *type;                 // the base plan's CSR (sorted edge order)
    const int32_t *d_row, *d_ptr, *d_col, *d_type;       // the delta: touched rows, their edge ranges, the sorted delta edges
    const int32_t *d_count;                              // live number of touched rows (device memory)
    int32_t cap_rows, cap_edges;
    MatArg rel, x, bnd;
    const long long *bnd_rows;                           // != NULL: `bnd` is a point boundary (one row per outer slice)
    int32_t has_bnd;
    void *out;
    long long out_stride_outer, out_stride_row;
    int32_t n_outer, row_len, num_out, num_in, num_rel;
    long long num_edge;
    int32_t hub_len;                                     // the split kernels alone: a base row longer than this is a hub
};

struct EditParams : DeltaParams {
    const int32_t *t_ptr, *t_col, *t_type;               // the tombstones: per touched row its dead (col, type) keys, sorted
    int32_t cap_keys;
};

struct SampleParams : EditParams {
    const int32_t *k_row, *k_col, *k_type;               // per outer slice `per_sample` dead (row, col, type) keys; type < 0: any
    int32_t per_sample;
};

struct OwnedParams : SampleParams {
    const int32_t *d_owner;                              // per delta edge: -1 live in every outer slice, s in slice s alone
};

// OWNED: is the delta edge whose owner is `owner` live in outer slice `outer`?  (compared only, never used as an index: any
// value but -1 and the slice's own number is live nowhere)
__device__ __forceinline__ bool owner_live(int owner, int outer) { return owner == -1 || owner == outer; }

// The walk of one (touched row, outer slice) by one 16-lane group.  (bi, bcol, btype) is always the next LIVE base edge of the
// row, (dj, dcol, dtype) the next live delta edge.  TOMBS reads EditParams' tombstones, KEYS SampleParams' per-slice keys; with
// KEYS a NULL t_ptr means "no tombstones".
// SPLIT (rspmm_edit_rows_split_kernel): a row whose base length exceeds p.hub_len is left to hub_row_walk below.
// OWNED (rspmm_edit_rows_owned_kernel; OwnedParams, a NULL t_ptr means "no tombstones"): a delta edge takes part in the slices
// its owner names, and a (row, slice) with no tombstone key and no live delta edge is left as the base walk wrote it.
template <typename T, int SUM, int MUL, bool TOMBS, bool KEYS, bool SPLIT = false, bool OWNED = false, typename Params>
__device__ __forceinline__ void edit_rows_walk(const Params &p) {
    constexpr int VEC = 16 / (int)sizeof(T);      // elements per 16-byte chunk
    using P = Pack<T, VEC>;
    const int l16 = threadIdx.x & 15;
    const long long group = (long long)blockIdx.x * (DELTA_THREADS / 16) + (threadIdx.x >> 4);
    const int k = (int)(group / p.n_outer), outer = (int)(group - (long long)k * p.n_outer);
    const int live = min(max(*p.d_count, 0), p.cap_rows);
    if (k >= live) return;
    const int row = p.d_row[k];
    if (row < 0 || row >= p.num_out) return;      // (a delta prepared for another graph: nothing is written)
    const int i = p.row_ptr[row];
    const int ie = p.row_ptr[row + 1];
    const int j = min(max(p.d_ptr[k], 0), p.cap_edges);
    const int je = min(max(p.d_ptr[k + 1], j), p.cap_edges);
    int q = 0, qe = 0;                            // (no tombstones: an empty key range)
    if constexpr (TOMBS) {                        // (two selects, not one branch: DESIGN.md 26 has the measurement)
        q = (!(KEYS || OWNED) || p.t_ptr) ? min(max(p.t_ptr[k], 0), p.cap_keys) : 0;
        qe = (!(KEYS || OWNED) || p.t_ptr) ? min(max(p.t_ptr[k + 1], q), p.cap_keys) : 0;
    }
    if (i < 0 || ie < i || ie > p.num_edge) return;
    if constexpr (SPLIT)
        if (ie - i > p.hub_len) return;
    if constexpr (OWNED) {
        // the early-out (a contract: the row is NOT written): no tombstone key in the row and no delta edge live in this slice.
        // The group's lanes share the row's delta range (bounded by the capacity) and OR their findings over the sixteen.
        if (q == qe) {
            int any = 0;
            for (int dj = j + l16; dj < je; dj += 16) any |= owner_live(p.d_owner[dj], outer) ? 1 : 0;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) any |= __shfl_xor(any, m, 16);
            if (!any) return;
        }
    }

    // KEYS: this slice's keys that name this row (compared only, never used as an index), filtered into registers once per
    // group; a group with none takes one always-false branch per edge
    int sc[SAMPLE_KEYS_MAX], st[SAMPLE_KEYS_MAX];
    unsigned smask = 0;
    if constexpr (KEYS) {
        const long long sbase = (long long)outer * p.per_sample;
#pragma unroll
        for (int u = 0; u < SAMPLE_KEYS_MAX; ++u) {
            sc[u] = 0, st[u] = 0;
            if (u < p.per_sample && p.k_row[sbase + u] == row) {
                sc[u] = p.k_col[sbase + u], st[u] = p.k_type[sbase + u];
                smask |= 1u << u;
            }
        }
    }
    [[maybe_unused]] const auto sample_dead = [&](int col, int type) {
        bool dead = false;
#pragma unroll
        for (int u = 0; u < SAMPLE_KEYS_MAX; ++u)
            dead |= ((smask >> u) & 1u) && sc[u] == col && (st[u] < 0 || st[u] == type);
        return dead;
    };

    const T *rel = reinterpret_cast<const T *>(p.rel.ptr) + outer * p.rel.stride_outer;
    const T *x = reinterpret_cast<const T *>(p.x.ptr) + outer * p.x.stride_outer;
    T *dst = reinterpret_cast<T *>(p.out) + outer * p.out_stride_outer + (long long)row * p.out_stride_row;
    const long long bnd_row = p.bnd_rows ? p.bnd_rows[outer] : -1;

    // (every lane of the group takes every trip, the lanes beyond a short row on chunk 0 without storing: the base indices
    // below pass between the group's lanes)
    for (int dbase = 0; dbase < p.row_len; dbase += 16 * VEC) {
        const bool dvalid = dbase + VEC * l16 < p.row_len;
        const int d0 = dvalid ? dbase + VEC * l16 : 0;
        int bi = i - 1, dj = j - 1, kq = q;
        int bcol = 0, btype = 0, dcol = 0, dtype = 0;
        // the base row's (col, type) pairs, sixteen at a time: lane l holds pair cbase + l, one coalesced load for sixteen
        // steps of the walk instead of a dependent load per step
        int cbase = i - 16, ccol = 0, ctype = 0;
        [[maybe_unused]] int kcol = INT32_MAX;           // TOMBS: the tombstone key under the cursor
        if constexpr (TOMBS) kcol = kq < qe ? p.t_col[kq] : INT32_MAX;
        // step to the next base edge that carries neither a tombstone nor one of the slice's keys (the key cursor only moves
        // forward: cols ascend along the row)
        const auto next_base = [&]() {
            for (++bi; bi < ie; ++bi) {
                if (bi >= cbase + 16) {
                    cbase = bi;
                    const int mine = min(bi + l16, ie - 1);
                    ccol = p.col[mine], ctype = p.type[mine];
                }
                bcol = __shfl(ccol, bi - cbase, 16), btype = __shfl(ctype, bi - cbase, 16);
                bool dead = false;
                if constexpr (TOMBS) {
                    while (kcol < bcol) {
                        ++kq;
                        kcol = kq < qe ? p.t_col[kq] : INT32_MAX;
                    }
                    if (kcol == bcol)
                        for (int s = kq; s < qe && p.t_col[s] == bcol; ++s) dead |= p.t_type[s] == btype;
                }
                if constexpr (KEYS)
                    if (smask && !dead) dead = sample_dead(bcol, btype);
                if (!dead) return;
            }
        };
        // step to the next delta edge that carries none of the slice's keys (tombstones never apply to delta edges)
        const auto next_delta = [&]() {
            for (++dj; dj < je; ++dj) {
                if constexpr (OWNED)
                    if (!owner_live(p.d_owner[dj], outer)) continue;
                dcol = p.d_col[dj], dtype = p.d_type[dj];
                if constexpr (KEYS) {
                    if (!smask || !sample_dead(dcol, dtype)) return;
                } else {
                    return;
                }
            }
        };
        next_base();
        next_delta();
        P acc;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[e] = nary_zero<T, SUM>();
        while (bi < ie || dj < je) {
            // the next DELTA_BATCH edges of the merged order: (col, type) each
            int c[DELTA_BATCH], t[DELTA_BATCH];
            bool take[DELTA_BATCH];
#pragma unroll
            for (int u = 0; u < DELTA_BATCH; ++u) {
                c[u] = 0, t[u] = 0, take[u] = false;
                if (bi < ie && (dj >= je || bcol <= dcol)) {        // (equal col: the base edge has the lower edge id)
                    c[u] = bcol, t[u] = btype, take[u] = true;
                    next_base();
                } else if (dj < je) {
                    c[u] = dcol, t[u] = dtype, take[u] = true;
                    next_delta();
                }
                // (an index outside the operands is never dereferenced: such an edge reads row 0 and is left out of the reduction)
                if (c[u] < 0 || c[u] >= p.num_in || t[u] < 0 || t[u] >= p.num_rel) c[u] = 0, t[u] = 0, take[u] = false;
            }
            P xv[DELTA_BATCH], rv[DELTA_BATCH];
#pragma unroll
            for (int u = 0; u < DELTA_BATCH; ++u) {
                xv[u] = *reinterpret_cast<const P *>(x + (long long)c[u] * p.x.stride_row + d0);
                rv[u] = *reinterpret_cast<const P *>(rel + (long long)t[u] * p.rel.stride_row + d0);
            }
#pragma unroll
            for (int u = 0; u < DELTA_BATCH; ++u) {
                if (take[u]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc.v[e] = nary<T, SUM>(acc.v[e], binary<T, MUL>(rv[u].v[e], xv[u].v[e]));
                }
            }
        }
        // the boundary epilogue of the reference-order kernels; a row with no surviving edge meets it with the start value
        if (p.has_bnd && (bnd_row < 0 || bnd_row == row)) {
            const P b = *reinterpret_cast<const P *>(reinterpret_cast<const T *>(p.bnd.ptr) + outer * p.bnd.stride_outer +
                                                     (bnd_row < 0 ? (long long)row * p.bnd.stride_row : 0) + d0);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[e] = nary<T, SUM>(acc.v[e], b.v[e]);
        } else if (SUM != ULTRA_SUM_ADD && p.has_bnd) {     // (min / max: a point boundary stands for zeros elsewhere)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[e] = nary<T, SUM>(acc.v[e], T(0));
        }
        if (dvalid) *reinterpret_cast<P *>(dst + d0) = acc;
    }
}

// The three shells keep their names: profiles and tools/retract_bench.py tell an add-only step from a retraction by them.
template <typename T, int SUM, int MUL>
__global__ void __launch_bounds__(DELTA_THREADS) rspmm_delta_rows_kernel(const DeltaParams p) {
    edit_rows_walk<T, SUM, MUL, false, false>(p);
}
template <typename T, int SUM, int MUL>
__global__ void __launch_bounds__(DELTA_THREADS) rspmm_edit_rows_kernel(const EditParams p) {
    edit_rows_walk<T, SUM, MUL, true, false>(p);
}
template <typename T, int SUM, int MUL>
__global__ void __launch_bounds__(DELTA_THREADS) rspmm_edit_rows_samples_kernel(const SampleParams p) {
    edit_rows_walk<T, SUM, MUL, true, true>(p);
}

// ---- hub rows: one WORKGROUP per (touched row longer than hub_len, outer slice) ----
// The same stream, the same messages and the same single chain of additions as edit_rows_walk, but the messages of the base
// edges are produced in parallel.  Per 64-/32-element trip the row's base slots go by in tiles of HUB_TILE consecutive slots
// through a three-stage pipeline, one __syncthreads a stage:
//   A  (producer threads, one per slot)        load the slot's (col, type), decide deadness -- outside the operands; a tombstone
//                                              (lower bound on col in the row's key range, then that col's keys); one of the
//                                              slice's keys (registers) -- and write col / type / live into an LDS meta tile;
//   B  (twelve producer 16-lane groups)        read the meta tile, gather x[col] and rel[type] of HUB_SLOTS slots at once
//                                              (a dead slot reads row 0, as the walk does), write the MESSAGE into an LDS tile;
//   C  (sixteen lanes of the consumer wave)    drain the tile in slot order into the one accumulator chain: before base slot s
//                                              every delta edge of a lower col (base first at equal col), then the slot's
//                                              message if it is live -- a dead slot is skipped, never added as a zero.  The
//                                              row's delta edges are the consumer's own: it holds the next live one, message
//                                              loaded, one edge ahead.
// Stage A works on tile it, B on tile it - 1, C on tile it - 2: the message tiles alternate, the meta tiles rotate by three
// (C still reads tile it - 2's cols while A writes tile it's).  Tile boundaries count base slots, dead ones included, so the
// trip count ntiles + 2 is known before the loop and every wave reaches every barrier; the only returns are ahead of the
// first barrier and uniform.  LDS indices are loop counters and thread indices; loaded values are only compared or range
// checked before they address x / rel.  No atomics, no flags, no communication between workgroups.
constexpr int HUB_TILE = 96;                                             // base slots a tile
constexpr int HUB_GROUPS = (DELTA_THREADS - 64) / 16;                    // producer 16-lane groups: three waves
constexpr int HUB_SLOTS = HUB_TILE / HUB_GROUPS;                         // gathers in flight per producer lane (x and rel each)
constexpr int HUB_DRAIN = 8;                                             // slots the consumer reads from LDS ahead of its chain
static_assert(HUB_TILE % HUB_DRAIN == 0, "the consumer's batches tile the tile");
static_assert(HUB_SLOTS * HUB_GROUPS == HUB_TILE && HUB_TILE <= DELTA_THREADS - 64, "a producer thread per slot, whole rounds of groups");

template <typename T, int SUM, int MUL, bool TOMBS, bool KEYS, bool OWNED = false, typename Params>
__device__ __forceinline__ void hub_row_walk(const Params &p, const long long wg) {
    constexpr int VEC = 16 / (int)sizeof(T);
    using P = Pack<T, VEC>;
    __shared__ P s_msg[2][HUB_TILE][16];                  // 2 * 96 * 256 B = 48 KiB
    __shared__ int s_col[3][HUB_TILE], s_type[3][HUB_TILE], s_live[3][HUB_TILE];      // 3,456 B
    const int tid = threadIdx.x, l16 = tid & 15, grp = tid >> 4;
    const bool producer = tid < DELTA_THREADS - 64;
    const bool drains = tid >= DELTA_THREADS - 64 && tid < DELTA_THREADS - 48;        // the consumer wave's first sixteen lanes
    const int k = (int)(wg / p.n_outer), outer = (int)(wg - (long long)k * p.n_outer);
    const int live = min(max(*p.d_count, 0), p.cap_rows);
    if (k >= live) return;
    const int row = p.d_row[k];
    if (row < 0 || row >= p.num_out) return;
    const int i = p.row_ptr[row];
    const int ie = p.row_ptr[row + 1];
    if (i < 0 || ie < i || ie > p.num_edge) return;
    const int n = ie - i;
    if (n <= p.hub_len) return;                           // (hub_len >= 0: a hub has an edge)
    const int j = min(max(p.d_ptr[k], 0), p.cap_edges);
    const int je = min(max(p.d_ptr[k + 1], j), p.cap_edges);
    int q = 0, qe = 0;
    if constexpr (TOMBS) {
        q = (!(KEYS || OWNED) || p.t_ptr) ? min(max(p.t_ptr[k], 0), p.cap_keys) : 0;
        qe = (!(KEYS || OWNED) || p.t_ptr) ? min(max(p.t_ptr[k + 1], q), p.cap_keys) : 0;
    }
    if constexpr (OWNED) {
        // the early-out of edit_rows_walk, ahead of the first barrier: every thread scans the same range (bounded by the
        // capacity) of the same workgroup-uniform addresses, so the whole workgroup returns or none of it does
        if (q == qe) {
            bool any = false;
            for (int dj = j; dj < je; ++dj) any |= owner_live(p.d_owner[dj], outer);
            if (!any) return;
        }
    }
    const int ntiles = (n - 1) / HUB_TILE + 1;

    int sc[SAMPLE_KEYS_MAX], st[SAMPLE_KEYS_MAX];
    unsigned smask = 0;
    if constexpr (KEYS) {
        const long long sbase = (long long)outer * p.per_sample;
#pragma unroll
        for (int u = 0; u < SAMPLE_KEYS_MAX; ++u) {
            sc[u] = 0, st[u] = 0;
            if (u < p.per_sample && p.k_row[sbase + u] == row) {
                sc[u] = p.k_col[sbase + u], st[u] = p.k_type[sbase + u];
                smask |= 1u << u;
            }
        }
    }
    [[maybe_unused]] const auto sample_dead = [&](int col, int type) {
        bool dead = false;
#pragma unroll
        for (int u = 0; u < SAMPLE_KEYS_MAX; ++u)
            dead |= ((smask >> u) & 1u) && sc[u] == col && (st[u] < 0 || st[u] == type);
        return dead;
    };

    const T *rel = reinterpret_cast<const T *>(p.rel.ptr) + outer * p.rel.stride_outer;
    const T *x = reinterpret_cast<const T *>(p.x.ptr) + outer * p.x.stride_outer;
    T *dst = reinterpret_cast<T *>(p.out) + outer * p.out_stride_outer + (long long)row * p.out_stride_row;
    const long long bnd_row = p.bnd_rows ? p.bnd_rows[outer] : -1;

    for (int dbase = 0; dbase < p.row_len; dbase += 16 * VEC) {
        const bool dvalid = dbase + VEC * l16 < p.row_len;
        const int d0 = dvalid ? dbase + VEC * l16 : 0;
        // the consumer's delta cursor: (dj, dcol) the next live delta edge, dmsg its message, dtake: inside the operands
        int dj = j - 1, dcol = 0;
        bool dtake = false;
        P dmsg, acc;
#pragma unroll
        for (int e = 0; e < VEC; ++e) dmsg.v[e] = T(0), acc.v[e] = nary_zero<T, SUM>();
        const auto next_delta = [&]() {
            for (++dj; dj < je; ++dj) {
                if constexpr (OWNED)
                    if (!owner_live(p.d_owner[dj], outer)) continue;
                dcol = p.d_col[dj];
                int dtype = p.d_type[dj];
                if constexpr (KEYS)
                    if (smask && sample_dead(dcol, dtype)) continue;
                int c = dcol;
                dtake = !(c < 0 || c >= p.num_in || dtype < 0 || dtype >= p.num_rel);
                if (!dtake) c = 0, dtype = 0;
                const P xv = *reinterpret_cast<const P *>(x + (long long)c * p.x.stride_row + d0);
                const P rv = *reinterpret_cast<const P *>(rel + (long long)dtype * p.rel.stride_row + d0);
#pragma unroll
                for (int e = 0; e < VEC; ++e) dmsg.v[e] = binary<T, MUL>(rv.v[e], xv.v[e]);
                return;
            }
        };
        const auto add_delta = [&]() {
            if (dtake) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc.v[e] = nary<T, SUM>(acc.v[e], dmsg.v[e]);
            }
            next_delta();
        };
        if (drains) next_delta();

        int ma = 0, mb = 2, mc = 1;                       // the meta tiles of stages A, B, C: it % 3, (it - 1) % 3, (it - 2) % 3
        for (int it = 0; it < ntiles + 2; ++it) {
            if (producer) {
                if (it < ntiles && tid < HUB_TILE) {      // stage A: slot it * HUB_TILE + tid of the row
                    const long long off = (long long)it * HUB_TILE + tid;
                    int c = 0, t = 0, lv = 0;
                    if (off < n) {
                        c = p.col[i + off], t = p.type[i + off];
                        bool dead = c < 0 || c >= p.num_in || t < 0 || t >= p.num_rel;
                        if constexpr (TOMBS) {
                            int lo = q, hi = qe;          // lower bound of c among the row's keys: at most 31 halvings
                            while (lo < hi) {
                                const int mid = lo + ((hi - lo) >> 1);
                                if (p.t_col[mid] < c) lo = mid + 1; else hi = mid;
                            }
                            for (int s = lo; s < qe && p.t_col[s] == c; ++s) dead |= p.t_type[s] == t;
                        }
                        if constexpr (KEYS)
                            if (smask && !dead) dead = sample_dead(c, t);
                        lv = dead ? 0 : 1;
                    }
                    s_col[ma][tid] = c, s_type[ma][tid] = t, s_live[ma][tid] = lv;
                }
                if (it >= 1 && it <= ntiles) {            // stage B: the messages of tile it - 1
                    const int mt = (it - 1) & 1;
                    P xv[HUB_SLOTS], rv[HUB_SLOTS];
#pragma unroll
                    for (int u = 0; u < HUB_SLOTS; ++u) {
                        const int s = grp + HUB_GROUPS * u;
                        const bool lv = s_live[mb][s] != 0;
                        const int c = lv ? s_col[mb][s] : 0, t = lv ? s_type[mb][s] : 0;
                        xv[u] = *reinterpret_cast<const P *>(x + (long long)c * p.x.stride_row + d0);
                        rv[u] = *reinterpret_cast<const P *>(rel + (long long)t * p.rel.stride_row + d0);
                    }
#pragma unroll
                    for (int u = 0; u < HUB_SLOTS; ++u) {
                        P m;
#pragma unroll
                        for (int e = 0; e < VEC; ++e) m.v[e] = binary<T, MUL>(rv[u].v[e], xv[u].v[e]);
                        s_msg[mt][grp + HUB_GROUPS * u][l16] = m;
                    }
                }
            } else if (drains && it >= 2) {               // stage C: tile it - 2 into the chain
                const int mt = it & 1;
                const int cnt = (int)min((long long)HUB_TILE, n - (long long)(it - 2) * HUB_TILE);
                // (HUB_DRAIN slots' col, live flag and message are read ahead of the chain: one LDS round trip a batch, not three
                // dependent ones a slot; a slot past the row's end was written as dead by stage A)
                for (int s0 = 0; s0 < cnt; s0 += HUB_DRAIN) {
                    int c[HUB_DRAIN], lv[HUB_DRAIN];
                    P m[HUB_DRAIN];
#pragma unroll
                    for (int u = 0; u < HUB_DRAIN; ++u) {
                        c[u] = s_col[mc][s0 + u], lv[u] = s_live[mc][s0 + u];
                        m[u] = s_msg[mt][s0 + u][l16];
                    }
#pragma unroll
                    for (int u = 0; u < HUB_DRAIN; ++u) {
                        if (s0 + u < cnt) {
                            while (dj < je && dcol < c[u]) add_delta();
                            if (lv[u]) {
#pragma unroll
                                for (int e = 0; e < VEC; ++e) acc.v[e] = nary<T, SUM>(acc.v[e], m[u].v[e]);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            const int was = mc;
            mc = mb, mb = ma, ma = was;
        }
        if (drains) {
            while (dj < je) add_delta();
            if (p.has_bnd && (bnd_row < 0 || bnd_row == row)) {
                const P b = *reinterpret_cast<const P *>(reinterpret_cast<const T *>(p.bnd.ptr) + outer * p.bnd.stride_outer +
                                                         (bnd_row < 0 ? (long long)row * p.bnd.stride_row : 0) + d0);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc.v[e] = nary<T, SUM>(acc.v[e], b.v[e]);
            } else if (SUM != ULTRA_SUM_ADD && p.has_bnd) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc.v[e] = nary<T, SUM>(acc.v[e], T(0));
            }
            if (dvalid) *reinterpret_cast<P *>(dst + d0) = acc;
        }
    }
}

// The split launch: blocks [0, small_blocks) walk the touched rows of at most hub_len base edges as the kernels above do,
// block small_blocks + w is the workgroup of (touched row, outer slice) w and ends at once unless that row is a hub.
template <typename T, int SUM, int MUL, bool TOMBS, bool KEYS, bool OWNED = false, typename Params>
__device__ __forceinline__ void split_rows_roles(const Params &p, const unsigned small_blocks) {
    if (blockIdx.x < small_blocks)
        edit_rows_walk<T, SUM, MUL, TOMBS, KEYS, true, OWNED>(p);
    else
        hub_row_walk<T, SUM, MUL, TOMBS, KEYS, OWNED>(p, (long long)(blockIdx.x - small_blocks));
}
template <typename T, int SUM, int MUL>
__global__ void __launch_bounds__(DELTA_THREADS) rspmm_delta_rows_split_kernel(const DeltaParams p, const unsigned small_blocks) {
    split_rows_roles<T, SUM, MUL, false, false>(p, small_blocks);
}
template <typename T, int SUM, int MUL>
__global__ void __launch_bounds__(DELTA_THREADS) rspmm_edit_rows_split_kernel(const EditParams p, const unsigned small_blocks) {
    split_rows_roles<T, SUM, MUL, true, false>(p, small_blocks);
}
template <typename T, int SUM, int MUL>
__global__ void __launch_bounds__(DELTA_THREADS) rspmm_edit_rows_samples_split_kernel(const SampleParams p, const unsigned small_blocks) {
    split_rows_roles<T, SUM, MUL, true, true>(p, small_blocks);
}
// delta edges OWNED by outer slices (ultra_rspmm_edit_rows_owned): one launch, both roles
template <typename T, int SUM, int MUL>
__global__ void __launch_bounds__(DELTA_THREADS) rspmm_edit_rows_owned_kernel(const OwnedParams p, const unsigned small_blocks) {
    split_rows_roles<T, SUM, MUL, true, false, true>(p, small_blocks);
}

// kernel K_'s instantiations by [dtype != ULTRA_F32][sum * 2 + mul]
#define ULTRA_ROWS_KERNELS(K_)                                                                               \
    {{K_<float, 0, 0>, K_<float, 0, 1>, K_<float, 1, 0>, K_<float, 1, 1>, K_<float, 2, 0>, K_<float, 2, 1>},   \
     {K_<double, 0, 0>, K_<double, 0, 1>, K_<double, 1, 0>, K_<double, 1, 1>, K_<double, 2, 0>, K_<double, 2, 1>}}

template <typename Params>
static hipError_t launch_rows(void (*const (&kernels)[2][6])(Params), bool f32, int sum, int mul, const Params &p, unsigned grid,
                              hipStream_t s) {
    if (sum < 0 || sum > 2 || mul < 0 || mul > 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernels[f32 ? 0 : 1][sum * 2 + mul], dim3(grid), dim3(DELTA_THREADS), 0, s, p);
    return hipGetLastError();
}

template <typename Params>
static hipError_t launch_split(void (*const (&kernels)[2][6])(Params, unsigned), bool f32, int sum, int mul, const Params &p,
                               unsigned small_blocks, unsigned hub_blocks, hipStream_t s) {
    if (sum < 0 || sum > 2 || mul < 0 || mul > 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernels[f32 ? 0 : 1][sum * 2 + mul], dim3(small_blocks + hub_blocks), dim3(DELTA_THREADS), 0, s, p, small_blocks);
    return hipGetLastError();
}

static void (*const DELTA_KERNELS[2][6])(DeltaParams) = ULTRA_ROWS_KERNELS(rspmm_delta_rows_kernel);
static void (*const EDIT_KERNELS[2][6])(EditParams) = ULTRA_ROWS_KERNELS(rspmm_edit_rows_kernel);
static void (*const SAMPLES_KERNELS[2][6])(SampleParams) = ULTRA_ROWS_KERNELS(rspmm_edit_rows_samples_kernel);
static void (*const DELTA_SPLIT_KERNELS[2][6])(DeltaParams, unsigned) = ULTRA_ROWS_KERNELS(rspmm_delta_rows_split_kernel);
static void (*const EDIT_SPLIT_KERNELS[2][6])(EditParams, unsigned) = ULTRA_ROWS_KERNELS(rspmm_edit_rows_split_kernel);
static void (*const SAMPLES_SPLIT_KERNELS[2][6])(SampleParams, unsigned) = ULTRA_ROWS_KERNELS(rspmm_edit_rows_samples_split_kernel);
static void (*const OWNED_KERNELS[2][6])(OwnedParams, unsigned) = ULTRA_ROWS_KERNELS(rspmm_edit_rows_owned_kernel);
#undef ULTRA_ROWS_KERNELS

static int delta_invalid(const char *who, const std::string &msg) {
    set_error(std::string(who) + ": " + msg);
    return ULTRA_ERR_INVALID;
}
static int delta_unsupported(const char *who, const std::string &msg) {
    set_error(std::string(who) + ": " + msg);
    return ULTRA_ERR_UNSUPPORTED;
}

static int delta_check_mat(const char *who, const ultra_mat *m, const char *name, int64_t min_rows, int64_t n_outer,
                           int64_t row_len) {
    if (!m || !m->ptr) return delta_invalid(who, std::string(name) + " is NULL");
    if (m->n_outer != n_outer) return delta_invalid(who, std::string(name) + ": n_outer mismatch");
    if (m->row_len != row_len) return delta_invalid(who, std::string(name) + ": row_len mismatch");
    if (m->n_row < min_rows) return delta_invalid(who, std::string(name) + ": too few rows");
    if (m->stride_row < row_len && m->n_row > 1) return delta_invalid(who, std::string(name) + ": stride_row < row_len");
    return ULTRA_OK;
}

static bool delta_vec_ok(const ultra_mat *m, int64_t step) {
    return (reinterpret_cast<uintptr_t>(m->ptr) & 15u) == 0 && m->stride_row % step == 0 && m->stride_outer % step == 0;
}

// Every entry: the checks, then rspmm_delta_rows_kernel (removed == NULL), rspmm_edit_rows_kernel, or -- with per-slice keys --
// rspmm_edit_rows_samples_kernel (which takes removed == NULL as "no tombstones").  split: the *_split_kernel of the same
// operands instead, one launch of grid + capacity_rows * n_outer workgroups; hub_len < 0 is the plan's seg_len.
static int delta_rows_impl(const char *who, ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const ultra_mat *relation,
                           const ultra_mat *input, const ultra_mat *boundary, const int64_t *point_rows_dev,
                           const ultra_mat *output, const ultra_delta *delta, const ultra_tombstones *removed, void *stream,
                           const ultra_sample_keys *keys = nullptr, bool split = false, int64_t hub_len = INT32_MAX,
                           bool owned = false, const int32_t *owner_dev = nullptr) {
    if (!plan) return delta_invalid(who, "plan is NULL");
    if (sum < 0 || sum > 2) return delta_invalid(who, "unknown sum code");
    if (mul != ULTRA_MUL_MUL && mul != ULTRA_MUL_ADD && mul != ULTRA_MUL_ROTATE) return delta_invalid(who, "unknown mul code");
    if (dtype != ULTRA_F32 && dtype != ULTRA_F64) return delta_invalid(who, "dtype must be ULTRA_F32 or ULTRA_F64");
    if (!delta) return delta_invalid(who, "delta is NULL");
    if (delta->capacity_rows < 0 || delta->capacity_edges < 0 || delta->capacity_rows >= (1ll << 30) ||
        delta->capacity_edges >= (1ll << 30))
        return delta_invalid(who, "delta: capacities must lie in [0, 2^30)");
    if (removed && (removed->capacity_keys < 0 || removed->capacity_keys >= (1ll << 30)))
        return delta_invalid(who, "removed: capacity_keys must lie in [0, 2^30)");
    if (!output || !output->ptr) return delta_invalid(who, "output is NULL");
    const int64_t n_outer = output->n_outer, row_len = output->row_len;
    if (n_outer < 0 || row_len <= 0) return delta_invalid(who, "output: negative n_outer or empty row_len");
    if (n_outer == 0 || delta->capacity_rows == 0) return ULTRA_OK;
    if (!delta->row_dev || !delta->ptr_dev || !delta->col_dev || !delta->type_dev || !delta->count_dev)
        return delta_invalid(who, "delta: a NULL array");
    if (owned && !owner_dev) return delta_invalid(who, "owner_dev is NULL");
    // (ptr_dev is read for every touched row; the key arrays only below a non-zero capacity)
    if (removed && (!removed->ptr_dev || (removed->capacity_keys > 0 && (!removed->col_dev || !removed->type_dev))))
        return delta_invalid(who, "removed: a NULL array");
    if (keys && (!keys->row_dev || !keys->col_dev || !keys->type_dev)) return delta_invalid(who, "keys: a NULL array");
    int rc;
    if ((rc = delta_check_mat(who, output, "output", plan->num_out, n_outer, row_len))) return rc;
    if ((rc = delta_check_mat(who, relation, "relation", plan->num_rel, n_outer, row_len))) return rc;
    if ((rc = delta_check_mat(who, input, "input", plan->num_in, n_outer, row_len))) return rc;
    if (point_rows_dev && !boundary) return delta_invalid(who, "a point boundary needs its value rows");
    if (boundary && (rc = delta_check_mat(who, boundary, "boundary", point_rows_dev ? 1 : plan->num_out, n_outer, row_len)))
        return rc;
    if (mul == ULTRA_MUL_ROTATE) return delta_unsupported(who, "rotate messages are not served");
    if ((plan->flags & ULTRA_PLAN_DENSE) || !(plan->flags & ULTRA_PLAN_EXACT_ORDER))
        return delta_unsupported(who, "served by ULTRA_PLAN_EXACT_ORDER plans in the sparse format only");
    const int64_t step = dtype == ULTRA_F32 ? 4 : 2;      // elements per 16 bytes
    if (row_len % step != 0 || !delta_vec_ok(output, step) || !delta_vec_ok(relation, step) || !delta_vec_ok(input, step) ||
        (boundary && !delta_vec_ok(boundary, step)))
        return delta_unsupported(who, "rows must be whole 16-byte chunks at 16-byte aligned addresses and strides");
    if (plan->num_out == 0 || plan->num_in == 0 || plan->num_rel == 0) return ULTRA_OK;
    const int64_t groups = delta->capacity_rows * n_outer;
    const int64_t grid = (groups + DELTA_THREADS / 16 - 1) / (DELTA_THREADS / 16);
    if (grid + (split ? groups : 0) >= (1ll << 31)) return delta_invalid(who, "capacity_rows * n_outer exceeds the launch grid");
    if ((rc = ultra_plan_upload(plan))) return rc;

    OwnedParams p;
    p.d_owner = owner_dev;
    p.row_ptr = plan->d.row_ptr, p.col = plan->d.col, p.type = plan->d.type;
    p.d_row = delta->row_dev, p.d_ptr = delta->ptr_dev, p.d_col = delta->col_dev, p.d_type = delta->type_dev;
    p.d_count = delta->count_dev;
    p.cap_rows = (int32_t)delta->capacity_rows, p.cap_edges = (int32_t)delta->capacity_edges;
    p.rel = MatArg{relation->ptr, relation->stride_outer, relation->stride_row};
    p.x = MatArg{input->ptr, input->stride_outer, input->stride_row};
    p.bnd = boundary ? MatArg{boundary->ptr, boundary->stride_outer, point_rows_dev ? 0 : boundary->stride_row}
                     : MatArg{nullptr, 0, 0};
    p.bnd_rows = boundary ? reinterpret_cast<const long long *>(point_rows_dev) : nullptr;
    p.has_bnd = boundary ? 1 : 0;
    p.out = output->ptr;
    p.out_stride_outer = output->stride_outer, p.out_stride_row = output->stride_row;
    p.n_outer = (int32_t)n_outer, p.row_len = (int32_t)row_len;
    p.num_out = (int32_t)plan->num_out, p.num_in = (int32_t)plan->num_in, p.num_rel = (int32_t)plan->num_rel;
    p.num_edge = plan->num_edge;
    p.hub_len = (int32_t)std::min<int64_t>(hub_len < 0 ? plan->seg_len : hub_len, INT32_MAX);
    p.t_ptr = removed ? removed->ptr_dev : nullptr, p.t_col = removed ? removed->col_dev : nullptr;
    p.t_type = removed ? removed->type_dev : nullptr, p.cap_keys = removed ? (int32_t)removed->capacity_keys : 0;
    p.k_row = keys ? keys->row_dev : nullptr, p.k_col = keys ? keys->col_dev : nullptr;
    p.k_type = keys ? keys->type_dev : nullptr, p.per_sample = keys ? (int32_t)keys->per_sample : 0;
    if (n_outer >= (1ll << 31) || row_len >= (1ll << 31)) return delta_invalid(who, "n_outer / row_len exceed 2^31");
    (void)hipGetLastError();   // drop any stale error left by other users of the HIP runtime
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool f32 = dtype == ULTRA_F32;
    if (owned) {      // (always the split shape: both roles in one launch)
        const hipError_t e = launch_split<OwnedParams>(OWNED_KERNELS, f32, sum, mul, p, (unsigned)grid, (unsigned)groups, s);
        if (e != hipSuccess) {
            set_error(std::string("rspmm_edit_rows_owned_kernel launch: ") + hipGetErrorString(e));
            return ULTRA_ERR_HIP;
        }
        return ULTRA_OK;
    }
    if (split) {
        const unsigned hubs = (unsigned)groups;
        const hipError_t e = keys      ? launch_split<SampleParams>(SAMPLES_SPLIT_KERNELS, f32, sum, mul, p, (unsigned)grid, hubs, s)
                             : removed ? launch_split<EditParams>(EDIT_SPLIT_KERNELS, f32, sum, mul, p, (unsigned)grid, hubs, s)
                                       : launch_split<DeltaParams>(DELTA_SPLIT_KERNELS, f32, sum, mul, p, (unsigned)grid, hubs, s);
        if (e != hipSuccess) {
            set_error(std::string(keys ? "rspmm_edit_rows_samples_split_kernel" : removed ? "rspmm_edit_rows_split_kernel"
                                                                                          : "rspmm_delta_rows_split_kernel") +
                      " launch: " + hipGetErrorString(e));
            return ULTRA_ERR_HIP;
        }
        return ULTRA_OK;
    }
    const hipError_t e = keys      ? launch_rows<SampleParams>(SAMPLES_KERNELS, f32, sum, mul, p, (unsigned)grid, s)
                         : removed ? launch_rows<EditParams>(EDIT_KERNELS, f32, sum, mul, p, (unsigned)grid, s)
                                   : launch_rows<DeltaParams>(DELTA_KERNELS, f32, sum, mul, p, (unsigned)grid, s);
    if (e != hipSuccess) {
        set_error(std::string(keys ? "rspmm_edit_rows_samples_kernel" : removed ? "rspmm_edit_rows_kernel" : "rspmm_delta_rows_kernel") +
                  " launch: " + hipGetErrorString(e));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

}  // namespace ultra

using namespace ultra;

extern "C" int32_t ultra_rspmm_delta_rows(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const ultra_mat *relation,
                                          const ultra_mat *input, const ultra_mat *boundary, const int64_t *point_rows_dev,
                                          const ultra_mat *output, const ultra_delta *delta, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return delta_rows_impl("ultra_rspmm_delta_rows", plan, sum, mul, dtype, relation, input, boundary, point_rows_dev, output, delta,
                           nullptr, stream);
}

extern "C" int32_t ultra_rspmm_edit_rows(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const ultra_mat *relation,
                                         const ultra_mat *input, const ultra_mat *boundary, const int64_t *point_rows_dev,
                                         const ultra_mat *output, const ultra_delta *delta, const ultra_tombstones *removed,
                                         void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return delta_rows_impl(removed ? "ultra_rspmm_edit_rows" : "ultra_rspmm_delta_rows", plan, sum, mul, dtype, relation, input,
                           boundary, point_rows_dev, output, delta, removed, stream);
}

extern "C" int32_t ultra_rspmm_edit_rows_samples(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const ultra_mat *relation,
                                                 const ultra_mat *input, const ultra_mat *boundary, const int64_t *point_rows_dev,
                                                 const ultra_mat *output, const ultra_delta *delta, const ultra_tombstones *removed,
                                                 const ultra_sample_keys *keys, void *stream) {
    const char *who = "ultra_rspmm_edit_rows_samples";
    if (!keys) return delta_invalid(who, "keys is NULL");
    if (keys->per_sample < 1 || keys->per_sample > SAMPLE_KEYS_MAX) return delta_invalid(who, "keys: per_sample must lie in [1, 8]");
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return delta_rows_impl(who, plan, sum, mul, dtype, relation, input, boundary, point_rows_dev, output, delta, removed, stream, keys);
}

extern "C" int32_t ultra_rspmm_edit_rows_split(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const ultra_mat *relation,
                                               const ultra_mat *input, const ultra_mat *boundary, const int64_t *point_rows_dev,
                                               const ultra_mat *output, const ultra_delta *delta, const ultra_tombstones *removed,
                                               const ultra_sample_keys *keys, int64_t hub_len, void *stream) {
    const char *who = "ultra_rspmm_edit_rows_split";
    if (keys && (keys->per_sample < 1 || keys->per_sample > SAMPLE_KEYS_MAX))
        return delta_invalid(who, "keys: per_sample must lie in [1, 8]");
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return delta_rows_impl(who, plan, sum, mul, dtype, relation, input, boundary, point_rows_dev, output, delta, removed, stream, keys,
                           true, hub_len);
}

extern "C" int32_t ultra_rspmm_edit_rows_owned(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const ultra_mat *relation,
                                               const ultra_mat *input, const ultra_mat *boundary, const int64_t *point_rows_dev,
                                               const ultra_mat *output, const ultra_delta *delta, const int32_t *owner_dev,
                                               const ultra_tombstones *removed, int64_t hub_len, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return delta_rows_impl("ultra_rspmm_edit_rows_owned", plan, sum, mul, dtype, relation, input, boundary, point_rows_dev, output,
                           delta, removed, stream, nullptr, true, hub_len, true, owner_dev);
}

extern "C" int32_t ultra_rspmm_hub_tile(void) { return HUB_TILE; }
