// One layer of the path beam search of BaseNBFNet.visualize (reference: ultra/base_nbfnet.py:173-232), with the
// semantics of DESIGN.md §9 -- the reference's with stable sorts and exact top-k keys:
//
//   candidates of destination v: (e, b) for every in-edge e of v whose source is not t, ascending edge id, then beam b;
//   m(e, b)      = dist_in[src(e), b] + grad[e]                                     (one fp32 add)
//   prev_rank    = smallest j with isclose(m(e, b), m(e, j)) (torch's default isclose on fp32), 0 if none
//   dropped      : same (src, dst, type, prev_rank) as the candidate directly before it (before any removal)
//   kept         : the top K survivors by value, descending, ties to the earlier candidate; -inf ranks last and ties;
//                  fewer than K survivors: padded with the last one kept; none: -inf and (0, 0, 0, 0).
//
// Input: a destination-major CSR whose slots keep ascending edge id within each row (built once per graph by the host
// layer: a stable sort by destination).  One wave per row scans its candidates in order, keeping the running top K in
// lanes 0..K-1 (lane = rank): each edge's K candidates are merged by counting ranks (a permutation of the union, so the
// kept entries land in distinct LDS slots) -- no atomics, one writer per destination, deterministic.  Rows of in-degree
// above ULTRA_BEAM_HUB_DEGREE go to a second kernel: one workgroup of 16 waves per row, each wave scanning a contiguous
// slice, then wave 0 merging the 16 partial lists in slice order (ties to the earlier slice = the earlier candidate).
//
// ultra_beam_search_layer_batch: S independent searches over the same CSR.  The sample is blockIdx.y of both kernels --
// each workgroup offsets the gradients, distances and outputs to its sample's slice and reads its sample's tail from a
// device array -- so a layer stays two launches, the per-row work (and with it every bit of the result) is the single
// entry's, and S searches fill S times as many workgroups: the hub kernel's 97 workgroups at FB15k237 become 97 S.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "../../include/ultra_rspmm.h"
#include "plan.hpp"
#include "device_scope.hpp"

namespace ultra {

constexpr int BEAM_ROW_WAVES = 4;     // rows per workgroup of the row kernel
constexpr int BEAM_HUB_WAVES = 16;    // waves per hub row

// torch.isclose(a, b) with rtol = 1e-5, atol = 1e-8 on fp32 (ATen: close = a == b | isfinite(|a - b|) & |a - b| <= atol + |rtol * b|)
__device__ __forceinline__ bool beam_isclose(float a, float b) {
    if (a == b) return true;
    const float err = fabsf(a - b);
    const float allowed = 1e-8f + fabsf(1e-5f * b);
    return isfinite(err) && err <= allowed;
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct BeamLds {
    float v[64];
    int src[64];
    int ty[64];
    int pr[64];
};

// running top-K of one wave: lane i < cnt holds the i-th best entry
struct BeamState {
    float v;
    int src, ty, pr;
    int cnt;    // wave-uniform
};

// Merge K new entries (lane b: value m, valid flag; ties among them go to the lower lane) into the state (whose entries all
// precede the new ones in candidate order, so they win ties).
__device__ __forceinline__ void beam_merge(BeamState &st, float m, bool valid, int src, int ty, int pr, int K, int lane,
                                           BeamLds &lds) {
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0ull) return;
    if (st.cnt == K) {
        const float last = __shfl(st.v, K - 1);
        if (!__any(valid && m > last)) return;     // nothing beats the K-th entry (ties stay with the state)
    }
    int rank_s = lane, rank_n = 0;
    for (int j = 0; j < K; ++j) {
        const float mj = __shfl(m, j);
        const float sj = __shfl(st.v, j);
        const bool vj = (vmask >> j) & 1ull;
        if (vj && mj > st.v) ++rank_s;
        if (j < st.cnt && sj >= m) ++rank_n;
        if (vj && j != lane && (mj > m || (mj == m && j < lane))) ++rank_n;
    }
    if (lane < st.cnt && rank_s < K) {
        lds.v[rank_s] = st.v;
        lds.src[rank_s] = st.src;
        lds.ty[rank_s] = st.ty;
        lds.pr[rank_s] = st.pr;
    }
    if (valid && rank_n < K) {
        lds.v[rank_n] = m;
        lds.src[rank_n] = src;
        lds.ty[rank_n] = ty;
        lds.pr[rank_n] = pr;
    }
    const int total = st.cnt + __popcll(vmask);
    st.cnt = total < K ? total : K;
    wave_lds_sync();
    if (lane < st.cnt) {
        st.v = lds.v[lane];
        st.src = lds.src[lane];
        st.ty = lds.ty[lane];
        st.pr = lds.pr[lane];
    }
    wave_lds_sync();
}

// prev_rank of lane b's candidate among the K candidates of one edge
__device__ __forceinline__ int beam_prev_rank(float m, int K) {
    int pr = 0;
    bool found = false;
    for (int j = 0; j < K; ++j) {
        const float mj = __shfl(m, j);
        if (!found && beam_isclose(m, mj)) {
            pr = j;
            found = true;
        }
    }
    return pr;
}

struct BeamArgs {
    const int64_t *row_ptr;
    const int32_t *src;
    const int32_t *type;
    const int32_t *eid;
    const float *grad;
    const float *dist_in;
    float *dist_out;
    int64_t *back_out;
    const int64_t *hub_rows;
    const int64_t *tails;      // per sample, on the device (ultra_beam_search_layer_batch); NULL: `tail` for the one sample
    int64_t num_node;
    int64_t num_edge;
    int64_t tail;
    int32_t K;
};

// The arguments of sample s (blockIdx.y): its slice of the gradients, distances and outputs, and its own tail.  The tail is
// only ever compared with source ids, never used as an index.
__device__ __forceinline__ BeamArgs beam_sample(BeamArgs a, int64_t s) {
    if (a.tails) a.tail = a.tails[s];
    const int64_t nk = a.num_node * a.K;
    a.grad += s * a.num_edge;
    a.dist_in += s * nk;
    a.dist_out += s * nk;
    a.back_out += s * nk * 4;
    return a;
}

// Where a scan takes its candidates from.  src_at(q): the source of slot q, or the sample's tail for a slot that takes no part
// (the scan skips a tail-sourced slot, and it never becomes "the candidate directly before"); rest(q, ty, g): the slot's type
// and gradient.  BaseSlots: the CSR's own slots.
struct BaseSlots {
    const BeamArgs &a;
    __device__ __forceinline__ int src_at(int64_t q) const { return a.src[q]; }
    __device__ __forceinline__ void rest(int64_t q, int &ty, float &g) const {
        ty = a.type[q];
        g = a.grad[a.eid[q]];
    }
};

// Scan slots [pb, pe) of row v into `st`.  The carry (the candidate directly before slot pb's first one) is computed from
// the row's slots before pb.
template <typename Slots>
__device__ void beam_scan(const BeamArgs &a, const Slots &slots, int64_t v, int64_t row_begin, int64_t pb, int64_t pe,
                          BeamState &st, int lane, BeamLds &lds) {
    const int K = a.K;
    const int t = (int)a.tail;
    bool has_prev = false;
    int prev_src = 0, prev_ty = 0, prev_pr = 0;
    {
        int64_t q = pb - 1;
        while (q >= row_begin && slots.src_at(q) == t) --q;
        if (q >= row_begin) {
            const int s = slots.src_at(q);
            int ty;
            float gv;
            slots.rest(q, ty, gv);
            const float m = lane < K ? a.dist_in[(int64_t)s * K + lane] + gv : -INFINITY;
            const int pr = beam_prev_rank(m, K);
            has_prev = true;
            prev_src = s;
            prev_ty = ty;
            prev_pr = __shfl(pr, K - 1);
        }
    }
    for (int64_t c0 = pb; c0 < pe; c0 += 64) {
        // the chunk's slots, one per lane (coalesced), handed out with shuffles
        const int64_t n = pe - c0 < 64 ? pe - c0 : 64;
        int my_src = t, my_ty = 0;
        float my_g = 0.f;
        if (lane < n) {
            my_src = slots.src_at(c0 + lane);
            slots.rest(c0 + lane, my_ty, my_g);
        }
        int s_next = __shfl(my_src, 0);
        float d_next = (lane < K && s_next != t) ? a.dist_in[(int64_t)s_next * K + lane] : -INFINITY;
        for (int c = 0; c < (int)n; ++c) {
            const int s = s_next;
            const float d = d_next;
            if (c + 1 < (int)n) {       // the next edge's beams in flight while this one is merged
                s_next = __shfl(my_src, c + 1);
                d_next = (lane < K && s_next != t) ? a.dist_in[(int64_t)s_next * K + lane] : -INFINITY;
            }
            if (s == t) continue;       // no path leaves t once it has arrived there (base_nbfnet.py:178-183)
            const int ty = __shfl(my_ty, c);
            const float gv = __shfl(my_g, c);
            const float m = lane < K ? d + gv : -INFINITY;
            const int pr = beam_prev_rank(m, K);
            const int pr_before = __shfl_up(pr, 1);
            bool dup;
            if (lane == 0)
                dup = has_prev && prev_src == s && prev_ty == ty && prev_pr == pr;
            else
                dup = pr == pr_before;
            const bool valid = lane < K && !dup;
            has_prev = true;
            prev_src = s;
            prev_ty = ty;
            prev_pr = __shfl(pr, K - 1);
            beam_merge(st, m, valid, s, ty, pr, K, lane, lds);
        }
    }
    (void)v;
}

__device__ __forceinline__ void beam_write(const BeamArgs &a, int64_t v, const BeamState &st, int lane) {
    const int K = a.K;
    const int last = st.cnt > 0 ? st.cnt - 1 : 0;
    const float pv = __shfl(st.v, last);
    const int psrc = __shfl(st.src, last), pty = __shfl(st.ty, last), ppr = __shfl(st.pr, last);
    if (lane >= K) return;
    float val;
    int64_t s, d, ty, pr;
    if (st.cnt == 0) {
        val = -INFINITY;
        s = d = ty = pr = 0;
    } else if (lane < st.cnt) {
        val = st.v;
        s = st.src;
        d = v;
        ty = st.ty;
        pr = st.pr;
    } else {
        val = pv;
        s = psrc;
        d = v;
        ty = pty;
        pr = ppr;
    }
    const int64_t o = v * K + lane;
    a.dist_out[o] = val;
    int64_t *be = a.back_out + o * 4;
    be[0] = s;
    be[1] = d;
    be[2] = ty;
    be[3] = pr;
}

__global__ void __launch_bounds__(64 * BEAM_ROW_WAVES) beam_row_kernel(BeamArgs all) {
    __shared__ BeamLds lds[BEAM_ROW_WAVES];
    const BeamArgs a = beam_sample(all, blockIdx.y);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * BEAM_ROW_WAVES + wave;
    if (v >= a.num_node) return;
    const int64_t rb = a.row_ptr[v], re = a.row_ptr[v + 1];
    if (re - rb > ULTRA_BEAM_HUB_DEGREE) return;       // beam_hub_kernel's row
    BeamState st;
    st.v = -INFINITY;
    st.src = st.ty = st.pr = 0;
    st.cnt = 0;
    beam_scan(a, BaseSlots{a}, v, rb, rb, re, st, lane, lds[wave]);
    beam_write(a, v, st, lane);
}

// The end of a sliced row: every wave parks its partial list, wave 0 merges them in slice order (ties to the earlier slice =
// the earlier candidate) and writes the row.
__device__ __forceinline__ void beam_merge_slices(const BeamArgs &a, int64_t v, BeamState &st, int wave, int lane,
                                                  BeamLds *scratch, BeamLds *part, int *part_cnt) {
    part[wave].v[lane] = st.v;
    part[wave].src[lane] = st.src;
    part[wave].ty[lane] = st.ty;
    part[wave].pr[lane] = st.pr;
    if (lane == 0) part_cnt[wave] = st.cnt;
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < BEAM_HUB_WAVES; ++w) {
        const int n = part_cnt[w];
        const bool valid = lane < n;
        beam_merge(st, part[w].v[lane], valid, part[w].src[lane], part[w].ty[lane], part[w].pr[lane], a.K, lane, scratch[0]);
    }
    beam_write(a, v, st, lane);
}

__global__ void __launch_bounds__(64 * BEAM_HUB_WAVES) beam_hub_kernel(BeamArgs all) {
    const BeamArgs a = beam_sample(all, blockIdx.y);
    __shared__ BeamLds scratch[BEAM_HUB_WAVES];
    __shared__ BeamLds part[BEAM_HUB_WAVES];
    __shared__ int part_cnt[BEAM_HUB_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t v = a.hub_rows[blockIdx.x];
    const int64_t rb = a.row_ptr[v], re = a.row_ptr[v + 1];
    const int64_t per = (re - rb + BEAM_HUB_WAVES - 1) / BEAM_HUB_WAVES;
    const int64_t pb = rb + per * wave < re ? rb + per * wave : re;
    const int64_t pe = pb + per < re ? pb + per : re;
    BeamState st;
    st.v = -INFINITY;
    st.src = st.ty = st.pr = 0;
    st.cnt = 0;
    beam_scan(a, BaseSlots{a}, v, rb, pb, pe, st, lane, scratch[wave]);
    beam_merge_slices(a, v, st, wave, lane, scratch, part, part_cnt);
}

// ---- the touched rows of a graph delta (ultra_beam_search_edit_rows_batch) ----
// The slots of touched row v on the MATERIALISED graph: positions [rb, re) are the row's base slots, where a slot whose
// (src, type) is among the row's dead keys answers with the tail (it takes no part); positions [re, re + added) are the row's
// added edges in ascending j, the materialised list's order.  An added edge with an index outside the operands takes no part.
struct BeamEdits {
    const int32_t *rows, *count, *add_ptr, *add_src, *add_type, *add_j, *dead_ptr, *dead_src, *dead_type;
    const float *add_grad;         // (num_sample, add_grad_stride)
    int64_t add_grad_stride;
    int32_t cap_rows, cap_edges, cap_keys;
};

struct EditSlots {
    const BeamArgs &a;
    const BeamEdits &e;
    const float *add_grad;         // this sample's row of the added gradients
    int64_t re;                    // the end of the base slots
    int ab, kb, ke;                // the row's first added edge, its dead-key range
    __device__ __forceinline__ bool dead(int s, int ty) const {
        int lo = kb, hi = ke;      // the first key >= (s, ty)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int ks = e.dead_src[mid], kt = e.dead_type[mid];
            if (ks < s || (ks == s && kt < ty)) lo = mid + 1;
            else hi = mid;
        }
        return lo < ke && e.dead_src[lo] == s && e.dead_type[lo] == ty;
    }
    __device__ __forceinline__ int src_at(int64_t q) const {
        const int t = (int)a.tail;
        if (q < re) {
            const int s = a.src[q];
            return (kb < ke && dead(s, a.type[q])) ? t : s;
        }
        const int64_t at = ab + (q - re);
        const int s = e.add_src[at], j = e.add_j[at];
        return (s < 0 || s >= a.num_node || j < 0 || j >= e.cap_edges) ? t : s;
    }
    __device__ __forceinline__ void rest(int64_t q, int &ty, float &g) const {
        if (q < re) {
            ty = a.type[q];
            g = a.grad[a.eid[q]];
            return;
        }
        const int64_t at = ab + (q - re);
        const int j = e.add_j[at];
        ty = e.add_type[at];
        g = (j >= 0 && j < e.cap_edges) ? add_grad[j] : 0.f;
    }
};

// One workgroup per (touched row, sample), the hub kernel's shape whatever the row's degree: sixteen contiguous slices of the
// base slots, the added edges as the tail of the last one.  Overwrites what the base launch wrote for the row.
__global__ void __launch_bounds__(64 * BEAM_HUB_WAVES) beam_edit_rows_kernel(BeamArgs all, BeamEdits e) {
    __shared__ BeamLds scratch[BEAM_HUB_WAVES];
    __shared__ BeamLds part[BEAM_HUB_WAVES];
    __shared__ int part_cnt[BEAM_HUB_WAVES];
    const int k = blockIdx.x;
    const int live = min(max(*e.count, 0), e.cap_rows);
    if (k >= live) return;                                 // (the whole workgroup)
    const BeamArgs a = beam_sample(all, blockIdx.y);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t v = e.rows[k];
    if (v < 0 || v >= a.num_node) return;                  // (a delta of another graph: nothing is written)
    const int64_t rb = a.row_ptr[v], re = a.row_ptr[v + 1];
    if (rb < 0 || re < rb || re > a.num_edge) return;
    EditSlots slots{a, e, e.add_grad + (int64_t)blockIdx.y * e.add_grad_stride, re, 0, 0, 0};
    slots.ab = min(max(e.add_ptr[k], 0), e.cap_edges);
    const int ae = min(max(e.add_ptr[k + 1], slots.ab), e.cap_edges);
    slots.kb = min(max(e.dead_ptr[k], 0), e.cap_keys);
    slots.ke = min(max(e.dead_ptr[k + 1], slots.kb), e.cap_keys);
    const int64_t per = (re - rb + BEAM_HUB_WAVES - 1) / BEAM_HUB_WAVES;
    const int64_t pb = rb + per * wave < re ? rb + per * wave : re;
    int64_t pe = pb + per < re ? pb + per : re;
    if (wave == BEAM_HUB_WAVES - 1) pe = re + (ae - slots.ab);
    BeamState st;
    st.v = -INFINITY;
    st.src = st.ty = st.pr = 0;
    st.cnt = 0;
    beam_scan(a, slots, v, rb, pb, pe, st, lane, scratch[wave]);
    beam_merge_slices(a, v, st, wave, lane, scratch, part, part_cnt);
}

}  // namespace ultra

namespace ultra {

// Both entry points: `num_sample` slices (the grid's y dimension) of one layer -- two launches whatever num_sample is.
static int32_t beam_launch(const char *who, const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                           const int32_t *csr_eid, const int64_t *hub_rows, int64_t num_hub, int64_t num_node, int64_t num_edge,
                           int64_t num_sample, const void *edge_grad, const void *dist_in, const int64_t *tails, int64_t tail,
                           int32_t num_beam, void *dist_out, int64_t *back_edge_out, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, dist_out);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    BeamArgs a;
    a.row_ptr = row_ptr;
    a.src = csr_src;
    a.type = csr_type;
    a.eid = csr_eid;
    a.grad = (const float *)edge_grad;
    a.dist_in = (const float *)dist_in;
    a.dist_out = (float *)dist_out;
    a.back_out = back_edge_out;
    a.hub_rows = hub_rows;
    a.tails = tails;
    a.num_node = num_node;
    a.num_edge = num_edge;
    a.tail = tail;
    a.K = num_beam;
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    const unsigned grid = (unsigned)((num_node + BEAM_ROW_WAVES - 1) / BEAM_ROW_WAVES);
    hipLaunchKernelGGL(beam_row_kernel, dim3(grid, (unsigned)num_sample), dim3(64 * BEAM_ROW_WAVES), 0, s, a);
    if (num_hub > 0)
        hipLaunchKernelGGL(beam_hub_kernel, dim3((unsigned)num_hub, (unsigned)num_sample), dim3(64 * BEAM_HUB_WAVES), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string(who) + " launch: " + hipGetErrorString(e));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

}  // namespace ultra

extern "C" int32_t ultra_beam_search_layer(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                           const int32_t *csr_eid, const int64_t *hub_rows, int64_t num_hub,
                                           int64_t num_node, int64_t num_edge, const void *edge_grad, const void *dist_in,
                                           int64_t tail, int32_t num_beam, void *dist_out, int64_t *back_edge_out,
                                           void *stream) {
    if (num_beam < 1 || num_beam > ULTRA_BEAM_MAX) {
        ultra::set_error("ultra_beam_search_layer: num_beam must be in [1, 64]");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (!row_ptr || !dist_out || !back_edge_out || !dist_in || num_node <= 0 || num_edge < 0 || num_hub < 0
        || num_node >= INT32_MAX || num_edge >= INT32_MAX || (num_hub > 0 && !hub_rows)
        || (num_edge > 0 && (!csr_src || !csr_type || !csr_eid || !edge_grad)) || tail < 0 || tail >= num_node) {
        ultra::set_error("ultra_beam_search_layer: NULL operand, empty graph or tail out of range");
        return ULTRA_ERR_INVALID;
    }
    return ultra::beam_launch("beam search", row_ptr, csr_src, csr_type, csr_eid, hub_rows, num_hub, num_node, num_edge, 1, edge_grad,
                              dist_in, nullptr, tail, num_beam, dist_out, back_edge_out, stream);
}

extern "C" int32_t ultra_beam_search_layer_batch(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                                 const int32_t *csr_eid, const int64_t *hub_rows, int64_t num_hub,
                                                 int64_t num_node, int64_t num_edge, int64_t num_sample, const void *edge_grad,
                                                 const void *dist_in, const int64_t *tails, int32_t num_beam, void *dist_out,
                                                 int64_t *back_edge_out, void *stream) {
    if (num_beam < 1 || num_beam > ULTRA_BEAM_MAX) {
        ultra::set_error("ultra_beam_search_layer_batch: num_beam must be in [1, 64]");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (num_sample < 0 || num_sample > 65535) {
        ultra::set_error("ultra_beam_search_layer_batch: num_sample must be in [0, 65535]");
        return ULTRA_ERR_INVALID;
    }
    if (num_sample == 0) return ULTRA_OK;
    if (!tails) {
        ultra::set_error("ultra_beam_search_layer_batch: tails is NULL");
        return ULTRA_ERR_INVALID;
    }
    if (!row_ptr || !dist_out || !back_edge_out || !dist_in || num_node <= 0 || num_edge < 0 || num_hub < 0
        || num_node >= INT32_MAX || num_edge >= INT32_MAX || (num_hub > 0 && !hub_rows)
        || (num_edge > 0 && (!csr_src || !csr_type || !csr_eid || !edge_grad))) {
        ultra::set_error("ultra_beam_search_layer_batch: NULL operand (row_ptr, csr, edge_grad, dist_in, dist_out, back_edge_out) "
                         "or empty graph");
        return ULTRA_ERR_INVALID;
    }
    return ultra::beam_launch("batched beam search", row_ptr, csr_src, csr_type, csr_eid, hub_rows, num_hub, num_node, num_edge,
                              num_sample, edge_grad, dist_in, tails, 0, num_beam, dist_out, back_edge_out, stream);
}

extern "C" int32_t ultra_beam_search_edit_rows_batch(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                                     const int32_t *csr_eid, int64_t num_node, int64_t num_edge,
                                                     int64_t num_sample, const void *edge_grad, const ultra_explain_edits *edits,
                                                     const void *added_grad, int64_t added_grad_stride, const void *dist_in,
                                                     const int64_t *tails, int32_t num_beam, void *dist_out,
                                                     int64_t *back_edge_out, void *stream) {
    const char *who = "ultra_beam_search_edit_rows_batch";
    if (num_beam < 1 || num_beam > ULTRA_BEAM_MAX) {
        ultra::set_error(std::string(who) + ": num_beam must be in [1, 64]");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (num_sample < 0 || num_sample > 65535) {
        ultra::set_error(std::string(who) + ": num_sample must be in [0, 65535]");
        return ULTRA_ERR_INVALID;
    }
    if (!edits || edits->capacity_rows < 0 || edits->capacity_edges < 0 || edits->capacity_keys < 0 ||
        edits->capacity_rows >= (1ll << 30) || edits->capacity_edges >= (1ll << 30) || edits->capacity_keys >= (1ll << 30)) {
        ultra::set_error(std::string(who) + ": edits is NULL or a capacity lies outside [0, 2^30)");
        return ULTRA_ERR_INVALID;
    }
    if (num_sample == 0 || edits->capacity_rows == 0) return ULTRA_OK;
    if (!tails || !row_ptr || !dist_out || !back_edge_out || !dist_in || num_node <= 0 || num_edge < 0 || num_node >= INT32_MAX ||
        num_edge >= INT32_MAX || (num_edge > 0 && (!csr_src || !csr_type || !csr_eid || !edge_grad)) || !edits->row_dev ||
        !edits->count_dev || !edits->add_ptr_dev || !edits->dead_ptr_dev ||
        (edits->capacity_edges > 0 && (!edits->add_src_dev || !edits->add_type_dev || !edits->add_j_dev || !added_grad)) ||
        (edits->capacity_keys > 0 && (!edits->dead_src_dev || !edits->dead_type_dev)) ||
        added_grad_stride < edits->capacity_edges) {
        ultra::set_error(std::string(who) + ": NULL operand, empty graph, or added_grad_stride < capacity_edges");
        return ULTRA_ERR_INVALID;
    }
    ULTRA_DEVICE_SCOPE(stream, dist_out);
    ultra::BeamArgs a;
    a.row_ptr = row_ptr;
    a.src = csr_src;
    a.type = csr_type;
    a.eid = csr_eid;
    a.grad = (const float *)edge_grad;
    a.dist_in = (const float *)dist_in;
    a.dist_out = (float *)dist_out;
    a.back_out = back_edge_out;
    a.hub_rows = nullptr;
    a.tails = tails;
    a.num_node = num_node;
    a.num_edge = num_edge;
    a.tail = 0;
    a.K = num_beam;
    ultra::BeamEdits e;
    e.rows = edits->row_dev, e.count = edits->count_dev, e.add_ptr = edits->add_ptr_dev, e.add_src = edits->add_src_dev;
    e.add_type = edits->add_type_dev, e.add_j = edits->add_j_dev, e.dead_ptr = edits->dead_ptr_dev;
    e.dead_src = edits->dead_src_dev, e.dead_type = edits->dead_type_dev;
    e.add_grad = (const float *)added_grad;
    e.add_grad_stride = added_grad_stride;
    e.cap_rows = (int32_t)edits->capacity_rows, e.cap_edges = (int32_t)edits->capacity_edges;
    e.cap_keys = (int32_t)edits->capacity_keys;
    (void)hipGetLastError();   // drop any stale error left by other users of the runtime
    hipLaunchKernelGGL(ultra::beam_edit_rows_kernel, dim3((unsigned)edits->capacity_rows, (unsigned)num_sample),
                       dim3(64 * ultra::BEAM_HUB_WAVES), 0, reinterpret_cast<hipStream_t>(stream), a, e);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        ultra::set_error(std::string(who) + " launch: " + hipGetErrorString(err));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}
