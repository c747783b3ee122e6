// The differentiable aggregate of the explanation route on (base graph, delta) (include/ultra_rspmm.h: ultra_explain_edits;
// DESIGN.md 27).  The base plan's forward / backward run with the tombstones' 0 / 1 keep vector as edge weights, so a dead
// edge is absent exactly; the launches here add what the delta's ADDED edges contribute:
//
//   ultra_rspmm_delta_edges_forward          output[s, dst]     += sum_j relation[s, type_j] * input[s, src_j]        (by destination)
//   ultra_rspmm_delta_edges_backward_input   input_grad[s, src] += sum_j relation[s, type_j] * output_grad[s, dst_j]  (by source)
//   ultra_rspmm_delta_edge_grad_samples      weight_grad[s, j]   = sum_d output_grad[s, dst_j, d] * (relation[s, type_j, d] * input[s, src_j, d])
//
// The first two are ONE kernel over a (rows, ptr, other end, type) layout: a 16-lane group per (touched row, outer slice), as in
// delta_kernels.hip, sums the row's messages in ascending j -- the order the layout stores them in -- and adds the total to the
// row with one add.  One writer per (row, slice), no atomics, the same bits run to run.  Rows wider than 64 floats take further
// trips of the same group.  The grids are sized by the layout's CAPACITY; the live counts are read from device memory and the
// groups beyond them end at once, so nothing is read on the host.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_rspmm.h"
#include "device_scope.hpp"
#include "plan.hpp"

namespace ultra {

constexpr int XL_THREADS = 256;      // sixteen 16-lane groups (or four waves) a workgroup

struct XlMat {
    const float *ptr;
    long long so, sr;
};

struct XlRowsParams {
    const int32_t *rows, *count, *ptr, *other, *type;
    int32_t cap_rows, cap_edges;
    XlMat rel, x;
    float *out;
    long long out_so, out_sr;
    int32_t n_outer, row_len, num_node, num_rel;
};

__global__ void __launch_bounds__(XL_THREADS) delta_edges_rows_kernel(const XlRowsParams p) {
    const int l16 = threadIdx.x & 15;
    const long long group = (long long)blockIdx.x * (XL_THREADS / 16) + (threadIdx.x >> 4);
    const int k = (int)(group / p.n_outer), outer = (int)(group - (long long)k * p.n_outer);
    const int live = min(max(*p.count, 0), p.cap_rows);
    if (k >= live) return;
    const int row = p.rows[k];
    if (row < 0 || row >= p.num_node) return;
    const int j = min(max(p.ptr[k], 0), p.cap_edges);
    const int je = min(max(p.ptr[k + 1], j), p.cap_edges);
    if (j == je) return;      // (a row touched by removals only: the keep vector has served it)
    const float *rel = p.rel.ptr + outer * p.rel.so;
    const float *x = p.x.ptr + outer * p.x.so;
    float *dst = p.out + outer * p.out_so + (long long)row * p.out_sr;
    for (int d0 = 4 * l16; d0 < p.row_len; d0 += 64) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int e = j; e < je; ++e) {
            const int c = p.other[e], t = p.type[e];
            if (c < 0 || c >= p.num_node || t < 0 || t >= p.num_rel) continue;      // (never dereferenced)
            const float4 xv = *reinterpret_cast<const float4 *>(x + (long long)c * p.x.sr + d0);
            const float4 rv = *reinterpret_cast<const float4 *>(rel + (long long)t * p.rel.sr + d0);
            acc.x += rv.x * xv.x;
            acc.y += rv.y * xv.y;
            acc.z += rv.z * xv.z;
            acc.w += rv.w * xv.w;
        }
        float4 o = *reinterpret_cast<const float4 *>(dst + d0);
        o.x += acc.x;
        o.y += acc.y;
        o.z += acc.z;
        o.w += acc.w;
        *reinterpret_cast<float4 *>(dst + d0) = o;
    }
}

struct XlGradParams {
    const int32_t *count, *add_ptr, *src, *dst, *type, *j;
    int32_t cap_rows, cap_edges;
    XlMat rel, x, og;
    float *wgrad;
    long long wgrad_so;
    int32_t row_len, num_node, num_rel;
};

__global__ void __launch_bounds__(XL_THREADS) delta_edge_grad_samples_kernel(const XlGradParams p) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (XL_THREADS / 64) + (threadIdx.x >> 6);
    const int outer = blockIdx.y;
    if (slot >= p.cap_edges) return;
    float *wg = p.wgrad + outer * p.wgrad_so;
    const int live = min(max(*p.count, 0), p.cap_rows);
    const int total = min(max(p.add_ptr[live], 0), p.cap_edges);      // the live number of added edges
    if (slot >= total) {      // (the columns at or above it: the slots' j are a permutation of [0, total))
        if (lane == 0) wg[slot] = 0.f;
        return;
    }
    const int s = p.src[slot], d = p.dst[slot], t = p.type[slot], j = p.j[slot];
    if (j < 0 || j >= p.cap_edges) return;
    float sum = 0.f;
    if (s >= 0 && s < p.num_node && d >= 0 && d < p.num_node && t >= 0 && t < p.num_rel) {
        const float *rel = p.rel.ptr + outer * p.rel.so + (long long)t * p.rel.sr;
        const float *x = p.x.ptr + outer * p.x.so + (long long)s * p.x.sr;
        const float *og = p.og.ptr + outer * p.og.so + (long long)d * p.og.sr;
        for (int e = lane; e < p.row_len; e += 64) sum += og[e] * (rel[e] * x[e]);
    }
    sum += __shfl_xor(sum, 32);
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 8);
    sum += __shfl_xor(sum, 4);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 1);
    if (lane == 0) wg[j] = sum;
}

static int xl_invalid(const char *who, const std::string &msg) {
    set_error(std::string(who) + ": " + msg);
    return ULTRA_ERR_INVALID;
}

static int xl_unsupported(const char *who, const std::string &msg) {
    set_error(std::string(who) + ": " + msg);
    return ULTRA_ERR_UNSUPPORTED;
}

// 0 = fine; the operand is (n_outer, n_row, row_len) fp32
static int xl_check_mat(const char *who, const ultra_mat *m, const char *name, int64_t n_outer, int64_t row_len) {
    if (!m || !m->ptr) return xl_invalid(who, std::string(name) + " is NULL");
    if (m->n_outer != n_outer) return xl_invalid(who, std::string(name) + ": n_outer mismatch");
    if (m->row_len != row_len) return xl_invalid(who, std::string(name) + ": row_len mismatch");
    if (m->n_row < 1 || m->n_row >= (1ll << 31)) return xl_invalid(who, std::string(name) + ": n_row must lie in [1, 2^31)");
    if (m->stride_row < row_len && m->n_row > 1) return xl_invalid(who, std::string(name) + ": stride_row < row_len");
    return ULTRA_OK;
}

static bool xl_vec_ok(const ultra_mat *m) {
    return (reinterpret_cast<uintptr_t>(m->ptr) & 15u) == 0 && m->stride_row % 4 == 0 && m->stride_outer % 4 == 0;
}

static int xl_check_edits(const char *who, const ultra_explain_edits *e) {
    if (!e) return xl_invalid(who, "edits is NULL");
    if (e->capacity_rows < 0 || e->capacity_edges < 0 || e->capacity_keys < 0 || e->capacity_rows >= (1ll << 30) ||
        e->capacity_edges >= (1ll << 30) || e->capacity_keys >= (1ll << 30))
        return xl_invalid(who, "edits: capacities must lie in [0, 2^30)");
    return ULTRA_OK;
}

static XlMat xl_mat(const ultra_mat *m) { return XlMat{reinterpret_cast<const float *>(m->ptr), m->stride_outer, m->stride_row}; }

// ultra_rspmm_delta_edges_forward / _backward_input: `out` rows get the messages of the layout (rows, count, ptr, other, type)
static int xl_rows(const char *who, const ultra_explain_edits *e, bool by_source, const ultra_mat *relation, const ultra_mat *x,
                   const ultra_mat *out, void *stream) {
    int rc;
    if ((rc = xl_check_edits(who, e))) return rc;
    if (!out || !out->ptr) return xl_invalid(who, "the written operand is NULL");
    const int64_t n_outer = out->n_outer, row_len = out->row_len;
    if (n_outer < 0 || n_outer >= (1ll << 31) || row_len <= 0 || row_len >= (1ll << 31))
        return xl_invalid(who, "n_outer / row_len outside [0, 2^31)");
    if (n_outer == 0 || e->capacity_rows == 0 || e->capacity_edges == 0) return ULTRA_OK;
    const int32_t *rows = by_source ? e->src_row_dev : e->row_dev, *count = by_source ? e->src_count_dev : e->count_dev;
    const int32_t *ptr = by_source ? e->src_ptr_dev : e->add_ptr_dev, *other = by_source ? e->src_dst_dev : e->add_src_dev;
    const int32_t *type = by_source ? e->src_type_dev : e->add_type_dev;
    if (!rows || !count || !ptr || !other || !type) return xl_invalid(who, "edits: a NULL array");
    if ((rc = xl_check_mat(who, out, "the written operand", n_outer, row_len))) return rc;
    if ((rc = xl_check_mat(who, relation, "relation", n_outer, row_len))) return rc;
    if ((rc = xl_check_mat(who, x, "the read operand", n_outer, row_len))) return rc;
    if (x->n_row != out->n_row) return xl_invalid(who, "input and output must have the graph's num_node rows each");
    if (row_len % 4 != 0 || !xl_vec_ok(out) || !xl_vec_ok(relation) || !xl_vec_ok(x))
        return xl_unsupported(who, "rows must be whole 16-byte chunks at 16-byte aligned addresses and strides");
    const int64_t groups = e->capacity_rows * n_outer;
    const int64_t grid = (groups + XL_THREADS / 16 - 1) / (XL_THREADS / 16);
    if (grid >= (1ll << 31)) return xl_invalid(who, "capacity_rows * n_outer exceeds the launch grid");
    XlRowsParams p;
    p.rows = rows, p.count = count, p.ptr = ptr, p.other = other, p.type = type;
    p.cap_rows = (int32_t)e->capacity_rows, p.cap_edges = (int32_t)e->capacity_edges;
    p.rel = xl_mat(relation), p.x = xl_mat(x);
    p.out = reinterpret_cast<float *>(out->ptr);
    p.out_so = out->stride_outer, p.out_sr = out->stride_row;
    p.n_outer = (int32_t)n_outer, p.row_len = (int32_t)row_len;
    p.num_node = (int32_t)out->n_row, p.num_rel = (int32_t)relation->n_row;
    (void)hipGetLastError();   // drop any stale error left by other users of the HIP runtime
    hipLaunchKernelGGL(delta_edges_rows_kernel, dim3((unsigned)grid), dim3(XL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), p);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        set_error(std::string("delta_edges_rows_kernel launch: ") + hipGetErrorString(err));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

}  // namespace ultra

using namespace ultra;

extern "C" int32_t ultra_rspmm_delta_edges_forward(const ultra_explain_edits *edits, const ultra_mat *relation,
                                                   const ultra_mat *input, const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return xl_rows("ultra_rspmm_delta_edges_forward", edits, false, relation, input, output, stream);
}

extern "C" int32_t ultra_rspmm_delta_edges_backward_input(const ultra_explain_edits *edits, const ultra_mat *relation,
                                                          const ultra_mat *output_grad, const ultra_mat *input_grad, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, input_grad ? input_grad->ptr : nullptr);
    return xl_rows("ultra_rspmm_delta_edges_backward_input", edits, true, relation, output_grad, input_grad, stream);
}

extern "C" int32_t ultra_rspmm_delta_edge_grad_samples(const ultra_explain_edits *edits, const ultra_mat *relation,
                                                       const ultra_mat *input, const ultra_mat *output_grad, void *weight_grad_dev,
                                                       int64_t weight_grad_stride, void *stream) {
    const char *who = "ultra_rspmm_delta_edge_grad_samples";
    int rc;
    if ((rc = xl_check_edits(who, edits))) return rc;
    if (!output_grad || !output_grad->ptr) return xl_invalid(who, "output_grad is NULL");
    const int64_t n_outer = output_grad->n_outer, row_len = output_grad->row_len;
    if (n_outer < 0 || n_outer > 65535 || row_len <= 0 || row_len >= (1ll << 31))
        return xl_invalid(who, "output_grad: n_outer must be in [0, 65535] and row_len positive");
    if (n_outer == 0 || edits->capacity_edges == 0) return ULTRA_OK;
    if (!weight_grad_dev) return xl_invalid(who, "weight_grad is NULL");
    if (weight_grad_stride < edits->capacity_edges) return xl_invalid(who, "weight_grad_stride < capacity_edges");
    if (!edits->count_dev || !edits->add_ptr_dev || !edits->add_src_dev || !edits->add_dst_dev || !edits->add_type_dev ||
        !edits->add_j_dev)
        return xl_invalid(who, "edits: a NULL array");
    if ((rc = xl_check_mat(who, output_grad, "output_grad", n_outer, row_len))) return rc;
    if ((rc = xl_check_mat(who, relation, "relation", n_outer, row_len))) return rc;
    if ((rc = xl_check_mat(who, input, "input", n_outer, row_len))) return rc;
    if (input->n_row != output_grad->n_row) return xl_invalid(who, "input and output_grad must have the graph's num_node rows each");
    ULTRA_DEVICE_SCOPE(stream, weight_grad_dev);
    XlGradParams p;
    p.count = edits->count_dev, p.add_ptr = edits->add_ptr_dev, p.src = edits->add_src_dev, p.dst = edits->add_dst_dev;
    p.type = edits->add_type_dev, p.j = edits->add_j_dev;
    p.cap_rows = (int32_t)edits->capacity_rows, p.cap_edges = (int32_t)edits->capacity_edges;
    p.rel = xl_mat(relation), p.x = xl_mat(input), p.og = xl_mat(output_grad);
    p.wgrad = reinterpret_cast<float *>(weight_grad_dev);
    p.wgrad_so = weight_grad_stride;
    p.row_len = (int32_t)row_len, p.num_node = (int32_t)input->n_row, p.num_rel = (int32_t)relation->n_row;
    const int64_t grid = (edits->capacity_edges + XL_THREADS / 64 - 1) / (XL_THREADS / 64);
    (void)hipGetLastError();
    hipLaunchKernelGGL(delta_edge_grad_samples_kernel, dim3((unsigned)grid, (unsigned)n_outer), dim3(XL_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), p);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        set_error(std::string("delta_edge_grad_samples_kernel launch: ") + hipGetErrorString(err));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}
