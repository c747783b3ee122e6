// Layer 0 of RelNBFNet on its one-hot boundary condition, read off the relation graph's BYTE ADJACENCY instead of a plan
// (ultra_nbf_dense_layer0_adjacency).
//
// layer0_kernels.hpp computes the same layer from the transposed sparse plan: it walks the out-edges of the query relation q.
// A relation graph that is kept current in place has no plan to walk -- but it has the bytes A[row][type][col] the
// reference-order layer kernel reads (dense_order_layer.hip `a_ex`), and "the out-edges of q" are the non-zero bytes of COLUMN
// q: at most four per row, one per type.  The parallel edges of one (row, col) come in type order in a reference-order plan, so
//     agg[b, i] = ((0 + rel[b, t0] * x0) + rel[b, t1] * x0) + ...   over the types t0 < t1 < ... with A[i][t][q] != 0,
// every product rounded on its own and added in that order, is the sum ultra_nbf_layer0 forms for row i.  The rest is that
// kernel's arithmetic restated step for step -- the boundary value at row q (added to the messages where q reaches itself, taken
// alone where it does not: 0 + x0 would turn a -0 into +0), one fmaf chain per output over k ascending with the terms of an
// all-zero input half skipped, bias added last, LayerNorm / ReLU by l0_finish, the residual on the source row only -- and a row
// that is neither q nor reached is relu(LayerNorm(bias)) computed FROM THE BIAS, not from a chain of zeros (a -0 bias entry
// would come out of the chain as +0): nbf_layer0_fill_kernel's constant.  Hence the same bits on every row.
//
// One workgroup per (sample, 32-row tile), one 16-lane group per row: a lane reads the four bytes of its row in column q and
// nothing else of the adjacency.  No atomics, no allocation, no host wait.  A tile none of whose rows is reached (most tiles of
// a sparse column) skips the weight staging.  At a few hundred rows the launch is a few dozen small workgroups that each run one
// dependent chain (bytes -> relation rows -> 64 or 128 fmaf steps -> LayerNorm): latency-bound, and not tuned beyond that.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "device_scope.hpp"
#include "layer0_update.hpp"
#include "plan.hpp"

namespace ultra {

constexpr int DL0_ROWS = 32;      // rows (16-lane groups) per workgroup

struct DenseLayer0Params {
    Layer0Params l0;              // src, q, rel, weight, bias, ln_w, ln_b, out, out_so, out_sr, num_node, n_outer, eps, flags
    const uint8_t *a_ex;          // [n_rt16][n_jc][64 lanes = row % 16 + 16 type][16 bytes = col % 16]
    int32_t n_jc;
};

__global__ void __launch_bounds__(16 * DL0_ROWS) dense_layer0_adjacency_kernel(const DenseLayer0Params dp) {
    __shared__ __attribute__((aligned(16))) float lds_wt[128 * 64];
    __shared__ __attribute__((aligned(16))) float lds_vec[DL0_ROWS * 80];   // one 64-vector (+ 16 LayerNorm moments) per group
    const Layer0Params &p = dp.l0;
    const int outer = blockIdx.y;
    const int l16 = threadIdx.x & 15;
    const long long row = (long long)blockIdx.x * DL0_ROWS + (threadIdx.x >> 4);
    const bool live = row < p.num_node;
    long long s = p.src[outer];
    s = s < 0 ? 0 : (s >= p.num_node ? p.num_node - 1 : s);   // (an out-of-range id reads a valid column instead of faulting)
    // the four cells of this row in column s, one per type (rows past the graph read nothing)
    bool cell[4] = {false, false, false, false};
    if (live) {
        const uint8_t *at = dp.a_ex + (((row >> 4) * dp.n_jc + (s >> 4)) * 64 + (row & 15)) * 16 + (s & 15);
#pragma unroll
        for (int t = 0; t < 4; ++t) cell[t] = at[16 * 16 * t] != 0;
    }
    const bool reached = cell[0] || cell[1] || cell[2] || cell[3];
    const bool is_src = live && row == s;
    const L0Vec vec = l0_load_vectors(p, l16);
    float *slot = lds_vec + (threadIdx.x >> 4) * 80;
    float *outp = p.out + outer * p.out_so + row * p.out_sr + 4 * l16;
    const bool any = __syncthreads_or(reached || is_src) != 0;
    if (!any) {     // the whole tile holds the constant row
        if (live) {
            float c0[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) c0[e] = vec.bias[e];   // W . 0 + bias
            l0_finish(c0, p, vec, slot, l16);
            *reinterpret_cast<float4 *>(outp) = make_float4(c0[0], c0[1], c0[2], c0[3]);
        }
        return;
    }
    float qv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) qv[e] = p.q ? p.q[(long long)outer * 64 + 4 * l16 + e] : 1.f;
    {   // transpose W[f][k] -> [k][f], as nbf_layer0_rows_kernel stages it
        const int f = threadIdx.x & 63;
#pragma unroll
        for (int kc = 4 * (threadIdx.x >> 6); kc < 128; kc += 4 * ((16 * DL0_ROWS) >> 6)) {
            const float4 wv = *reinterpret_cast<const float4 *>(p.weight + f * 128 + kc);
            lds_wt[(kc + 0) * 64 + f] = wv.x;
            lds_wt[(kc + 1) * 64 + f] = wv.y;
            lds_wt[(kc + 2) * 64 + f] = wv.z;
            lds_wt[(kc + 3) * 64 + f] = wv.w;
        }
    }
    __syncthreads();
    if (!live) return;
    float y[4];
    if (!reached && !is_src) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = vec.bias[e];
        l0_finish(y, p, vec, slot, l16);
        *reinterpret_cast<float4 *>(outp) = make_float4(y[0], y[1], y[2], y[3]);
        return;
    }
    const float *relb = reinterpret_cast<const float *>(p.rel.ptr) + outer * p.rel.stride_outer;
    float agg[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {       // type order = the edge order of the run
        if (cell[t]) {
            const float4 rv = *reinterpret_cast<const float4 *>(relb + (long long)t * p.rel.stride_row + 4 * l16);
            const float r4[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float m = r4[e] * qv[e];
                agg[e] = agg[e] + m;
            }
        }
    }
    if (is_src) {       // + boundary (layers.py:200); alone where no edge leads back to the source row
#pragma unroll
        for (int e = 0; e < 4; ++e) agg[e] = reached ? agg[e] + qv[e] : qv[e];
    }
    // y = (W[:, :64] . x + W[:, 64:] . agg) + bias; x = q on the source row, 0 elsewhere (those terms are exact zeros and skipped)
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = 0.f;
    if (is_src) {
        *reinterpret_cast<float4 *>(slot + 4 * l16) = make_float4(qv[0], qv[1], qv[2], qv[3]);
#pragma unroll
        for (int k4 = 0; k4 < 16; ++k4) {
            const float4 x4 = *reinterpret_cast<const float4 *>(slot + 4 * k4);
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float4 wv = *reinterpret_cast<const float4 *>(lds_wt + (4 * k4 + e) * 64 + 4 * l16);
                y[0] = __builtin_fmaf(xs[e], wv.x, y[0]);
                y[1] = __builtin_fmaf(xs[e], wv.y, y[1]);
                y[2] = __builtin_fmaf(xs[e], wv.z, y[2]);
                y[3] = __builtin_fmaf(xs[e], wv.w, y[3]);
            }
        }
    }
    *reinterpret_cast<float4 *>(slot + 4 * l16) = make_float4(agg[0], agg[1], agg[2], agg[3]);
#pragma unroll
    for (int k4 = 0; k4 < 16; ++k4) {
        const float4 a4 = *reinterpret_cast<const float4 *>(slot + 4 * k4);   // same address in the group: broadcast
        const float as[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float4 wv = *reinterpret_cast<const float4 *>(lds_wt + (64 + 4 * k4 + e) * 64 + 4 * l16);
            y[0] = __builtin_fmaf(as[e], wv.x, y[0]);
            y[1] = __builtin_fmaf(as[e], wv.y, y[1]);
            y[2] = __builtin_fmaf(as[e], wv.z, y[2]);
            y[3] = __builtin_fmaf(as[e], wv.w, y[3]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] += vec.bias[e];
    l0_finish(y, p, vec, slot, l16);
    if (is_src && (p.flags & L0_RESIDUAL)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] += qv[e];
    }
    *reinterpret_cast<float4 *>(outp) = make_float4(y[0], y[1], y[2], y[3]);
}

// Called by ultra_nbf_dense_layer0_adjacency (rspmm_api.hip) with the operands checked.
int launch_dense_layer0_adjacency(const void *a_ex_dev, int64_t n, const ultra_mat *rel, const int64_t *src_rows, const void *src_vals,
                                  const void *weight, const void *bias, const void *ln_w, const void *ln_b, float eps, int flags,
                                  const ultra_mat *out, hipStream_t stream) {
    DenseLayer0Params dp;
    std::memset(&dp, 0, sizeof(dp));
    dp.a_ex = static_cast<const uint8_t *>(a_ex_dev);
    dp.n_jc = (int32_t)((n + 15) / 16);
    dp.l0.src = src_rows;
    dp.l0.q = static_cast<const float *>(src_vals);
    dp.l0.rel = MatArg{rel->ptr, rel->stride_outer, rel->stride_row};
    dp.l0.weight = static_cast<const float *>(weight);
    dp.l0.bias = static_cast<const float *>(bias);
    dp.l0.ln_w = static_cast<const float *>(ln_w);
    dp.l0.ln_b = static_cast<const float *>(ln_b);
    dp.l0.out = static_cast<float *>(out->ptr);
    dp.l0.out_so = out->stride_outer;
    dp.l0.out_sr = out->stride_row;
    dp.l0.num_node = n;
    dp.l0.n_outer = (int32_t)out->n_outer;
    dp.l0.eps = eps;
    dp.l0.flags = flags;
    const dim3 grid((unsigned)((n + DL0_ROWS - 1) / DL0_ROWS), (unsigned)out->n_outer);
    hipLaunchKernelGGL(dense_layer0_adjacency_kernel, grid, dim3(16 * DL0_ROWS), 0, stream, dp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("dense_layer0_adjacency_kernel launch: ") + hipGetErrorString(e));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

}  // namespace ultra
