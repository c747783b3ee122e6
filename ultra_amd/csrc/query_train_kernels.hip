// Training UltraQuery: traversal dropout as a keep vector and the query loss.
//
// ultra_traversal_dropout -- UltraQuery.traversal_dropout (reference: ultra/ultraquery.py:34-83) without a filtered copy of
//   the graph.  For a projection over B samples with relations r_b and symbolic sets s_b (B, N):
//     k(e)  = #{b : r_b == type(e), s_b[src(e)] != 0} + #{b : inv(r_b) == type(e), s_b[dst(e)] != 0}
//             (the edge's multiplicity in the reference's concatenated edge_match lists; != 0 counts NaN, not -0.0)
//     keep(e) = 0  iff  not must_keep(e) and ((k(e) > 0 and u1[e] <= q[k(e)]) or (more > 0 and u2[e] <= more))
//     must_keep(e) = deg_out(src) <= 1 or deg_in(dst) <= 1 (full graph);  q[k] = 1 - (1 - ratio)^k (host, fp64 -> fp32)
//   Two launches: dropout_mask_kernel turns the relations into bit sets of samples per relation -- direct[r] holds the b with
//   r_b == r, inverse[r] those with inv(r_b) == r -- and dropout_edge_kernel visits each edge once: an edge whose type no
//   sample asked for costs two mask-word loads, a matching one reads s_b at its source (direct) or tail (inverse) only.
//   No atomics, no host synchronisation: the same bits on every run.
//
// ultra_query_loss -- run_query.py:94-114 and its gradient:
//     l = binary_cross_entropy_with_logits(pred, target);  w = 1 / num_pos on positives,
//     softmax(pred_neg / T) over the negatives (T > 0, a constant) or 1 / num_neg (T == 0)
//     loss = mean_b( sum_i l w / sum_i w );   grad = w (sigmoid(pred) - target) / (sum_i w * rows)
//   (exp(x / T - max) with the argument's rounding errors carried along: exp_arg.hpp)
//   One workgroup per row; every sum runs in a fixed order (per-thread strides, then an LDS tree).  The last workgroup to
//   finish (a counter in the workspace, reset by that workgroup) averages the row losses in row order: reproducible.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ultra_nbfnet.h"
#include "plan.hpp"
#include "device_scope.hpp"
#include "exp_arg.hpp"

namespace ultra {

constexpr int DROPOUT_THREADS = 256;
constexpr int QLOSS_THREADS = 256;

__device__ __forceinline__ long long inverse_relation(long long r, long long num_relation, int rel_plus_one) {
    if (rel_plus_one) return r ^ 1;
    const long long half = num_relation / 2;
    return r >= half ? r - half : r + half;
}

// one thread per (relation, word): bits of the samples b in [32 word, 32 word + 32) whose relation (inverse) is `relation`
__global__ void __launch_bounds__(DROPOUT_THREADS) dropout_mask_kernel(const int64_t *__restrict__ r_index, long long batch,
                                                                       long long num_relation, int rel_plus_one, int words,
                                                                       uint32_t *__restrict__ direct, uint32_t *__restrict__ inverse) {
    const long long idx = blockIdx.x * (long long)DROPOUT_THREADS + threadIdx.x;
    if (idx >= num_relation * words) return;
    const long long rel = idx / words;
    const int w = (int)(idx - rel * words);
    uint32_t d = 0, v = 0;
    for (int j = 0; j < 32; ++j) {
        const long long b = 32LL * w + j;
        if (b >= batch) break;
        const long long r = r_index[b];
        if (r == rel) d |= 1u << j;
        if (inverse_relation(r, num_relation, rel_plus_one) == rel) v |= 1u << j;
    }
    direct[idx] = d;
    inverse[idx] = v;
}

template <typename T>
__global__ void __launch_bounds__(DROPOUT_THREADS) dropout_edge_kernel(
    const int64_t *__restrict__ edge_index, const int64_t *__restrict__ edge_type, long long num_edge, long long num_node,
    long long num_relation, const int32_t *__restrict__ deg_out, const int32_t *__restrict__ deg_in, const uint32_t *__restrict__ direct,
    const uint32_t *__restrict__ inverse, int words, const T *__restrict__ sym, const float *__restrict__ q,
    const float *__restrict__ u1, const float *__restrict__ u2, float more, float *__restrict__ keep, int32_t *__restrict__ k_out) {
    const long long e = blockIdx.x * (long long)DROPOUT_THREADS + threadIdx.x;
    if (e >= num_edge) return;
    const long long src = edge_index[e], dst = edge_index[num_edge + e], rel = edge_type[e];
    int k = 0;
    if (rel >= 0 && rel < num_relation) {
        const uint32_t *dm = direct + rel * words, *im = inverse + rel * words;
        for (int w = 0; w < words; ++w) {
            uint32_t d = dm[w], v = im[w];
            while (d) {
                const long long b = 32LL * w + __builtin_ctz(d);
                d &= d - 1;
                k += sym[b * num_node + src] != T(0);       // NaN != 0 is true; -0.0 != 0 is false (nonzero())
            }
            while (v) {
                const long long b = 32LL * w + __builtin_ctz(v);
                v &= v - 1;
                k += sym[b * num_node + dst] != T(0);
            }
        }
    }
    const bool must_keep = deg_out[src] <= 1 || deg_in[dst] <= 1;
    bool drop = false;
    if (!must_keep) {
        drop = (k > 0 && u1[e] <= q[k]) || (more > 0.f && u2[e] <= more);
    }
    keep[e] = drop ? 0.f : 1.f;
    if (k_out) k_out[e] = k;
}

__device__ __forceinline__ float block_sum(float v, float *red) {
    // fixed-order tree over the workgroup: the same bits on every run
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = QLOSS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

__device__ __forceinline__ float block_max(float v, float *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = QLOSS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

__global__ void __launch_bounds__(QLOSS_THREADS) query_loss_kernel(const float *__restrict__ pred, const uint8_t *__restrict__ target,
                                                                   int rows, long long n, float temperature, float *__restrict__ row_loss,
                                                                   uint32_t *__restrict__ counter, float *__restrict__ loss,
                                                                   float *__restrict__ grad) {
    __shared__ float red[QLOSS_THREADS];
    __shared__ bool last;
    const int b = blockIdx.x;
    const float *p = pred + (long long)b * n;
    const uint8_t *y = target + (long long)b * n;
    float *g = grad + (long long)b * n;
    const int tid = threadIdx.x;

    const float inv_t = temperature > 0.f ? 1.f / temperature : 0.f;      // (pred / T as a product: exp_arg.hpp)
    float npos = 0.f, mx = -__builtin_inff();
    for (long long i = tid; i < n; i += QLOSS_THREADS) {
        if (y[i]) npos += 1.f;
        else if (temperature > 0.f) mx = fmaxf(mx, p[i] * inv_t);
    }
    npos = block_sum(npos, red);
    const float nneg = (float)n - npos;
    float z = 1.f;
    if (temperature > 0.f) {
        mx = block_max(mx, red);
        float s = 0.f;
        for (long long i = tid; i < n; i += QLOSS_THREADS)
            if (!y[i]) s += exp_scaled_minus(p[i], inv_t, mx);
        z = block_sum(s, red);
    }
    const float wpos = 1.f / npos, wneg = 1.f / nneg;
    float lw = 0.f, ws = 0.f;
    for (long long i = tid; i < n; i += QLOSS_THREADS) {
        const float x = p[i], t = y[i] ? 1.f : 0.f;
        const float w = y[i] ? wpos : (temperature > 0.f ? exp_scaled_minus(x, inv_t, mx) / z : wneg);
        // (1 - t) x - log_sigmoid(x),  log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))
        const float l = (1.f - t) * x - (fminf(x, 0.f) - log1pf(expf(-fabsf(x))));
        lw += l * w;
        ws += w;
    }
    lw = block_sum(lw, red);
    ws = block_sum(ws, red);
    const float scale = 1.f / (ws * (float)rows);
    for (long long i = tid; i < n; i += QLOSS_THREADS) {
        const float x = p[i], t = y[i] ? 1.f : 0.f;
        const float w = y[i] ? wpos : (temperature > 0.f ? exp_scaled_minus(x, inv_t, mx) / z : wneg);
        const float sig = 1.f / (1.f + expf(-x));
        g[i] = w * (sig - t) * scale;
    }
    if (tid == 0) {
        row_loss[b] = lw / ws;
        __threadfence();
        last = atomicAdd(counter, 1u) == (uint32_t)(rows - 1);
    }
    __syncthreads();
    if (last && tid == 0) {
        __threadfence();
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += __builtin_nontemporal_load(row_loss + r);
        *loss = s / (float)rows;
        *counter = 0u;
    }
}

}  // namespace ultra

using namespace ultra;

extern "C" {

int64_t ultra_traversal_dropout_mask_words(int64_t batch) { return batch > 0 ? (batch + 31) / 32 : 0; }

int32_t ultra_traversal_dropout(const int64_t *edge_index, const int64_t *edge_type, int64_t num_edge, int64_t num_node,
                                int64_t num_relation, int32_t inverse_rel_plus_one, const int32_t *deg_out, const int32_t *deg_in,
                                const int64_t *r_index, int64_t batch, int32_t dtype, const void *sym, const float *q,
                                const float *u1, const float *u2, float more_dropout, void *masks, float *keep, int32_t *k_out,
                                void *stream) {
    ULTRA_DEVICE_SCOPE(stream, edge_index);
    if (num_edge < 0 || num_node <= 0 || num_relation <= 0 || batch <= 0 || (dtype != 0 && dtype != 1) || !deg_out || !deg_in ||
        !r_index || !sym || !q || !u1 || !masks || !keep || (num_edge > 0 && (!edge_index || !edge_type)) ||
        (more_dropout > 0.f && !u2)) {
        set_error("ultra_traversal_dropout: bad argument");
        return ULTRA_ERR_INVALID;
    }
    if (batch >= (1LL << 31) || num_relation >= (1LL << 31)) {
        set_error("ultra_traversal_dropout: batch and num_relation must be below 2^31");
        return ULTRA_ERR_UNSUPPORTED;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int words = (int)ultra_traversal_dropout_mask_words(batch);
    uint32_t *direct = (uint32_t *)masks, *inverse = direct + num_relation * words;
    (void)hipGetLastError();
    const long long mask_threads = num_relation * words;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((mask_threads + DROPOUT_THREADS - 1) / DROPOUT_THREADS)),
                       dim3(DROPOUT_THREADS), 0, s, r_index, (long long)batch, (long long)num_relation, (int)inverse_rel_plus_one,
                       words, direct, inverse);
    if (num_edge > 0) {
        const dim3 grid((unsigned)((num_edge + DROPOUT_THREADS - 1) / DROPOUT_THREADS));
        if (dtype == 0)
            hipLaunchKernelGGL(dropout_edge_kernel<float>, grid, dim3(DROPOUT_THREADS), 0, s, edge_index, edge_type,
                               (long long)num_edge, (long long)num_node, (long long)num_relation, deg_out, deg_in, direct, inverse,
                               words, (const float *)sym, q, u1, u2, more_dropout, keep, k_out);
        else
            hipLaunchKernelGGL(dropout_edge_kernel<double>, grid, dim3(DROPOUT_THREADS), 0, s, edge_index, edge_type,
                               (long long)num_edge, (long long)num_node, (long long)num_relation, deg_out, deg_in, direct, inverse,
                               words, (const double *)sym, q, u1, u2, more_dropout, keep, k_out);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("traversal dropout kernels: launch failed: ") + hipGetErrorString(e));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

int32_t ultra_query_loss(const void *pred, const uint8_t *target, int64_t rows, int64_t n, float temperature, void *work,
                         void *loss, void *grad, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, pred);
    if (!pred || !target || !work || !loss || !grad || rows < 1 || rows >= (1LL << 31) || n < 1) {
        set_error("ultra_query_loss: NULL operand, rows outside [1, 2^31) or no columns");
        return ULTRA_ERR_INVALID;
    }
    (void)hipGetLastError();
    // work: the row losses (rows floats), then the completion counter (zero on entry; left at zero)
    float *row_loss = (float *)work;
    uint32_t *counter = (uint32_t *)(row_loss + rows);
    hipLaunchKernelGGL(query_loss_kernel, dim3((unsigned)rows), dim3(QLOSS_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       (const float *)pred, target, (int)rows, (long long)n, temperature, row_loss, counter, (float *)loss,
                       (float *)grad);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string("query_loss_kernel launch: ") + hipGetErrorString(e));
        return ULTRA_ERR_HIP;
    }
    return ULTRA_OK;
}

}  // extern "C"
