// What the layer-0 kernels share: the flag bits, the operand block, and the LayerNorm / ReLU of one row held by a 16-lane
// group.  Included by layer0_kernels.hpp (the walk over the transposed plan, ultra_nbf_layer0) and by
// dense_layer0_adjacency.hip (the same layer read off the relation graph's byte adjacency).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rspmm_kernels.hpp"
#include "torch_math.hpp"

namespace ultra {

// L0_MAX: the max aggregate (layers.py:206-207).  The messages of the zero rows are exact zeros and the boundary tensor is
// zero off the source row, so a reached row aggregates max(0, messages from s[b]) and every other row 0 -- the same constant
// output row as under the sum; the source row meets its boundary value q, the messages of its self loops, and a zero only
// if some OTHER node has an edge onto it.
// L0_ONLY_FILL / L0_SKIP_FILL: the constant fill depends on the layer's parameters only -- a caller may launch it ahead of
// time (beside the relation model, whose output the special rows need) and the special rows later.
enum { L0_LN = 1, L0_RELU = 2, L0_RESIDUAL = 4, L0_MAX = 8, L0_ONLY_FILL = 16, L0_SKIP_FILL = 32 };

struct Layer0Params {
    const int32_t *trow_ptr;   // transposed plan: row = gathered source
    const int32_t *tcol;       // = aggregation target
    const int32_t *ttype;
    const int32_t *tperm;
    const uint8_t *self_loop;  // [num_node] bit 0: the node has an edge onto itself, bit 1: an in-edge from another node
    const float *w;            // edge weights in original edge order, or NULL
    const int64_t *src;        // [n_outer] source row s[b]
    const float *q;            // [n_outer][64] boundary value of the source row, or NULL = ones (RelNBFNet)
    MatArg rel;                // (n_outer, num_rel, 64)
    const float *weight;       // (64, 128) row-major = linear.weight
    const float *bias, *ln_w, *ln_b;   // (64); bias may be NULL
    float *out;
    long long out_so, out_sr;
    long long num_node;
    int32_t n_outer;
    float eps;
    int32_t flags;
};

// LayerNorm / ReLU of one 64-feature row held by a 16-lane group (4 features per lane), layers.py:235-238
struct L0Vec {
    float bias[4], ln_w[4], ln_b[4];
};

__device__ __forceinline__ L0Vec l0_load_vectors(const Layer0Params &p, int l16) {
    L0Vec v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v.bias[e] = p.bias ? p.bias[4 * l16 + e] : 0.f;
        v.ln_w[e] = (p.flags & L0_LN) ? p.ln_w[4 * l16 + e] : 1.f;
        v.ln_b[e] = (p.flags & L0_LN) ? p.ln_b[4 * l16 + e] : 0.f;
    }
    return v;
}

// LayerNorm (the reference's operation order, torch_math.hpp) and ReLU of a row held by a 16-lane group, feature
// 4 l16 + e in register e.  `slot` = 64 + 16 floats of LDS private to the group: the row is parked there, lanes 0..7 run
// the Welford accumulator i = l16 over features 8 j + i, every lane merges the eight (LDS operations of one wave
// execute in order: no barrier between the group's writes and reads).
__device__ __forceinline__ void l0_finish(float (&y)[4], const Layer0Params &p, const L0Vec &vec, float *slot, const int l16) {
    if (p.flags & L0_LN) {
        *reinterpret_cast<float4 *>(slot + 4 * l16) = make_float4(y[0], y[1], y[2], y[3]);
        float xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = slot[8 * j + (l16 & 7)];
        const Moments w = welford8(xv);
        if (l16 < 8) {
            slot[64 + 2 * l16] = w.m1;
            slot[64 + 2 * l16 + 1] = w.m2;
        }
        Moments all[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) all[i] = Moments{slot[64 + 2 * i], slot[64 + 2 * i + 1]};
        float mean, rstd;
        merge8(all, p.eps, mean, rstd);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = ln_apply(y[e], mean, rstd, vec.ln_w[e], vec.ln_b[e]);
    }
    if (p.flags & L0_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fmaxf(y[e], 0.f);
    }
}

}  // namespace ultra
