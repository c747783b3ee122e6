// C-ABI entry points of libultra_amd.so (include/ultra_rspmm.h): plan upload, forward, backward,
// the reference-shaped stateless exports and the measurement hooks.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "device_scope.hpp"
#include "layer0_kernels.hpp"
#include "rspmm_bwd_kernels.hpp"
#include "rspmm_kernels.hpp"
#include "rspmm_order_kernels.hpp"
#include "rspmm_rows_kernels.hpp"
#include "rows_bwd_kernels.hpp"

namespace ultra {

// explicit instantiations live in rspmm_variant_*.hip
#define ULTRA_EXTERN_VARIANT(T_, VEC_, MODE_) \
    template <>                               \
    hipError_t launch_fwd_variant<T_, VEC_, MODE_>(int, int, const FwdParams &, int, int, size_t, hipStream_t);
ULTRA_EXTERN_VARIANT(float, 4, 0)
ULTRA_EXTERN_VARIANT(float, 1, 0)
ULTRA_EXTERN_VARIANT(float, 4, 1)
ULTRA_EXTERN_VARIANT(float, 4, 2)
ULTRA_EXTERN_VARIANT(double, 4, 0)
ULTRA_EXTERN_VARIANT(double, 1, 0)
ULTRA_EXTERN_VARIANT(double, 4, 1)
ULTRA_EXTERN_VARIANT(double, 4, 2)

// explicit instantiations live in rspmm_order_*.hip
#define ULTRA_EXTERN_ORDER_VARIANT(T_, L_, W_) \
    template <>                                \
    hipError_t launch_order_variant<T_, L_, W_>(int, int, const OrderParams &, int, size_t, hipStream_t);
ULTRA_EXTERN_ORDER_VARIANT(float, true, true)
ULTRA_EXTERN_ORDER_VARIANT(float, true, false)
ULTRA_EXTERN_ORDER_VARIANT(float, false, true)
ULTRA_EXTERN_ORDER_VARIANT(float, false, false)
ULTRA_EXTERN_ORDER_VARIANT(double, true, true)
ULTRA_EXTERN_ORDER_VARIANT(double, true, false)
ULTRA_EXTERN_ORDER_VARIANT(double, false, true)
ULTRA_EXTERN_ORDER_VARIANT(double, false, false)

int launch_dense_relation_grad(ultra_plan *p, const ultra_mat *x, const ultra_mat *og, const ultra_mat *rgrad, float *scratch,
                               hipStream_t stream);   // rspmm_dense.hip
int launch_dense_forward(ultra_plan *p, int sum, int mul, int dtype, const void *w, const ultra_mat *rel, const ultra_mat *x,
                         const ultra_mat *bnd, const int64_t *bnd_rows, const ultra_mat *out,
                         hipStream_t stream);   // rspmm_dense.hip

int launch_dense_order_layer(ultra_plan *p, const ultra_mat *rel, const ultra_mat *x, const ultra_mat *bnd, const int64_t *bnd_rows,
                             const void *weight, const void *bias, const void *ln_w, const void *ln_b, float eps, int flags,
                             const ultra_mat *out, hipStream_t stream, bool shared_chip);   // dense_order_layer.hip
int launch_dense_order_layer_adjacency(const void *a_ex_dev, int64_t n, const ultra_mat *rel, const ultra_mat *x, const ultra_mat *bnd,
                                       const int64_t *bnd_rows, const void *weight, const void *bias, const void *ln_w,
                                       const void *ln_b, float eps, int flags, const ultra_mat *out, hipStream_t stream,
                                       bool shared_chip);   // dense_order_layer.hip
int launch_dense_layer0_adjacency(const void *a_ex_dev, int64_t n, const ultra_mat *rel, const int64_t *src_rows, const void *src_vals,
                                  const void *weight, const void *bias, const void *ln_w, const void *ln_b, float eps, int flags,
                                  const ultra_mat *out, hipStream_t stream);   // dense_layer0_adjacency.hip

int launch_dense_layer(ultra_plan *p, const ultra_mat *rel, const ultra_mat *x, const ultra_mat *bnd, const int64_t *bnd_rows,
                       const void *weight, const void *bias, const void *ln_w, const void *ln_b, float eps, int flags,
                       const ultra_mat *out, hipStream_t stream);   // dense_layer.hip

static ultra_tuning g_tuning = {0, 0, -1, -1, 0, {0, 0, 0}};
// ultra_tuning.reserved[], by the names ultra_amd/rspmm.py gives them
static int general_walk() { return g_tuning.reserved[0]; }   // reference-order plans on the general walk kernel
static int unit_walk() { return g_tuning.reserved[1]; }      // the order kernels walk units of four rows, not group streams
static int update_form() { return g_tuning.reserved[2]; }    // where forward_update applies the layer update (choose_update_form)

// measurement hook: per-workgroup clock trace of the order kernel.  State, not an argument: set by an ABI call of its own
// (ultra_order_trace) and read by every order launch of the thread until it is cleared.
static thread_local long long *g_order_trace = nullptr;
// ultra_rspmm_weight_epoch: the caller's tag of the edge-weight vector it is about to pass (0 = none).  A plan that has
// ALREADY brought the vector with this tag, at this address, into its own edge order keeps that copy: the fine-tuning step hands
// one 0/1 keep vector to 5 forward and 10 backward walks, each of which would otherwise re-run the same permutation (24 us at
// YAGO3-10's size).  Consumed by the next weighted API call of the thread (the entry points reset it on their way out).
static thread_local int64_t g_w_epoch = 0;
struct WeightEpochScope {
    ~WeightEpochScope() { g_w_epoch = 0; }
};

// ---- the device-side error word (OrderParams::err) ----
// One word of pinned, mapped host memory per process: a kernel whose bounded spin gave up stores (code << 24 | workgroup) there
// with a system-scope store; the host reads it without any HIP call -- at the next forward entry and in ultra_device_error().
// (one word PER DEVICE: a give-up on device k is reported by the next forward on device k -- or by ultra_device_error() called with
// device k current -- not by whatever launch of another device's thread happens to come first)
static constexpr int MAX_ERR_DEVICES = 64;
static uint32_t *g_dev_err[MAX_ERR_DEVICES] = {nullptr};
static int current_device_slot() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return dev >= 0 && dev < MAX_ERR_DEVICES ? dev : 0;
}
static uint32_t *device_error_word() {
    const int slot = current_device_slot();
    if (!g_dev_err[slot]) {
        void *ptr = nullptr;
        if (hipHostMalloc(&ptr, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;      // (no word: the kernels then only keep their spins bounded)
        }
        std::memset(ptr, 0, 64);
        g_dev_err[slot] = static_cast<uint32_t *>(ptr);
    }
    return g_dev_err[slot];
}
static int take_device_error() {
    uint32_t *cell = g_dev_err[current_device_slot()];
    if (!cell) return ULTRA_OK;
    const uint32_t word = __atomic_exchange_n(cell, 0u, __ATOMIC_RELAXED);
    if (!word) return ULTRA_OK;
    static const char *const what[] = {"?", "an update wave waiting for rows from the walkers", "an update wave waiting for the other update waves",
                                       "a walker waiting for the chain consumer", "an update wave waiting for the chain consumer",
                                       "a walker waiting for a free row of the hand-off ring", "an update wave waiting for its tile"};
    const uint32_t code = word >> 24;
    set_error(std::string("rspmm_order_kernel: a bounded wait of the hand-off between walkers and update waves gave up (") +
              (code < 7 ? what[code] : "?") + ", workgroup " + std::to_string(word & 0xffffffu) +
              "): the launch was ended instead of hanging; its output is incomplete");
    return ULTRA_ERR_HIP;
}

static int hip_fail(hipError_t e, const char *what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return ULTRA_ERR_HIP;
}
#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(_e, #expr);  \
    } while (0)

static int invalid(const std::string &msg) {
    set_error(msg);
    return ULTRA_ERR_INVALID;
}

template <typename V>
static int upload_array(V **dst, const std::vector<V> &src) {
    *dst = nullptr;
    const size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(V);
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), bytes));
    if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice));
    return ULTRA_OK;
}

static int upload_plan(ultra_plan *p) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (p->on_device) {
        if (p->d.device != dev)
            return invalid("the plan was uploaded to device " + std::to_string(p->d.device) + " but this call runs on device " +
                           std::to_string(dev) + " (operands / stream of another GPU): build one plan per device");
        return ULTRA_OK;
    }
    int rc;
    if (p->flags & ULTRA_PLAN_DENSE) {
        if ((rc = upload_array(&p->d.a_frag, p->a_frag))) return rc;
        if (!p->a16.empty() && (rc = upload_array(&p->d.a16, p->a16))) return rc;
        if (!p->a_ex.empty() && (rc = upload_array(&p->d.a_ex, p->a_ex))) return rc;
        p->d.device = dev;
        p->on_device = true;
        return ULTRA_OK;
    }
    if ((rc = upload_array(&p->d.row_ptr, p->row_ptr))) return rc;
    if ((rc = upload_array(&p->d.col, p->col))) return rc;
    if ((rc = upload_array(&p->d.type, p->type))) return rc;
    if (p->flags & ULTRA_PLAN_EXACT_ORDER) {
        // the order kernels prefetch records unconditionally: both streams are padded with readable zeros.  The four groups
        // of a wave walk as many rounds as the LONGEST of their rows: a short row at the end of the list requests up to that
        // many records past its own end (the assembly walks; the C++ walk stops advancing, rspmm_order_kernels.hpp), so the
        // padding covers the longest row a lane group walks (rows above chain_min are chain rows: items[0, n_chain)).
        int64_t longest = 0;
        for (size_t i = (size_t)p->n_chain; i < p->items.size(); ++i) longest = std::max<int64_t>(longest, p->items[i].len);
        const size_t pad = (size_t)ORDER_PAD + (size_t)std::min<int64_t>(longest, 1 << 20);
        std::vector<int32_t> perm_pad(p->perm), rec_pad(p->rec);
        perm_pad.resize(p->perm.size() + pad, 0);
        rec_pad.resize(p->rec.size() + 2 * pad, 0);
        if ((rc = upload_array(&p->d.perm, perm_pad))) return rc;
        if ((rc = upload_array(&p->d.rec, rec_pad))) return rc;
    } else if ((rc = upload_array(&p->d.perm, p->perm))) {
        return rc;
    }
    if ((rc = upload_array(&p->d.erow, p->erow))) return rc;
    if ((rc = upload_array(&p->d.packed, p->packed))) return rc;
    if ((rc = upload_array(&p->d.items, p->items))) return rc;
    if ((rc = upload_array(&p->d.split_row, p->split_row))) return rc;
    if ((rc = upload_array(&p->d.split_ptr, p->split_ptr))) return rc;
    if (!p->self_loop.empty() && (rc = upload_array(&p->d.self_loop, p->self_loop))) return rc;
    p->d.device = dev;
    p->on_device = true;
    return ULTRA_OK;
}

static void free_schedules(ultra_plan *p) {
    std::lock_guard<std::mutex> lock(p->sched_mu);
    for (auto &kv : p->schedules) {
        Schedule *s = kv.second;
        if (s->d_chunk_ptr) (void)hipFree(s->d_chunk_ptr);
        if (s->d_unit_ptr) (void)hipFree(s->d_unit_ptr);
        if (s->d_units) (void)hipFree(s->d_units);
        if (s->d_chunks) (void)hipFree(s->d_chunks);
        if (s->d_srec) (void)hipFree(s->d_srec);
        if (s->d_sdesc) (void)hipFree(s->d_sdesc);
        if (s->d_prow) (void)hipFree(s->d_prow);
        if (s->d_prow_ptr) (void)hipFree(s->d_prow_ptr);
        delete s;
    }
    p->schedules.clear();
}

// The static work assignment of a reference-order plan for `nparts` workgroups per span: built and uploaded on first
// use (warm-up calls do that before any hipGraph capture), then read-only.
static int get_schedule(ultra_plan *p, int32_t nparts, Schedule **out, int32_t walkers = 16) {
    std::lock_guard<std::mutex> lock(p->sched_mu);
    const int32_t key = nparts | (walkers == 12 ? ULTRA_SCHEDULE_12_WALKERS : 0);   // (nparts <= the workgroup count of a launch)
    auto it = p->schedules.find(key);
    if (it != p->schedules.end()) {
        *out = it->second;
        return ULTRA_OK;
    }
    Schedule *s = build_schedule(p, nparts, walkers);
    int rc;
    if ((rc = upload_array(&s->d_chunk_ptr, s->chunk_ptr)) || (rc = upload_array(&s->d_unit_ptr, s->unit_ptr)) ||
        (rc = upload_array(&s->d_units, s->units)) || (rc = upload_array(&s->d_chunks, s->chunks)) ||
        (rc = upload_array(&s->d_srec, s->srec)) || (rc = upload_array(&s->d_sdesc, s->sdesc)) ||
        (rc = upload_array(&s->d_prow, s->prow)) || (rc = upload_array(&s->d_prow_ptr, s->prow_ptr))) {
        delete s;
        return rc;
    }
    p->schedules[key] = s;
    *out = s;
    return ULTRA_OK;
}

static void free_device(ultra_plan *p) {
    free_schedules(p);
    if (!p->on_device) return;
    (void)hipFree(p->d.row_ptr);
    (void)hipFree(p->d.col);
    (void)hipFree(p->d.type);
    (void)hipFree(p->d.perm);
    (void)hipFree(p->d.erow);
    (void)hipFree(p->d.packed);
    (void)hipFree(p->d.items);
    if (p->d.rec) (void)hipFree(p->d.rec);
    (void)hipFree(p->d.split_row);
    (void)hipFree(p->d.split_ptr);
    if (p->d.a_frag) (void)hipFree(p->d.a_frag);
    if (p->d.a16) (void)hipFree(p->d.a16);
    if (p->d.a_ex) (void)hipFree(p->d.a_ex);
    if (p->d.self_loop) (void)hipFree(p->d.self_loop);
    for (WeightCopy &c : p->d.w_copy)
        if (c.buf) (void)hipFree(c.buf);
    if (p->d.partial) (void)hipFree(p->d.partial);
    for (void *q : {p->d.rb_rec_c, p->d.rb_seg_c, p->d.rb_multi_c, p->d.rb_rec_t, p->d.rb_seg_t, p->d.rb_multi_t, p->d.rb_work})
        if (q) (void)hipFree(q);
    p->rb_built = false;
    p->d = DevicePlan();
    p->on_device = false;
}

static int ensure_scratch(void **buf, size_t *have, size_t need, const ultra_plan *owner = nullptr) {
    if (need <= *have) return ULTRA_OK;
    if (owner && owner->pinned > 0 && *buf)
        return invalid("this plan's scratch buffer is referenced by a captured hipGraph (ultra_plan_pin) and the call needs a "
                       "larger one: use a separate plan, or release the graph first");
    if (*buf) HIP_TRY(hipFree(*buf));  // implicit device sync: no in-flight kernel still reads it
    *buf = nullptr;
    *have = 0;
    HIP_TRY(hipMalloc(buf, need));
    *have = need;
    return ULTRA_OK;
}

struct DevInfo {
    int cu = 0;
    size_t lds_optin = 0;
};
static int device_info(DevInfo *out) {
    static DevInfo cache[64];
    static bool have[64] = {false};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return invalid("device id out of range");
    if (!have[dev]) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        cache[dev].cu = prop.multiProcessorCount;
        // gfx950: 160 KiB per workgroup (MI355X_MICROARCH: a single workgroup may use all of it)
        size_t lds = prop.sharedMemPerBlock;
        if (prop.maxSharedMemoryPerMultiProcessor > lds) lds = prop.maxSharedMemoryPerMultiProcessor;
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 && lds < 160 * 1024) lds = 160 * 1024;
        cache[dev].lds_optin = lds;
        have[dev] = true;
    }
    *out = cache[dev];
    return ULTRA_OK;
}

// workgroups of a walk launch: the tuning's, else one per CU
static int launch_grid(const DevInfo &di) { return std::max(1, g_tuning.grid > 0 ? g_tuning.grid : di.cu); }

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int check_mat(const ultra_mat *m, const char *name, int64_t min_rows, int64_t n_outer, int64_t row_len) {
    if (!m || !m->ptr) return invalid(std::string(name) + " is NULL");
    if (m->n_outer != n_outer) return invalid(std::string(name) + ": n_outer mismatch");
    if (m->row_len != row_len) return invalid(std::string(name) + ": row_len mismatch (the reference's checkSize on dim 1)");
    if (m->n_row < min_rows) return invalid(std::string(name) + ": too few rows");
    if (m->stride_row < row_len && m->n_row > 1) return invalid(std::string(name) + ": stride_row < row_len");
    return ULTRA_OK;
}

static bool mat_vec_ok(const ultra_mat *m, int64_t step) {
    return aligned16(m->ptr) && (m->stride_row % step == 0) && (m->stride_outer % step == 0);
}

// What one forward call carries besides its operands.
struct FwdCall {
    // bnd_rows != NULL: `bnd` is a POINT boundary -- one row per outer slice (n_row == 1), added to output row
    // bnd_rows[outer] only (the NBFNet boundary condition is zero everywhere else, models.py:135-141); sum aggregate only.
    const int64_t *bnd_rows = nullptr;
    // upd != NULL: the layer update of every output row is applied by the same launch (ultra_rspmm_forward_update); served by
    // the stream walk only -- ULTRA_ERR_UNSUPPORTED otherwise, with nothing launched.
    const OrderParams::Update *upd = nullptr;
    int keep_mode = 0;      // ultra_rspmm_forward_masked: the weight stream is a 0/1 keep mask (weigh(), rspmm_kernels.hpp)
    // ultra_rspmm_forward_masked_samples: one keep mask per outer slice, w_stride_outer elements apart.  Served by the weighted
    // reference-order kernels only (they read w[perm[.]] from a per-span base: no sorted copy to make per slice) --
    // ULTRA_ERR_UNSUPPORTED on every other route, with nothing launched.
    bool w_samples = false;
    int64_t w_stride_outer = 0;
    hipEvent_t ev_before = nullptr, ev_after = nullptr;   // measurement hook: recorded right before / after the main kernel launch
};

// Sums the partial rows of the plan's split rows into `dst` in slot order (after the walk that wrote them to q->d.partial).
static int launch_fixup(const ultra_plan *q, const ultra_mat *dst, int sum, int dtype, int vec, hipStream_t stream,
                        const MatArg *bnd = nullptr, const long long *bnd_rows = nullptr) {
    if (q->split_row.empty()) return ULTRA_OK;
    FixupParams xp;
    std::memset(&xp, 0, sizeof(xp));
    xp.split_row = q->d.split_row, xp.split_ptr = q->d.split_ptr;
    xp.n_split = (int32_t)q->split_row.size();
    xp.partial = q->d.partial;
    if (bnd) xp.bnd = *bnd;
    xp.bnd_rows = bnd_rows;
    xp.has_bnd = bnd ? 1 : 0;
    xp.out = dst->ptr, xp.out_stride_outer = dst->stride_outer, xp.out_stride_row = dst->stride_row;
    xp.n_outer = (int32_t)dst->n_outer, xp.row_len = (int32_t)dst->row_len;
    const long long total = (long long)xp.n_split * dst->n_outer * (dst->row_len / vec);
    const int blocks = (int)std::min<long long>((total + 15) / 16, 16384);      // 16 output vectors per workgroup
#define ULTRA_FIX(T_, V_)                                                                                          \
    switch (sum) {                                                                                                \
        case 0: hipLaunchKernelGGL((rspmm_fixup_kernel<T_, V_, 0>), dim3(blocks), dim3(256), 0, stream, xp); break; \
        case 1: hipLaunchKernelGGL((rspmm_fixup_kernel<T_, V_, 1>), dim3(blocks), dim3(256), 0, stream, xp); break; \
        default: hipLaunchKernelGGL((rspmm_fixup_kernel<T_, V_, 2>), dim3(blocks), dim3(256), 0, stream, xp); break; \
    }
    if (dtype == ULTRA_F32) {
        if (vec == 4) { ULTRA_FIX(float, 4) } else { ULTRA_FIX(float, 1) }
    } else {
        if (vec == 4) { ULTRA_FIX(double, 4) } else { ULTRA_FIX(double, 1) }
    }
#undef ULTRA_FIX
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// Per-call edge weights -> sorted order: *dst is the plan's copy of `w` in its own edge order, permuted by a launch on
// `stream` unless the plan already holds this very vector (ultra_rspmm_weight_epoch).
static int sorted_weights(ultra_plan *p, const void *w, int dtype, hipStream_t stream, const void **dst) {
    // A launch that is being recorded into a hipGraph keeps its permuted copy in a buffer of its own (d.w_copy[1]): replays
    // then never overwrite the copy an eager caller may still hold a tag for, and inside ONE capture a tagged vector is
    // permuted once (a hit taken from outside the capture -- the warm-up runs -- would leave the replays without the
    // permutation: the capture id is part of the key).
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    unsigned long long cap_id = 0;
    if (hipStreamGetCaptureInfo(stream, &capturing, &cap_id) != hipSuccess) {
        (void)hipGetLastError();
        capturing = hipStreamCaptureStatusNone;
    }
    const bool in_cap = capturing != hipStreamCaptureStatusNone;
    if (!in_cap) cap_id = 0;
    const size_t w_bytes = (size_t)p->num_edge * (dtype == ULTRA_F32 ? 4 : 8);
    WeightCopy &c = p->d.w_copy[in_cap ? 1 : 0];
    int rc;
    if (!in_cap) {      // (both buffers exist before any capture begins: no allocation while a stream records)
        for (WeightCopy &b : p->d.w_copy)
            if ((rc = ensure_scratch(&b.buf, &b.bytes, w_bytes, p))) return rc;
    } else if (c.bytes < w_bytes) {
        return invalid("a weighted rspmm call is being captured on a plan that has not served one eagerly (run the step once "
                       "before capturing it: the plan's scratch buffers are allocated there)");
    }
    const bool hit = g_w_epoch != 0 && c.cap_id == cap_id && c.epoch == g_w_epoch && c.src == w && c.dtype == dtype && c.stream == stream;
    if (!hit) {
        const int blocks = (int)std::min<int64_t>((p->num_edge + 255) / 256, 4096);
        if (dtype == ULTRA_F32)
            hipLaunchKernelGGL(permute_weight_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float *)w,
                               p->d.perm, (float *)c.buf, p->num_edge);
        else
            hipLaunchKernelGGL(permute_weight_kernel<double>, dim3(blocks), dim3(256), 0, stream, (const double *)w,
                               p->d.perm, (double *)c.buf, p->num_edge);
        HIP_TRY(hipGetLastError());
        c.epoch = g_w_epoch, c.src = w, c.dtype = dtype, c.stream = stream, c.cap_id = cap_id;   // (epoch 0: untagged, never hit)
    }
    *dst = c.buf;
    return ULTRA_OK;
}

// The dtype x VEC x MODE ladder of the walk kernels' launchers: calls launch(T(), VEC, MODE) with the element type as a
// value and the two numbers as std::integral_constant.
template <typename Launch>
static hipError_t launch_walk_variant(int dtype, int vec, int mode, const Launch &launch) {
    const auto of_type = [&](auto t) {
        using std::integral_constant;
        if (vec == 1) return launch(t, integral_constant<int, 1>(), integral_constant<int, 0>());
        if (mode == 0) return launch(t, integral_constant<int, 4>(), integral_constant<int, 0>());
        if (mode == 1) return launch(t, integral_constant<int, 4>(), integral_constant<int, 1>());
        return launch(t, integral_constant<int, 4>(), integral_constant<int, 2>());
    };
    return dtype == ULTRA_F32 ? of_type(float()) : of_type(double());
}

// forward_update on the order kernel: which form applies the layer update -- 1, the tail after the walk, or 3, beside it --
// with the LDS size and the stream / chain lists that form reads.  UNSUPPORTED where the call or the form asked for does not fit.
static int choose_update_form(ultra_plan *p, const OrderParams::Update *upd, const Schedule *sched, const DevInfo &di,
                              size_t rel_bytes, size_t ring_bytes, OrderParams *op, size_t *lds) {
    int rc;
    if (!op->use_streams || op->row_len != 64) {
        set_error("ultra_rspmm_forward_update: this call is not served by the stream walk (fp32, 64-element rows, unit "
                  "weights, relation slice in LDS, point boundary or none)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    op->upd = *upd;
    op->upd.prow = sched->d_prow;
    op->upd.prow_ptr = sched->d_prow_ptr;
    op->upd.mode = 1;
    *lds = std::max(*lds, (size_t)UPDATE_LDS_FLOATS * sizeof(float));   // (the weight image takes the dead relation slice's place)
    Schedule *sched12 = nullptr;
    // (the form beside the walk reads the twelve-walker schedules, whose records are pre-multiplied by the 256-byte pitch
    // of whole-span rows: plan.hpp ULTRA_STREAM_PRESHIFT)
    const bool pitch_ok = !ULTRA_STREAM_PRESHIFT || op->x_row_bytes == 256u;
    // Form 3: beside the walk with the rows passing through LDS -- the walkers park every finished aggregate row AND its x
    // row (a marker step gathers at its own row's offset) in a 64-row ring; the update waves keep the weight matrix in
    // registers, so the room is there even beside a 474-relation slice, and they take no memory round trip (DESIGN.md
    // 3.8c).  Measured on MI355X, layer in a hipGraph, against the tail form: FB15k237 bs 8 85.7 us vs 94.4, bs 16 166 vs
    // 192, bs 4 68.5 vs 69.6, max aggregate 110.6 vs 113.7, CoDEx-L bs 8 324 vs 375 -- but WN18RR bs 8 141 vs 128: with 5
    // steps a row the update is most of the work, and here only four of the sixteen waves do it.  So: on request
    // (ultra_tuning.reserved[2] == 3) always, by default (0) from 10 steps a row up; 1 asks for the tail form.
    const bool walk_heavy = (double)(p->num_edge + p->num_out) >= 10.0 * (double)p->num_out;
    const bool want3 = update_form() == 3 || (update_form() == 0 && walk_heavy);
    if (want3 && pitch_ok && ORDER_WAVES == 16 && upd->out_stride_row * (int64_t)sizeof(float) == (int64_t)op->x_row_bytes) {
        if ((rc = get_schedule(p, op->nparts, &sched12, ORDER_WALKERS))) return rc;
        const size_t overlay = std::max(ring_bytes, (size_t)UPD2_OVERLAY_BYTES);
        const size_t need = rel_bytes + overlay + UPD2_CTL_BYTES;
        if (need <= di.lds_optin && sched12->max_chain_rows <= UPD2_MAX_CHAIN_ROWS) {
            op->upd.mode = 3;
            op->max_stream_steps = sched12->max_stream_steps;
            op->upd.ctl_off = (uint32_t)(rel_bytes + overlay);
            op->srec = sched12->d_srec;
            op->sdesc = reinterpret_cast<const int2 *>(sched12->d_sdesc);
            op->chunk_ptr = sched12->d_chunk_ptr;      // (its own chain list: shorter chain rows are stream rows there)
            op->chunks = reinterpret_cast<const int4 *>(sched12->d_chunks);
            *lds = need;
        }
    }
    if (update_form() == 2) {
        set_error("ultra_rspmm_forward_update: update form 2 (rows by reference) was removed in ABI 6; ask for 0 (the library's "
                  "choice), 1 (tail) or 3 (beside the walk, rows through LDS)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (update_form() >= 2 && op->upd.mode != update_form()) {
        set_error("ultra_rspmm_forward_update: the update beside the walk does not fit this call (LDS / rows per workgroup)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    return ULTRA_OK;
}

// The operands of a forward call as both kernel routes read them (forward_impl has checked them).
static FwdParams fwd_params(const ultra_plan *p, int mul, const void *w, const ultra_mat *rel, const ultra_mat *x,
                            const ultra_mat *bnd, const ultra_mat *out, int SPAN, int64_t esz, const FwdCall &call) {
    const int64_t *bnd_rows = call.bnd_rows;
    FwdParams fp;
    std::memset(&fp, 0, sizeof(fp));
    fp.col = p->d.col;
    fp.type = p->d.type;
    fp.packed = p->d.packed;
    fp.items = p->d.items;
    fp.n_w = (int32_t)p->n_w;
    fp.n_item = (int32_t)p->items.size();
    fp.n_unit = (int32_t)p->n_unit;
    if (mul != BIN_RHS) fp.rel = MatArg{rel->ptr, rel->stride_outer, rel->stride_row};
    if (mul != BIN_LHS) fp.x = MatArg{x->ptr, x->stride_outer, x->stride_row};
    if (bnd) fp.bnd = MatArg{bnd->ptr, bnd->stride_outer, bnd_rows ? 0 : bnd->stride_row};
    fp.bnd_rows = bnd ? reinterpret_cast<const long long *>(bnd_rows) : nullptr;
    fp.out = out->ptr;
    fp.out_stride_outer = out->stride_outer;
    fp.out_stride_row = out->stride_row;
    fp.n_outer = (int32_t)out->n_outer;
    fp.row_len = (int32_t)out->row_len;
    fp.spans_per_outer = (int32_t)((out->row_len + SPAN - 1) / SPAN);
    fp.n_span = fp.spans_per_outer * fp.n_outer;
    fp.num_rel = (int32_t)p->num_rel;
    fp.num_in = (int32_t)p->num_in;
    fp.type_bits = p->type_bits;
    fp.unit_w = w ? 0 : 1;
    fp.packed_on = p->packed_ok ? 1 : 0;
    fp.has_bnd = bnd ? 1 : 0;
    fp.keep_mode = (w && call.keep_mode) ? 1 : 0;
    if (mul != BIN_LHS) fp.x_row_bytes = (uint32_t)(x->stride_row * esz);
    if (mul != BIN_RHS) fp.rel_row_bytes = (uint32_t)(rel->stride_row * esz);
    fp.rot_half_bytes = (uint32_t)((out->row_len / 2) * esz);
    return fp;
}

// Reference-order plans: the order kernels (no scratch, no fix-up launch).  `fp` describes the operands (forward_impl).
static int forward_order(ultra_plan *p, int sum, int mul, int dtype, const void *w, const ultra_mat *x, const ultra_mat *bnd,
                         const ultra_mat *out, hipStream_t stream, const FwdCall &call, const FwdParams &fp, const DevInfo &di,
                         size_t ring_bytes, bool point_fill) {
    const size_t esz = dtype == ULTRA_F32 ? 4 : 8;
    const int64_t row_len = out->row_len;
    const int64_t *bnd_rows = call.bnd_rows;
    int rc;
    // (+ one row: the stream walk's row markers carry relation index num_rel)
    const size_t rel_bytes = (mul != BIN_RHS) ? (size_t)(p->num_rel + 1) * 64 * esz : 0;
    const bool rel_lds = g_tuning.rel_lds != 0 && rel_bytes > 0 && rel_bytes + ring_bytes <= di.lds_optin;
    const int grid = launch_grid(di);
    OrderParams op;
    std::memset(&op, 0, sizeof(op));
    op.smod = std::min<int32_t>(fp.n_span, grid);
    op.nparts = grid / op.smod;
    Schedule *sched = nullptr;
    if ((rc = get_schedule(p, op.nparts, &sched))) return rc;
    op.rec = p->d.rec;
    op.perm = p->d.perm;
    op.w = w;
    op.items = reinterpret_cast<const int4 *>(p->d.items);
    op.unit_ptr = sched->d_unit_ptr;
    op.units = sched->d_units;
    op.chunk_ptr = sched->d_chunk_ptr;
    op.chunks = reinterpret_cast<const int4 *>(sched->d_chunks);
    op.n_chain = (int32_t)p->n_chain;
    op.n_item = (int32_t)p->items.size();
    op.rel = fp.rel, op.x = fp.x, op.bnd = fp.bnd;
    op.bnd_rows = fp.bnd_rows;
    op.bnd_fill_on = point_fill ? 1 : 0;
    op.bnd_fill = 0.f;
    op.out = fp.out;
    op.out_stride_outer = fp.out_stride_outer, op.out_stride_row = fp.out_stride_row;
    op.n_outer = fp.n_outer, op.row_len = fp.row_len, op.spans_per_outer = fp.spans_per_outer, op.n_span = fp.n_span;
    op.num_rel = fp.num_rel;
    op.has_bnd = fp.has_bnd;
    op.has_chain = p->n_chain > 0 ? 1 : 0;
    op.keep_mode = fp.keep_mode;
    op.w_stride_outer = (w && call.w_samples) ? (int32_t)call.w_stride_outer : 0;
    op.x_row_bytes = fp.x_row_bytes, op.rel_row_bytes = fp.rel_row_bytes;
    op.trace = g_order_trace;
    op.err = device_error_word();
    // The group streams (assembly walk) serve the inference configuration: fp32, unit weights, relation slice in
    // LDS, mul / add messages, whole 64-element spans, no boundary or a point boundary, source and output rows of
    // one stride (a marker's gather offset is its store offset), every output row also a source row.
    op.srec = sched->d_srec;
    op.sdesc = reinterpret_cast<const int2 *>(sched->d_sdesc);
    op.use_streams = (unit_walk() == 0 && dtype == ULTRA_F32 && rel_lds && !w && (mul == BIN_MUL || mul == BIN_ADD) &&
                      row_len % 64 == 0 && (!bnd || bnd_rows) && out->stride_row == x->stride_row &&
                      p->num_out <= p->num_in && (uint64_t)p->num_out * (uint64_t)out->stride_row * esz < (1ull << 32))
                         ? 1
                         : 0;
    size_t lds = (rel_lds ? rel_bytes : 0) + ring_bytes;
    if (call.upd && (rc = choose_update_form(p, call.upd, sched, di, rel_bytes, ring_bytes, &op, &lds))) return rc;
    if (call.ev_before) HIP_TRY(hipEventRecord(call.ev_before, stream));
#define ULTRA_ORDER_LAUNCH(T_)                                                                          \
    (rel_lds ? (w ? launch_order_variant<T_, true, true>(sum, mul, op, grid, lds, stream)                \
                  : launch_order_variant<T_, true, false>(sum, mul, op, grid, lds, stream))              \
             : (w ? launch_order_variant<T_, false, true>(sum, mul, op, grid, lds, stream)               \
                  : launch_order_variant<T_, false, false>(sum, mul, op, grid, lds, stream)))
    const hipError_t e = dtype == ULTRA_F32 ? ULTRA_ORDER_LAUNCH(float) : ULTRA_ORDER_LAUNCH(double);
#undef ULTRA_ORDER_LAUNCH
    if (e != hipSuccess) return hip_fail(e, "rspmm_order_kernel launch");
    if (call.ev_after) HIP_TRY(hipEventRecord(call.ev_after, stream));
    return ULTRA_OK;
}

// The general walk (rotate messages included) and the fix-up launch of its split rows.  `fp` describes the operands
// (forward_impl); the route adds what is its own: sorted weights, the partial rows, the launch geometry.
static int forward_walk(ultra_plan *p, int sum, int mul, int dtype, const void *w, const ultra_mat *bnd, const ultra_mat *out,
                        hipStream_t stream, const FwdCall &call, FwdParams &fp, const DevInfo &di, int VEC, bool rot_far) {
    const size_t esz = dtype == ULTRA_F32 ? 4 : 8;
    const bool rot = bin_is_rot(mul);
    int rc;
    if (w && p->num_edge > 0 && (rc = sorted_weights(p, w, dtype, stream, &fp.w_sorted))) return rc;
    if (p->n_slot > 0) {
        if ((rc = ensure_scratch(&p->d.partial, &p->d.partial_bytes, (size_t)p->n_slot * fp.n_outer * fp.row_len * esz, p)))
            return rc;
        fp.partial = p->d.partial;
    }

    // variant selection
    const int SPAN = 16 * VEC;
    const size_t rel_bytes = (mul != BIN_RHS) ? (size_t)p->num_rel * SPAN * esz : 0;
    const size_t x_bytes = (mul != BIN_LHS) ? (size_t)p->num_in * SPAN * esz : 0;
    int mode = MODE_GLOBAL;
    if (VEC == 4 && !rot_far) {
        if (g_tuning.x_lds != 0 && g_tuning.rel_lds != 0 && rel_bytes + x_bytes <= di.lds_optin && x_bytes > 0)
            mode = MODE_ALL_LDS;
        else if (g_tuning.rel_lds != 0 && rel_bytes <= di.lds_optin && rel_bytes > 0)
            mode = MODE_REL_LDS;
    }
    const size_t lds = mode == MODE_ALL_LDS ? rel_bytes + x_bytes : (mode == MODE_REL_LDS ? rel_bytes : 0);
    const int threads = g_tuning.threads > 0 ? g_tuning.threads : 1024;
    const int grid = launch_grid(di);
    fp.smod = std::min<int32_t>(fp.n_span, grid);
    fp.nparts = grid / fp.smod;

    if (call.ev_before) HIP_TRY(hipEventRecord(call.ev_before, stream));
    const int rmul = rot_far ? mul + (BIN_ROTG - BIN_ROT) : mul;
    const hipError_t e = launch_walk_variant(dtype, VEC, mode, [&](auto t, auto vec, auto lds_mode) {
        using T = decltype(t);
        constexpr int V = decltype(vec)::value, M = decltype(lds_mode)::value;
        return rot ? launch_rot_variant<T, V, M>(sum, rmul, fp, grid, threads, lds, stream)
                   : launch_fwd_variant<T, V, M>(sum, mul, fp, grid, threads, lds, stream);
    });
    if (e != hipSuccess) return hip_fail(e, "rspmm_fwd_kernel launch");
    if (call.ev_after) HIP_TRY(hipEventRecord(call.ev_after, stream));
    return launch_fixup(p, out, sum, dtype, VEC, stream, bnd ? &fp.bnd : nullptr, fp.bnd_rows);
}

// Generic forward on a plan (internal: accepts the BIN_LHS / BIN_RHS variants used by backward): validates, describes the
// operands, and hands the call to the one route that serves it -- the dense format, the reference-order kernels or the walk.
static int forward_impl(ultra_plan *p, int sum, int mul, int dtype, const void *w, const ultra_mat *rel,
                        const ultra_mat *x, const ultra_mat *bnd, const ultra_mat *out, hipStream_t stream,
                        const FwdCall &call = FwdCall()) {
    const int64_t *bnd_rows = call.bnd_rows;
    if (!p) return invalid("plan is NULL");
    (void)hipGetLastError();   // drop any stale error left by other users of the HIP runtime
    if (int derr = take_device_error()) return derr;   // (an earlier launch ended on a bounded wait: say so now)
    // (mul: an internal BIN_* code -- the public entries have mapped ULTRA_MUL_ROTATE to BIN_ROT)
    const bool rot = mul >= BIN_ROT && mul <= BIN_ROT_CX;
    if (sum < 0 || sum > 2 || mul < 0 || (mul > 3 && !rot)) return invalid("unknown sum/mul code");
    if (rot && mul != BIN_ROT && sum != ULTRA_SUM_ADD) return invalid("unknown sum/mul code");
    if (dtype != ULTRA_F32 && dtype != ULTRA_F64) return invalid("dtype must be ULTRA_F32 or ULTRA_F64");
    if (!out || !out->ptr) return invalid("output is NULL");
    const int64_t n_outer = out->n_outer, row_len = out->row_len;
    if (n_outer <= 0 || row_len <= 0) return invalid("output: empty n_outer / row_len");
    if (rot && (row_len & 1)) return invalid("rotate: row_len must be even (a row is real half | imaginary half)");
    int rc;
    if ((rc = check_mat(out, "output", p->num_out, n_outer, row_len))) return rc;
    if (mul != BIN_RHS && (rc = check_mat(rel, "relation", p->num_rel, n_outer, row_len))) return rc;
    if (mul != BIN_LHS && (rc = check_mat(x, "input", p->num_in, n_outer, row_len))) return rc;
    if (bnd_rows && !bnd) return invalid("a point boundary needs its value rows");
    // min / max with a point boundary: the boundary tensor it stands for is ZERO off the query rows, and zero is not the
    // identity of min / max -- every other row meets the value 0 at its flush (layers.py:206-207)
    const bool point_fill = bnd_rows && sum != ULTRA_SUM_ADD;
    if (bnd && (rc = check_mat(bnd, "boundary", bnd_rows ? 1 : p->num_out, n_outer, row_len))) return rc;
    if (p->num_out == 0) return ULTRA_OK;
    if ((rc = upload_plan(p))) return rc;
    if (call.upd && ((p->flags & ULTRA_PLAN_DENSE) || !(p->flags & ULTRA_PLAN_EXACT_ORDER))) {
        set_error("ultra_rspmm_forward_update: served by reference-order plans in the sparse format only");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (point_fill && ((p->flags & ULTRA_PLAN_DENSE) || !(p->flags & ULTRA_PLAN_EXACT_ORDER))) {
        set_error("a point boundary under min / max is served by reference-order plans in the sparse format only");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (call.w_samples && (rot || (p->flags & ULTRA_PLAN_DENSE) || !(p->flags & ULTRA_PLAN_EXACT_ORDER))) {
        set_error("ultra_rspmm_forward_masked_samples: served by reference-order plans in the sparse format, mul / add messages");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (rot && (p->flags & ULTRA_PLAN_DENSE)) {
        set_error("rotate messages are served by the plans in the sparse format");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (p->flags & ULTRA_PLAN_DENSE) {
        if (call.ev_before) HIP_TRY(hipEventRecord(call.ev_before, stream));
        if ((rc = launch_dense_forward(p, sum, mul, dtype, w, rel, x, bnd, bnd_rows, out, stream))) return rc;
        if (call.ev_after) HIP_TRY(hipEventRecord(call.ev_after, stream));
        return ULTRA_OK;
    }
    DevInfo di;
    if ((rc = device_info(&di))) return rc;

    const size_t esz = dtype == ULTRA_F32 ? 4 : 8;
    const int64_t step = dtype == ULTRA_F32 ? 4 : 2;  // elements per 16 bytes
    bool vec4 = (row_len % 4 == 0) && mat_vec_ok(out, step);
    if (mul != BIN_RHS) vec4 = vec4 && mat_vec_ok(rel, step);
    if (mul != BIN_LHS) vec4 = vec4 && mat_vec_ok(x, step);
    if (bnd) vec4 = vec4 && mat_vec_ok(bnd, step);
    // rotate: a lane's 16-byte chunk and its partner's (row_len / 2 elements away) lie in ONE half each
    if (rot) vec4 = vec4 && (row_len % 8 == 0);
    const int VEC = vec4 ? 4 : 1;
    const int SPAN = 16 * VEC;
    // ... and a row of exactly one span has its halves in lanes 0-7 | 8-15 of a group: the partner comes by a lane exchange.
    // Every other row length loads it (the BIN_ROTG* kernels, operands through L2).
    const bool rot_far = rot && !(VEC == 4 && row_len == SPAN);

    if ((p->flags & ULTRA_PLAN_TYPE_RUNS) && !(p->flags & ULTRA_PLAN_EXACT_ORDER)) {
        if (!(sum == ULTRA_SUM_ADD && mul == BIN_MUL)) {
            set_error("a ULTRA_PLAN_TYPE_RUNS plan serves add_mul only (distributivity)");
            return ULTRA_ERR_UNSUPPORTED;
        }
        mul = BIN_MUL_TYPED;
    }
    // 32-bit byte offsets inside one operand slice (uniform 64-bit base + 32-bit voffset loads)
    const auto slice_bytes = [&](const ultra_mat *m, int64_t rows) { return (uint64_t)rows * (uint64_t)m->stride_row * esz; };
    if ((mul != BIN_LHS && slice_bytes(x, p->num_in) >= (1ull << 32)) ||
        (mul != BIN_RHS && slice_bytes(rel, p->num_rel) >= (1ull << 32))) {
        set_error("rspmm: an operand slice (rows * stride_row) exceeds 4 GiB; use the batch-major layout");
        return ULTRA_ERR_UNSUPPORTED;
    }
    FwdParams fp = fwd_params(p, mul, w, rel, x, bnd, out, SPAN, (int64_t)esz, call);

    // (rotate: reference-order plans are walked by the general kernel -- one 16-lane group per row, chain rows included,
    // in sorted edge order; the order kernels and their generated walks serve mul / add)
    // ring: [2 halves][15 quads][64 lanes][4 messages]
    const size_t ring_bytes = p->n_chain > 0 ? (size_t)2 * CHAIN_SLOTS * 64 * esz : 0;
    if ((p->flags & ULTRA_PLAN_EXACT_ORDER) && !rot && VEC == 4 && general_walk() == 0 && p->num_in < (1 << 24) &&
        p->num_rel < (1 << 24) && (mul == BIN_LHS || x->stride_row * (int64_t)esz < (1 << 24)) &&
        (mul == BIN_RHS || rel->stride_row * (int64_t)esz < (1 << 24)) && ring_bytes <= di.lds_optin)
        return forward_order(p, sum, mul, dtype, w, x, bnd, out, stream, call, fp, di, ring_bytes, point_fill);
    if (call.upd) {
        set_error("ultra_rspmm_forward_update: this call is not served by the reference-order kernels");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (call.w_samples) {
        set_error("ultra_rspmm_forward_masked_samples: this call is not served by the reference-order kernels (row length, "
                  "alignment or tuning)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    // The general walk below applies a point boundary at row bnd_rows[outer] only: it has no fill for the OTHER rows, which under
    // min / max must meet the boundary tensor's zeros (layers.py:206-207).  A reference-order plan that missed the order kernels
    // (rows not a multiple of 4 elements, misaligned strides, general_walk tuning, 2^24 rows) therefore answers UNSUPPORTED -- the
    // layer then passes the dense boundary tensor -- instead of returning FLT_LOWEST / negative aggregates.
    if (point_fill) {
        set_error("a point boundary under min / max: this call is not served by the reference-order kernels (row length, "
                  "alignment or tuning); pass the boundary as a tensor");
        return ULTRA_ERR_UNSUPPORTED;
    }
    return forward_walk(p, sum, mul, dtype, w, bnd, out, stream, call, fp, di, VEC, rot_far);
}

static int ensure_backward_plans(ultra_plan *p) {
    if (p->tplan && p->rplan) return ULTRA_OK;
    if ((int64_t)p->h_row.size() != p->num_edge) return invalid("plan was built without its edge list; backward unavailable");
    ultra_plan_opts o;
    std::memset(&o, 0, sizeof(o));
    o.seg_len = p->seg_len;
    o.g_max = p->g_max;
    // The backward sums are scatter-adds in the reference (atomicAdd on the GPU, rspmm.cu:153-214): no summation order
    // to reproduce, so the transposed plans are always the re-associating kind (split hub rows, balanced units).
    o.flags = p->flags & ~ULTRA_PLAN_EXACT_ORDER;
    // (a plan derived while captured graphs hold its parent is held by the same graphs: it inherits the pin count, so the
    // graphs' later -1 finds it pinned -- ultra_plan_pin)
    if (!p->tplan) {
        p->tplan = build_plan(p->h_col.data(), p->h_row.data(), p->h_type.data(), p->num_edge, p->num_in, p->num_out,
                              p->num_rel, &o, false);
        p->tplan->pinned = p->pinned;
    }
    if (!p->rplan) {
        p->rplan = build_plan(p->h_type.data(), p->h_col.data(), p->h_row.data(), p->num_edge, p->num_rel, p->num_in,
                              p->num_out, &o, false);
        p->rplan->pinned = p->pinned;
    }
    return ULTRA_OK;
}

// Backward of min / max as gathers: the destinations walk the transposed (which = 0: input_grad) and the relation-major
// (1: relation_grad) plan -- no atomics, the same bits run to run.  `launch(rel_grad, gp, grid)` starts the gather kernel
// `what`, whose spans make spans_per_outer a row; the fix-up of the split rows takes fix_vec-wide chunks.
template <typename Launch>
static int backward_gather(ultra_plan *p, int dtype, const void *w, const EdgeParams &ep, const ultra_mat *xgrad,
                           const ultra_mat *rgrad, int32_t spans_per_outer, int fix_vec, const char *what, hipStream_t stream,
                           const Launch &launch) {
    const size_t esz = dtype == ULTRA_F32 ? 4 : 8;
    int rc;
    if ((rc = ensure_backward_plans(p))) return rc;
    for (int which = 0; which < 2; ++which) {
        ultra_plan *q = which == 0 ? p->tplan : p->rplan;
        const ultra_mat *dst = which == 0 ? xgrad : rgrad;
        if ((rc = upload_plan(q))) return rc;
        if (q->n_slot > 0 &&
            (rc = ensure_scratch(&q->d.partial, &q->d.partial_bytes, (size_t)q->n_slot * ep.n_outer * ep.row_len * esz, q)))
            return rc;
        GatherBwdParams gp;
        std::memset(&gp, 0, sizeof(gp));
        gp.items = q->d.items;
        gp.n_item = (int32_t)q->items.size();
        gp.col = q->d.col, gp.type = q->d.type, gp.perm = q->d.perm;
        gp.w = w;
        gp.rel = ep.rel, gp.x = ep.x, gp.out = ep.out, gp.og = ep.og;
        gp.grad = dst->ptr, gp.grad_so = dst->stride_outer, gp.grad_sr = dst->stride_row;
        gp.partial = q->d.partial;
        gp.n_outer = ep.n_outer, gp.row_len = ep.row_len;
        gp.spans_per_outer = spans_per_outer;
        gp.n_span = gp.spans_per_outer * gp.n_outer;
        const int grid = 2048;
        gp.smod = std::min<int32_t>(gp.n_span, grid);
        gp.nparts = grid / gp.smod;
        const hipError_t e = launch(which == 1, gp, grid);
        if (e != hipSuccess) return hip_fail(e, what);
        if ((rc = launch_fixup(q, dst, 0, dtype, fix_vec, stream))) return rc;
    }
    return ULTRA_OK;
}

static int backward_impl(ultra_plan *p, int sum, int mul, int dtype, const void *w, const ultra_mat *rel,
                         const ultra_mat *x, const ultra_mat *outm, const ultra_mat *og, void *wgrad,
                         const ultra_mat *rgrad, const ultra_mat *xgrad, hipStream_t stream, const ultra_mat *xbase = nullptr) {
    // xbase (sum == add): input_grad = xbase + the gathered sum -- the input's gradient from its OTHER consumer (the layer
    // update, which reads the same input), added in the walk's epilogue instead of by a separate pass; may alias input_grad
    if (!p) return invalid("plan is NULL");
    if (xbase && (sum != ULTRA_SUM_ADD || !xgrad)) return invalid("input_grad_base is served under sum == add, with an input_grad");
    (void)hipGetLastError();
    if (p->flags & ULTRA_PLAN_DENSE) return invalid("a ULTRA_PLAN_DENSE plan has no backward; use the (row, col) plan");
    if (sum < 0 || sum > 2 || mul < 0 || mul > ULTRA_MUL_ROTATE) return invalid("unknown sum/mul code");
    const bool rot = mul == ULTRA_MUL_ROTATE;
    if (dtype != ULTRA_F32 && dtype != ULTRA_F64) return invalid("dtype must be ULTRA_F32 or ULTRA_F64");
    if (!og || !og->ptr) return invalid("output_grad is NULL");
    const int64_t n_outer = og->n_outer, row_len = og->row_len;
    if (n_outer <= 0 || row_len <= 0) return invalid("output_grad: empty n_outer / row_len");   // (as the forward: rspmm.cpp's checkSize)
    if (rot && (row_len & 1)) return invalid("rotate: row_len must be even (a row is real half | imaginary half)");
    int rc;
    if ((rc = check_mat(rel, "relation", p->num_rel, n_outer, row_len))) return rc;
    if ((rc = check_mat(x, "input", p->num_in, n_outer, row_len))) return rc;
    if ((rc = check_mat(outm, "output", p->num_out, n_outer, row_len))) return rc;
    if ((rc = check_mat(og, "output_grad", p->num_out, n_outer, row_len))) return rc;
    if ((rc = check_mat(rgrad, "relation_grad", p->num_rel, n_outer, row_len))) return rc;
    // input_grad == NULL (sum == add only): the caller takes the input gradient elsewhere -- the gather over the transposed
    // graph is an rspmm forward, and a graph with a dense-format twin runs it on the matrix cores (rspmm.py Plan.backward)
    if (!xgrad && sum != ULTRA_SUM_ADD) return invalid("input_grad may be NULL under sum == add only");
    if (xgrad && (rc = check_mat(xgrad, "input_grad", p->num_in, n_outer, row_len))) return rc;
    if (xbase && (rc = check_mat(xbase, "input_grad_base", p->num_in, n_outer, row_len))) return rc;
    if ((rc = upload_plan(p))) return rc;

    const int64_t step = dtype == ULTRA_F32 ? 4 : 2;
    const bool vec4 = (row_len % 4 == 0) && mat_vec_ok(rel, step) && mat_vec_ok(x, step) && mat_vec_ok(outm, step) &&
                      mat_vec_ok(og, step) && mat_vec_ok(rgrad, step) && (!xgrad || mat_vec_ok(xgrad, step));

    EdgeParams ep;
    std::memset(&ep, 0, sizeof(ep));
    ep.erow = p->d.erow;
    ep.col = p->d.col;
    ep.type = p->d.type;
    ep.perm = p->d.perm;
    ep.w = w;
    ep.num_edge = p->num_edge;
    ep.num_out = (int32_t)p->num_out;
    ep.rel = MatArg{rel->ptr, rel->stride_outer, rel->stride_row};
    ep.x = MatArg{x->ptr, x->stride_outer, x->stride_row};
    ep.out = MatArg{outm->ptr, outm->stride_outer, outm->stride_row};
    ep.og = MatArg{og->ptr, og->stride_outer, og->stride_row};
    ep.rgrad = rgrad->ptr;
    ep.rgrad_so = rgrad->stride_outer;
    ep.rgrad_sr = rgrad->stride_row;
    ep.xgrad = xgrad ? xgrad->ptr : nullptr;
    ep.xgrad_so = xgrad ? xgrad->stride_outer : 0;
    ep.xgrad_sr = xgrad ? xgrad->stride_row : 0;
    ep.wgrad = wgrad;
    ep.n_outer = (int32_t)n_outer;
    ep.row_len = (int32_t)row_len;

    if (sum == ULTRA_SUM_ADD) {      // both gradients are rspmm forwards over the transposed / relation-major plans
        if ((rc = ensure_backward_plans(p))) return rc;
        // input_grad[col] = sum_e w * d(rel (x) in)/d in * out_grad[row]   (rspmm.cpp:110-112)
        // rotate: ROT(conj(rel), out_grad) -- the same walk with the relation operand conjugated
        if (xgrad && (rc = forward_impl(p->tplan, ULTRA_SUM_ADD, rot ? BIN_ROT_CREL : mul == ULTRA_MUL_MUL ? BIN_MUL : BIN_RHS, dtype,
                                        w, rel, og, xbase, xgrad, stream)))
            return rc;
        // relation_grad[type] = sum_e w * d(rel (x) in)/d rel * out_grad[row]   (rspmm.cpp:106-108)
        // rotate: ROT(conj(input), out_grad), out_grad in the relation operand's place
        if ((rc = forward_impl(p->rplan, ULTRA_SUM_ADD, rot ? BIN_ROT_CX : mul == ULTRA_MUL_MUL ? BIN_MUL : BIN_LHS, dtype, w, og, x,
                               nullptr, rgrad, stream)))
            return rc;
        if (!wgrad || p->num_edge <= 0) return ULTRA_OK;
        if (rot) return launch_rot_edge_kernel(dtype, sum, /*want_ri=*/false, ep, stream);
        return launch_edge_kernel(dtype, vec4 ? 4 : 1, sum, mul, /*want_ri=*/false, ep, stream);
    }
    // rotate under min / max: the gather on its own kernel -- 16 complex elements a span, scalar loads, so EVERY even row
    // length and alignment takes it (no atomics on any route: the same bits run to run)
    if (rot && p->num_edge > 0) {
        const bool fix4 = (row_len % 4 == 0) && mat_vec_ok(rgrad, step) && mat_vec_ok(xgrad, step);
        const auto launch = [&](bool rel_grad, const GatherBwdParams &gp, int grid) {
            return dtype == ULTRA_F32 ? launch_rot_gather_bwd_t<float>(sum, rel_grad, gp, grid, stream)
                                      : launch_rot_gather_bwd_t<double>(sum, rel_grad, gp, grid, stream);
        };
        if ((rc = backward_gather(p, dtype, w, ep, xgrad, rgrad, (int32_t)((row_len / 2 + 15) / 16), fix4 ? 4 : 1,
                                  "rspmm_rot_minmax_bwd_gather_kernel launch", stream, launch)))
            return rc;
        return wgrad ? launch_rot_edge_kernel(dtype, sum, /*want_ri=*/false, ep, stream) : ULTRA_OK;
    }
    // min / max: gradient flows to every edge whose message equals the output (operator.cuh:62-64,75-77).  With whole
    // 16-byte chunks the destinations GATHER over the transposed / relation-major plans (no atomics, deterministic); the
    // reference's scatter with atomics (restated in rspmm_edge_bwd_kernel) remains for unaligned / odd-length rows.
    if (vec4 && row_len % 4 == 0 && p->num_edge > 0) {
        const auto launch = [&](bool rel_grad, const GatherBwdParams &gp, int grid) {
            return dtype == ULTRA_F32 ? launch_gather_bwd_t<float>(sum, mul, rel_grad, gp, grid, stream)
                                      : launch_gather_bwd_t<double>(sum, mul, rel_grad, gp, grid, stream);
        };
        if ((rc = backward_gather(p, dtype, w, ep, xgrad, rgrad, (int32_t)((row_len + 63) / 64), 4,
                                  "rspmm_minmax_bwd_gather_kernel launch", stream, launch)))
            return rc;
        return wgrad ? launch_edge_kernel(dtype, 4, sum, mul, /*want_ri=*/false, ep, stream) : ULTRA_OK;
    }
    if ((rc = launch_fill_zero(dtype, rgrad, p->num_rel, stream))) return rc;
    if ((rc = launch_fill_zero(dtype, xgrad, p->num_in, stream))) return rc;
    if (p->num_edge > 0 && !rot) return launch_edge_kernel(dtype, vec4 ? 4 : 1, sum, mul, /*want_ri=*/true, ep, stream);
    return ULTRA_OK;
}

// add_mul forward for an input that is zero outside one row per outer slice (NBFNet layer 0: the boundary condition).
static int forward_onehot_impl(ultra_plan *p, int dtype, const void *w, const ultra_mat *rel, const ultra_mat *x,
                               const int64_t *src_rows, const ultra_mat *bnd, const ultra_mat *out, hipStream_t stream) {
    if (!p) return invalid("plan is NULL");
    (void)hipGetLastError();
    if (dtype != ULTRA_F32 && dtype != ULTRA_F64) return invalid("dtype must be ULTRA_F32 or ULTRA_F64");
    if (!out || !out->ptr || !src_rows) return invalid("output / src_rows is NULL");
    if (p->flags & (ULTRA_PLAN_TYPE_RUNS | ULTRA_PLAN_DENSE)) return invalid("use the (row, col) plan for the one-hot path");
    const int64_t n_outer = out->n_outer, row_len = out->row_len;
    int rc;
    if ((rc = check_mat(out, "output", p->num_out, n_outer, row_len))) return rc;
    if ((rc = check_mat(rel, "relation", p->num_rel, n_outer, row_len))) return rc;
    if ((rc = check_mat(x, "input", p->num_in, n_outer, row_len))) return rc;
    if (bnd && (rc = check_mat(bnd, "boundary", p->num_out, n_outer, row_len))) return rc;
    if (p->num_out != p->num_in) return invalid("one-hot path needs a square graph (source rows are output rows)");
    if ((rc = ensure_backward_plans(p))) return rc;
    if ((rc = upload_plan(p->tplan))) return rc;
    const size_t esz = dtype == ULTRA_F32 ? 4 : 8;
    if (out->stride_row == row_len && (n_outer == 1 || out->stride_outer == out->n_row * row_len) && out->n_row == p->num_out &&
        aligned16(out->ptr) && ((size_t)n_outer * p->num_out * row_len * esz) % 16 == 0) {
        // contiguous: streaming 16-byte zero fill.  (A kernel rather than hipMemsetAsync: memset nodes captured into a
        // hipGraph were observed to replay wrongly once eager memsets interleave with the replays on ROCm 7.2.)
        const long long n16 = (long long)((size_t)n_outer * p->num_out * row_len * esz / 16);
        hipLaunchKernelGGL(zero16_kernel, dim3(1024), dim3(256), 0, stream, reinterpret_cast<float4 *>(out->ptr), n16);
        HIP_TRY(hipGetLastError());
    } else if ((rc = launch_fill_zero(dtype, out, p->num_out, stream))) {
        return rc;
    }
    const int64_t step = dtype == ULTRA_F32 ? 4 : 2;
    const bool vec4 = (row_len % 4 == 0) && mat_vec_ok(out, step) && mat_vec_ok(rel, step) && mat_vec_ok(x, step);
    OneHotParams op;
    std::memset(&op, 0, sizeof(op));
    op.trow_ptr = p->tplan->d.row_ptr;
    op.tcol = p->tplan->d.col;
    op.ttype = p->tplan->d.type;
    op.tperm = p->tplan->d.perm;
    op.w = w;
    op.src = src_rows;
    op.rel = MatArg{rel->ptr, rel->stride_outer, rel->stride_row};
    op.x = MatArg{x->ptr, x->stride_outer, x->stride_row};
    if (bnd) op.bnd = MatArg{bnd->ptr, bnd->stride_outer, bnd->stride_row};
    op.out = out->ptr;
    op.out_so = out->stride_outer;
    op.out_sr = out->stride_row;
    op.n_outer = (int32_t)n_outer;
    op.row_len = (int32_t)row_len;
    op.has_bnd = bnd ? 1 : 0;
    const dim3 grid(64, (unsigned)n_outer), block(256);   // 1024 sixteen-lane groups per outer slice
    if (dtype == ULTRA_F32) {
        if (vec4) hipLaunchKernelGGL((rspmm_onehot_kernel<float, 4>), grid, block, 0, stream, op);
        else hipLaunchKernelGGL((rspmm_onehot_kernel<float, 1>), grid, block, 0, stream, op);
    } else {
        if (vec4) hipLaunchKernelGGL((rspmm_onehot_kernel<double, 4>), grid, block, 0, stream, op);
        else hipLaunchKernelGGL((rspmm_onehot_kernel<double, 1>), grid, block, 0, stream, op);
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// Layer 0 of an NBFNet on its one-hot boundary condition (layer0_kernels.hpp).
static int layer0_impl(ultra_plan *p, const void *w, const ultra_mat *rel, const int64_t *src_rows, const void *src_vals,
                       const void *weight, const void *bias, const void *ln_w, const void *ln_b, float eps, int flags,
                       const ultra_mat *out, hipStream_t stream) {
    if (!p) return invalid("plan is NULL");
    (void)hipGetLastError();
    const bool only_fill = (flags & L0_ONLY_FILL) != 0;
    if (flags & ~(L0_LN | L0_RELU | L0_RESIDUAL | L0_MAX | L0_ONLY_FILL | L0_SKIP_FILL))
        return invalid("ultra_nbf_layer0: unknown flag bits " + std::to_string(flags & ~(L0_LN | L0_RELU | L0_RESIDUAL | L0_MAX | L0_ONLY_FILL | L0_SKIP_FILL)));
    if (only_fill && (flags & L0_SKIP_FILL)) return invalid("ultra_nbf_layer0: ULTRA_LAYER0_ONLY_FILL excludes ULTRA_LAYER0_SKIP_FILL");
    if (!out || !out->ptr || (!only_fill && (!src_rows || !weight))) return invalid("ultra_nbf_layer0: NULL operand");
    if ((flags & L0_LN) && (!ln_w || !ln_b)) return invalid("ultra_nbf_layer0: LayerNorm needs its weight and bias");
    if (p->flags & (ULTRA_PLAN_TYPE_RUNS | ULTRA_PLAN_DENSE)) return invalid("use the (row, col) plan for the layer-0 path");
    if (out->row_len != 64) {
        set_error("ultra_nbf_layer0: only hidden dim 64 is built (the ULTRA checkpoints' shape)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    const int64_t n_outer = out->n_outer;
    int rc;
    if ((rc = check_mat(out, "output", p->num_out, n_outer, 64))) return rc;
    if (!only_fill && (rc = check_mat(rel, "relation", p->num_rel, n_outer, 64))) return rc;
    if (p->num_out != p->num_in) return invalid("layer-0 path needs a square graph (source rows are output rows)");
    if (!mat_vec_ok(out, 4) || (!only_fill && (!mat_vec_ok(rel, 4) || !aligned16(weight) || (src_vals && !aligned16(src_vals)))))
        return invalid("ultra_nbf_layer0: operands must be 16-byte aligned with strides that are multiples of 4");
    if (n_outer == 0 || p->num_out == 0) return ULTRA_OK;
    Layer0Params lp;
    std::memset(&lp, 0, sizeof(lp));
    if (!only_fill) {
        if ((rc = ensure_backward_plans(p))) return rc;
        if ((rc = upload_plan(p->tplan))) return rc;
        if ((rc = upload_plan(p))) return rc;
        if (!p->d.self_loop) return invalid("plan was built without its edge list; layer-0 path unavailable");
        lp.trow_ptr = p->tplan->d.row_ptr;
        lp.tcol = p->tplan->d.col;
        lp.ttype = p->tplan->d.type;
        lp.tperm = p->tplan->d.perm;
        lp.self_loop = p->d.self_loop;
        lp.rel = MatArg{rel->ptr, rel->stride_outer, rel->stride_row};
    }
    lp.w = static_cast<const float *>(w);
    lp.src = src_rows;
    lp.q = static_cast<const float *>(src_vals);
    lp.weight = static_cast<const float *>(weight);
    lp.bias = static_cast<const float *>(bias);
    lp.ln_w = static_cast<const float *>(ln_w);
    lp.ln_b = static_cast<const float *>(ln_b);
    lp.out = static_cast<float *>(out->ptr);
    lp.out_so = out->stride_outer;
    lp.out_sr = out->stride_row;
    lp.num_node = p->num_out;
    lp.n_outer = (int32_t)n_outer;
    lp.eps = eps;
    lp.flags = flags;
    const long long rows = (long long)n_outer * p->num_out;
    const int fill_blocks = (int)std::min<long long>((rows + 15) / 16, 1024);
    if (!(flags & L0_SKIP_FILL)) {
        hipLaunchKernelGGL(nbf_layer0_fill_kernel, dim3(fill_blocks), dim3(256), 0, stream, lp);
        HIP_TRY(hipGetLastError());
    }
    if (!only_fill) {
        // one 16-lane group per out-edge of the source, 64 groups a workgroup: enough workgroups that the hub with the most
        // out-edges is served in ONE pass (a pass is a chain of three dependent loads + the 128-term update: 3+ us; the FB15k237
        // shape's 9,067-edge hub took five of them on the former 32 workgroups a sample); workgroups past a source's last edge
        // leave at once
        ultra_plan *tp = p->tplan;
        if (tp->max_row_len < 0) {
            int32_t m = 0;
            for (size_t r = 0; r + 1 < tp->row_ptr.size(); ++r) m = std::max(m, tp->row_ptr[r + 1] - tp->row_ptr[r]);
            tp->max_row_len = m;
        }
        const unsigned l0_blocks = (unsigned)std::min(std::max((tp->max_row_len + 63) / 64, 32), 256);
        hipLaunchKernelGGL(nbf_layer0_rows_kernel, dim3(l0_blocks, (unsigned)n_outer), dim3(1024), 0, stream, lp);
        HIP_TRY(hipGetLastError());
    }
    return ULTRA_OK;
}

// The public forward entries' `mul` (ULTRA_MUL_*) as forward_impl's internal BIN_* code.
static int internal_mul(int32_t *mul) {
    if (*mul < 0 || *mul > ULTRA_MUL_ROTATE) return invalid("unknown mul code");
    if (*mul == ULTRA_MUL_ROTATE) *mul = BIN_ROT;
    return ULTRA_OK;
}

// ultra_rspmm_forward_update behind its device scope; `call` brings the point rows (and the events of the timed entry)
static int forward_update(ultra_plan *plan, int sum, int mul, const ultra_mat *relation, const ultra_mat *input,
                          const ultra_mat *point_values, const ultra_mat *aggregate, const void *weight, const void *bias,
                          const void *ln_weight, const void *ln_bias, float eps, int flags, const ultra_mat *output,
                          hipStream_t stream, FwdCall call) {
    if (mul < 0 || mul > 1) return invalid("unknown mul code");
    if ((call.bnd_rows == nullptr) != (point_values == nullptr)) return invalid("ultra_rspmm_forward_update: half a point boundary");
    if (!weight || !output || !output->ptr || !aggregate || !aggregate->ptr || ((flags & CONV_LN) && (!ln_weight || !ln_bias)))
        return invalid("ultra_rspmm_forward_update: NULL operand");
    if (flags & ~(CONV_LN | CONV_RELU | CONV_RESIDUAL | CONV_DBG_NO_MATRIX | CONV_DBG_NO_UPDATE | CONV_DBG_LOSE_ARRIVAL))
        return invalid("ultra_rspmm_forward_update: unknown flag");
    if (!plan) return invalid("plan is NULL");
    if (output->row_len != 64 || output->n_outer != aggregate->n_outer || output->n_row != aggregate->n_row ||
        output->stride_row < 64 || (output->stride_row % 4) != 0 || (output->stride_outer % 4) != 0 ||
        (reinterpret_cast<uintptr_t>(output->ptr) & 15) || output->ptr == aggregate->ptr || (input && output->ptr == input->ptr))
        return invalid("ultra_rspmm_forward_update: output must be a 16-byte aligned (n_outer, num_node, 64) tensor of its own");
    OrderParams::Update u;
    std::memset(&u, 0, sizeof(u));
    u.weight = (const float *)weight, u.bias = (const float *)bias;
    u.ln_w = (const float *)ln_weight, u.ln_b = (const float *)ln_bias;
    u.out = (float *)output->ptr;
    u.out_stride_outer = output->stride_outer, u.out_stride_row = output->stride_row;
    u.eps = eps, u.flags = flags;
    call.upd = &u;
    return forward_impl(plan, sum, mul, ULTRA_F32, nullptr, relation, input, point_values, aggregate, stream, call);
}

static ultra_mat dense2d(const void *ptr, int64_t rows, int64_t dim) {
    ultra_mat m;
    m.ptr = const_cast<void *>(ptr);
    m.n_outer = 1;
    m.stride_outer = 0;
    m.n_row = rows;
    m.stride_row = dim;
    m.row_len = dim;
    return m;
}

// The reference-shaped stateless exports: copy the edge list to the host, check sortedness
// (rspmm.py:16-18), build a throw-away plan, run, free.
static int stateless_plan(ultra_plan **plan, const int64_t *ei_dev, const int64_t *et_dev, int64_t E, int64_t N,
                          int64_t R, hipStream_t stream) {
    *plan = nullptr;
    if (E < 0 || N < 0 || R < 0) return invalid("negative size");
    std::vector<int64_t> ei((size_t)2 * E), et((size_t)E);
    HIP_TRY(hipStreamSynchronize(stream));
    if (E > 0) {
        HIP_TRY(hipMemcpy(ei.data(), ei_dev, sizeof(int64_t) * 2 * E, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(et.data(), et_dev, sizeof(int64_t) * E, hipMemcpyDeviceToHost));
        int64_t maxc = 0;
        for (int64_t e = 0; e < E; ++e) maxc = std::max(maxc, ei[(size_t)(E + e)]);
        for (int64_t e = 1; e < E; ++e) {
            const int64_t k0 = ei[(size_t)e - 1] * (maxc + 1) + ei[(size_t)(E + e - 1)];
            const int64_t k1 = ei[(size_t)e] * (maxc + 1) + ei[(size_t)(E + e)];
            if (k1 < k0) {
                set_error("Expect sorted `edge_index`");
                return ULTRA_ERR_UNSORTED;
            }
        }
    }
    ultra_plan_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.flags = ULTRA_PLAN_EXACT_ORDER;      // the reference's summation order (rspmm.cpp:61-72)
    return ultra_plan_create(plan, ei.data(), et.data(), E, N, N, R, &opts);
}

}  // namespace ultra

using namespace ultra;

extern "C" {

int32_t ultra_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t ultra_plan_upload(ultra_plan *plan) {
    if (!plan) return invalid("plan is NULL");
    return upload_plan(plan);
}

int32_t ultra_plan_pin(ultra_plan *plan, int32_t delta) {
    if (!plan) return invalid("plan is NULL");
    // (derived backward plans inherit their parent's count when they are built: ensure_backward_plans)
    const auto bump = [&](ultra_plan *q) { q->pinned = std::max<int32_t>(0, q->pinned + delta); };
    bump(plan);
    if (plan->tplan) bump(plan->tplan);
    if (plan->rplan) bump(plan->rplan);
    return ULTRA_OK;
}

int32_t ultra_plan_destroy(ultra_plan *plan) {
    if (!plan) return ULTRA_OK;
    if (plan->tplan) ultra_plan_destroy(plan->tplan);
    if (plan->rplan) ultra_plan_destroy(plan->rplan);
    free_device(plan);
    delete plan;
    return ULTRA_OK;
}

int32_t ultra_rspmm_weight_epoch(int64_t epoch) {
    g_w_epoch = epoch;
    return ULTRA_OK;
}

int32_t ultra_rspmm_forward(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const void *edge_weight_dev,
                            const ultra_mat *relation, const ultra_mat *input, const ultra_mat *boundary,
                            const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    WeightEpochScope weight_epoch_scope;
    if (int rc = internal_mul(&mul)) return rc;
    return forward_impl(plan, sum, mul, dtype, edge_weight_dev, relation, input, boundary, output,
                        reinterpret_cast<hipStream_t>(stream));
}

int32_t ultra_rspmm_forward_masked(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const void *edge_keep_dev,
                                   const ultra_mat *relation, const ultra_mat *input, const ultra_mat *boundary,
                                   const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    WeightEpochScope weight_epoch_scope;
    if (int rc = internal_mul(&mul)) return rc;
    if (!edge_keep_dev) return invalid("ultra_rspmm_forward_masked: edge_keep is NULL");
    FwdCall call;
    call.keep_mode = 1;
    return forward_impl(plan, sum, mul, dtype, edge_keep_dev, relation, input, boundary, output,
                        reinterpret_cast<hipStream_t>(stream), call);
}

int32_t ultra_rspmm_forward_masked_samples(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const void *edge_keep_dev,
                                           int64_t keep_stride, const ultra_mat *relation, const ultra_mat *input,
                                           const ultra_mat *boundary, const ultra_mat *output, void *stream) {
    if (!plan) return invalid("plan is NULL");
    if (keep_stride < plan->num_edge) return invalid("ultra_rspmm_forward_masked_samples: keep_stride < num_edge");
    if (!edge_keep_dev) return invalid("ultra_rspmm_forward_masked_samples: edge_keep is NULL");
    if (!output || !output->ptr) return invalid("output is NULL");
    if (output->n_outer == 0) return ULTRA_OK;
    if (keep_stride > INT32_MAX) {
        set_error("ultra_rspmm_forward_masked_samples: keep_stride beyond 2^31 - 1 elements");
        return ULTRA_ERR_UNSUPPORTED;
    }
    ULTRA_DEVICE_SCOPE(stream, output->ptr);
    WeightEpochScope weight_epoch_scope;
    if (int rc = internal_mul(&mul)) return rc;
    FwdCall call;
    call.keep_mode = 1;
    call.w_samples = true;
    call.w_stride_outer = keep_stride;
    return forward_impl(plan, sum, mul, dtype, edge_keep_dev, relation, input, boundary, output,
                        reinterpret_cast<hipStream_t>(stream), call);
}

int32_t ultra_rspmm_forward_point(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const void *edge_weight_dev,
                                  const ultra_mat *relation, const ultra_mat *input, const int64_t *point_rows_dev,
                                  const ultra_mat *point_values, const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    WeightEpochScope weight_epoch_scope;
    if (int rc = internal_mul(&mul)) return rc;
    if (!point_rows_dev || !point_values) return invalid("ultra_rspmm_forward_point: NULL point boundary");
    return forward_impl(plan, sum, mul, dtype, edge_weight_dev, relation, input, point_values, output,
                        reinterpret_cast<hipStream_t>(stream), FwdCall{point_rows_dev});
}

int32_t ultra_rspmm_forward_update(ultra_plan *plan, int32_t sum, int32_t mul, const ultra_mat *relation, const ultra_mat *input,
                                   const int64_t *point_rows_dev, const ultra_mat *point_values, const ultra_mat *aggregate,
                                   const void *weight, const void *bias, const void *ln_weight, const void *ln_bias, float eps,
                                   int32_t flags, const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return forward_update(plan, sum, mul, relation, input, point_values, aggregate, weight, bias, ln_weight, ln_bias, eps, flags,
                          output, reinterpret_cast<hipStream_t>(stream), FwdCall{point_rows_dev});
}

int32_t ultra_rspmm_forward_onehot(ultra_plan *plan, int32_t dtype, const void *edge_weight_dev,
                                   const ultra_mat *relation, const ultra_mat *input, const int64_t *src_rows_dev,
                                   const ultra_mat *boundary, const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return forward_onehot_impl(plan, dtype, edge_weight_dev, relation, input, src_rows_dev, boundary, output,
                               reinterpret_cast<hipStream_t>(stream));
}

int32_t ultra_nbf_layer0(ultra_plan *plan, const void *edge_weight_dev, const ultra_mat *relation, const int64_t *src_rows_dev,
                         const void *src_values_dev, const void *weight, const void *bias, const void *ln_weight,
                         const void *ln_bias, float eps, int32_t flags, const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    return layer0_impl(plan, edge_weight_dev, relation, src_rows_dev, src_values_dev, weight, bias, ln_weight, ln_bias, eps,
                       flags, output, reinterpret_cast<hipStream_t>(stream));
}

int32_t ultra_nbf_dense_layer(ultra_plan *plan, const ultra_mat *relation, const ultra_mat *input, const ultra_mat *boundary,
                              const int64_t *point_rows_dev, const void *weight, const void *bias, const void *ln_weight,
                              const void *ln_bias, float eps, int32_t flags, const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    if (!plan) return invalid("plan is NULL");
    (void)hipGetLastError();
    if (!output || !output->ptr || !weight) return invalid("ultra_nbf_dense_layer: NULL operand");
    if ((flags & 1) && (!ln_weight || !ln_bias)) return invalid("ultra_nbf_dense_layer: LayerNorm needs its weight and bias");
    if (point_rows_dev && !boundary) return invalid("ultra_nbf_dense_layer: point rows without their values");
    const int64_t n_outer = output->n_outer;
    int rc;
    if ((rc = check_mat(output, "output", plan->num_out, n_outer, output->row_len))) return rc;
    if ((rc = check_mat(relation, "relation", plan->num_rel, n_outer, output->row_len))) return rc;
    if ((rc = check_mat(input, "input", plan->num_in, n_outer, output->row_len))) return rc;
    if (boundary && (rc = check_mat(boundary, "boundary", point_rows_dev ? 1 : plan->num_out, n_outer, output->row_len))) return rc;
    if (n_outer == 0 || plan->num_out == 0) return ULTRA_OK;
    if ((rc = upload_plan(plan))) return rc;
    if (flags & ULTRA_LAYER_REFERENCE_ORDER) {
        // (a launch-grid tuning below the CU count = this forward shares the chip with another batch in flight)
        DevInfo di;
        if ((rc = device_info(&di))) return rc;
        const bool shared_chip = g_tuning.grid > 0 && g_tuning.grid < di.cu;
        return launch_dense_order_layer(plan, relation, input, boundary, point_rows_dev, weight, bias, ln_weight, ln_bias, eps,
                                        flags & 7, output, reinterpret_cast<hipStream_t>(stream), shared_chip);
    }
    return launch_dense_layer(plan, relation, input, boundary, point_rows_dev, weight, bias, ln_weight, ln_bias, eps, flags,
                              output, reinterpret_cast<hipStream_t>(stream));
}

// what the two byte-adjacency entries ask of (a_ex_dev, num_node)
static int check_adjacency(const char *name, const void *a_ex_dev, int64_t num_node) {
    if (!a_ex_dev) return invalid(std::string(name) + ": the adjacency is NULL");
    if (num_node <= 0 || num_node > ULTRA_DENSE_MAX_IN_ROW)
        return invalid(std::string(name) + ": num_node must lie in [1, " + std::to_string(ULTRA_DENSE_MAX_IN_ROW) + "], got " +
                       std::to_string((long long)num_node));
    return ULTRA_OK;
}

int32_t ultra_nbf_dense_layer_adjacency(const void *a_ex_dev, int64_t num_node, const ultra_mat *relation, const ultra_mat *input,
                                        const ultra_mat *boundary, const int64_t *point_rows_dev, const void *weight,
                                        const void *bias, const void *ln_weight, const void *ln_bias, float eps, int32_t flags,
                                        const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    (void)hipGetLastError();
    int rc;
    if ((rc = check_adjacency("ultra_nbf_dense_layer_adjacency", a_ex_dev, num_node))) return rc;
    if (!(flags & ULTRA_LAYER_REFERENCE_ORDER))
        return invalid("ultra_nbf_dense_layer_adjacency: served in the reference's order only (ULTRA_LAYER_REFERENCE_ORDER)");
    if (!output || !output->ptr || !weight) return invalid("ultra_nbf_dense_layer_adjacency: NULL operand");
    if ((flags & 1) && (!ln_weight || !ln_bias)) return invalid("ultra_nbf_dense_layer_adjacency: LayerNorm needs its weight and bias");
    if (point_rows_dev && !boundary) return invalid("ultra_nbf_dense_layer_adjacency: point rows without their values");
    const int64_t n_outer = output->n_outer;
    if ((rc = check_mat(output, "output", num_node, n_outer, output->row_len))) return rc;
    if ((rc = check_mat(relation, "relation", 4, n_outer, output->row_len))) return rc;
    if ((rc = check_mat(input, "input", num_node, n_outer, output->row_len))) return rc;
    if (boundary && (rc = check_mat(boundary, "boundary", point_rows_dev ? 1 : num_node, n_outer, output->row_len))) return rc;
    if (n_outer == 0) return ULTRA_OK;
    DevInfo di;
    if ((rc = device_info(&di))) return rc;
    const bool shared_chip = g_tuning.grid > 0 && g_tuning.grid < di.cu;
    return launch_dense_order_layer_adjacency(a_ex_dev, num_node, relation, input, boundary, point_rows_dev, weight, bias, ln_weight,
                                              ln_bias, eps, flags & 7, output, reinterpret_cast<hipStream_t>(stream), shared_chip);
}

int32_t ultra_nbf_dense_layer0_adjacency(const void *a_ex_dev, int64_t num_node, const ultra_mat *relation, const int64_t *src_rows_dev,
                                         const void *src_values_dev, const void *weight, const void *bias, const void *ln_weight,
                                         const void *ln_bias, float eps, int32_t flags, const ultra_mat *output, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    (void)hipGetLastError();
    int rc;
    if ((rc = check_adjacency("ultra_nbf_dense_layer0_adjacency", a_ex_dev, num_node))) return rc;
    if (flags & ~(L0_LN | L0_RELU | L0_RESIDUAL | L0_MAX))
        return invalid("ultra_nbf_dense_layer0_adjacency: unknown flag bits " + std::to_string(flags & ~(L0_LN | L0_RELU | L0_RESIDUAL | L0_MAX)));
    if (!output || !output->ptr || !src_rows_dev || !weight) return invalid("ultra_nbf_dense_layer0_adjacency: NULL operand");
    if ((flags & L0_LN) && (!ln_weight || !ln_bias)) return invalid("ultra_nbf_dense_layer0_adjacency: LayerNorm needs its weight and bias");
    if (output->row_len != 64 || (flags & L0_MAX)) {
        set_error("ultra_nbf_dense_layer0_adjacency: the sum aggregate at hidden dim 64 (weight (64, 128)) in fp32 only");
        return ULTRA_ERR_UNSUPPORTED;
    }
    const int64_t n_outer = output->n_outer;
    if ((rc = check_mat(output, "output", num_node, n_outer, 64))) return rc;
    if ((rc = check_mat(relation, "relation", 4, n_outer, 64))) return rc;
    if (n_outer > 65535) return invalid("ultra_nbf_dense_layer0_adjacency: at most 65535 samples a launch");
    if (!mat_vec_ok(output, 4) || !mat_vec_ok(relation, 4) || !aligned16(weight) || (src_values_dev && !aligned16(src_values_dev)))
        return invalid("ultra_nbf_dense_layer0_adjacency: operands must be 16-byte aligned with strides that are multiples of 4");
    if (n_outer == 0) return ULTRA_OK;
    return launch_dense_layer0_adjacency(a_ex_dev, num_node, relation, src_rows_dev, src_values_dev, weight, bias, ln_weight, ln_bias,
                                         eps, flags, output, reinterpret_cast<hipStream_t>(stream));
}

int32_t ultra_rspmm_backward(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const void *edge_weight_dev,
                             const ultra_mat *relation, const ultra_mat *input, const ultra_mat *output,
                             const ultra_mat *output_grad, void *weight_grad_dev, const ultra_mat *relation_grad,
                             const ultra_mat *input_grad, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    WeightEpochScope weight_epoch_scope;
    return backward_impl(plan, sum, mul, dtype, edge_weight_dev, relation, input, output, output_grad, weight_grad_dev,
                         relation_grad, input_grad, reinterpret_cast<hipStream_t>(stream));
}

int32_t ultra_rspmm_backward_add(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const void *edge_weight_dev,
                                 const ultra_mat *relation, const ultra_mat *input, const ultra_mat *output,
                                 const ultra_mat *output_grad, void *weight_grad_dev, const ultra_mat *relation_grad,
                                 const ultra_mat *input_grad_base, const ultra_mat *input_grad, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    WeightEpochScope weight_epoch_scope;
    if (!input_grad_base) return invalid("ultra_rspmm_backward_add: input_grad_base is NULL");
    return backward_impl(plan, sum, mul, dtype, edge_weight_dev, relation, input, output, output_grad, weight_grad_dev,
                         relation_grad, input_grad, reinterpret_cast<hipStream_t>(stream), input_grad_base);
}

int32_t ultra_rspmm_edge_grad_samples(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype, const ultra_mat *relation,
                                      const ultra_mat *input, const ultra_mat *output_grad, void *weight_grad_dev,
                                      int64_t weight_grad_stride, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, weight_grad_dev);
    if (!plan) return invalid("ultra_rspmm_edge_grad_samples: plan is NULL");
    if (sum != ULTRA_SUM_ADD || (mul != ULTRA_MUL_MUL && mul != ULTRA_MUL_ADD) || dtype != ULTRA_F32) {
        set_error("ultra_rspmm_edge_grad_samples: served for the sum aggregate, mul / add messages and fp32 only (sum, mul, dtype)");
        return ULTRA_ERR_UNSUPPORTED;
    }
    (void)hipGetLastError();
    if (plan->flags & ULTRA_PLAN_DENSE) return invalid("ultra_rspmm_edge_grad_samples: a ULTRA_PLAN_DENSE plan has no edge list; use the (row, col) plan");
    if (!output_grad || !output_grad->ptr) return invalid("ultra_rspmm_edge_grad_samples: output_grad is NULL");
    const int64_t n_outer = output_grad->n_outer, row_len = output_grad->row_len;
    if (n_outer <= 0 || n_outer > 65535 || row_len <= 0 || row_len >= INT32_MAX)
        return invalid("ultra_rspmm_edge_grad_samples: output_grad: n_outer must be in [1, 65535] and row_len positive");
    int rc;
    if ((rc = check_mat(relation, "relation", plan->num_rel, n_outer, row_len))) return rc;
    if ((rc = check_mat(input, "input", plan->num_in, n_outer, row_len))) return rc;
    if ((rc = check_mat(output_grad, "output_grad", plan->num_out, n_outer, row_len))) return rc;
    if (plan->num_edge > 0 && !weight_grad_dev) return invalid("ultra_rspmm_edge_grad_samples: weight_grad is NULL");
    if (weight_grad_stride < plan->num_edge) return invalid("ultra_rspmm_edge_grad_samples: weight_grad_stride < num_edge");
    if (plan->num_edge <= 0) return ULTRA_OK;
    if ((rc = upload_plan(plan))) return rc;
    const bool vec4 = (row_len % 4 == 0) && mat_vec_ok(relation, 4) && mat_vec_ok(input, 4) && mat_vec_ok(output_grad, 4);
    EdgeSamplesParams ep;
    std::memset(&ep, 0, sizeof(ep));
    ep.erow = plan->d.erow;
    ep.col = plan->d.col;
    ep.type = plan->d.type;
    ep.perm = plan->d.perm;
    ep.num_edge = plan->num_edge;
    ep.rel = MatArg{relation->ptr, relation->stride_outer, relation->stride_row};
    ep.x = MatArg{input->ptr, input->stride_outer, input->stride_row};
    ep.og = MatArg{output_grad->ptr, output_grad->stride_outer, output_grad->stride_row};
    ep.wgrad = weight_grad_dev;
    ep.wgrad_so = weight_grad_stride;
    ep.row_len = (int32_t)row_len;
    return launch_edge_grad_samples(vec4 ? 4 : 1, mul == ULTRA_MUL_MUL ? BIN_MUL : BIN_ADD, (int)n_outer, ep,
                                    reinterpret_cast<hipStream_t>(stream));
}

int32_t ultra_rspmm_dense_relation_grad(ultra_plan *plan, const ultra_mat *input, const ultra_mat *output_grad,
                                        const ultra_mat *relation_grad, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, output_grad ? output_grad->ptr : nullptr);
    if (!plan) return invalid("plan is NULL");
    (void)hipGetLastError();
    if (!(plan->flags & ULTRA_PLAN_DENSE)) {
        set_error("ultra_rspmm_dense_relation_grad: served by ULTRA_PLAN_DENSE plans");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (!input || !input->ptr || !output_grad || !output_grad->ptr || !relation_grad || !relation_grad->ptr)
        return invalid("ultra_rspmm_dense_relation_grad: NULL operand");
    const int64_t n_outer = output_grad->n_outer, row_len = output_grad->row_len;
    if (n_outer <= 0 || row_len <= 0) return invalid("output_grad: empty n_outer / row_len");
    int rc;
    if ((rc = check_mat(input, "input", plan->num_in, n_outer, row_len))) return rc;
    if ((rc = check_mat(output_grad, "output_grad", plan->num_out, n_outer, row_len))) return rc;
    if ((rc = check_mat(relation_grad, "relation_grad", plan->num_rel, n_outer, row_len))) return rc;
    if ((rc = upload_plan(plan))) return rc;
    if ((rc = ensure_scratch(&plan->d.partial, &plan->d.partial_bytes,
                             (size_t)plan->dense_rt * plan->num_rel * n_outer * row_len * sizeof(float), plan)))
        return rc;
    return launch_dense_relation_grad(plan, input, output_grad, relation_grad, static_cast<float *>(plan->d.partial),
                                      reinterpret_cast<hipStream_t>(stream));
}

// rspmm on a list of output rows (rspmm_rows_kernels.hpp): shared argument checks of the forward and the backward entry
static int rows_params(ultra_plan *p, int mul, const void *w, const ultra_mat *rel, const ultra_mat *x, const int64_t *rows,
                       int64_t n_list, RowsParams *rp, const char *who) {
    if (!p) return invalid("plan is NULL");
    (void)hipGetLastError();
    if (p->flags & ULTRA_PLAN_DENSE) {
        set_error(std::string(who) + ": served by (row, col) plans");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if (mul < 0 || mul > 1) return invalid("unknown mul code");
    if (!rows || n_list <= 0 || !x || !x->ptr || !rel || !rel->ptr) return invalid(std::string(who) + ": NULL operand or empty row list");
    const int64_t n_outer = x->n_outer, row_len = x->row_len;
    int rc;
    if ((rc = check_mat(x, "input", p->num_in, n_outer, row_len))) return rc;
    if ((rc = check_mat(rel, "relation", p->num_rel, n_outer, row_len))) return rc;
    if (row_len % 64 != 0 || !mat_vec_ok(x, 4) || !mat_vec_ok(rel, 4) || n_outer * (row_len / 64) * n_list > (1ll << 31)) {
        set_error(std::string(who) + ": fp32 rows of whole 64-element spans, 16-byte aligned");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if ((rc = upload_plan(p))) return rc;
    std::memset(rp, 0, sizeof(*rp));
    rp->row_ptr = p->d.row_ptr, rp->col = p->d.col, rp->type = p->d.type, rp->perm = p->d.perm;
    rp->w = static_cast<const float *>(w);
    rp->rel = MatArg{rel->ptr, rel->stride_outer, rel->stride_row};
    rp->x = MatArg{x->ptr, x->stride_outer, x->stride_row};
    rp->rows = reinterpret_cast<const long long *>(rows);
    rp->n_outer = (int32_t)n_outer, rp->n_list = (int32_t)n_list, rp->row_len = (int32_t)row_len, rp->spans = (int32_t)(row_len / 64);
    rp->mul_add = mul == ULTRA_MUL_ADD ? 1 : 0;
    return ULTRA_OK;
}

int32_t ultra_rspmm_rows_forward(ultra_plan *plan, int32_t mul, const void *edge_weight_dev, const ultra_mat *relation,
                                 const ultra_mat *input, const int64_t *rows_dev, int64_t n_list, const ultra_mat *boundary,
                                 const int64_t *point_rows_dev, const void *point_values_dev, void *aggregate_dev, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, aggregate_dev);
    RowsParams rp;
    int rc;
    if ((rc = rows_params(plan, mul, edge_weight_dev, relation, input, rows_dev, n_list, &rp, "ultra_rspmm_rows_forward"))) return rc;
    if (!aggregate_dev) return invalid("ultra_rspmm_rows_forward: aggregate is NULL");
    if (boundary) {
        if ((rc = check_mat(boundary, "boundary", plan->num_out, rp.n_outer, rp.row_len))) return rc;
        if (!mat_vec_ok(boundary, 4)) return invalid("boundary: rows must be 16-byte aligned");
        rp.bnd = MatArg{boundary->ptr, boundary->stride_outer, boundary->stride_row};
    }
    if (point_rows_dev && !point_values_dev) return invalid("a point boundary needs its value rows");
    rp.point_rows = reinterpret_cast<const long long *>(point_rows_dev);
    rp.point_vals = static_cast<const float *>(point_values_dev);
    rp.agg = static_cast<float *>(aggregate_dev);
    const long long waves = (long long)rp.n_outer * rp.spans * rp.n_list;
    hipLaunchKernelGGL(rspmm_rows_kernel<false>, dim3((unsigned)waves), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), rp);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// The edge list grouped by `key` (counting sort, original order inside a group) and cut into segments of ROWS_BWD_SEG edges:
// rec = {aggregation row, other operand's row, original edge id, 0}; seg = {owner, first, end, partial row or -1}; multi = the
// owners that need a combine = {owner, first partial row, partial rows, 0}.  every_owner_partial: every owner goes through the
// partial rows (relation gradient: few owners, long lists), else owners with one segment are written by the gather itself.
static int build_rows_bwd_group(const std::vector<int32_t> &key, const std::vector<int32_t> &other, const std::vector<int32_t> &row,
                                int64_t n_owner, bool every_owner_partial, int64_t seg_len, void **d_rec, void **d_seg, void **d_multi,
                                int64_t *n_seg, int64_t *n_multi, int64_t *n_part) {
    const int64_t E = (int64_t)key.size();
    std::vector<int64_t> ptr(n_owner + 1, 0);
    for (int64_t e = 0; e < E; ++e) ptr[key[e] + 1]++;
    for (int64_t o = 0; o < n_owner; ++o) ptr[o + 1] += ptr[o];
    std::vector<int32_t> rec((size_t)std::max<int64_t>(E, 1) * 4, 0);
    {
        std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
        for (int64_t e = 0; e < E; ++e) {
            const int64_t k = fill[key[e]]++;
            rec[4 * k + 0] = row[e], rec[4 * k + 1] = other[e], rec[4 * k + 2] = (int32_t)e;
        }
    }
    std::vector<int32_t> seg, multi;
    int64_t parts = 0;
    for (int64_t o = 0; o < n_owner; ++o) {
        const int64_t beg = ptr[o], end = ptr[o + 1];
        int64_t pieces = (end - beg + seg_len - 1) / seg_len;
        if (pieces < 1 && !every_owner_partial) pieces = 1;      // (an owner without edges still writes its row)
        const bool through_partials = every_owner_partial || pieces > 1;
        if (through_partials) {
            multi.push_back((int32_t)o), multi.push_back((int32_t)parts), multi.push_back((int32_t)pieces), multi.push_back(0);
        }
        for (int64_t k = 0; k < pieces; ++k) {
            seg.push_back((int32_t)o);
            seg.push_back((int32_t)(beg + k * seg_len));
            seg.push_back((int32_t)std::min<int64_t>(end, beg + (k + 1) * seg_len));
            seg.push_back(through_partials ? (int32_t)parts++ : -1);
        }
    }
    *n_seg = (int64_t)seg.size() / 4, *n_multi = (int64_t)multi.size() / 4, *n_part = parts;
    if (seg.empty()) seg.assign(4, 0);
    if (multi.empty()) multi.assign(4, 0);
    int rc;
    if ((rc = upload_array(reinterpret_cast<int32_t **>(d_rec), rec))) return rc;
    if ((rc = upload_array(reinterpret_cast<int32_t **>(d_seg), seg))) return rc;
    return upload_array(reinterpret_cast<int32_t **>(d_multi), multi);
}

static int ensure_rows_bwd_index(ultra_plan *p) {
    if (p->rb_built) return ULTRA_OK;
    if ((int64_t)p->h_row.size() != p->num_edge) return invalid("plan was built without its edge list; backward unavailable");
    int rc;
    if ((rc = build_rows_bwd_group(p->h_col, p->h_type, p->h_row, p->num_in, false, ROWS_BWD_SEG, &p->d.rb_rec_c, &p->d.rb_seg_c, &p->d.rb_multi_c,
                                   &p->rb_n_seg_c, &p->rb_n_multi_c, &p->rb_n_part_c)))
        return rc;
    if ((rc = build_rows_bwd_group(p->h_type, p->h_col, p->h_row, p->num_rel, true, ROWS_BWD_SEG_TYPE, &p->d.rb_rec_t, &p->d.rb_seg_t, &p->d.rb_multi_t,
                                   &p->rb_n_seg_t, &p->rb_n_multi_t, &p->rb_n_part_t)))
        return rc;
    p->rb_built = true;
    return ULTRA_OK;
}

int32_t ultra_rspmm_rows_backward_gather(ultra_plan *plan, int32_t mul, const void *edge_weight_dev, const ultra_mat *relation,
                                         const ultra_mat *input, const int64_t *rows_dev, int64_t n_list,
                                         const void *aggregate_grad_dev, const void *update_grad_dev, const int64_t *point_rows_dev,
                                         void *point_values_grad_dev, const ultra_mat *relation_grad, const ultra_mat *input_grad,
                                         void *stream) {
    ULTRA_DEVICE_SCOPE(stream, aggregate_grad_dev);
    RowsParams rp;
    int rc;
    if ((rc = rows_params(plan, mul, edge_weight_dev, relation, input, rows_dev, n_list, &rp, "ultra_rspmm_rows_backward_gather"))) return rc;
    if (!aggregate_grad_dev || !relation_grad || !input_grad || !relation_grad->ptr || !input_grad->ptr)
        return invalid("ultra_rspmm_rows_backward_gather: NULL gradient operand");
    if (point_values_grad_dev && !point_rows_dev) return invalid("point_values_grad needs point_rows");
    if ((rc = check_mat(relation_grad, "relation_grad", plan->num_rel, rp.n_outer, rp.row_len))) return rc;
    if ((rc = check_mat(input_grad, "input_grad", plan->num_in, rp.n_outer, rp.row_len))) return rc;
    if (rp.row_len != 64 || n_list > ROWS_BWD_MAX_LIST || plan->num_out != plan->num_in || !mat_vec_ok(relation_grad, 4) ||
        !mat_vec_ok(input_grad, 4)) {
        set_error("ultra_rspmm_rows_backward_gather: 64-element rows, at most 1024 listed rows per sample, square graphs; otherwise "
                  "ultra_rspmm_rows_backward");
        return ULTRA_ERR_UNSUPPORTED;
    }
    if ((rc = ensure_rows_bwd_index(plan))) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t n_outer = rp.n_outer, n_chunk = (n_outer + 7) / 8, N = plan->num_out;
    // workspace: slot table | combined aggregate gradient | combined update share | partial rows (input grad) | partial rows (relation grad)
    const size_t slot_bytes = (size_t)n_chunk * N * 16;
    const size_t g_bytes = (size_t)n_outer * n_list * 64 * sizeof(float);
    const size_t px_bytes = (size_t)std::max<int64_t>(plan->rb_n_part_c, 1) * 8 * 64 * sizeof(float);
    const size_t pr_bytes = (size_t)std::max<int64_t>(plan->rb_n_part_t, 1) * 8 * 64 * sizeof(float);
    if ((rc = ensure_scratch(&plan->d.rb_work, &plan->d.rb_work_bytes, slot_bytes + 2 * g_bytes + px_bytes + pr_bytes, plan))) return rc;
    char *work = static_cast<char *>(plan->d.rb_work);
    uint16_t *slot = reinterpret_cast<uint16_t *>(work);
    float *gc = reinterpret_cast<float *>(work + slot_bytes), *uc = reinterpret_cast<float *>(work + slot_bytes + g_bytes);
    float *px = reinterpret_cast<float *>(work + slot_bytes + 2 * g_bytes);
    float *pr = reinterpret_cast<float *>(work + slot_bytes + 2 * g_bytes + px_bytes);
    {
        const long long n16 = (long long)(slot_bytes / 16);
        hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)std::min<long long>((n16 + 255) / 256, 2048)), dim3(256), 0, s,
                           reinterpret_cast<uint4 *>(slot), n16);
        RowsPrepParams pp;
        pp.rows = rp.rows;
        pp.agg_grad = static_cast<const float *>(aggregate_grad_dev);
        pp.upd_grad = static_cast<const float *>(update_grad_dev);
        pp.point_rows = reinterpret_cast<const long long *>(point_rows_dev);
        pp.slot = slot, pp.gc = gc, pp.uc = uc;
        pp.values_grad = static_cast<float *>(point_values_grad_dev);
        pp.num_row = N, pp.n_list = (int)n_list;
        hipLaunchKernelGGL(rows_prepare_kernel, dim3((unsigned)n_outer), dim3(1024), 0, s, pp);
    }
    for (int64_t chunk = 0; chunk < n_chunk; ++chunk) {
        RowsGatherParams gp;
        std::memset(&gp, 0, sizeof(gp));
        gp.slot = slot + (size_t)chunk * N * 8;
        gp.keep = rp.w;
        gp.gc = gc;
        gp.n_list = (int)n_list, gp.o0 = (int)(chunk * 8), gp.nb = (int)std::min<int64_t>(8, n_outer - chunk * 8);
        gp.mul_add = rp.mul_add;
        // ---- input gradient: owners = sources ----
        gp.rec = static_cast<const int4 *>(plan->d.rb_rec_c), gp.seg = static_cast<const int4 *>(plan->d.rb_seg_c);
        gp.n_seg = (int)plan->rb_n_seg_c;
        gp.uc = update_grad_dev ? uc : nullptr;
        gp.other = rp.rel;
        gp.out = static_cast<float *>(input_grad->ptr), gp.out_so = input_grad->stride_outer, gp.out_sr = input_grad->stride_row;
        gp.partial = px;
        if (gp.n_seg > 0)
            hipLaunchKernelGGL(rows_bwd_gather_kernel<true>, dim3((unsigned)((gp.n_seg + 15) / 16)), dim3(256), 0, s, gp);
        RowsCombineParams cp;
        std::memset(&cp, 0, sizeof(cp));
        cp.slot = gp.slot, cp.n_list = gp.n_list, cp.o0 = gp.o0, cp.nb = gp.nb;
        if (plan->rb_n_multi_c > 0) {
            cp.multi = static_cast<const int4 *>(plan->d.rb_multi_c), cp.n_multi = (int)plan->rb_n_multi_c;
            cp.partial = px, cp.uc = gp.uc;
            cp.out = gp.out, cp.out_so = gp.out_so, cp.out_sr = gp.out_sr;
            hipLaunchKernelGGL(rows_bwd_combine_kernel, dim3((unsigned)cp.n_multi), dim3(1024), 0, s, cp);
        }
        // ---- relation gradient: owners = types ----
        gp.rec = static_cast<const int4 *>(plan->d.rb_rec_t), gp.seg = static_cast<const int4 *>(plan->d.rb_seg_t);
        gp.n_seg = (int)plan->rb_n_seg_t;
        gp.uc = nullptr;
        gp.other = rp.x;
        gp.out = static_cast<float *>(relation_grad->ptr), gp.out_so = relation_grad->stride_outer, gp.out_sr = relation_grad->stride_row;
        gp.partial = pr;
        if (gp.n_seg > 0)
            hipLaunchKernelGGL(rows_bwd_gather_kernel<false>, dim3((unsigned)((gp.n_seg + 15) / 16)), dim3(256), 0, s, gp);
        if (plan->rb_n_multi_t > 0) {
            cp.multi = static_cast<const int4 *>(plan->d.rb_multi_t), cp.n_multi = (int)plan->rb_n_multi_t;
            cp.partial = pr, cp.uc = nullptr;
            cp.out = gp.out, cp.out_so = gp.out_so, cp.out_sr = gp.out_sr;
            hipLaunchKernelGGL(rows_bwd_combine_kernel, dim3((unsigned)cp.n_multi), dim3(1024), 0, s, cp);
        }
    }
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

int32_t ultra_rspmm_rows_backward(ultra_plan *plan, int32_t mul, const void *edge_weight_dev, const ultra_mat *relation,
                                  const ultra_mat *input, const int64_t *rows_dev, int64_t n_list, const void *aggregate_grad_dev,
                                  const ultra_mat *relation_grad, const ultra_mat *input_grad, void *stream) {
    ULTRA_DEVICE_SCOPE(stream, aggregate_grad_dev);
    RowsParams rp;
    int rc;
    if ((rc = rows_params(plan, mul, edge_weight_dev, relation, input, rows_dev, n_list, &rp, "ultra_rspmm_rows_backward"))) return rc;
    if (!aggregate_grad_dev) return invalid("ultra_rspmm_rows_backward: aggregate_grad is NULL");
    if ((rc = check_mat(relation_grad, "relation_grad", plan->num_rel, rp.n_outer, rp.row_len))) return rc;
    if ((rc = check_mat(input_grad, "input_grad", plan->num_in, rp.n_outer, rp.row_len))) return rc;
    rp.agg = const_cast<float *>(static_cast<const float *>(aggregate_grad_dev));
    rp.xgrad = static_cast<float *>(input_grad->ptr), rp.xgrad_so = input_grad->stride_outer, rp.xgrad_sr = input_grad->stride_row;
    rp.rgrad = static_cast<float *>(relation_grad->ptr), rp.rgrad_so = relation_grad->stride_outer, rp.rgrad_sr = relation_grad->stride_row;
    const long long waves = (long long)rp.n_outer * rp.spans * rp.n_list;
    hipLaunchKernelGGL(rspmm_rows_kernel<true>, dim3((unsigned)waves), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), rp);
    HIP_TRY(hipGetLastError());
    return ULTRA_OK;
}

// Times `once` (a launch sequence on stream s) with HIP events: the mean of `iters` back-to-back calls, and -- the figure
// comparable with rocprofv3's per-kernel average -- the main kernel alone: `once` hands the pair of events it is given to
// forward_impl, which records them right around that launch.
static int time_launches(const std::function<int(hipEvent_t, hipEvent_t)> &once, hipStream_t s, int32_t warmup, int32_t iters, float *ms_per_call, float *ms_main_kernel,
                         const char *who) {
    if (!ms_per_call || iters <= 0) return invalid(std::string(who) + ": bad iters / ms_per_call");
    int rc;
    for (int i = 0; i < warmup; ++i)
        if ((rc = once(nullptr, nullptr)))
            return rc;
    struct Events {   // (destroyed on every path out)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    // (1) the whole launch sequence (weight permute + main kernel + fix-up), back to back
    HIP_TRY(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        if ((rc = once(nullptr, nullptr)))
            return rc;
    HIP_TRY(hipEventRecord(e1, s));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_call = ms / (float)iters;
    // (2) the main kernel alone: events recorded right around its launch, one iteration at a time
    if (ms_main_kernel) {
        double acc = 0.0;
        for (int i = 0; i < iters; ++i) {
            if ((rc = once(e0, e1))) return rc;
            HIP_TRY(hipEventSynchronize(e1));
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            acc += ms;
        }
        *ms_main_kernel = (float)(acc / iters);
    }
    return ULTRA_OK;
}

int32_t ultra_rspmm_forward_timed(ultra_plan *plan, int32_t sum, int32_t mul, int32_t dtype,
                                  const void *edge_weight_dev, const ultra_mat *relation, const ultra_mat *input,
                                  const ultra_mat *boundary, const int64_t *point_rows_dev, const ultra_mat *output,
                                  void *stream, int32_t warmup, int32_t iters, float *ms_per_call, float *ms_main_kernel) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);
    if (int rc = internal_mul(&mul)) return rc;
    FwdCall call{point_rows_dev};
    const auto once = [&](hipEvent_t before, hipEvent_t after) {
        call.ev_before = before, call.ev_after = after;
        return forward_impl(plan, sum, mul, dtype, edge_weight_dev, relation, input, boundary, output,
                            reinterpret_cast<hipStream_t>(stream), call);
    };
    return time_launches(once, reinterpret_cast<hipStream_t>(stream), warmup, iters, ms_per_call, ms_main_kernel,
                         "ultra_rspmm_forward_timed");
}

int32_t ultra_rspmm_forward_update_timed(ultra_plan *plan, int32_t sum, int32_t mul, const ultra_mat *relation, const ultra_mat *input,
                                         const int64_t *point_rows_dev, const ultra_mat *point_values, const ultra_mat *aggregate,
                                         const void *weight, const void *bias, const void *ln_weight, const void *ln_bias, float eps,
                                         int32_t flags, const ultra_mat *output, void *stream, int32_t warmup, int32_t iters,
                                         float *ms_per_call, float *ms_main_kernel) {
    ULTRA_DEVICE_SCOPE(stream, output ? output->ptr : nullptr);   // (the events are created and recorded on the operands' device)
    FwdCall call{point_rows_dev};
    const auto once = [&](hipEvent_t before, hipEvent_t after) {
        call.ev_before = before, call.ev_after = after;
        return forward_update(plan, sum, mul, relation, input, point_values, aggregate, weight, bias, ln_weight, ln_bias, eps, flags,
                              output, reinterpret_cast<hipStream_t>(stream), call);
    };
    return time_launches(once, reinterpret_cast<hipStream_t>(stream), warmup, iters, ms_per_call, ms_main_kernel,
                         "ultra_rspmm_forward_update_timed");
}

int32_t ultra_order_trace(void *trace_dev) {
    g_order_trace = static_cast<long long *>(trace_dev);
    return ULTRA_OK;
}

int32_t ultra_plan_schedule_info(ultra_plan *plan, int32_t nparts, ultra_schedule_info *info) {
    const int32_t walkers = (nparts & ULTRA_SCHEDULE_12_WALKERS) ? 12 : 16;
    nparts &= ~ULTRA_SCHEDULE_12_WALKERS;
    if (!plan || !info || nparts <= 0) return invalid("ultra_plan_schedule_info: bad argument");
    if (!(plan->flags & ULTRA_PLAN_EXACT_ORDER)) return invalid("schedules belong to ULTRA_PLAN_EXACT_ORDER plans");
    Schedule *s = build_schedule(plan, nparts, walkers);
    info->nparts = nparts;
    info->n_chunk = (int64_t)s->chunk_ptr.back();   // (the array carries CHUNK_PAD readable entries behind the last chunk)
    info->n_unit = (int64_t)s->units.size();
    info->max_cost = s->max_cost;
    info->mean_cost = s->mean_cost;
    int64_t mc = 0, mu = 0;
    for (int32_t q = 0; q < nparts; ++q) {
        mc = std::max<int64_t>(mc, s->chunk_ptr[(size_t)q + 1] - s->chunk_ptr[(size_t)q]);
        mu = std::max<int64_t>(mu, s->unit_ptr[(size_t)q + 1] - s->unit_ptr[(size_t)q]);
    }
    info->max_chunk_per_part = mc;
    info->max_unit_per_part = mu;
    delete s;
    return ULTRA_OK;
}

int32_t ultra_plan_schedule_export(ultra_plan *plan, int32_t nparts, int32_t which, int32_t *dst, int64_t capacity, int64_t *count) {
    const int32_t walkers = (nparts & ULTRA_SCHEDULE_12_WALKERS) ? 12 : 16;
    nparts &= ~ULTRA_SCHEDULE_12_WALKERS;
    if (!plan || !count || nparts <= 0) return invalid("ultra_plan_schedule_export: bad argument");
    if (!(plan->flags & ULTRA_PLAN_EXACT_ORDER)) return invalid("schedules belong to ULTRA_PLAN_EXACT_ORDER plans");
    Schedule *s = build_schedule(plan, nparts, walkers);
    const int32_t *src = nullptr;
    int64_t n = 0;
    switch (which) {
        case 0: src = s->chunk_ptr.data(), n = (int64_t)s->chunk_ptr.size(); break;
        case 1: src = s->unit_ptr.data(), n = (int64_t)s->unit_ptr.size(); break;
        case 2: src = s->units.data(), n = (int64_t)s->units.size(); break;
        case 3: src = reinterpret_cast<const int32_t *>(s->chunks.data()), n = (int64_t)s->chunk_ptr.back() * 4; break;
        case 4: src = s->sdesc.data(), n = (int64_t)s->sdesc.size(); break;
        case 5: src = s->srec.data(), n = (int64_t)s->srec.size() - s->srec_pad; break;
        case 6: src = s->prow.data(), n = (int64_t)s->prow.size(); break;
        case 7: src = s->prow_ptr.data(), n = (int64_t)s->prow_ptr.size(); break;
        default: delete s; return invalid("ultra_plan_schedule_export: unknown array id");
    }
    *count = n;
    int rc = ULTRA_OK;
    if (dst) {
        if (capacity < n) rc = invalid("ultra_plan_schedule_export: destination too small");
        else if (n) std::memcpy(dst, src, (size_t)n * sizeof(int32_t));
        // (the export shows LOGICAL records -- (col, type), markers (row, num_relation) -- whatever the device format of this
        // schedule's streams is: plan.hpp ULTRA_STREAM_PRESHIFT)
        if (rc == ULTRA_OK && which == 5 && s->rec_shift)
            for (int64_t i = 0; i < n; ++i) dst[i] = (int32_t)((uint32_t)dst[i] >> s->rec_shift);
    }
    delete s;
    return rc;
}

int32_t ultra_device_error(void) { return take_device_error(); }

int32_t ultra_set_tuning(const ultra_tuning *t) {
    if (!t) {
        g_tuning = ultra_tuning{0, 0, -1, -1, 0, {0, 0, 0}};
        return ULTRA_OK;
    }
    if (t->threads < 0 || t->threads > 1024 || (t->threads % 64) != 0) return invalid("threads must be a multiple of 64 <= 1024");
    g_tuning = *t;
    return ULTRA_OK;
}

int32_t ultra_get_tuning(ultra_tuning *t) {
    if (!t) return invalid("NULL");
    *t = g_tuning;
    return ULTRA_OK;
}

#define ULTRA_DEFINE_REFERENCE_ENTRY(SUM, MUL, SUMC, MULC)                                                           \
    int32_t ultra_rspmm_##SUM##_##MUL##_forward_cuda(                                                                \
        const int64_t *edge_index_dev, const int64_t *edge_type_dev, const void *edge_weight_dev,                    \
        const void *relation_dev, const void *input_dev, void *output_dev, int64_t num_edge, int64_t num_node,       \
        int64_t num_relation, int64_t dim, int32_t dtype, void *stream) {                                            \
        ULTRA_DEVICE_SCOPE(stream, edge_index_dev);                                                                                  \
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);                                                       \
        ultra_plan *plan = nullptr;                                                                                  \
        int rc = stateless_plan(&plan, edge_index_dev, edge_type_dev, num_edge, num_node, num_relation, s);         \
        if (rc) return rc;                                                                                           \
        ultra_mat rel = dense2d(relation_dev, num_relation, dim), in = dense2d(input_dev, num_node, dim),            \
                  out = dense2d(output_dev, num_node, dim);                                                          \
        rc = ultra_rspmm_forward(plan, SUMC, MULC, dtype, edge_weight_dev, &rel, &in, nullptr, &out, stream);        \
        if (rc == ULTRA_OK && hipStreamSynchronize(s) != hipSuccess) rc = ULTRA_ERR_HIP;                             \
        ultra_plan_destroy(plan);                                                                                    \
        return rc;                                                                                                   \
    }                                                                                                                \
    int32_t ultra_rspmm_##SUM##_##MUL##_backward_cuda(                                                               \
        const int64_t *edge_index_dev, const int64_t *edge_type_dev, const void *edge_weight_dev,                    \
        const void *relation_dev, const void *input_dev, const void *output_dev, const void *output_grad_dev,        \
        void *weight_grad_dev, void *relation_grad_dev, void *input_grad_dev, int64_t num_edge, int64_t num_node,    \
        int64_t num_relation, int64_t dim, int32_t dtype, void *stream) {                                            \
        ULTRA_DEVICE_SCOPE(stream, edge_index_dev);                                                                                  \
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);                                                       \
        ultra_plan *plan = nullptr;                                                                                  \
        int rc = stateless_plan(&plan, edge_index_dev, edge_type_dev, num_edge, num_node, num_relation, s);         \
        if (rc) return rc;                                                                                           \
        ultra_mat rel = dense2d(relation_dev, num_relation, dim), in = dense2d(input_dev, num_node, dim),            \
                  out = dense2d(output_dev, num_node, dim), og = dense2d(output_grad_dev, num_node, dim),            \
                  rg = dense2d(relation_grad_dev, num_relation, dim), xg = dense2d(input_grad_dev, num_node, dim);   \
        rc = ultra_rspmm_backward(plan, SUMC, MULC, dtype, edge_weight_dev, &rel, &in, &out, &og, weight_grad_dev,   \
                                  &rg, &xg, stream);                                                                 \
        if (rc == ULTRA_OK && hipStreamSynchronize(s) != hipSuccess) rc = ULTRA_ERR_HIP;                             \
        ultra_plan_destroy(plan);                                                                                    \
        return rc;                                                                                                   \
    }

ULTRA_DEFINE_REFERENCE_ENTRY(add, mul, ULTRA_SUM_ADD, ULTRA_MUL_MUL)
ULTRA_DEFINE_REFERENCE_ENTRY(min, mul, ULTRA_SUM_MIN, ULTRA_MUL_MUL)
ULTRA_DEFINE_REFERENCE_ENTRY(max, mul, ULTRA_SUM_MAX, ULTRA_MUL_MUL)
ULTRA_DEFINE_REFERENCE_ENTRY(add, add, ULTRA_SUM_ADD, ULTRA_MUL_ADD)
ULTRA_DEFINE_REFERENCE_ENTRY(min, add, ULTRA_SUM_MIN, ULTRA_MUL_ADD)
ULTRA_DEFINE_REFERENCE_ENTRY(max, add, ULTRA_SUM_MAX, ULTRA_MUL_ADD)

}  // extern "C"
