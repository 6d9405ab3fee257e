// cavoid_policy_host.hpp -- the handle behind `cavoid_policy *` (include/cavoid.h), shared by the translation units that launch on it:
// cavoid_policy_capi.hip (inference / trainer pass), cavoid_policy_ws.hip (the weight-sharing network's) and cavoid_actor.hip (the fused
// actor kernel) -- and the handle, argument and buffer plumbing the first two have in common.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "cavoid_host.hpp"
#include "cavoid_policy.hpp"
#include "cavoid_policy_split.hpp"

using cavoid::f32x4;

struct cavoid_policy {
    int device = 0;
    int max_other = 0, num_actions = 0, in_size = 0;
    bool loaded = false, normalize = false, backward_loaded = false;
    float min_policy = 0.0f;
    uint64_t seed = 0;
    void *slab = nullptr;
    f32x4 *frags = nullptr;
    uint4 *sfrags = nullptr;         // split weight fragments of the inference kernel (cavoid_policy_split.hpp)
    float *sbias = nullptr;          // ... and its biases (packed order; the LSTM gates pre-scaled by log2 e / 2 log2 e like their weight columns)
    int split_products = cavoid::kSpDefaultProducts;   // 16 (default): float16 pieces, three products; 3 / 4 / 5: bf16 pieces (CAVOID_POLICY_PRODUCTS)
    int form = -1;                   // CAVOID_POLICY_FORM = quad (0) / oct (1) / duo (2) / unset (-1: duo from two tiles per CU on, else quad): the stand-alone inference
                                     // launch's tile-to-wavefront mapping (same results in every form)
    int num_cus = 256;
    bool crowd = false;              // max_other > kPolMaxOthers: inference on policy_crowd_forward_kernel only (cavoid_policy_crowd.hpp); with ws: the ring kernels of cavoid_policy_wsring.hpp
    bool ws = false;                 // MULTI_AGENT_ARCH 'weight_sharing' (cavoid_policy_create_ws): frags / bias hold the pack of cavoid_policy_ws.hpp
    bool use_split = true;           // CAVOID_POLICY_F32=1: run inference on the float32-MFMA kernel instead (A/B runs)
    float *bias = nullptr, *avg = nullptr, *std = nullptr;
    int32_t *step_counter = nullptr;
    uint32_t *clamped_weights = nullptr;   // device counter: weights the float16 split saturated at the last cavoid_policy_load
    uint32_t *blocks_done = nullptr, *cu_tickets = nullptr;
    float *clip_scale = nullptr;     // [16] per-variable gradient scales of cavoid_policy_apply's clip (cavoid_policy_step.hip)
    uint32_t *apply_ticket = nullptr; // ... and its workgroup ticket: the last workgroup of the update launch writes the step count
    int row_tiles = 4;               // 16-row tiles per workgroup (64 rows, 2 workgroups per CU); the 32-row / 4-per-CU
                                     // instantiation was measured and dropped: 175 vs 132 us
};

// the inference launch of a weight-sharing handle (cavoid_policy_ws.hip): cavoid_policy_forward / _rows route there
int cavoid_policy_ws_launch(cavoid_policy *h, const cavoid::PolicyArgs &a, int64_t blocks, hipStream_t stream);
// the trainer's forward pass of a crowd handle (cavoid_policy_train_ring.hip): cavoid_policy_train / _train_regression route there, then launch
// policy_backward_kernel themselves.  _opt_in: the two ring kernels' dynamic LDS, at creation (on failure the handle is gone)
int cavoid_policy_train_ring_opt_in(cavoid_policy *h);
int cavoid_policy_train_ring_launch(cavoid_policy *h, const cavoid::PolicyArgs &a, unsigned blocks, int loss_kind, hipStream_t stream);

// a cavoid_policy_create_ws_crowd handle (ws and crowd both set; cavoid_policy_wsring.hip): cavoid_policy_ws_launch and the trainer pass of
// cavoid_policy_ws.hip route their forward launch there, then launch policy_ws_backward_kernel themselves.  _backward_opt_in
// (cavoid_policy_ws.hip): that kernel's dynamic LDS, at creation (on failure the handle is gone)
int cavoid_policy_wsring_launch(cavoid_policy *h, const cavoid::PolicyArgs &a, int64_t blocks, hipStream_t stream);
int cavoid_policy_wsring_train_launch(cavoid_policy *h, const cavoid::PolicyArgs &a, float *f_in, unsigned blocks, int loss_kind, hipStream_t stream);
int cavoid_policy_ws_backward_opt_in(cavoid_policy *h);

// ---- creation -------------------------------------------------------------------------------------------------------------------
// The handle of cavoid_policy_create / _create_ws, once the caller has checked the argument ranges: the device check, then one zeroed
// slab carved into the handle's device arrays -- f32_frags float32 weight fragments and, with_split, the inference kernel's split copy.
inline int policy_new_handle(int32_t max_other, int32_t num_actions, int device, int64_t f32_frags, bool with_split, cavoid_policy **out) {
    using namespace cavoid;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CAVOID_ENODEVICE;
    HIP_TRY(hipSetDevice(device));
    cavoid_policy *h = new (std::nothrow) cavoid_policy();
    if (!h) return CAVOID_ENOMEM;
    h->device = device; h->max_other = max_other; h->num_actions = num_actions;
    h->in_size = 1 + kPolHost + kPolOther * max_other;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_frag = carve((size_t)f32_frags * sizeof(f32x4)), o_bias = carve(kBiasFloats * sizeof(float));
    const size_t o_sfrag = carve(with_split ? (size_t)kSpPackFrags8 * sizeof(uint4) : 0), o_sbias = carve(with_split ? kBiasFloats8 * sizeof(float) : 0);
    const size_t o_avg = carve(h->in_size * sizeof(float)), o_std = carve(h->in_size * sizeof(float));
    const size_t o_step = carve(sizeof(int32_t)), o_done = carve(sizeof(uint32_t)), o_tick = carve(kPolCuSlots * sizeof(uint32_t));
    const size_t o_clamp = carve(sizeof(uint32_t)), o_clip = carve(16 * sizeof(float)), o_ticket = carve(sizeof(uint32_t));
    if (hipMalloc(&h->slab, off) != hipSuccess) { delete h; return CAVOID_ENOMEM; }
    if (hipMemset(h->slab, 0, off) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); (void)hipFree(h->slab); delete h; return CAVOID_EHIP; }
    unsigned char *b = static_cast<unsigned char *>(h->slab);
    h->frags = reinterpret_cast<f32x4 *>(b + o_frag); h->bias = reinterpret_cast<float *>(b + o_bias);
    if (with_split) { h->sfrags = reinterpret_cast<uint4 *>(b + o_sfrag); h->sbias = reinterpret_cast<float *>(b + o_sbias); }
    h->avg = reinterpret_cast<float *>(b + o_avg); h->std = reinterpret_cast<float *>(b + o_std);
    h->step_counter = reinterpret_cast<int32_t *>(b + o_step); h->blocks_done = reinterpret_cast<uint32_t *>(b + o_done);
    h->cu_tickets = reinterpret_cast<uint32_t *>(b + o_tick);
    h->clamped_weights = reinterpret_cast<uint32_t *>(b + o_clamp);
    h->clip_scale = reinterpret_cast<float *>(b + o_clip);
    h->apply_ticket = reinterpret_cast<uint32_t *>(b + o_ticket);
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->num_cus <= 0) h->num_cus = 256;
    *out = h;
    return CAVOID_OK;
}

// A 64-row workgroup's LDS (70 KB) is above the 64 KB static limit: it is dynamic, and every kernel that takes it is opted in at
// creation.  On failure the handle is gone.
struct PolicyLdsOptIn { const void *kernel; size_t bytes; };
template <size_t N>
inline int policy_opt_in_lds(cavoid_policy *h, const PolicyLdsOptIn (&kernels)[N]) {
    for (const PolicyLdsOptIn &k : kernels)
        if (hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes) != hipSuccess) {
            g_last_hip_error = (int)hipGetLastError(); (void)hipFree(h->slab); delete h; return CAVOID_EHIP;
        }
    return CAVOID_OK;
}

// ---- load -----------------------------------------------------------------------------------------------------------------------
// what follows the pack launches of cavoid_policy_load / _load_ws
inline int policy_finish_load(cavoid_policy *h, const cavoid_policy_weights *w, hipStream_t s) {
    h->backward_loaded = w->with_backward != 0;
    h->normalize = w->avg != nullptr;
    if (h->normalize) {
        HIP_TRY(hipMemcpyAsync(h->avg, w->avg, h->in_size * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->std, w->std, h->in_size * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    h->min_policy = w->min_policy;
    h->loaded = true;
    return CAVOID_OK;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
// the PolicyArgs fields every pass fills from the handle and its input rows
inline cavoid::PolicyArgs policy_common_args(const cavoid_policy *h, const float *x, int64_t rows, int64_t row_stride) {
    cavoid::PolicyArgs a{};
    a.x = x; a.rows = rows; a.stride = row_stride; a.max_other = h->max_other; a.num_actions = h->num_actions; a.in_size = h->in_size;
    a.avg = h->normalize ? h->avg : nullptr; a.std = h->normalize ? h->std : nullptr;
    a.frags = h->frags; a.bias = h->bias; a.min_policy = h->min_policy; a.cu_tickets = h->cu_tickets;
    return a;
}

// The trainer pass up to its launches, on the fields cavoid_policy_train_buffers and cavoid_policy_train_ws_buffers share (the caller
// has checked the handle, the inputs and its own buffers): validates, zeroes loss and db, and fills the TRAIN forward's arguments.
// *blocks = the launch size of both kernels, 0 when rows == 0 (nothing to launch).  Every tile of the buffers is processed (tiles past
// `rows` carry zero gradients), so that the caller can run its weight-gradient GEMMs over all capacity_rows without reading stale rows.
template <class Buffers>
inline int policy_train_begin(cavoid_policy *h, const float *x, int64_t rows, int64_t row_stride, const float *y_r, const int32_t *a_idx, float beta,
                              float log_epsilon, const Buffers *b, hipStream_t s, cavoid::PolicyArgs *a, unsigned *blocks) {
    const int64_t rows64 = (rows + 63) / 64 * 64;
    if (b->capacity_rows < rows64 || b->capacity_rows % 64 != 0 || b->capacity_rows / 64 > 0x7fffffffLL || !b->z1 || !b->z2 || !b->z3 ||
        !b->l1_in || !b->gh || !b->loss || !b->g1 || !b->g2 || !b->g3 || !b->db)
        return CAVOID_EINVAL;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(b->loss, 0, 2 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(b->db, 0, cavoid::kBiasFloats * sizeof(float), s));
    *blocks = rows == 0 ? 0u : (unsigned)(b->capacity_rows / 64);
    *a = policy_common_args(h, x, rows, row_stride);
    a->y_r = y_r; a->a_idx = a_idx; a->beta = beta; a->log_eps = log_epsilon;
    a->rows64 = b->capacity_rows;                          // leading dimension (in rows) of the per-step buffers
    a->z1 = b->z1; a->z2 = b->z2; a->z3 = b->z3; a->l1_in = b->l1_in; a->gh = b->gh; a->loss = b->loss; a->db = b->db;
    return CAVOID_OK;
}
