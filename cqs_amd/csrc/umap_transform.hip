// umap_transform.hip — new rows placed into an existing UMAP layout (include/cqs_hip.h "UMAP transform of new rows",
// DESIGN.md §3.18a): transform_kernel, the whole transform of a block of new vertices in ONE launch, and its three entry
// points - over caller-held anchors, over a layout handle's resident coordinates, and over an index (search, then place).
// The anchors do not move, so no new vertex depends on another: weights, initial position and every epoch of a vertex are
// the private loop of one wave.  The argument plan and the scalar rules are umap_transform_host.h's / umap_host.h's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "abi_guard.h"
#include "index_internal.h"
#include "roctx.h"
#include "umap_internal.h"
#include "umap_transform_host.h"
#include "wave_ops.h"

namespace cqs_umap {

constexpr uint32_t kTransformWaves = 4;   // waves (= new vertices) per workgroup
constexpr uint32_t kDrawBatch = 8;        // draws whose gathers are issued together

struct TransformParams {
    uint64_t n, m;
    const float2* anchors;      // [n]
    const uint32_t* rows;       // [m, stride] anchor ids
    const float* scores;        // [m, stride]
    const uint32_t* counts;     // [m]
    float2* out_xy;             // [m]
    float* out_sigma;           // [m], nullable
    float* out_weights;         // [m, stride], nullable
    uint32_t stride, negative_samples, n_epochs, epochs;   // epochs <= n_epochs: how many to run
    uint32_t id_base;           // vertex v of the call hashes as id_base + v
    float a, b, learning_rate, repulsion;
    uint64_t seed;
};

// One slot's share of an epoch: the attraction to its anchor (in registers), then its draws' repulsions in draw order.
// The draws' gathers go out kDrawBatch at a time before the first of them is used.
__device__ __forceinline__ void slot_terms(const TransformParams& p, uint32_t hv, uint32_t slot, float2 y, float2 yj, float& sx,
                                           float& sy) {
#pragma clang fp contract(off)
    {
        const float dx = y.x - yj.x, dy = y.y - yj.y;
        const float d2 = dx * dx + dy * dy;
        if (d2 > 0.f) {
            const float ca = attract_coeff(p.a, p.b, d2);
            sx += clip4(ca * dx);
            sy += clip4(ca * dy);
        }
    }
    for (uint32_t k0 = 0; k0 < p.negative_samples; k0 += kDrawBatch) {
        float2 yq[kDrawBatch];
#pragma unroll
        for (uint32_t j = 0; j < kDrawBatch; ++j)
            if (k0 + j < p.negative_samples) yq[j] = p.anchors[draw_vertex(hash_draw(hv, slot, k0 + j), p.n)];
#pragma unroll
        for (uint32_t j = 0; j < kDrawBatch; ++j)
            if (k0 + j < p.negative_samples) {
                const float dx = y.x - yq[j].x, dy = y.y - yq[j].y;
                const float d2 = dx * dx + dy * dy;
                if (d2 > 0.f) {
                    const float cr = repel_coeff(p.a, p.b, p.repulsion, d2);
                    sx += clip4(cr * dx);
                    sy += clip4(cr * dy);
                }
            }
    }
}

// One wave per new vertex; lane l holds the slots l and l + 64 of its list (at most CQS_HIP_NEIGHBORS_MAX = 100), as
// smooth_knn_kernel does.  The bisection is wave-uniform (psum is one wave_sum64_shfl a round, the same bits in every
// lane), and so are W, the initial position and every epoch's update: y lives in every lane's registers with the same
// bits, the two anchors of a lane are gathered once, and only the draws' coordinates are read per epoch - from the anchor
// array, 8 bytes each, L2 / Infinity Cache resident.  No LDS, no atomics, one writer per output word, nothing that depends
// on the grid.
__global__ __launch_bounds__(64 * kTransformWaves) void transform_kernel(const TransformParams p) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t v = (uint64_t)blockIdx.x * kTransformWaves + (threadIdx.x >> 6);
    if (v >= p.m) return;                                   // (the whole wave)
    const uint32_t c = p.counts[v];
    const uint64_t base = v * p.stride;
    const bool has0 = lane < c, has1 = lane + 64u < c;
    const uint32_t j0 = has0 ? p.rows[base + lane] : 0u;
    const uint32_t j1 = has1 ? p.rows[base + lane + 64u] : 0u;
    const float d0 = has0 ? distance_of(p.scores[base + lane]) : 0.f;
    const float d1 = has1 ? distance_of(p.scores[base + lane + 64u]) : 0.f;
    // the anchors of this lane's slots: fixed for all epochs
    const float2 y0 = has0 ? p.anchors[j0] : make_float2(0.f, 0.f);
    const float2 y1 = has1 ? p.anchors[j1] : make_float2(0.f, 0.f);

    // sigma (rho = 0) and the weights
    float sigma = 0.f, w0 = 0.f, w1 = 0.f;
    if (c != 0) {                                           // (wave-uniform)
        const float mean = cqs::wave_sum64_shfl(d0 + d1) / (float)c;
        const float target = transform_target(c);
        float lo = 0.f, hi = INFINITY, mid = 1.f;
        for (uint32_t round = 0; round < kBisectRounds; ++round) {
            float part = 0.f;
            if (has0) part = psum_term(d0, 0.f, mid);
            if (has1) part += psum_term(d1, 0.f, mid);
            const float psum = cqs::wave_sum64_shfl(part);
            if (fabsf(psum - target) < kBisectTolerance) break;
            bisect_step(psum, target, &lo, &hi, &mid);
        }
        sigma = fmaxf(mid, kMinSigmaScale * mean);
        if (has0) w0 = forward_weight(d0, 0.f, sigma);
        if (has1) w1 = forward_weight(d1, 0.f, sigma);
    }
    if (p.out_sigma && lane == 0) p.out_sigma[v] = sigma;
    if (p.out_weights) {                                    // slots past the count are written as 0
        if (lane < p.stride) p.out_weights[base + lane] = w0;
        if (lane + 64u < p.stride) p.out_weights[base + lane + 64u] = w1;
    }
    const float W = cqs::wave_sum64_shfl(w0 + w1);
    if (!(W > 0.f)) {                                       // c == 0, or every weight underflowed: the origin, never moves
        if (lane == 0) p.out_xy[v] = make_float2(0.f, 0.f);
        return;
    }
    const float w_top = cqs::wave_max64(fmaxf(w0, w1));

    // the initial position: each quotient and each product rounded once, slot l before slot l + 64, then the butterfly
    float2 y;
    {
        float sx = 0.f, sy = 0.f;
        if (has0) {
            const float q = w0 / W;
            const float px = q * y0.x, py = q * y0.y;
            sx += px;
            sy += py;
        }
        if (has1) {
            const float q = w1 / W;
            const float px = q * y1.x, py = q * y1.y;
            sx += px;
            sy += py;
        }
        y.x = cqs::wave_sum64_shfl(sx);
        y.y = cqs::wave_sum64_shfl(sy);
    }

    const float p0 = w0 / w_top, p1 = w1 / w_top;
    const uint32_t id = p.id_base + (uint32_t)v;
    for (uint32_t e = 1; e <= p.epochs; ++e) {
        const float alpha = transform_alpha(p.learning_rate, e, p.n_epochs);
        const uint32_t hv = hash_vertex(p.seed, e, id);
        float sx = 0.f, sy = 0.f;
        if (has0 && active(e, p0)) slot_terms(p, hv, lane, y, y0, sx, sy);
        if (has1 && active(e, p1)) slot_terms(p, hv, lane + 64u, y, y1, sx, sy);
        sx = cqs::wave_sum64_shfl(sx);
        sy = cqs::wave_sum64_shfl(sy);
        const float mx = alpha * sx, my = alpha * sy;
        y.x = y.x + mx;
        y.y = y.y + my;
    }
    if (lane == 0) p.out_xy[v] = y;
}

// ---- the launch ----------------------------------------------------------------------------------------------------------
struct DeviceBlock {   // what one call holds on the device besides the anchors; freed when it leaves scope
    uint32_t* rows = nullptr;
    float* scores = nullptr;
    uint32_t* counts = nullptr;
    float2* xy = nullptr;
    float* sigma = nullptr;
    float* weights = nullptr;
    ~DeviceBlock() {
        (void)hipFree(rows); (void)hipFree(scores); (void)hipFree(counts); (void)hipFree(xy); (void)hipFree(sigma); (void)hipFree(weights);
    }
};

// The arguments have passed plan_transform and m > 0; the device is current; d_anchors holds n pairs on it.  Uploads the
// lists, launches once on st, downloads the answers and waits.  The outputs are written only after the wait succeeded.
static hipError_t run_transform(hipStream_t st, uint64_t n, const float* d_anchors, uint64_t m, uint32_t stride,
                                const uint64_t* rows, const float* scores, const uint32_t* counts, const cqs_hip_layout_params& prm,
                                uint32_t E, uint64_t id_base, uint32_t epochs, float* out_xy, float* out_sigma, float* out_weights) {
    const size_t slots = (size_t)m * stride;
    std::vector<uint32_t> rows32(slots, 0u);                // ids are below n <= 2^31; slots past a count are not read
    for (uint64_t i = 0; i < m; ++i)
        for (uint32_t s = 0; s < counts[i]; ++s) rows32[i * stride + s] = (uint32_t)rows[i * stride + s];
    std::vector<float> xy((size_t)m * 2), sigma(out_sigma ? (size_t)m : 0), weights(out_weights ? slots : 0);
    DeviceBlock d;
    hipError_t e = hipMalloc(&d.rows, slots * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d.scores, slots * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&d.counts, (size_t)m * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d.xy, (size_t)m * sizeof(float2));
    if (e == hipSuccess && out_sigma) e = hipMalloc(&d.sigma, (size_t)m * sizeof(float));
    if (e == hipSuccess && out_weights) e = hipMalloc(&d.weights, slots * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(d.rows, rows32.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d.scores, scores, slots * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d.counts, counts, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return e; }
    TransformParams p;
    p.n = n; p.m = m; p.anchors = (const float2*)d_anchors; p.rows = d.rows; p.scores = d.scores; p.counts = d.counts;
    p.out_xy = d.xy; p.out_sigma = d.sigma; p.out_weights = d.weights;
    p.stride = stride; p.negative_samples = prm.negative_samples; p.n_epochs = E; p.epochs = transform_epochs_to_run(epochs, E);
    p.id_base = (uint32_t)id_base;
    p.a = prm.a; p.b = prm.b; p.learning_rate = prm.learning_rate; p.repulsion = prm.repulsion; p.seed = prm.seed;
    const uint32_t groups = (uint32_t)((m + kTransformWaves - 1) / kTransformWaves);
    hipLaunchKernelGGL(transform_kernel, dim3(groups), dim3(64 * kTransformWaves), 0, st, p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(xy.data(), d.xy, (size_t)m * sizeof(float2), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out_sigma) e = hipMemcpyAsync(sigma.data(), d.sigma, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out_weights) e = hipMemcpyAsync(weights.data(), d.weights, slots * sizeof(float), hipMemcpyDeviceToHost, st);
    const hipError_t waited = hipStreamSynchronize(st);     // (always: the host vectors leave scope)
    if (e == hipSuccess) e = waited;
    if (e != hipSuccess) return e;
    memcpy(out_xy, xy.data(), xy.size() * sizeof(float));
    if (out_sigma) memcpy(out_sigma, sigma.data(), sigma.size() * sizeof(float));
    if (out_weights) memcpy(out_weights, weights.data(), weights.size() * sizeof(float));
    return hipSuccess;
}

static int32_t device_code(hipError_t e) { return e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE; }

static void say_device(const char* what, hipError_t e) {
    char buf[256];
    snprintf(buf, sizeof buf, "transform: %s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    set_handleless_error(buf);
}

}  // namespace cqs_umap

extern "C" {

// Test hook (not part of the public header): the next cqs_hip_layout_transform on this handle fails as a device error
// would, before any device work - the layout ends up poisoned, the outputs untouched.
void cqs_hip_debug_layout_fail_next(cqs_hip_layout* x) CQS_ABI_TRY {
    if (x) x->inject_fail.store(1, std::memory_order_release);
} CQS_ABI_CATCH_VOID

int32_t cqs_hip_umap_transform(int32_t device, uint64_t n, const float* anchors_xy, uint64_t m, uint32_t stride,
                               const uint64_t* nbr_rows, const float* nbr_scores, const uint32_t* nbr_counts,
                               const cqs_hip_layout_params* params, uint64_t id_base, uint32_t epochs, float* out_xy,
                               float* out_sigma, float* out_weights) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_umap_transform");
    char why[192];
    cqs_umap::TransformPlanned plan;
    if (!cqs_umap::plan_transform(n, anchors_xy != nullptr, m, stride, nbr_rows, nbr_scores, nbr_counts, params,
                                  params ? params->n_epochs : 0u, id_base, out_xy != nullptr, &plan, why, sizeof why)) {
        cqs_umap::set_handleless_error(why);
        return CQS_HIP_ERR_INVALID;
    }
    cqs_umap::set_handleless_error("");
    if (plan.nothing) return CQS_HIP_OK;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) { cqs_umap::set_handleless_error("transform: no HIP device"); return CQS_HIP_ERR_NO_DEVICE; }
    if (device < 0 || device >= cnt) { cqs_umap::set_handleless_error("transform: no such device"); return CQS_HIP_ERR_INVALID; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { cqs_umap::say_device("hipSetDevice", e); return CQS_HIP_ERR_DEVICE; }
    hipStream_t st = nullptr;
    float* d_anchors = nullptr;
    e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&d_anchors, (size_t)n * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(d_anchors, anchors_xy, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = cqs_umap::run_transform(st, n, d_anchors, m, stride, nbr_rows, nbr_scores, nbr_counts, *params, plan.n_epochs, id_base,
                                    epochs, out_xy, out_sigma, out_weights);
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    (void)hipFree(d_anchors);
    if (e != hipSuccess) { cqs_umap::say_device("device work failed", e); return cqs_umap::device_code(e); }
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

int32_t cqs_hip_layout_transform(cqs_hip_layout* x, uint64_t m, uint32_t stride, const uint64_t* nbr_rows,
                                 const float* nbr_scores, const uint32_t* nbr_counts, uint32_t n_epochs, uint64_t id_base,
                                 uint32_t epochs, float* out_xy, float* out_sigma, float* out_weights) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_layout_transform");
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    char why[192];
    cqs_umap::TransformPlanned plan;
    if (!cqs_umap::plan_transform(x->n, true, m, stride, nbr_rows, nbr_scores, nbr_counts, &x->params, n_epochs, id_base,
                                  out_xy != nullptr, &plan, why, sizeof why))
        return cqs_umap::lfail(x, CQS_HIP_ERR_INVALID, why);
    if (plan.nothing) return CQS_HIP_OK;
    hipError_t e = x->inject_fail.exchange(0, std::memory_order_acq_rel) ? hipErrorUnknown : hipSetDevice(x->device);
    if (e == hipSuccess)
        e = cqs_umap::run_transform(x->stream, x->n, x->d_xy[x->cur], m, stride, nbr_rows, nbr_scores, nbr_counts, x->params,
                                    plan.n_epochs, id_base, epochs, out_xy, out_sigma, out_weights);
    if (e != hipSuccess) return cqs_umap::lfail(x, cqs_umap::device_code(e), "layout_transform: device work failed", e);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// `search` of the new vectors over the first n_anchors rows in blocks of 256 (the index is held per block), then the
// handle-less transform on the index's device.
int32_t cqs_hip_index_umap_transform(cqs_hip_index* idx, uint64_t n_anchors, const float* anchors_xy, const float* vectors,
                                     uint64_t m, uint32_t n_neighbors, uint32_t n_epochs, uint64_t seed, float* out_xy) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_umap_transform");
    if (!idx) return CQS_HIP_ERR_INVALID;
    const auto refuse = [&](int32_t code, const char* what) {   // (a transform's failure does not poison the index)
        std::lock_guard<std::mutex> g(idx->mu);
        idx->last_error = what;
        return code;
    };
    if (idx->sh) return refuse(CQS_HIP_ERR_INVALID, "umap_transform: not built for a row-sharded handle");
    if (cqs_hip_index_row_base(idx) != 0) return refuse(CQS_HIP_ERR_INVALID, "umap_transform: the handle's row_base is not 0");
    const uint64_t len = cqs_hip_index_len(idx);
    if (n_anchors > len) return refuse(CQS_HIP_ERR_INVALID, "umap_transform: more anchors than the index has rows");
    if (m && (!out_xy || !vectors || !anchors_xy)) return refuse(CQS_HIP_ERR_INVALID, "umap_transform: null buffer");
    if (m == 0) return CQS_HIP_OK;
    if (m > CQS_HIP_KNN_MAX_TARGETS) return refuse(CQS_HIP_ERR_INVALID, "umap_transform: more than CQS_HIP_KNN_MAX_TARGETS new vertices");
    if (n_anchors == 0) return refuse(CQS_HIP_ERR_INVALID, "umap_transform: no anchors");
    const uint32_t k = n_neighbors < 1u ? 1u : (n_neighbors > CQS_HIP_NEIGHBORS_MAX ? CQS_HIP_NEIGHBORS_MAX : n_neighbors);
    const uint32_t dim = cqs_hip_index_dim(idx);
    std::vector<uint32_t> keep;
    if (n_anchors != len) {                                  // the first n_anchors rows: whole words, then the ragged one
        keep.assign((size_t)((len + 31) / 32), 0u);
        for (uint64_t wd = 0; wd < n_anchors / 32; ++wd) keep[wd] = 0xFFFFFFFFu;
        if (n_anchors % 32) keep[n_anchors / 32] = (1u << (n_anchors % 32)) - 1u;
    }
    std::vector<uint64_t> rows((size_t)m * k, 0);            // (search leaves the slots past a count alone)
    std::vector<float> scores((size_t)m * k, 0.f);
    std::vector<uint32_t> counts((size_t)m, 0u);
    for (uint64_t at = 0; at < m; at += 256) {
        const uint32_t b = (uint32_t)(m - at < 256 ? m - at : 256);
        const int32_t rc = cqs_hip_index_search(idx, vectors + at * dim, b, dim, k, keep.empty() ? nullptr : keep.data(),
                                                CQS_HIP_MODE_RAW, 0.f, rows.data() + at * k, scores.data() + at * k, counts.data() + at);
        if (rc != CQS_HIP_OK) return rc;
    }
    cqs_hip_layout_params p;
    cqs_hip_layout_params_default(&p);
    p.n_epochs = n_epochs;
    p.seed = seed;
    const int32_t rc = cqs_hip_umap_transform(cqs_hip_index_device(idx), n_anchors, anchors_xy, m, k, rows.data(), scores.data(),
                                              counts.data(), &p, n_anchors, CQS_HIP_TRANSFORM_ALL, out_xy, nullptr, nullptr);
    if (rc != CQS_HIP_OK) {
        char why[256];
        cqs_hip_layout_last_error(nullptr, why, sizeof why);
        return refuse(rc, why);
    }
    return CQS_HIP_OK;
} CQS_ABI_CATCH(idx)

}  // extern "C"
