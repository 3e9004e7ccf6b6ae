// umap_layout.hip — the layout handle of include/cqs_hip.h's "UMAP layout of a kNN graph": `create` (the argument plan and
// the adjacency of umap_host.h on the host, the weights of umap_graph.hip on the device, the hashed initial coordinates),
// the epoch kernel - the hot path - and `run`, which launches it once per epoch on the layout's own stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "abi_guard.h"
#include "index_internal.h"
#include "pca_host.h"
#include "roctx.h"
#include "search_host.h"
#include "umap_host.h"
#include "umap_internal.h"
#include "wave_ops.h"

namespace cqs_umap {

constexpr uint32_t kEpochWaves = 4;   // waves (= vertices) per workgroup

struct EpochParams {
    uint64_t n;
    const uint64_t* off;
    const uint32_t* nbr;
    const float* w;
    const float2* cur;
    float2* next;
    float w_max, a, b, repulsion, alpha;
    uint32_t negative_samples, epoch;   // epoch: 1-based
    uint64_t seed;
};

// One wave per vertex, lanes across its adjacency entries in strides of 64 (a hub's in-degree can be thousands).  A lane
// tests its entry's active rule, gathers the other end's coordinates (8 bytes; the whole coordinate array is 8 MB at 1M
// vertices and stays in L2 / Infinity Cache while the adjacency streams at 8 bytes per entry), adds the attraction twice
// and then the entry's draws.  The lanes' sums are added by the fixed butterfly of wave_sum64_shfl and lane 0 stores the
// new coordinates into the other buffer: a snapshot update, no LDS, no atomics, nothing that depends on the grid.
// Registers are few and nothing is shared, so four waves a workgroup is only the unit of scheduling; the latency of the
// gathers is hidden by the other waves on the SIMD.
__global__ __launch_bounds__(64 * kEpochWaves) void layout_epoch_kernel(const EpochParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t v64 = (uint64_t)blockIdx.x * kEpochWaves + (threadIdx.x >> 6);
    if (v64 >= p.n) return;                                  // (the whole wave)
    const uint32_t v = (uint32_t)v64;
    const uint64_t base = p.off[v], end = p.off[v + 1];
    const float2 yi = p.cur[v];
    const uint32_t hv = hash_vertex(p.seed, p.epoch, v);
    float sx = 0.f, sy = 0.f;
    for (uint64_t t = base + lane; t < end; t += 64u) {
        const float prob = p.w[t] / p.w_max;
        if (!active(p.epoch, prob)) continue;
        const uint32_t slot = (uint32_t)(t - base);
        {
            const float2 yj = p.cur[p.nbr[t]];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const float d2 = dx * dx + dy * dy;
            if (d2 > 0.f) {
                const float ca = attract_coeff(p.a, p.b, d2);
                sx += 2.0f * clip4(ca * dx);
                sy += 2.0f * clip4(ca * dy);
            }
        }
        for (uint32_t k = 0; k < p.negative_samples; ++k) {
            const uint32_t q = draw_vertex(hash_draw(hv, slot, k), p.n);
            if (q == v) continue;
            const float2 yq = p.cur[q];
            const float dx = yi.x - yq.x, dy = yi.y - yq.y;
            const float d2 = dx * dx + dy * dy;
            if (d2 > 0.f) {
                const float cr = repel_coeff(p.a, p.b, p.repulsion, d2);
                sx += clip4(cr * dx);
                sy += clip4(cr * dy);
            }
        }
    }
    sx = cqs::wave_sum64_shfl(sx);
    sy = cqs::wave_sum64_shfl(sy);
    if (lane == 0) p.next[v] = make_float2(yi.x + p.alpha * sx, yi.y + p.alpha * sy);
}

// ---- the handle ----------------------------------------------------------------------------------------------------------
static thread_local std::string t_create_error;   // why this thread's last `create` was refused

void set_handleless_error(const char* text) { t_create_error = text; }

int32_t lfail(cqs_hip_layout* x, int32_t code, const char* what, hipError_t e) {
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else snprintf(buf, sizeof buf, "%s", what);
    x->last_error = buf;
    if (code == CQS_HIP_ERR_DEVICE) x->poisoned.store(true, std::memory_order_release);
    return code;
}

#define LAYOUT_TRY(x, expr)                                                                                              \
    do {                                                                                                                 \
        hipError_t _e = (expr);                                                                                          \
        if (_e != hipSuccess)                                                                                            \
            return cqs_umap::lfail((x), _e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, #expr, _e);  \
    } while (0)

static void release(cqs_hip_layout* x) {
    (void)hipSetDevice(x->device);
    if (x->stream) { (void)hipStreamSynchronize(x->stream); (void)hipStreamDestroy(x->stream); }
    (void)hipFree(x->d_off); (void)hipFree(x->d_cnt); (void)hipFree(x->d_nbr); (void)hipFree(x->d_w);
    (void)hipFree(x->d_rho); (void)hipFree(x->d_sigma); (void)hipFree(x->d_xy[0]); (void)hipFree(x->d_xy[1]);
    delete x;
}

// The device half of `create`: the adjacency up, the weights, the initial coordinates.  The handle is the caller's to
// release on failure.
static int32_t fill(cqs_hip_layout* x, const Adjacency& adj, const uint32_t* counts, uint64_t seed) {
    const uint64_t n = x->n, edges = x->edges;
    LAYOUT_TRY(x, hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
    if (n == 0) return CQS_HIP_OK;
    const size_t e1 = (size_t)(edges ? edges : 1);
    float* d_dist = nullptr;
    LAYOUT_TRY(x, hipMalloc(&x->d_off, (size_t)(n + 1) * sizeof(uint64_t)));
    LAYOUT_TRY(x, hipMalloc(&x->d_cnt, (size_t)n * sizeof(uint32_t)));
    LAYOUT_TRY(x, hipMalloc(&x->d_nbr, e1 * sizeof(uint32_t)));
    LAYOUT_TRY(x, hipMalloc(&x->d_w, e1 * sizeof(float)));
    LAYOUT_TRY(x, hipMalloc(&x->d_rho, (size_t)n * sizeof(float)));
    LAYOUT_TRY(x, hipMalloc(&x->d_sigma, (size_t)n * sizeof(float)));
    LAYOUT_TRY(x, hipMalloc(&x->d_xy[0], (size_t)n * sizeof(float2)));
    LAYOUT_TRY(x, hipMalloc(&x->d_xy[1], (size_t)n * sizeof(float2)));
    LAYOUT_TRY(x, hipMalloc(&d_dist, e1 * sizeof(float)));
    std::vector<float> xy((size_t)n * 2, 0.f);
    if (n >= 2)
        for (uint64_t i = 0; i < n; ++i) {
            xy[2 * i] = initial_coord(seed, (uint32_t)i, 0u);
            xy[2 * i + 1] = initial_coord(seed, (uint32_t)i, 1u);
        }
    hipError_t e = hipMemcpyAsync(x->d_off, adj.off.data(), (size_t)(n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(x->d_cnt, counts, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess && edges) e = hipMemcpyAsync(x->d_nbr, adj.nbr.data(), (size_t)edges * sizeof(uint32_t), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess && edges) e = hipMemcpyAsync(d_dist, adj.dist.data(), (size_t)edges * sizeof(float), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(x->d_xy[0], xy.data(), (size_t)n * sizeof(float2), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess) e = graph_weights(x->stream, n, edges, x->d_off, x->d_cnt, x->d_nbr, d_dist, x->d_rho, x->d_sigma, x->d_w, &x->w_max);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream);   // (the host arrays leave scope)
    (void)hipFree(d_dist);
    LAYOUT_TRY(x, e);
    return CQS_HIP_OK;
}

}  // namespace cqs_umap

using cqs_umap::lfail;

extern "C" {

void cqs_hip_layout_params_default(cqs_hip_layout_params* p) CQS_ABI_TRY {
    if (!p) return;
    p->a = 1.5769434603f;
    p->b = 0.8950608779f;
    p->learning_rate = 1.0f;
    p->repulsion = 1.0f;
    p->negative_samples = 5;
    p->n_epochs = 0;
    p->seed = 42;
} CQS_ABI_CATCH_VOID

int32_t cqs_hip_layout_create(int32_t device, uint64_t n, uint32_t stride, const uint64_t* knn_rows, const float* knn_scores,
                              const uint32_t* knn_counts, const cqs_hip_layout_params* params, cqs_hip_layout** out) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_layout_create");
    if (out) *out = nullptr;
    char why[192];
    cqs_umap::Planned plan;
    if (!cqs_umap::plan_layout(out != nullptr, n, stride, knn_rows, knn_scores, knn_counts, params, &plan, why, sizeof why)) {
        cqs_umap::t_create_error = why;
        return CQS_HIP_ERR_INVALID;
    }
    cqs_umap::t_create_error.clear();
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) { cqs_umap::t_create_error = "layout: no HIP device"; return CQS_HIP_ERR_NO_DEVICE; }
    if (device < 0 || device >= cnt) { cqs_umap::t_create_error = "layout: no such device"; return CQS_HIP_ERR_INVALID; }
    cqs_umap::Adjacency adj;
    cqs_umap::build_adjacency(n, stride, knn_rows, knn_scores, knn_counts, &adj);
    cqs_hip_layout* x = new cqs_hip_layout();
    x->device = device;
    x->n = n;
    x->edges = adj.off[n];
    x->params = *params;
    x->n_epochs = plan.n_epochs;
    int32_t rc = CQS_HIP_OK;
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) rc = lfail(x, CQS_HIP_ERR_DEVICE, "hipSetDevice", e);
    else rc = cqs_umap::fill(x, adj, knn_counts, params->seed);
    if (rc != CQS_HIP_OK) {
        cqs_umap::t_create_error = x->last_error;
        cqs_umap::release(x);
        return rc;
    }
    *out = x;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

uint64_t cqs_hip_layout_len(const cqs_hip_layout* x) CQS_ABI_TRY {
    return x ? x->n : 0;
} CQS_ABI_CATCH_VAL(0)

uint64_t cqs_hip_layout_edges(const cqs_hip_layout* x) CQS_ABI_TRY {
    return x ? x->edges : 0;
} CQS_ABI_CATCH_VAL(0)

uint32_t cqs_hip_layout_epochs(const cqs_hip_layout* x) CQS_ABI_TRY {
    return x ? x->n_epochs : 0;
} CQS_ABI_CATCH_VAL(0)

int32_t cqs_hip_layout_graph(cqs_hip_layout* x, uint64_t* offsets, uint32_t* nbrs, float* weights, float* rho, float* sigma,
                             float* w_max) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (w_max) *w_max = x->w_max;
    if (x->n == 0) {
        if (offsets) offsets[0] = 0;
        return CQS_HIP_OK;
    }
    LAYOUT_TRY(x, hipSetDevice(x->device));
    const size_t n = (size_t)x->n, edges = (size_t)x->edges;
    if (offsets) LAYOUT_TRY(x, hipMemcpyAsync(offsets, x->d_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, x->stream));
    if (nbrs && edges) LAYOUT_TRY(x, hipMemcpyAsync(nbrs, x->d_nbr, edges * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    if (weights && edges) LAYOUT_TRY(x, hipMemcpyAsync(weights, x->d_w, edges * sizeof(float), hipMemcpyDeviceToHost, x->stream));
    if (rho) LAYOUT_TRY(x, hipMemcpyAsync(rho, x->d_rho, n * sizeof(float), hipMemcpyDeviceToHost, x->stream));
    if (sigma) LAYOUT_TRY(x, hipMemcpyAsync(sigma, x->d_sigma, n * sizeof(float), hipMemcpyDeviceToHost, x->stream));
    LAYOUT_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

int32_t cqs_hip_layout_set_coords(cqs_hip_layout* x, const float* xy) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (x->n == 0) return CQS_HIP_OK;
    if (!xy) return lfail(x, CQS_HIP_ERR_INVALID, "set_coords: null coordinates");
    LAYOUT_TRY(x, hipSetDevice(x->device));
    LAYOUT_TRY(x, hipMemcpyAsync(x->d_xy[x->cur], xy, (size_t)x->n * sizeof(float2), hipMemcpyHostToDevice, x->stream));
    LAYOUT_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

int32_t cqs_hip_layout_coords(cqs_hip_layout* x, float* xy) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (x->n == 0) return CQS_HIP_OK;
    if (!xy) return lfail(x, CQS_HIP_ERR_INVALID, "coords: null output buffer");
    LAYOUT_TRY(x, hipSetDevice(x->device));
    LAYOUT_TRY(x, hipMemcpyAsync(xy, x->d_xy[x->cur], (size_t)x->n * sizeof(float2), hipMemcpyDeviceToHost, x->stream));
    LAYOUT_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

int32_t cqs_hip_layout_run(cqs_hip_layout* x, uint32_t epochs, uint32_t* epoch_after) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_layout_run");
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (epoch_after) *epoch_after = x->epoch;
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    const uint32_t left = x->n_epochs - x->epoch;
    const uint32_t todo = epochs < left ? epochs : left;
    if (x->n < 2 || x->edges == 0) {                         // nothing moves: only the counter does
        x->epoch += todo;
        if (epoch_after) *epoch_after = x->epoch;
        return CQS_HIP_OK;
    }
    if (todo == 0) return CQS_HIP_OK;
    LAYOUT_TRY(x, hipSetDevice(x->device));
    cqs_umap::EpochParams p;
    p.n = x->n; p.off = x->d_off; p.nbr = x->d_nbr; p.w = x->d_w;
    p.w_max = x->w_max; p.a = x->params.a; p.b = x->params.b; p.repulsion = x->params.repulsion;
    p.negative_samples = x->params.negative_samples; p.seed = x->params.seed;
    const uint32_t groups = (uint32_t)((x->n + cqs_umap::kEpochWaves - 1) / cqs_umap::kEpochWaves);
    for (uint32_t i = 0; i < todo; ++i) {
        p.epoch = x->epoch + 1u;
        p.alpha = cqs_umap::alpha_of(x->params.learning_rate, p.epoch, x->n_epochs);
        p.cur = (const float2*)x->d_xy[x->cur];
        p.next = (float2*)x->d_xy[x->cur ^ 1];
        hipLaunchKernelGGL(cqs_umap::layout_epoch_kernel, dim3(groups), dim3(64 * cqs_umap::kEpochWaves), 0, x->stream, p);
        LAYOUT_TRY(x, hipGetLastError());
        x->cur ^= 1;
        x->epoch += 1u;
    }
    LAYOUT_TRY(x, hipStreamSynchronize(x->stream));
    if (epoch_after) *epoch_after = x->epoch;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

size_t cqs_hip_layout_last_error(const cqs_hip_layout* x, char* buf, size_t cap) CQS_ABI_TRY {
    if (!buf || cap == 0) return 0;
    if (!x) return cqs_search::copy_last_error(cqs_umap::t_create_error.data(), cqs_umap::t_create_error.size(), buf, cap);
    std::lock_guard<std::mutex> g(x->mu);
    return cqs_search::copy_last_error(x->last_error.data(), x->last_error.size(), buf, cap);
} CQS_ABI_CATCH_VAL(0)

void cqs_hip_layout_destroy(cqs_hip_layout* x) CQS_ABI_TRY {
    if (!x) return;
    cqs_umap::release(x);
} CQS_ABI_CATCH_VOID

// cqs_hip_index_knn_graph over the whole corpus, then a layout run to its end: the index is held per graph call only.
// init == CQS_HIP_UMAP_INIT_PCA: the layout starts from the scaled PCA projection of the rows (pca_host.h) where there is one.
int32_t cqs_hip_index_umap_project_init(cqs_hip_index* idx, uint32_t n_neighbors, uint32_t n_epochs, uint64_t seed,
                                        uint32_t init, float* out_xy) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_umap_project");
    if (!idx) return CQS_HIP_ERR_INVALID;
    const auto refuse = [&](int32_t code, const char* what) {   // (a layout's failure does not poison the index)
        std::lock_guard<std::mutex> g(idx->mu);
        idx->last_error = what;
        return code;
    };
    const uint64_t n = cqs_hip_index_len(idx);
    if (cqs_hip_index_row_base(idx) != 0) return refuse(CQS_HIP_ERR_INVALID, "umap_project: the handle's row_base is not 0");
    if (n && !out_xy) return refuse(CQS_HIP_ERR_INVALID, "umap_project: null output buffer");
    if (init != CQS_HIP_UMAP_INIT_RANDOM && init != CQS_HIP_UMAP_INIT_PCA) return refuse(CQS_HIP_ERR_INVALID, "umap_project: unknown init");
    std::vector<float> start;                                   // the PCA initial coordinates; empty: the hashed ones stay
    if (init == CQS_HIP_UMAP_INIT_PCA && n >= 2) {
        // what the layout would refuse anyway, before the index is held for the passes
        if (n_epochs > cqs_umap::kMaxEpochs) return refuse(CQS_HIP_ERR_INVALID, "layout: more than 10000 epochs");
        const uint32_t dim = cqs_hip_index_dim(idx), nc = dim < 2 ? 1u : 2u;
        std::vector<float> mean(dim), axes((size_t)nc * dim), proj((size_t)n * nc);
        float variance[2], total;
        int32_t rc = cqs_hip_index_pca(idx, nc, 0, seed, mean.data(), axes.data(), variance, &total);
        if (rc == CQS_HIP_OK) rc = cqs_hip_index_pca_project(idx, mean.data(), axes.data(), nc, 0, n, proj.data());
        if (rc != CQS_HIP_OK) return rc;                        // (the reason is in the index's last_error)
        start.resize((size_t)n * 2);
        if (!cqs_pca::noisy_scale_coords(proj.data(), n, nc, seed, start.data())) start.clear();
    }
    uint32_t limit = n_neighbors > 1 ? n_neighbors - 1u : 1u;
    if (limit > CQS_HIP_NEIGHBORS_MAX) limit = CQS_HIP_NEIGHBORS_MAX;
    std::vector<uint64_t> rows((size_t)n * limit);
    std::vector<float> scores((size_t)n * limit);
    std::vector<uint32_t> counts((size_t)n);
    for (uint64_t at = 0; at < n; at += 4096) {
        const uint64_t m = n - at < 4096 ? n - at : 4096;
        const int32_t rc = cqs_hip_index_knn_graph(idx, at, m, limit, rows.data() + at * limit, scores.data() + at * limit,
                                                   counts.data() + at);
        if (rc != CQS_HIP_OK) return rc;
    }
    cqs_hip_layout_params p;
    cqs_hip_layout_params_default(&p);
    p.n_epochs = n_epochs;
    p.seed = seed;
    cqs_hip_layout* lay = nullptr;
    char why[256];
    int32_t rc = cqs_hip_layout_create(cqs_hip_index_device(idx), n, limit, rows.data(), scores.data(), counts.data(), &p, &lay);
    if (rc != CQS_HIP_OK) {
        cqs_hip_layout_last_error(nullptr, why, sizeof why);
        return refuse(rc, why);
    }
    if (!start.empty()) rc = cqs_hip_layout_set_coords(lay, start.data());
    if (rc == CQS_HIP_OK) rc = cqs_hip_layout_run(lay, cqs_hip_layout_epochs(lay), nullptr);
    if (rc == CQS_HIP_OK) rc = cqs_hip_layout_coords(lay, out_xy);
    if (rc != CQS_HIP_OK) {
        cqs_hip_layout_last_error(lay, why, sizeof why);
        cqs_hip_layout_destroy(lay);
        return refuse(rc, why);
    }
    cqs_hip_layout_destroy(lay);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(idx)

int32_t cqs_hip_index_umap_project(cqs_hip_index* idx, uint32_t n_neighbors, uint32_t n_epochs, uint64_t seed,
                                   float* out_xy) CQS_ABI_TRY {
    return cqs_hip_index_umap_project_init(idx, n_neighbors, n_epochs, seed, CQS_HIP_UMAP_INIT_RANDOM, out_xy);
} CQS_ABI_CATCH(idx)

}  // extern "C"
