// umap_internal.h — the layout handle of include/cqs_hip.h's "UMAP layout of a kNN graph" and what umap_layout.hip asks
// of umap_graph.hip.  Internal to libcqs_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>

#include "../../include/cqs_hip.h"

struct cqs_hip_layout {
    mutable std::mutex mu;
    std::atomic<bool> poisoned{false};
    std::atomic<int> inject_fail{0};   // test hook: the next transform fails as a device error would
    std::string last_error;
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t n = 0, edges = 0;
    cqs_hip_layout_params params{};
    uint32_t n_epochs = 0;   // E: the params' value or its default for n
    uint32_t epoch = 0;      // epochs done
    // the adjacency (umap_host.h's order)
    uint64_t* d_off = nullptr;    // [n + 1]
    uint32_t* d_cnt = nullptr;    // [n] forward entries of each vertex
    uint32_t* d_nbr = nullptr;    // [edges]
    float* d_w = nullptr;         // [edges] s(i, j)
    float* d_rho = nullptr;       // [n]
    float* d_sigma = nullptr;     // [n]
    float w_max = 0.f;
    float* d_xy[2] = {nullptr, nullptr};   // [n, 2] each; d_xy[cur] holds the coordinates after `epoch` epochs
    int cur = 0;
};

namespace cqs_umap {

// rho, sigma and the weights of the adjacency already on the device; d_dist [edges] is the forward entries' distances.
// Enqueues on st and waits; *w_max is the grid maximum (0 where edges == 0).
hipError_t graph_weights(hipStream_t st, uint64_t n, uint64_t edges, const uint64_t* d_off, const uint32_t* d_cnt,
                         const uint32_t* d_nbr, const float* d_dist, float* d_rho, float* d_sigma, float* d_w, float* w_max);

// What umap_transform.hip asks of umap_layout.hip: a handle's failure (text, and poison on a device error; caller holds
// mu), and this thread's handle-less text, the one cqs_hip_layout_last_error(NULL, ..) returns.
int32_t lfail(cqs_hip_layout* x, int32_t code, const char* what, hipError_t e = hipSuccess);
void set_handleless_error(const char* text);

}  // namespace cqs_umap
