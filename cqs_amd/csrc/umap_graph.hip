// umap_graph.hip — the fuzzy simplicial set of a kNN graph on the device (include/cqs_hip.h "UMAP layout of a kNN graph"):
//     smooth_knn_kernel     per vertex rho (smallest positive distance) and sigma (umap-learn's bisection), one wave each
//     union_weights_kernel  s(i, j) of every adjacency entry in adjacency order, and the grid maximum
// The adjacency itself (offsets, ids, the forward entries' distances) is built on the host by umap_host.h at `create`;
// both kernels call that header's scalar rules, so the host restates them exactly.
#include <hip/hip_runtime.h>

#include <cstring>

#include "umap_host.h"
#include "umap_internal.h"
#include "wave_ops.h"

namespace cqs_umap {

constexpr uint32_t kWavesPerGroup = 4;

// One wave per vertex; lane l holds the forward slots l and l + 64 (a list has at most CQS_HIP_NEIGHBORS_MAX = 100), as
// knn_finish_kernel does.  rho is a wave minimum, the mean a wave sum; the bisection is wave-uniform: psum is one
// wave_sum64_shfl per round, the same bits in every lane, so every lane takes the same branch.
__global__ __launch_bounds__(64 * kWavesPerGroup) void smooth_knn_kernel(uint64_t n, const uint64_t* off, const uint32_t* cnt,
                                                                         const float* dist, float* rho_out, float* sigma_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t v = (uint64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
    if (v >= n) return;                                   // (the whole wave)
    const uint32_t c = cnt[v];
    const uint64_t base = off[v];
    const bool has0 = lane < c, has1 = lane + 64u < c;
    const float d0 = has0 ? dist[base + lane] : 0.f;
    const float d1 = has1 ? dist[base + lane + 64u] : 0.f;
    if (c == 0) {
        if (lane == 0) { rho_out[v] = 0.f; sigma_out[v] = 0.f; }
        return;
    }
    // the smallest d > 0: -max(-d) over the positive ones, -inf where there is none
    float neg = -INFINITY;
    if (has0 && d0 > 0.f) neg = -d0;
    if (has1 && d1 > 0.f) neg = fmaxf(neg, -d1);
    neg = cqs::wave_max64(neg);
    const float rho = neg == -INFINITY ? 0.f : -neg;
    const float mean = cqs::wave_sum64_shfl(d0 + d1) / (float)c;
    const float target = log2f((float)(c + 1u));
    float lo = 0.f, hi = INFINITY, mid = 1.f;
    for (uint32_t round = 0; round < kBisectRounds; ++round) {
        float part = 0.f;
        if (has0) part = psum_term(d0, rho, mid);
        if (has1) part += psum_term(d1, rho, mid);
        const float psum = cqs::wave_sum64_shfl(part);
        if (fabsf(psum - target) < kBisectTolerance) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) * 0.5f;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.f : (lo + hi) * 0.5f;
        }
    }
    if (lane == 0) {
        rho_out[v] = rho;
        sigma_out[v] = fmaxf(mid, kMinSigmaScale * mean);
    }
}

// One wave per vertex, lanes across its adjacency entries in strides of 64.  Entry (v, j): the forward weight where the
// entry is one of v's own list, and the reverse one looked up in j's forward list (at most 100 compares); both come from
// forward_weight on (distance, rho, sigma) of the listing vertex, so the two ends of an edge compute the same two numbers
// and fuzzy_union, symmetric in them, the same bits.  The maximum is order-free: lanes, then the wave, then one atomic
// max per wave on the bits (weights are >= 0, where the bits order as the values).
__global__ __launch_bounds__(64 * kWavesPerGroup) void union_weights_kernel(uint64_t n, const uint64_t* off, const uint32_t* cnt,
                                                                            const uint32_t* nbr, const float* dist,
                                                                            const float* rho, const float* sigma, float* w,
                                                                            unsigned int* w_max_bits) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t v = (uint64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
    if (v >= n) return;
    const uint64_t base = off[v], end = off[v + 1];
    const uint32_t c = cnt[v];
    const float rho_v = rho[v], sigma_v = sigma[v];
    float m = 0.f;
    for (uint64_t t = base + lane; t < end; t += 64u) {
        const uint32_t j = nbr[t];
        const float wij = t - base < c ? forward_weight(dist[t], rho_v, sigma_v) : 0.f;
        float wji = 0.f;
        const uint64_t oj = off[j];
        const uint32_t cj = cnt[j];
        for (uint32_t r = 0; r < cj; ++r)
            if (nbr[oj + r] == (uint32_t)v) {
                wji = forward_weight(dist[oj + r], rho[j], sigma[j]);
                break;
            }
        const float s = fuzzy_union(wij, wji);
        w[t] = s;
        m = fmaxf(m, s);
    }
    m = cqs::wave_max64(m);
    if (lane == 0 && end > base) atomicMax(w_max_bits, __float_as_uint(m));
}

hipError_t graph_weights(hipStream_t st, uint64_t n, uint64_t edges, const uint64_t* d_off, const uint32_t* d_cnt,
                         const uint32_t* d_nbr, const float* d_dist, float* d_rho, float* d_sigma, float* d_w, float* w_max) {
    *w_max = 0.f;
    if (n == 0) return hipSuccess;
    const uint32_t groups = (uint32_t)((n + kWavesPerGroup - 1) / kWavesPerGroup);
    unsigned int* d_max = nullptr;
    hipError_t e = hipMalloc(&d_max, sizeof(unsigned int));
    if (e != hipSuccess) return e;
    unsigned int bits = 0;
    e = hipMemsetAsync(d_max, 0, sizeof(unsigned int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(smooth_knn_kernel, dim3(groups), dim3(64 * kWavesPerGroup), 0, st, n, d_off, d_cnt, d_dist, d_rho, d_sigma);
        e = hipGetLastError();
    }
    if (e == hipSuccess && edges) {
        hipLaunchKernelGGL(union_weights_kernel, dim3(groups), dim3(64 * kWavesPerGroup), 0, st, n, d_off, d_cnt, d_nbr, d_dist,
                           d_rho, d_sigma, d_w, d_max);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bits, d_max, sizeof bits, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_max);
    if (e == hipSuccess) memcpy(w_max, &bits, sizeof bits);
    return e;
}

}  // namespace cqs_umap
