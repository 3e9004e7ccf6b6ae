// umap_host.h — the device-free part of the UMAP layout (include/cqs_hip.h "UMAP layout of a kNN graph"):
// the argument plan with its refusals in their documented order, the adjacency builder (forward lists, then a stable
// counting-sort transpose of them for the incoming-only ends), and the scalar rules the kernels share with the host: the
// hash and the draw, the initial coordinates, the active rule, alpha, the two force coefficients and the clip.  Plain C++
// over the caller's arrays, no HIP, no handle: umap_layout.hip calls the plan and the builder at `create`, the kernels of
// umap_graph.hip / umap_layout.hip call the scalar rules, and tests/umap_host_driver.cpp runs all of it under ASAN + UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/cqs_hip.h"

#if defined(__HIPCC__)
#define CQS_UMAP_HD __host__ __device__
#else
#define CQS_UMAP_HD
#endif

namespace cqs_umap {

constexpr uint64_t kMaxVertices = 1ull << 31;
constexpr uint32_t kMaxEpochs = 10000;
constexpr uint32_t kBisectRounds = 64;
constexpr float kBisectTolerance = 1e-5f;
constexpr float kMinSigmaScale = 1e-3f;

// ---- the argument plan ---------------------------------------------------------------------------------------------------
struct Planned {
    uint32_t n_epochs;   // params.n_epochs, or its default for this n where that is 0
};

// cqs_hip_layout_create's arguments, refused in the documented order (false; *why says which, Planned zeroed):
//   1 a NULL out, params or array (arrays may be NULL where n == 0: there is nothing to read)
//   2 n > 2^31
//   3 stride == 0 or stride > CQS_HIP_NEIGHBORS_MAX
//   4 a count greater than stride
//   5 a neighbour id >= n or equal to its own vertex (the text names the first such vertex)
//   6 a non-finite a, b, learning_rate or repulsion, or a non-positive a or b
//   7 n_epochs > 10000
inline bool plan_layout(bool out_present, uint64_t n, uint32_t stride, const uint64_t* rows, const float* scores,
                        const uint32_t* counts, const cqs_hip_layout_params* p, Planned* out, char* why, size_t why_cap) {
    *out = Planned{0};
    const auto say = [&](const char* s) { snprintf(why, why_cap, "layout: %s", s); return false; };
    if (why_cap) why[0] = 0;
    if (!out_present) return say("null output handle");
    if (!p) return say("null params");
    if (n > 0 && (!rows || !scores || !counts)) return say("null graph array");
    if (n > kMaxVertices) return say("more than 2^31 vertices");
    if (stride == 0 || stride > CQS_HIP_NEIGHBORS_MAX) return say("stride not in [1, CQS_HIP_NEIGHBORS_MAX]");
    for (uint64_t i = 0; i < n; ++i)
        if (counts[i] > stride) {
            snprintf(why, why_cap, "layout: vertex %llu has a count greater than the stride", (unsigned long long)i);
            return false;
        }
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t s = 0; s < counts[i]; ++s) {
            const uint64_t j = rows[i * stride + s];
            if (j >= n || j == i) {
                snprintf(why, why_cap, "layout: vertex %llu lists %s", (unsigned long long)i,
                         j == i ? "itself" : "a neighbour outside the graph");
                return false;
            }
        }
    if (!std::isfinite(p->a) || !std::isfinite(p->b) || !std::isfinite(p->learning_rate) || !std::isfinite(p->repulsion))
        return say("non-finite a, b, learning_rate or repulsion");
    if (!(p->a > 0.f) || !(p->b > 0.f)) return say("a and b must be positive");
    if (p->n_epochs > kMaxEpochs) return say("more than 10000 epochs");
    out->n_epochs = p->n_epochs ? p->n_epochs : (n <= 10000 ? 500u : 200u);
    return true;
}

// ---- the adjacency -------------------------------------------------------------------------------------------------------
// Vertex i's entries are off[i] .. off[i + 1]: its forward list in list order (counts[i] entries, each with its distance
// d = max(0, 1 - score) in f32), then the vertices that list i and are not in i's list, in ascending id (distance 0,
// unused: that direction is absent).  Every undirected edge so lies at both of its ends.
struct Adjacency {
    std::vector<uint64_t> off;    // [n + 1]
    std::vector<uint32_t> nbr;    // [edges]
    std::vector<float> dist;      // [edges]
};

CQS_UMAP_HD inline float distance_of(float score) {
    const float d = 1.0f - score;
    return d > 0.f ? d : 0.f;     // (a NaN score gives 0)
}

// Does i's forward list name j?  At most `stride` compares.
inline bool lists(const uint64_t* rows, const uint32_t* counts, uint32_t stride, uint64_t i, uint64_t j) {
    for (uint32_t s = 0; s < counts[i]; ++s)
        if (rows[i * stride + s] == j) return true;
    return false;
}

// The arguments have passed plan_layout.  n < 2 gives n + 1 zero offsets and no entries.
inline void build_adjacency(uint64_t n, uint32_t stride, const uint64_t* rows, const float* scores, const uint32_t* counts,
                            Adjacency* out) {
    out->off.assign(n + 1, 0);
    out->nbr.clear();
    out->dist.clear();
    if (n < 2) return;
    // counting sort, pass 1: the incoming-only ends of each vertex
    std::vector<uint64_t> incoming(n, 0);
    for (uint64_t j = 0; j < n; ++j)
        for (uint32_t s = 0; s < counts[j]; ++s) {
            const uint64_t i = rows[j * stride + s];
            if (!lists(rows, counts, stride, i, j)) ++incoming[i];
        }
    for (uint64_t i = 0; i < n; ++i) out->off[i + 1] = out->off[i] + counts[i] + incoming[i];
    out->nbr.assign(out->off[n], 0);
    out->dist.assign(out->off[n], 0.f);
    // the forward lists, and each vertex's cursor behind its own
    for (uint64_t i = 0; i < n; ++i) {
        for (uint32_t s = 0; s < counts[i]; ++s) {
            out->nbr[out->off[i] + s] = (uint32_t)rows[i * stride + s];
            out->dist[out->off[i] + s] = distance_of(scores[i * stride + s]);
        }
        incoming[i] = out->off[i] + counts[i];
    }
    // pass 2, stable: j ascending, so each vertex's incoming-only ends land in ascending id
    for (uint64_t j = 0; j < n; ++j)
        for (uint32_t s = 0; s < counts[j]; ++s) {
            const uint64_t i = rows[j * stride + s];
            if (!lists(rows, counts, stride, i, j)) out->nbr[incoming[i]++] = (uint32_t)j;
        }
}

// ---- the hash, the draw and the initial coordinates ----------------------------------------------------------------------
// murmur3's 32-bit finaliser
CQS_UMAP_HD inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// The part of the hash that a vertex's entries share in one epoch.
CQS_UMAP_HD inline uint32_t hash_vertex(uint64_t seed, uint32_t epoch, uint32_t vertex) {
    uint32_t h = fmix32((uint32_t)seed ^ 0x9E3779B9u);
    h = fmix32(h ^ (uint32_t)(seed >> 32));
    h = fmix32(h ^ epoch);
    return fmix32(h ^ vertex);
}
CQS_UMAP_HD inline uint32_t hash_draw(uint32_t vertex_hash, uint32_t slot, uint32_t draw) {
    return fmix32(fmix32(vertex_hash ^ slot) ^ draw);
}
CQS_UMAP_HD inline uint32_t hash5(uint64_t seed, uint32_t epoch, uint32_t vertex, uint32_t slot, uint32_t draw) {
    return hash_draw(hash_vertex(seed, epoch, vertex), slot, draw);
}
// A vertex of [0, n) from a hash; n <= 2^31.
CQS_UMAP_HD inline uint32_t draw_vertex(uint32_t h, uint64_t n) { return (uint32_t)(((uint64_t)h * n) >> 32); }
// Coordinate c (0 = x, 1 = y) of vertex i before the first epoch: uniform in [-10, 10) from the hash at epoch 0, slot 0,
// draw c.  The top 24 bits convert exactly; the product and the difference are each rounded once.  Host only (create).
inline float initial_coord(uint64_t seed, uint32_t vertex, uint32_t c) {
    const float u = (float)(hash5(seed, 0u, vertex, 0u, c) >> 8);
    const float scaled = u * (20.0f / 16777216.0f);
    return scaled - 10.0f;
}

// ---- the epoch's scalar rules --------------------------------------------------------------------------------------------
// An entry of probability p = s / w_max is active in epoch e (1-based) iff the integer part of e * p moves: all f32, each
// product rounded once.  p == 1 is active in every epoch; p below 1 / n_epochs at most once; a denormal or zero p never.
CQS_UMAP_HD inline bool active(uint32_t e, float p) { return floorf((float)e * p) != floorf((float)(e - 1u) * p); }
// alpha of epoch e of E: lr * (1 - (e - 1) / E)
inline float alpha_of(float lr, uint32_t e, uint32_t E) {
    const float done = (float)(e - 1u) / (float)E;
    const float left = 1.0f - done;
    return lr * left;
}
CQS_UMAP_HD inline float clip4(float x) { return fminf(4.0f, fmaxf(-4.0f, x)); }
// ca = -2ab d2^(b-1) / (a d2^b + 1), d2 > 0; d2^(b-1) as d2^b / d2 (one power per term)
CQS_UMAP_HD inline float attract_coeff(float a, float b, float d2) {
    const float pw = powf(d2, b);
    return (-2.0f * a * b) * (pw / d2) / (a * pw + 1.0f);
}
// cr = 2 repulsion b / ((0.001 + d2) (a d2^b + 1)), d2 > 0
CQS_UMAP_HD inline float repel_coeff(float a, float b, float repulsion, float d2) {
    const float pw = powf(d2, b);
    return (2.0f * repulsion * b) / ((0.001f + d2) * (a * pw + 1.0f));
}

// ---- smooth-kNN's scalar rules (the bisection itself is a wave's: umap_graph.hip) -----------------------------------------
// one term of psum, and the forward weight, of a neighbour at distance d
CQS_UMAP_HD inline float psum_term(float d, float rho, float mid) {
    const float x = d - rho;
    return x > 0.f ? expf(-x / mid) : 1.0f;
}
CQS_UMAP_HD inline float forward_weight(float d, float rho, float sigma) {
    const float x = d - rho;
    return (x <= 0.f || sigma == 0.f) ? 1.0f : expf(-x / sigma);
}
// the fuzzy union of the two directions (0 for an absent one): the same bits whichever end computes it
CQS_UMAP_HD inline float fuzzy_union(float wij, float wji) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float sum = wij + wji;
    const float prod = wij * wji;
    return sum - prod;
}

}  // namespace cqs_umap
