// umap_transform_host.h — the device-free part of the UMAP transform (include/cqs_hip.h "UMAP transform of new rows",
// DESIGN.md §3.18a): the argument plan with its refusals in their documented order, the default epoch count, the
// quarter-rate alpha, the bisection's target, and the f32 restatement of a vertex's weights and initial position, the
// wave's order of addition included (64 host slots added as wave_sum64_shfl adds its lanes).  Plain C++ over the caller's
// arrays, no HIP, no handle: umap_transform.hip calls the plan and the scalar rules, transform_kernel restates the wave
// functions lane by lane, and tests/umap_transform_host_driver.cpp runs all of it under ASAN + UBSan.
#pragma once
#include "umap_host.h"

namespace cqs_umap {

constexpr uint64_t kMaxVertexIds = 1ull << 32;   // a vertex id is hashed as a u32

// ---- the argument plan ---------------------------------------------------------------------------------------------------
struct TransformPlanned {
    bool nothing;        // m == 0: the call returns OK and touches nothing
    uint32_t n_epochs;   // E: n_epochs, or its default for this m where that is 0
};

// E where n_epochs is 0: umap-learn's transform defaults
inline uint32_t transform_default_epochs(uint64_t m) { return m <= 10000 ? 100u : 30u; }

// The transform's arguments, refused in the documented order (false; *why says which, *out zeroed).  `n_epochs` is the
// count that holds for the call: the params' own for the handle-less call, the argument's for a layout handle.
//   1 NULL params; out_xy, an array or the anchors NULL while m > 0
//   2 m == 0 is accepted here (nothing = true)
//   3 n == 0
//   4 n > 2^31
//   5 m > CQS_HIP_KNN_MAX_TARGETS
//   6 id_base + m > 2^32
//   7 stride == 0 or stride > CQS_HIP_NEIGHBORS_MAX
//   8 a count greater than stride
//   9 a neighbour id >= n (the text names the first such vertex)
//  10 the layout's parameter checks: a non-finite a, b, learning_rate or repulsion, a non-positive a or b, n_epochs > 10000
inline bool plan_transform(uint64_t n, bool anchors_present, uint64_t m, uint32_t stride, const uint64_t* rows,
                           const float* scores, const uint32_t* counts, const cqs_hip_layout_params* p, uint32_t n_epochs,
                           uint64_t id_base, bool out_present, TransformPlanned* out, char* why, size_t why_cap) {
    *out = TransformPlanned{false, 0};
    const auto say = [&](const char* s) { snprintf(why, why_cap, "transform: %s", s); return false; };
    if (why_cap) why[0] = 0;
    if (!p) return say("null params");
    if (m > 0 && !out_present) return say("null output buffer");
    if (m > 0 && (!rows || !scores || !counts)) return say("null neighbour array");
    if (m > 0 && !anchors_present) return say("null anchors");
    if (m == 0) {
        out->nothing = true;
        return true;
    }
    if (n == 0) return say("no anchors");
    if (n > kMaxVertices) return say("more than 2^31 anchors");
    if (m > CQS_HIP_KNN_MAX_TARGETS) return say("more than CQS_HIP_KNN_MAX_TARGETS new vertices");
    if (id_base > kMaxVertexIds - m) return say("id_base + m is greater than 2^32");
    if (stride == 0 || stride > CQS_HIP_NEIGHBORS_MAX) return say("stride not in [1, CQS_HIP_NEIGHBORS_MAX]");
    for (uint64_t i = 0; i < m; ++i)
        if (counts[i] > stride) {
            snprintf(why, why_cap, "transform: vertex %llu has a count greater than the stride", (unsigned long long)i);
            return false;
        }
    for (uint64_t i = 0; i < m; ++i)
        for (uint32_t s = 0; s < counts[i]; ++s)
            if (rows[i * stride + s] >= n) {
                snprintf(why, why_cap, "transform: vertex %llu lists a neighbour outside the anchors", (unsigned long long)i);
                return false;
            }
    if (!std::isfinite(p->a) || !std::isfinite(p->b) || !std::isfinite(p->learning_rate) || !std::isfinite(p->repulsion))
        return say("non-finite a, b, learning_rate or repulsion");
    if (!(p->a > 0.f) || !(p->b > 0.f)) return say("a and b must be positive");
    if (n_epochs > kMaxEpochs) return say("more than 10000 epochs");
    out->n_epochs = n_epochs ? n_epochs : transform_default_epochs(m);
    return true;
}

// How many of the E epochs a call runs: `epochs` clamped at E (CQS_HIP_TRANSFORM_ALL is the largest u32).
inline uint32_t transform_epochs_to_run(uint32_t epochs, uint32_t E) { return epochs < E ? epochs : E; }

// ---- the scalar rules ----------------------------------------------------------------------------------------------------
// alpha of epoch e of E: (lr / 4) * (1 - (e - 1) / E), each operation rounded once
CQS_UMAP_HD inline float transform_alpha(float lr, uint32_t e, uint32_t E) {
    const float done = (float)(e - 1u) / (float)E;
    const float left = 1.0f - done;
    return (lr * 0.25f) * left;
}
// the bisection's target: the list holds all n_neighbors entries and no self entry
CQS_UMAP_HD inline float transform_target(uint32_t c) { return log2f((float)c); }
// One step of the header's bisection after psum has been compared with the target (the caller has tested the tolerance).
CQS_UMAP_HD inline void bisect_step(float psum, float target, float* lo, float* hi, float* mid) {
    if (psum > target) {
        *hi = *mid;
        *mid = (*lo + *hi) * 0.5f;
    } else {
        *lo = *mid;
        *mid = *hi == INFINITY ? *mid * 2.f : (*lo + *hi) * 0.5f;
    }
}

// ---- a wave on the host --------------------------------------------------------------------------------------------------
// 64 slots added as wave_sum64_shfl adds its lanes: v[l] += v[l ^ 32], then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; every slot ends with
// the same bits.
inline float host_wave_sum64(const float* lanes) {
    float v[64], t[64];
    for (int l = 0; l < 64; ++l) v[l] = lanes[l];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 64; ++l) v[l] = t[l];
    }
    return v[0];
}

// Weights of one new vertex from its c <= CQS_HIP_NEIGHBORS_MAX raw scores, as transform_kernel computes them: lane l
// holds the slots l and l + 64.  Writes w[0 .. c), returns sigma (0 where c == 0).
inline float transform_weights(const float* scores, uint32_t c, float* w) {
    if (c == 0) return 0.f;
    float d[128] = {0.f}, lanes[64];
    for (uint32_t t = 0; t < c; ++t) d[t] = distance_of(scores[t]);
    for (int l = 0; l < 64; ++l) lanes[l] = d[l] + d[l + 64];
    const float mean = host_wave_sum64(lanes) / (float)c;
    const float target = transform_target(c);
    float lo = 0.f, hi = INFINITY, mid = 1.f;
    for (uint32_t round = 0; round < kBisectRounds; ++round) {
        for (uint32_t l = 0; l < 64; ++l) {
            float part = 0.f;
            if (l < c) part = psum_term(d[l], 0.f, mid);
            if (l + 64u < c) part += psum_term(d[l + 64u], 0.f, mid);
            lanes[l] = part;
        }
        const float psum = host_wave_sum64(lanes);
        if (fabsf(psum - target) < kBisectTolerance) break;
        bisect_step(psum, target, &lo, &hi, &mid);
    }
    const float sigma = fmaxf(mid, kMinSigmaScale * mean);
    for (uint32_t t = 0; t < c; ++t) w[t] = forward_weight(d[t], 0.f, sigma);
    return sigma;
}

// Initial position of one new vertex: y = sum of (w_t / W) * Y[j_t], each quotient and each product rounded once, a lane's
// two slots added first and the lanes then as the wave adds.  xy is the anchors' [n, 2]; ids are below n.  c == 0 or
// W == 0 gives the origin and false: the vertex never moves.
inline bool transform_initial(const float* w, const uint64_t* ids, uint32_t c, const float* xy, float* out_x, float* out_y) {
    *out_x = 0.f;
    *out_y = 0.f;
    if (c == 0) return false;
    float wp[128] = {0.f}, lanes[64], lx[64], ly[64];
    for (uint32_t t = 0; t < c; ++t) wp[t] = w[t];
    for (int l = 0; l < 64; ++l) lanes[l] = wp[l] + wp[l + 64];
    const float W = host_wave_sum64(lanes);
    if (!(W > 0.f)) return false;
    for (uint32_t l = 0; l < 64; ++l) {
        float sx = 0.f, sy = 0.f;
        for (uint32_t t = l; t < c; t += 64u) {
            const float q = wp[t] / W;
            const float px = q * xy[2 * ids[t]];
            const float py = q * xy[2 * ids[t] + 1];
            sx += px;
            sy += py;
        }
        lx[l] = sx;
        ly[l] = sy;
    }
    *out_x = host_wave_sum64(lx);
    *out_y = host_wave_sum64(ly);
    return true;
}

}  // namespace cqs_umap
