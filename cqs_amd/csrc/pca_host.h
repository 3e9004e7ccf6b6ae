// pca_host.h — the device-free part of cqs_hip_index_pca / cqs_hip_index_pca_project and of the PCA initial coordinates of
// cqs_hip_index_umap_project_init (include/cqs_hip.h "PCA of the stored rows"): the argument plans with
// their refusals in the documented order, the constants the kernels share with the host (the slab, the block width), the
// start matrix, Gram-Schmidt with its breakdown rule, the 8 x 8 Jacobi eigen-solve, the sign rule, one host step of the
// subspace iteration, and umap-learn's noisy_scale_coords.  Plain C++ over the caller's arrays, no HIP, no handle:
// index_pca.hip calls all of it between its launches, and tests/pca_host_driver.cpp runs it under ASAN + UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "umap_host.h"

namespace cqs_pca {

constexpr uint32_t kBlock = 8;            // p: columns of the iterated block (the device always carries 8; dim < 8 zeroes the rest)
constexpr uint32_t kSlabRows = 1024;      // rows of one slab = one partial [dim x 8] + [8] of a pass
constexpr uint32_t kBatchRows = 16;       // rows a workgroup holds on chip at once (one MFMA tile's M / K)
constexpr uint32_t kTileDims = 1024;      // columns of the corpus one workgroup accumulates (dim > 1024: several workgroups a slab)
constexpr uint32_t kDefaultPasses = 16;
constexpr uint32_t kMaxPasses = 64;
constexpr uint64_t kProjectRowsPerLaunch = (uint64_t)CQS_HIP_KNN_MAX_TARGETS * 16u;

inline uint64_t slabs_of(uint64_t n) { return (n + kSlabRows - 1) / kSlabRows; }

// What the calls see of their handle (all zero beside a null one).
struct Handle {
    bool present;
    bool sharded;
    uint64_t row_base;
    uint64_t len;
    uint32_t dim;
};

struct Planned {
    uint32_t p;         // min(kBlock, dim)
    uint32_t passes;    // n_passes, or kDefaultPasses where that is 0
};

// cqs_hip_index_pca's arguments, refused in the documented order: a null handle; a null output; n_components == 0,
// > CQS_HIP_PCA_MAX_COMPONENTS or > dim; n_passes > 64; a row-sharded handle; fewer than 2 rows.
inline bool plan_pca(const Handle& h, uint32_t n_components, uint32_t n_passes, bool outputs, Planned* out, const char** why) {
    *out = Planned{0, 0};
    *why = "";
    if (!h.present) { *why = "pca: null handle"; return false; }
    if (!outputs) { *why = "pca: null output buffer"; return false; }
    if (n_components == 0 || n_components > CQS_HIP_PCA_MAX_COMPONENTS || n_components > h.dim) {
        *why = "pca: n_components not in [1, min(CQS_HIP_PCA_MAX_COMPONENTS, dim)]";
        return false;
    }
    if (n_passes > kMaxPasses) { *why = "pca: more than 64 passes"; return false; }
    if (h.sharded) { *why = "pca: not built for a row-sharded handle"; return false; }
    if (h.len < 2) { *why = "pca: fewer than 2 rows"; return false; }
    out->p = h.dim < kBlock ? h.dim : kBlock;
    out->passes = n_passes ? n_passes : kDefaultPasses;
    return true;
}

enum class Plan : int32_t { Invalid = -1, Nothing = 0, Run = 1 };

// cqs_hip_index_pca_project's arguments, in the documented order: a null handle; (m == 0: OK, nothing touched;) a null
// mean, axes or output; n_components == 0, > CQS_HIP_PCA_MAX_COMPONENTS or > dim; a row-sharded handle; any part of the
// range outside the index.  *local_first = first_row - row_base.
inline Plan plan_project(const Handle& h, bool mean_axes, bool output, uint32_t n_components, uint64_t first_row, uint64_t m,
                         uint64_t* local_first, const char** why) {
    *local_first = 0;
    *why = "";
    if (!h.present) { *why = "pca_project: null handle"; return Plan::Invalid; }
    if (m == 0) return Plan::Nothing;
    if (!mean_axes) { *why = "pca_project: null mean or axes"; return Plan::Invalid; }
    if (!output) { *why = "pca_project: null output buffer"; return Plan::Invalid; }
    if (n_components == 0 || n_components > CQS_HIP_PCA_MAX_COMPONENTS || n_components > h.dim) {
        *why = "pca_project: n_components not in [1, min(CQS_HIP_PCA_MAX_COMPONENTS, dim)]";
        return Plan::Invalid;
    }
    if (h.sharded) { *why = "pca_project: not built for a row-sharded handle"; return Plan::Invalid; }
    if (first_row < h.row_base || first_row - h.row_base >= h.len || m > h.len - (first_row - h.row_base)) {
        *why = "pca_project: range not in this index";
        return Plan::Invalid;
    }
    *local_first = first_row - h.row_base;
    return Plan::Run;
}

// ---- the start matrix ----------------------------------------------------------------------------------------------------
// V0[d][j] = float(hash(seed, 0, d, 2, j) >> 8) * 2^-23 - 1: uniform in [-1, 1), every step exact in f32.
inline float start_entry(uint64_t seed, uint32_t d, uint32_t j) {
    const float u = (float)(cqs_umap::hash5(seed, 0u, d, 2u, j) >> 8);
    const float scaled = u * (1.0f / 8388608.0f);
    return scaled - 1.0f;
}

// ---- Gram-Schmidt ----------------------------------------------------------------------------------------------------------
// a is [dim][kBlock] row-major f64; columns 0 .. p-1 are orthonormalised in column order, columns p .. 7 are zeroed.
// Column j: subtract its components along columns 0 .. j-1 one after the other (modified Gram-Schmidt), twice, then
// divide by its norm.  Breakdown: where the column's norm before is 0 or not finite, or its norm after is not greater than
// 1e-10 times the norm before (it lay in the span of the earlier columns), the column is replaced by the first unit basis
// vector e_d, d ascending, whose residual against the earlier columns has a squared norm of at least 1 / (2 dim) - one
// exists, the squared residuals of all dim unit vectors add up to dim - j - and that residual is normalised instead.
// Returns the number of columns replaced.
inline uint32_t gram_schmidt(double* a, uint32_t dim, uint32_t p) {
    uint32_t replaced = 0;
    const auto norm_of = [&](uint32_t j) {
        double s = 0.0;
        for (uint32_t d = 0; d < dim; ++d) s += a[(size_t)d * kBlock + j] * a[(size_t)d * kBlock + j];
        return std::sqrt(s);
    };
    const auto project_out = [&](uint32_t j) {
        for (int round = 0; round < 2; ++round)
            for (uint32_t i = 0; i < j; ++i) {
                double dot = 0.0;
                for (uint32_t d = 0; d < dim; ++d) dot += a[(size_t)d * kBlock + i] * a[(size_t)d * kBlock + j];
                for (uint32_t d = 0; d < dim; ++d) a[(size_t)d * kBlock + j] -= dot * a[(size_t)d * kBlock + i];
            }
    };
    for (uint32_t j = 0; j < p; ++j) {
        const double before = norm_of(j);
        double after = 0.0;
        bool ok = std::isfinite(before) && before > 0.0;
        if (ok) {
            project_out(j);
            after = norm_of(j);
            ok = std::isfinite(after) && after > 1e-10 * before;
        }
        if (!ok) {
            ++replaced;
            for (uint32_t e = 0; e < dim; ++e) {
                for (uint32_t d = 0; d < dim; ++d) a[(size_t)d * kBlock + j] = d == e ? 1.0 : 0.0;
                project_out(j);
                after = norm_of(j);
                if (after * after >= 1.0 / (2.0 * dim)) break;
            }
        }
        for (uint32_t d = 0; d < dim; ++d) a[(size_t)d * kBlock + j] /= after;
    }
    for (uint32_t j = p; j < kBlock; ++j)
        for (uint32_t d = 0; d < dim; ++d) a[(size_t)d * kBlock + j] = 0.0;
    return replaced;
}

// ---- the small eigen-solve -------------------------------------------------------------------------------------------------
// Cyclic Jacobi on the symmetric p x p matrix h (row-major, stride kBlock; destroyed): eigenvalues descending in lambda,
// the matching eigenvectors in the columns of w (stride kBlock).  Equal eigenvalues keep their order of appearance on the
// diagonal.
inline void jacobi_eigen(double* h, uint32_t p, double* lambda, double* w) {
    for (uint32_t i = 0; i < kBlock; ++i)
        for (uint32_t j = 0; j < kBlock; ++j) w[i * kBlock + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (uint32_t i = 0; i < p; ++i)
            for (uint32_t j = 0; j < p; ++j) (i == j ? diag : off) += h[i * kBlock + j] * h[i * kBlock + j];
        if (!(off > 1e-40 * diag)) break;   // (also leaves on a NaN)
        for (uint32_t a = 0; a + 1 < p; ++a)
            for (uint32_t b = a + 1; b < p; ++b) {
                const double apq = h[a * kBlock + b];
                if (apq == 0.0) continue;
                const double theta = (h[b * kBlock + b] - h[a * kBlock + a]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (uint32_t k = 0; k < p; ++k) {   // columns a, b
                    const double ka = h[k * kBlock + a], kb = h[k * kBlock + b];
                    h[k * kBlock + a] = c * ka - s * kb;
                    h[k * kBlock + b] = s * ka + c * kb;
                }
                for (uint32_t k = 0; k < p; ++k) {   // rows a, b
                    const double ak = h[a * kBlock + k], bk = h[b * kBlock + k];
                    h[a * kBlock + k] = c * ak - s * bk;
                    h[b * kBlock + k] = s * ak + c * bk;
                }
                for (uint32_t k = 0; k < p; ++k) {
                    const double ka = w[k * kBlock + a], kb = w[k * kBlock + b];
                    w[k * kBlock + a] = c * ka - s * kb;
                    w[k * kBlock + b] = s * ka + c * kb;
                }
            }
    }
    uint32_t order[kBlock];
    for (uint32_t i = 0; i < p; ++i) order[i] = i;
    for (uint32_t i = 1; i < p; ++i)       // stable insertion sort, descending
        for (uint32_t j = i; j > 0 && h[order[j] * kBlock + order[j]] > h[order[j - 1] * kBlock + order[j - 1]]; --j) {
            const uint32_t t = order[j]; order[j] = order[j - 1]; order[j - 1] = t;
        }
    double sorted[kBlock * kBlock];
    for (uint32_t c = 0; c < p; ++c) {
        lambda[c] = h[order[c] * kBlock + order[c]];
        for (uint32_t k = 0; k < p; ++k) sorted[k * kBlock + c] = w[k * kBlock + order[c]];
    }
    for (uint32_t c = 0; c < p; ++c)
        for (uint32_t k = 0; k < p; ++k) w[k * kBlock + c] = sorted[k * kBlock + c];
}

// The sign rule on an f32 axis: its component of largest magnitude is positive, the lowest index on ties.
inline void fix_sign(float* axis, uint32_t dim) {
    uint32_t at = 0;
    for (uint32_t d = 1; d < dim; ++d)
        if (std::fabs(axis[d]) > std::fabs(axis[at])) at = d;
    if (axis[at] < 0.f)
        for (uint32_t d = 0; d < dim; ++d) axis[d] = -axis[d];
}

// ---- the host steps of the iteration -------------------------------------------------------------------------------------
// The start block: V0 orthonormalised.  v is [dim][kBlock] f64.
inline void start_block(uint64_t seed, uint32_t dim, uint32_t p, double* v) {
    for (uint32_t d = 0; d < dim; ++d)
        for (uint32_t j = 0; j < kBlock; ++j) v[(size_t)d * kBlock + j] = j < p ? (double)start_entry(seed, d, j) : 0.0;
    gram_schmidt(v, dim, p);
}

// What a pass hands the device: V rounded to f32, and c[j] = the shifted mean's component along column j, negated (the
// MFMA chain of t starts from it).  shift_mean is mu - x_0 in f64.
inline void device_block(const double* v, const double* shift_mean, uint32_t dim, float* v32, float* neg_c) {
    for (size_t i = 0; i < (size_t)dim * kBlock; ++i) v32[i] = (float)v[i];
    for (uint32_t j = 0; j < kBlock; ++j) {
        double s = 0.0;
        for (uint32_t d = 0; d < dim; ++d) s += shift_mean[d] * (double)v32[(size_t)d * kBlock + j];
        neg_c[j] = (float)-s;
    }
}

// Z^T Z V from a pass's sums: y [dim][kBlock] (in place) and s [kBlock], both over the shifted rows x - x_0.
inline void centre_pass(double* y, const double* s, const double* shift_mean, uint32_t dim) {
    for (uint32_t d = 0; d < dim; ++d)
        for (uint32_t j = 0; j < kBlock; ++j) y[(size_t)d * kBlock + j] -= shift_mean[d] * s[j];
}

// The last step: H = V^T Y symmetrised, its eigenvectors W, axes = V W (the first n_components columns, f32, sign rule),
// variance[k] = lambda_k / (n - 1).  False: an entry of H or one of the p Rayleigh values is not finite
// (nothing is written).
inline bool finish(const double* v, const double* y, uint32_t dim, uint32_t p, uint64_t n, uint32_t n_components, float* axes,
                   float* variance) {
    double h[kBlock * kBlock] = {0}, lambda[kBlock] = {0}, w[kBlock * kBlock];
    for (uint32_t i = 0; i < p; ++i)
        for (uint32_t j = 0; j < p; ++j) {
            double s = 0.0;
            for (uint32_t d = 0; d < dim; ++d) s += v[(size_t)d * kBlock + i] * y[(size_t)d * kBlock + j];
            h[i * kBlock + j] = s;
        }
    for (uint32_t i = 0; i < p; ++i)
        for (uint32_t j = i + 1; j < p; ++j) h[i * kBlock + j] = h[j * kBlock + i] = 0.5 * (h[i * kBlock + j] + h[j * kBlock + i]);
    for (uint32_t i = 0; i < p; ++i)       // (Jacobi leaves a NaN where it finds it: every entry is asked, not the leading ones)
        for (uint32_t j = 0; j < p; ++j)
            if (!std::isfinite(h[i * kBlock + j])) return false;
    jacobi_eigen(h, p, lambda, w);
    for (uint32_t k = 0; k < p; ++k)
        if (!std::isfinite((float)(lambda[k] / (double)(n - 1)))) return false;   // (as the f32 it is returned in)
    for (uint32_t k = 0; k < n_components; ++k) {
        for (uint32_t d = 0; d < dim; ++d) {
            double s = 0.0;
            for (uint32_t j = 0; j < p; ++j) s += v[(size_t)d * kBlock + j] * w[j * kBlock + k];
            axes[(size_t)k * dim + d] = (float)s;
        }
        fix_sign(axes + (size_t)k * dim, dim);
        variance[k] = (float)(lambda[k] / (double)(n - 1));
    }
    return true;
}

// ---- umap-learn's noisy_scale_coords ---------------------------------------------------------------------------------------
// jitter of coordinate c of vertex i: (float(hash(seed, 0, i, 1, c) >> 8) * 2^-24 - 0.5) * 2e-4, each step rounded once
inline float jitter(uint64_t seed, uint32_t vertex, uint32_t c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float u = (float)(cqs_umap::hash5(seed, 0u, vertex, 1u, c) >> 8);
    const float unit = u * (1.0f / 16777216.0f);
    const float centred = unit - 0.5f;
    return centred * 2e-4f;
}

// proj [n][nc] (nc = 1 or 2) -> xy [n][2]: coord = proj * (10 / max|proj|) + jitter in f32, the quotient, the product and
// the sum each rounded once; a missing second coordinate counts as 0.  False (xy untouched): max|proj| is 0 or not finite,
// or so small that the quotient overflows - the caller keeps the hashed uniform coordinates.
inline bool noisy_scale_coords(const float* proj, uint64_t n, uint32_t nc, uint64_t seed, float* xy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float top = 0.f;
    for (uint64_t i = 0; i < n * nc; ++i) {
        const float a = std::fabs(proj[i]);
        if (!std::isfinite(a)) return false;
        if (a > top) top = a;
    }
    if (!(top > 0.f)) return false;
    const float scale = 10.0f / top;
    if (!std::isfinite(scale)) return false;   // (a denormal maximum)
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t c = 0; c < 2u; ++c) {
            const float scaled = (c < nc ? proj[i * nc + c] : 0.f) * scale;
            xy[2 * i + c] = scaled + jitter(seed, (uint32_t)i, c);
        }
    return true;
}

}  // namespace cqs_pca
