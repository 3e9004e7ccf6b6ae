// scan_i8.h — the int8 copy of the dense index's shadow: build and scan (scan_i8.hip), and the host-side arithmetic of its
// error bound (header-only, so a CPU test can check it).  Internal to libcqs_hip.so.
//
// Layout: [n, dim] int8 codes c plus one f32 scale per row; the row the copy stands for is x~_i = scale * c_i as a real
// number.  A quarter of the f32 bytes.  The scan's candidates go through the bf16 shadow's select, rescore and certify
// (scan_bf16.h) with this copy's own bound and k', so a search stays exact.
#pragma once
#include "scan_bf16.h"

namespace cqs {

constexpr uint32_t kI8MaxQ = 4;   // queries per block the int8 copy serves: a pass carries <= 4 queries (16 f32 query
                                  // registers per query and chunk), so from 5 queries on two int8 passes read what one
                                  // bf16 pass of 8 reads and the bf16 copy keeps the block

// Candidates rescored for a top-k search through the int8 copy.  The bound is about 7x the bf16 one, so the window of rows
// whose approximate score can hide a top-k row is wider: at least 1.5x the largest k' any measured query needed
// (profiles/i8_scan_bench.json).  Past kMaxK - 1 the int8 copy cannot answer and the bf16 copy does.
inline uint32_t i8_kprime(uint32_t k) { return 10u * k + 150u; }
inline bool i8_k_ok(uint32_t k) { return i8_kprime(k) <= kShadowKMax - 1u; }

// The dim rule of the int8 copy: a lane's 16-byte load is 16 components.
inline bool i8_dim_ok(uint32_t dim) { return dim % 16u == 0u && dim <= kShadowMaxDim; }

// Relative error of the int8 scan's score against the real dot product x~ . q.  The kernel converts each code to f32
// (exact: |c| <= 127), runs an (even, odd) FMA chain of 8 per 1024-component chunk, adds the two, a 6-level butterfly, and
// multiplies the sum by the row's scale: the longest path rounds 8 * chunks + 1 + 6 + 1 times, 16 for dim <= 1024 and 24
// beyond, never more than dim + 2 (dim >= 16).  gamma_(dim + 2) also covers the f32 scan's own gamma_dim, so the build
// folds one gamma over ||x|| + ||x~||.
CQS_HD inline double i8_gamma(uint32_t dim) { return shadow_gamma(dim + 2u); }

// Per-query bound of the int8 scan: |s - s~| <= B_q for every finite row, s the f32 scan's score and s~ the int8 scan's.
//   |s - x.q| <= gamma ||x|| ||q||,  |x.q - x~.q| <= ||x - x~|| ||q||,  |x~.q - s~| <= gamma' ||x~|| ||q||
// with r_max >= ||x - x~|| + i8_gamma (||x|| + ||x~||) from the build.  Absolute term: a rounding whose result is
// subnormal errs by <= 2^-150 instead; the <= dim such roundings of the code chain are scaled by the row scale
// <= max|x_i| / 127 * (1 + u) <= norm_max / 64, the f32 chain's <= dim and the final multiply's one are not:
// dim 2^-150 (norm_max / 64 + 1) + 2^-150 <= dim 2^-140 (1 + norm_max).
// +inf (no certificate) where the bf16 bound gives it, and where the unscaled code sum, |sum c_i q_i| <= 127 sqrt(dim) ||q||,
// could leave the f32 range although the scaled score does not.
CQS_HD inline float i8_query_bound(double q_norm2, double r_max, double norm_max, uint32_t dim) {
    const double qn = sqrt(q_norm2) * (1.0 + 0x1p-40);
    if (!(qn * norm_max * (1.0 + i8_gamma(dim)) < 0x1p100)) return INFINITY;
    if (!(qn * 128.0 * sqrt((double)dim) < 0x1p100)) return INFINITY;
    return round_up_f32(qn * r_max * (1.0 + 0x1p-40) + (double)dim * 0x1p-140 * (1.0 + norm_max));
}

#if defined(__HIPCC__)
// B_q of the int8 copy from one wave: wave_shadow_bound with this copy's bound function (same f64 sum of squares, same
// 2^-40 slack for its order).  Shared by i8_bound_kernel and the fused rescore + certify kernel.
__device__ __forceinline__ float wave_i8_bound(const float* qp, uint32_t dim, double r_max, double norm_max, uint32_t lane) {
    return i8_query_bound(wave_q_norm2(qp, dim, lane), r_max, norm_max, dim);
}

// Build: one pass over rows [row0, row0 + rows) of the f32 corpus.  Per row: scale = max|x_i| / 127 in f32 (0 for a row
// whose maximum is zero or underflows: all codes 0; NaN for a row with a non-finite component: its score is non-finite in
// the int8 scan as it is in the f32 one), c_i = round-to-nearest-even(x_i / scale) clamped to [-127, 127].  stats[0..2] as
// launch_shadow_build: maxima over the finite rows of ||x - x~|| + gamma (||x|| + ||x~||) and of max(||x||, ||x~||), f64
// bits, from the stored codes and scale; stats[2] |= 1 for a component of magnitude >= 2^64.
hipError_t launch_i8_build(const float* rows, int8_t* codes, float* scales, uint64_t row0, uint64_t n_rows, uint32_t dim,
                           double gamma, unsigned long long* stats, hipStream_t st);

// bq[i] = i8_query_bound(...) for the b queries: launch_shadow_bound with the int8 copy's function.
hipError_t launch_i8_bound(const float* q, uint32_t b, uint32_t dim, double r_max, double norm_max, float* bq, hipStream_t st);

// Approximate scan of the int8 copy: launch_scan_bf16's contract (scores / gmax / gaux layout, one-sided drop rules with
// this copy's B_q), passes of <= kI8MaxQ queries.
hipError_t launch_scan_i8(const ScanArgs& a, const int8_t* codes, const float* scales, const float* bq, hipStream_t st);
#endif

}  // namespace cqs
