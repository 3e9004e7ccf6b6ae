// scan_bf16.h — the bf16 shadow of a dense index: build, scan, rescore + certify (scan_bf16.hip), and the host-side
// arithmetic of its error bound (header-only, so a CPU test can check it).  Internal to libcqs_hip.so.
//
// A search over the shadow is exact: the approximate scan picks k' + 1 candidates, their f32 rows are rescored with the
// f32 gemv kernel's own arithmetic, and the answer is kept only when no row outside the first k' candidates can enter
// the top k.  Otherwise the query is re-run on the f32 scan: by the host (host searches) or by the gated
// f32 launches that follow on the same stream (cqs_hip_index_search_device).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "scan_kernels.h"
#define CQS_HD __host__ __device__
#else
#define CQS_HD
#endif

namespace cqs {

constexpr uint32_t kShadowMaxQ = 32;         // queries per shadow block (the combining queue's block cap)
constexpr uint32_t kShadowMaxDim = 2048;     // (bf16 chunk = 512 components: up to 4 chunks per row)
constexpr uint32_t kShadowKMax = 1024;       // = kMaxK (scan_kernels.h; checked in scan_bf16.hip)

// Candidates rescored from the f32 rows for a top-k search: k' = min(2k + 32, kMaxK - 1); the select then returns k' + 1
// approximate keys (<= kMaxK).  k' < k (only k = kMaxK) means the shadow cannot answer and the f32 scan runs.
inline uint32_t shadow_kprime(uint32_t k) {
    const uint32_t kp = 2u * k + 32u;
    return kp < kShadowKMax - 1u ? kp : kShadowKMax - 1u;
}

// Relative f32 error of a `dim`-term dot product computed by FMA chains and a butterfly whose longest path rounds at most
// dim times: gamma_dim = dim u / (1 - dim u), u = 2^-24 (IEEE fma and add, subnormals kept).
CQS_HD inline double shadow_gamma(uint32_t dim) {
    const double du = (double)dim * 0x1p-24;
    return du / (1.0 - du);
}

// Smallest f32 >= v (v >= 0, finite; +inf if v is past the f32 range).
CQS_HD inline float round_up_f32(double v) {
    float f = (float)v;   // (f64 -> f32 conversion rounds to nearest on host and device alike)
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

// Per-query bound B_q = ||q||_2 * R (plus an absolute term for underflow in the dim roundings of either chain), rounded
// up, so that |s - s~| <= B_q for every finite row.  q_norm2 = sum of q_i^2 in f64.  +inf (no certificate for this
// query) when ||q|| * max(||x||, ||x~||) could reach the f32 overflow range, where one path could overflow and the other not.
// One definition for both sides: the device computes q_norm2 as its own f64 sum (shadow_bound_kernel), in another order
// than a host loop.  Each of the <= 2048 f64 additions errs by at most 2^-53 relative, so any summation order lands within
// 2048 * 2^-53 = 2^-42 of the exact sum of squares (all terms >= 0), and the sqrt halves that: the 2^-40 factor on ||q||
// covers it with room to spare, whoever summed.
CQS_HD inline float shadow_query_bound(double q_norm2, double r_max, double norm_max, uint32_t dim) {
    const double qn = sqrt(q_norm2) * (1.0 + 0x1p-40);            // f64 sum + sqrt: relative error far below 2^-40
    if (!(qn * norm_max * (1.0 + shadow_gamma(dim)) < 0x1p100)) return INFINITY;
    return round_up_f32(qn * r_max * (1.0 + 0x1p-40) + (double)dim * 0x1p-140);
}

#if defined(__HIPCC__)
// ||q||^2 of one query as one wave sums it, in every lane: lane l adds the squares of components l, l + 64, ... in f64 (each
// square is exact), then an xor butterfly 32 -> 1.  One definition for the stand-alone bound kernels and the fused
// rescore + certify kernel, so that B_q has the same bits whoever computes it.
__device__ __forceinline__ double wave_q_norm2(const float* qp, uint32_t dim, uint32_t lane) {
    double s2 = 0.0;
    for (uint32_t d = lane; d < dim; d += 64u) s2 += (double)qp[d] * (double)qp[d];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s2 += __shfl_xor(s2, m, 64);
    return s2;
}
// B_q of the bf16 copy from one wave (the value is meant for lane 0; NaN / inf in q: +inf).
__device__ __forceinline__ float wave_shadow_bound(const float* qp, uint32_t dim, double r_max, double norm_max, uint32_t lane) {
    return shadow_query_bound(wave_q_norm2(qp, dim, lane), r_max, norm_max, dim);
}

// Build: one pass over rows [row0, row0 + rows) of the f32 corpus -> bf16 rows (round to nearest even, NaN stays NaN),
// and over the rows whose components are all finite the maxima of r = ||x - x~|| + gamma (||x|| + ||x~||) and of
// max(||x||, ||x~||), as f64 bits (both >= 0, so the bits order like the values).  stats[0] / stats[1] must be zero (or
// hold the maxima of earlier rows) on entry; stats[2] |= 1 if a finite row has a component with |x_i| >= 2^64.
hipError_t launch_shadow_build(const float* rows, uint16_t* shadow, uint64_t row0, uint64_t n_rows, uint32_t dim,
                               double gamma, unsigned long long* stats, hipStream_t st);

// bq[i] = shadow_query_bound(||q_i||^2 in f64, r_max, norm_max, dim) for the b queries q [b, dim] (device): one wave per
// query.  A non-finite query gets +inf (no certificate).
hipError_t launch_shadow_bound(const float* q, uint32_t b, uint32_t dim, double r_max, double norm_max, float* bq,
                               hipStream_t st);

// Approximate scan of the shadow: the scores / gmax / gaux layout of launch_scan (gemv passes of <= 8 queries), so the
// select's unchanged body (inside launch_rescore_certify's kernel) picks each query's top k' + 1.  a.rows is ignored; bq: device [a.b], B_q of each query
// (a.b <= kShadowMaxQ), read by the PIPELINE drop rule only.
hipError_t launch_scan_bf16(const ScanArgs& a, const uint16_t* shadow, const float* bq, hipStream_t st);

// One launch for the tail of a shadow search (rescore_certify_kernel), after the shadow scan `a` describes (launch_scan_bf16 /
// launch_scan_i8 with these very arguments: a.k = k' + 1, a.rows = the f32 rows).  Select each query's top k' + 1 approximate
// keys from the scan's scores / gmax / gaux (select_finish_kernel's body, run by every workgroup of the query for itself),
// rescore the first min(count, k') from the f32 rows (the gemv kernel's arithmetic and epilogue), take the top k by the
// select's rank sort, write out_keys [b, k] / out_counts [b] as launch_select does, and cert[b] = 1 when that answer is
// provably the f32 scan's (else the caller re-runs the query on the f32 scan).  cert is written before the kernel ends.
// Leaves the work-queue heads (a.work) zeroed for the next scan, as launch_select does.  ekeys: [b, k'] scratch.
// bound: 1 / 2 = compute B_q of the bf16 / int8 copy here (launch_shadow_bound's / launch_i8_bound's bits, from r_max and
// norm_max) into bq [b]; 0 = bq already holds it (a launch_*_bound earlier on st: PIPELINE searches, whose scan reads it).
// tickets: device [b], zero on entry (once, at allocation) and left zero: the workgroups of a query count their arrivals
// there, and the last one certifies.
// counters, counters2: nullable device [2] each: += certified, += not certified queries of the block (device-API searches,
// whose outcome the host never sees; the second pair counts what the int8 copy served).
// prefix: the finisher sorts the first tail_prefix_first candidates' keys and certifies on them where it can (tail_prefix.h);
// false: it sorts all at once.  Same outputs either way.  prefix_counts: nullable device [2], += queries certified on the prefix,
// += queries whose prefix failed and that went on.  prefix_first: where the copy's k' leaves room for a proper prefix, the query's
// workgroups select and rescore that prefix alone, and the finisher does the rest by itself if the prefix does not certify
// (tail_plan.h); same outputs, verdicts and counts either way.  dbg: nullable device [16 + 2 * kDbgWaves + 3]
// (CQS_HIP_DEBUG_STAMPS), phase stamps of query 0's tail.
constexpr uint32_t kDbgTailSlow = 16u + 2u * kDbgWaves;   // the slow path's stamps: behind the f32 scan's per-wave ones (scan_kernels.h)
constexpr uint32_t kDbgTailSlowWords = 3u;
hipError_t launch_rescore_certify(const ScanArgs& a, uint32_t row_base, uint32_t k, uint32_t kprime, uint32_t bound,
                                  double r_max, double norm_max, float* bq, uint32_t* tickets, uint64_t* ekeys,
                                  uint64_t* out_keys, uint32_t* out_counts, uint32_t* cert, unsigned long long* counters,
                                  unsigned long long* counters2, bool prefix, bool prefix_first, unsigned long long* prefix_counts,
                                  unsigned long long* dbg, hipStream_t st);
#endif

}  // namespace cqs
