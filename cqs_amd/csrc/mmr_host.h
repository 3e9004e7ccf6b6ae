// mmr_host.h — the device-free part of cqs_hip_index_pairwise / cqs_hip_index_mmr: argument checks and the answers that
// need no device work (`mmr_rerank`, src/search/mmr.rs:59-69).  Plain C++ over the caller's arrays, no HIP, no handle:
// mmr.hip and sharded.hip call it under their mutex, tests/mmr_host_driver.cpp runs it under ASAN + UBSan on the CPU.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/cqs_hip.h"

namespace cqs_mmr {

enum class Plan : int32_t {
    Invalid = -1,    // CQS_HIP_ERR_INVALID; *why says which argument
    Empty = 0,       // count 0, CQS_HIP_OK (mmr.rs:64-66)
    Identity = 1,    // picks 0 .. limit-1, CQS_HIP_OK, no device work (mmr.rs:67-69)
    Device = 2,      // the Gram matrix (and the greedy loop) run on the device
};

// The candidate list itself: m within the pool limit, every row inside [row_base, row_base + n).
inline Plan check_rows(const uint64_t* cand_rows, uint32_t m, uint64_t row_base, uint64_t n, const char** why) {
    if (m > CQS_HIP_MMR_MAX) { *why = "pool larger than CQS_HIP_MMR_MAX"; return Plan::Invalid; }
    if (m == 0) return Plan::Empty;
    if (!cand_rows) { *why = "null candidate rows"; return Plan::Invalid; }
    for (uint32_t i = 0; i < m; ++i)
        if (cand_rows[i] < row_base || cand_rows[i] - row_base >= n) { *why = "candidate row not in this index"; return Plan::Invalid; }
    return Plan::Device;
}

// cqs_hip_index_mmr.  *limit / *lambda come back as the loop uses them: lambda.clamp(0, 1) (mmr.rs:60), limit.min(n) (:62).
// Stated departure from mmr.rs: a non-finite lambda or candidate score is refused (the reference's env parser refuses the
// former, mmr.rs:166-178; no search of this library emits the latter).  Arguments are checked before the early answers,
// so a bad list is refused whatever limit and lambda say.
inline Plan plan_mmr(const uint64_t* cand_rows, const float* cand_scores, uint32_t m, uint64_t row_base, uint64_t n,
                     uint32_t* limit, float* lambda, const char** why) {
    if (!std::isfinite(*lambda)) { *why = "non-finite lambda"; return Plan::Invalid; }
    const Plan rows = check_rows(cand_rows, m, row_base, n, why);
    if (rows == Plan::Invalid) return rows;
    if (m && !cand_scores) { *why = "null candidate scores"; return Plan::Invalid; }
    for (uint32_t i = 0; i < m; ++i)
        if (!std::isfinite(cand_scores[i])) { *why = "non-finite candidate score"; return Plan::Invalid; }
    *lambda = *lambda < 0.f ? 0.f : (*lambda > 1.f ? 1.f : *lambda);   // mmr.rs:60
    if (*limit > m) *limit = m;                                        // mmr.rs:62
    if (*limit == 0) return Plan::Empty;                               // mmr.rs:64-66 (m == 0 lands here too)
    if (*lambda >= 1.f || m <= *limit) return Plan::Identity;          // mmr.rs:67-69
    return Plan::Device;
}

}  // namespace cqs_mmr
