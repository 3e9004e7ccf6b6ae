// search_host.h — the device-free rules of the host search path, once: the argument plan of cqs_hip_index_search /
// cqs_hip_index_search_filtered, the kept-row count of a bitset and k_eff, query staging, neighbours' clamp and
// self-exclusion, the packed-key helpers.  Plain C++ over the caller's arrays, no HIP, no handle: index.hip, index_combine.hip
// and sharded.hip call it under their mutexes, tests/search_host_driver.cpp runs it under ASAN + UBSan on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/cqs_hip.h"

namespace cqs_search {

enum class Plan : int32_t {
    Invalid = -1,    // CQS_HIP_ERR_INVALID; *why is the message
    Empty = 0,       // CQS_HIP_OK, every count 0 (b == 0: nothing touched); a non-empty *why goes to last_error as it is
    Run = 1,         // arguments in order, counts zeroed: there is device work
};

// The arguments of one host search call.  keep_bitsets / keep_stride_words: the filtered variant's (`filtered` set).
struct Args {
    const float* queries;
    uint32_t b, query_dim, k, mode;
    uint64_t* out_rows;
    float* out_scores;
    uint32_t* out_counts;
    bool filtered = false;
    const uint32_t* keep_bitsets = nullptr;
    uint64_t keep_stride_words = 0;
};

// The checks and early answers of `search_impl` (src/cagra.rs:445-470) in the order the entry points have always made
// them, over an index of n rows of `dim` floats.  The poisoned check and the mutex stay with the caller.
inline Plan plan_search(const Args& a, uint64_t n, uint32_t dim, uint32_t max_k, const char** why) {
    const auto refuse = [&](const char* plain, const char* filtered) { *why = a.filtered ? filtered : plain; return Plan::Invalid; };
    *why = "";
    if (a.b == 0) return Plan::Empty;
    if (!a.queries || !a.out_counts || (a.filtered && !a.keep_bitsets)) return refuse("search: null buffer", "search_filtered: null buffer");
    for (uint32_t i = 0; i < a.b; ++i) a.out_counts[i] = 0;
    if (n == 0 || a.k == 0) return Plan::Empty;                 // src/cagra.rs:445-447
    if (a.query_dim != dim) {                                   // src/cagra.rs:449-456
        *why = "search: query dimension mismatch (empty result)";
        return Plan::Empty;
    }
    if (a.k > max_k) return refuse("search: k > max_k", "search_filtered: k > max_k");
    if (a.mode > CQS_HIP_MODE_PIPELINE) return refuse("search: bad mode", "search_filtered: bad mode");
    if (!a.out_rows || !a.out_scores) return refuse("search: null output buffer", "search_filtered: null output buffer");
    if (a.filtered && a.keep_stride_words < (n + 31) / 32) return refuse("", "search_filtered: bitset stride shorter than the index");
    return Plan::Run;
}

// Set bits among bits [first_bit, first_bit + nbits) of a host bitset (first_bit % 32 == 0; src/cagra.rs:747-775).  Bits of
// the last word past nbits are not rows; a whole number of words reads no word past them.
inline uint64_t popcount_bits(const uint32_t* words, uint64_t first_bit, uint64_t nbits) {
    const uint32_t* w = words + first_bit / 32;
    uint64_t c = 0;
    for (uint64_t i = 0; i < nbits / 32; ++i) c += (uint64_t)__builtin_popcount(w[i]);
    if (nbits % 32) c += (uint64_t)__builtin_popcount(w[nbits / 32] & ((1u << (nbits % 32)) - 1u));
    return c;
}

enum class Keep : int32_t {
    Unfiltered = 0,  // no bitset, or one that keeps every row (src/cagra.rs:760-762)
    Empty = 1,       // nothing kept: every count 0 (:765-767)
    Filtered = 2,    // *k_eff = min(*k_eff, kept rows) (:775)
};

// The whole-handle rule for a nullable bitset over n rows.
inline Keep plan_keep(const uint32_t* keep, uint64_t n, uint32_t* k_eff) {
    if (!keep) return Keep::Unfiltered;
    const uint64_t included = popcount_bits(keep, 0, n);
    if (included == 0) return Keep::Empty;
    if (included >= n) return Keep::Unfiltered;
    if (included < *k_eff) *k_eff = (uint32_t)included;
    return Keep::Filtered;
}

// A query with a non-finite component has an empty result (src/cagra.rs:464-470).
inline bool query_finite(const float* q, uint32_t dim) {
    bool ok = true;
    for (uint32_t d = 0; d < dim; ++d) ok &= std::isfinite(q[d]);
    return ok;
}

// Stage one query: a finite one is copied (true), any other leaves a zero row (false: it has no answer).
inline bool stage_query(float* dst, const float* src, uint32_t dim) {
    const bool ok = query_finite(src, dim);
    if (ok) memcpy(dst, src, (size_t)dim * sizeof(float));
    else memset(dst, 0, (size_t)dim * sizeof(float));
    return ok;
}

// `find_neighbors` (src/cli/commands/search/neighbors.rs:86-132): *limit = limit.clamp(1, SIMILAR_LIMIT_MAX) (:95,
// cli/limits.rs:40); returns the k the scan asks for, limit + 1 cut to the n rows there are - 0 when the target is the only row.
inline uint32_t neighbors_k(uint32_t* limit, uint64_t n) {
    if (*limit < 1u) *limit = 1u;
    if (*limit > CQS_HIP_NEIGHBORS_MAX) *limit = CQS_HIP_NEIGHBORS_MAX;
    if (n <= 1) return 0;
    return (uint64_t)*limit + 1u < n ? *limit + 1u : (uint32_t)n;
}

// The first `limit` of the cnt results that are not the target (neighbors.rs:116-118): top-(limit+1) of all rows minus the
// target = top-limit of all rows but the target under the same total order.  Returns how many were written.
inline uint32_t drop_self(const uint64_t* rows, const float* scores, uint32_t cnt, uint64_t target_row, uint32_t limit,
                          uint64_t* out_rows, float* out_scores) {
    uint32_t outc = 0;
    for (uint32_t i = 0; i < cnt && outc < limit; ++i) {
        if (rows[i] == target_row) continue;
        out_rows[outc] = rows[i];
        out_scores[outc] = scores[i];
        ++outc;
    }
    return outc;
}

// cqs_hip_unpack_keys: key = (order-preserving score bits << 32) | (0xFFFFFFFF - row).  Either output may be null.
inline void unpack_keys(const uint64_t* keys, size_t count, uint64_t* rows, float* scores) {
    for (size_t i = 0; i < count; ++i) {
        const uint32_t ok = (uint32_t)(keys[i] >> 32);
        const uint32_t bits = (ok & 0x80000000u) ? (ok ^ 0x80000000u) : ~ok;
        float f;
        memcpy(&f, &bits, 4);
        if (scores) scores[i] = f;
        if (rows) rows[i] = (uint64_t)(0xFFFFFFFFu - (uint32_t)keys[i]);
    }
}

// cqs_hip_merge_keys: k-way merge of descending lists; n_lists is small (<= #GPUs), so a linear scan over the list heads
// is cheaper than a heap.
inline size_t merge_keys(const uint64_t* lists, const uint32_t* counts, size_t n_lists, size_t stride, size_t k, uint64_t* out_keys) {
    std::vector<size_t> pos(n_lists, 0);
    size_t outc = 0;
    while (outc < k) {
        size_t best = n_lists;
        uint64_t bk = 0;
        for (size_t l = 0; l < n_lists; ++l) {
            if (pos[l] < counts[l]) {
                const uint64_t v = lists[l * stride + pos[l]];
                if (best == n_lists || v > bk) { best = l; bk = v; }
            }
        }
        if (best == n_lists) break;
        out_keys[outc++] = bk;
        pos[best]++;
    }
    return outc;
}

// cqs_hip_index_last_error: the message (len bytes, no terminator needed) cut to the caller's buffer, cap >= 1.
inline size_t copy_last_error(const char* msg, size_t len, char* buf, size_t cap) {
    const size_t m = len < cap - 1 ? len : cap - 1;
    memcpy(buf, msg, m);
    buf[m] = 0;
    return m;
}

}  // namespace cqs_search
