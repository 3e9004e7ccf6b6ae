// update_host.h — the device-free part of cqs_hip_index_update: the id list checked (range, duplicates), the local rows,
// the order in which the list is staged (ascending by destination row, so the scatter's writes walk the corpus forward),
// and that order cut into passes that fit the staging buffer.  Plain C++ over the caller's arrays, no
// HIP, no handle: index_update.hip calls it under the handle's mutex, tests/update_host_driver.cpp runs it under ASAN +
// UBSan on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace cqs_update {

// The staging buffer's byte budget: one pass stages at most this many bytes (its rows as f32 and one u32 destination
// each), once in pinned host memory and once on the device.  A memory bound, not a tuned number: it is what the handle
// may keep allocated between calls (it keeps what its largest update needed, never more than this), the same 64 MiB that
// remove's bounce buffer is allowed.  10 000 rows of 768 f32 (the reference's enrichment pass "10 k to 50 k rows" in
// batches) are 29 MiB: one pass.
constexpr uint64_t kStageBytes = 64ull << 20;

// Rows per pass of an index of `dim` components under the byte budget (>= 1: one row of <= 4096 f32 always fits).
inline uint64_t budget_rows(uint32_t dim) {
    const uint64_t r = kStageBytes / ((uint64_t)dim * sizeof(float) + sizeof(uint32_t));
    return r ? r : 1;
}

// One trip through the staging buffer: entries order[first, first + count) of the plan.
struct Pass { size_t first, count; };

enum class Plan : int32_t {
    Invalid = -1,   // CQS_HIP_ERR_INVALID; *why says which argument; nothing planned
    Nothing = 0,    // m == 0: CQS_HIP_OK, the index stays as it is
    Update = 1,     // vectors[order[j]] goes to local row local[order[j]], j ascending
};

// cqs_hip_index_update's arguments.  `rows` are global ids in [row_base, row_base + n), in any order, each at most once
// (the reference stages its updates under a primary key: a duplicate fails the statement, and here it would let two
// waves write one row).  *local: rows[i] - row_base per list entry (n + row_base < 2^32: create / extend keep it so).
// *order: the list positions 0 .. m - 1, ascending by local row.
inline Plan plan_update(const uint64_t* rows, const float* vectors, uint64_t m, uint64_t row_base, uint64_t n,
                        std::vector<uint32_t>* local, std::vector<uint64_t>* order, const char** why) {
    local->clear();
    order->clear();
    if (m == 0) return Plan::Nothing;
    if (!rows) { *why = "null rows"; return Plan::Invalid; }
    if (!vectors) { *why = "null vectors"; return Plan::Invalid; }
    for (uint64_t i = 0; i < m; ++i)
        if (rows[i] < row_base || rows[i] - row_base >= n) { *why = "row id not in this index"; return Plan::Invalid; }
    if (m > n) { *why = "row id named twice"; return Plan::Invalid; }   // (pigeonhole; nothing of size m is allocated)
    local->resize(m);
    for (uint64_t i = 0; i < m; ++i) (*local)[i] = (uint32_t)(rows[i] - row_base);
    order->resize(m);
    std::iota(order->begin(), order->end(), (uint64_t)0);
    const uint32_t* l = local->data();
    std::sort(order->begin(), order->end(), [l](uint64_t a, uint64_t b) { return l[a] < l[b]; });
    for (uint64_t j = 1; j < m; ++j)
        if (l[(*order)[j]] == l[(*order)[j - 1]]) {
            local->clear();
            order->clear();
            *why = "row id named twice";
            return Plan::Invalid;
        }
    return Plan::Update;
}

// The m planned entries, in order, in passes of at most budget (>= 1) entries.
inline std::vector<Pass> cut_passes(uint64_t m, uint64_t budget) {
    std::vector<Pass> passes;
    if (budget == 0) budget = 1;
    for (uint64_t first = 0; first < m; first += budget)
        passes.push_back(Pass{(size_t)first, (size_t)std::min(budget, m - first)});
    return passes;
}

// The planned entries whose local row lies in [lo, hi): a contiguous range [*first, *first + count) of `order` (a shard's
// part of a row-sharded handle's update).
inline size_t entries_in(const std::vector<uint32_t>& local, const std::vector<uint64_t>& order, uint64_t lo, uint64_t hi,
                         size_t* first) {
    const auto below = [&local](uint64_t entry, uint64_t row) { return (uint64_t)local[entry] < row; };
    const auto a = std::lower_bound(order.begin(), order.end(), lo, below);
    const auto b = std::lower_bound(a, order.end(), hi, below);
    *first = (size_t)(a - order.begin());
    return (size_t)(b - a);
}

}  // namespace cqs_update
