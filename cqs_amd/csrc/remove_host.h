// remove_host.h — the device-free part of cqs_hip_index_remove: the id list checked, sorted and deduplicated, the surviving
// rows as runs, and the runs cut into passes that fit a bounce buffer.  Plain C++ over the caller's
// array, no HIP, no handle: index_remove.hip calls it under the handle's mutex, tests/remove_host_driver.cpp runs it under
// ASAN + UBSan on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cqs_remove {

// `rows` surviving rows that sit at local rows [src, src + rows) and belong at [dst, dst + rows); dst < src.
struct Run { uint64_t src, dst, rows; };
// One trip through the bounce buffer: destination rows [dst, dst + rows), whose sources runs [run_first, run_first +
// run_count) hold (the first and the last of them perhaps only in part: a pass boundary may cut a run).
struct Pass { uint64_t dst, rows; size_t run_first, run_count; };

enum class Plan : int32_t {
    Invalid = -1,   // CQS_HIP_ERR_INVALID; *why says which argument; nothing planned
    Nothing = 0,    // m == 0: CQS_HIP_OK, the index stays as it is
    Remove = 1,     // `removed` rows go; `runs` move (none: the removed rows are the index's last)
};

// cqs_hip_index_remove's arguments.  `rows` are global ids in [row_base, row_base + n), in any order, duplicates allowed.
// *removed: the distinct local rows, ascending.  *runs: the surviving rows ABOVE the first removed row, ascending (the rows
// below it stay where they are and are not named); consecutive runs' destinations are consecutive, the first run's
// destination is the first removed row, the last run ends at row n - removed->size().
inline Plan plan_remove(const uint64_t* rows, uint64_t m, uint64_t row_base, uint64_t n, std::vector<uint64_t>* removed,
                        std::vector<Run>* runs, const char** why) {
    removed->clear();
    runs->clear();
    if (m == 0) return Plan::Nothing;
    if (!rows) { *why = "null rows"; return Plan::Invalid; }
    for (uint64_t i = 0; i < m; ++i)
        if (rows[i] < row_base || rows[i] - row_base >= n) { *why = "row id not in this index"; return Plan::Invalid; }
    removed->reserve(m);
    for (uint64_t i = 0; i < m; ++i) removed->push_back(rows[i] - row_base);
    std::sort(removed->begin(), removed->end());
    removed->erase(std::unique(removed->begin(), removed->end()), removed->end());
    uint64_t dst = (*removed)[0];
    for (size_t i = 0; i < removed->size(); ++i) {
        const uint64_t src = (*removed)[i] + 1;                                        // the rows between this removed row
        const uint64_t end = i + 1 < removed->size() ? (*removed)[i + 1] : n;          // and the next one (or the end)
        if (end > src) { runs->push_back(Run{src, dst, end - src}); dst += end - src; }
    }
    return Plan::Remove;
}

// The runs' destination rows, in order, in passes of at most budget_rows rows (>= 1).  Why a pass may write its
// destination once its sources are in the bounce buffer: every planned row has src > dst and src grows with dst, so the
// pass's destination [dst, dst + rows) ends at or below the end of its own source range, and every later pass's sources
// lie above that end (pass_overlap_ok states both, tests/remove_host_driver.cpp checks them for every pass).
inline std::vector<Pass> cut_passes(const std::vector<Run>& runs, uint64_t budget_rows) {
    std::vector<Pass> passes;
    if (budget_rows == 0) budget_rows = 1;
    size_t r = 0;            // the run the next pass starts in
    uint64_t used = 0;       // ... and how many of its rows earlier passes took
    while (r < runs.size()) {
        Pass p{runs[r].dst + used, 0, r, 0};
        while (r < runs.size() && p.rows < budget_rows) {
            const uint64_t take = std::min(runs[r].rows - used, budget_rows - p.rows);
            p.rows += take;
            used += take;
            ++p.run_count;
            if (used == runs[r].rows) { ++r; used = 0; }
        }
        passes.push_back(p);
    }
    return passes;
}

// The row that belongs at destination row d (inside the runs' destinations): what the device's lookup computes.
inline uint64_t source_of(const std::vector<Run>& runs, uint64_t d) {
    size_t lo = 0, hi = runs.size();   // runs[lo].dst <= d < runs[hi].dst (hi == size: the end)
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (runs[mid].dst <= d) lo = mid; else hi = mid;
    }
    return runs[lo].src + (d - runs[lo].dst);
}

// The two facts the in-place compaction rests on, for pass i: its destination ends at or below the end of its sources, and
// the first source of the next pass lies at or above that destination's end.
inline bool pass_overlap_ok(const std::vector<Run>& runs, const std::vector<Pass>& passes, size_t i) {
    const Pass& p = passes[i];
    if (p.rows == 0) return false;
    const uint64_t dst_end = p.dst + p.rows;
    const uint64_t src_end = source_of(runs, dst_end - 1) + 1;
    if (dst_end > src_end || source_of(runs, p.dst) <= p.dst) return false;
    return i + 1 == passes.size() || source_of(runs, passes[i + 1].dst) >= dst_end;
}

}  // namespace cqs_remove
