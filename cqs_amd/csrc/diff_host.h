// diff_host.h — the device-free part of cqs_hip_index_diff: the argument plan (the refusals in their order, row_base taken
// off into the u32 rows a pass stages), the cut of the pair list into passes, the rule by which the passes' lists of
// modified pairs concatenate, the lock over two handles, and one pair's arithmetic and the ordered compaction restated on
// host arrays.  Plain C++ over the caller's arrays, no HIP, no handle: index_diff.hip calls it under
// both handles' mutexes and its kernels share finish_pair and the class bits; tests/diff_host_driver.cpp runs it under
// ASAN + UBSan, and its lock under TSan, on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CQS_DIFF_HD __host__ __device__
#else
#define CQS_DIFF_HD
#endif

namespace cqs_diff {

// Pairs per pass: what the staging block is sized for at most (24 bytes a pair, pinned and on the device).  A memory
// bound, not a tuned number.
constexpr uint64_t kPassPairs = 1ull << 20;
// Pairs per tile of the compaction: a tile's modified pairs are counted and written by one workgroup; tiles are fixed by
// the pass alone ([kTile * t, min(kTile * t + kTile, pairs))), so the list does not depend on the grid.
constexpr uint32_t kTile = 1024;

// A pair's class word.
constexpr uint32_t kModified = 1u;    // sim < threshold
constexpr uint32_t kUndefined = 2u;   // full_cosine_similarity gave None: sim is 0.0

enum class Plan : int32_t {
    Invalid = -1,   // CQS_HIP_ERR_INVALID; *why says which refusal; outputs untouched
    Nothing = 0,    // m == 0: CQS_HIP_OK, out_counts = {0, 0, 0} if non-null, nothing else touched
    Run = 1,        // every pair names a stored row on each side
};

// What the call sees of one of its handles (all zero beside a null one).
struct Side {
    bool present;    // a non-null handle
    bool sharded;    // made by cqs_hip_index_create_sharded / _load_sharded
    int32_t device;
    uint32_t dim;
    uint64_t row_base;
    uint64_t len;    // rows stored
};

struct Args {
    const uint64_t* rows_a;
    const uint64_t* rows_b;
    uint64_t m;
    float threshold;
    bool out_counts, out_mod_pairs, out_mod_sims;   // which of the nullable outputs are there
};

// cqs_hip_index_diff's arguments, refused in the documented order: a null handle; (m == 0 asks for nothing); null rows_a,
// rows_b or out_counts; exactly one of the two list outputs; a NaN threshold; a row-sharded handle; handles on different
// devices; different dims; a row outside its index (the text names the first such pair and its side, a before b).
inline Plan plan_diff(const Side& a, const Side& b, const Args& g, std::string* why) {
    why->clear();
    if (!a.present || !b.present) { *why = "null handle"; return Plan::Invalid; }
    if (g.m == 0) return Plan::Nothing;
    if (!g.rows_a) { *why = "null rows_a"; return Plan::Invalid; }
    if (!g.rows_b) { *why = "null rows_b"; return Plan::Invalid; }
    if (!g.out_counts) { *why = "null out_counts"; return Plan::Invalid; }
    if (g.out_mod_pairs != g.out_mod_sims) { *why = "out_mod_pairs and out_mod_sims go together"; return Plan::Invalid; }
    if (g.threshold != g.threshold) { *why = "threshold is NaN"; return Plan::Invalid; }
    if (a.sharded || b.sharded) { *why = "not built for a row-sharded handle"; return Plan::Invalid; }
    if (a.device != b.device) { *why = "the two handles are on different devices"; return Plan::Invalid; }
    if (a.dim != b.dim) { *why = "the two handles differ in dim"; return Plan::Invalid; }
    for (uint64_t i = 0; i < g.m; ++i) {
        const bool in_a = g.rows_a[i] >= a.row_base && g.rows_a[i] - a.row_base < a.len;
        const bool in_b = g.rows_b[i] >= b.row_base && g.rows_b[i] - b.row_base < b.len;
        if (!in_a || !in_b) {
            *why = "pair " + std::to_string(i) + ": row of " + (in_a ? "b" : "a") + " not in its index";
            return Plan::Invalid;
        }
    }
    return Plan::Run;
}

// One trip through the staging block: pairs [first, first + count) of the call.
struct Pass { uint64_t first, count; };

// The m pairs, in order, in passes of at most budget (>= 1) pairs.
inline std::vector<Pass> cut_passes(uint64_t m, uint64_t budget) {
    std::vector<Pass> passes;
    if (budget == 0) budget = 1;
    for (uint64_t first = 0; first < m; first += budget) passes.push_back(Pass{first, std::min(budget, m - first)});
    return passes;
}

// A pass's rows of one side as the kernel takes them: local (row_base taken off; n + row_base < 2^32, create / extend
// keep it so).  The plan has checked the range.
inline void local_rows(const uint64_t* rows, uint64_t row_base, const Pass& p, uint32_t* out) {
    for (uint64_t j = 0; j < p.count; ++j) out[j] = (uint32_t)(rows[p.first + j] - row_base);
}

// One entry of a pass's compacted list, as diff_write_kernel stores it (8 bytes): the pair's index in the pass and the
// bits of its sim.
struct ListEntry { uint32_t index, sim_bits; };

// The concatenation rule: a pass's compacted list (pass-local pair indices, ascending) lands behind what the earlier
// passes gave, its indices moved by the pass's first pair.  Passes are taken in order, so the call's list is ascending
// too.  Returns the new length.
inline uint64_t append_modified(const Pass& p, const ListEntry* list, uint32_t count, uint64_t at, uint64_t* out_mod_pairs,
                                float* out_mod_sims) {
    for (uint32_t j = 0; j < count; ++j) {
        out_mod_pairs[at + j] = p.first + list[j].index;
        memcpy(&out_mod_sims[at + j], &list[j].sim_bits, 4);
    }
    return at + count;
}

// Both handles' mutexes for the length of a call: taken in address order, once when the two are one, released in the
// reverse order.  Two calls that name the same two handles the other way round take them in the same order.
template <class Mutex>
class PairLock {
public:
    PairLock(Mutex& x, Mutex& y) : lo_(&x), hi_(&y) {
        if (lo_ == hi_) hi_ = nullptr;
        else if (std::less<Mutex*>()(hi_, lo_)) std::swap(lo_, hi_);
        lo_->lock();
        if (hi_) hi_->lock();
    }
    ~PairLock() {
        if (hi_) hi_->unlock();
        lo_->unlock();
    }
    PairLock(const PairLock&) = delete;
    PairLock& operator=(const PairLock&) = delete;

private:
    Mutex* lo_;
    Mutex* hi_;
};

// ---- one pair -----------------------------------------------------------------------------------------------------------
// `full_cosine_similarity(a, b).unwrap_or(0.0)` (src/math.rs:35-67, src/diff.rs:191-202) from the three f64 sums, and the
// pair's class against the threshold: the kernel's last step, by this one code.
CQS_DIFF_HD inline float finish_pair(double dot, double na, double nb, float threshold, uint32_t* cls) {
    const double denom = sqrt(na) * sqrt(nb);
    float sim = 0.f;
    uint32_t c = 0;
    if (denom == 0.0) {
        c = kUndefined;
    } else {
        sim = (float)(dot / denom);
        if (!__builtin_isfinite(sim)) { sim = 0.f; c = kUndefined; }
    }
    if (sim < threshold) c |= kModified;
    *cls = c;
    return sim;
}

// One component into a lane's three sums (fused, so host and device round alike).
CQS_DIFF_HD inline void accumulate(double x, double y, double* dot, double* na, double* nb) {
    *dot = fma(x, y, *dot);
    *na = fma(x, x, *na);
    *nb = fma(y, y, *nb);
}

// The kernel's sums for one pair on the host, in the kernel's order - a function of dim alone: lane l of 64 takes the
// 16-byte pieces l, l + 64, ... of both rows, component by component; then the xor-butterfly (32, 16, 8, 4, 2, 1) in which
// every lane adds its partner's value to its own.  dim % 4 == 0.
inline float pair_sim(const float* a, const float* b, uint32_t dim, float threshold, uint32_t* cls) {
    double s[3][64];
    for (uint32_t l = 0; l < 64u; ++l) {
        double dot = 0.0, na = 0.0, nb = 0.0;
        for (uint32_t c = l * 4u; c < dim; c += 256u)
            for (uint32_t e = 0; e < 4u; ++e) accumulate((double)a[c + e], (double)b[c + e], &dot, &na, &nb);
        s[0][l] = dot;
        s[1][l] = na;
        s[2][l] = nb;
    }
    for (uint32_t off = 32; off >= 1u; off >>= 1)
        for (uint32_t v = 0; v < 3u; ++v) {
            double t[64];
            for (uint32_t l = 0; l < 64u; ++l) t[l] = s[v][l] + s[v][l ^ off];
            for (uint32_t l = 0; l < 64u; ++l) s[v][l] = t[l];
        }
    return finish_pair(s[0][0], s[1][0], s[2][0], threshold, cls);
}

// The compaction of a pass on host arrays: the modified pairs' entries densely, in ascending index; counts[0] = modified,
// counts[1] = undefined.  What diff_count_kernel + diff_write_kernel leave in the staging block.
inline void compact(const uint32_t* cls, const float* sims, uint32_t pairs, ListEntry* out, uint32_t counts[2]) {
    counts[0] = counts[1] = 0;
    for (uint32_t i = 0; i < pairs; ++i) {
        if (cls[i] & kUndefined) ++counts[1];
        if (cls[i] & kModified) {
            out[counts[0]].index = i;
            memcpy(&out[counts[0]].sim_bits, &sims[i], 4);
            ++counts[0];
        }
    }
}

}  // namespace cqs_diff
