// match_host.h — the device-free part of cqs_hip_index_match: the argument plan (the refusals in their order), the
// global -> local row conversion, the packed best-partner key with its "none" sentinel, the rule by which the answers of
// two calls over different blocks of the other side's list merge, and the mutual pairs of a finished answer (DESIGN.md
// §3.17a).  Plain C++ over the caller's arrays, no HIP, no handle: index_match.hip calls it under both handles' mutexes
// and its kernel packs the same key; tests/match_host_driver.cpp runs it under ASAN + UBSan on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace cqs_match {

constexpr uint32_t kMaxRows = 65536;             // CQS_HIP_MATCH_MAX: rows per side of one call
constexpr uint64_t kNone = ~0ull;                // out_best of a row without a finite entry (its score is 0.0f)

enum class Plan : int32_t {
    Invalid = -1,   // CQS_HIP_ERR_INVALID; *why says which refusal; outputs untouched
    Nothing = 0,    // m_a == 0 && m_b == 0: CQS_HIP_OK, nothing touched
    Run = 1,        // every listed row is a stored row of its side (one side may be empty: the other's rows get kNone)
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
    uint32_t m_a;
    const uint64_t* rows_b;
    uint32_t m_b;
    bool out_best_a, out_score_a, out_best_b, out_score_b;   // which outputs are there
};

inline bool row_inside(uint64_t row, const Side& s) { return row >= s.row_base && row - s.row_base < s.len; }

// cqs_hip_index_match's arguments, refused in the documented order: a null handle; (both lists empty asks for nothing);
// a null list of a side with rows; a null output of a side with rows; a list above kMaxRows; a row-sharded handle;
// handles on different devices; different dims; a row outside its index (the text names the side and the first such
// position, all of a before b).
inline Plan plan_match(const Side& a, const Side& b, const Args& g, std::string* why) {
    why->clear();
    if (!a.present || !b.present) { *why = "null handle"; return Plan::Invalid; }
    if (g.m_a == 0 && g.m_b == 0) return Plan::Nothing;
    if (g.m_a && !g.rows_a) { *why = "null rows_a"; return Plan::Invalid; }
    if (g.m_b && !g.rows_b) { *why = "null rows_b"; return Plan::Invalid; }
    if (g.m_a && !(g.out_best_a && g.out_score_a)) { *why = "null output of side a"; return Plan::Invalid; }
    if (g.m_b && !(g.out_best_b && g.out_score_b)) { *why = "null output of side b"; return Plan::Invalid; }
    if (g.m_a > kMaxRows) { *why = "m_a above CQS_HIP_MATCH_MAX"; return Plan::Invalid; }
    if (g.m_b > kMaxRows) { *why = "m_b above CQS_HIP_MATCH_MAX"; return Plan::Invalid; }
    if (a.sharded || b.sharded) { *why = "not built for a row-sharded handle"; return Plan::Invalid; }
    if (a.device != b.device) { *why = "the two handles are on different devices"; return Plan::Invalid; }
    if (a.dim != b.dim) { *why = "the two handles differ in dim"; return Plan::Invalid; }
    for (uint32_t i = 0; i < g.m_a; ++i)
        if (!row_inside(g.rows_a[i], a)) { *why = "rows_a[" + std::to_string(i) + "] not in its index"; return Plan::Invalid; }
    for (uint32_t j = 0; j < g.m_b; ++j)
        if (!row_inside(g.rows_b[j], b)) { *why = "rows_b[" + std::to_string(j) + "] not in its index"; return Plan::Invalid; }
    return Plan::Run;
}

// A side's rows as the kernel takes them: local (row_base taken off; n + row_base < 2^32, create / extend keep it so).
// The plan has checked the range.
inline void local_rows(const uint64_t* rows, uint64_t row_base, uint32_t m, uint32_t* out) {
    for (uint32_t i = 0; i < m; ++i) out[i] = (uint32_t)(rows[i] - row_base);
}

// ---- the packed candidate -----------------------------------------------------------------------------------------------
// (ordered_u32(score) << 32) | (0xFFFFFFFF - position): the greater key is the greater score under the f32 total order,
// the lower position among equal scores - one `max` per pair, in any order.  A non-finite score packs to 0 = "none": no
// finite score has ordered bits 0 (those are the bits of a negative NaN), so every real candidate is above it.
inline uint32_t ordered_bits(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
inline float from_ordered_bits(uint32_t k) {
    const uint32_t b = (k >> 31) ? k ^ 0x80000000u : ~k;
    float x;
    memcpy(&x, &b, 4);
    return x;
}
inline bool is_finite(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}
inline uint64_t pack(float score, uint32_t position) {
    return is_finite(score) ? ((uint64_t)ordered_bits(score) << 32) | (uint64_t)(0xFFFFFFFFu - position) : 0ull;
}
// A key as the outputs state it: (position, score), or (kNone, 0.0f) for key 0.
inline void unpack(uint64_t key, uint64_t* best, float* score) {
    if (key == 0) { *best = kNone; *score = 0.0f; return; }
    *best = 0xFFFFFFFFu - (uint32_t)key;
    *score = from_ordered_bits((uint32_t)(key >> 32));
}

// ---- answers over blocks of the other side ------------------------------------------------------------------------------
// (best, score) holds a row's answer over some blocks of the other side's list, positions global in that list;
// (other_best, other_score) its answer over another block.  The greater score under the total order wins, then the lower
// position; kNone loses to everything.  The rule is a maximum of a total order, so blocks merge in any order.
inline void merge_best(uint64_t* best, float* score, uint64_t other_best, float other_score) {
    if (other_best == kNone) return;
    if (*best != kNone) {
        const uint32_t mine = ordered_bits(*score), theirs = ordered_bits(other_score);
        if (mine > theirs || (mine == theirs && *best <= other_best)) return;
    }
    *best = other_best;
    *score = other_score;
}

// The pairs (i, j) that chose each other - best_a[i] == j and best_b[j] == i - with score_a[i] >= threshold (an f32
// compare; a NaN threshold keeps nothing), in ascending i.  One-to-one: i names one j, and j names one i.
inline std::vector<std::pair<uint64_t, uint64_t>> mutual_pairs(const uint64_t* best_a, const float* score_a, uint64_t m_a,
                                                               const uint64_t* best_b, uint64_t m_b, float threshold) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    for (uint64_t i = 0; i < m_a; ++i) {
        const uint64_t j = best_a[i];
        if (j == kNone || j >= m_b || best_b[j] != i) continue;
        if (score_a[i] >= threshold) out.emplace_back(i, j);
    }
    return out;
}

}  // namespace cqs_match
