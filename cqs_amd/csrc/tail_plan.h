// tail_plan.h — the tiers of the shadow search's tail kernel ("Prefix first"): how many candidates its first
// select asks for, how many slots and workgroups per query that makes, and where the first tier is on by default.
// Header-only and device-free, so the host launcher and the kernel (scan_bf16.hip) and a CPU test
// (tests/tail_plan_driver.cpp) share one arithmetic.
//
// Tier 1: where the copy's k' leaves room for a proper prefix (tail_prefix.h: 6k + 40 < k', the int8 copy's k' = 10k + 150),
// every workgroup selects j1 + 1 keys and the query's waves rescore candidates 0 .. j1 - 1 only; the finisher certifies on
// them, and where that fails it alone selects k' + 1 and rescores the rest.  No proper prefix possible (the bf16 copy), or
// the tier switched off: first = 0, and slots and grid are the ones of the tail without tiers.
#pragma once
#include "tail_prefix.h"

namespace cqs {

constexpr uint32_t kTailWaves = 16;   // waves per workgroup of the tail kernel, one slot each and round

// Candidates of tier 1 (j1 = tail_prefix_first(k, k')), or 0: no tiers.  `prefix` is the finisher's prefix sort
// (CQS_HIP_TAIL_PREFIX), without which there is no certificate on a prefix; `prefix_first` this tier's own switch.
CQS_TP_HD inline uint32_t tail_plan_first(uint32_t k, uint32_t kprime, bool prefix, bool prefix_first) {
    if (!prefix || !prefix_first) return 0u;
    const uint32_t j1 = tail_prefix_first(k, kprime);
    return j1 < kprime ? j1 : 0u;
}

// Slots of the query's waves before the ticket: B_q and one per candidate.  Also the keys the first select asks for (one
// past the candidates: the first key outside them).
CQS_TP_HD inline uint32_t tail_plan_slots(uint32_t kprime, uint32_t first) { return (first ? first : kprime) + 1u; }

// Workgroups per query: one wave per slot while the block's workgroups fit the device in one round (cap), else fewer
// workgroups whose waves take several slots each.  Never 0.
CQS_TP_HD inline uint32_t tail_plan_workgroups(uint32_t slots, uint32_t b, uint32_t n_cu, uint32_t per_cu) {
    const uint32_t want = (slots + kTailWaves - 1u) / kTailWaves;
    uint32_t cap = b ? n_cu * per_cu / b : 0u;
    if (cap < 1u) cap = 1u;
    return want < cap ? want : cap;
}

// Where tier 1 is on when CQS_HIP_TAIL_PREFIX_FIRST is unset.  A query whose prefix fails pays the slow path (one workgroup
// selects again and fetches the remaining rows); the tier pays where (share of failing queries) x (slow path's extra time) <
// half the saving.  Measured on one MI355X over Gaussian unit rows x 768 ("Prefix first";
// profiles/prefix_first_cells.json): the slow path costs +23.1 us - an upper figure: it was taken on planted crowds of tied
// scores, where the last sort runs its exact-rank branch (8.6 us where a Gaussian query's takes about 4); of 330 seeded queries
// the prefix fails for 0 / 2 / 0 / 0 at 1M rows and for 0 / 75 / 105 / 86 at 10M rows (k = 1 / 20 / 50 / 87): 0.14 us expected
// loss against a saving of 1.8-2.5 us at 1M, 5.3 us at 10M.  The bound lies between the two sizes measured; nothing was
// measured in between.  k is a parameter because the share depends on it (none fail at k = 1 at either size); the rule does not
// use it yet: at both sizes every k >= 20 falls on the same side, and k = 1 alone was not worth a second threshold.
constexpr uint64_t kTailFirstMaxRows = 4ull << 20;
CQS_TP_HD inline bool tail_prefix_first_default(uint64_t n_pad, uint32_t /*k*/) { return n_pad <= kTailFirstMaxRows; }

}  // namespace cqs
