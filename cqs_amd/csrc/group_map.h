// group_map.h — which rows a maximum of the select's index stands for (DESIGN.md §3.2, §3.11 "Workgroup maxima").  The scans
// cut the padded corpus into tasks (TaskTiers); a producer publishes one (maximum, argmax, runner-up) triple per GROUP of G
// consecutive tasks: G = 1 for every scan but the int8 copy's, whose 256-thread workgroup owns four consecutive tasks and
// publishes one triple for them (G = 4).  Header-only and host-and-device, so the scan, the select and a CPU test
// (tests/group_map_driver.cpp) run the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CQS_GM_HD __host__ __device__
#else
#define CQS_GM_HD
#endif

#ifndef CQS_SCAN_TIER_B
#define CQS_SCAN_TIER_B 2u   // 32-row tasks at the end of the corpus, in units of (n_cu * 4 / 2)
#endif

namespace cqs {

// Work-queue tasks in row order: nA tasks of 64 rows, then nB of 32, then nC of 16 (64 nA + 32 nB +
// 16 nC = n_pad).  One task = one wave's unit of work.
struct TaskTiers {
    uint32_t nA, nB, nC;
    CQS_GM_HD uint32_t total() const { return nA + nB + nC; }
    // first row and row count of task t
    CQS_GM_HD uint32_t locate(uint32_t t, uint32_t& rows) const {
        if (t < nA) { rows = 64u; return t * 64u; }
        if (t < nA + nB) { rows = 32u; return nA * 64u + (t - nA) * 32u; }
        rows = 16u;
        return nA * 64u + nB * 32u + (t - nA - nB) * 16u;
    }
};

// Task sizes over the padded corpus (measured at 768-d, 1 query; MI355X, 256 CUs):
//   < 8 64-row tasks per CU (<= 131k rows): 16-row tasks, so a 17.5k-row corpus still reaches every CU;
//   otherwise 64-row tasks (8 batches of 8 rows: the double buffer's fill/drain is amortised), with the
//   last two rounds' worth of 32-row tasks: the launch ends when its slowest wave does, and halving the
//   final tasks halves that tail (-5 us of 460 at 1M rows).  16-row tail tasks cost more than they gain.
inline TaskTiers plan_tiers(uint32_t n_pad, uint32_t n_cu, bool uniform64) {
    TaskTiers t{0u, 0u, 0u};
    const uint32_t n64 = n_pad / 64u, waves = n_cu * 4u;
    if (uniform64) { t.nA = n64; return t; }  // matrix-core kernel: 64-row groups only
    if (n64 < 8u * n_cu) { t.nC = n_pad / 16u; return t; }
    const uint32_t nb = CQS_SCAN_TIER_B * (waves / 2u) & ~1u;
    if (n64 >= 6u * waves && n64 > nb / 2u) { t.nA = n64 - nb / 2u; t.nB = nb; }
    else t.nA = n64;
    return t;
}

constexpr uint32_t kMaxGroupTasks = 4;   // largest G: the waves of the int8 scan's workgroup

// Group g = tasks [G g, min(G g + G, n_tasks)): at most 4 x 64 = 256 consecutive rows.  A group may straddle a tier boundary
// (64-row tasks followed by 32-row ones) and the last one may be partial.  G is a power of two <= kMaxGroupTasks.
struct GroupMap {
    TaskTiers tiers;
    uint32_t G;   // tasks per group
    CQS_GM_HD uint32_t n_tasks() const { return tiers.total(); }
    CQS_GM_HD uint32_t total() const { return (tiers.total() + G - 1u) / G; }
    CQS_GM_HD uint32_t first_task(uint32_t g) const { return G * g; }
    CQS_GM_HD uint32_t tasks(uint32_t g) const {
        const uint32_t left = tiers.total() - G * g;
        return left < G ? left : G;
    }
    // first row of group g
    CQS_GM_HD uint32_t base(uint32_t g) const {
        uint32_t r;
        return tiers.locate(G * g, r);
    }
    // first row and row count (<= 256) of group g
    CQS_GM_HD uint32_t locate(uint32_t g, uint32_t& rows) const {
        uint32_t r;
        const uint32_t first = tiers.locate(G * g, r);
        if (G == 1u) { rows = r; return first; }
        const uint32_t last = tiers.locate(G * g + tasks(g) - 1u, r);
        rows = last + r - first;
        return first;
    }
};

// What a producer publishes per task or group: the maximum of its rows' scores (-inf: no live row), the lowest row that
// holds it (relative to the first row) and the largest score of the OTHER rows (equal to the maximum when it occurs twice).
struct MaxTriple {
    float max;
    uint32_t arg;
    float sec;
};

// The group's triple from its tasks' triples w[0, nw) in task order, off[i] = task i's first row - the group's first row.
// Winner = the first task whose maximum equals the largest: with its own arg the lowest row among equal maxima.  Runner-up
// = the larger of the winner's own runner-up and the other tasks' maxima.  -inf passes through (all -inf: task 0's triple);
// there are no NaNs in a stored score row.
CQS_GM_HD inline MaxTriple combine_triples(const MaxTriple* w, const uint32_t* off, uint32_t nw) {
    // One pass, no indexing by a run-time winner (registers on the device).  `out` is the rule applied to tasks [0, i): a
    // later task with a larger maximum takes over, and the runner-up is then its own or the maximum it beat (which was at
    // least every earlier runner-up); any other task, an equal maximum included, can only raise the runner-up.
    MaxTriple out{w[0].max, off[0] + w[0].arg, w[0].sec};
    for (uint32_t i = 1; i < nw; ++i) {
        if (w[i].max > out.max) {
            out.sec = w[i].sec > out.max ? w[i].sec : out.max;
            out.max = w[i].max;
            out.arg = off[i] + w[i].arg;
        } else if (w[i].max > out.sec) {
            out.sec = w[i].max;
        }
    }
    return out;
}

}  // namespace cqs
