// group_map_driver.cpp — stand-alone check of cqs_amd/csrc/group_map.h (no device): the map from the select's maxima
// groups to tasks and rows, the rule that combines up to four wave triples into a group's, and the select's premise with
// four tasks per group.  Built with -fsanitize=address,undefined and run by tests/test_group_map_cpu.py.  Prints one
// "name ok <cases>" line per part; any failure prints "FAIL ..." and exits 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../cqs_amd/csrc/group_map.h"

using namespace cqs;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

static const float NINF = -INFINITY;

// ---- the map ------------------------------------------------------------------------------------------------------
// Groups partition [0, n_pad) in order, hold <= 256 rows each, and agree with the tasks they are made of.
static void check_map(const TaskTiers& t, uint32_t G, uint32_t n_pad) {
    const GroupMap m{t, G};
    const uint32_t n_tasks = t.total();
    CHECK(m.n_tasks() == n_tasks && m.total() == (n_tasks + G - 1) / G, "total %u %u G %u", m.total(), n_tasks, G);
    uint32_t next_row = 0, next_task = 0;
    for (uint32_t g = 0; g < m.total(); ++g) {
        uint32_t rows = 0;
        const uint32_t base = m.locate(g, rows);
        CHECK(base == next_row && base == m.base(g), "group %u starts at %u, want %u (G %u, tiers %u %u %u)", g, base, next_row, G, t.nA, t.nB, t.nC);
        CHECK(rows >= 16 && rows <= 256, "group %u has %u rows", g, rows);
        CHECK(m.first_task(g) == next_task, "group %u first task %u want %u", g, m.first_task(g), next_task);
        const uint32_t nt = m.tasks(g);
        CHECK(nt >= 1 && nt <= G && (nt == G || g + 1 == m.total()), "group %u has %u tasks", g, nt);
        uint32_t sum = 0;
        for (uint32_t j = 0; j < nt; ++j) {   // its tasks, in order, back to back
            uint32_t tr = 0;
            const uint32_t tb = t.locate(next_task + j, tr);
            CHECK(tb == base + sum, "task %u of group %u at %u want %u", j, g, tb, base + sum);
            sum += tr;
        }
        CHECK(sum == rows, "group %u: %u rows, its tasks %u", g, rows, sum);
        next_row += rows;
        next_task += nt;
    }
    CHECK(next_row == n_pad && next_task == n_tasks, "covered %u rows of %u, %u tasks of %u", next_row, n_pad, next_task, n_tasks);
}

static uint32_t map_cases() {
    uint32_t cases = 0, seen_res[3][4] = {{0}};
    bool straddle = false;
    const uint32_t n_cu = 256;
    auto one = [&](const TaskTiers& t, uint32_t n_pad) {
        CHECK(64u * t.nA + 32u * t.nB + 16u * t.nC == n_pad, "tiers %u %u %u do not cover %u", t.nA, t.nB, t.nC, n_pad);
        const int regime = t.nC ? 0 : (t.nB ? 2 : 1);
        ++seen_res[regime][t.total() % 4u];
        if (t.nB && t.nA % 4u) straddle = true;
        for (uint32_t G : {1u, 2u, 4u}) { check_map(t, G, n_pad); ++cases; }
    };
    // plan_tiers at 256 CUs: 16-row tasks below 131 072 rows, 64-row tasks up to 393 216, then 64 + 32.  n_pad in steps of 16 /
    // 64 (the index pads to 256, which leaves n_tasks a multiple of 4 on this device; other CU counts and callers do not)
    for (uint32_t n_pad = 16; n_pad <= 2048; n_pad += 16) one(plan_tiers(n_pad, n_cu, false), n_pad);
    for (uint32_t n_pad = 131072 - 512; n_pad < 131072; n_pad += 16) one(plan_tiers(n_pad, n_cu, false), n_pad);
    for (uint32_t n_pad = 131072; n_pad <= 131072 + 1024; n_pad += 64) one(plan_tiers(n_pad, n_cu, false), n_pad);
    for (uint32_t n_pad = 393216 - 512; n_pad <= 393216 + 1024; n_pad += 64) one(plan_tiers(n_pad, n_cu, false), n_pad);
    for (uint32_t n_pad : {1000192u, 1000000u, 1000064u, 1000128u}) one(plan_tiers(n_pad, n_cu, false), n_pad);
    for (uint32_t cu : {1u, 7u, 104u, 228u, 304u})
        for (uint32_t n_pad = 256; n_pad <= 700000; n_pad += 9984 + 64 * (cu % 3)) one(plan_tiers(n_pad, cu, false), n_pad);
    for (uint32_t n_pad = 64; n_pad <= 4096; n_pad += 64) one(plan_tiers(n_pad, n_cu, true), n_pad);   // uniform 64-row groups
    // hand-built tiers: every residue of nA and nB, with and without 16-row tasks behind them
    for (uint32_t nA = 0; nA < 9; ++nA)
        for (uint32_t nB = 0; nB < 9; ++nB)
            for (uint32_t nC = 0; nC < 6; ++nC)
                if (nA + nB + nC) one(TaskTiers{nA, nB, nC}, 64 * nA + 32 * nB + 16 * nC);
    for (int r = 0; r < 3; ++r)
        for (int m = 0; m < 4; ++m) CHECK(seen_res[r][m] > 0, "regime %d never had n_tasks mod 4 = %d", r, m);
    CHECK(straddle, "no group straddled the 64 / 32-row boundary");
    return cases;
}

// ---- the combine rule -----------------------------------------------------------------------------------------------
// A wave's triple over rows s[0, n): maximum, lowest row that holds it, largest of the OTHER rows (what the scans compute).
static MaxTriple wave_triple(const float* s, uint32_t n) {
    MaxTriple t{NINF, 0, NINF};
    for (uint32_t i = 0; i < n; ++i)
        if (s[i] > t.max) { t.max = s[i]; t.arg = i; }
    for (uint32_t i = 0; i < n; ++i)
        if (i != t.arg && s[i] > t.sec) t.sec = s[i];
    return t;
}
static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

// One group of `nw` tasks with the given row counts: the combined triple against brute force over the group's rows.
static void check_group(const std::vector<float>& s, const std::vector<uint32_t>& trows) {
    MaxTriple w[kMaxGroupTasks];
    uint32_t off[kMaxGroupTasks], at = 0;
    for (size_t i = 0; i < trows.size(); ++i) {
        w[i] = wave_triple(s.data() + at, trows[i]);
        off[i] = at;
        at += trows[i];
    }
    const MaxTriple got = combine_triples(w, off, (uint32_t)trows.size());
    const MaxTriple want = wave_triple(s.data(), at);
    CHECK(same_bits(got.max, want.max) && got.arg == want.arg && same_bits(got.sec, want.sec),
          "combine: got (%g, %u, %g) want (%g, %u, %g) over %u rows in %zu tasks", got.max, got.arg, got.sec, want.max, want.arg,
          want.sec, at, trows.size());
}

static uint32_t combine_cases() {
    std::mt19937 rng(0xC950);
    std::uniform_real_distribution<float> uni(-1.f, 1.f);
    const uint32_t sizes[3] = {64, 32, 16};
    uint32_t cases = 0;
    for (int it = 0; it < 4000; ++it) {
        const uint32_t nw = 1 + rng() % 4;
        std::vector<uint32_t> trows(nw);
        uint32_t tier = rng() % 3;
        for (uint32_t i = 0; i < nw; ++i) {   // tiers only shrink along a group (64 -> 32 -> 16)
            if (tier < 2 && rng() % 4 == 0) ++tier;
            trows[i] = sizes[tier];
        }
        uint32_t n = 0;
        for (uint32_t r : trows) n += r;
        std::vector<float> s(n);
        const int kind = it % 8;
        for (auto& v : s) v = (kind == 1) ? NINF : uni(rng);
        if (kind == 2 || kind == 3) {   // mostly dropped rows
            for (auto& v : s) if (rng() % 8) v = NINF;
        }
        if (kind == 4) {   // ties at the maximum inside one wave
            const uint32_t a = rng() % trows[0], b = rng() % trows[0];
            s[a] = s[b] = 2.f;
        }
        if (kind == 5 && nw > 1) {   // ties at the maximum across waves (and a third copy somewhere)
            s[rng() % trows[0]] = 2.f;
            s[n - 1 - rng() % trows[nw - 1]] = 2.f;
            if (rng() % 2) s[rng() % n] = 2.f;
        }
        if (kind == 6) {   // one finite row
            for (auto& v : s) v = NINF;
            s[rng() % n] = uni(rng);
        }
        if (kind == 7) s[n - 1 - rng() % trows[nw - 1]] = 3.f;   // the maximum in the last (partial group's last) task
        if (kind == 0 && rng() % 2) {   // a few distinct values only: ties everywhere
            for (auto& v : s) v = (float)(int)(rng() % 3);
        }
        check_group(s, trows);
        ++cases;
    }
    return cases;
}

// ---- the select's premise with G tasks per group --------------------------------------------------------------------
// Host restatement of select_body: histogram the group maxima over a monotone bin map, T = the highest bin with at least k
// maxima at or above it; then every top-k entry lies in a group whose maximum's bin is >= T - and, for the direct path, a
// listed group whose runner-up's bin is < T holds exactly one entry with bin >= T: its maximum, at base + arg.
static uint32_t bin_linear(float s) {
    const float t = (s + 1.0f) * 2048.0f;
    const int b = (int)t;
    return (uint32_t)(b < 0 ? 0 : (b > 4095 ? 4095 : b));
}

static uint32_t premise_cases() {
    std::mt19937 rng(0xC951);
    std::normal_distribution<float> gauss(0.f, 0.04f);
    uint32_t cases = 0;
    for (int it = 0; it < 60; ++it) {
        const uint32_t nA = rng() % 40, nB = rng() % 9, nC = (nA + nB) ? rng() % 5 : 1 + rng() % 40;
        const TaskTiers t{nA, nB, nC};
        const uint32_t n_pad = 64 * nA + 32 * nB + 16 * nC;
        std::vector<float> s(n_pad);
        for (auto& v : s) v = (it % 5 == 4 && rng() % 3) ? 0.25f : gauss(rng);   // (a crowd of equal scores every fifth case)
        for (auto& v : s) if (rng() % 16 == 0) v = NINF;
        for (uint32_t G : {1u, 4u}) {
            const GroupMap m{t, G};
            std::vector<MaxTriple> trip(m.total());
            for (uint32_t g = 0; g < m.total(); ++g) {   // as the scan publishes them: wave triples, combined
                MaxTriple w[kMaxGroupTasks];
                uint32_t off[kMaxGroupTasks], rows = 0;
                const uint32_t base = m.locate(g, rows);
                for (uint32_t j = 0; j < m.tasks(g); ++j) {
                    uint32_t tr = 0;
                    const uint32_t tb = t.locate(m.first_task(g) + j, tr);
                    w[j] = wave_triple(s.data() + tb, tr);
                    off[j] = tb - base;
                }
                trip[g] = combine_triples(w, off, m.tasks(g));
            }
            for (uint32_t k : {1u, 7u, 21u, 351u}) {
                std::vector<uint32_t> hist(4096, 0);
                uint32_t total = 0;
                for (const auto& x : trip) if (x.max != NINF) { ++hist[bin_linear(x.max)]; ++total; }
                uint32_t T = 0;
                if (total >= k) { uint32_t acc = 0; for (T = 4095;; --T) { acc += hist[T]; if (acc >= k) break; } }
                // brute-force top k by (score, lowest row first)
                std::vector<uint32_t> order;
                for (uint32_t i = 0; i < n_pad; ++i) if (s[i] != NINF) order.push_back(i);
                std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return s[a] > s[b]; });
                if (order.size() > k) order.resize(k);
                std::vector<char> in_top(n_pad, 0);
                for (uint32_t r : order) in_top[r] = 1;
                std::vector<char> listed(n_pad, 0);   // rows the select would hold as candidates
                for (uint32_t g = 0; g < m.total(); ++g) {
                    if (trip[g].max == NINF || bin_linear(trip[g].max) < T) continue;
                    uint32_t rows = 0;
                    const uint32_t base = m.locate(g, rows);
                    const bool need = trip[g].sec != NINF && bin_linear(trip[g].sec) >= T;
                    if (!need) {
                        listed[base + trip[g].arg] = 1;
                        CHECK(same_bits(s[base + trip[g].arg], trip[g].max), "direct group %u: arg does not hold the maximum", g);
                    } else {
                        for (uint32_t i = 0; i < rows; ++i) if (s[base + i] != NINF && bin_linear(s[base + i]) >= T) listed[base + i] = 1;
                    }
                }
                for (uint32_t r : order) CHECK(listed[r], "G %u k %u: top-k row %u (%g) is not a candidate (T %u)", G, k, r, s[r], T);
                for (uint32_t i = 0; i < n_pad; ++i)   // ... and the candidates are exactly the entries with bin >= T
                    CHECK(listed[i] == (s[i] != NINF && bin_linear(s[i]) >= T ? 1 : 0) || total < k, "G %u k %u: row %u listed %d", G, k, i, listed[i]);
                ++cases;
            }
        }
    }
    return cases;
}

int main() {
    const uint32_t m = map_cases();
    if (!g_fail) printf("map ok %u\n", m);
    const uint32_t c = combine_cases();
    if (!g_fail) printf("combine ok %u\n", c);
    const uint32_t p = premise_cases();
    if (!g_fail) printf("premise ok %u\n", p);
    if (g_fail) { printf("FAIL %d checks\n", g_fail); return 1; }
    printf("all ok\n");
    return 0;
}
