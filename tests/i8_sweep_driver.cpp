// i8_sweep_driver.cpp — stand-alone check of cqs_amd/csrc/i8_sweep.h (no device): the map from launched workgroups to the
// workgroups whose tasks they take, for both sweep parities, and the plain-load window of a nontemporal int8 scan.  Built
// with -fsanitize=address,undefined and run by tests/test_i8_serpentine_cpu.py.  Prints one "name ok <cases>" line per
// part; any failure prints "FAIL ..." and exits 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../cqs_amd/csrc/i8_sweep.h"

using namespace cqs;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

// Tiers the scan can meet (plan_tiers at 256 CUs over the test sizes) and hand-built ones with every n_tasks mod 4, a
// partial last group and a group across the 64 / 32-row boundary (nA not a multiple of 4).
static std::vector<TaskTiers> all_tiers(std::vector<uint32_t>* pads) {
    std::vector<TaskTiers> v;
    for (uint32_t n_pad : {256u, 512u, 4352u, 131072u, 131328u, 393216u, 393472u, 1000192u}) {
        v.push_back(plan_tiers(n_pad, 256u, false));
        pads->push_back(n_pad);
    }
    for (uint32_t nA : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 41u})
        for (uint32_t nB : {0u, 1u, 2u, 3u, 6u})
            for (uint32_t nC : {0u, 1u, 5u}) {
                if (nA + nB + nC == 0) continue;
                v.push_back(TaskTiers{nA, nB, nC});
                pads->push_back(64u * nA + 32u * nB + 16u * nC);
            }
    return v;
}

// ---- the mapping: a bijection whose image workgroups cover exactly the tasks, and so the rows, they cover forwards ----
static int check_mapping() {
    int cases = 0;
    std::vector<uint32_t> pads;
    const std::vector<TaskTiers> tiers = all_tiers(&pads);
    bool mod_seen[4] = {false, false, false, false}, straddle = false, partial = false;
    for (size_t i = 0; i < tiers.size(); ++i) {
        const GroupMap m{tiers[i], kMaxGroupTasks};
        const uint32_t n_wg = m.total();
        mod_seen[m.n_tasks() % 4u] = true;
        for (uint32_t rev = 0; rev < 2; ++rev) {
            std::vector<uint32_t> hit(n_wg, 0u);
            std::vector<uint32_t> row_hit(pads[i], 0u);
            for (uint32_t b = 0; b < n_wg; ++b) {
                const uint32_t g = sweep_group(b, n_wg, rev);
                CHECK(g < n_wg, "workgroup %u of %u maps to %u (rev %u)", b, n_wg, g, rev);
                if (g >= n_wg) continue;
                ++hit[g];
                CHECK(rev ? g == n_wg - 1u - b : g == b, "workgroup %u maps to %u (rev %u)", b, g, rev);
                for (uint32_t w = 0; w < kMaxGroupTasks; ++w) {   // the kernel's waves: task 4 g + w, gone past the last
                    const uint32_t t = g * kMaxGroupTasks + w;
                    if (t >= m.n_tasks()) { CHECK(w >= m.tasks(g), "a live task dropped"); continue; }
                    uint32_t tr = 0;
                    const uint32_t base = tiers[i].locate(t, tr);
                    for (uint32_t r = base; r < base + tr; ++r) {
                        CHECK(r < pads[i], "row %u past the pad %u", r, pads[i]);
                        if (r < pads[i]) ++row_hit[r];
                    }
                }
                uint32_t rows = 0, r0 = 0, r1 = 0;
                m.locate(g, rows);
                tiers[i].locate(m.first_task(g), r0);
                tiers[i].locate(m.first_task(g) + m.tasks(g) - 1u, r1);
                if (r0 != r1) straddle = true;
                if (m.tasks(g) < kMaxGroupTasks) partial = true;
            }
            for (uint32_t g = 0; g < n_wg; ++g) CHECK(hit[g] == 1u, "workgroup %u taken %u times (rev %u)", g, hit[g], rev);
            for (uint32_t r = 0; r < pads[i]; ++r) CHECK(row_hit[r] == 1u, "row %u covered %u times (rev %u)", r, row_hit[r], rev);
            ++cases;
        }
    }
    CHECK(mod_seen[0] && mod_seen[1] && mod_seen[2] && mod_seen[3], "an n_tasks mod 4 is missing");
    CHECK(straddle && partial, "no group across the tier boundary (%d) or no partial last group (%d)", (int)straddle, (int)partial);
    return cases;
}

// ---- the window: exactly the workgroups whose bytes meet the first or the last w bytes --------------------------------
static int check_window() {
    int cases = 0;
    std::vector<uint32_t> pads;
    const std::vector<TaskTiers> tiers = all_tiers(&pads);
    for (size_t i = 0; i < tiers.size(); ++i) {
        const GroupMap m{tiers[i], kMaxGroupTasks};
        const uint32_t n_wg = m.total();
        for (uint32_t short_by : {0u, 1u, 15u, 200u}) {   // n below the pad: the last workgroups read fewer rows, or none
            if (short_by >= pads[i]) continue;
            const uint32_t n = pads[i] - short_by;
            for (uint32_t dim : {16u, 768u, 2048u}) {
                const uint64_t total = (uint64_t)n * dim;
                const uint64_t ws[] = {0u, 1u, (uint64_t)dim, 256ull * dim, 256ull * dim + 1u, 3ull * 256u * dim - 1u, total / 3u,
                                       total / 2u, total / 2u + 1u, total - 1u, total, total + 1u, ~0ull};
                for (uint64_t w : ws) {
                    const PlainWindow pw = plain_window(m, n, dim, w);
                    const uint64_t we = w < total ? w : total;
                    uint32_t n_plain = 0;
                    for (uint32_t g = 0; g < n_wg; ++g) {
                        uint32_t rows = 0;
                        const uint32_t first = m.locate(g, rows);
                        const uint64_t b = (uint64_t)(first < n ? first : n) * dim;
                        const uint64_t e = (uint64_t)(first + rows < n ? first + rows : n) * dim;
                        if (b == e) continue;   // reads nothing: either policy
                        const bool want = we > 0 && (b < we || e > total - we);
                        CHECK(pw.plain(g) == want, "tiers %u %u %u n %u dim %u w %llu: workgroup %u [%llu, %llu) plain %d want %d (lo %u hi %u)",
                              tiers[i].nA, tiers[i].nB, tiers[i].nC, n, dim, (unsigned long long)w, g, (unsigned long long)b,
                              (unsigned long long)e, (int)pw.plain(g), (int)want, pw.lo, pw.hi);
                        n_plain += want;
                    }
                    if (w == 0) CHECK(n_plain == 0 && pw.lo == 0 && pw.hi == n_wg, "w = 0 leaves %u plain", n_plain);
                    if (w >= total) {
                        for (uint32_t g = 0; g < n_wg; ++g) CHECK(pw.plain(g), "w >= the copy: workgroup %u not plain", g);
                    }
                    ++cases;
                }
            }
        }
    }
    return cases;
}

int main() {
    const int a = check_mapping();
    printf("mapping ok %d\n", a);
    const int b = check_window();
    printf("window ok %d\n", b);
    if (g_fail) { printf("FAIL %d checks\n", g_fail); return 1; }
    printf("all ok\n");
    return 0;
}
