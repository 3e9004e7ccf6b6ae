// tail_plan_driver.cpp — stand-alone check of cqs_amd/csrc/tail_plan.h (no device): the tiers of the shadow search's tail
// kernel over every k the select takes, the k' of both copies, blocks of 1..8 queries and devices of 1, 8 and 256 CUs.
// Built with -fsanitize=address,undefined and run by tests/test_tail_plan_cpu.py.  Prints one "name ok <cases>" line per
// group; any failure prints "FAIL ..." and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../cqs_amd/csrc/scan_i8.h"
#include "../cqs_amd/csrc/tail_plan.h"

using namespace cqs;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_fail; } } while (0)

// The tail without tiers, written out: B_q and k' candidates, one wave each; ceil / 16 workgroups under the cap.
static uint32_t plain_slots(uint32_t kprime) { return kprime + 1u; }
static uint32_t plain_workgroups(uint32_t kprime, uint32_t b, uint32_t n_cu) {
    const uint32_t want = (kprime + 1u + 15u) / 16u;
    uint32_t cap = n_cu / b;
    if (cap < 1u) cap = 1u;
    return want < cap ? want : cap;
}

int main() {
    uint32_t cases = 0, tiered = 0, halved = 0;
    for (uint32_t k = 1; k <= 128; ++k) {
        std::vector<uint32_t> kps{shadow_kprime(k)};
        if (i8_k_ok(k)) kps.push_back(i8_kprime(k));
        for (uint32_t kp : kps) {
            const bool room = tail_prefix_first(k, kp) < kp;      // a proper prefix is possible
            for (int prefix = 0; prefix < 2; ++prefix)
                for (int sw = 0; sw < 2; ++sw) {
                    const uint32_t first = tail_plan_first(k, kp, prefix != 0, sw != 0);
                    const uint32_t slots = tail_plan_slots(kp, first);
                    CHECK(slots <= plain_slots(kp), "slots %u above the tail's %u: k %u k' %u", slots, plain_slots(kp), k, kp);
                    CHECK(slots >= 2u, "slots %u: k %u k' %u", slots, k, kp);
                    if (room && prefix && sw) {
                        CHECK(first == tail_prefix_first(k, kp) && first == 6u * k + 40u && first < kp, "j1 %u: k %u k' %u", first, k, kp);
                        CHECK(slots == first + 1u, "tier 1 slots %u, j1 %u", slots, first);
                        CHECK(first >= k, "the prefix holds fewer than k rows: j1 %u k %u", first, k);
                        ++tiered;
                    } else {
                        CHECK(first == 0u && slots == plain_slots(kp), "no tiers, but first %u slots %u: k %u k' %u prefix %d switch %d",
                              first, slots, k, kp, prefix, sw);
                    }
                    for (uint32_t b = 1; b <= 8; ++b)
                        for (uint32_t n_cu : {1u, 8u, 256u}) {
                            const uint32_t g = tail_plan_workgroups(slots, b, n_cu, 1u);
                            const uint32_t g0 = plain_workgroups(kp, b, n_cu);
                            uint32_t cap = n_cu / b;
                            if (cap < 1u) cap = 1u;
                            CHECK(g >= 1u && g <= cap, "grid %u outside [1, %u]: k %u k' %u b %u CUs %u", g, cap, k, kp, b, n_cu);
                            CHECK(g <= g0, "grid %u above the tail's %u", g, g0);
                            CHECK((uint64_t)g * 16u >= slots || g == cap, "grid %u short of %u slots under cap %u", g, slots, cap);
                            if (first == 0u) CHECK(g == g0, "no tiers, but grid %u != %u: k %u k' %u b %u CUs %u", g, g0, k, kp, b, n_cu);
                            else if (g * 2u <= g0 + 1u) ++halved;
                            ++cases;
                        }
                }
        }
    }
    CHECK(tiered == 87u, "every int8 k from 1 to 87 has a tier, no bf16 k has: %u", tiered);
    CHECK(halved > 0u, "no grid shrank");
    printf("plan ok %u (tiered %u)\n", cases, tiered);

    // the headline: k = 20 through the int8 copy on 256 CUs
    CHECK(tail_plan_first(20, 350, true, true) == 160u && tail_plan_slots(350, 160) == 161u &&
          tail_plan_workgroups(161, 1, 256, 1) == 11u && tail_plan_workgroups(351, 1, 256, 1) == 22u, "headline");
    // b = 0 is the launcher's early return; the plan still divides by nothing
    CHECK(tail_plan_workgroups(161, 0, 256, 1) == 1u, "b = 0");
    printf("headline ok\n");

    // the default rule is monotone in the rows: on up to its bound, off beyond
    bool was = true;
    for (uint64_t n = 64; n <= (1ull << 32); n <<= 1)
        for (uint32_t k : {1u, 20u, 50u, 87u}) {
            const bool on = tail_prefix_first_default(n, k);
            CHECK(on == (n <= kTailFirstMaxRows), "default at %llu rows k %u", (unsigned long long)n, k);
            if (k == 1u) { CHECK(was || !on, "default comes back on at %llu rows", (unsigned long long)n); was = on; }
        }
    CHECK(tail_prefix_first_default(1u << 20, 20) , "on at 1M rows");
    printf("default ok\n");
    if (g_fail) { printf("FAILED %d\n", g_fail); return 1; }
    printf("all ok\n");
    return 0;
}
