// tail_prefix_driver.cpp — stand-alone check of cqs_amd/csrc/tail_prefix.h (no device): the prefix certificate of the shadow
// search's tail against brute force, on random and adversarial lists.  Built with -fsanitize=address,undefined and run by
// tests/test_tail_prefix_cpu.py.  Prints one "name ok <cases>" line per group; any failure prints "FAIL ..." and exits 1.
//
// Model of one query: n rows, each with an approximate score a, an exact score s with |s - a| <= B (as real numbers) and a
// "dropped" flag (the f32 epilogue's: the row is not in the exact answer and its rescored key is 0).  The select hands over
// the top k' + 1 rows by (a, row); a finisher that sorts a prefix first - tail_prefix_first's, and every other length in steps -
// and tries the certificate on it must give the outputs of sorting all k' at once, and a certified answer must be the
// brute-force top k of the kept rows.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../cqs_amd/csrc/tail_prefix.h"

using namespace cqs;

static uint32_t okey(float s) {
    uint32_t b;
    memcpy(&b, &s, 4);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
static uint64_t pack(float s, uint32_t row) { return ((uint64_t)okey(s) << 32) | (0xFFFFFFFFu - row); }
static float clamp01(float t) { return t < 0.f ? 0.f : (t > 1.f ? 1.f : t); }

struct Query {
    std::vector<float> a, s;
    std::vector<char> dropped;
    float B;
    uint32_t mode, k, kprime;
};
struct Out {
    std::vector<uint64_t> keys;
    bool cert;
    uint32_t rescored;
    bool operator==(const Out& o) const { return keys == o.keys && cert == o.cert; }
};

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_fail; } } while (0)

// The select: approximate keys sorted descending, at most k' + 1 of them.
static std::vector<uint64_t> select_keys(const Query& q) {
    std::vector<uint64_t> ak;
    for (uint32_t i = 0; i < q.a.size(); ++i) ak.push_back(pack(q.a[i], i));
    std::sort(ak.begin(), ak.end(), std::greater<uint64_t>());
    if (ak.size() > q.kprime + 1u) ak.resize(q.kprime + 1u);
    return ak;
}
static uint64_t exact_key(const Query& q, uint64_t akey) {
    const uint32_t row = 0xFFFFFFFFu - (uint32_t)akey;
    return q.dropped[row] ? 0ull : pack(q.s[row], row);
}

// The finisher: round = 0: every candidate at once; 0xFFFFFFFF: the kernel's prefix (tail_prefix_first), then the rest; else
// prefixes growing by `round`.
static Out tail(const Query& q, const std::vector<uint64_t>& ak, uint32_t round) {
    const uint32_t ac = (uint32_t)ak.size(), nc = std::min(ac, q.kprime);
    std::vector<uint64_t> kept;
    Out o{{}, false, 0};
    uint32_t done = 0;
    for (;;) {
        uint32_t hi = (round == 0u || nc - done < round) ? nc : done + round;
        if (round == 0xFFFFFFFFu) hi = done == 0u ? tail_prefix_first(q.k, nc) : nc;
        for (uint32_t i = done; i < hi; ++i)
            if (const uint64_t e = exact_key(q, ak[i])) kept.push_back(e);
        std::sort(kept.begin(), kept.end(), std::greater<uint64_t>());
        done = hi;
        const uint32_t m = (uint32_t)kept.size();
        bool ok = false, stop = false;
        if (hi >= nc) {   // rules (a) / (b)
            stop = true;
            if (std::fabs(q.B) <= 3.4028234664e38f) {
                if (ac <= q.kprime) ok = true;
                else if (m >= q.k) ok = tail_prefix_certifies(ak[q.kprime], q.B, q.mode, tail_key_score(kept[q.k - 1]));
            }
        } else if (m >= q.k && tail_prefix_certifies(ak[hi], q.B, q.mode, tail_key_score(kept[q.k - 1]))) {
            stop = ok = true;
        }
        if (stop) {
            o.keys.assign(kept.begin(), kept.begin() + std::min(m, q.k));
            o.cert = ok;
            o.rescored = done;
            return o;
        }
    }
}

static std::vector<uint64_t> brute(const Query& q) {
    std::vector<uint64_t> all;
    for (uint32_t i = 0; i < q.s.size(); ++i)
        if (!q.dropped[i]) all.push_back(pack(q.s[i], i));
    std::sort(all.begin(), all.end(), std::greater<uint64_t>());
    if (all.size() > q.k) all.resize(q.k);
    return all;
}

// One query through every round size: same outputs as the full path; a certified answer is the brute-force one.
static void check(const Query& q, const char* what, uint32_t* prefix_certs, uint32_t* prefix_fails) {
    const std::vector<uint64_t> ak = select_keys(q);
    const Out full = tail(q, ak, 0);
    if (full.cert) CHECK(full.keys == brute(q), "%s: certified full answer differs from brute force", what);
    const uint32_t ncq = std::min<uint32_t>((uint32_t)ak.size(), q.kprime), j1 = tail_prefix_first(q.k, ncq);
    CHECK(j1 <= ncq && (j1 == ncq || j1 >= q.k), "prefix length %u of %u at k %u", j1, ncq, q.k);
    for (uint32_t round : {0xFFFFFFFFu, 1u, 7u, 16u, 32u, 64u, 128u}) {
        const Out r = tail(q, ak, round);
        CHECK(r == full, "%s: round %u k %u k' %u B %g mode %u: cert %d/%d, %zu/%zu keys, rescored %u", what, round, q.k, q.kprime,
              (double)q.B, q.mode, (int)r.cert, (int)full.cert, r.keys.size(), full.keys.size(), r.rescored);
        const uint32_t nc = std::min<uint32_t>((uint32_t)ak.size(), q.kprime);
        if (r.rescored < nc) ++*prefix_certs;
        else if (round == 0xFFFFFFFFu ? j1 < nc : nc > round) ++*prefix_fails;
    }
}

int main() {
    std::mt19937 rng(20250101);
    std::uniform_real_distribution<float> u01(0.f, 1.f);
    uint32_t pc = 0, pf = 0, cases = 0;

    // key_score inverts okey on every kind of float; the certificate's clamp
    for (float f : {0.f, -0.f, 1.f, -1.f, 0.148f, 1e-40f, -1e-40f, 3.4e38f, -3.4e38f, INFINITY, -INFINITY}) {
        uint32_t x, y;
        const float g = tail_key_score(pack(f, 5));
        memcpy(&x, &f, 4); memcpy(&y, &g, 4);
        CHECK(x == y, "key_score(%g)", (double)f);
    }
    CHECK(tail_prefix_certifies(pack(0.5f, 0), 0.25f, 0, 0.76f) && !tail_prefix_certifies(pack(0.5f, 0), 0.25f, 0, 0.75f), "strict");
    CHECK(!tail_prefix_certifies(pack(0.9f, 0), 0.5f, 1, 1.0f) && tail_prefix_certifies(pack(-3.f, 0), 0.5f, 1, 1e-30f), "clamp");
    CHECK(!tail_prefix_certifies(pack(-3.f, 0), 0.5f, 1, 0.f), "clamp at 0 is not below 0");
    printf("scalars ok\n");

    // the prefix length
    CHECK(tail_prefix_first(20, 350) == 160 && tail_prefix_first(20, 100) == 100 && tail_prefix_first(1, 160) == 46 &&
          tail_prefix_first(87, 1020) == 562 && tail_prefix_first(5, 0) == 0, "prefix length");
    for (uint32_t k = 1; k <= 1024; ++k) {
        const uint32_t kp = 2u * k + 32u < 1023u ? 2u * k + 32u : 1023u;
        CHECK(tail_prefix_first(k, kp) == kp, "the bf16 copy's k' leaves no proper prefix: k %u", k);
    }
    printf("rule ok\n");

    // random lists: gaussian-tailed scores, errors anywhere within the bound, RAW and PIPELINE, drops by a threshold
    for (int t = 0; t < 3000; ++t) {
        Query q;
        q.k = 1u + rng() % 24u;
        q.kprime = (t % 2) ? 10u * q.k + 150u : 2u * q.k + 32u;
        q.mode = t % 3 == 0 ? 1u : 0u;
        const uint32_t n = (t % 7 == 0) ? rng() % (q.kprime + 2u) : 400u + rng() % 600u;   // (n <= k': rule (a))
        q.B = (t % 11 == 0) ? 0.f : 0.02f * u01(rng) * u01(rng);
        if (t % 97 == 0) q.B = INFINITY;
        const float thr = q.mode ? 0.3f + 0.5f * u01(rng) : 0.f;
        std::normal_distribution<float> nd(0.3f, 0.2f);
        for (uint32_t i = 0; i < n; ++i) {
            const float a = nd(rng);
            const float Bf = std::isfinite(q.B) ? q.B : 0.01f;
            float s = a + Bf * (2.f * u01(rng) - 1.f) * 0.999f;
            if (std::fabs((double)s - (double)a) > (double)Bf) s = a;
            bool drop = false;
            if (q.mode) { s = clamp01(s); drop = !(s >= thr); }
            q.a.push_back(a); q.s.push_back(s); q.dropped.push_back(drop);
        }
        check(q, "random", &pc, &pf);
        ++cases;
    }
    printf("random ok %u (prefix certified %u, went on %u)\n", cases, pc, pf);
    CHECK(pc > 1000 && pf > 100, "both outcomes must occur: %u %u", pc, pf);

    // adversarial: errors at the bound's edge pushing outsiders up and insiders down; exact ties at the cut; B = 0;
    // all keys equal in score; a crowd within 2B below the k-th; the top-k approximate rows dropped
    cases = 0;
    for (int t = 0; t < 1500; ++t) {
        Query q;
        q.k = 1u + rng() % 20u;
        q.kprime = 10u * q.k + 150u;
        q.mode = (t % 5 == 4) ? 1u : 0u;
        const int kind = t % 5;
        q.B = kind == 1 ? 0.f : 0x1p-7f;
        const uint32_t n = 600;
        for (uint32_t i = 0; i < n; ++i) {
            float a, s;
            bool drop = false;
            if (kind == 0) {          // a descends by B / 8 per row: every error at the edge, signs alternating by blocks
                a = 0.9f - (float)i * (q.B / 8.f);
                s = (i / 3u) % 2u ? a + q.B : a - q.B;
                if (std::fabs((double)s - (double)a) > (double)q.B) s = a;
            } else if (kind == 1) {   // B = 0: s == a, runs of equal scores across the cut
                a = 0.5f - (float)(i / 9u) * 0x1p-10f;
                s = a;
            } else if (kind == 2) {   // all equal
                a = s = 0.25f;
            } else if (kind == 3) {   // k good rows, then a crowd of 150 within 2B below the k-th, then the rest
                a = i < q.k ? 0.8f : (i < q.k + 150u ? 0.8f - 2.f * q.B * u01(rng) : 0.5f * u01(rng));
                s = a + q.B * (2.f * u01(rng) - 1.f) * 0.99f;
                if (std::fabs((double)s - (double)a) > (double)q.B) s = a;
            } else {                  // PIPELINE: the best approximate rows fall under the threshold once exact
                a = 0.7f - (float)i * 0x1p-12f;
                s = clamp01(a - q.B * 0.99f * (i < 2u * q.k ? 1.f : -0.5f));
                if (std::fabs((double)s - (double)a) > (double)q.B) s = clamp01(a);
                drop = !(s >= 0.7f - q.B * 0.9f - (float)(t % 40) * 0x1p-9f);
            }
            q.a.push_back(a); q.s.push_back(s); q.dropped.push_back(drop);
        }
        std::vector<uint32_t> perm(n);   // row numbers in random order: ties are broken by row, not by position
        for (uint32_t i = 0; i < n; ++i) perm[i] = i;
        std::shuffle(perm.begin(), perm.end(), rng);
        Query p = q;
        for (uint32_t i = 0; i < n; ++i) { p.a[perm[i]] = q.a[i]; p.s[perm[i]] = q.s[i]; p.dropped[perm[i]] = q.dropped[i]; }
        check(p, "adversarial", &pc, &pf);
        ++cases;
    }
    printf("adversarial ok %u\n", cases);
    if (g_fail) { printf("FAILED %d\n", g_fail); return 1; }
    printf("all ok\n");
    return 0;
}
