// Stand-alone driver for the device-free rules of the host search path (cqs_amd/csrc/search_host.h).  Built with
// -fsanitize=address,undefined and run on the CPU by tests/test_search_host_cpu.py; every array is a heap block of exactly
// its documented length, so a read or write past it is an error.  Prints one line per case, fields separated by '|'.
#include <cfloat>
#include <cstdio>
#include <limits>
#include <memory>

#include "../cqs_amd/csrc/search_host.h"

using namespace cqs_search;

static const uint32_t kMaxK = 1024;

// plan_search over an index of n rows x 64: which pointers are null, and what became of the counts (prefilled with 7).
struct Nulls { bool queries, counts, keep, rows, scores; };
static void plan_case(const char* name, bool filtered, uint32_t b, Nulls nul, uint64_t n, uint32_t qdim, uint32_t k, uint32_t mode,
                      uint64_t stride) {
    std::unique_ptr<float[]> q(nul.queries ? nullptr : new float[(size_t)b * qdim]());
    std::unique_ptr<uint32_t[]> counts(nul.counts ? nullptr : new uint32_t[b]);
    std::unique_ptr<uint32_t[]> keep(nul.keep ? nullptr : new uint32_t[(size_t)b * stride]());
    std::unique_ptr<uint64_t[]> rows(nul.rows ? nullptr : new uint64_t[(size_t)b * k]());
    std::unique_ptr<float[]> scores(nul.scores ? nullptr : new float[(size_t)b * k]());
    for (uint32_t i = 0; counts && i < b; ++i) counts[i] = 7;
    Args a{q.get(), b, qdim, k, mode, rows.get(), scores.get(), counts.get(), filtered, keep.get(), stride};
    const char* why = "?";
    const Plan p = plan_search(a, n, 64, kMaxK, &why);
    uint32_t zero = 0, kept = 0;
    for (uint32_t i = 0; counts && i < b; ++i) { zero += counts[i] == 0; kept += counts[i] == 7; }
    const char* st = !counts || b == 0 ? "-" : (zero == b ? "zeroed" : (kept == b ? "untouched" : "mixed"));
    std::printf("%s_%s|%d|%s|%s\n", filtered ? "f" : "s", name, (int)p, st, why);
}

static void plan_cases(bool f) {
    const Nulls none{false, false, !f, false, false}, all{true, true, true, true, true};
    const Nulls no_out{false, false, !f, true, true};
    const uint32_t bad_mode = CQS_HIP_MODE_PIPELINE + 1;
    plan_case("b0_all_null", f, 0, all, 300, 64, 20, 0, 10);
    plan_case("b0_bad_everything", f, 0, all, 300, 48, kMaxK + 1, bad_mode, 0);
    plan_case("null_queries", f, 3, Nulls{true, false, !f, false, false}, 300, 64, 20, 0, 10);
    plan_case("null_counts", f, 3, Nulls{false, true, !f, false, false}, 300, 64, 20, 0, 10);
    plan_case("null_queries_k_over", f, 3, Nulls{true, false, !f, false, false}, 300, 64, kMaxK + 1, 0, 10);
    if (f) plan_case("null_keep", f, 3, Nulls{false, false, true, false, false}, 300, 64, 20, 0, 10);
    if (f) plan_case("null_keep_k0", f, 3, Nulls{false, false, true, false, false}, 300, 64, 0, 0, 10);
    plan_case("k0_null_out", f, 3, no_out, 300, 64, 0, 0, 10);
    plan_case("k0_dim_mismatch", f, 3, none, 300, 48, 0, 0, 10);
    plan_case("k0_short_stride", f, 3, none, 300, 64, 0, 0, 9);
    plan_case("n0_k_over", f, 3, no_out, 0, 64, kMaxK + 1, 0, 0);
    plan_case("dim_mismatch", f, 3, none, 300, 48, 20, 0, 10);
    plan_case("dim_mismatch_k_over", f, 3, no_out, 300, 48, kMaxK + 1, bad_mode, 10);
    plan_case("k_max", f, 2, none, 300, 64, kMaxK, 0, 10);
    plan_case("k_over", f, 2, none, 300, 64, kMaxK + 1, 0, 10);
    plan_case("k_over_bad_mode", f, 2, no_out, 300, 64, kMaxK + 1, bad_mode, 10);
    plan_case("bad_mode", f, 3, none, 300, 64, 20, bad_mode, 10);
    plan_case("bad_mode_null_out", f, 3, no_out, 300, 64, 20, bad_mode, 9);
    plan_case("pipeline_mode", f, 3, none, 300, 64, 20, CQS_HIP_MODE_PIPELINE, 10);
    plan_case("null_rows", f, 3, Nulls{false, false, !f, true, false}, 300, 64, 20, 0, 10);
    plan_case("null_scores", f, 3, Nulls{false, false, !f, false, true}, 300, 64, 20, 0, 10);
    plan_case("null_out_short_stride", f, 3, no_out, 300, 64, 20, 0, 9);
    plan_case("short_stride", f, 3, none, 300, 64, 20, 0, 9);      // the plain variant has no stride: Run
    plan_case("exact_stride", f, 3, none, 300, 64, 20, 0, 10);
    plan_case("one_row", f, 1, none, 1, 64, 1, 0, 1);
}

static uint64_t count_bit_by_bit(const uint32_t* w, uint64_t first, uint64_t nbits) {
    uint64_t c = 0;
    for (uint64_t i = first; i < first + nbits; ++i) c += (w[i / 32] >> (i % 32)) & 1u;
    return c;
}

// plan_keep over n rows: ceil(n/32) words exactly; `garbage` sets every bit past n in the last word.
static void keep_case(const char* name, uint64_t n, int fill, bool three) {
    const size_t words = (size_t)((n + 31) / 32);
    std::unique_ptr<uint32_t[]> w(new uint32_t[words]);
    for (size_t i = 0; i < words; ++i) w[i] = fill ? 0xFFFFFFFFu : 0u;
    if (!fill && n % 32) w[words - 1] = ~((1u << (n % 32)) - 1u);               // garbage past n only
    if (three) for (uint64_t r : {(uint64_t)0, n / 2, n - 1}) w[r / 32] |= 1u << (r % 32);
    uint32_t k_eff = 20;
    const Keep p = plan_keep(w.get(), n, &k_eff);
    std::printf("%s_%llu|%d|%u|%llu|%llu\n", name, (unsigned long long)n, (int)p, k_eff,
                (unsigned long long)popcount_bits(w.get(), 0, n), (unsigned long long)count_bit_by_bit(w.get(), 0, n));
}

static void keep_cases() {
    for (uint64_t n : {1, 31, 32, 33, 300}) {
        keep_case("keep_ones", n, 1, false);
        keep_case("keep_zero", n, 0, false);
        if (n >= 4) keep_case("keep_three", n, 0, true);
    }
    uint32_t k_eff = 20;
    std::printf("keep_null|%d|%u\n", (int)plan_keep(nullptr, 300, &k_eff), k_eff);
    // a shard's part of a global bitset: rows [256, 300) of 300 (10 words), then a whole number of words of a 9-word block
    std::unique_ptr<uint32_t[]> g(new uint32_t[10]);
    for (uint32_t i = 0; i < 10; ++i) g[i] = 0x9E3779B9u * (i + 1);
    std::printf("shard_256_44|%llu|%llu\n", (unsigned long long)popcount_bits(g.get(), 256, 44), (unsigned long long)count_bit_by_bit(g.get(), 256, 44));
    std::printf("shard_0_256|%llu|%llu\n", (unsigned long long)popcount_bits(g.get(), 0, 256), (unsigned long long)count_bit_by_bit(g.get(), 0, 256));
    std::unique_ptr<uint32_t[]> h(new uint32_t[9]);
    for (uint32_t i = 0; i < 9; ++i) h[i] = 0x85EBCA6Bu * (i + 3);
    std::printf("shard_256_32|%llu|%llu\n", (unsigned long long)popcount_bits(h.get(), 256, 32), (unsigned long long)count_bit_by_bit(h.get(), 256, 32));
    std::printf("shard_288_0|%llu\n", (unsigned long long)popcount_bits(h.get(), 288, 0));
}

static void stage_case(const char* name, uint32_t at, float v) {
    const uint32_t dim = 8;
    std::unique_ptr<float[]> src(new float[dim]), dst(new float[dim]);
    for (uint32_t d = 0; d < dim; ++d) { src[d] = 0.25f * (float)(d + 1) - 1.0f; dst[d] = 5.0f; }
    if (at < dim) src[at] = v;
    const bool ok = stage_query(dst.get(), src.get(), dim);
    bool same = true, zero = true;
    for (uint32_t d = 0; d < dim; ++d) { same &= memcmp(&dst[d], &src[d], 4) == 0; zero &= dst[d] == 0.0f && !std::signbit(dst[d]); }
    std::printf("%s|%d|%s|%d\n", name, (int)ok, same ? "copied" : (zero ? "zero" : "other"), (int)query_finite(src.get(), dim));
}

static void drop_case(const char* name, std::initializer_list<uint64_t> rows_in, std::initializer_list<float> scores_in, uint64_t target,
                      uint32_t limit) {
    const uint32_t cnt = (uint32_t)rows_in.size();
    std::unique_ptr<uint64_t[]> rows(new uint64_t[cnt]), out_rows(new uint64_t[limit]);
    std::unique_ptr<float[]> scores(new float[cnt]), out_scores(new float[limit]);
    uint32_t i = 0;
    for (uint64_t r : rows_in) rows[i++] = r;
    i = 0;
    for (float s : scores_in) scores[i++] = s;
    const uint32_t c = drop_self(rows.get(), scores.get(), cnt, target, limit, out_rows.get(), out_scores.get());
    std::printf("%s|%u|", name, c);
    for (i = 0; i < c; ++i) std::printf("%s%llu:%g", i ? "," : "", (unsigned long long)out_rows[i], (double)out_scores[i]);
    std::printf("\n");
}

static void neighbors_cases() {
    const uint32_t limits[] = {0, 1, 5, 99, 100, 101, 1000, 0xFFFFFFFFu};
    const uint64_t ns[] = {0, 1, 2, 6, 101, 300};
    for (uint64_t n : ns)
        for (uint32_t l : limits) {
            uint32_t limit = l;
            const uint32_t k = neighbors_k(&limit, n);
            std::printf("nk_%u_%llu|%u|%u\n", l, (unsigned long long)n, limit, k);
        }
    drop_case("drop_first", {4, 9, 2, 7}, {1.0f, 0.8f, 0.6f, 0.4f}, 4, 3);
    drop_case("drop_middle", {9, 2, 4, 7}, {0.9f, 0.8f, 0.7f, 0.4f}, 4, 3);
    drop_case("drop_last", {9, 2, 7, 4}, {0.9f, 0.8f, 0.7f, 0.4f}, 4, 3);
    drop_case("drop_absent", {9, 2, 7, 5}, {0.9f, 0.8f, 0.7f, 0.4f}, 4, 3);         // cut to limit
    drop_case("drop_tie", {4, 3, 8, 6}, {1.0f, 0.5f, 0.5f, 0.25f}, 4, 3);           // a duplicate SCORE on other rows: both stay
    drop_case("drop_short", {4, 9}, {1.0f, 0.5f}, 4, 100);
    drop_case("drop_none", {}, {}, 4, 1);
}

static uint64_t pack(float s, uint32_t row) {   // the select kernels' key: order-preserving score bits, then 0xFFFFFFFF - row
    uint32_t b;
    memcpy(&b, &s, 4);
    const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)o << 32) | (uint64_t)(0xFFFFFFFFu - row);
}

static void merge_case(const char* name, size_t n_lists, size_t stride, std::initializer_list<uint32_t> counts_in, const uint64_t* flat,
                       size_t k) {
    std::unique_ptr<uint32_t[]> counts(new uint32_t[n_lists]);
    size_t i = 0, last = 0;
    for (uint32_t c : counts_in) { counts[i++] = c; last = c; }
    const size_t len = n_lists ? (n_lists - 1) * stride + last : 0;    // the last list ends at its count
    std::unique_ptr<uint64_t[]> lists(new uint64_t[len]), out(new uint64_t[k]);
    for (i = 0; i < len; ++i) lists[i] = flat[i];
    const size_t m = merge_keys(n_lists ? lists.get() : nullptr, n_lists ? counts.get() : nullptr, n_lists, stride, k, out.get());
    std::unique_ptr<uint64_t[]> rows(new uint64_t[m]);
    unpack_keys(out.get(), m, rows.get(), nullptr);
    std::printf("%s|%zu|", name, m);
    for (i = 0; i < m; ++i) std::printf("%s%llu", i ? "," : "", (unsigned long long)rows[i]);
    std::printf("\n");
}

static void key_cases() {
    const float vals[] = {0.0f, -0.0f, -1.5f, std::numeric_limits<float>::denorm_min(), FLT_MAX, -FLT_MAX, 0.73f};
    const uint32_t rws[] = {0, 1, 299, 0xFFFFFFFEu, 7, 0x80000000u, 12345};
    const size_t n = sizeof vals / sizeof vals[0];
    std::unique_ptr<uint64_t[]> keys(new uint64_t[n]), rows(new uint64_t[n]);
    std::unique_ptr<float[]> scores(new float[n]);
    for (size_t i = 0; i < n; ++i) keys[i] = pack(vals[i], rws[i]);
    unpack_keys(keys.get(), n, rows.get(), scores.get());
    bool ok = true;
    for (size_t i = 0; i < n; ++i) ok &= memcmp(&scores[i], &vals[i], 4) == 0 && rows[i] == rws[i];
    unpack_keys(keys.get(), n, nullptr, scores.get());
    unpack_keys(keys.get(), n, rows.get(), nullptr);
    unpack_keys(nullptr, 0, nullptr, nullptr);
    for (size_t i = 0; i < n; ++i) ok &= memcmp(&scores[i], &vals[i], 4) == 0 && rows[i] == rws[i];
    std::printf("roundtrip|%s\n", ok ? "exact" : "differs");
    std::printf("key_order|%d\n", (int)(pack(0.5f, 3) > pack(0.5f, 8) && pack(0.5f, 8) > pack(0.25f, 0) && pack(-1.0f, 0) > pack(-2.0f, 0)));
    // three descending lists, stride 4; 0.9 and 0.5 are tied across lists: the smaller row wins
    const uint64_t z = 0;
    const uint64_t flat[] = {pack(0.9f, 5), pack(0.5f, 7), z, z, pack(0.9f, 2), pack(0.5f, 1), z, z, pack(0.7f, 9)};
    merge_case("merge_k4", 3, 4, {2, 2, 1}, flat, 4);
    merge_case("merge_k_large", 3, 4, {2, 2, 1}, flat, 10);
    merge_case("merge_k0", 3, 4, {2, 2, 1}, flat, 0);
    merge_case("merge_zero_counts", 3, 4, {0, 0, 0}, flat, 5);
    merge_case("merge_middle_empty", 3, 4, {2, 0, 1}, flat, 5);
    merge_case("merge_no_lists", 0, 4, {}, flat, 5);
}

static void error_case(size_t cap) {
    const char text[] = "search: k > max_k";
    const size_t len = sizeof text - 1;
    std::unique_ptr<char[]> msg(new char[len]), buf(new char[cap]);
    memcpy(msg.get(), text, len);                                  // no terminator behind the message
    const size_t m = copy_last_error(msg.get(), len, buf.get(), cap);
    std::printf("error_cap_%zu|%zu|%s\n", cap, m, buf.get());
}

int main() {
    plan_cases(false);
    plan_cases(true);
    keep_cases();
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    stage_case("stage_finite", 99, 0.f);
    stage_case("stage_extremes", 3, -FLT_MAX);
    stage_case("stage_nan_first", 0, nan);
    stage_case("stage_nan_last", 7, nan);
    stage_case("stage_inf_first", 0, inf);
    stage_case("stage_inf_last", 7, inf);
    stage_case("stage_ninf_first", 0, -inf);
    stage_case("stage_ninf_last", 7, -inf);
    neighbors_cases();
    key_cases();
    for (size_t cap : {1, 2, 17, 18, 100}) error_case(cap);
    return 0;
}
