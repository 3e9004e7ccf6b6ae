// Stand-alone driver for the device-free part of cqs_hip_index_pairwise / cqs_hip_index_mmr (cqs_amd/csrc/mmr_host.h):
// argument checks and the answers mmr.rs:64-69 gives without a loop.  Built with -fsanitize=address,undefined and run on
// the CPU by tests/test_mmr_cpu.py; every array is a heap block of exactly its length, so a read past m is an error.
// Prints one line per case: "<name> <plan> <limit> <lambda>".
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>

#include "../cqs_amd/csrc/mmr_host.h"

using cqs_mmr::Plan;

static void mmr_case(const char* name, uint32_t m, bool rows_null, bool scores_null, uint64_t row_base, uint64_t n, uint32_t limit,
                     float lambda, int64_t bad_row_at, float bad_score) {
    std::unique_ptr<uint64_t[]> rows(m && !rows_null ? new uint64_t[m] : nullptr);
    std::unique_ptr<float[]> scores(m && !scores_null ? new float[m] : nullptr);
    for (uint32_t i = 0; rows && i < m; ++i) rows[i] = row_base + (i * 7u) % (n ? n : 1);
    for (uint32_t i = 0; scores && i < m; ++i) scores[i] = 1.0f - (float)i / 2048.0f;
    if (rows && bad_row_at >= 0) rows[bad_row_at] = row_base + n;
    if (rows && bad_row_at == -2) rows[m - 1] = row_base - 1;
    if (scores && !std::isnan(bad_score)) scores[m / 2] = bad_score;
    const char* why = "";
    const Plan p = cqs_mmr::plan_mmr(rows.get(), scores.get(), m, row_base, n, &limit, &lambda, &why);
    std::printf("%s %d %u %g %s\n", name, (int)p, limit, (double)lambda, p == Plan::Invalid ? why : "-");
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    mmr_case("device", 500, false, false, 1000003, 2048, 20, 0.7f, -1, nan);
    mmr_case("clamp_low", 33, false, false, 0, 2048, 5, -3.0f, -1, nan);
    mmr_case("clamp_high", 33, false, false, 0, 2048, 5, 7.0f, -1, nan);
    mmr_case("lambda_one", 33, false, false, 0, 2048, 5, 1.0f, -1, nan);
    mmr_case("limit_zero", 33, false, false, 0, 2048, 0, 0.5f, -1, nan);
    mmr_case("empty", 0, true, true, 0, 2048, 5, 0.5f, -1, nan);
    mmr_case("limit_ge_m", 33, false, false, 0, 2048, 33, 0.5f, -1, nan);
    mmr_case("limit_huge", 33, false, false, 0, 2048, 0xFFFFFFFFu, 0.5f, -1, nan);
    mmr_case("m_max", 1024, false, false, 0, 2048, 100, 0.5f, -1, nan);
    mmr_case("m_over", 1025, false, false, 0, 2048, 100, 0.5f, -1, nan);
    mmr_case("nan_lambda", 33, false, false, 0, 2048, 5, nan, -1, nan);
    mmr_case("inf_lambda", 33, false, false, 0, 2048, 5, inf, -1, nan);
    mmr_case("inf_score", 33, false, false, 0, 2048, 5, 0.5f, -1, inf);
    mmr_case("ninf_score", 33, false, false, 0, 2048, 5, 0.5f, -1, -inf);
    mmr_case("row_past_end", 33, false, false, 1000003, 2048, 5, 0.5f, 32, nan);
    mmr_case("row_below_base", 33, false, false, 1000003, 2048, 5, 0.5f, -2, nan);
    mmr_case("bad_row_identity", 33, false, false, 0, 2048, 5, 1.0f, 0, nan);
    mmr_case("null_rows", 33, true, false, 0, 2048, 5, 0.5f, -1, nan);
    mmr_case("null_scores", 33, false, true, 0, 2048, 5, 0.5f, -1, nan);
    mmr_case("empty_index", 1, false, false, 0, 0, 1, 0.5f, -1, nan);
    // pairwise's check alone
    {
        std::unique_ptr<uint64_t[]> rows(new uint64_t[3]{5, 5, 9});
        const char* why = "";
        std::printf("pairwise_ok %d\n", (int)cqs_mmr::check_rows(rows.get(), 3, 5, 5, &why));
        std::printf("pairwise_past %d\n", (int)cqs_mmr::check_rows(rows.get(), 3, 5, 4, &why));
        std::printf("pairwise_empty %d\n", (int)cqs_mmr::check_rows(nullptr, 0, 5, 4, &why));
        std::printf("pairwise_null %d\n", (int)cqs_mmr::check_rows(nullptr, 3, 5, 4, &why));
    }
    return 0;
}
