// tail_prefix.h — the prefix certificate of the shadow search's tail ("Prefix certificate").  Header-only
// and host-and-device, so the tail kernel (scan_bf16.hip) and a CPU test (tests/tail_prefix_driver.cpp) run the same
// functions.
//
// a_1 >= a_2 >= ... are the approximate scores of the select's sorted keys, B = B_q >= 0 with |s_i - a_i| <= B for every
// finite row (s_i the exact f32 score, after the epilogue's clamp in PIPELINE mode, where the clamp is applied to a_i + B
// as well).  For any prefix j < count: rescore candidates 1..j and take s_(k)(j), the k-th largest kept exact score among
// them.  If at least k were kept and clamp(a_(j+1) + B) < s_(k)(j), then every row outside the prefix has
// s <= clamp(a + B) <= clamp(a_(j+1) + B) < s_(k)(j): the prefix's top k is the corpus' top k.  s_(k)(j) only grows with j
// and a_(j+1) only shrinks, so a prefix that certifies implies that every longer one does, with the same top k.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CQS_TP_HD __host__ __device__
#else
#define CQS_TP_HD
#endif

namespace cqs {

// The score of a packed key: the inverse of okey on the key's top half (scan_device.h).
CQS_TP_HD inline float tail_key_score(uint64_t key) {
    const uint32_t ok = (uint32_t)(key >> 32);
    const uint32_t bits = (ok & 0x80000000u) ? (ok ^ 0x80000000u) : ~ok;
    float f;
    memcpy(&f, &bits, sizeof f);
    return f;
}

// The certificate's inequality for the prefix that ends just before `key_next` (the first approximate key outside it):
// no row at or below that key can reach s_k, the k-th largest kept exact score inside the prefix.  B must be finite.
CQS_TP_HD inline bool tail_prefix_certifies(uint64_t key_next, float B, uint32_t mode, float s_k) {
    float t = tail_key_score(key_next) + B;
    if (mode == 1u) t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);   // PIPELINE: exact scores are clamped to [0, 1]
    return t < s_k;
}

// How many of the nc = min(count, k') rescored candidates the tail kernel's finisher sorts first: the rank sort is quadratic in
// what it sorts, and most of the k' are never needed.  The prefix a query needs is about #{a_i >= a_k - B}; measured on the
// int8 copy (the wider bound) over Gaussian unit rows at 1M and 10M x 768 it was at most 42 / 86 / 226 / 424 at k = 1 / 5 / 20 /
// 50, and 6k + 40 covers the p99 at 1M (28 / 57 / 148 / 306).  A query that needs more pays a second sort, not its answer.
// Only the int8 copy's k' = 10k + 150 leaves room for a proper prefix: the bf16 copy's k' = 2k + 32 is below 6k + 40 at every
// k, so there the result is nc and the finisher sorts once, as before.
CQS_TP_HD inline uint32_t tail_prefix_first(uint32_t k, uint32_t nc) {
    const uint32_t j = 6u * k + 40u;
    return j < nc ? j : nc;
}

}  // namespace cqs
