// tags_host.h — the device-free part of the row tags: the per-row rule that tags_keep_kernel computes,
// the all-pass test, the range rules of set_tags, the keep rule over a kept-row COUNT (plan_keep's twin for a bitset that
// only exists on the device), where the tagged prefix ends after a removal, and the transposed table of up to 32 filters
// with the verdict word tags_keep_multi_kernel looks up in it (§3.14a).  Plain C++ over the caller's arrays, no HIP,
// no handle: index_tags.hip, index_remove.hip and the sparse index call it under their mutexes, the kernels call tag_kept
// and tag_verdicts, tests/tags_host_driver.cpp and tests/tags_multi_host_driver.cpp run all of it under ASAN + UBSan on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "search_host.h"

#if defined(__HIPCC__)
#define CQS_TAGS_HD __host__ __device__
#else
#define CQS_TAGS_HD
#endif

namespace cqs_tags {

constexpr uint32_t kFields = 4;                     // 8-bit fields of a tag: field f = (tag >> 8 f) & 255
constexpr uint32_t kWordsPerField = 8;              // a field's 256-bit set of allowed values
constexpr uint32_t kAllowWords = kFields * kWordsPerField;   // the filter: 32 words, 128 bytes

// The whole rule.  A row is kept iff, for every field, the bit named by the row's field value is set: bit v of field f's
// set is bit v % 32 of word 8 f + v / 32.  `allow` holds kAllowWords words (host memory on the host, LDS in the kernel).
CQS_TAGS_HD inline bool tag_kept(uint32_t tag, const uint32_t* allow) {
    uint32_t keep = 1u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t f = 0; f < kFields; ++f) {
        const uint32_t v = (tag >> (8u * f)) & 255u;
        keep &= allow[kWordsPerField * f + (v >> 5)] >> (v & 31u);
    }
    return (keep & 1u) != 0u;
}

// No field is constrained: the filter keeps every row whatever its tag, and the search is the unfiltered one.
inline bool all_pass(const uint32_t* allow) {
    uint32_t a = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < kAllowWords; ++i) a &= allow[i];
    return a == 0xFFFFFFFFu;
}

enum class Set : int32_t {
    Invalid = -1,   // CQS_HIP_ERR_INVALID; *why says which rule; nothing planned
    Nothing = 0,    // m == 0: CQS_HIP_OK, the handle stays as it is
    Write = 1,      // tags go to local rows [*first_local, *first_local + m); the prefix becomes *new_tagged rows
};

// set_tags' arguments against an index of `len` rows from `row_base` whose first `tagged` rows have a tag.  The tagged rows
// stay a prefix: a call may overwrite inside it and / or extend it, never leave a gap, never reach past the index.
inline Set plan_set_tags(uint64_t first_row, const uint32_t* tags, uint64_t m, uint64_t row_base, uint64_t len, uint64_t tagged,
                         uint64_t* first_local, uint64_t* new_tagged, const char** why) {
    *first_local = 0;
    *new_tagged = tagged;
    if (m == 0) return Set::Nothing;
    if (!tags) { *why = "null tags"; return Set::Invalid; }
    if (first_row < row_base) { *why = "first row below this index"; return Set::Invalid; }
    const uint64_t local = first_row - row_base;
    if (local > tagged) { *why = "gap: first row past the tagged rows"; return Set::Invalid; }
    if (m > len - local) { *why = "range past the end of the index"; return Set::Invalid; }   // (local <= tagged <= len)
    *first_local = local;
    *new_tagged = std::max(tagged, local + m);
    return Set::Write;
}

// plan_keep (search_host.h) for a bitset nobody popcounts on the host: `included` is the kernel's exact count of kept rows
// among the index's n.  Same three answers, same k_eff.
inline cqs_search::Keep plan_keep_count(uint64_t included, uint64_t n, uint32_t* k_eff) {
    if (included == 0) return cqs_search::Keep::Empty;
    if (included >= n) return cqs_search::Keep::Unfiltered;
    if (included < *k_eff) *k_eff = (uint32_t)included;
    return cqs_search::Keep::Filtered;
}

// The tagged prefix after the local rows removed[0 .. count) (distinct, ascending) left an index whose first `tagged` rows
// had a tag: the survivors keep their order, so it shrinks by the removed rows that lay inside it.
template <typename Id>
inline uint64_t tagged_after_remove(const Id* removed, size_t count, uint64_t tagged) {
    const size_t below = (size_t)(std::lower_bound(removed, removed + count, tagged,
                                                   [](const Id& r, uint64_t t) { return (uint64_t)r < t; }) - removed);
    return tagged - below;
}

// ---- up to 32 filters at once (tags_keep_multi_kernel) ----------------------------------------------
constexpr uint32_t kMaxFilters = 32;                // filters per table = bits of a verdict word (= cqs_idx::kCombineCap)
constexpr uint32_t kTableWords = kFields * 256;     // tbl[field][value]: 4 KB

// The filters transposed: bit j of tbl[256 fld + v] is set iff filter j (the 32 words at allows + 32 j) allows value v in
// field fld; bits >= f are zero.  1 <= f <= kMaxFilters.  Per (field, word of the sets) one 32 x 32 bit-matrix transpose
// (row j = filter j's word, zero from f on): five masked swap rounds instead of 32 K single-bit moves.
inline void transpose_filters(const uint32_t* allows, uint32_t f, uint32_t* tbl) {
    for (uint32_t w = 0; w < kAllowWords; ++w) {            // w = 8 fld + v / 32, and tbl's index is 32 w + v % 32
        uint32_t a[32];
        for (uint32_t j = 0; j < 32; ++j) a[j] = j < f ? allows[(size_t)kAllowWords * j + w] : 0u;
        uint32_t m = 0x0000FFFFu;
        for (uint32_t s = 16; s != 0; s >>= 1, m ^= m << s)
            for (uint32_t r = 0; r < 32; r = (r + s + 1) & ~s) {
                const uint32_t t = ((a[r] >> s) ^ a[r + s]) & m;     // swap (rows r.., columns +s) with (rows r + s.., columns +0)
                a[r] ^= t << s;
                a[r + s] ^= t;
            }
        for (uint32_t v = 0; v < 32; ++v) tbl[32u * w + v] = a[v];
    }
}

// A row's verdicts under all the filters of a table: bit j = tag_kept(tag, filter j).  Four lookups, however many filters.
CQS_TAGS_HD inline uint32_t tag_verdicts(uint32_t tag, const uint32_t* tbl) {
    return tbl[tag & 255u] & tbl[256u + ((tag >> 8) & 255u)] & tbl[512u + ((tag >> 16) & 255u)] & tbl[768u + (tag >> 24)];
}

// The bitset tags_keep_kernel writes for n rows, on the host: ceil(n / 32) words, bits past n are 0.  Returns the kept rows.
inline uint64_t keep_words(const uint32_t* tags, uint64_t n, const uint32_t* allow, uint32_t* out_words) {
    uint64_t kept = 0;
    for (uint64_t w = 0; w < (n + 31) / 32; ++w) out_words[w] = 0u;
    for (uint64_t i = 0; i < n; ++i)
        if (tag_kept(tags[i], allow)) { out_words[i >> 5] |= 1u << (i & 31u); ++kept; }
    return kept;
}

}  // namespace cqs_tags
