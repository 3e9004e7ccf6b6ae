// sparse_geometry.h — everything the sparse index derives from its chunk count and its list lengths: the padded row, the
// chunks a wave owns, the select's group size, and which lists get a range directory.  Plain C++, no HIP: the constructors
// (sparse_index_create.hip, finish_create) and the in-place updates (sparse_index_update.hip) derive it with this one code,
// so an updated handle has the geometry a fresh create of the same documents would have.  Also the constants and the
// resolved query term that the host headers (sparse_build_host.h) share with the scoring kernel.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace cqs {

constexpr uint32_t kSparsePad = 1024;                  // n_pad granule (a multiple of every wave range)
constexpr unsigned long long kNoDir = ~0ull;           // a list without a range directory: the wave bisects it
constexpr uint64_t kSparseMaxChunks = 0xFFFFFFFFull - kSparsePad;   // create refuses n >= this
constexpr uint32_t kUnscored = 0xFFFFFFFFu;    // LDS marker: `scores.entry(chunk)` does not exist yet (a NaN bit pattern: weights that
                                               // carry it are refused at build / search, a sum that lands on it is stored as 0x7FC00000)
constexpr uint32_t kMaxTerms = 1u << 16;        // per query
constexpr uint32_t kSparseMaxBatch = 64;       // queries per cqs_hip_sparse_index_search_batch call

struct SparseTerm {            // one query term, resolved on the host
    unsigned long long start;  // first posting of the token's list
    unsigned long long dir;    // first entry of the list's range directory (kNoDir: none - the wave bisects the list)
    uint32_t len;              // postings in the list
    float w;                   // query weight
};

struct SparseGeometry {
    uint32_t n_pad, rw, sh;
    bool group16;
};

inline SparseGeometry sparse_geometry(uint64_t n, uint32_t n_cu) {
    SparseGeometry g{};
    g.n_pad = (uint32_t)((n + kSparsePad - 1) / kSparsePad * kSparsePad);
    if (g.n_pad == 0) g.n_pad = kSparsePad;
    // chunks per wave: enough waves to keep ~16 per CU in flight, 64 ... 1024 chunks each
    g.rw = 1024;
    while (g.rw > 64u && g.n_pad / g.rw < n_cu * 16u) g.rw >>= 1;
    g.sh = 0;
    while ((1u << g.sh) < g.rw) ++g.sh;
    // measured (select at k = 500): 20k chunks 40 -> 24 us, 100k 29 -> 23, 1M 29 -> 45: 16-chunk groups while their maxima fit
    // one pass of the select's workgroup (1024 threads x 16 registers)
    g.group16 = g.n_pad / 16u <= 16384u;
    return g;
}

// Range directories: dir[r] = how many postings of the list sit below position r * rw, r = 0 .. n_pad / rw - what a wave
// needs to find its slice of the list with two adjacent loads.  Longest lists first, within a budget of entries equal
// to the postings' own bytes (2 P entries x 4 B = P x 8 B; never less than 64 MB.  Round 4's floor was 256 MB: a 100k-chunk
// index with a 30k-token vocabulary paid 192 MB of directories - and the same again as a host staging vector - for
// 80 MB of postings): at 1M chunks rw = 128, so a list's directory is 7 813 + 1 entries and the ~25 k longest
// lists of a 96 M-posting index get one; lists left without (shorter than kDirMinLen, or past the budget) are bisected.
// -> the directories' total entries; (*dir_off)[t] = list t's first entry, kNoDir = none.  `off` has one entry per list + 1.
inline uint64_t sparse_plan_directories(const std::vector<uint64_t>& off, const SparseGeometry& g, std::vector<uint64_t>* dir_off) {
    constexpr uint64_t kDirMinLen = 32;
    const size_t lists = off.empty() ? 0 : off.size() - 1;
    const uint64_t P = off.empty() ? 0 : off.back();
    const uint64_t R1 = (uint64_t)(g.n_pad / g.rw) + 1;
    const uint64_t budget = std::max<uint64_t>(16ull << 20, 2ull * P);
    dir_off->assign(lists, kNoDir);
    std::vector<uint32_t> order;
    for (size_t t = 0; t < lists; ++t)
        if (off[t + 1] - off[t] >= kDirMinLen) order.push_back((uint32_t)t);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const uint64_t lx = off[x + 1] - off[x], ly = off[y + 1] - off[y];
        return lx != ly ? lx > ly : x < y;
    });
    uint64_t used = 0;
    for (uint32_t t : order) {
        if (used + R1 > budget || off[t + 1] - off[t] > 0xFFFFFFFFull) break;
        (*dir_off)[t] = used;
        used += R1;
    }
    return used;
}

}  // namespace cqs
