// i8_sweep.h — the order in which the int8 scan's workgroups sweep the copy, and which of them load plainly (DESIGN.md
// §3.11, "Serpentine sweep").  Consecutive searches sweep the copy in alternating directions: launched workgroup i takes the
// tasks of workgroup n_wg - 1 - i when the search's parity is set, so a search starts in the rows the one before it read
// last.  Those rows can only be found in the Infinity Cache if they were loaded in a way that allocates there, so the
// workgroups whose rows lie within `w` bytes of either end of the copy use plain loads and the rest stay nontemporal.
// Header-only and host-and-device, so the scan, its launcher and a CPU test (tests/i8_sweep_driver.cpp) run the same functions.
#pragma once
#include "group_map.h"

namespace cqs {

// Plain-load bytes at each end of an int8 copy that scans nontemporally (CQS_HIP_I8_SERPENTINE unset or 1).  Measured at
// 1M x 768 (profiles/i8_serpentine_pmc.txt): 64 / 128 / 192 MiB took 2.5 / 3.8 / 3.0 us off a 117.5 us scan.  Half the
// Infinity Cache: a line `d` bytes from the turning point is read again after 2 d bytes of scan traffic.
constexpr uint64_t kI8PlainBytes = 128ull << 20;

// The workgroup whose tasks launched workgroup `i` of `n_wg` takes: a bijection of [0, n_wg) for either parity.
CQS_GM_HD inline uint32_t sweep_group(uint32_t i, uint32_t n_wg, uint32_t rev) { return rev ? n_wg - 1u - i : i; }

// Workgroups [0, lo) and [hi, n_wg) load plainly (lo > hi: every one does).
struct PlainWindow {
    uint32_t lo, hi;
    CQS_GM_HD bool plain(uint32_t g) const { return g < lo || g >= hi; }
};

// Bytes [begin, end) of the copy that workgroup g of `m` (G = 4) reads: its rows below n, `dim` bytes each.  A workgroup
// whose rows all lie in the padding reads nothing: [n dim, n dim).
inline void sweep_bytes(const GroupMap& m, uint32_t g, uint32_t n, uint32_t dim, uint64_t& begin, uint64_t& end) {
    uint32_t rows;
    const uint32_t first = m.locate(g, rows);
    const uint64_t lo = first < n ? first : n, hi = (uint64_t)first + rows < n ? (uint64_t)first + rows : n;
    begin = lo * dim;
    end = hi * dim;
}

// Exactly the workgroups whose bytes intersect the first or the last `w` bytes of the n x dim copy load plainly.  Both
// conditions are monotone in g (begin and end never decrease), so each edge is one binary search.  w = 0: none;
// w >= n dim: every workgroup that reads anything.
inline PlainWindow plain_window(const GroupMap& m, uint32_t n, uint32_t dim, uint64_t w) {
    const uint32_t n_wg = m.total();
    const uint64_t total = (uint64_t)n * dim;
    if (w > total) w = total;
    uint64_t b, e;
    uint32_t a = 0u, z = n_wg;   // lo = the first g with begin(g) >= w
    while (a < z) {
        const uint32_t mid = a + (z - a) / 2u;
        sweep_bytes(m, mid, n, dim, b, e);
        if (b < w) a = mid + 1u; else z = mid;
    }
    const uint32_t lo = a;
    a = 0u; z = n_wg;            // hi = the first g with end(g) > total - w
    while (a < z) {
        const uint32_t mid = a + (z - a) / 2u;
        sweep_bytes(m, mid, n, dim, b, e);
        if (e > total - w) z = mid; else a = mid + 1u;
    }
    return PlainWindow{lo, a};
}

}  // namespace cqs
