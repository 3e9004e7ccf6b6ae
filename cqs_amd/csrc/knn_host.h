// knn_host.h — the device-free part of cqs_hip_index_knn_graph: the argument plan (the refusals in their order, the clamp
// of `limit`, the k the scan asks for), the cut of the asked range into the corpus's fixed tiles, and the finish rule that
// turns a tile's packed keys into a target's answer.  Plain C++ over the caller's arrays, no HIP, no
// handle: index_knn.hip calls it under the handle's mutex and its finish kernel runs the same slot rule, one slot per
// lane; tests/knn_host_driver.cpp runs it under ASAN + UBSan on the CPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "search_host.h"

#if defined(__HIPCC__)
#define CQS_KNN_HD __host__ __device__
#else
#define CQS_KNN_HD
#endif

namespace cqs_knn {

constexpr uint32_t kTileMax = 256;   // rows of a tile = queries of its block: one sweep of the matrix-core scan

enum class Plan : int32_t {
    Invalid = -1,   // CQS_HIP_ERR_INVALID; *why says which refusal; outputs untouched
    Nothing = 0,    // m == 0: CQS_HIP_OK, nothing touched
    Run = 1,        // the range is in order: Planned says what to run (k1 == 0: no device work, every count 0)
};

// What the call sees of its handle (all zero beside a null one).
struct Handle {
    bool present;         // a non-null handle
    bool sharded;         // made by cqs_hip_index_create_sharded / _load_sharded
    uint64_t row_base;
    uint64_t len;         // rows stored
    uint32_t max_block;   // max_query_block of the handle (a function of len alone)
};

struct Planned {
    uint32_t limit;       // L = clamp(limit, 1, CQS_HIP_NEIGHBORS_MAX): the output stride
    uint32_t k1;          // neighbors_k(L, len): what each tile's search asks for; 0 = the index holds one row
    uint32_t tile;        // T = min(kTileMax, max_block)
    uint64_t local_first; // first_row - row_base
};

// cqs_hip_index_knn_graph's arguments, refused in the documented order: a null handle, a null output with m > 0,
// m > CQS_HIP_KNN_MAX_TARGETS, any part of the range outside the index, a row-sharded handle.  m == 0 asks for nothing
// and is answered before any of the checks that read the range.
inline Plan plan_knn(const Handle& h, uint64_t first_row, uint64_t m, uint32_t limit, bool outputs, Planned* out,
                     const char** why) {
    *why = "";
    *out = Planned{0, 0, 0, 0};
    if (!h.present) { *why = "null handle"; return Plan::Invalid; }
    if (m == 0) return Plan::Nothing;
    if (!outputs) { *why = "null output buffer"; return Plan::Invalid; }
    if (m > CQS_HIP_KNN_MAX_TARGETS) { *why = "more than CQS_HIP_KNN_MAX_TARGETS targets in one call"; return Plan::Invalid; }
    if (first_row < h.row_base || first_row - h.row_base >= h.len || m > h.len - (first_row - h.row_base)) {
        *why = "range not in this index";
        return Plan::Invalid;
    }
    if (h.sharded) { *why = "not built for a row-sharded handle"; return Plan::Invalid; }
    out->limit = limit;
    out->k1 = cqs_search::neighbors_k(&out->limit, h.len);
    out->tile = h.max_block < kTileMax ? (h.max_block ? h.max_block : 1u) : kTileMax;
    out->local_first = first_row - h.row_base;
    return Plan::Run;
}

// One block of a call: the queries are the local rows [tile_first, tile_first + tile_rows) - a whole tile of the corpus,
// whatever part of it was asked for - of which the targets tile_first + emit_first + [0, emit_count) are emitted, to the
// call's output rows out_offset + [0, emit_count).
struct Tile { uint64_t tile_first; uint32_t tile_rows, emit_first, emit_count; uint64_t out_offset; };

// The tiles that local rows [local_first, local_first + m) touch, in row order.  Tiles are fixed by (len, tile) alone:
// [tile * t, min(tile * t + tile, len)).  The caller has checked the range against len; tile >= 1.
inline std::vector<Tile> cut_tiles(uint64_t local_first, uint64_t m, uint64_t len, uint32_t tile) {
    std::vector<Tile> tiles;
    if (tile == 0) tile = 1;
    const uint64_t end = local_first + m;
    for (uint64_t row = local_first; row < end;) {
        const uint64_t t0 = row / tile * tile;
        const uint64_t t1 = t0 + tile < len ? t0 + tile : len;
        const uint64_t stop = end < t1 ? end : t1;
        tiles.push_back(Tile{t0, (uint32_t)(t1 - t0), (uint32_t)(row - t0), (uint32_t)(stop - row), row - local_first});
        row = stop;
    }
    return tiles;
}

// ---- the finish rule, slot by slot (what one lane of knn_finish_kernel does with each of its slots) --------------------
// A key is (order-preserving score bits << 32) | (0xFFFFFFFF - global row), as every select of this library packs it.
CQS_KNN_HD inline uint32_t key_mark(uint32_t global_row) { return 0xFFFFFFFFu - global_row; }
CQS_KNN_HD inline uint64_t key_row(uint64_t key) { return (uint64_t)(0xFFFFFFFFu - (uint32_t)key); }
CQS_KNN_HD inline uint32_t key_score_bits(uint64_t key) {   // the f32 bits of the score (cqs_search::unpack_keys)
    const uint32_t ok = (uint32_t)(key >> 32);
    return (ok & 0x80000000u) ? (ok ^ 0x80000000u) : ~ok;
}
// Where the key in slot s goes once the target's own key, in slot self (self >= cnt: it is not among them), is dropped:
// slots before it stay, slots after it move up one place (cqs_search::drop_self).  s != self.
CQS_KNN_HD inline uint32_t dest_slot(uint32_t s, uint32_t self) { return s > self ? s - 1u : s; }
// How many of the cnt keys are emitted: all but the target's, at most `limit` - where the target is absent (it lies in a
// run of equal rows longer than k1) the last key falls off instead.
CQS_KNN_HD inline uint32_t emitted(uint32_t cnt, bool self_found, uint32_t limit) {
    const uint32_t left = cnt - (self_found ? 1u : 0u);
    return left < limit ? left : limit;
}

// The kernel's work for one target on host arrays: keys[0, cnt) of its query, cnt <= k1, into out_rows / out_scores
// [0, limit), zeros past the count.  Returns the count.
inline uint32_t finish_target(const uint64_t* keys, uint32_t cnt, uint32_t global_row, uint32_t limit, uint64_t* out_rows,
                              float* out_scores) {
    uint32_t self = cnt;
    for (uint32_t s = 0; s < cnt; ++s)
        if ((uint32_t)keys[s] == key_mark(global_row)) { self = s; break; }
    const uint32_t count = emitted(cnt, self < cnt, limit);
    for (uint32_t s = 0; s < cnt; ++s) {
        if (s == self) continue;
        const uint32_t d = dest_slot(s, self);
        if (d >= limit) continue;
        const uint32_t bits = key_score_bits(keys[s]);
        out_rows[d] = key_row(keys[s]);
        memcpy(&out_scores[d], &bits, 4);
    }
    for (uint32_t d = count; d < limit; ++d) { out_rows[d] = 0; out_scores[d] = 0.f; }
    return count;
}

}  // namespace cqs_knn
