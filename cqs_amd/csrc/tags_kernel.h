// tags_kernel.h — the launchers of tags_keep_kernel and tags_keep_multi_kernel (index_tags.hip), which know no index (the
// dense and the sparse one share the former): the keep-bitset of a tag filter, or of up to 32 at once, written on the
// device where the scans read it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cqs {

constexpr uint32_t kTagThreads = 256;        // one row per lane and step
constexpr uint32_t kTagMaxBlocks = 2048;     // grid cap; the tiles of 256 rows beyond it are taken grid-stride

// The workgroups a launch over n >= 1 rows has (= the partial counts it writes).
inline uint32_t tags_keep_blocks(uint32_t n) {
    const uint32_t tiles = n / kTagThreads + (n % kTagThreads ? 1u : 0u);
    return tiles < kTagMaxBlocks ? tiles : kTagMaxBlocks;
}

// Enqueue on `st`: d_keep[0, ceil(n / 32)) = the bitset of tags_host.h's tag_kept over d_tags[0, n) under the filter
// `allow` (host, 32 words; read before the call returns), bits past n zero; d_partials (nullable: nobody counts)
// [tags_keep_blocks(n)] = the rows each workgroup kept - every entry written, their sum is the exact count.  n >= 1.
hipError_t launch_tags_keep(const uint32_t* d_tags, uint32_t n, const uint32_t* allow, uint32_t* d_keep, uint32_t* d_partials,
                            hipStream_t st);

// ---- up to 32 filters in one pass over the tags (tags_keep_multi_kernel) ------------------------------
constexpr uint32_t kTagMultiGroups = 4;                                     // 64-row groups a wave takes per step
constexpr uint32_t kTagMultiRows = kTagThreads * kTagMultiGroups;           // rows per workgroup and step: 1024
// Grid cap.  One workgroup per compute unit of an MI355X: the partial counts are [blocks][f] words, so the one copy the
// host waits for is at most 256 x 32 x 4 B = 32 KB (8 KB at f = 8); 1M rows are four steps per workgroup.
constexpr uint32_t kTagMultiMaxBlocks = 256;

// The workgroups a multi-filter launch over n >= 1 rows has (max_blocks: a smaller grid cap, 0 = kTagMultiMaxBlocks).
inline uint32_t tags_keep_multi_blocks(uint32_t n, uint32_t max_blocks) {
    const uint32_t tiles = n / kTagMultiRows + (n % kTagMultiRows ? 1u : 0u);
    const uint32_t cap = max_blocks && max_blocks < kTagMultiMaxBlocks ? max_blocks : kTagMultiMaxBlocks;
    return tiles < cap ? tiles : cap;
}

// Enqueue on `st`: for every filter j < f (1 <= f <= 32) of the transposed table d_tbl (device, tags_host.h's
// transpose_filters: 1024 words), d_tab[j * stride_words + [0, ceil(n / 32))) = the bitset launch_tags_keep writes for
// filter j - bits past n zero, no word past ceil(n / 32) written, rows >= f of the table not touched.  Each tag is read
// once.  d_partials [tags_keep_multi_blocks(n, max_blocks)][f] = the rows each workgroup kept under each filter, every
// entry written.  n >= 1, stride_words >= ceil(n / 32).
hipError_t launch_tags_keep_multi(const uint32_t* d_tags, uint32_t n, const uint32_t* d_tbl, uint32_t f, uint32_t* d_tab,
                                  uint32_t stride_words, uint32_t* d_partials, uint32_t max_blocks, hipStream_t st);

}  // namespace cqs
