// tags_kernel.h — the launcher of tags_keep_kernel (index_tags.hip), shared by the dense and the sparse index: the
// keep-bitset of a tag filter, written on the device where the scans read it.
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

}  // namespace cqs
