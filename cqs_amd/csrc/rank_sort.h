// rank_sort.h — the select's in-LDS rank sort of <= 1024 distinct packed keys, used by select_finish_kernel
// (scan_kernels.hip) and the select inside the shadow's tail kernel; and its form over all 1024 threads, used by that kernel's
// finishing workgroup (scan_bf16.hip).  Device code only; internal to libcqs_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cqs {

// Rank sort: the keys are distinct, so rank(i) = #{j : key[j] > key[i]} is a permutation.
// One key per thread, count broadcast LDS reads, no barriers inside the loop.
// Round 5: the ranks are taken on the keys' TOP HALVES (the ordered score bits), four per 16-byte LDS read:
// 1 read + 4 compares + 4 adds per four keys instead of 4 reads + 4 64-bit compares + 8 (7 -> ~3 us at 510 keys).
// Two equal scores among the candidates get the same rank and leave a hole in the output - detected below, and
// only then are the ranks retaken on the full keys (exact: scores equal in all 32 bits are duplicates or ties).
// Block of 1024 threads, count <= 1024.  s_sorted: >= count u64, s_ok: >= count + 3 u32, s_flag: one u32 (all LDS,
// none aliasing s_keys).  Leaves s_sorted[0, count) sorted descending; every thread returns after the last barrier.
__device__ __forceinline__ void rank_sort_keys(const uint64_t* s_keys, uint32_t count, uint64_t* s_sorted, uint32_t* s_ok,
                                               uint32_t* s_flag) {
    __syncthreads();
    const uint32_t cpad = (count + 3u) & ~3u;
    if (threadIdx.x < cpad) s_ok[threadIdx.x] = threadIdx.x < count ? (uint32_t)(s_keys[threadIdx.x] >> 32) : 0u;
    if (threadIdx.x < count) s_sorted[threadIdx.x] = 0ull;       // (no valid key is 0)
    if (threadIdx.x == 0) s_flag[0] = 0u;
    __syncthreads();
    if (threadIdx.x < count) {
        const uint64_t mine = s_keys[threadIdx.x];
        const uint32_t mh = (uint32_t)(mine >> 32);
        uint32_t rank = 0;
#pragma unroll 8
        for (uint32_t j = 0; j < cpad; j += 4u) {                 // (unrolled: eight 16-byte reads in flight, not one)
            const uint4 o = *reinterpret_cast<const uint4*>(&s_ok[j]);
            rank += (o.x > mh) ? 1u : 0u;
            rank += (o.y > mh) ? 1u : 0u;
            rank += (o.z > mh) ? 1u : 0u;
            rank += (o.w > mh) ? 1u : 0u;
        }
        s_sorted[rank] = mine;
    }
    __syncthreads();
    if (threadIdx.x < count && s_sorted[threadIdx.x] == 0ull) s_flag[0] = 1u;   // a hole: two candidates share their score bits
    __syncthreads();
    if (s_flag[0] != 0u) {
        if (threadIdx.x < count) {
            const uint64_t mine = s_keys[threadIdx.x];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < count; ++j) rank += (s_keys[j] > mine) ? 1u : 0u;
            s_sorted[rank] = mine;
        }
        __syncthreads();
    }
}

// rank_sort_keys over all 1024 threads: 2^S threads per key (2^S * count <= 1024, S <= 3), each ranking its key
// against one of 2^S segments of the list, the partial ranks added across the 2^S neighbouring lanes.  The finisher sorts
// about 350 keys at k = 20: one thread per key keeps six waves at 2 x 350 compares each while ten idle.  Same contract, same
// result (a rank is a count, however it is split); the rare equal-score case goes to the exact single-thread ranks.
__device__ __forceinline__ void rank_sort_keys_wide(const uint64_t* s_keys, uint32_t count, uint64_t* s_sorted, uint32_t* s_ok,
                                                    uint32_t* s_flag) {
    __syncthreads();
    const uint32_t cpad = (count + 3u) & ~3u;
    if (threadIdx.x < cpad) s_ok[threadIdx.x] = threadIdx.x < count ? (uint32_t)(s_keys[threadIdx.x] >> 32) : 0u;
    if (threadIdx.x < count) s_sorted[threadIdx.x] = 0ull;       // (no valid key is 0)
    if (threadIdx.x == 0) s_flag[0] = 0u;
    __syncthreads();
    const uint32_t S = count <= 128u ? 3u : (count <= 256u ? 2u : (count <= 512u ? 1u : 0u));
    const uint32_t i = threadIdx.x >> S, part = threadIdx.x & ((1u << S) - 1u);
    const uint32_t seg = (((cpad >> 2) + (1u << S) - 1u) >> S) << 2;   // words per segment, a multiple of 4
    const bool mine_ok = i < count;
    const uint64_t mine = mine_ok ? s_keys[i] : 0ull;
    const uint32_t mh = (uint32_t)(mine >> 32);
    uint32_t rank = 0;
    const uint32_t j0 = part * seg, j1 = j0 + seg < cpad ? j0 + seg : cpad;
    if (mine_ok) {
#pragma unroll 4
        for (uint32_t j = j0; j < j1; j += 4u) {
            const uint4 o = *reinterpret_cast<const uint4*>(&s_ok[j]);
            rank += (o.x > mh) ? 1u : 0u;
            rank += (o.y > mh) ? 1u : 0u;
            rank += (o.z > mh) ? 1u : 0u;
            rank += (o.w > mh) ? 1u : 0u;
        }
    }
    for (uint32_t d = 1u; d < (1u << S); d <<= 1) rank += __shfl_xor(rank, d, 64);   // (the 2^S lanes of a key are neighbours in one wave)
    if (mine_ok && part == 0u) s_sorted[rank] = mine;
    __syncthreads();
    if (threadIdx.x < count && s_sorted[threadIdx.x] == 0ull) s_flag[0] = 1u;   // a hole: two candidates share their score bits
    __syncthreads();
    if (s_flag[0] != 0u) {
        if (threadIdx.x < count) {
            const uint64_t own = s_keys[threadIdx.x];
            uint32_t r = 0;
            for (uint32_t j = 0; j < count; ++j) r += (s_keys[j] > own) ? 1u : 0u;
            s_sorted[r] = own;
        }
        __syncthreads();
    }
}

}  // namespace cqs
