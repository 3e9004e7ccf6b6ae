// scan_fallback.hip — the f32 fallback of a device-API shadow search as one gated launch (scan_fallback.h).
//
//  f32_topk_fallback_kernel  gate closed (every query of the block certified - almost every search): every workgroup reads
//                            the gate words and returns.  Gate open: an exact brute-force top-k of the whole block.  The
//                            workgroups stride over 256-row tiles; one wave scores 16 rows of a tile against every query
//                            with the tail kernel's exact chain (f32_score.h); each workgroup keeps its own top k of packed
//                            keys per query in LDS; the last workgroup of a query to arrive merges the lists.
//
// Wave = 64 lanes.  gfx950 only.
#include "scan_fallback.h"
#include "f32_score.h"
#include "launch_util.h"
#include "rank_sort.h"

namespace cqs {

constexpr uint32_t kFbThreads = 1024;   // the block shape rank_sort_keys is written for
constexpr uint32_t kFbWaveRows = 16;    // rows of a tile one wave scores
constexpr uint32_t kFbTileRows = (kFbThreads / 64u) * kFbWaveRows;   // 256
// Keys one query's LDS list holds: at most kFbBuf - kFbTileRows on entry to a tile (or to a 256-key step of the finisher),
// which appends at most kFbTileRows; a longer list is cut back to its top k before the next tile.
constexpr uint32_t kFbBuf = 768;
static_assert(kFallbackMaxK + kFbTileRows <= kFbBuf && kFbBuf <= kFbThreads, "a cut list plus one tile fits the buffer and the sort");

struct FallbackParams {
    const float* rows;       // [n, dim] f32
    const float* q;          // [b, dim]
    uint32_t n, dim, b, k, mode, row_base;
    float thr;
    const uint32_t* keep;    // nullable shared bitset, ceil(n / 32) words
    const uint32_t* gate;    // [b]
    uint64_t* lists;         // [b, gridDim.x, k]: each workgroup's top k of each query, descending, 0 = none.  Handed to the
                             // finishing workgroup inside the launch (agent-scope accesses only)
    uint32_t* tickets;       // [b] arrivals of each query's workgroups: 0 on entry, 0 again on exit
    uint64_t* out_keys;      // [b, k]
    uint32_t* out_counts;    // [b]
};

// The LDS of a workgroup, all of it dynamic (16-byte aligned carve): the sort's scratch, then per query its state, its
// zero-padded fragments [NCH * 256] and its key list [kFbBuf].
struct FallbackLds {
    uint64_t* sorted;   // [kFbBuf]
    uint32_t* ok;       // [kFbBuf + 4]
    uint64_t* thr;      // [kMaxGemvQ] the k-th key of the list when it was last cut (0: fewer than k yet): keys below it are out
    uint32_t* cnt;      // [kMaxGemvQ] keys in the list
    uint32_t* last;     // [kMaxGemvQ] this workgroup finishes the query
    uint32_t* flag;     // rank_sort_keys'
    float* q;           // [b][NCH * 256]
    uint64_t* keys;     // [b][kFbBuf]
};
constexpr size_t kFbLdsFixed = kFbBuf * 8u + (kFbBuf + 4u) * 4u + kMaxGemvQ * 8u + kMaxGemvQ * 4u + kMaxGemvQ * 4u + 16u;
static_assert(kFbLdsFixed % 16u == 0u, "the per-query arrays start 16-byte aligned");
inline size_t fallback_lds_bytes(uint32_t b, uint32_t nch) { return kFbLdsFixed + (size_t)b * (nch * 1024u + kFbBuf * 8u); }

__device__ __forceinline__ FallbackLds carve_lds(unsigned char* base, uint32_t b, uint32_t qwords) {
    FallbackLds l;
    l.sorted = (uint64_t*)base;                  base += kFbBuf * 8u;
    l.ok = (uint32_t*)base;                      base += (kFbBuf + 4u) * 4u;
    l.thr = (uint64_t*)base;                     base += kMaxGemvQ * 8u;
    l.cnt = (uint32_t*)base;                     base += kMaxGemvQ * 4u;
    l.last = (uint32_t*)base;                    base += kMaxGemvQ * 4u;
    l.flag = (uint32_t*)base;                    base += 16u;
    l.q = (float*)base;                          base += (size_t)b * qwords * 4u;
    l.keys = (uint64_t*)base;
    return l;
}

// Cut query qi's list back to its top min(count, k) keys, sorted descending, and note the k-th as the list's threshold.  Every
// thread of the workgroup calls it, behind a barrier that follows the last append; ends on a barrier.
__device__ __forceinline__ void cut_list(const FallbackLds& l, uint32_t qi, uint32_t k) {
    uint64_t* keys = l.keys + (size_t)qi * kFbBuf;
    const uint32_t m = l.cnt[qi];
    rank_sort_keys(keys, m, l.sorted, l.ok, l.flag);
    const uint32_t kept = m < k ? m : k;
    if (threadIdx.x < kept) keys[threadIdx.x] = l.sorted[threadIdx.x];
    if (threadIdx.x == 0) {
        l.cnt[qi] = kept;
        l.thr[qi] = kept == k ? l.sorted[k - 1u] : 0ull;
    }
    __syncthreads();
}

// The lists that may overflow on the next 256 appends, as a bit per query.  Between two barriers, so that every thread reads
// the same counts and the workgroup takes the cuts together.
__device__ __forceinline__ uint32_t lists_to_cut(const FallbackLds& l, uint32_t b) {
    __syncthreads();
    uint32_t need = 0u;
    for (uint32_t qi = 0; qi < b; ++qi) need |= (l.cnt[qi] > kFbBuf - kFbTileRows ? 1u : 0u) << qi;
    __syncthreads();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)need);
}

// Gate open: nobody waits for anybody.  A workgroup stores its b lists, adds one to each query's ticket, and the one whose
// add returns gridDim.x - 1 knows that every other has stored: it merges that query's lists, writes the answer and puts the
// ticket back to 0 for the next search.  The keys are totally ordered (score bits, then row), so the top k of the union of
// the workgroups' top-k lists is the top k of the corpus, ties by row included.
// Visibility (per-XCD L2s are not coherent, a CU's L1 is never refreshed): the tail kernel's protocol.  Every list word is
// stored write-through by an agent-scope atomic store, each wave drains its stores before the workgroup's barrier, one lane
// per query then adds to the ticket, and the finisher reads the lists by agent-scope atomic loads only, after the add has
// returned and a barrier that the adding wave joins.  Rows, queries, the bitset and the gate come from earlier launches and
// are read plainly.
template <int NCH, bool NT>
__global__ __launch_bounds__(1024) void f32_topk_fallback_kernel(const FallbackParams p) {
    if (gate_closed(p.gate, p.b)) return;   // (same words, same decision as the gated scan + select; before any load or barrier)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_fb[];
    constexpr uint32_t QW = (uint32_t)NCH * 256u;
    constexpr int RI = NCH <= 4 ? 4 : (NCH <= 6 ? 2 : 1);   // rows in flight per wave: RI * NCH 16-byte loads per lane, and the
                                                            // 128 VGPRs of a 1024-thread block hold them beside a query's fragments
    const uint32_t b = p.b, k = p.k, n = p.n, dim = p.dim;
    const FallbackLds l = carve_lds(s_fb, b, QW);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

    for (uint32_t i = threadIdx.x; i < b * QW; i += kFbThreads) {
        const uint32_t qi = i / QW, d = i % QW;
        l.q[i] = d < dim ? p.q[(size_t)qi * dim + d] : 0.f;
    }
    if (threadIdx.x < kMaxGemvQ) { l.cnt[threadIdx.x] = 0u; l.thr[threadIdx.x] = 0ull; l.last[threadIdx.x] = 0u; }
    __syncthreads();

    // ---- score: tiles blockIdx.x, + gridDim.x, ... -----------------------------------------------------------------------
    const uint32_t last_row = n - 1u;
    const uint32_t n_tiles = (n + kFbTileRows - 1u) / kFbTileRows;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t row0 = tile * kFbTileRows + wave * kFbWaveRows;
        uint32_t mask = 0u;   // the wave's rows inside the corpus that the filter keeps
        if (row0 < n) {
            const uint32_t left = n - row0;
            mask = left >= kFbWaveRows ? 0xFFFFu : (1u << left) - 1u;
            if (p.keep) mask &= p.keep[row0 >> 5] >> (row0 & 31u);   // (row0 % 16 == 0: the 16 bits lie in one word)
        }
        mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)mask);
        for (uint32_t j = 0; j < kFbWaveRows / (uint32_t)RI; ++j) {
            const uint32_t m = (mask >> ((uint32_t)RI * j)) & ((1u << RI) - 1u);
            if (m == 0u) continue;   // all RI rows filtered out / past the end: skip their reads
            const uint32_t r0 = row0 + (uint32_t)RI * j;
            f4 x[RI][NCH];
#pragma unroll
            for (int r = 0; r < RI; ++r) {
                const uint32_t row = r0 + (uint32_t)r > last_row ? last_row : r0 + (uint32_t)r;
                f32_row_fragments<NCH, NT>(p.rows + (size_t)row * dim, dim, lane, x[r]);
            }
            for (uint32_t qi = 0; qi < b; ++qi) {
                f4 qv[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) qv[c] = *(const f4*)(l.q + qi * QW + (uint32_t)c * 256u + lane * 4u);
#pragma unroll
                for (int r = 0; r < RI; ++r) {
                    float s = f32_dot_chain<NCH>(x[r], qv);
                    const bool emit = f32_emit(s, p.mode, p.thr);
                    if (lane == 0u && ((m >> r) & 1u) && emit) {
                        const uint64_t key = pack_key(okey(s), p.row_base + r0 + (uint32_t)r);
                        if (key > l.thr[qi]) l.keys[(size_t)qi * kFbBuf + atomicAdd(&l.cnt[qi], 1u)] = key;
                    }
                }
            }
        }
        const uint32_t need = lists_to_cut(l, b);
        for (uint32_t qi = 0; qi < b; ++qi)
            if ((need >> qi) & 1u) cut_list(l, qi, k);
    }

    // ---- hand-off: the workgroup's top k of every query, then one ticket per query ------------------------------------------
    __syncthreads();
    for (uint32_t qi = 0; qi < b; ++qi) {
        cut_list(l, qi, k);
        if (threadIdx.x < k)
            __hip_atomic_store(p.lists + ((size_t)qi * gridDim.x + blockIdx.x) * k + threadIdx.x,
                               threadIdx.x < l.cnt[qi] ? l.keys[(size_t)qi * kFbBuf + threadIdx.x] : 0ull, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x < b) {
        const uint32_t t = __hip_atomic_fetch_add(p.tickets + threadIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        l.last[threadIdx.x] = t == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();

    // ---- finish: the queries whose last list was this workgroup's ----------------------------------------------------------
    for (uint32_t qi = 0; qi < b; ++qi) {
        if (l.last[qi] == 0u) continue;   // (workgroup-uniform: written before the barrier above, never again)
        if (threadIdx.x == 0) { l.cnt[qi] = 0u; l.thr[qi] = 0ull; }
        __syncthreads();
        const uint64_t* lists = p.lists + (size_t)qi * gridDim.x * k;
        const uint32_t total = gridDim.x * k;
        for (uint32_t c0 = 0; c0 < total; c0 += kFbThreads) {
            const uint32_t idx = c0 + threadIdx.x;
            const uint64_t key = idx < total ? __hip_atomic_load(lists + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            for (uint32_t step = 0; step < kFbThreads / kFbTileRows; ++step) {   // 256 keys at a time: what the list has room for
                if (threadIdx.x / kFbTileRows == step && key > l.thr[qi])       // (0 = no key: never above a threshold)
                    l.keys[(size_t)qi * kFbBuf + atomicAdd(&l.cnt[qi], 1u)] = key;
                if ((lists_to_cut(l, b) >> qi) & 1u) cut_list(l, qi, k);
            }
        }
        cut_list(l, qi, k);   // (behind lists_to_cut's barriers)
        const uint32_t outc = l.cnt[qi];
        for (uint32_t i = threadIdx.x; i < k; i += kFbThreads)
            p.out_keys[(size_t)qi * k + i] = i < outc ? l.keys[(size_t)qi * kFbBuf + i] : 0ull;
        if (threadIdx.x == 0) {
            p.out_counts[qi] = outc;
            __hip_atomic_store(p.tickets + qi, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // armed for the next search
        }
    }
}

hipError_t launch_f32_topk_fallback(const ScanArgs& a, uint32_t row_base, const uint32_t* gate, uint64_t* lists,
                                    uint32_t* tickets, uint64_t* out_keys, uint32_t* out_counts, hipStream_t st) {
    if (!f32_topk_fallback_takes(a) || !gate || !lists || !tickets || a.n_cu == 0u) return hipErrorInvalidValue;
    const FallbackParams p{a.rows, a.q, a.n, a.dim, a.b, a.k, a.mode, row_base, a.threshold, a.keep, gate, lists, tickets,
                           out_keys, out_counts};
    const uint32_t nch = (a.dim + 255u) / 256u;
    const uint32_t n_tiles = (a.n + kFbTileRows - 1u) / kFbTileRows;
    const dim3 grid(n_tiles < a.n_cu ? n_tiles : a.n_cu), block(kFbThreads);   // (<= n_cu: what `lists` is sized for)
    const size_t lds = fallback_lds_bytes(a.b, nch);
    auto launch = [&](auto nch_c, auto nt_c) -> hipError_t {
        auto kern = f32_topk_fallback_kernel<decltype(nch_c)::value, decltype(nt_c)::value>;
        if (lds > 48u * 1024u) {
            static DynLdsOnce once;   // per instantiation
            const hipError_t e = once.ensure((const void*)kern, lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, block, lds, st, p);
        return hipGetLastError();
    };
    auto by_nt = [&](auto nch_c) -> hipError_t {
        return a.nontemporal ? launch(nch_c, std::true_type{}) : launch(nch_c, std::false_type{});
    };
    switch (nch) {
        case 1: return by_nt(std::integral_constant<int, 1>{});
        case 2: return by_nt(std::integral_constant<int, 2>{});
        case 3: return by_nt(std::integral_constant<int, 3>{});
        case 4: return by_nt(std::integral_constant<int, 4>{});
        case 5: return by_nt(std::integral_constant<int, 5>{});
        case 6: return by_nt(std::integral_constant<int, 6>{});
        case 7: return by_nt(std::integral_constant<int, 7>{});
        case 8: return by_nt(std::integral_constant<int, 8>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace cqs
