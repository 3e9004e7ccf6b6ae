// scan_kernels.h — launch interface of the gfx950 scan + top-k kernels.
// Internal to libcqs_hip.so (the public boundary is include/cqs_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "group_map.h"
#include "wave_ops.h"   // wave_dpp, wave_max16, wave_max64: the scans' maxima

namespace cqs {

// Geometry shared by host and device code.
constexpr uint32_t kTaskRows = 64;        // rows of the largest work-queue task (= maxima group of the MFMA path)
constexpr uint32_t kTaskRowsSmall = 16;   // rows of the smallest task (bounds the number of maxima groups)
constexpr uint32_t kRowsPerBlock = 256;   // n_pad granule (score row stride)
constexpr uint32_t kHistBins = 4096;      // threshold-search histogram bins
constexpr uint32_t kCandCap = 8192;       // candidates one sort block holds in LDS
constexpr uint32_t kMaxK = 1024;
constexpr uint32_t kMaxGemvQ = 8;         // queries per HBM-streaming scan pass
constexpr uint32_t kDbgWaves = 4096;      // per-wave start/end stamps kept by the scan when ScanArgs.dbg is set
constexpr uint32_t kWorkWords = 64;       // work-queue heads (one per scan launch of a search); zero on entry,
                                          // re-zeroed by select_finish (a shadow search: by its tail kernel)

// TaskTiers (tasks in row order), plan_tiers and the GroupMap of the select's maxima index: group_map.h.

struct ScanArgs {
    const float* rows;      // [n, dim] f32, row-major, HBM
    uint32_t n;             // rows in this index/shard
    uint32_t n_pad;         // n rounded up to kRowsPerBlock (score row stride)
    uint32_t dim;
    const float* q;         // [b, dim] f32, device
    uint32_t b;             // queries
    float* scores;          // [b, n_pad] f32, device
    const uint32_t* keep;   // nullable device bitset, ceil(n/32) words
    const uint32_t* keep_tab = nullptr;   // nullable device table [rows][keep_stride] of bitsets, one row per query (gemv
                            // passes only; `keep` must be null): query i of the block is filtered by row keep_slot[i]
    uint32_t keep_stride = 0;             // words per table row (>= ceil(n/32)); 0 = the shared bitset `keep`
    const uint8_t* keep_slot = nullptr;   // host [b]: table row of each query (passed to the kernels by value, pass by pass)
    uint32_t mode;          // CQS_HIP_MODE_*
    float threshold;
    bool nontemporal;       // stream the corpus past L2 (corpus >> Infinity Cache)
    bool linear_bins;       // scores bounded in [-1,1] (cosine / pipeline mode): linear histogram bins
    bool range_bins = false;// select only: linear bins over the range of the row's own group maxima (the sparse index)
    uint32_t k;
    float* gmax;            // [b, tiers.total()] per-task maxima (written by the scan)
    uint64_t* gaux = nullptr;// nullable, [b, tiers.total()]: (lane of the task's maximum << 32) | f32 bits of its runner-up
                            // (written by the gemv scan and the sparse index; the matrix-core scan does not: its select
                            // launch ignores the field)
    TaskTiers tiers;        // plan_tiers(n_pad, n_cu, uniform_groups(b, dim))
    uint32_t group_tasks = 1;   // tasks per entry of gmax / gaux (GroupMap::G): 1, or 4 for the int8 scan, whose workgroup
                            // publishes one triple for its four tasks; gmax / gaux are then [b, ceil(tiers.total() / 4)]
    uint32_t sweep_rev = 0; // int8 scan only: 1 = its workgroups take the tasks in reverse order (i8_sweep.h; same outputs)
    uint64_t plain_bytes = 0;   // int8 scan only, nontemporal: bytes at each end of the copy that are loaded plainly
    uint32_t* work;         // [kWorkWords] work-queue heads (zero on entry)
    uint32_t n_cu;          // compute units of the device
    bool gemv_only = false; // never the matrix-core kernel, whatever b: blocks of > 8 queries run as passes of <= 8
                            // (the scores of a gemv pass do not depend on how many queries share it)
    void* dbg;              // nullable: (16 + 2 * kDbgWaves) x u64: select_finish phase stamps, then the scan's
                            // per-wave start/end stamps (CQS_HIP_DEBUG_STAMPS=1)
    const uint32_t* gate = nullptr;  // nullable device [b] (gemv passes, b <= 64): every workgroup of the gemv scan and of
                            // the select reads gate[0, b) at entry and returns at once when all are 1 (the bf16 shadow has
                            // certified every query of the block; see gate_closed).  A gated scan is launched on the
                            // persistent grid where that has fewer workgroups than one per task (launch_gemv)
};

// scores[q][row] = dot(rows[row], q) (+ mode / bitset / non-finite handling; dropped
// entries = -inf), gmax[q][t] = max over the rows of task t (a.tiers).
hipError_t launch_scan(const ScanArgs& a, hipStream_t stream);

// Exact top-k of each query's score row (one workgroup per query; see select_finish_kernel).
// Output: out_keys[b*k] packed (ordered(score)<<32 | ~global_row) sorted descending,
// out_counts[b].  Leaves the work-queue heads zeroed for the next search.
hipError_t launch_select(const ScanArgs& a, uint32_t row_base, uint64_t* out_keys, uint32_t* out_counts,
                         hipStream_t stream);

// Batched path (scan_mfma.hip): query block [q0, q0+nq), nq <= 256, on the f32 matrix cores.
// a.q must be readable and zero-padded up to mfma_query_tile(nq) rows past q0.
hipError_t launch_scan_mfma(const ScanArgs& a, uint32_t q0, uint32_t nq, uint32_t work_slot, hipStream_t stream);
uint32_t mfma_query_tile(uint32_t nq);
constexpr uint32_t kMfmaMinQueries = 9;   // below this the HBM-streaming gemv passes win
inline bool use_mfma(uint32_t b, uint32_t dim) { return b >= kMfmaMinQueries && dim % 32u == 0; }
inline bool uniform_groups(uint32_t b, uint32_t dim) { return use_mfma(b, dim); }  // kernels that need 64-row groups only

bool scan_dim_supported(uint32_t dim);

// ScanArgs::keep_tab is usable by a gemv launch: no shared bitset beside it, a slot per query, rows that cover the corpus.
inline bool keep_tab_ok(const ScanArgs& a) {
    return !a.keep && a.keep_slot && a.keep_stride >= (a.n + 31u) / 32u;
}

#if defined(__HIPCC__)
// The f32 fallback gate of the device-API shadow search (index.hip, cqs_hip_index_search_device): true when gate[0, b)
// are all 1.  Invariants, kept by every kernel that takes a gate:
//  - the gemv scan and the select decide the same way from the same words (this function, at entry, in every wave;
//    the words were written by an earlier kernel of the stream - the last workgroup of the shadow's tail kernel, before
//    that kernel ended - and do not change during the launch);
//  - a skipped scan never touches the work-queue heads, and the skipped select has nothing to re-zero: the shadow's tail
//    kernel (rescore_certify_kernel, which contains the shadow pass's select) has zeroed them already - exactly one of its
//    workgroups, (0, 0), after the shadow scan that advanced them has ended and before the gated scan can start (kernel
//    boundaries on one stream either side).  A gated scan runs on the persistent grid (launch_gemv) and does dequeue from
//    them when its gate is open; the gated select that follows then re-zeroes them;
//  - the launches between the shadow's tail kernel and the gated select include no memset (gemv blocks of <= 32 queries
//    stay under kWorkWords launches); a memset added there must be gated too;
//  - the one-launch form of the fallback (scan_fallback.hip, f32_topk_fallback_kernel: the blocks scan_fallback.h takes)
//    stands in the pair's place: the same words, the same decision, at entry in every wave before any other load or barrier;
//    nothing is launched between the tail kernel and it; gate open or closed it never touches the work-queue heads, the
//    score rows, gmax or gaux (it has no work queue and no score row), so the heads stay as the tail kernel zeroed them; its
//    own tickets are zero between launches (the finisher of each query puts its ticket back).
__device__ __forceinline__ bool gate_closed(const uint32_t* gate, uint32_t b) {
    uint32_t all = 1u;
    for (uint32_t i = 0; i < b; ++i) all &= gate[i];   // (uniform: scalar loads, no vector registers at entry)
    return all != 0u;
}
#endif

}  // namespace cqs
