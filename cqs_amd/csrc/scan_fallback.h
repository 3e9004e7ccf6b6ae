// scan_fallback.h — the f32 fallback behind a certified shadow search as ONE gated launch (scan_fallback.hip,
// f32_topk_fallback_kernel): an exact brute-force top-k over the f32 rows with no score row, no gmax /
// gaux and no select_body.  The other form of the fallback - the gated scan_gemv_kernel + select_finish_kernel pair -
// stays for every block this one does not take.  Internal to libcqs_hip.so.
#pragma once
#include "scan_kernels.h"

namespace cqs {

constexpr uint32_t kFallbackMaxK = 128;   // bounds the hand-off scratch ([b, grid, k] keys) and the finisher's merge

// Key words of the hand-off scratch for a device of n_cu compute units (the grid never exceeds one workgroup per CU).
inline size_t f32_topk_fallback_words(uint32_t n_cu) { return (size_t)kMaxGemvQ * n_cu * kFallbackMaxK; }

// Blocks the one-launch form takes: one gemv pass' worth of queries, k up to the cap, a shared keep-bitset or none (a
// per-query table keeps the two gated launches), the shadow's dims.
inline bool f32_topk_fallback_takes(const ScanArgs& a) {
    return a.b >= 1u && a.b <= kMaxGemvQ && a.k >= 1u && a.k <= kFallbackMaxK && !a.keep_tab && a.dim >= 8u &&
           a.dim % 4u == 0u && a.dim <= 2048u && a.n >= 1u && a.n <= 0xFFFF0000u;
}

// One launch on st: every workgroup reads gate[0, a.b) at entry (gate_closed) and returns when all are 1.  Otherwise the
// exact top a.k of every query of the block over a.rows (scan_gemv_kernel's score bits and epilogue, a.keep, a.mode /
// a.threshold) into out_keys [b, k] / out_counts [b], as launch_scan + launch_select write them.  lists: device scratch of
// f32_topk_fallback_words(a.n_cu) u64; tickets: device [kMaxGemvQ], zero on entry (once, at allocation) and left zero.
// Never touches a.work, a.scores, a.gmax or a.gaux.  hipErrorInvalidValue for a block f32_topk_fallback_takes refuses.
hipError_t launch_f32_topk_fallback(const ScanArgs& a, uint32_t row_base, const uint32_t* gate, uint64_t* lists,
                                    uint32_t* tickets, uint64_t* out_keys, uint32_t* out_counts, hipStream_t st);

}  // namespace cqs
