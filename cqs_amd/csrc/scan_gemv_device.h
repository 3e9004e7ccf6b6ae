// scan_gemv_device.h — what the three HBM-streaming ("gemv") scans share: scan_gemv_kernel (f32, scan_kernels.hip),
// scan_bf16_kernel (scan_bf16.hip) and scan_i8_kernel (scan_i8.hip).  Device side: the persistent grid's dequeue (f32
// and bf16).  Host side: the pass parameters every launcher fills the same way and the NT x FULL launch switch, as
// templates over each kernel's own params struct (ScanParams / Bf16ScanParams / I8ScanParams keep their fields and their
// kernarg layout).  The kernels' task mask, batch loop and emission are still written out in each kernel: moved into
// function templates here, hipcc orders the instructions of most instantiations differently.
// Internal to libcqs_hip.so.
#pragma once
#include <type_traits>
#include "scan_kernels.h"
#include "scan_device.h"

namespace cqs {

// ---- device ------------------------------------------------------------------------------------------------------------
// The persistent grid's dequeue (f32 and bf16 scans): lane 0 draws a ticket with atomicAdd(p.work + opaque_zero(), 1u).
// A zero the compiler cannot see through.  With a provably uniform address hipcc rewrites the
// dequeue into a wave-aggregated atomic followed at once by s_waitcnt vmcnt(0) + readfirstlane,
// draining every row load in flight.  A "divergent" address keeps the plain returning atomic,
// whose ticket is only waited for where it is used.
__device__ __forceinline__ uint32_t opaque_zero() {
    uint32_t z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}

// ---- host --------------------------------------------------------------------------------------------------------------
// The fields every gemv pass sets the same way, for queries [q0, q0 + nq) of the block.  pq: the per-query table form.
template <class Params>
inline void fill_gemv_pass(Params& p, const ScanArgs& a, uint32_t q0, uint32_t nq, bool pq) {
    p.n = a.n; p.n_pad = a.n_pad; p.dim = a.dim;
    p.q = a.q + (size_t)q0 * a.dim;
    p.scores = a.scores + (size_t)q0 * a.n_pad;
    p.keep = pq ? a.keep_tab : a.keep; p.mode = a.mode; p.thr = a.threshold;
    p.keep_stride = pq ? a.keep_stride : 0u;
    for (uint32_t i = 0; i < kMaxGemvQ; ++i) p.slot[i] = (pq && i < nq) ? a.keep_slot[q0 + i] : (uint8_t)0;
    p.nq = nq;
    p.tiers = a.tiers;
    p.n_tasks = a.tiers.total();
    p.gmax = a.gmax + (size_t)q0 * p.n_tasks;
    p.gaux = a.gaux ? a.gaux + (size_t)q0 * p.n_tasks : nullptr;
}

// The NT x FULL launch switch: launch(std::bool_constant<NT>, std::bool_constant<FULL>) for the two runtime flags.
template <class Launch>
inline auto for_nt_full(bool nt, bool full, Launch launch) {
    if (nt) return full ? launch(std::true_type{}, std::true_type{}) : launch(std::true_type{}, std::false_type{});
    return full ? launch(std::false_type{}, std::true_type{}) : launch(std::false_type{}, std::false_type{});
}

}  // namespace cqs
