// f32_score.h — the exact f32 score of one (row, query) as ONE wave computes it, bit for bit what scan_gemv_kernel
// (scan_kernels.hip) stores for that pair: the single definition of those bits outside that kernel.  Called by the shadow's
// tail kernel for its candidates (scan_bf16.hip, rescore_certify_kernel) and by the one-launch f32 fallback for every row
// (scan_fallback.hip, f32_topk_fallback_kernel).  Device code only; internal to libcqs_hip.so.
//
// NCH = ceil(dim / 256) 1-KiB chunks per row; lane owns floats [c*256 + lane*4, +4) of chunk c.  Past a partial last chunk
// the row fragment comes from a clamped in-row address and the query fragment is zero, so the loads stay unconditional.
#pragma once
#include "scan_device.h"

namespace cqs {

// The lane's fragments of the row at rp.  NT: stream past the caches (corpora far larger than them).
template <int NCH, bool NT = false>
__device__ __forceinline__ void f32_row_fragments(const float* rp, uint32_t dim, uint32_t lane, f4 (&x)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t idx = (uint32_t)c * 256u + lane * 4u;
        const uint32_t off = idx < dim ? idx : dim - 4u;
        if (NT) x[c] = __builtin_nontemporal_load((const f4*)(rp + off));
        else x[c] = *(const f4*)(rp + off);
    }
}

// The lane's fragments of the query at qp: zero past the row's end.  (A kernel that scores many rows against one query
// keeps them, in this layout with these zeros, where it likes.)
template <int NCH>
__device__ __forceinline__ void f32_query_fragments(const float* qp, uint32_t dim, uint32_t lane, f4 (&qv)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t idx = (uint32_t)c * 256u + lane * 4u;
        const f4 v = *(const f4*)(qp + (idx < dim ? idx : dim - 4u));
        qv[c] = idx < dim ? v : (f4)(0.f);
    }
}

// The lane's fragments of the row at rp and of the query at qp (zero past the row's end), chunk by chunk.
template <int NCH>
__device__ __forceinline__ void f32_fragments(const float* rp, const float* qp, uint32_t dim, uint32_t lane, f4 (&x)[NCH],
                                              f4 (&qv)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t idx = (uint32_t)c * 256u + lane * 4u;
        const bool in = idx < dim;
        const uint32_t off = in ? idx : dim - 4u;
        x[c] = *(const f4*)(rp + off);
        const f4 v = *(const f4*)(qp + off);
        qv[c] = in ? v : (f4)(0.f);
    }
}

// The same words with every load of both issued before the first is waited for: the barrier keeps the zeroing behind the
// loads, so a row costs one round trip, not one per chunk.  For a kernel in which the compiler, left to itself, puts each
// chunk's zeroing right behind its load (the tiered tail kernel, scan_bf16.hip: seen in its code, 0.5 us per launch).
template <int NCH>
__device__ __forceinline__ void f32_fragments_batched(const float* rp, const float* qp, uint32_t dim, uint32_t lane, f4 (&x)[NCH],
                                                      f4 (&qv)[NCH]) {
    f32_row_fragments<NCH>(rp, dim, lane, x);
    f32_row_fragments<NCH>(qp, dim, lane, qv);   // (the same clamped offsets)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NCH; ++c) qv[c] = (uint32_t)c * 256u + lane * 4u < dim ? qv[c] : (f4)(0.f);
}

// The dot product of the two, in every lane: an (even, odd) packed-FMA chain over the chunks in order, even + odd, then the xor
// butterfly at distances 32 -> 1 - the tree treduce builds for every RI x BQ of the scan (each node adds the same two partial
// sums; IEEE addition commutes).  Every lane of the wave must call it.
template <int NCH>
__device__ __forceinline__ float f32_dot_chain(const f4 (&x)[NCH], const f4 (&qv)[NCH]) {
    f2 acc2 = (f2)(0.f);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const f2 xlo = __builtin_shufflevector(x[c], x[c], 0, 1);
        const f2 xhi = __builtin_shufflevector(x[c], x[c], 2, 3);
        acc2 = __builtin_elementwise_fma(xlo, __builtin_shufflevector(qv[c], qv[c], 0, 1), acc2);
        acc2 = __builtin_elementwise_fma(xhi, __builtin_shufflevector(qv[c], qv[c], 2, 3), acc2);
    }
    float s = acc2.x + acc2.y;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    return s;
}

// scan_gemv_kernel's epilogue on one score: non-finite dropped; PIPELINE (mode 1): clamp(0, 1), then `>= threshold`.
// Returns whether the row is emitted; s is then the emitted score.
__device__ __forceinline__ bool f32_emit(float& s, uint32_t mode, float thr) {
    bool keep = __builtin_fabsf(s) <= 3.4028234664e38f;
    if (keep && mode == 1u) {
        s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
        keep = s >= thr;
    }
    return keep;
}

}  // namespace cqs
