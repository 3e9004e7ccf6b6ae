// scan_device.h — device helpers shared by the scan kernels (the f32 scan scan_kernels.hip, the shadow scans scan_bf16.hip
// and scan_i8.hip) and the select (select_device.h): the vector typedefs, the ordered score keys and the transposed
// butterfly.  What only the three HBM-streaming scans' launchers and dequeue share is in scan_gemv_device.h.
// Internal to libcqs_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cqs {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) uint32_t kc32;   // constant address space: uniform addresses load through the scalar cache

// ---- ordered keys ----------------------------------------------------------
// f32 -> u32 preserving IEEE total order (what Rust's f32::total_cmp sorts by).
__device__ __forceinline__ uint32_t okey(float x) {
    uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// Dropped entries are stored as -inf: okey(-inf) = 0x007FFFFF.  Every finite
// score has a larger key; +inf / NaN never reach the score rows.
constexpr uint32_t kInvalidKey = 0x007FFFFFu;

__device__ __forceinline__ uint64_t pack_key(uint32_t ok, uint32_t global_row) {
    return ((uint64_t)ok << 32) | (uint64_t)(0xFFFFFFFFu - global_row);
}

// ---- transposed butterfly reduction ---------------------------------------
// v[0..NV) hold per-lane partial sums of NV independent dot products.  After
// the call v[0] of lane L is the complete sum of product number L / (64/NV).
// Cost: NV-1 + log2(64/NV) cross-lane ops instead of 6*NV.
template <int N, int M, int NV>
__device__ __forceinline__ void treduce_level(float (&v)[NV], int lane) {
    // Compile-time level (N live values, exchange distance M): a runtime loop over the levels makes
    // v[i + n/2] a variable index, which hipcc lowers to an NV-way v_cmp/v_cndmask chain per element.
    if constexpr (N > 1) {
        const bool hi = (lane & M) != 0;
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const float keep = hi ? v[i + N / 2] : v[i];
            const float send = hi ? v[i] : v[i + N / 2];
            v[i] = keep + __shfl_xor(send, M, 64);
        }
        treduce_level<N / 2, M / 2, NV>(v, lane);
    } else if constexpr (M >= 1) {
        v[0] += __shfl_xor(v[0], M, 64);
        treduce_level<1, M / 2, NV>(v, lane);
    }
}
template <int NV>
__device__ __forceinline__ void treduce(float (&v)[NV], int lane) {
    treduce_level<NV, 32, NV>(v, lane);
}

}  // namespace cqs
