// wave_ops.h - the wave reductions of every kernel file, and the only place that names their cross-lane builtins (DPP,
// v_permlane16/32_swap of a value WITH ITSELF, v_readlane).  One definition each: a reduction's ORDER OF ADDITIONS is part
// of the results (fused and unfused kernels, batch and query chain are compared bit for bit), so it is stated per function.
// Trap met with hipcc (ROCm 7.2): read the two results of a swap with __uint_as_float(a[i]) or through unsigned locals,
// never with __builtin_bit_cast(float, a[1]) - bit_cast of an ext-vector ELEMENT lvalue reads element 0 whatever the index
// (the front end emits `extractelement 0` twice), which turns a row-pair sum into twice the even row's value.
// Internal to libcqs_hip.so.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace cqs {
typedef unsigned lane_u2 __attribute__((ext_vector_type(2)));
// a[0] = the value of the EVEN 16-lane row of this lane's row pair, a[1] = of the ODD one, in both rows
__device__ __forceinline__ lane_u2 swap16_self(unsigned x) { return __builtin_amdgcn_permlane16_swap(x, x, false, false); }
// a[0] = the value of lanes 0-31 (same lane & 31), a[1] = of lanes 32-63, in both halves
__device__ __forceinline__ lane_u2 swap32_self(unsigned x) { return __builtin_amdgcn_permlane32_swap(x, x, false, false); }

// v of the lane that DPP control CTRL pairs this one with, inside its 16-lane row: 0xB1 = quad_perm xor 1, 0x4E = xor 2,
// 0x141 = row_half_mirror, 0x140 = row_mirror - in that order the four steps of a row reduction
template <int CTRL>
__device__ __forceinline__ float wave_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// ---- between lanes l, l ^ 16 (xor16) / l, l ^ 32 (xor32), VALU only (a __shfl_xor is a ds_bpermute trip through the LDS queue)
// max(even row, odd row) of the row pair, in both
__device__ __forceinline__ float xor16_max(float v) {
    const lane_u2 a = swap16_self(__float_as_uint(v));
    return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
// max(lanes 0-31, lanes 32-63), in both
__device__ __forceinline__ float xor32_max(float v) {
    const lane_u2 a = swap32_self(__float_as_uint(v));
    return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
// even row + odd row (in that order), in both
__device__ __forceinline__ float xor16_sum(float v) {
    const lane_u2 a = swap16_self(__float_as_uint(v));
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
// lanes 0-31 + lanes 32-63 (in that order), in both
__device__ __forceinline__ float xor32_sum(float v) {
    const lane_u2 a = swap32_self(__float_as_uint(v));
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
// the value of lane ^ 32
__device__ __forceinline__ float xor32_value(float v, int lane) {
    const lane_u2 a = swap32_self(__float_as_uint(v));
    return __uint_as_float(lane < 32 ? a[1] : a[0]);
}

// ---- maxima (exact and order-free), in every lane of the group
// over each aligned group of 16 lanes: the four DPP steps
__device__ __forceinline__ float wave_max16(float m) {
    m = fmaxf(m, wave_dpp<0xB1>(m));
    m = fmaxf(m, wave_dpp<0x4E>(m));
    m = fmaxf(m, wave_dpp<0x141>(m));
    m = fmaxf(m, wave_dpp<0x140>(m));
    return m;
}
// over each 32-lane half of the wave: rows, then the row pair
__device__ __forceinline__ float half_wave_max(float m) { return xor16_max(wave_max16(m)); }
// over the 64 lanes: rows, row pairs, halves
__device__ __forceinline__ float wave_max64(float m) { return xor32_max(xor16_max(wave_max16(m))); }

// ---- sums
// over each aligned group of 16 lanes, in all of them: v += partner at each of the four DPP steps (xor 1, xor 2, half
// mirror, mirror)
__device__ __forceinline__ float wave_sum16(float v) {
    v += wave_dpp<0xB1>(v);
    v += wave_dpp<0x4E>(v);
    v += wave_dpp<0x141>(v);
    v += wave_dpp<0x140>(v);
    return v;
}
// over the 32 lanes of this lane's half-wave, the same bits in all of them: wave_sum16, then even row + odd row.  The row
// norms of add_norm_kernel, of the pair-split fused kernel and of the QKV epilogue all add in this order.
__device__ __forceinline__ float half_wave_sum32(float v) { return xor16_sum(wave_sum16(v)); }
// over the wave as (lanes 0-31) + (lanes 32-63) of half_wave_sum32: the order in which two workgroups that own the two
// column halves of a row (gemm_rowfuse.hip) can also sum, so add_norm_kernel and the pair-split kernel stay bit-identical
__device__ __forceinline__ float row_sum_of_halves(float v) { return xor32_sum(half_wave_sum32(v)); }
// over the wave, uniform (scalar registers): wave_sum16, then ((row 0 + row 1) + row 2) + row 3 through four v_readlane
__device__ __forceinline__ float wave_sum64_readlane(float v) {
    const int b = __builtin_bit_cast(int, wave_sum16(v));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
}
// over the wave, in every lane: the __shfl_xor butterfly v += lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  That order of additions
// is part of the results of every kernel that calls it (tests compare them bit for bit with each other and with recorded
// outputs): not to be "upgraded" to the DPP forms above, which add in another order.
__device__ __forceinline__ float wave_sum64_shfl(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the same butterfly over f64 (two ds_bpermute a step): every lane ends with the same bits, v[l] + v[l ^ off] being the
// same addition in both partners.  index_diff.hip's three sums add in this order; diff_host.h restates it on 64 host slots.
__device__ __forceinline__ double wave_sum64_shfl(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
}  // namespace cqs
#endif
