// shadow_build_device.h — one row of the dense index's shadow, converted by one wave: the per-row bodies of
// shadow_build_kernel (scan_bf16.hip), i8_build_kernel (scan_i8.hip) and row_update_kernel (index_update.hip).  The
// conversion arithmetic exists here alone, so a row that cqs_hip_index_update rewrites holds the bytes a fresh build gives
// it and folds the same terms into the same stats words.  Device code only; wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_bf16.h"
#include "scan_device.h"

namespace cqs {

typedef __bf16 bf2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }          // component 2i
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }  // component 2i + 1

constexpr int kI8BuildVecs = (int)(kShadowMaxDim / 256u);   // f4 per lane that hold a row of up to kShadowMaxDim

// The f32 row xp -> its bf16 copy op (v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN), and the row's terms of R
// into stats[0..2] (launch_shadow_build's contract).  xp and op never overlap.  The whole wave calls it; dim % 8 == 0.
__device__ __forceinline__ void shadow_build_row(const float* __restrict__ xp, uint16_t* __restrict__ op, uint32_t dim,
                                                 double gamma, unsigned long long* __restrict__ stats, int lane) {
    double d2 = 0.0, n2 = 0.0, t2 = 0.0;
    bool fin = true, big = false;
    for (uint32_t i = (uint32_t)lane * 2u; i < dim; i += 128u) {   // dim % 8 == 0: pairs never straddle the row end
        const f2 v = *(const f2*)(xp + i);
        const bf2 h = __builtin_convertvector(v, bf2);
        const uint32_t w = __builtin_bit_cast(uint32_t, h);
        *(uint32_t*)(op + i) = w;
        const float t0 = bf_lo(w), t1 = bf_hi(w);
        fin = fin && __builtin_isfinite(v.x) && __builtin_isfinite(v.y);
        big = big || __builtin_fabsf(v.x) >= 0x1p64f || __builtin_fabsf(v.y) >= 0x1p64f;
        const double e0 = (double)v.x - (double)t0, e1 = (double)v.y - (double)t1;   // exact in f64
        d2 += e0 * e0 + e1 * e1;
        n2 += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
        t2 += (double)t0 * (double)t0 + (double)t1 * (double)t1;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        d2 += __shfl_xor(d2, m, 64);
        n2 += __shfl_xor(n2, m, 64);
        t2 += __shfl_xor(t2, m, 64);
    }
    const bool all_fin = __ballot(!fin) == 0ull;
    const bool any_big = __ballot(big) != 0ull;
    if (lane == 0 && all_fin) {   // rows with a non-finite component score non-finite in both paths: no part in R
        const double nx = sqrt(n2), nt = sqrt(t2);
        const double rb = sqrt(d2) + gamma * (nx + nt);
        atomicMax(&stats[0], (unsigned long long)__double_as_longlong(rb));
        atomicMax(&stats[1], (unsigned long long)__double_as_longlong(nx > nt ? nx : nt));
        if (any_big) atomicMax(&stats[2], 1ull);
    }
}

// The f32 row xp, held in registers -> its int8 codes op and its scale *scale_out (launch_i8_build's contract), and the
// row's terms of the int8 copy's R into stats[0..2].  The whole wave calls it; dim % 16 == 0, dim <= kShadowMaxDim.
__device__ __forceinline__ void i8_build_row(const float* __restrict__ xp, int8_t* __restrict__ op,
                                             float* __restrict__ scale_out, uint32_t dim, double gamma,
                                             unsigned long long* __restrict__ stats, uint32_t lane) {
    f4 v[kI8BuildVecs];
    float m = 0.f;
    bool fin = true;
#pragma unroll
    for (int j = 0; j < kI8BuildVecs; ++j) {   // dim % 16 == 0: a lane's four floats never straddle the row end
        const uint32_t i = (uint32_t)j * 256u + lane * 4u;
        v[j] = i < dim ? *(const f4*)(xp + i) : (f4)(0.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            fin = fin && __builtin_isfinite(v[j][e]);
            m = fmaxf(m, __builtin_fabsf(v[j][e]));   // (fmaxf drops a NaN operand; `fin` carries it)
        }
    }
    m = wave_max64(m);
    const bool all_fin = __ballot(!fin) == 0ull;
    const float scale = all_fin ? m / 127.f : __builtin_nanf("");
    const bool zero = !(scale > 0.f);   // (and the non-finite rows: their codes are 0, their scale NaN)
    double d2 = 0.0, n2 = 0.0, t2 = 0.0;
#pragma unroll
    for (int j = 0; j < kI8BuildVecs; ++j) {
        const uint32_t i = (uint32_t)j * 256u + lane * 4u;
        if (i >= dim) continue;
        uint32_t w = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float c = zero ? 0.f : __builtin_rintf(v[j][e] / scale);
            c = c < -127.f ? -127.f : (c > 127.f ? 127.f : c);
            w |= ((uint32_t)(int)c & 0xFFu) << (8 * e);
            const double t = (double)scale * (double)c;   // x~: exact in f64 (24-bit scale, 7-bit code)
            const double d = (double)v[j][e] - t;
            d2 += d * d;
            n2 += (double)v[j][e] * (double)v[j][e];
            t2 += t * t;
        }
        *(uint32_t*)(op + i) = w;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        d2 += __shfl_xor(d2, s, 64);
        n2 += __shfl_xor(n2, s, 64);
        t2 += __shfl_xor(t2, s, 64);
    }
    if (lane == 0u) {
        *scale_out = scale;
        if (all_fin) {   // rows with a non-finite component score non-finite in both paths: no part in R
            const double nx = sqrt(n2), nt = sqrt(t2);
            atomicMax(&stats[0], (unsigned long long)__double_as_longlong(sqrt(d2) + gamma * (nx + nt)));
            atomicMax(&stats[1], (unsigned long long)__double_as_longlong(nx > nt ? nx : nt));
            if (m >= 0x1p64f) atomicMax(&stats[2], 1ull);
        }
    }
}

}  // namespace cqs
