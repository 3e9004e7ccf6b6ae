// engine_common.h — what the handles of the two transformer engines (embedder_internal.h, bert_internal.h) share that is not the
// ticket protocol (ticket_pool.h): the weights' rounding to bf16, and under hipcc the failure rule, typed device allocation and
// the growth of a pinned buffer.  The rounding is device-free: tests/ticket_pool_driver.cpp checks it on the CPU.
#pragma once
#include <stdint.h>
#include <string.h>

namespace cqs {

// f32 -> bf16 bits, round to nearest even; a NaN (signalling ones included) stays a NaN instead of rounding up to infinity.
inline uint16_t f32_to_bf16_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

}  // namespace cqs

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "../../include/cqs_hip.h"

namespace cqs {

// E: a handle with `std::string last_error` and `std::atomic<bool> poisoned`.  A device error poisons the handle.
template <class E>
int32_t efail(E* e, int32_t code, const std::string& what, hipError_t he = hipSuccess) {
    std::string msg = what;
    if (he != hipSuccess) msg += std::string(": ") + hipGetErrorString(he);
    if (e) {
        e->last_error = msg;
        if (code == CQS_HIP_ERR_DEVICE) e->poisoned.store(true, std::memory_order_release);
    }
    return code;
}
#define E_TRY(e, expr)                                                                                                               \
    do {                                                                                                                             \
        hipError_t _h = (expr);                                                                                                      \
        if (_h != hipSuccess) return cqs::efail((e), _h == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, #expr, _h); \
    } while (0)

template <class T>
hipError_t dmalloc(T** p, size_t count) { return hipMalloc((void**)p, count * sizeof(T)); }

// A pinned host buffer of at least `need` bytes (*cap: the bytes it holds), grown with a quarter of slack so that batches of
// creeping sizes do not reallocate each time.  The old contents are dropped; a failure leaves it empty.
template <class T>
hipError_t grow_pinned(T** p, size_t* cap, size_t need) {
    if (need <= *cap) return hipSuccess;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t bytes = need + need / 4 + 256;
    const hipError_t he = hipHostMalloc((void**)p, bytes, hipHostMallocDefault);
    if (he == hipSuccess) *cap = bytes;
    return he;
}

}  // namespace cqs
#endif
