// activations.h - the two GELUs of every GEMM epilogue, ONE definition each: the batch chain, the query chain and the
// fused / two-launch projections are compared with each other (tests/test_query_path_gpu.py, tests/test_embed_gpu.py),
// which holds only while they all evaluate the same expression in the same order.  Internal to libcqs_hip.so.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace cqs {
// erf GELU (BERT's hidden_act = "gelu"): 0.5 x (1 + erf(x / sqrt 2)), erf by Abramowitz-Stegun 7.1.26 (|error| <=
// 1.5e-7: one exp + one rcp + a degree-5 polynomial; libm's erff costs 40 % of the whole 768 -> 3072 GEMM here)
__device__ __forceinline__ float gelu_erf(float x) {
    const float z = __builtin_fabsf(x) * 0.70710678118654752f;
    const float t = __frcp_rn(1.0f + 0.3275911f * z);
    const float poly = ((((1.061405429f * t - 1.453152027f) * t + 1.421413741f) * t - 0.284496736f) * t + 0.254829592f) * t;
    const float e = 1.0f - poly * __expf(-z * z);            // erf(|x| / sqrt 2)
    return 0.5f * x * (1.0f + __builtin_copysignf(e, x));
}
// tanh GELU (Gemma's GeGLU gate): 0.5 x (1 + tanh(u)) = x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): one v_exp +
// one v_rcp
__device__ __forceinline__ float gelu_tanh(float x) {
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    const float two_u = 2.0f * k0 * (x + k1 * x * x * x);
    return x * __frcp_rn(1.0f + __expf(-two_u));
}
}  // namespace cqs
#endif
