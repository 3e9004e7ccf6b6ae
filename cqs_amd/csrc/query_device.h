// query_device.h — what the kernel files of the search-time chain share (query_gemm.hip, query_attention.hip,
// query_forward.hip): the kernels' parameter structs, the diagnostic stamps, the plain kernels' bias + activation, the launch
// helper with its debug-repeat form, and the launchers' signatures.  Plans and LDS layouts: query_plan.h.
#pragma once
#include "embed_kernels.h"
#include "activations.h"
#include "launch_util.h"
#include "query_plan.h"

namespace cqs {

// Diagnostic stamps (off unless the engine was created under CQS_HIP_QUERY_STAMPS=1): workgroup b (< 256) of chain
// kernel `slot` writes the 100 MHz realtime counter at phase i - where a 4 us kernel that moves 30 KB spends its time.
#define QF_STAMP(P, i)                                                                                      \
    do {                                                                                                    \
        if ((P).dbg && threadIdx.x == 0 && blockIdx.x < 256u)                                               \
            (P).dbg[((size_t)(P).dbg_slot * 256u + blockIdx.x) * 8u + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)

enum { QF_PRO_NONE = 0, QF_PRO_EMBED = 1, QF_PRO_ADDNORM = 2, QF_PRO_POOL = 3,
       QF_PRO_ADDLN = 4 /* BERT: x = LayerNorm(xb_in + y) gamma + beta (bf16 stream), the GEMM's activations = x */ };
enum { QF_EPI_BF16 = 0, QF_EPI_GEGLU = 1, QF_EPI_F32 = 2 };

struct QfGemmParams {
    const int32_t* tok;       // EMBED: token ids [T]
    const bf16_t* emb;        // EMBED: token table [vocab, H]
    float scale;              // EMBED: sqrt(H)
    const float* x_in;        // ADDNORM / POOL: residual stream [64, H] f32
    const bf16_t* y;          // ADDNORM / POOL: branch output [64, H] bf16
    const float* w_post;      // ADDNORM / POOL: post-branch norm weight [H]
    const float* w_next;      // next pre-norm weight [H] (POOL: the model's final norm)
    float* x_out;             // EMBED / ADDNORM: new residual stream [64, H] (written by workgroup 0; != x_in)
    float eps;
    const bf16_t* A;          // PRO_NONE: activations [64, K] bf16 (one_row: [K])
    const bf16_t* W;          // [N, K] bf16
    void* C;                  // [64, ldc] bf16 / f32 (POOL and its successor: one row)
    uint32_t K, ldc;
    uint32_t T;               // tokens, 1..64: a LAUNCH parameter (the engine keeps one captured graph per length)
    int32_t one_row;          // 1: the GEMM's activations are ONE row (the pooled vector)
    const float* bias;        // nullable, [N] f32 added before the activation (BERT projections; not with GEGLU)
    int32_t act;              // 1 = erf-GELU after the bias (BERT's FFN)
    const bf16_t* xb_in;      // ADDLN: the bf16 residual stream [rows, H]; w_post = gamma, w_next = beta, eps
    bf16_t* xb_out;           // ADDLN: the new stream (written by the workgroups of column tile 0; != xb_in)
    unsigned long long* dbg;  // nullable (CQS_HIP_QUERY_STAMPS=1): [kernel slot][workgroup < 256][8] realtime stamps
    uint32_t dbg_slot;
};

struct QfAttnParams {
    const bf16_t* qkv;        // [64, (heads + 2 kv) 256] bf16, as the QKV projection wrote it
    bf16_t* out;              // qf_attention_kernel: [64, heads 256] bf16
    const float* wq;          // q-head norm weight [256]
    const float* wk;          // k-head norm weight [256]
    const float* cos_sin;     // [max_seq][128][2] of the layer type
    float eps, q_scale;
    uint32_t heads, kv_heads;
    uint32_t window;          // 0 = full attention; else |q - k| < window
    uint32_t T;               // launch parameter (see QfGemmParams)
    const int32_t* pos;       // 65-128 tokens: [128] = 0, 1, 2, ... (the positions qk_norm_rope_kernel rotates by)
    // qf_attn_oproj_kernel only: y = attn Wo^T
    const bf16_t* wo;         // [H, heads 256] bf16
    bf16_t* y;                // [64, H] bf16
    uint32_t H;
    unsigned long long* dbg;
    uint32_t dbg_slot;
};

// bias + activation of the plain / staged kernels' epilogue (columns col .. col + 3)
__device__ __forceinline__ f4 qf_bias_act(f4 v, const float* __restrict__ bias, int32_t act, uint32_t col) {
    if (bias) v += *(const f4*)(bias + col);
    if (act == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
    }
    return v;
}

// Launch `kern` as the plan says, with the dynamic LDS bytes of the kernel's own layout: a plan that disagrees with the
// layout is refused before anything runs.
template <class Kern, class P>
hipError_t qf_launch(Kern kern, DynLdsOnce& once, const P& p0, const QfLaunch& l, size_t layout_lds, hipStream_t st) {
    if (l.lds_bytes != layout_lds) return hipErrorInvalidValue;
    const dim3 grid(l.grid_x, l.grid_y);
    const hipError_t e = once.ensure((const void*)kern, layout_lds);
    if (e != hipSuccess) return e;
    if (qf_switches().debug_repeat == 2 && p0.dbg) {   // diagnostic: every kernel twice (cold vs warm operands), slots 2 s and 2 s + 1
        P q = p0;
        q.dbg_slot = 2 * p0.dbg_slot;
        hipLaunchKernelGGL(kern, grid, dim3(l.threads), layout_lds, st, q);
        q.dbg_slot++;
        hipLaunchKernelGGL(kern, grid, dim3(l.threads), layout_lds, st, q);
    } else {
        hipLaunchKernelGGL(kern, grid, dim3(l.threads), layout_lds, st, p0);
    }
    return hipGetLastError();
}

// The launchers: a plan of query_plan.h -> the one template instantiation of its form.  query_gemm.hip instantiates
// qf_launch_pro for the chain's projections (hidden 256 / 768) and the BERT engines' add + LayerNorm ones, qf_launch_gemm
// for bf16 and f32 output.
template <int NCH, int PRO, int EPI>
hipError_t qf_launch_pro(const QfProPlan& pl, const QfGemmParams& p, hipStream_t st);
template <int EPI>
hipError_t qf_launch_gemm(const QfGemmPlan& pl, const QfGemmParams& p, hipStream_t st);
hipError_t qf_launch_attn(const QfAttnPlan& pl, const QfAttnParams& a, hipStream_t st);      // query_attention.hip

}  // namespace cqs
