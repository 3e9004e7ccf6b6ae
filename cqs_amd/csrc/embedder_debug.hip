// embedder_debug.hip — the EmbeddingGemma engine's test / tuning hooks (cqs_hip_debug_*; none is part of the public header).
#include "embedder_internal.h"

#include <algorithm>

using namespace cqs_emb;

extern "C" {

// Test hook (not part of the public header): the fused projection + add + norms kernel on / off and the token count it
// starts at, for THIS engine (the environment is read once, at finalize).  min_rows = 0 keeps the current threshold.
void cqs_hip_debug_embedder_set_fuse_norm(cqs_hip_embedder* e, int32_t on, uint32_t min_rows) CQS_ABI_TRY {
    if (!e) return;
    std::lock_guard<std::mutex> lk(e->mu);
    e->fuse_norm = on < 0 ? 0 : (on > 2 ? 2 : on);     // 0 = two launches, 1 = the 64-row kernel, 2 = the pair-split kernel
    if (min_rows) e->fuse_min_rows = min_rows;
} CQS_ABI_CATCH_VOID

// Test hook (not part of the public header): pretend a pair exchange of the fused projection kernel timed out (what the
// kernel's bounded spin reports through the pinned error word), and read how often the engine has fallen back.
void cqs_hip_debug_embedder_fake_fuse_timeout(cqs_hip_embedder* e) CQS_ABI_TRY {
    if (!e || !e->fuse_err) return;
    std::lock_guard<std::mutex> lk(e->mu);
    *(volatile unsigned*)e->fuse_err = 1u;
} CQS_ABI_CATCH_VOID
uint32_t cqs_hip_debug_embedder_fuse_fallbacks(cqs_hip_embedder* e) CQS_ABI_TRY {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return e->fuse_fallbacks;
} CQS_ABI_CATCH_VAL(0)

// Test hook (not part of the public header): the 256-row kernel's in-register GeGLU pairing on / off for THIS engine.
void cqs_hip_debug_embedder_set_geglu4(cqs_hip_embedder* e, int32_t on) CQS_ABI_TRY {
    if (!e) return;
    std::lock_guard<std::mutex> lk(e->mu);
    e->geglu4 = on != 0;
} CQS_ABI_CATCH_VOID

// Test hook (not part of the public header): the QKV projection's fused norm + RoPE epilogue on / off for THIS engine.
void cqs_hip_debug_embedder_set_fuse_qkv(cqs_hip_embedder* e, int32_t on) CQS_ABI_TRY {
    if (!e) return;
    std::lock_guard<std::mutex> lk(e->mu);
    e->fuse_qkv = on != 0;
} CQS_ABI_CATCH_VOID

// Diagnostic (not part of the public header; CQS_HIP_QUERY_STAMPS=1 at engine creation): the stamps the query chain's
// workgroups left in context `ctx` ([kernel slot][256][8] u64).  Returns the number of u64 copied.
uint64_t cqs_hip_debug_query_stamps(cqs_hip_embedder* e, uint32_t ctx, unsigned long long* out, uint64_t cap) CQS_ABI_TRY {
    if (!e || !out || ctx >= (uint32_t)cqs_hip_embedder::kCtx) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    Ctx& c = e->ctx[ctx];
    if (!c.q_dbg) return 0;
    const uint64_t words = std::min<uint64_t>(cap, ((uint64_t)e->g.layers * 5 + 2) * 256 * 8 * 2);
    if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(c.stream) != hipSuccess ||
        hipMemcpy(out, c.q_dbg, words * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return words;
} CQS_ABI_CATCH_VAL(0)

// Test hook (not part of the public header): what the search-time chain left in context `ctx`'s scratch - the state a
// query's sentence vector is pooled from and that never leaves the device otherwise.  Call it after a blocking query of
// T tokens on that context.  Waits for the context's stream, then copies out the first T rows of
//   x    f32  [T, hidden]   the residual stream entering the head (q_x0 or q_x1; *which_x says which: 0 or 1),
//   y    bf16 [T, hidden]   the last layer's down projection (the head adds rms(y, post_ffw) to x itself),
//   qkv  bf16 [T, (heads + 2 kv_heads) * 256] and h bf16 [T, intermediate] of the last layer,
// and d1 bf16 [dense_hidden], the Dense 1 output.  Any pointer may be NULL.  Only reads: launches nothing, writes no device
// memory, so the scratch stays as the query left it.
int32_t cqs_hip_debug_embedder_query_state(cqs_hip_embedder* e, uint32_t ctx, uint32_t T, float* x, uint16_t* y, uint16_t* qkv,
                                           uint16_t* h, uint16_t* d1, int32_t* which_x) CQS_ABI_TRY {
    if (!e || ctx >= (uint32_t)cqs_hip_embedder::kCtx) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    Ctx& c = e->ctx[ctx];
    if (!e->finalized || !e->query_path || !c.q_meta) return efail(e, CQS_HIP_ERR_INVALID, "query_state: no search-time query has run on this context");
    if (T < 1u || T > e->query_max_tokens) return efail(e, CQS_HIP_ERR_INVALID, "query_state: T outside the search-time chain's lengths");
    const cqs::EmbedGeom& g = e->g;
    // launch_query_forward's buffer walk: layer 0 gathers into x0 and its GeGLU prologue moves on to x1; every later layer
    // moves twice (QKV prologue, GeGLU prologue) - the head reads the buffer the last GeGLU prologue wrote
    int cur = 0;
    for (uint32_t l = 0; l < g.layers; ++l) cur ^= (l == 0 ? 1 : 0);
    E_TRY(e, hipSetDevice(e->device));
    E_TRY(e, hipStreamSynchronize(c.stream));
    const size_t H = g.hidden;
    if (x) E_TRY(e, hipMemcpy(x, cur ? c.q_x1 : c.q_x0, (size_t)T * H * sizeof(float), hipMemcpyDeviceToHost));
    if (y) E_TRY(e, hipMemcpy(y, c.q_y, (size_t)T * H * sizeof(bf16_t), hipMemcpyDeviceToHost));
    if (qkv) E_TRY(e, hipMemcpy(qkv, c.q_qkv, (size_t)T * nqkv(g) * sizeof(bf16_t), hipMemcpyDeviceToHost));
    if (h) E_TRY(e, hipMemcpy(h, c.q_h, (size_t)T * g.inter * sizeof(bf16_t), hipMemcpyDeviceToHost));
    if (d1) E_TRY(e, hipMemcpy(d1, c.q_d1, (size_t)g.dense_hidden * sizeof(bf16_t), hipMemcpyDeviceToHost));
    if (which_x) *which_x = cur;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

// Test / tuning aid (not part of the public header): one GEMM launch on caller-provided device buffers
// (bf16 A [M,K], bf16 W [N,K], C per out_kind) on `stream`; the kernel is chosen like in the forward
// (CQS_HIP_GEMM_TILE forces one).
int32_t cqs_hip_debug_gemm_run(const void* A, const void* W, void* C, uint32_t M, uint32_t N, uint32_t K, uint32_t ldc,
                               int32_t out_kind, void* stream) CQS_ABI_TRY {
    const hipError_t e = (out_kind & 0x100)   // + 0x100: the Dense head's skinny kernel
                             ? cqs::launch_gemm_skinny((const bf16_t*)A, (const bf16_t*)W, C, M, N, K, ldc,
                                                       (cqs::GemmOut)(out_kind & 0xff), (hipStream_t)stream)
                             : cqs::launch_gemm_bf16((const bf16_t*)A, (const bf16_t*)W, C, M, N, K, ldc, (cqs::GemmOut)out_kind,
                                                     (hipStream_t)stream);
    return e == hipSuccess ? CQS_HIP_OK : CQS_HIP_ERR_DEVICE;
} CQS_ABI_CATCH_NOHANDLE

// Tuning aid (not part of the public header): average milliseconds of one C[M,N] = A[M,K] W[N,K]^T
// launch over `iters` back-to-back launches on random bf16 operands.
float cqs_hip_debug_gemm_ms(uint32_t M, uint32_t N, uint32_t K, uint32_t iters, int32_t out_kind) CQS_ABI_TRY {
    bf16_t *A = nullptr, *W = nullptr;
    void* C = nullptr;
    if (dmalloc(&A, (size_t)M * K) != hipSuccess || dmalloc(&W, (size_t)N * K) != hipSuccess ||
        hipMalloc(&C, (size_t)M * N * 4) != hipSuccess) return -1.f;
    std::vector<uint16_t> h((size_t)std::max(M, N) * K);
    uint32_t st = 12345u;
    for (auto& v : h) { st = st * 1664525u + 1013904223u; v = f32_to_bf16_bits(((st >> 8) & 0xFFFF) / 32768.0f - 1.0f); }
    (void)hipMemcpy(A, h.data(), (size_t)M * K * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(W, h.data(), (size_t)N * K * 2, hipMemcpyHostToDevice);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const cqs::GemmOut ok = (cqs::GemmOut)out_kind;
    const uint32_t ldc = ok == cqs::GEMM_OUT_GEGLU ? N / 2 : N;
    (void)cqs::launch_gemm_bf16(A, W, C, M, N, K, ldc, ok, nullptr);
    (void)hipEventRecord(e0, nullptr);
    for (uint32_t i = 0; i < iters; ++i) (void)cqs::launch_gemm_bf16(A, W, C, M, N, K, ldc, ok, nullptr);
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipFree(A); (void)hipFree(W); (void)hipFree(C);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms / (float)iters;
} CQS_ABI_CATCH_VAL(-1.f)

}  // extern "C"
