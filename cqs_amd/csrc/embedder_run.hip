// embedder_run.hip — the EmbeddingGemma forward behind the C ABI (include/cqs_hip.h, embed section): a context's scratch, batch
// packing (batch_tables.h), the batch chain, the search-time chain with its graph capture, and the submit / collect tickets
// (ticket_pool.h).  The handle: embedder_internal.h; the weights: embedder.hip.
#include "embedder_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>

#include "roctx.h"

using namespace cqs_emb;

void cqs_emb::free_query_scratch(Ctx& c) {
    for (int v = 0; v < 2; ++v)
        for (uint32_t i = 0; i < cqs::kQueryFwdMaxTokens; ++i) {
            if (c.q_exec[v][i]) (void)hipGraphExecDestroy(c.q_exec[v][i]);
            if (c.q_graph[v][i]) (void)hipGraphDestroy(c.q_graph[v][i]);
            c.q_exec[v][i] = nullptr; c.q_graph[v][i] = nullptr;
        }
    if (c.q_tok_pin) (void)hipHostFree(c.q_tok_pin);
    if (c.q_out_pin) (void)hipHostFree(c.q_out_pin);
    c.q_tok_pin = nullptr; c.q_out_pin = nullptr; c.q_tok_pin_dev = nullptr; c.q_out_pin_dev = nullptr;
    void** all[] = {(void**)&c.q_dbg, (void**)&c.q_pos, (void**)&c.q_meta, (void**)&c.q_x0, (void**)&c.q_x1, (void**)&c.q_out, (void**)&c.q_qkv, (void**)&c.q_attn,
                    (void**)&c.q_y, (void**)&c.q_h, (void**)&c.q_d1};
    for (void** p : all) { (void)hipFree(*p); *p = nullptr; }
}

void cqs_emb::free_scratch(Ctx& c) {
    void** all[] = {(void**)&c.x, (void**)&c.y, (void**)&c.hidden, (void**)&c.out, (void**)&c.xn, (void**)&c.qkv,
                    (void**)&c.vt, (void**)&c.attn, (void**)&c.h, (void**)&c.pooled, (void**)&c.d1, (void**)&c.d_meta, &c.xch};
    for (void** p : all) { (void)hipFree(*p); *p = nullptr; }
    c.tb = {};
    c.tok_cap = c.seq_cap = c.vt_ld = c.blk_cap = 0;
}

namespace {

constexpr cqs::BatchKind kKind = cqs::BATCH_GEMMA;

int32_t ensure_scratch(cqs_hip_embedder* e, Ctx& c, const cqs::BatchShape& s) {
    const cqs::EmbedGeom& g = e->g;
    if (s.M <= c.tok_cap && s.B <= c.seq_cap && s.vt_cols <= c.vt_ld && s.nblk <= c.blk_cap) return CQS_HIP_OK;
    E_TRY(e, hipStreamSynchronize(c.stream));
    const uint32_t Mc = std::max(s.M, c.tok_cap), Bc = std::max(s.B, c.seq_cap);
    const uint32_t vc = std::max(s.vt_cols, c.vt_ld), bc = std::max(s.nblk, c.blk_cap);
    free_scratch(c);   // pointers nulled, capacities zeroed: a failed hipMalloc below leaves a consistent (empty) scratch
    const size_t H = g.hidden;
    E_TRY(e, dmalloc(&c.x, (size_t)Mc * H));
    E_TRY(e, dmalloc(&c.y, (size_t)Mc * H));
    E_TRY(e, dmalloc(&c.hidden, (size_t)Mc * H));
    E_TRY(e, dmalloc(&c.out, (size_t)Bc * H));
    E_TRY(e, dmalloc(&c.xn, (size_t)Mc * H));
    E_TRY(e, dmalloc(&c.qkv, (size_t)Mc * nqkv(g)));
    E_TRY(e, dmalloc(&c.vt, (size_t)g.kv_heads * g.head_dim * vc));
    E_TRY(e, hipMemset(c.vt, 0, (size_t)g.kv_heads * g.head_dim * vc * sizeof(bf16_t)));  // pad columns stay finite
    E_TRY(e, dmalloc(&c.attn, (size_t)Mc * g.heads * g.head_dim));
    E_TRY(e, dmalloc(&c.h, (size_t)Mc * g.inter));
    E_TRY(e, dmalloc(&c.pooled, (size_t)Bc * H));
    E_TRY(e, dmalloc(&c.d1, (size_t)Bc * g.dense_hidden));
    E_TRY(e, dmalloc(&c.d_meta, cqs::table_words(kKind, {Bc, Mc, bc, vc})));
    E_TRY(e, hipMalloc(&c.xch, cqs::gemm_addnorm_pair_scratch_bytes(Mc)));
    E_TRY(e, hipMemset(c.xch, 0, cqs::gemm_addnorm_pair_scratch_bytes(Mc)));     // tag 0 = never written
    c.xch_tag = 0;
    c.tok_cap = Mc; c.seq_cap = Bc; c.vt_ld = vc; c.blk_cap = bc;
    return CQS_HIP_OK;
}

// ---- batch packing into a submission slot ------------------------------------------------------------------
int32_t slot_reserve(cqs_hip_embedder* e, Slot& sl, const cqs::BatchShape& s) {
    E_TRY(e, cqs::grow_pinned(&sl.meta, &sl.meta_cap, cqs::table_words(kKind, s) * sizeof(int32_t)));
    E_TRY(e, cqs::grow_pinned(&sl.out, &sl.out_cap, (size_t)s.B * e->g.hidden * sizeof(float)));
    if (!sl.ev0) {
        E_TRY(e, hipEventCreate(&sl.ev0));
        E_TRY(e, hipEventCreate(&sl.ev1));
        E_TRY(e, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    sl.shape = s;
    return CQS_HIP_OK;
}

// batch_tables.h's refusals as this engine's errors
int32_t table_fail(cqs_hip_embedder* e, cqs::BatchCode code) {
    const char* what = code == cqs::BATCH_TOO_LONG          ? "embed: sequence longer than max_seq"
                       : code == cqs::BATCH_TOO_MANY_TOKENS ? "embed: batch holds too many tokens"
                       : code == cqs::BATCH_MASK_NOT_PREFIX ? "embed: attention_mask must be a right-padded prefix mask"
                                                            : "embed: token id out of range";
    return code == cqs::BATCH_OK ? CQS_HIP_OK : efail(e, CQS_HIP_ERR_INVALID, what);
}

// Fill the slot's tables from per-sequence lengths + a token fetcher (sequence, position in it, packed row).
template <class TokAt>
int32_t slot_fill(cqs_hip_embedder* e, Slot& sl, const uint32_t* lens, uint32_t B, TokAt tok_at) {
    cqs::BatchShape s;
    int32_t rc = table_fail(e, cqs::batch_shape(kKind, lens, B, e->g.max_seq, &s));
    if (rc == CQS_HIP_OK) rc = slot_reserve(e, sl, s);
    if (rc != CQS_HIP_OK) return rc;
    return table_fail(e, cqs::fill_tables(kKind, cqs::carve(kKind, sl.meta, s), s, lens, tok_at, cqs::NoTypes{}, (int64_t)e->g.vocab, 0));
}

// The padded [B, L] contract of `session.run` (src/embedder/core.rs:1031-1035): mask rows are 1...10...0.
int32_t pack_padded(cqs_hip_embedder* e, Slot& sl, const int64_t* ids, const int64_t* mask, uint32_t B, uint32_t L) {
    std::vector<uint32_t> lens(B);
    const int32_t rc = table_fail(e, cqs::prefix_lens(mask, B, L, e->g.max_seq, lens.data()));
    if (rc != CQS_HIP_OK) return rc;
    return slot_fill(e, sl, lens.data(), B, [&](uint32_t b, uint32_t j, uint32_t) { return ids[(size_t)b * L + j]; });
}

int32_t pack_ragged(cqs_hip_embedder* e, Slot& sl, const int32_t* tokens, const uint32_t* lens, uint32_t B) {
    return slot_fill(e, sl, lens, B, [&](uint32_t, uint32_t, uint32_t row) { return (int64_t)tokens[row]; });
}

// Enqueue on the context's stream: tables H2D (one copy), the layers; leaves `hidden` (final norm, packed) in its scratch.
int32_t run_layers(cqs_hip_embedder* e, Ctx& c, Slot& sl) {
    const cqs::EmbedGeom& g = e->g;
    const uint32_t M = sl.shape.M, H = g.hidden;
    hipStream_t st = c.stream;
    int32_t rc = ensure_scratch(e, c, sl.shape);
    if (rc != CQS_HIP_OK) return rc;
    c.tb = cqs::carve<const int32_t>(kKind, c.d_meta, sl.shape);
    E_TRY(e, hipMemcpyAsync(c.d_meta, sl.meta, cqs::table_words(kKind, sl.shape) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    E_TRY(e, hipEventRecord(sl.ev0, st));
    const uint32_t nblk = sl.shape.nblk;
    const bool need_vt = cqs::attention_reads_vt(nblk, g.heads, g.kv_heads);
    int qkv_tn = (e->fuse_qkv && !need_vt) ? cqs::gemm_qkv_rope_tile(M, H, g.heads, g.kv_heads, g.head_dim) : 0;
    if (qkv_tn == 5 && !e->L[0].wqkv_f) qkv_tn = 0;
    const bool qkv_fused = qkv_tn != 0;
    E_TRY(e, cqs::launch_embed_norm(c.tb.tok, e->emb, sqrtf((float)H), e->L[0].n_in, g.rms_eps, c.x, c.xn, M, H, st));
    for (uint32_t l = 0; l < g.layers; ++l) {
        const LayerW& w = e->L[l];
        const bool full = ((l + 1u) % g.sliding_pattern) == 0u;
        const float* rope = full ? e->rope_global : e->rope_local;
        // QKV projection.  Full rounds of 256 x 320 tiles: each tile = one q / k head + a slice of v, and the GEMM's epilogue
        // does the head's RMSNorm + RoPE (+ q scale) itself - no kv_prep launch, no Q prologue in the attention kernel
        if (qkv_fused) {
            cqs::QkvEpilogue ep{c.tb.pos, w.n_q, w.n_k, rope, g.rms_eps, g.q_scale, g.heads, g.kv_heads};
            E_TRY(e, cqs::launch_gemm_qkv_rope(c.xn, qkv_tn == 5 ? w.wqkv_f : w.wqkv, c.qkv, M, H, qkv_tn, ep, st));
        } else {
            E_TRY(e, cqs::launch_gemm_bf16(c.xn, w.wqkv, c.qkv, M, nqkv(g), H, nqkv(g), cqs::GEMM_OUT_BF16, st));
            // k heads + V^T here; the attention kernel normalises / rotates its own Q fragments (q is 3/4 of the rope's bytes)
            E_TRY(e, cqs::launch_kv_prep(c.qkv, c.vt, c.tb.pos, w.n_q, w.n_k, rope, g.rms_eps, g.q_scale, M, g.heads, g.kv_heads,
                                         c.tb.blk, nblk, c.tb.seq_start, c.tb.seq_len, c.tb.vt_start, c.vt_ld, need_vt ? 1 : 0, st));
        }
        E_TRY(e, cqs::launch_attention(c.qkv, c.vt, c.attn, c.tb.blk, nblk, c.tb.seq_start, c.tb.seq_len,
                                       c.tb.vt_start, c.vt_ld, g.heads, g.kv_heads, full ? 0u : g.window, qkv_fused ? nullptr : w.n_q, rope,
                                       g.rms_eps, g.q_scale, st));
        const int fuse = (e->fuse_norm && M >= e->fuse_min_rows && e->fuse_err_dev) ? e->fuse_norm : 0;
        auto proj_norm = [&](const bf16_t* Ain, const bf16_t* Wp, const bf16_t* Wpk, uint32_t Kp, const float* wpost, const float* wnext, float* outp, int fin) -> int32_t {
            if (fuse == 2 && Wpk && cqs::gemm_addnorm_supported(M, H, Kp)) {
                if (++c.xch_tag == 0u) c.xch_tag = 1u;
                E_TRY(e, cqs::launch_gemm_addnorm_pair(Ain, Wpk, c.x, wpost, wnext, g.rms_eps, c.xn, outp, fin, M, H, Kp, c.xch, c.xch_tag, e->fuse_err_dev, st));
            } else if (fuse == 1 && cqs::gemm_addnorm_supported(M, H, Kp)) {
                E_TRY(e, cqs::launch_gemm_addnorm(Ain, Wp, c.x, wpost, wnext, g.rms_eps, c.xn, outp, fin, M, H, Kp, st));
            } else {
                E_TRY(e, cqs::launch_gemm_bf16(Ain, Wp, c.y, M, H, Kp, H, cqs::GEMM_OUT_BF16, st));
                E_TRY(e, cqs::launch_add_norm(c.x, c.y, wpost, wnext, g.rms_eps, c.xn, outp, fin, M, H, st));
            }
            return CQS_HIP_OK;
        };
        // o_proj, then x += norm(y)(1 + w); xn = norm(x)(1 + w'): one launch where workgroups can own whole rows
        if ((rc = proj_norm(c.attn, w.wo, w.wo_p, g.heads * g.head_dim, w.n_post_attn, w.n_pre_ffw, nullptr, 0)) != CQS_HIP_OK) return rc;
        E_TRY(e, cqs::launch_gemm_bf16(c.xn, w.wgu, c.h, M, 2u * g.inter, H, g.inter, cqs::GEMM_OUT_GEGLU, st, nullptr, e->geglu4 ? w.wgu_f : nullptr));
        const bool last = (l + 1u == g.layers);
        const float* w_next = last ? e->n_final : e->L[l + 1].n_in;
        if ((rc = proj_norm(c.h, w.wd, w.wd_p, g.inter, w.n_post_ffw, w_next, c.hidden, last ? 1 : 0)) != CQS_HIP_OK) return rc;
    }
    return CQS_HIP_OK;
}

// ---- the search-time path: ONE sequence of <= 64 tokens (`embed_query`, src/embedder/core.rs:768-856) ---------------
// 98 launches (4 per layer + 2) of query_forward.hip instead of the batch chain's ~230, replayed from a hipGraph
// captured on the context's second query (eager launches of 2-3 us kernels are host-bound: ~3.5 us of host time each).
bool slot_takes_query_path(const cqs_hip_embedder* e, const Slot& sl) {
    return e->query_path && sl.shape.B == 1 && sl.shape.M >= 1 && sl.shape.M <= e->query_max_tokens;
}

int32_t ensure_query_scratch(cqs_hip_embedder* e, Ctx& c) {
    if (c.q_meta) return CQS_HIP_OK;
    const cqs::EmbedGeom& g = e->g;
    const size_t R = cqs::kQueryFwdMaxTokens, H = g.hidden;
    hipError_t he = hipSuccess;
    auto grab = [&](auto** p, size_t count) { if (he == hipSuccess) he = dmalloc(p, count); };
    grab(&c.q_meta, R + 1); grab(&c.q_pos, R); grab(&c.q_x0, R * H); grab(&c.q_x1, R * H); grab(&c.q_out, H);
    grab(&c.q_qkv, R * nqkv(g)); grab(&c.q_attn, R * g.heads * g.head_dim); grab(&c.q_y, R * H); grab(&c.q_h, R * g.inter);
    grab(&c.q_d1, (size_t)g.dense_hidden);
    // rows past a query's length are read (never used): keep them finite from the start
    if (he == hipSuccess && getenv("CQS_HIP_QUERY_STAMPS")) {
        const size_t words = ((size_t)g.layers * 5 + 2) * 256 * 8 * 2;   // x 2: CQS_HIP_QUERY_DEBUG_REPEAT=2
        grab(&c.q_dbg, words);
        if (he == hipSuccess) he = hipMemsetAsync(c.q_dbg, 0, words * 8, c.stream);
    }
    if (he == hipSuccess) he = hipHostMalloc((void**)&c.q_tok_pin, R * sizeof(int32_t), hipHostMallocDefault);
    if (he == hipSuccess) he = hipHostMalloc((void**)&c.q_out_pin, H * sizeof(float), hipHostMallocDefault);
    if (he == hipSuccess) he = hipHostGetDevicePointer((void**)&c.q_tok_pin_dev, c.q_tok_pin, 0);
    if (he == hipSuccess) he = hipHostGetDevicePointer((void**)&c.q_out_pin_dev, c.q_out_pin, 0);
    if (he == hipSuccess) memset(c.q_tok_pin, 0, R * sizeof(int32_t));
    if (he == hipSuccess) {
        std::vector<int32_t> iota(R);
        for (size_t i = 0; i < R; ++i) iota[i] = (int32_t)i;
        he = hipMemcpy(c.q_pos, iota.data(), R * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    if (he == hipSuccess) he = hipMemsetAsync(c.q_x0, 0, R * H * 4, c.stream);
    if (he == hipSuccess) he = hipMemsetAsync(c.q_x1, 0, R * H * 4, c.stream);
    if (he == hipSuccess) he = hipMemsetAsync(c.q_qkv, 0, R * nqkv(g) * 2, c.stream);
    if (he == hipSuccess) he = hipMemsetAsync(c.q_attn, 0, R * g.heads * g.head_dim * 2, c.stream);
    if (he == hipSuccess) he = hipMemsetAsync(c.q_y, 0, R * H * 2, c.stream);
    if (he == hipSuccess) he = hipMemsetAsync(c.q_h, 0, R * g.inter * 2, c.stream);
    if (he != hipSuccess) {
        free_query_scratch(c);
        return efail(e, he == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, "query scratch", he);
    }
    return CQS_HIP_OK;
}

// Enqueue on the context's stream: [T, tokens] H2D, the chain (graph replay once captured); leaves the sentence
// vector (f32 [hidden], not normalised) in c.q_out.
int32_t run_query(cqs_hip_embedder* e, Ctx& c, Slot& sl, bool direct) {
    const cqs::EmbedGeom& g = e->g;
    hipStream_t st = c.stream;
    int32_t rc = ensure_query_scratch(e, c);
    if (rc != CQS_HIP_OK) return rc;
    const int var = direct ? 1 : 0;
    const int32_t* tok = cqs::carve<const int32_t>(kKind, sl.meta, sl.shape).tok;
    if (direct) memcpy(c.q_tok_pin, tok, (size_t)sl.shape.M * sizeof(int32_t));     // the context is idle: nobody reads it now
    else E_TRY(e, hipMemcpyAsync(c.q_meta, tok, (size_t)sl.shape.M * sizeof(int32_t), hipMemcpyHostToDevice, st));
    E_TRY(e, hipEventRecord(sl.ev0, st));
    cqs::QueryFwd f{};
    f.tok = c.q_meta; f.pos = c.q_pos; f.T = sl.shape.M; f.emb = e->emb; f.embed_scale = sqrtf((float)g.hidden); f.layer = e->QL.data(); f.layers = g.layers;
    f.n_final = e->n_final; f.dense1 = e->dense1; f.dense2 = e->dense2; f.rope_global = e->rope_global; f.rope_local = e->rope_local;
    f.hidden = g.hidden; f.heads = g.heads; f.kv_heads = g.kv_heads; f.inter = g.inter; f.dense_hidden = g.dense_hidden;
    f.window = g.window; f.sliding_pattern = g.sliding_pattern; f.eps = g.rms_eps; f.q_scale = g.q_scale;
    f.dbg = c.q_dbg;
    f.x0 = c.q_x0; f.x1 = c.q_x1; f.qkv = c.q_qkv; f.attn = c.q_attn; f.y = c.q_y; f.h = c.q_h; f.d1 = c.q_d1; f.out = c.q_out;
    if (direct) { f.tok = c.q_tok_pin_dev; f.out = c.q_out_pin_dev; }
    const int gi = (int)sl.shape.M - 1;
    if (c.q_exec[var][gi]) {
        E_TRY(e, hipGraphLaunch(c.q_exec[var][gi], st));
        e->q_replays++;
        return CQS_HIP_OK;
    }
    if (e->query_graph && !c.q_capture_failed[var][gi] && e->q_len_ran[gi]) {
        // capture the chain (kernel launches only; every argument is a fixed device address), instantiate, replay
        const char* stage = "hipStreamBeginCapture";
        hipError_t he = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (he == hipSuccess) {
            const hipError_t le = cqs::launch_query_forward(f, st);
            hipGraph_t gr = nullptr;
            he = hipStreamEndCapture(st, &gr);
            stage = "hipStreamEndCapture";
            if (he == hipSuccess && le != hipSuccess) { he = le; stage = "a launch inside the capture"; }
            if (he == hipSuccess) { he = hipGraphInstantiate(&c.q_exec[var][gi], gr, nullptr, nullptr, 0); stage = "hipGraphInstantiate"; }
            if (he == hipSuccess) {
                c.q_graph[var][gi] = gr;
                e->q_captured++;
                E_TRY(e, hipGraphLaunch(c.q_exec[var][gi], st));
                e->q_replays++;
                return CQS_HIP_OK;
            }
            if (gr) (void)hipGraphDestroy(gr);
            c.q_exec[var][gi] = nullptr;
        }
        (void)hipGetLastError();
        // not a device failure (the eager chain below computes the same thing), but never silent: counted, latched for
        // this (variant, length) only, and the cause is left in last_error
        c.q_capture_failed[var][gi] = true;
        e->q_capture_failures++;
        e->last_error = std::string("query graph capture failed at ") + stage + " (" + std::to_string(sl.shape.M) + " tokens, variant " +
                        std::to_string(var) + "): " + hipGetErrorString(he) + "; this length runs eagerly";
    }
    E_TRY(e, cqs::launch_query_forward(f, st));
    e->q_len_ran[gi] = true;
    e->q_eager++;
    return CQS_HIP_OK;
}

// ---- submit / collect ---------------------------------------------------------------------------------------
// submit: validate + pack into a free slot's pinned tables (host work), enqueue H2D + forward + pool / dense +
// D2H on the engine's stream, return a ticket; nothing waits for the device.  collect: wait for that slot's
// event, hand the rows out.  With kSlots tickets in flight the host packs batch i+1 (and the caller tokenises
// batch i+2) while the device runs batch i - the overlap the reference gets from its parse -> embed -> write
// channel pipeline (src/cli/pipeline/mod.rs:61-244), moved under the `session.run` seam.

// The batch path of one packed slot: H2D of its tables, the layers, pool + Dense head, D2H, the slot's events.
int32_t enqueue_batch_chain(cqs_hip_embedder* e, Ctx& c, Slot& sl) {
    hipStream_t st = c.stream;
    const uint32_t H = e->g.hidden, B = sl.shape.B;
    int32_t rc = run_layers(e, c, sl);
    if (rc != CQS_HIP_OK) return rc;
    const cqs::EmbedGeom& g = e->g;
    E_TRY(e, cqs::launch_mean_pool(c.hidden, c.tb.seq_start, c.tb.seq_len, c.pooled, B, H, st));
    E_TRY(e, cqs::launch_gemm_skinny(c.pooled, e->dense1, c.d1, B, g.dense_hidden, H, g.dense_hidden, cqs::GEMM_OUT_BF16, st));
    E_TRY(e, cqs::launch_gemm_skinny(c.d1, e->dense2, c.out, B, H, g.dense_hidden, H, cqs::GEMM_OUT_F32, st));
    E_TRY(e, hipEventRecord(sl.ev1, st));
    E_TRY(e, hipMemcpyAsync(sl.out, c.out, (size_t)B * H * sizeof(float), hipMemcpyDeviceToHost, st));
    E_TRY(e, hipEventRecord(sl.done, st));
    return CQS_HIP_OK;
}

// The number of a slot with no ticket in flight; kNone (and last_error set) when there is none.
int free_slot(cqs_hip_embedder* e) {
    const int si = e->pool.take();
    if (si == e->pool.kNone) (void)efail(e, CQS_HIP_ERR_INVALID, "embed: every submission slot is in flight (collect a ticket first)");
    return si;
}

int32_t submit_locked(cqs_hip_embedder* e, uint32_t B, const std::function<int32_t(Slot&)>& pack, uint64_t* ticket) {
    if (e->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (!e->finalized) return efail(e, CQS_HIP_ERR_INVALID, "embed: weights not finalized");
    if (!ticket) return efail(e, CQS_HIP_ERR_INVALID, "embed: null ticket");
    *ticket = 0;
    if (B == 0) return efail(e, CQS_HIP_ERR_INVALID, "embed: empty batch");
    const int si = free_slot(e);
    if (si == e->pool.kNone) return CQS_HIP_ERR_INVALID;
    Slot* sl = &e->slot[si];
    E_TRY(e, hipSetDevice(e->device));
    int32_t rc = pack(*sl);
    if (rc != CQS_HIP_OK) return rc;
    sl->direct = sl->batch_chain = sl->rerun = false;
    // the context with fewer tickets in flight, unless the batch fills the CUs on its own (batch_tables.h: both rules) or
    // CQS_HIP_EMBED_CONTEXTS=1 puts every ticket on one stream (tickets still overlap host packing / copies)
    const auto chosen = e->pool.choose_context(si, cqs::exact_rounds(sl->shape.M, e->n_cu) || e->single_ctx);
    const int ci = chosen.ctx;
    Ctx& c = e->ctx[ci];
    hipStream_t st = c.stream;
    const uint32_t H = e->g.hidden;
    if (sl->shape.M == 0) {
        // every row empty: zero vectors (src/embedder/pooling.rs:113-119); still a ticket, nothing enqueued
        memset(sl->out, 0, (size_t)B * H * sizeof(float));
        E_TRY(e, hipEventRecord(sl->ev0, st));
        E_TRY(e, hipEventRecord(sl->ev1, st));
        E_TRY(e, hipEventRecord(sl->done, st));
    } else if (slot_takes_query_path(e, *sl)) {
        sl->direct = e->query_direct && chosen.load[ci] == 0;   // nothing else in flight on this context
        rc = run_query(e, c, *sl, sl->direct);
        if (rc != CQS_HIP_OK) return rc;
        E_TRY(e, hipEventRecord(sl->ev1, st));
        if (!sl->direct) E_TRY(e, hipMemcpyAsync(sl->out, c.q_out, (size_t)H * sizeof(float), hipMemcpyDeviceToHost, st));
        E_TRY(e, hipEventRecord(sl->done, st));
    } else {
        rc = enqueue_batch_chain(e, c, *sl);
        if (rc != CQS_HIP_OK) return rc;
        sl->batch_chain = true;
    }
    *ticket = e->pool.publish(si, 0);
    return CQS_HIP_OK;
}

}  // namespace

extern "C" {

int32_t cqs_hip_embed_submit(cqs_hip_embedder* e, const int64_t* ids, const int64_t* mask, uint32_t B, uint32_t L,
                             uint64_t* ticket) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_embed_submit");
    if (!e) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!ids || !mask || L == 0) return efail(e, CQS_HIP_ERR_INVALID, "embed: null buffer / empty sequence");
    return submit_locked(e, B, [&](Slot& sl) { return pack_padded(e, sl, ids, mask, B, L); }, ticket);
} CQS_ABI_CATCH(e)

int32_t cqs_hip_embed_submit_ragged(cqs_hip_embedder* e, const int32_t* tokens, const uint32_t* lens, uint32_t B,
                                    uint64_t* ticket) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_embed_submit_ragged");
    if (!e) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!lens || (!tokens && B)) return efail(e, CQS_HIP_ERR_INVALID, "embed: null buffer");
    return submit_locked(e, B, [&](Slot& sl) { return pack_ragged(e, sl, tokens, lens, B); }, ticket);
} CQS_ABI_CATCH(e)

int32_t cqs_hip_embed_collect(cqs_hip_embedder* e, uint64_t ticket, float* out) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_embed_collect");
    if (!e) return CQS_HIP_ERR_INVALID;
    int si = 0;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (ticket == 0) return efail(e, CQS_HIP_ERR_INVALID, "collect: null ticket");
        const cqs::CollectCode cc = e->pool.begin_collect(ticket, 0, &si);
        if (cc == cqs::COLLECT_UNKNOWN) return efail(e, CQS_HIP_ERR_INVALID, "collect: unknown ticket");
        if (cc == cqs::COLLECT_BUSY) return efail(e, CQS_HIP_ERR_INVALID, "collect: this ticket is already being collected");
    }
    Slot* sl = &e->slot[si];
    // wait outside the lock: other threads may submit meanwhile; the slot stays ours until the guard below lets it go
    (void)hipSetDevice(e->device);
    const hipError_t he = hipEventSynchronize(sl->done);
    std::lock_guard<std::mutex> lk(e->mu);
    decltype(e->pool)::Collecting release{e->pool, si};
    Ctx& c = e->ctx[e->pool.slot[si].ctx];
    if (he != hipSuccess) return efail(e, CQS_HIP_ERR_DEVICE, "collect: device failure", he);
    if (e->fuse_err && *(volatile unsigned*)e->fuse_err != 0u) {
        // A pair of the fused projection kernel never met (gemm_rowfuse.hip: workgroup b waits for granules of workgroup
        // b ^ 8 of the same launch, which needs both resident - true on an otherwise idle device, not promised by HIP):
        // rows of EVERY batch-chain ticket in flight may be garbage.  Round 5: the engine drops to the
        // two-launch chain (no cross-workgroup exchange, the same bits) for good and recomputes those tickets - this
        // one here, the others at their own collect - instead of poisoning itself.
        (void)hipDeviceSynchronize();
        *(volatile unsigned*)e->fuse_err = 0u;
        e->fuse_norm = 0;
        e->fuse_fallbacks++;
        e->pool.for_each_in_flight([&](int i) { if (e->slot[i].batch_chain) e->slot[i].rerun = true; });
    }
    if (sl->rerun) {
        sl->rerun = false;
        int32_t rc = enqueue_batch_chain(e, c, *sl);
        if (rc == CQS_HIP_OK && hipEventSynchronize(sl->done) != hipSuccess) rc = efail(e, CQS_HIP_ERR_DEVICE, "collect: device failure in the recomputed batch");
        if (rc != CQS_HIP_OK) return rc;
    }
    const uint32_t H = e->g.hidden, B = sl->shape.B;
    if (out) {                         // out == NULL: abandon the ticket (wait, release the slot, drop the rows)
        memcpy(out, sl->direct ? c.q_out_pin : sl->out, (size_t)B * H * sizeof(float));
        const int32_t* seq_len = cqs::carve<const int32_t>(kKind, sl->meta, sl->shape).seq_len;
        for (uint32_t b = 0; b < B; ++b)   // empty rows: exact zeros, like the reference's zero-mask pooling
            if (seq_len[b] == 0) memset(out + (size_t)b * H, 0, (size_t)H * sizeof(float));
    }
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, sl->ev0, sl->ev1) == hipSuccess) e->last_ms = ms;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

// `session.run` (src/embedder/core.rs:1097): submit + collect.
int32_t cqs_hip_embed(cqs_hip_embedder* e, const int64_t* ids, const int64_t* mask, uint32_t B, uint32_t L, float* out) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_embed");
    if (!e) return CQS_HIP_ERR_INVALID;
    if (B == 0) return CQS_HIP_OK;
    if (!out) { std::lock_guard<std::mutex> lk(e->mu); return efail(e, CQS_HIP_ERR_INVALID, "embed: null buffer / empty sequence"); }
    uint64_t t = 0;
    const int32_t rc = cqs_hip_embed_submit(e, ids, mask, B, L, &t);
    if (rc != CQS_HIP_OK) return rc;
    return cqs_hip_embed_collect(e, t, out);
} CQS_ABI_CATCH(e)

// `Embedder::warm()` (src/embedder/core.rs:933-957: pay first-call cost before the first real query).  The search-time
// chain keeps one captured hipGraph per (query length, execution context, variant); without this call each is built
// the first time its length is seen (an eager chain + capture + instantiate + first replay on that query's clock).
// Runs every length 1..max_tokens once eagerly (sets the kernels' launch attributes), then captures, instantiates and
// replays each graph once, on both contexts, with token id 0.  Needs a free submission slot; nothing may be in flight.
int32_t cqs_hip_embedder_warm(cqs_hip_embedder* e, uint32_t max_tokens) CQS_ABI_TRY {
    if (!e) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (!e->finalized) return efail(e, CQS_HIP_ERR_INVALID, "warm: weights not finalized");
    if (!e->query_path || max_tokens == 0) return CQS_HIP_OK;
    if (e->pool.in_flight() != 0) return efail(e, CQS_HIP_ERR_INVALID, "warm: tickets are in flight (collect them first)");
    Slot& sl = e->slot[e->pool.take()];
    E_TRY(e, hipSetDevice(e->device));
    const uint32_t Tmax = std::min(max_tokens, std::min(e->query_max_tokens, e->g.max_seq));
    int32_t rc = slot_reserve(e, sl, {1, Tmax, 1, 0});
    if (rc != CQS_HIP_OK) return rc;
    memset(sl.meta, 0, sl.meta_cap);                            // token id 0 at every position, wherever a shape puts `tok`
    const int n_ctx = e->single_ctx ? 1 : cqs_hip_embedder::kCtx;
    for (uint32_t T = 1; T <= Tmax; ++T) {
        sl.shape = {1, T, 1, 0};
        for (int ci = 0; ci < n_ctx; ++ci) {
            Ctx& c = e->ctx[ci];
            for (int var = 1; var >= 0; --var) {
                if (var == 1 && !e->query_direct) continue;
                for (int tries = 0; tries < 3; ++tries) {
                    if ((rc = run_query(e, c, sl, var == 1)) != CQS_HIP_OK) return rc;
                    if (c.q_exec[var][T - 1] || c.q_capture_failed[var][T - 1] || !e->query_graph) break;
                }
            }
            E_TRY(e, hipStreamSynchronize(c.stream));
        }
    }
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

// Search-time chain counters since the engine was made: graphs captured, captures that failed (those lengths run
// eagerly; the cause is in last_error), graph replays, eager chain runs.  Any pointer may be NULL.
void cqs_hip_embedder_query_graph_stats(const cqs_hip_embedder* e, uint64_t* captured, uint64_t* failed, uint64_t* replays,
                                        uint64_t* eager) CQS_ABI_TRY {
    uint64_t v[4] = {0, 0, 0, 0};
    if (e) {
        std::lock_guard<std::mutex> lk(e->mu);
        v[0] = e->q_captured; v[1] = e->q_capture_failures; v[2] = e->q_replays; v[3] = e->q_eager;
    }
    if (captured) *captured = v[0];
    if (failed) *failed = v[1];
    if (replays) *replays = v[2];
    if (eager) *eager = v[3];
} CQS_ABI_CATCH_VOID

// Diagnostic twin (synchronous): final-norm hidden states [B, L, hidden], zeros at padded positions.
int32_t cqs_hip_embed_hidden(cqs_hip_embedder* e, const int64_t* ids, const int64_t* mask, uint32_t B, uint32_t L, float* out) CQS_ABI_TRY {
    if (!e) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (!e->finalized) return efail(e, CQS_HIP_ERR_INVALID, "embed: weights not finalized");
    if (B == 0) return CQS_HIP_OK;
    if (!ids || !mask || !out || L == 0) return efail(e, CQS_HIP_ERR_INVALID, "embed: null buffer / empty sequence");
    const int si = free_slot(e);
    if (si == e->pool.kNone) return CQS_HIP_ERR_INVALID;
    Slot* sl = &e->slot[si];
    E_TRY(e, hipSetDevice(e->device));
    int32_t rc = pack_padded(e, *sl, ids, mask, B, L);
    if (rc != CQS_HIP_OK) return rc;
    const uint32_t H = e->g.hidden;
    memset(out, 0, (size_t)B * L * H * sizeof(float));
    if (sl->shape.M == 0) return CQS_HIP_OK;
    Ctx& c = e->ctx[0];
    rc = run_layers(e, c, *sl);
    if (rc != CQS_HIP_OK) return rc;
    hipStream_t st = c.stream;
    E_TRY(e, hipEventRecord(sl->ev1, st));
    std::vector<float> packed((size_t)sl->shape.M * H);
    E_TRY(e, hipMemcpyAsync(packed.data(), c.hidden, packed.size() * 4, hipMemcpyDeviceToHost, st));
    E_TRY(e, hipStreamSynchronize(st));
    const auto tb = cqs::carve<const int32_t>(kKind, sl->meta, sl->shape);
    for (uint32_t b = 0; b < B; ++b)
        memcpy(out + (size_t)b * L * H, packed.data() + (size_t)tb.seq_start[b] * H, (size_t)tb.seq_len[b] * H * 4);
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, sl->ev0, sl->ev1) == hipSuccess) e->last_ms = ms;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

}  // extern "C"
