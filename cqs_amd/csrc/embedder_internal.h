// embedder_internal.h — the EmbeddingGemma engine's handle and the helpers its three sources share: embedder.hip (weights:
// create, set_tensor, finalize, load_dir, destroy), embedder_run.hip (scratch, packing, the two chains, tickets) and
// embedder_debug.hip (the cqs_hip_debug_* hooks).  Plays the role of the ORT `Session` inside the reference's `Embedder`
// (src/embedder/core.rs:34-226, `session.run` at :1097): one engine per device, inference serialised behind a mutex
// exactly like `Mutex<Option<Session>>` (core.rs:35-39), errors reported as status codes (-> `EmbedderError::InferenceFailed`,
// src/embedder/mod.rs:36-60).  Shared with the BERT-family engine (bert_internal.h): the ticket bookkeeping (ticket_pool.h)
// and the failure rule, allocation helpers and bf16 rounding (engine_common.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cqs_hip.h"
#include "abi_guard.h"
#include "batch_tables.h"
#include "embed_kernels.h"
#include "engine_common.h"
#include "ticket_pool.h"

namespace cqs_emb {

using cqs::bf16_t;

struct LayerW {
    bf16_t *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wd = nullptr;
    bf16_t *wo_p = nullptr, *wd_p = nullptr;      // wo / wd in the block order of the pair-split fused kernel (made at finalize)
    bf16_t* wgu_f = nullptr;                      // wgu rows interleaved per 4 (the 256-row kernel's in-register GeGLU pairing; made at finalize)
    bf16_t* wqkv_f = nullptr;                     // wqkv rows in tile order for the fused norm + RoPE epilogue (made at finalize)
    float *n_in = nullptr, *n_post_attn = nullptr, *n_pre_ffw = nullptr, *n_post_ffw = nullptr, *n_q = nullptr, *n_k = nullptr;
};

}  // namespace cqs_emb

struct cqs_hip_embedder {
    using bf16_t = cqs::bf16_t;
    int device = 0;
    uint32_t n_cu = 256;                  // compute units of `device` (cqs::exact_rounds); 256 when the attribute query fails
    cqs_hip_embed_config cfg{};
    cqs::EmbedGeom g{};
    float last_ms = -1.f;

    bf16_t* emb = nullptr;
    float* n_final = nullptr;
    bf16_t *dense1 = nullptr, *dense2 = nullptr;
    std::vector<cqs_emb::LayerW> L;
    std::vector<cqs::QueryFwdLayer> QL;   // the same pointers in the query path's layout (filled by finalize)
    bool query_path = false;              // geometry supported and not disabled by CQS_HIP_QUERY_PATH=0
    uint32_t query_max_tokens = 64;       // longest single sequence the search-time chain serves (cqs::query_forward_max_tokens)
    bool query_graph = true;              // CQS_HIP_QUERY_GRAPH=0: launch the query chain eagerly
    bool query_direct = true;             // CQS_HIP_QUERY_DIRECT=0: token ids / result always through copy calls
    bool single_ctx = false;              // CQS_HIP_EMBED_CONTEXTS=1: one execution context (A/B hook for the two-chain overlap)
    // o_proj / down fused with the residual add + both norms (gemm_rowfuse.hip).  Read ONCE, at finalize
    // (CQS_HIP_GEMM_FUSE_NORM / _MIN_ROWS); tests flip it through cqs_hip_debug_embedder_set_fuse_norm.
    uint32_t fuse_fallbacks = 0;          // times a pair-exchange timeout sent this engine back to the two-launch chain (0 or 1)
    int fuse_norm = 2;                    // 0 = two launches, 1 = the 64-row kernel of round 3, 2 = the pair-split kernel (128 rows x 384 columns)
    uint32_t fuse_min_rows = 4096;        // token count from which the fused kernel runs (pair-split kernel, ragged 10k-token batches, tickets in
                                          // flight: 9.6 k chunks/s at 1024-4096, 9.4 k at 2048 / 8192, 8.3 k at 12288; round 3's 64-row kernel needed 12288)
    bool geglu4 = true;                   // CQS_HIP_GEGLU4=0: the 256-row kernel's GeGLU pairs gate / up through an f32 LDS stage (round 2) instead of in registers
    bool fuse_qkv = true;                 // CQS_HIP_QKV_FUSE=0: QKV GEMM + kv_prep + the attention kernel's own Q norm instead of the fused epilogue
    unsigned* fuse_err = nullptr;         // pinned host word (device-visible at fuse_err_dev): set by the pair kernel if an exchange timed out
    unsigned* fuse_err_dev = nullptr;
    float *rope_global = nullptr, *rope_local = nullptr;  // [max_seq][128][2]
    std::map<std::string, bool> seen;
    bool finalized = false;

    // Execution contexts: a HIP stream + the activation scratch of one batch.  Consecutive tickets alternate between
    // the two, so the kernels of batch i+1 fill the CUs that batch i's kernels leave idle at their heads and tails
    // (every kernel here is one round of one workgroup per CU: load burst, compute, store burst, all CUs in phase;
    // measured +3-5 % forward throughput with two chains in flight).  Weights are shared.
    struct Ctx {
        hipStream_t stream = nullptr;
        // scratch, sized for tok_cap packed tokens / seq_cap sequences
        uint32_t tok_cap = 0, seq_cap = 0, vt_ld = 0, blk_cap = 0;
        float *x = nullptr, *hidden = nullptr, *out = nullptr;
        bf16_t *y = nullptr, *xn = nullptr, *qkv = nullptr, *vt = nullptr, *attn = nullptr, *h = nullptr, *pooled = nullptr, *d1 = nullptr;
        // per-batch integer tables in ONE device block sized for the capacities (one H2D per batch from the slot's pinned
        // twin; batch_tables.h, Gemma kind), and that block carved for the batch it holds
        int32_t* d_meta = nullptr;
        cqs::BatchTables<const int32_t> tb;
        void* xch = nullptr;   // pair-split fused projection: the partners' row-sum granules (gemm_addnorm_pair_scratch_bytes(tok_cap))
        uint32_t xch_tag = 0;  // sequence number of the last launch that used xch (the granules' tag; never 0)
        // search-time path (query_forward.hip): fixed 64-row scratch, allocated once and never moved, so that the
        // captured graphs' kernel arguments stay valid; the token ids arrive in q_meta by one H2D per query
        int32_t* q_meta = nullptr;
        int32_t* q_pos = nullptr;          // [kQueryFwdMaxTokens] = 0, 1, 2, ...
        float *q_x0 = nullptr, *q_x1 = nullptr, *q_out = nullptr;
        bf16_t *q_qkv = nullptr, *q_attn = nullptr, *q_y = nullptr, *q_h = nullptr, *q_d1 = nullptr;
        // one captured chain per query length T = 1..64 (T is a launch parameter of every kernel: no load waits for a
        // length read from memory, no row past T is touched), captured the first time a length is seen
        // [variant][T - 1]; variant 1 = "direct": the token ids are read from, and the sentence vector is written to,
        // the context's own pinned host buffers (q_tok_pin / q_out_pin, device-visible) - no H2D / D2H copy node and no
        // copy call around the chain.  Used when the context has no other ticket in flight (the blocking `embed_query`
        // call); a second ticket queued on the same context would overwrite those buffers, so it takes variant 0.
        hipGraph_t q_graph[2][cqs::kQueryFwdMaxTokens] = {};
        hipGraphExec_t q_exec[2][cqs::kQueryFwdMaxTokens] = {};
        bool q_capture_failed[2][cqs::kQueryFwdMaxTokens] = {};   // capture / instantiate refused for THIS (variant, length): it stays eager
        int32_t* q_tok_pin = nullptr;      // pinned host, 64 ids
        float* q_out_pin = nullptr;        // pinned host, [hidden]
        int32_t* q_tok_pin_dev = nullptr;  // their device addresses
        float* q_out_pin_dev = nullptr;
        unsigned long long* q_dbg = nullptr;   // CQS_HIP_QUERY_STAMPS=1: per-kernel, per-workgroup stamps of the last query
    };
    static constexpr int kCtx = 2;
    Ctx ctx[kCtx];
    // Search-time chain bookkeeping (cqs_hip_embedder_query_graph_stats).  A length's kernels differ by length class
    // (row-block variants), and their dynamic-LDS attributes are set on first launch - which must not happen inside a
    // stream capture: the first query of every length runs eagerly, the second is captured.
    bool q_len_ran[cqs::kQueryFwdMaxTokens] = {};   // this length's kernels have been launched once (attributes set)
    uint64_t q_captured = 0, q_capture_failures = 0, q_replays = 0, q_eager = 0;

    // Submission slots (pinned host staging + events): batch i+1 is packed and enqueued while batch i computes;
    // results come back through the slot's pinned `out` (cqs_hip_embed_submit / _collect).  Ticket, context and the
    // collector of slot i: pool.slot[i] (ticket_pool.h).
    struct Slot {
        int32_t* meta = nullptr;   // pinned twin of d_meta, carved at `shape`
        size_t meta_cap = 0;       // bytes
        float* out = nullptr;      // pinned [B, hidden]
        size_t out_cap = 0;        // bytes
        cqs::BatchShape shape;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;   // forward start / end (timing), ev_done after the D2H
        hipEvent_t done = nullptr;
        bool direct = false;       // the result is in the context's q_out_pin, not in `out`
        bool batch_chain = false;  // the ticket ran the batch path (whose fused projections exchange row sums across workgroups)
        bool rerun = false;        // a pair exchange timed out while this ticket was in flight: recompute it at its collect
    };
    static constexpr int kSlots = 3;
    Slot slot[kSlots];
    cqs::TicketPool<kSlots, 0> pool;

    mutable std::mutex mu;
    std::atomic<bool> poisoned{false};
    std::string last_error;
};

namespace cqs_emb {

using Ctx = cqs_hip_embedder::Ctx;
using Slot = cqs_hip_embedder::Slot;

using cqs::dmalloc;
using cqs::efail;
using cqs::f32_to_bf16_bits;

inline uint32_t nqkv(const cqs::EmbedGeom& g) { return (g.heads + 2u * g.kv_heads) * g.head_dim; }

// embedder_run.hip (cqs_hip_embedder_destroy gives a context's scratch back through them)
void free_scratch(Ctx& c);
void free_query_scratch(Ctx& c);

}  // namespace cqs_emb
