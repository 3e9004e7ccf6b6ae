// bert_internal.h — the BERT-family engine's handle and the declarations its two sources share: bert_engine.hip (weights: create,
// set_tensor, finalize, load_dir, destroy) and bert_run.hip (scratch, the encoder chain, the heads, every encode / submit /
// collect entry point).  No CPU fallback: without a GPU `cqs_hip_bert_create` fails.
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
#include "bert_kernels.h"
#include "engine_common.h"
#include "ticket_pool.h"

namespace cqs_bert {

using cqs::bf16_t;

struct BertLayer {
    bf16_t *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
};

}  // namespace cqs_bert

struct cqs_hip_bert {
    using bf16_t = cqs::bf16_t;
    int device = 0;
    cqs_hip_bert_config cfg{};
    uint32_t vpad = 0;                       // vocab rounded up to a multiple of 192 (decoder N tile)
    std::map<std::string, std::vector<float>> pending;    // host copies until finalize
    bool finalized = false;

    bf16_t *word = nullptr, *posw = nullptr, *typew = nullptr;     // word: [vpad, H] (rows >= vocab are zero)
    float *emb_g = nullptr, *emb_b = nullptr;
    std::vector<cqs_bert::BertLayer> L;
    // masked-LM head
    bf16_t* wt = nullptr;
    float *bt = nullptr, *lnt_g = nullptr, *lnt_b = nullptr, *bdec = nullptr;   // bdec [vpad]
    // classifier head
    bf16_t *wp = nullptr, *wc = nullptr;     // wc [16-padded labels, H]
    float *bp = nullptr, *bc = nullptr;
    std::vector<void*> owned;                // every device allocation of the weights

    // Execution contexts (a HIP stream + the activation scratch of one batch each; weights shared): consecutive tickets
    // alternate, so batch i + 1's kernel chain fills the CUs batch i's leaves idle and its H2D / host packing overlap
    // batch i's compute - the submit / collect scheme of the EmbeddingGemma engine (embedder_run.hip), which the reference's
    // index pipeline needs from the SPLADE encoder just as well (src/splade/mod.rs:774-1075 is called per batch from it).
    struct Ctx {
        hipStream_t stream = nullptr;
        uint32_t tok_cap = 0, seq_cap = 0, blk_cap = 0;
        bf16_t *x = nullptr, *x2 = nullptr, *y = nullptr, *qkv = nullptr, *att = nullptr, *h = nullptr, *pooled = nullptr;   // x2: the other residual buffer of the fused small-batch chain
        float *dense = nullptr, *cls = nullptr;
        uint32_t *sp_ids = nullptr, *sp_cnt = nullptr;  // device-side threshold filter: [sp_rows * sp_cap] ids / weights, [sp_rows] counts
        float* sp_w = nullptr;
        size_t sp_rows = 0, sp_cap = 0;
        int32_t* d_meta = nullptr;                // the batch's integer tables (batch_tables.h, BERT kind), sized for the capacities,
        cqs::BatchTables<const int32_t> tb;       // and that block carved for the batch it holds (run_encoder)
    };
    static constexpr int kCtx = 2;
    Ctx ctx[kCtx];
    // Submission slots: pinned tables (packed on the host while earlier tickets run) + pinned results + a completion event.
    // Ticket, kind (bert_run.hip: KIND_SPARSE / KIND_EMBED), context and the collector of slot i: pool.slot[i] (ticket_pool.h).
    struct Slot {
        uint32_t B = 0, cap = 0;
        int32_t* meta = nullptr;     // pinned twin of d_meta
        size_t meta_cap = 0;         // bytes
        char* out = nullptr;         // pinned results: sparse: ids [B cap] u32 | weights [B cap] f32 | counts [B] u32; embed: [B, H] f32
        size_t out_cap = 0;          // bytes
        hipEvent_t done = nullptr;
    };
    // Three TICKET slots (the public contract: up to 3 tickets in flight) + one slot RESERVED for the blocking calls
    // (cqs_hip_splade_encode, _encode_sparse, cqs_hip_rerank_logits, cqs_hip_bert_embed, _hidden), so that a search-time
    // query or rerank never fails because an index run holds every ticket; a blocking call that finds the reserved slot
    // taken by another thread's blocking call waits for it.
    static constexpr int kSlots = 3;
    Slot slot[kSlots + 1];
    cqs::TicketPool<kSlots, 1> pool;

    std::mutex mu;
    std::atomic<bool> poisoned{false};
    std::string last_error;
};

namespace cqs_bert {

using BCtx = cqs_hip_bert::Ctx;
using BSlot = cqs_hip_bert::Slot;
using cqs::efail;

// bert_run.hip (cqs_hip_bert_destroy gives a context's scratch back through it)
void free_scratch(BCtx& c);

}  // namespace cqs_bert
