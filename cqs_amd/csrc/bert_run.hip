// bert_run.hip — the BERT-family forward behind the C ABI (include/cqs_hip.h, "BERT-family auxiliary models"): the device side
// of cqs's SPLADE sparse encoder (`SpladeEncoder::encode_batch`, src/splade/mod.rs:774-1075: ORT runs a BERT masked-LM, Rust
// pools its logits), of its cross-encoder reranker (`compute_scores_opt`, src/reranker.rs:343-533: ORT runs
// BertForSequenceClassification, Rust applies a sigmoid) and of the BERT-family embedder presets.  SURVEY.md §8(f)4.  Operator
// semantics: oracle/bert_ref.py.  A context's scratch, the encoder chain, the heads, and the submit / collect tickets
// (ticket_pool.h).  The handle: bert_internal.h; the weights: bert_engine.hip.
#include "bert_internal.h"

#include <algorithm>
#include <cstdlib>

#include "roctx.h"

using namespace cqs_bert;

void cqs_bert::free_scratch(BCtx& c) {
    void** all[] = {(void**)&c.x, (void**)&c.x2, (void**)&c.y, (void**)&c.qkv, (void**)&c.att, (void**)&c.h,
                    (void**)&c.pooled, (void**)&c.dense, (void**)&c.cls, (void**)&c.d_meta};
    for (void** p : all) { (void)hipFree(*p); *p = nullptr; }
    (void)hipFree(c.sp_ids); (void)hipFree(c.sp_w); (void)hipFree(c.sp_cnt);
    c.sp_ids = c.sp_cnt = nullptr; c.sp_w = nullptr; c.sp_rows = c.sp_cap = 0;
    c.tb = {};
    c.tok_cap = c.seq_cap = c.blk_cap = 0;
}

namespace {

enum { KIND_SPARSE = 1, KIND_EMBED = 2 };    // what a ticket collects to: SPLADE vectors / pooled embeddings

int32_t ensure_scratch(cqs_hip_bert* e, BCtx& c, uint32_t M, uint32_t B, uint32_t nblk) {
    if (M <= c.tok_cap && B <= c.seq_cap && nblk <= c.blk_cap) return CQS_HIP_OK;
    E_TRY(e, hipStreamSynchronize(c.stream));
    const uint32_t Mc = std::max(M, c.tok_cap), Bc = std::max(B, c.seq_cap), bc = std::max(nblk, c.blk_cap);
    free_scratch(c);
    const cqs_hip_bert_config& cf = e->cfg;
    const size_t H = cf.hidden;
    E_TRY(e, hipMalloc((void**)&c.x, (size_t)Mc * H * 2));
    E_TRY(e, hipMalloc((void**)&c.x2, (size_t)std::min<uint32_t>(Mc, 64u) * H * 2));
    E_TRY(e, hipMalloc((void**)&c.y, (size_t)Mc * H * 2));
    E_TRY(e, hipMalloc((void**)&c.qkv, (size_t)Mc * 3 * H * 2));
    E_TRY(e, hipMalloc((void**)&c.att, (size_t)Mc * H * 2));
    E_TRY(e, hipMalloc((void**)&c.h, (size_t)Mc * cf.intermediate * 2));
    if (cf.head == CQS_HIP_BERT_HEAD_MLM) {
        E_TRY(e, hipMalloc((void**)&c.dense, (size_t)Bc * cf.vocab_size * 4));
    } else if (cf.head == CQS_HIP_BERT_HEAD_NONE) {
        E_TRY(e, hipMalloc((void**)&c.dense, (size_t)Bc * H * 4));            // pooled embeddings
    } else {
        E_TRY(e, hipMalloc((void**)&c.pooled, (size_t)Bc * H * 2));
        E_TRY(e, hipMalloc((void**)&c.cls, (size_t)Bc * 16 * 4));
    }
    E_TRY(e, hipMalloc((void**)&c.d_meta, cqs::table_words(cqs::BATCH_BERT, {Bc, Mc, bc, 0}) * sizeof(int32_t)));
    c.tok_cap = Mc; c.seq_cap = Bc; c.blk_cap = bc;
    return CQS_HIP_OK;
}

// The device side of the threshold filter: room for `batch` rows of `cap` entries.
int32_t ensure_sparse(cqs_hip_bert* e, BCtx& c, uint32_t batch, uint32_t cap) {
    if ((size_t)batch <= c.sp_rows && (size_t)cap <= c.sp_cap) return CQS_HIP_OK;
    E_TRY(e, hipStreamSynchronize(c.stream));
    (void)hipFree(c.sp_ids); (void)hipFree(c.sp_w); (void)hipFree(c.sp_cnt);
    c.sp_ids = c.sp_cnt = nullptr; c.sp_w = nullptr;
    const size_t rows = std::max<size_t>(batch, c.sp_rows), cp = std::max<size_t>(cap, c.sp_cap);
    c.sp_rows = c.sp_cap = 0;
    E_TRY(e, hipMalloc((void**)&c.sp_ids, rows * cp * 4));
    E_TRY(e, hipMalloc((void**)&c.sp_w, rows * cp * 4));
    E_TRY(e, hipMalloc((void**)&c.sp_cnt, rows * 4));
    c.sp_rows = rows; c.sp_cap = cp;
    return CQS_HIP_OK;
}

// Validate + pack a ragged batch into the slot's pinned tables, upload them, run the encoder on context `c`; leaves the
// final hidden states in c.x and the batch's device tables in c.tb.
int32_t run_encoder(cqs_hip_bert* e, BCtx& c, BSlot& sl, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens, uint32_t B,
                    uint32_t* M_out) {
    const cqs_hip_bert_config& cf = e->cfg;
    constexpr cqs::BatchKind kKind = cqs::BATCH_BERT;
    auto refuse = [&](cqs::BatchCode code) {      // batch_tables.h's refusals as this engine's errors
        const char* what = code == cqs::BATCH_TOO_LONG          ? "bert: sequence longer than max_position_embeddings"
                           : code == cqs::BATCH_TOO_MANY_TOKENS ? "bert: batch holds too many tokens"
                           : code == cqs::BATCH_BAD_TYPE        ? "bert: token type id out of range"
                                                                : "bert: token id out of range";
        return code == cqs::BATCH_OK ? CQS_HIP_OK : efail(e, CQS_HIP_ERR_INVALID, what);
    };
    cqs::BatchShape s;
    int32_t rc = refuse(cqs::batch_shape(kKind, lens, B, cf.max_pos, &s));
    if (rc != CQS_HIP_OK) return rc;
    const uint32_t M = s.M, nblk = s.nblk, max_len = B ? *std::max_element(lens, lens + B) : 0u;
    *M_out = M;
    sl.B = B;
    if (M == 0) return CQS_HIP_OK;
    const size_t words = cqs::table_words(kKind, s);
    E_TRY(e, cqs::grow_pinned(&sl.meta, &sl.meta_cap, words * sizeof(int32_t)));
    rc = refuse(cqs::fill_tables(kKind, cqs::carve(kKind, sl.meta, s), s, lens,
                                 [&](uint32_t, uint32_t, uint32_t row) { return (int64_t)tokens[row]; },
                                 [&](uint32_t, uint32_t, uint32_t row) { return (int64_t)(type_ids ? type_ids[row] : 0); },
                                 (int64_t)cf.vocab_size, (int64_t)cf.type_vocab));
    if (rc == CQS_HIP_OK) rc = ensure_scratch(e, c, M, B, nblk);
    if (rc != CQS_HIP_OK) return rc;
    hipStream_t st = c.stream;
    E_TRY(e, hipMemcpyAsync(c.d_meta, sl.meta, words * sizeof(int32_t), hipMemcpyHostToDevice, st));
    c.tb = cqs::carve<const int32_t>(kKind, c.d_meta, s);
    const uint32_t H = cf.hidden, I = cf.intermediate;
    E_TRY(e, cqs::launch_bert_embed_ln(c.tb.tok, c.tb.pos, c.tb.tt, e->word, e->posw, e->typew, e->emb_g, e->emb_b, cf.ln_eps, c.x, M, H, st));
    // Up to 64 tokens (a search-time query): 5 launches per layer instead of 7 - each residual add + LayerNorm runs in the
    // prologue of the projection that consumes it (launch_gemm_small_rows_addln: every workgroup normalises the rows it
    // multiplies; the stream alternates between two buffers because everybody reads the old one)
    {
        const char* sr = getenv("CQS_HIP_GEMM_SMALL_ROWS");       // (the switch of the small-rows kernels covers this chain too)
        const bool fused = M <= 64u && !(sr && sr[0] == '0') && (H == 768u || H == 1024u || H == 256u) && H % 16u == 0 && I % 16u == 0;
        if (fused) {
            bf16_t* cur = c.x;
            bf16_t* oth = c.x2;
            for (uint32_t l = 0; l < cf.layers; ++l) {
                const BertLayer& w = e->L[l];
                if (l == 0) {
                    E_TRY(e, cqs::launch_gemm_bias(cur, w.wqkv, w.bqkv, c.qkv, M, 3u * H, H, 3u * H, cqs::GEMM_OUT_BF16, st));
                } else {
                    const BertLayer& pv = e->L[l - 1];
                    E_TRY(e, cqs::launch_gemm_small_rows_addln(cur, c.y, pv.ln2_g, pv.ln2_b, cf.ln_eps, oth, w.wqkv, w.bqkv, c.qkv, M, 3u * H, H,
                                                               3u * H, cqs::GEMM_OUT_BF16, st));
                    std::swap(cur, oth);
                }
                E_TRY(e, cqs::launch_bert_attention(c.qkv, c.att, c.tb.blk, nblk, c.tb.seq_start, c.tb.seq_len, B, max_len, cf.heads, H / cf.heads, st));
                E_TRY(e, cqs::launch_gemm_bias(c.att, w.wo, w.bo, c.y, M, H, H, H, cqs::GEMM_OUT_BF16, st));
                E_TRY(e, cqs::launch_gemm_small_rows_addln(cur, c.y, w.ln1_g, w.ln1_b, cf.ln_eps, oth, w.w1, w.b1, c.h, M, I, H, I,
                                                           cqs::GEMM_OUT_BF16_GELU, st));
                std::swap(cur, oth);
                E_TRY(e, cqs::launch_gemm_bias(c.h, w.w2, w.b2, c.y, M, H, I, H, cqs::GEMM_OUT_BF16, st));
            }
            const BertLayer& lw = e->L[cf.layers - 1u];
            E_TRY(e, cqs::launch_bert_add_ln(cur, c.y, lw.ln2_g, lw.ln2_b, cf.ln_eps, c.x, M, H, st));     // the final hidden states, in c.x
            return CQS_HIP_OK;
        }
    }
    for (uint32_t l = 0; l < cf.layers; ++l) {
        const BertLayer& w = e->L[l];
        E_TRY(e, cqs::launch_gemm_bias(c.x, w.wqkv, w.bqkv, c.qkv, M, 3u * H, H, 3u * H, cqs::GEMM_OUT_BF16, st));
        E_TRY(e, cqs::launch_bert_attention(c.qkv, c.att, c.tb.blk, nblk, c.tb.seq_start, c.tb.seq_len, B, max_len, cf.heads, H / cf.heads, st));
        E_TRY(e, cqs::launch_gemm_bias(c.att, w.wo, w.bo, c.y, M, H, H, H, cqs::GEMM_OUT_BF16, st));
        E_TRY(e, cqs::launch_bert_add_ln(c.x, c.y, w.ln1_g, w.ln1_b, cf.ln_eps, c.x, M, H, st));
        E_TRY(e, cqs::launch_gemm_bias(c.x, w.w1, w.b1, c.h, M, I, H, I, cqs::GEMM_OUT_BF16_GELU, st));
        E_TRY(e, cqs::launch_gemm_bias(c.h, w.w2, w.b2, c.y, M, H, I, H, cqs::GEMM_OUT_BF16, st));
        E_TRY(e, cqs::launch_bert_add_ln(c.x, c.y, w.ln2_g, w.ln2_b, cf.ln_eps, c.x, M, H, st));
    }
    return CQS_HIP_OK;
}

// Encoder + masked-LM head + pooling + activation: leaves the [batch, vocab] activations in c.dense (device).
// *M_out == 0: every sequence empty (nothing was launched; the activations are all ln(1 + 0) = 0).
int32_t splade_forward(cqs_hip_bert* e, BCtx& c, BSlot& sl, const int32_t* tokens, const uint32_t* lens, uint32_t batch, uint32_t* M_out) {
    uint64_t tot = 0;
    for (uint32_t b = 0; b < batch; ++b) tot += lens[b];
    if (tot && !tokens) return efail(e, CQS_HIP_ERR_INVALID, "splade: null tokens");
    int32_t rc = run_encoder(e, c, sl, tokens, nullptr, lens, batch, M_out);
    if (rc != CQS_HIP_OK) return rc;
    const uint32_t M = *M_out;
    if (M == 0) return CQS_HIP_OK;
    const cqs_hip_bert_config& cf = e->cfg;
    const size_t V = cf.vocab_size;
    hipStream_t st = c.stream;
    const uint32_t H = cf.hidden;
    // BertLMPredictionHead: LayerNorm(gelu(x Wt^T + bt)) E^T + b, decoder tied to the (zero-padded) word embeddings.
    // The [tokens, vocab] logits are never stored: the decoder GEMM's epilogue keeps, per sequence and vocabulary
    // entry, the maximum of max(0, logit) (atomic max on the float bits), then one small pass takes ln(1 + .).
    E_TRY(e, cqs::launch_gemm_bias(c.x, e->wt, e->bt, c.y, M, H, H, H, cqs::GEMM_OUT_BF16_GELU, st));
    E_TRY(e, cqs::launch_bert_add_ln(c.y, nullptr, e->lnt_g, e->lnt_b, cf.ln_eps, c.y, M, H, st));
    E_TRY(e, hipMemsetAsync(c.dense, 0, (size_t)batch * V * 4, st));
    E_TRY(e, cqs::launch_gemm_rowmax(c.y, e->word, e->bdec, (uint32_t*)c.dense, M, e->vpad, H, (uint32_t)V, c.tb.row_seq, (uint32_t)V, st));
    E_TRY(e, cqs::launch_splade_activate(c.dense, (size_t)batch * V, st));
    return CQS_HIP_OK;
}

int32_t check_ready(cqs_hip_bert* e, uint32_t head) {
    if (e->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (!e->finalized) return efail(e, CQS_HIP_ERR_INVALID, "bert: weights not finalized");
    if (head != 0xFFFFFFFFu && e->cfg.head != head) return efail(e, CQS_HIP_ERR_INVALID, "bert: this engine was built with the other head");
    return CQS_HIP_OK;
}

// Set (per thread) by the blocking forms around their submit: the submission takes the reserved slot.
thread_local bool tl_blocking_call = false;
struct BlockingScope {
    BlockingScope() { tl_blocking_call = true; }
    ~BlockingScope() { tl_blocking_call = false; }
};

// What every call that runs the encoder does once its arguments are checked: the device, a submission slot with its event,
// and the context the next ticket runs on (consecutive tickets alternate).  reserved: the blocking calls' own slot (another
// thread's blocking call may hold it: `lk`, the handle's mutex, is released while this one waits).
int32_t begin_run(cqs_hip_bert* e, std::unique_lock<std::mutex>& lk, bool reserved, int* si, BCtx** c) {
    E_TRY(e, hipSetDevice(e->device));
    *si = reserved ? e->pool.take_reserved(lk) : e->pool.take();
    if (*si == e->pool.kNone) return efail(e, CQS_HIP_ERR_INVALID, "bert: every submission slot is in flight (collect a ticket first)");
    *c = &e->ctx[e->pool.choose_context(*si).ctx];
    BSlot& sl = e->slot[*si];
    if (!sl.done) E_TRY(e, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    return CQS_HIP_OK;
}

// Wait for a ticket (outside the lock: other threads may submit meanwhile), hand its results out through copy(slot) and
// release the slot, whatever path leaves.  what: the entry point's prefix in the error strings.
template <class Copy>
int32_t collect_ticket(cqs_hip_bert* e, uint64_t ticket, int kind, const std::string& what, Copy copy) {
    int si = 0;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        const cqs::CollectCode cc = e->pool.begin_collect(ticket, kind, &si);
        if (cc == cqs::COLLECT_UNKNOWN) return efail(e, CQS_HIP_ERR_INVALID, what + " collect: unknown ticket");
        if (cc == cqs::COLLECT_BUSY) return efail(e, CQS_HIP_ERR_INVALID, what + " collect: this ticket is already being collected");
    }
    (void)hipSetDevice(e->device);
    const hipError_t he = hipEventSynchronize(e->slot[si].done);
    std::lock_guard<std::mutex> lk(e->mu);
    decltype(e->pool)::Collecting release{e->pool, si};
    if (he != hipSuccess) return efail(e, CQS_HIP_ERR_DEVICE, what + " collect: device failure", he);
    return copy(e->slot[si]);
}

}  // namespace

extern "C" {

// `SpladeEncoder::encode_batch` below the tokenizer: sequences back to back (i32 ids) + their lengths; out_dense
// [batch, vocab] f32 = ln(1 + max(0, max over the sequence's tokens of the MLM logits)) - the model's pre-pooled
// `sparse_vector` output form (src/splade/mod.rs:960-978); the caller keeps entries > threshold.
int32_t cqs_hip_splade_encode(cqs_hip_bert* e, const int32_t* tokens, const uint32_t* lens, uint32_t batch, float* out_dense) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_splade_encode");
    if (!e) return CQS_HIP_ERR_INVALID;
    std::unique_lock<std::mutex> lk(e->mu);
    int32_t rc = check_ready(e, CQS_HIP_BERT_HEAD_MLM);
    if (rc != CQS_HIP_OK) return rc;
    if (batch == 0) return CQS_HIP_OK;
    if (!lens || !out_dense) return efail(e, CQS_HIP_ERR_INVALID, "splade: null buffer");
    int si; BCtx* c;
    if ((rc = begin_run(e, lk, true, &si, &c)) != CQS_HIP_OK) return rc;
    uint32_t M = 0;
    rc = splade_forward(e, *c, e->slot[si], tokens, lens, batch, &M);
    if (rc != CQS_HIP_OK) return rc;
    const size_t V = e->cfg.vocab_size;
    if (M == 0) { memset(out_dense, 0, (size_t)batch * V * 4); return CQS_HIP_OK; }   // all empty: ln(1 + 0) = 0 everywhere
    E_TRY(e, hipMemcpyAsync(out_dense, c->dense, (size_t)batch * V * 4, hipMemcpyDeviceToHost, c->stream));
    E_TRY(e, hipStreamSynchronize(c->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

// The same with the threshold filter of src/splade/mod.rs:1049-1062 on the device, as a TICKET: submit packs the batch
// into a free slot's pinned tables, enqueues H2D + encoder + head + filter + D2H on one of the two execution contexts
// and returns without waiting; collect waits for that ticket and hands out sequence b's entries > threshold as
// (id, weight), ascending id, at out_ids / out_weights [b * cap ..], out_counts[b] = how many passed.  A count above
// `cap` means the row was cut off after its first `cap` entries: the caller re-encodes that sequence through
// cqs_hip_splade_encode (trained models keep 100-300 entries, src/splade/mod.rs:44).  Up to 3 tickets in flight; a
// ticket is released only by collecting it (out_ids = NULL: abandon).
int32_t cqs_hip_splade_submit_sparse(cqs_hip_bert* e, const int32_t* tokens, const uint32_t* lens, uint32_t batch, float threshold,
                                     uint32_t cap, uint64_t* ticket) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_splade_submit_sparse");
    if (!e) return CQS_HIP_ERR_INVALID;
    std::unique_lock<std::mutex> lk(e->mu);
    int32_t rc = check_ready(e, CQS_HIP_BERT_HEAD_MLM);
    if (rc != CQS_HIP_OK) return rc;
    if (!ticket) return efail(e, CQS_HIP_ERR_INVALID, "splade: null ticket");
    *ticket = 0;
    if (batch == 0 || !lens || cap == 0) return efail(e, CQS_HIP_ERR_INVALID, "splade: empty batch / null buffer / zero cap");
    int si; BCtx* c;
    if ((rc = begin_run(e, lk, tl_blocking_call, &si, &c)) != CQS_HIP_OK) return rc;
    BSlot& sl = e->slot[si];
    uint32_t M = 0;
    rc = splade_forward(e, *c, sl, tokens, lens, batch, &M);
    if (rc != CQS_HIP_OK) return rc;
    const size_t n = (size_t)batch * cap;
    E_TRY(e, cqs::grow_pinned(&sl.out, &sl.out_cap, n * 8 + (size_t)batch * 4));
    hipStream_t st = c->stream;
    if (M == 0) {
        memset(sl.out + n * 8, 0, (size_t)batch * 4);                                // activations all 0: nothing passes `>`
    } else {
        if ((rc = ensure_sparse(e, *c, batch, cap)) != CQS_HIP_OK) return rc;
        E_TRY(e, cqs::launch_splade_sparsify(c->dense, batch, e->cfg.vocab_size, threshold, cap, c->sp_ids, c->sp_w, c->sp_cnt, st));
        E_TRY(e, hipMemcpyAsync(sl.out, c->sp_ids, n * 4, hipMemcpyDeviceToHost, st));
        E_TRY(e, hipMemcpyAsync(sl.out + n * 4, c->sp_w, n * 4, hipMemcpyDeviceToHost, st));
        E_TRY(e, hipMemcpyAsync(sl.out + n * 8, c->sp_cnt, (size_t)batch * 4, hipMemcpyDeviceToHost, st));
    }
    E_TRY(e, hipEventRecord(sl.done, st));
    sl.cap = cap;
    *ticket = e->pool.publish(si, KIND_SPARSE);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

int32_t cqs_hip_splade_collect_sparse(cqs_hip_bert* e, uint64_t ticket, uint32_t* out_ids, float* out_weights, uint32_t* out_counts) CQS_ABI_TRY {
    if (!e) return CQS_HIP_ERR_INVALID;
    return collect_ticket(e, ticket, KIND_SPARSE, "splade", [&](const BSlot& sl) -> int32_t {
        if (!out_ids) return CQS_HIP_OK;                                    // NULL: abandon the ticket
        if (!out_weights || !out_counts) return efail(e, CQS_HIP_ERR_INVALID, "splade collect: null buffer");
        const size_t n = (size_t)sl.B * sl.cap;
        memcpy(out_ids, sl.out, n * 4);
        memcpy(out_weights, sl.out + n * 4, n * 4);
        memcpy(out_counts, sl.out + n * 8, (size_t)sl.B * 4);
        return CQS_HIP_OK;
    });
} CQS_ABI_CATCH(e)

// blocking form: submit + collect
int32_t cqs_hip_splade_encode_sparse(cqs_hip_bert* e, const int32_t* tokens, const uint32_t* lens, uint32_t batch,
                                     float threshold, uint32_t cap, uint32_t* out_ids, float* out_weights, uint32_t* out_counts) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_splade_encode_sparse");
    if (!e) return CQS_HIP_ERR_INVALID;
    if (batch == 0) {
        std::lock_guard<std::mutex> lk(e->mu);
        return check_ready(e, CQS_HIP_BERT_HEAD_MLM);
    }
    if (!out_ids || !out_weights || !out_counts) { std::lock_guard<std::mutex> lk(e->mu); return efail(e, CQS_HIP_ERR_INVALID, "splade: null buffer / zero cap"); }
    uint64_t t = 0;
    BlockingScope reserved_slot;
    const int32_t rc = cqs_hip_splade_submit_sparse(e, tokens, lens, batch, threshold, cap, &t);
    if (rc != CQS_HIP_OK) return rc;
    return cqs_hip_splade_collect_sparse(e, t, out_ids, out_weights, out_counts);
} CQS_ABI_CATCH(e)

// `compute_scores_opt` below the tokenizer (src/reranker.rs:343-533): (query, passage) pairs already encoded as ids +
// token type ids; out_logits [batch, num_labels] f32 (the caller applies sigmoid to column 0).
int32_t cqs_hip_rerank_logits(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens,
                              uint32_t batch, float* out_logits) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_rerank_logits");
    if (!e) return CQS_HIP_ERR_INVALID;
    std::unique_lock<std::mutex> lk(e->mu);
    int32_t rc = check_ready(e, CQS_HIP_BERT_HEAD_CLASSIFIER);
    if (rc != CQS_HIP_OK) return rc;
    if (batch == 0) return CQS_HIP_OK;
    if (!lens || !out_logits || !tokens) return efail(e, CQS_HIP_ERR_INVALID, "rerank: null buffer");
    for (uint32_t b = 0; b < batch; ++b)
        if (lens[b] == 0) return efail(e, CQS_HIP_ERR_INVALID, "rerank: empty sequence (no [CLS] row to pool)");
    int si; BCtx* c;
    if ((rc = begin_run(e, lk, true, &si, &c)) != CQS_HIP_OK) return rc;
    uint32_t M = 0;
    rc = run_encoder(e, *c, e->slot[si], tokens, type_ids, lens, batch, &M);
    if (rc != CQS_HIP_OK) return rc;
    const cqs_hip_bert_config& cf = e->cfg;
    hipStream_t st = c->stream;
    const uint32_t H = cf.hidden;
    // BertPooler on every sequence's first token (row seq_start[b] of the packed hidden states: the skinny GEMM reads its
    // rows through that table), dense + tanh, then the classifier (labels padded to 16).
    E_TRY(e, cqs::launch_gemm_rows(c->x, H, e->wp, e->bp, 1, c->att, batch, H, H, H, cqs::GEMM_OUT_BF16, st, c->tb.seq_start));
    E_TRY(e, cqs::launch_gemm_rows(c->att, H, e->wc, e->bc, 0, c->cls, batch, 16, H, 16, cqs::GEMM_OUT_F32, st));
    std::vector<float> tmp((size_t)batch * 16);
    E_TRY(e, hipMemcpyAsync(tmp.data(), c->cls, tmp.size() * 4, hipMemcpyDeviceToHost, st));
    E_TRY(e, hipStreamSynchronize(st));
    for (uint32_t b = 0; b < batch; ++b)
        for (uint32_t j = 0; j < cf.num_labels; ++j) out_logits[(size_t)b * cf.num_labels + j] = tmp[(size_t)b * 16 + j];
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

// The BERT-family EMBEDDER presets (e5-base, v9-200k, bge-large, bge-large-ft: src/embedder/models.rs:346-405) below the
// tokenizer: `session.run` -> last_hidden_state -> `mean_pool` / `cls_pool` (src/embedder/pooling.rs:87-128), all on the
// device.  out [batch, hidden] f32, NOT normalised (the caller's `normalize_l2`, core.rs:1196-1203).  Ticket form (what
// the index pipeline's embed stage uses, src/cli/pipeline/embedding.rs:226-421) + the blocking `session.run` form.
int32_t cqs_hip_bert_embed_submit(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens, uint32_t batch,
                                  uint32_t pooling, uint64_t* ticket) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_bert_embed_submit");
    if (!e) return CQS_HIP_ERR_INVALID;
    std::unique_lock<std::mutex> lk(e->mu);
    int32_t rc = check_ready(e, CQS_HIP_BERT_HEAD_NONE);
    if (rc != CQS_HIP_OK) return rc;
    if (!ticket) return efail(e, CQS_HIP_ERR_INVALID, "bert_embed: null ticket");
    *ticket = 0;
    if (batch == 0 || !lens || pooling > 1u) return efail(e, CQS_HIP_ERR_INVALID, "bert_embed: empty batch / null buffer / unknown pooling");
    {
        uint64_t tot = 0;
        for (uint32_t b = 0; b < batch; ++b) tot += lens[b];
        if (tot && !tokens) return efail(e, CQS_HIP_ERR_INVALID, "bert_embed: null tokens");
    }
    int si; BCtx* c;
    if ((rc = begin_run(e, lk, tl_blocking_call, &si, &c)) != CQS_HIP_OK) return rc;
    BSlot& sl = e->slot[si];
    uint32_t M = 0;
    rc = run_encoder(e, *c, sl, tokens, type_ids, lens, batch, &M);
    if (rc != CQS_HIP_OK) return rc;
    const uint32_t H = e->cfg.hidden;
    E_TRY(e, cqs::grow_pinned(&sl.out, &sl.out_cap, (size_t)batch * H * 4));
    hipStream_t st = c->stream;
    if (M == 0) {
        memset(sl.out, 0, (size_t)batch * H * 4);                                    // every sequence empty: zero vectors
    } else {
        E_TRY(e, cqs::launch_bert_pool(c->x, c->tb.seq_start, c->tb.seq_len, c->dense, batch, H, (int)pooling, st));
        E_TRY(e, hipMemcpyAsync(sl.out, c->dense, (size_t)batch * H * 4, hipMemcpyDeviceToHost, st));
    }
    E_TRY(e, hipEventRecord(sl.done, st));
    *ticket = e->pool.publish(si, KIND_EMBED);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

int32_t cqs_hip_bert_embed_collect(cqs_hip_bert* e, uint64_t ticket, float* out) CQS_ABI_TRY {
    if (!e) return CQS_HIP_ERR_INVALID;
    return collect_ticket(e, ticket, KIND_EMBED, "bert_embed", [&](const BSlot& sl) -> int32_t {
        if (out) memcpy(out, sl.out, (size_t)sl.B * e->cfg.hidden * 4);              // NULL: abandon the ticket
        return CQS_HIP_OK;
    });
} CQS_ABI_CATCH(e)

int32_t cqs_hip_bert_embed(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens, uint32_t batch,
                           uint32_t pooling, float* out) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_bert_embed");
    if (!e) return CQS_HIP_ERR_INVALID;
    if (batch == 0) {
        std::lock_guard<std::mutex> lk(e->mu);
        return check_ready(e, CQS_HIP_BERT_HEAD_NONE);
    }
    if (!out) { std::lock_guard<std::mutex> lk(e->mu); return efail(e, CQS_HIP_ERR_INVALID, "bert_embed: null buffer / unknown pooling"); }
    uint64_t t = 0;
    BlockingScope reserved_slot;
    const int32_t rc = cqs_hip_bert_embed_submit(e, tokens, type_ids, lens, batch, pooling, &t);
    if (rc != CQS_HIP_OK) return rc;
    return cqs_hip_bert_embed_collect(e, t, out);
} CQS_ABI_CATCH(e)

// Diagnostic: final hidden states of the packed tokens, f32 [sum(lens), hidden].
int32_t cqs_hip_bert_hidden(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens,
                            uint32_t batch, float* out_hidden) CQS_ABI_TRY {
    if (!e) return CQS_HIP_ERR_INVALID;
    std::unique_lock<std::mutex> lk(e->mu);
    int32_t rc = check_ready(e, 0xFFFFFFFFu);
    if (rc != CQS_HIP_OK) return rc;
    if (batch == 0) return CQS_HIP_OK;
    if (!lens || !out_hidden || !tokens) return efail(e, CQS_HIP_ERR_INVALID, "bert: null buffer");
    int si; BCtx* c;
    if ((rc = begin_run(e, lk, true, &si, &c)) != CQS_HIP_OK) return rc;
    uint32_t M = 0;
    rc = run_encoder(e, *c, e->slot[si], tokens, type_ids, lens, batch, &M);
    if (rc != CQS_HIP_OK || M == 0) return rc;
    std::vector<uint16_t> tmp((size_t)M * e->cfg.hidden);
    E_TRY(e, hipMemcpyAsync(tmp.data(), c->x, tmp.size() * 2, hipMemcpyDeviceToHost, c->stream));
    E_TRY(e, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < tmp.size(); ++i) {
        const uint32_t u = (uint32_t)tmp[i] << 16;
        memcpy(&out_hidden[i], &u, 4);
    }
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

}  // extern "C"
