// bert_engine.hip — the BERT-family engine's weights behind the C ABI (include/cqs_hip.h, "BERT-family auxiliary models"):
// config_default, create, set_tensor, finalize, load_dir with its ONNX / safetensors feeders, destroy and the small accessors.
// The forward and the tickets: bert_run.hip; the handle: bert_internal.h.
#include "bert_internal.h"

#include <cstdio>
#include <memory>
#include <new>

#include <sys/stat.h>

#include "onnx_reader.h"
#include "safetensors_reader.h"

using namespace cqs_bert;

namespace {

const std::vector<float>* find(cqs_hip_bert* e, const std::string& name, size_t count) {
    auto it = e->pending.find(name);
    if (it == e->pending.end() || it->second.size() != count) return nullptr;
    return &it->second;
}

int32_t up_bf16(cqs_hip_bert* e, bf16_t** dst, const float* src, size_t count, size_t alloc_count = 0) {
    if (alloc_count < count) alloc_count = count;
    std::vector<uint16_t> tmp(alloc_count, 0);
    for (size_t i = 0; i < count; ++i) tmp[i] = cqs::f32_to_bf16_bits(src[i]);
    E_TRY(e, hipMalloc((void**)dst, alloc_count * 2));
    e->owned.push_back(*dst);
    E_TRY(e, hipMemcpy(*dst, tmp.data(), alloc_count * 2, hipMemcpyHostToDevice));
    return CQS_HIP_OK;
}
int32_t up_f32(cqs_hip_bert* e, float** dst, const float* src, size_t count, size_t alloc_count = 0) {
    if (alloc_count < count) alloc_count = count;
    std::vector<float> tmp(alloc_count, 0.f);
    memcpy(tmp.data(), src, count * 4);
    E_TRY(e, hipMalloc((void**)dst, alloc_count * 4));
    e->owned.push_back(*dst);
    E_TRY(e, hipMemcpy(*dst, tmp.data(), alloc_count * 4, hipMemcpyHostToDevice));
    return CQS_HIP_OK;
}

}  // namespace

extern "C" {

int32_t cqs_hip_bert_config_default(uint32_t head, cqs_hip_bert_config* c) CQS_ABI_TRY {
    if (!c) return CQS_HIP_ERR_INVALID;
    memset(c, 0, sizeof(*c));
    c->vocab_size = 30522; c->max_pos = 512; c->type_vocab = 2; c->ln_eps = 1e-12f; c->num_labels = 1; c->head = head;
    if (head == CQS_HIP_BERT_HEAD_MLM) {            // naver/splade-cocondenser-ensembledistil = bert-base-uncased geometry
        c->hidden = 768; c->layers = 12; c->heads = 12; c->intermediate = 3072;
    } else if (head == CQS_HIP_BERT_HEAD_CLASSIFIER) {   // cross-encoder/ms-marco-MiniLM-L-6-v2 (src/reranker.rs:7,35)
        c->hidden = 384; c->layers = 6; c->heads = 12; c->intermediate = 1536;
    } else if (head == CQS_HIP_BERT_HEAD_NONE) {         // intfloat/e5-base-v2 = BERT-base (src/embedder/models.rs:346-358)
        c->hidden = 768; c->layers = 12; c->heads = 12; c->intermediate = 3072;
    } else {
        return CQS_HIP_ERR_INVALID;
    }
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

int32_t cqs_hip_bert_create(const cqs_hip_bert_config* cfg, int32_t device, cqs_hip_bert** out) CQS_ABI_TRY {
    if (!cfg || !out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    const cqs_hip_bert_config& c = *cfg;
    auto tiles = [](uint32_t n) { return n && (n % 192u == 0 || n % 256u == 0 || n % 320u == 0); };   // a GEMM tile width divides it
    const bool ok_cfg = c.hidden && c.hidden % 128u == 0 && c.hidden <= 1024u && c.layers && c.heads &&
                        c.hidden % c.heads == 0 && (c.hidden / c.heads == 32u || c.hidden / c.heads == 64u) &&
                        tiles(c.hidden) && tiles(3u * c.hidden) && tiles(c.intermediate) && c.vocab_size && c.max_pos && c.type_vocab &&
                        (c.head == CQS_HIP_BERT_HEAD_MLM || c.head == CQS_HIP_BERT_HEAD_CLASSIFIER || c.head == CQS_HIP_BERT_HEAD_NONE) &&
                        (c.head != CQS_HIP_BERT_HEAD_CLASSIFIER || (c.num_labels >= 1 && c.num_labels <= 16)) && c.ln_eps > 0.f;
    if (!ok_cfg) return CQS_HIP_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return CQS_HIP_ERR_NO_DEVICE;
    cqs_hip_bert* e = new (std::nothrow) cqs_hip_bert();
    if (!e) return CQS_HIP_ERR_NOMEM;
    std::unique_ptr<cqs_hip_bert, void (*)(cqs_hip_bert*)> owner(e, cqs_hip_bert_destroy);   // every failing exit gives the handle (and its streams) back
    e->device = device;
    e->cfg = c;
    e->vpad = (c.vocab_size + 191u) / 192u * 192u;
    e->L.resize(c.layers);
    if (hipSetDevice(device) != hipSuccess) return CQS_HIP_ERR_DEVICE;
    for (BCtx& cx : e->ctx)
        if (hipStreamCreateWithFlags(&cx.stream, hipStreamNonBlocking) != hipSuccess) return CQS_HIP_ERR_DEVICE;
    *out = owner.release();
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

// HF names, with or without the leading `bert.`; data f32, row-major; copied.
int32_t cqs_hip_bert_set_tensor(cqs_hip_bert* e, const char* name, const float* data, uint64_t count) CQS_ABI_TRY {
    if (!e || !name || !data) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->finalized) return efail(e, CQS_HIP_ERR_INVALID, "bert: weights already finalized");
    std::string n(name);
    if (n.rfind("bert.", 0) == 0) n = n.substr(5);
    e->pending[n].assign(data, data + count);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

int32_t cqs_hip_bert_finalize(cqs_hip_bert* e) CQS_ABI_TRY {
    if (!e) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->finalized) return CQS_HIP_OK;
    E_TRY(e, hipSetDevice(e->device));
    const cqs_hip_bert_config& c = e->cfg;
    const size_t H = c.hidden, I = c.intermediate, V = c.vocab_size;
    auto need = [&](const std::string& name, size_t count) -> const float* {
        const std::vector<float>* v = find(e, name, count);
        if (!v) efail(e, CQS_HIP_ERR_INVALID, "bert: missing or mis-sized tensor " + name);
        return v ? v->data() : nullptr;
    };
    int32_t rc;
#define NEED(var, name, count) const float* var = need(name, count); if (!var) return CQS_HIP_ERR_INVALID
#define UP(call) if ((rc = (call)) != CQS_HIP_OK) return rc
    NEED(word, "embeddings.word_embeddings.weight", V * H);
    NEED(posw, "embeddings.position_embeddings.weight", (size_t)c.max_pos * H);
    NEED(typew, "embeddings.token_type_embeddings.weight", (size_t)c.type_vocab * H);
    NEED(eg, "embeddings.LayerNorm.weight", H);
    NEED(eb, "embeddings.LayerNorm.bias", H);
    UP(up_bf16(e, &e->word, word, V * H, (size_t)e->vpad * H));      // zero rows up to vpad: the tied decoder's padded N
    UP(up_bf16(e, &e->posw, posw, (size_t)c.max_pos * H));
    UP(up_bf16(e, &e->typew, typew, (size_t)c.type_vocab * H));
    UP(up_f32(e, &e->emb_g, eg, H));
    UP(up_f32(e, &e->emb_b, eb, H));
    for (uint32_t l = 0; l < c.layers; ++l) {
        const std::string p = "encoder.layer." + std::to_string(l) + ".";
        BertLayer& w = e->L[l];
        NEED(wq, p + "attention.self.query.weight", H * H);
        NEED(wk, p + "attention.self.key.weight", H * H);
        NEED(wv, p + "attention.self.value.weight", H * H);
        NEED(bq, p + "attention.self.query.bias", H);
        NEED(bk, p + "attention.self.key.bias", H);
        NEED(bv, p + "attention.self.value.bias", H);
        std::vector<float> fw(3 * H * H), fb(3 * H);
        memcpy(fw.data(), wq, H * H * 4); memcpy(fw.data() + H * H, wk, H * H * 4); memcpy(fw.data() + 2 * H * H, wv, H * H * 4);
        memcpy(fb.data(), bq, H * 4); memcpy(fb.data() + H, bk, H * 4); memcpy(fb.data() + 2 * H, bv, H * 4);
        UP(up_bf16(e, &w.wqkv, fw.data(), fw.size()));
        UP(up_f32(e, &w.bqkv, fb.data(), fb.size()));
        NEED(wo, p + "attention.output.dense.weight", H * H);
        NEED(bo, p + "attention.output.dense.bias", H);
        NEED(g1, p + "attention.output.LayerNorm.weight", H);
        NEED(b1n, p + "attention.output.LayerNorm.bias", H);
        NEED(w1, p + "intermediate.dense.weight", I * H);
        NEED(b1, p + "intermediate.dense.bias", I);
        NEED(w2, p + "output.dense.weight", H * I);
        NEED(b2, p + "output.dense.bias", H);
        NEED(g2, p + "output.LayerNorm.weight", H);
        NEED(b2n, p + "output.LayerNorm.bias", H);
        UP(up_bf16(e, &w.wo, wo, H * H)); UP(up_f32(e, &w.bo, bo, H));
        UP(up_f32(e, &w.ln1_g, g1, H)); UP(up_f32(e, &w.ln1_b, b1n, H));
        UP(up_bf16(e, &w.w1, w1, I * H)); UP(up_f32(e, &w.b1, b1, I));
        UP(up_bf16(e, &w.w2, w2, H * I)); UP(up_f32(e, &w.b2, b2, H));
        UP(up_f32(e, &w.ln2_g, g2, H)); UP(up_f32(e, &w.ln2_b, b2n, H));
    }
    if (c.head == CQS_HIP_BERT_HEAD_MLM) {
        NEED(wt, "cls.predictions.transform.dense.weight", H * H);
        NEED(bt, "cls.predictions.transform.dense.bias", H);
        NEED(lg, "cls.predictions.transform.LayerNorm.weight", H);
        NEED(lb, "cls.predictions.transform.LayerNorm.bias", H);
        NEED(bd, "cls.predictions.bias", V);
        UP(up_bf16(e, &e->wt, wt, H * H)); UP(up_f32(e, &e->bt, bt, H));
        UP(up_f32(e, &e->lnt_g, lg, H)); UP(up_f32(e, &e->lnt_b, lb, H));
        UP(up_f32(e, &e->bdec, bd, V, e->vpad));
    } else if (c.head == CQS_HIP_BERT_HEAD_CLASSIFIER) {
        NEED(wp, "pooler.dense.weight", H * H);
        NEED(bp, "pooler.dense.bias", H);
        NEED(wc, "classifier.weight", (size_t)c.num_labels * H);
        NEED(bc, "classifier.bias", c.num_labels);
        UP(up_bf16(e, &e->wp, wp, H * H)); UP(up_f32(e, &e->bp, bp, H));
        UP(up_bf16(e, &e->wc, wc, (size_t)c.num_labels * H, (size_t)16 * H));    // zero rows up to 16 labels
        UP(up_f32(e, &e->bc, bc, c.num_labels, 16));
    }
#undef NEED
#undef UP
    e->pending.clear();
    e->finalized = true;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

// `create_session` for these two models (src/embedder/provider.rs:254-447 via src/splade/mod.rs:433-560 and
// src/reranker.rs:266-330): the local bundle is `{dir}/onnx/model.onnx` (+ external data) or `{dir}/model.onnx`
// (src/reranker.rs:548-556); a Hugging Face checkpoint directory (`model.safetensors`) is accepted as well.
// ONNX initialisers are found as in the embedding engine (onnx_reader.cpp): named tensors by name, anonymous
// transposed MatMul operands through the consuming node's module path.
int32_t cqs_hip_bert_load_dir(const char* model_dir, const cqs_hip_bert_config* cfg, int32_t device, cqs_hip_bert** out) CQS_ABI_TRY {
    if (!model_dir || !cfg || !out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    cqs_hip_bert* e = nullptr;
    int32_t rc = cqs_hip_bert_create(cfg, device, &e);
    if (rc != CQS_HIP_OK) return rc;
    struct Owner {   // every exit but the last, exceptions out of the readers included, gives the handle back
        cqs_hip_bert* p;
        ~Owner() { if (p) cqs_hip_bert_destroy(p); }
    } owner{e};
    const std::string d(model_dir);
    auto exists = [](const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; };
    // names both readers may hand over -> the engine's; unknown tensors (graph constants, position_ids) are skipped
    auto canon = [&](std::string n) -> std::string {
        if (n.rfind("bert.", 0) == 0) n = n.substr(5);
        if (n.rfind("layer.", 0) == 0) n = "encoder." + n;                 // (onnx_reader strips a leading `encoder.`)
        if (n == "cls.predictions.decoder.bias") n = "cls.predictions.bias";
        if (n == "cls.predictions.decoder.weight") return std::string();    // tied to the word embeddings
        const bool known = n.rfind("embeddings.", 0) == 0 || n.rfind("encoder.layer.", 0) == 0 ||
                           (e->cfg.head == CQS_HIP_BERT_HEAD_MLM && n.rfind("cls.predictions.", 0) == 0) ||
                           (e->cfg.head == CQS_HIP_BERT_HEAD_CLASSIFIER && (n.rfind("pooler.", 0) == 0 || n.rfind("classifier.", 0) == 0));
        return known ? n : std::string();
    };
    std::string err;
    int fed = -1;
    std::string onnx = d + "/onnx/model.onnx";
    if (!exists(onnx)) onnx = d + "/model.onnx";
    if (exists(onnx)) {
        fed = cqs_onnx::load(onnx, e->cfg.hidden, 0,
            [&](const std::string& name, const float* data, uint64_t count, const std::vector<uint64_t>&) -> int {
                const std::string n = canon(name);
                if (n.empty()) return 0;
                return cqs_hip_bert_set_tensor(e, n.c_str(), data, count) == CQS_HIP_OK ? 1 : -1;
            }, err);
    } else if (exists(d + "/model.safetensors")) {
        fed = cqs_st::load(d + "/model.safetensors", [&](const std::string& name, const float* data, uint64_t count) -> int {
            const std::string n = canon(name);
            if (n.empty()) return 0;
            return cqs_hip_bert_set_tensor(e, n.c_str(), data, count) == CQS_HIP_OK ? 1 : -1;
        }, err);
    } else {
        err = "no onnx/model.onnx, model.onnx or model.safetensors under " + d;
    }
    if (fed < 0) {
        fprintf(stderr, "[cqs_hip] bert load_dir failed: %s\n", err.c_str());
        return CQS_HIP_ERR_INVALID;
    }
    rc = cqs_hip_bert_finalize(e);
    if (rc != CQS_HIP_OK) {
        fprintf(stderr, "[cqs_hip] bert load_dir failed: %s\n", e->last_error.c_str());
        return rc;
    }
    owner.p = nullptr;
    *out = e;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

void cqs_hip_bert_destroy(cqs_hip_bert* e) CQS_ABI_TRY {
    if (!e) return;
    (void)hipSetDevice(e->device);
    for (BCtx& c : e->ctx)
        if (c.stream) (void)hipStreamSynchronize(c.stream);
    for (void* p : e->owned) (void)hipFree(p);
    for (BCtx& c : e->ctx) {
        free_scratch(c);
        if (c.stream) (void)hipStreamDestroy(c.stream);
    }
    for (BSlot& sl : e->slot) {
        if (sl.meta) (void)hipHostFree(sl.meta);
        if (sl.out) (void)hipHostFree(sl.out);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    delete e;
} CQS_ABI_CATCH_VOID

uint32_t cqs_hip_bert_vocab(const cqs_hip_bert* e) CQS_ABI_TRY { return e ? e->cfg.vocab_size : 0; } CQS_ABI_CATCH_VAL(0)
int32_t cqs_hip_bert_poisoned(const cqs_hip_bert* e) CQS_ABI_TRY { return e && e->poisoned.load(std::memory_order_acquire) ? 1 : 0; } CQS_ABI_CATCH_NOHANDLE
size_t cqs_hip_bert_last_error(cqs_hip_bert* e, char* buf, size_t cap) CQS_ABI_TRY {
    if (!e || !buf || cap == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t m = e->last_error.size() < cap - 1 ? e->last_error.size() : cap - 1;
    memcpy(buf, e->last_error.data(), m);
    buf[m] = 0;
    return m;
} CQS_ABI_CATCH_VAL(0)

}  // extern "C"
