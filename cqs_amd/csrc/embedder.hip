// embedder.hip — the EmbeddingGemma engine's weights behind the C ABI (include/cqs_hip.h, embed section): create, set_tensor,
// finalize, load_dir with its safetensors / ONNX feeders, destroy and the small accessors.  The forward and the tickets:
// embedder_run.hip; the handle: embedder_internal.h.
#include "embedder_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <new>

#include <sys/stat.h>

#include "onnx_reader.h"
#include "safetensors_reader.h"

using namespace cqs_emb;

namespace {

int32_t upload_bf16(cqs_hip_embedder* e, bf16_t* dst, const float* src, size_t count) {
    std::vector<uint16_t> tmp(count);
    for (size_t i = 0; i < count; ++i) tmp[i] = f32_to_bf16_bits(src[i]);
    E_TRY(e, hipMemcpy(dst, tmp.data(), count * 2, hipMemcpyHostToDevice));
    return CQS_HIP_OK;
}
int32_t upload_f32(cqs_hip_embedder* e, float* dst, const float* src, size_t count) {
    E_TRY(e, hipMemcpy(dst, src, count * 4, hipMemcpyHostToDevice));
    return CQS_HIP_OK;
}

const char* kLayerTensors[] = {"input_layernorm.weight", "self_attn.q_proj.weight", "self_attn.k_proj.weight",
                               "self_attn.v_proj.weight", "self_attn.o_proj.weight", "self_attn.q_norm.weight",
                               "self_attn.k_norm.weight", "post_attention_layernorm.weight",
                               "pre_feedforward_layernorm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
                               "mlp.down_proj.weight", "post_feedforward_layernorm.weight"};

// safetensors file -> set_tensor under the names `rename` maps to ("" = skip); reader: safetensors_reader.cpp
int32_t load_safetensors(cqs_hip_embedder* e, const std::string& path, const std::function<std::string(const std::string&)>& rename) {
    std::string err;
    int32_t inner = CQS_HIP_OK;
    const int fed = cqs_st::load(path, [&](const std::string& raw_name, const float* data, uint64_t count) -> int {
        const std::string name = rename(raw_name);
        if (name.empty()) return 0;
        inner = cqs_hip_embedder_set_tensor(e, name.c_str(), data, count);
        return inner == CQS_HIP_OK ? 1 : -1;
    }, err);
    if (fed < 0) return inner != CQS_HIP_OK ? inner : efail(e, CQS_HIP_ERR_INVALID, "load_dir: " + err);
    return CQS_HIP_OK;
}

// Is `name` one of the tensors cqs_hip_embedder_set_tensor accepts for this geometry?
bool known_tensor(const cqs_hip_embedder* e, const std::string& name) {
    if (name == "embed_tokens.weight" || name == "norm.weight" || name == "dense1.weight" || name == "dense2.weight") return true;
    if (name.rfind("layers.", 0) != 0) return false;
    const size_t dot = name.find('.', 7);
    if (dot == std::string::npos) return false;
    for (size_t i = 7; i < dot; ++i) if (name[i] < '0' || name[i] > '9') return false;
    if ((uint32_t)atoi(name.substr(7, dot - 7).c_str()) >= e->g.layers) return false;
    const std::string t = name.substr(dot + 1);
    for (const char* k : kLayerTensors) if (t == k) return true;
    return false;
}

}  // namespace

extern "C" {

void cqs_hip_embed_config_default(cqs_hip_embed_config* c) CQS_ABI_TRY {
    if (!c) return;
    c->vocab_size = 262144; c->hidden = 768; c->layers = 24; c->heads = 3; c->kv_heads = 1; c->head_dim = 256;
    c->intermediate = 1152; c->dense_hidden = 3072; c->sliding_window = 512; c->sliding_pattern = 6; c->max_seq = 2048;
    c->rms_eps = 1e-6f; c->rope_theta_global = 1e6f; c->rope_theta_local = 1e4f; c->query_pre_attn_scalar = 256.f;
} CQS_ABI_CATCH_VOID

int32_t cqs_hip_embedder_create(const cqs_hip_embed_config* c, int32_t device, cqs_hip_embedder** out) CQS_ABI_TRY {
    if (!c || !out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    if (c->head_dim != 256 || c->hidden == 0 || c->hidden % 256 || c->hidden > 1024 || c->intermediate % 64 ||
        c->dense_hidden % 128 || c->kv_heads == 0 || c->heads % c->kv_heads || c->heads / c->kv_heads > 4 || c->heads + c->kv_heads > 8 ||
        c->layers == 0 || c->sliding_pattern == 0 || c->max_seq == 0 || c->vocab_size == 0 || c->hidden % 128)
        return CQS_HIP_ERR_INVALID;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return CQS_HIP_ERR_NO_DEVICE;
    if (device < 0 || device >= cnt) return CQS_HIP_ERR_INVALID;
    cqs_hip_embedder* e = new (std::nothrow) cqs_hip_embedder();
    if (!e) return CQS_HIP_ERR_NOMEM;
    struct Owner {   // an exception below (L.resize, the rope table) must not leak the handle or its device buffers
        cqs_hip_embedder* p;
        ~Owner() { if (p) cqs_hip_embedder_destroy(p); }
    } owner{e};
    e->device = device;
    e->cfg = *c;
    cqs::EmbedGeom& g = e->g;
    g.vocab = c->vocab_size; g.hidden = c->hidden; g.layers = c->layers; g.heads = c->heads; g.kv_heads = c->kv_heads;
    g.head_dim = c->head_dim; g.inter = c->intermediate; g.dense_hidden = c->dense_hidden;
    g.window = c->sliding_window / 2u + 1u;  // bidirectional (configuration_gemma3.py:105-106)
    g.sliding_pattern = c->sliding_pattern; g.max_seq = c->max_seq; g.rms_eps = c->rms_eps;
    g.theta_global = c->rope_theta_global; g.theta_local = c->rope_theta_local;
    g.q_scale = 1.0f / sqrtf(c->query_pre_attn_scalar);
    bool ok = hipSetDevice(device) == hipSuccess;
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0) e->n_cu = (uint32_t)n_cu;
    for (cqs_hip_embedder::Ctx& c : e->ctx) ok = ok && hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) == hipSuccess;
    if (ok && hipHostMalloc((void**)&e->fuse_err, 64, hipHostMallocDefault) == hipSuccess) {
        *e->fuse_err = 0u;
        if (hipHostGetDevicePointer((void**)&e->fuse_err_dev, e->fuse_err, 0) != hipSuccess) { (void)hipGetLastError(); e->fuse_err_dev = nullptr; }
    } else (void)hipGetLastError();                        // (no mappable word: the engine keeps the two-launch chain)
    const size_t H = g.hidden, D = g.head_dim;
    e->L.resize(g.layers);
    ok = ok && dmalloc(&e->emb, (size_t)g.vocab * H) == hipSuccess && dmalloc(&e->n_final, H) == hipSuccess &&
         dmalloc(&e->dense1, (size_t)g.dense_hidden * H) == hipSuccess && dmalloc(&e->dense2, H * g.dense_hidden) == hipSuccess &&
         dmalloc(&e->rope_global, (size_t)g.max_seq * 256) == hipSuccess && dmalloc(&e->rope_local, (size_t)g.max_seq * 256) == hipSuccess;
    for (uint32_t l = 0; ok && l < g.layers; ++l) {
        LayerW& w = e->L[l];
        ok = dmalloc(&w.wqkv, (size_t)nqkv(g) * H) == hipSuccess && dmalloc(&w.wo, H * g.heads * D) == hipSuccess &&
             dmalloc(&w.wgu, (size_t)2 * g.inter * H) == hipSuccess && dmalloc(&w.wd, H * g.inter) == hipSuccess &&
             dmalloc(&w.n_in, H) == hipSuccess && dmalloc(&w.n_post_attn, H) == hipSuccess && dmalloc(&w.n_pre_ffw, H) == hipSuccess &&
             dmalloc(&w.n_post_ffw, H) == hipSuccess && dmalloc(&w.n_q, D) == hipSuccess && dmalloc(&w.n_k, D) == hipSuccess;
    }
    if (!ok) return CQS_HIP_ERR_NOMEM;
    // RoPE tables, computed like transformers does (fp32 inv_freq, fp32 angle; modeling_gemma3.py:188-224)
    std::vector<float> tab((size_t)g.max_seq * 256);
    for (int t = 0; t < 2; ++t) {
        const float theta = t == 0 ? g.theta_global : g.theta_local;
        for (uint32_t pz = 0; pz < g.max_seq; ++pz)
            for (uint32_t i = 0; i < 128; ++i) {
                const float inv = 1.0f / powf(theta, (float)(2 * i) / 256.0f);
                const float a = (float)pz * inv;
                tab[((size_t)pz * 128 + i) * 2] = cosf(a);
                tab[((size_t)pz * 128 + i) * 2 + 1] = sinf(a);
            }
        if (hipMemcpy(t == 0 ? e->rope_global : e->rope_local, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return CQS_HIP_ERR_DEVICE;
    }
    owner.p = nullptr;
    *out = e;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

int32_t cqs_hip_embedder_set_tensor(cqs_hip_embedder* e, const char* cname, const float* data, uint64_t count) CQS_ABI_TRY {
    if (!e || !cname || !data) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->finalized) return efail(e, CQS_HIP_ERR_INVALID, "set_tensor after finalize");
    if (hipSetDevice(e->device) != hipSuccess) return efail(e, CQS_HIP_ERR_DEVICE, "hipSetDevice");
    const cqs::EmbedGeom& g = e->g;
    const std::string name(cname);
    const size_t H = g.hidden, D = g.head_dim, I = g.inter;
    auto need = [&](size_t n) { return count == n; };
    int32_t rc = CQS_HIP_ERR_INVALID;
    if (name == "embed_tokens.weight") { if (need((size_t)g.vocab * H)) rc = upload_bf16(e, e->emb, data, count); }
    else if (name == "norm.weight") { if (need(H)) rc = upload_f32(e, e->n_final, data, count); }
    else if (name == "dense1.weight") { if (need((size_t)g.dense_hidden * H)) rc = upload_bf16(e, e->dense1, data, count); }
    else if (name == "dense2.weight") { if (need((size_t)g.dense_hidden * H)) rc = upload_bf16(e, e->dense2, data, count); }
    else if (name.rfind("layers.", 0) == 0) {
        const size_t dot = name.find('.', 7);
        if (dot == std::string::npos) return efail(e, CQS_HIP_ERR_INVALID, "set_tensor: bad name " + name);
        const uint32_t l = (uint32_t)atoi(name.substr(7, dot - 7).c_str());
        if (l >= g.layers) return efail(e, CQS_HIP_ERR_INVALID, "set_tensor: layer out of range in " + name);
        LayerW& w = e->L[l];
        const std::string t = name.substr(dot + 1);
        if (t == "input_layernorm.weight") { if (need(H)) rc = upload_f32(e, w.n_in, data, count); }
        else if (t == "post_attention_layernorm.weight") { if (need(H)) rc = upload_f32(e, w.n_post_attn, data, count); }
        else if (t == "pre_feedforward_layernorm.weight") { if (need(H)) rc = upload_f32(e, w.n_pre_ffw, data, count); }
        else if (t == "post_feedforward_layernorm.weight") { if (need(H)) rc = upload_f32(e, w.n_post_ffw, data, count); }
        else if (t == "self_attn.q_norm.weight") { if (need(D)) rc = upload_f32(e, w.n_q, data, count); }
        else if (t == "self_attn.k_norm.weight") { if (need(D)) rc = upload_f32(e, w.n_k, data, count); }
        // q | k | v rows stacked into one [nqkv, H] matrix: one GEMM produces all three
        else if (t == "self_attn.q_proj.weight") { if (need(g.heads * D * H)) rc = upload_bf16(e, w.wqkv, data, count); }
        else if (t == "self_attn.k_proj.weight") { if (need(g.kv_heads * D * H)) rc = upload_bf16(e, w.wqkv + (size_t)g.heads * D * H, data, count); }
        else if (t == "self_attn.v_proj.weight") { if (need(g.kv_heads * D * H)) rc = upload_bf16(e, w.wqkv + (size_t)(g.heads + g.kv_heads) * D * H, data, count); }
        else if (t == "self_attn.o_proj.weight") { if (need(H * g.heads * D)) rc = upload_bf16(e, w.wo, data, count); }
        else if (t == "mlp.down_proj.weight") { if (need(H * I)) rc = upload_bf16(e, w.wd, data, count); }
        else if (t == "mlp.gate_proj.weight" || t == "mlp.up_proj.weight") {
            // gate / up rows interleaved per 32 channels: rows [64c, 64c+32) = gate channels [32c, 32c+32),
            // rows [64c+32, 64c+64) = the same channels' up rows -> the GEMM epilogue fuses gelu(gate)*up
            if (need(I * H)) {
                const size_t off = (t == "mlp.up_proj.weight") ? 32 : 0;
                rc = CQS_HIP_OK;
                for (size_t c = 0; c < I / 32 && rc == CQS_HIP_OK; ++c)
                    rc = upload_bf16(e, w.wgu + (64 * c + off) * H, data + 32 * c * H, 32 * H);
            }
        } else return efail(e, CQS_HIP_ERR_INVALID, "set_tensor: unknown tensor " + name);
    } else return efail(e, CQS_HIP_ERR_INVALID, "set_tensor: unknown tensor " + name);
    if (rc == CQS_HIP_ERR_INVALID) return efail(e, rc, "set_tensor: wrong element count for " + name);
    if (rc == CQS_HIP_OK) e->seen[name] = true;
    return rc;
} CQS_ABI_CATCH(e)

int32_t cqs_hip_embedder_finalize(cqs_hip_embedder* e) CQS_ABI_TRY {
    if (!e) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<std::string> need = {"embed_tokens.weight", "norm.weight", "dense1.weight", "dense2.weight"};
    for (uint32_t l = 0; l < e->g.layers; ++l)
        for (const char* t : kLayerTensors) need.push_back("layers." + std::to_string(l) + "." + t);
    for (const std::string& n : need)
        if (!e->seen.count(n)) return efail(e, CQS_HIP_ERR_INVALID, "finalize: missing tensor " + n);
    // the pair-split fused projection kernel streams its weights in 2 KB blocks: re-order wo / wd once (hidden 768 only)
    if (e->g.hidden == 768u && (e->g.heads * e->g.head_dim) % 64u == 0u && e->g.inter % 64u == 0u) {
        if (hipSetDevice(e->device) != hipSuccess) return efail(e, CQS_HIP_ERR_DEVICE, "hipSetDevice");
        const uint32_t H = e->g.hidden, Ko = e->g.heads * e->g.head_dim, Kd = e->g.inter;
        for (LayerW& w : e->L) {
            if (!w.wo_p) E_TRY(e, dmalloc(&w.wo_p, (size_t)H * Ko));
            if (!w.wd_p) E_TRY(e, dmalloc(&w.wd_p, (size_t)H * Kd));
            E_TRY(e, cqs::launch_pack_rowfuse_w(w.wo, w.wo_p, H, Ko, nullptr));
            E_TRY(e, cqs::launch_pack_rowfuse_w(w.wd, w.wd_p, H, Kd, nullptr));
        }
        E_TRY(e, hipDeviceSynchronize());
    }
    if (e->g.heads == 3u * e->g.kv_heads && e->g.head_dim == 256u) {     // QKV rows in tile order for the fused norm + RoPE epilogue
        if (hipSetDevice(e->device) != hipSuccess) return efail(e, CQS_HIP_ERR_DEVICE, "hipSetDevice");
        for (LayerW& w : e->L) {
            if (!w.wqkv_f) E_TRY(e, dmalloc(&w.wqkv_f, (size_t)(e->g.heads + e->g.kv_heads) * 320u * e->g.hidden));
            E_TRY(e, cqs::launch_permute_qkv_rows(w.wqkv, w.wqkv_f, e->g.heads, e->g.kv_heads, e->g.hidden, nullptr));
        }
        E_TRY(e, hipDeviceSynchronize());
    }
    if (const char* fq = getenv("CQS_HIP_QKV_FUSE")) e->fuse_qkv = fq[0] != '0';
    if (const char* g4 = getenv("CQS_HIP_GEGLU4")) e->geglu4 = g4[0] != '0';
    if ((2u * e->g.inter) % 64u == 0u) {                               // gate / up rows interleaved per 4 for the in-register pairing
        if (hipSetDevice(e->device) != hipSuccess) return efail(e, CQS_HIP_ERR_DEVICE, "hipSetDevice");
        for (LayerW& w : e->L) {
            if (!w.wgu_f) E_TRY(e, dmalloc(&w.wgu_f, (size_t)2 * e->g.inter * e->g.hidden));
            E_TRY(e, cqs::launch_permute_geglu_rows(w.wgu, w.wgu_f, 2u * e->g.inter, e->g.hidden, nullptr));
        }
        E_TRY(e, hipDeviceSynchronize());
    }
    e->QL.resize(e->L.size());
    for (size_t l = 0; l < e->L.size(); ++l) {
        const LayerW& w = e->L[l];
        e->QL[l] = cqs::QueryFwdLayer{w.wqkv, w.wo, w.wgu, w.wd, w.n_in, w.n_post_attn, w.n_pre_ffw, w.n_post_ffw, w.n_q, w.n_k};
    }
    const char* qp = getenv("CQS_HIP_QUERY_PATH");
    const char* qg = getenv("CQS_HIP_QUERY_GRAPH");
    e->query_path = cqs::query_forward_supported(e->g) && !(qp && qp[0] == '0');
    e->query_graph = !(qg && qg[0] == '0');
    e->query_max_tokens = cqs::query_forward_max_tokens(e->g);
    const char* qd = getenv("CQS_HIP_QUERY_DIRECT");
    e->query_direct = !(qd && qd[0] == '0');
    const char* ec = getenv("CQS_HIP_EMBED_CONTEXTS");
    e->single_ctx = ec && ec[0] == '1';
    if (const char* fn = getenv("CQS_HIP_GEMM_FUSE_NORM")) e->fuse_norm = fn[0] == '0' ? 0 : (fn[0] == '1' ? 1 : 2);
    if (const char* fr = getenv("CQS_HIP_GEMM_FUSE_NORM_MIN_ROWS")) e->fuse_min_rows = (uint32_t)atoi(fr);
    e->finalized = true;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(e)

int32_t cqs_hip_embedder_load_dir(const char* dir, const cqs_hip_embed_config* cfg, int32_t device, cqs_hip_embedder** out) CQS_ABI_TRY {
    if (!dir || !out) return CQS_HIP_ERR_INVALID;
    cqs_hip_embed_config c;
    if (cfg) c = *cfg; else cqs_hip_embed_config_default(&c);
    cqs_hip_embedder* e = nullptr;
    int32_t rc = cqs_hip_embedder_create(&c, device, &e);
    if (rc != CQS_HIP_OK) return rc;
    struct Owner {   // every exit but the last, exceptions out of the readers included, gives the handle back
        cqs_hip_embedder* p;
        ~Owner() { if (p) cqs_hip_embedder_destroy(p); }
    } owner{e};
    const std::string d(dir);
    auto strip = [](const std::string& n) -> std::string {  // HF checkpoints prefix text-model tensors with "model."
        if (n.rfind("model.", 0) == 0) return n.substr(6);
        return n;
    };
    // What the reference's local-model hook holds (CQS_ONNX_DIR, src/embedder/download.rs:12-41): the structured
    // layout `onnx/model.onnx` (src/embedder/models.rs:455-457) or the flat `model.onnx`, each with its external-data
    // sidecar next to it (download.rs:82).  A Hugging Face checkpoint directory (model.safetensors + 2_Dense/ +
    // 3_Dense/) is read too.
    struct stat stt;
    std::string onnx;
    for (const char* cand : {"/onnx/model.onnx", "/model.onnx"})
        if (onnx.empty() && stat((d + cand).c_str(), &stt) == 0) onnx = d + cand;
    if (!onnx.empty()) {
        std::string err;
        const int fed = cqs_onnx::load(onnx, e->g.hidden, e->g.dense_hidden,
            [&](const std::string& name, const float* data, uint64_t count, const std::vector<uint64_t>&) -> int {
                if (!known_tensor(e, name)) return 0;                      // graph constants etc.
                return cqs_hip_embedder_set_tensor(e, name.c_str(), data, count) == CQS_HIP_OK ? 1 : -1;
            }, err);
        if (fed < 0) rc = efail(e, CQS_HIP_ERR_INVALID, "load_dir: " + err + (e->last_error.empty() ? "" : " (" + e->last_error + ")"));
    } else {
        rc = load_safetensors(e, d + "/model.safetensors", strip);
        if (rc == CQS_HIP_OK)
            rc = load_safetensors(e, d + "/2_Dense/model.safetensors", [](const std::string& n) { return n == "linear.weight" ? std::string("dense1.weight") : std::string(); });
        if (rc == CQS_HIP_OK)
            rc = load_safetensors(e, d + "/3_Dense/model.safetensors", [](const std::string& n) { return n == "linear.weight" ? std::string("dense2.weight") : std::string(); });
    }
    if (rc == CQS_HIP_OK) rc = cqs_hip_embedder_finalize(e);
    if (rc != CQS_HIP_OK) {
        fprintf(stderr, "[cqs_hip] embedder load_dir failed: %s\n", e->last_error.c_str());
        return rc;
    }
    owner.p = nullptr;
    *out = e;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

void cqs_hip_embedder_destroy(cqs_hip_embedder* e) CQS_ABI_TRY {
    if (!e) return;
    (void)hipSetDevice(e->device);
    for (Ctx& c : e->ctx)
        if (c.stream) (void)hipStreamSynchronize(c.stream);
    void* g[] = {e->emb, e->n_final, e->dense1, e->dense2, e->rope_global, e->rope_local};
    for (void* p : g) (void)hipFree(p);
    if (e->fuse_err) (void)hipHostFree(e->fuse_err);
    for (Ctx& c : e->ctx) { free_scratch(c); free_query_scratch(c); }
    for (cqs_hip_embedder::Slot& sl : e->slot) {
        if (sl.meta) (void)hipHostFree(sl.meta);
        if (sl.out) (void)hipHostFree(sl.out);
        if (sl.ev0) (void)hipEventDestroy(sl.ev0);
        if (sl.ev1) (void)hipEventDestroy(sl.ev1);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    for (LayerW& w : e->L) {
        void* ws[] = {w.wgu_f, w.wqkv_f, w.wo_p, w.wd_p, w.wqkv, w.wo, w.wgu, w.wd, w.n_in, w.n_post_attn, w.n_pre_ffw, w.n_post_ffw, w.n_q, w.n_k};
        for (void* p : ws) (void)hipFree(p);
    }
    for (Ctx& c : e->ctx)
        if (c.stream) (void)hipStreamDestroy(c.stream);
    delete e;
} CQS_ABI_CATCH_VOID

uint32_t cqs_hip_embedder_dim(const cqs_hip_embedder* e) CQS_ABI_TRY { return e ? e->g.hidden : 0; } CQS_ABI_CATCH_VAL(0)
uint32_t cqs_hip_embedder_max_seq(const cqs_hip_embedder* e) CQS_ABI_TRY { return e ? e->g.max_seq : 0; } CQS_ABI_CATCH_VAL(0)
int32_t cqs_hip_embedder_poisoned(const cqs_hip_embedder* e) CQS_ABI_TRY { return e && e->poisoned.load(std::memory_order_acquire) ? 1 : 0; } CQS_ABI_CATCH_NOHANDLE
float cqs_hip_embedder_last_ms(const cqs_hip_embedder* e) CQS_ABI_TRY { return e ? e->last_ms : -1.f; } CQS_ABI_CATCH_VAL(-1.f)
size_t cqs_hip_embedder_last_error(const cqs_hip_embedder* e, char* buf, size_t cap) CQS_ABI_TRY {
    if (!e || !buf || cap == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t m = e->last_error.size() < cap - 1 ? e->last_error.size() : cap - 1;
    memcpy(buf, e->last_error.data(), m);
    buf[m] = 0;
    return m;
} CQS_ABI_CATCH_VAL(0)

// `normalize_l2` (src/embedder/pooling.rs:60-67) over the rows of a host matrix: norm_sq folded left to right in
// f32, scaled by 1/sqrt when > 0, zero rows stay zero.  Host helper for callers that keep embeddings in one array.
void cqs_hip_normalize_l2_rows(float* rows, uint64_t n, uint32_t dim) CQS_ABI_TRY {
#pragma clang fp contract(off)   // Rust does not fuse x * x + acc: keep the reference's roundings
    if (!rows) return;
    for (uint64_t r = 0; r < n; ++r) {
        float* v = rows + r * dim;
        float norm_sq = 0.f;
        for (uint32_t i = 0; i < dim; ++i) norm_sq += v[i] * v[i];
        if (norm_sq > 0.f) {
            const float inv = 1.0f / sqrtf(norm_sq);
            for (uint32_t i = 0; i < dim; ++i) v[i] *= inv;
        }
    }
} CQS_ABI_CATCH_VOID

}  // extern "C"
