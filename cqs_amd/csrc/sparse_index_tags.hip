// sparse_index_tags.hip — chunk tags of the sparse index (the dense index's scheme, index_tags.hip, over
// chunk indices): set_tags, tagged_chunks, search_tagged, and what happens to the tags when chunks leave or join.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "sparse_internal.h"
#include "tags_host.h"

using cqs_sparse::search_locked;
using cqs_sparse::sfail;

// The tags after an update (declared in sparse_internal.h).  remove renumbers the surviving chunks densely in their order,
// so the host copy loses the removed chunks' entries and the device copy is written again from it (4 B per chunk, beside a
// rewrite of every posting); extend appends chunks without a tag, so only a column the index has outgrown is regrown.
namespace cqs_sparse {

static void tags_dropped(cqs_hip_sparse_index* s, const char* what) {
    (void)hipGetLastError();
    if (s->d_tags) (void)hipFree(s->d_tags);
    s->d_tags = nullptr;
    s->tags_cap = 0;
    s->h_tags.clear();
    s->last_error = what;
}

void tags_after_remove(cqs_hip_sparse_index* s, const std::vector<uint32_t>& removed) {
    if (s->h_tags.empty() || removed.empty()) return;
    const uint64_t tagged = cqs_tags::tagged_after_remove(removed.data(), removed.size(), s->h_tags.size());
    size_t j = 0, out = 0;
    for (size_t c = 0; c < s->h_tags.size(); ++c) {
        if (j < removed.size() && removed[j] == c) { ++j; continue; }
        s->h_tags[out++] = s->h_tags[c];
    }
    s->h_tags.resize((size_t)tagged);                        // (= out: the rule and the walk agree)
    if (tagged && hipMemcpy(s->d_tags, s->h_tags.data(), (size_t)tagged * 4, hipMemcpyHostToDevice) != hipSuccess)
        tags_dropped(s, "sparse remove: the chunk tags could not be rewritten; they are dropped (set_tags again)");
}

void tags_after_extend(cqs_hip_sparse_index* s) {
    if (!s->d_tags || s->tags_cap >= s->n) return;
    uint32_t* nd = nullptr;
    const uint64_t cap = std::max<uint64_t>(s->n, 2 * s->tags_cap);
    hipError_t he = hipMalloc((void**)&nd, (size_t)cap * 4);
    if (he == hipSuccess && !s->h_tags.empty()) he = hipMemcpy(nd, s->h_tags.data(), s->h_tags.size() * 4, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        if (nd) (void)hipFree(nd);
        tags_dropped(s, "sparse extend: no memory to regrow the chunk tags; they are dropped (set_tags again)");
        return;
    }
    (void)hipFree(s->d_tags);
    s->d_tags = nd;
    s->tags_cap = cap;
}

}  // namespace cqs_sparse

extern "C" {

int32_t cqs_hip_sparse_index_set_tags(cqs_hip_sparse_index* s, uint64_t first_chunk, const uint32_t* tags, uint64_t m) CQS_ABI_TRY {
    if (!s) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    uint64_t first = 0, new_tagged = 0;
    const char* why = "";
    const cqs_tags::Set plan = cqs_tags::plan_set_tags(first_chunk, tags, m, 0, s->n, s->h_tags.size(), &first, &new_tagged, &why);
    if (plan == cqs_tags::Set::Invalid) return sfail(s, CQS_HIP_ERR_INVALID, std::string("sparse set_tags: ") + why);
    if (plan == cqs_tags::Set::Nothing) return CQS_HIP_OK;
    S_TRY(s, hipSetDevice(s->device));
    S_TRY(s, hipStreamSynchronize(s->stream));
    if (!s->d_tags || s->tags_cap < s->n) {                  // (a column that a failed regrow dropped comes back here, whole)
        uint32_t* nd = nullptr;
        S_TRY(s, hipMalloc((void**)&nd, (size_t)s->n * 4));
        if (!s->h_tags.empty()) {
            const hipError_t he = hipMemcpy(nd, s->h_tags.data(), s->h_tags.size() * 4, hipMemcpyHostToDevice);
            if (he != hipSuccess) { (void)hipFree(nd); return sfail(s, CQS_HIP_ERR_DEVICE, "sparse set_tags: copy", he); }
        }
        if (s->d_tags) (void)hipFree(s->d_tags);
        s->d_tags = nd;
        s->tags_cap = s->n;
    }
    S_TRY(s, hipMemcpy(s->d_tags + first, tags, (size_t)m * 4, hipMemcpyHostToDevice));
    s->h_tags.resize((size_t)new_tagged);
    memcpy(s->h_tags.data() + first, tags, (size_t)m * 4);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(s)

uint64_t cqs_hip_sparse_index_tagged_chunks(const cqs_hip_sparse_index* s) CQS_ABI_TRY {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<cqs_hip_sparse_index*>(s)->mu);
    return s->h_tags.size();
} CQS_ABI_CATCH_VAL(0)

int32_t cqs_hip_sparse_index_search_tagged(cqs_hip_sparse_index* s, const uint32_t* q_tokens, const float* q_weights, uint32_t n_terms,
                                           uint32_t k, const uint32_t* allow, uint64_t* out_chunks, float* out_scores,
                                           uint32_t* out_count) CQS_ABI_TRY {
    if (!s) return CQS_HIP_ERR_INVALID;
    {
        std::lock_guard<std::mutex> g(s->mu);
        if (!allow) return sfail(s, CQS_HIP_ERR_INVALID, "sparse search_tagged: null allow");
        if (s->poisoned.load(std::memory_order_acquire)) { if (out_count) *out_count = 0; return CQS_HIP_ERR_POISONED; }
        if (s->h_tags.size() < s->n)
            return sfail(s, CQS_HIP_ERR_INVALID, "sparse search_tagged: tags cover " + std::to_string(s->h_tags.size()) + " of " +
                                                     std::to_string(s->n) + " chunks");
        if (!cqs_tags::all_pass(allow)) {
            if (!out_count) return sfail(s, CQS_HIP_ERR_INVALID, "sparse search: null out_count");
            const uint64_t q_off[2] = {0, n_terms};
            return search_locked(s, q_off, q_tokens, q_weights, 1u, k, nullptr, out_chunks, out_scores, out_count, allow);
        }
    }
    // no field is constrained: the keep_bitset == NULL call (and its place in the combining queue)
    return cqs_hip_sparse_index_search(s, q_tokens, q_weights, n_terms, k, nullptr, out_chunks, out_scores, out_count);
} CQS_ABI_CATCH(s)

}  // extern "C"
