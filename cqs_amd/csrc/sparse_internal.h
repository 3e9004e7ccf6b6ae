// sparse_internal.h — the sparse index handle and what crosses its translation units: sparse_index.hip (the scoring kernel
// and the search), sparse_index_create.hip (constructors, destroy, accessors), sparse_index_persist.hip (save / load),
// sparse_index_tags.hip (chunk tags), sparse_index_update.hip (remove / extend in place).
// Internal to libcqs_hip.so (the public boundary is include/cqs_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cqs_hip.h"
#include "combine_queue.h"
#include "sparse_build_host.h"
#include "sparse_geometry.h"

// the host headers' posting is the device's uint2, member for member
static_assert(sizeof(cqs_sparse_build::Posting) == sizeof(uint2) && alignof(cqs_sparse_build::Posting) == alignof(uint2) &&
                  offsetof(cqs_sparse_build::Posting, x) == offsetof(uint2, x) && offsetof(cqs_sparse_build::Posting, y) == offsetof(uint2, y),
              "cqs_sparse_build::Posting must have uint2's layout");

// One single-query search waiting for a shared pair of launches (the combining queue of cqs_hip_sparse_index_search).
// Lives on its caller's stack; the pointers are the caller's own buffers.
struct cqs_sparse_req {
    const uint32_t* q_tokens;
    const float* q_weights;
    uint32_t n_terms, k;
    uint64_t* out_chunks;
    float* out_scores;
    uint32_t* out_count;
    int32_t rc = 0;
    bool done = false;
};

struct cqs_hip_sparse_index {
    std::mutex mu;
    // combining queue (combine_queue.h): concurrent unfiltered single-query calls share launches; cq.wait_us is CQS_HIP_COMBINE_WAIT_US
    cqs_combine::Queue<cqs_sparse_req, cqs::kSparseMaxBatch> cq;
    bool combine = true;                     // CQS_HIP_COMBINE=0 turns it off (read at create)
    std::atomic<uint64_t> stat_passes{0}, stat_queries{0};
    std::string last_error;
    std::atomic<bool> poisoned{false};
    int device = 0;
    uint64_t n = 0, n_postings = 0;
    uint32_t n_pad = 0, rw = 64, sh = 6, n_cu = 256;
    bool ranked = false;
    bool group16 = false;                    // maxima per 16 chunks instead of 64 (indexes up to 262 144 chunks)
    std::vector<uint32_t> tok;               // sorted distinct token ids
    std::vector<uint64_t> off;               // [tok.size() + 1]
    std::vector<uint32_t> chunk_of_rank;     // host copy (empty: identity)
    hipStream_t stream = nullptr;
    uint2* d_post = nullptr;
    uint32_t* d_chunk_of_rank = nullptr;
    float* d_scores = nullptr;
    float* d_gmax = nullptr;
    uint32_t* d_work = nullptr;
    uint32_t* d_keep = nullptr;
    cqs::SparseTerm* d_terms = nullptr;
    uint32_t* d_qoff = nullptr;              // [kSparseMaxBatch + 1] first term of every query of a batch
    uint32_t* h_qoff = nullptr;              // pinned
    uint32_t b_cap = 0;                      // queries the score / maxima / key scratch holds
    uint32_t terms_cap = 0;
    cqs::SparseTerm* h_terms = nullptr;      // pinned
    uint32_t* d_dir = nullptr;               // range directories, list after list: n_pad / rw + 1 entries each
    std::vector<uint64_t> dir_off;           // [tok.size()]: a list's first entry in d_dir, kNoDir = none
    uint64_t dir_entries = 0;
    uint32_t* h_keep = nullptr;              // pinned, ceil(n / 32) words
    uint64_t* d_out_keys = nullptr;
    uint32_t* d_out_count = nullptr;
    uint64_t* h_out_keys = nullptr;          // pinned + device-visible, kMaxK + 1 words (the last one: the count): the select writes here
    uint64_t* h_out_keys_dev = nullptr;      // its device address (null: not mappable -> device buffer + two copies)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    unsigned long long* d_dbg = nullptr;     // CQS_HIP_DEBUG_STAMPS=1: select_finish phase stamps of the last search (printed to stderr)
    float last_ms = 0.f;
    std::atomic<bool> want_timing{false};    // set by the first last_search that asks for the time: searches are timed from then on
    uint64_t last_touched = 0;
    // Chunk tags: one u32 per chunk INDEX (what keep_bitset is indexed by), chunks [0, h_tags.size()) have
    // one.  The host copy is the master - remove renumbers it with the chunks, extend keeps it - and d_tags its device copy
    // (null until the first set_tags; tags_cap entries, regrown from the host copy when the index outgrows it).
    std::vector<uint32_t> h_tags;
    uint32_t* d_tags = nullptr;
    uint64_t tags_cap = 0;
};

namespace cqs_sparse {

inline int32_t sfail(cqs_hip_sparse_index* s, int32_t code, const std::string& what, hipError_t he = hipSuccess) {
    s->last_error = what;
    if (he != hipSuccess) s->last_error += std::string(": ") + hipGetErrorString(he);
    if (code == CQS_HIP_ERR_DEVICE) s->poisoned = true;
    return code;
}

// sparse_index_create.hip.  create_handle is every constructor: the device checked (CQS_HIP_ERR_NO_DEVICE), a fresh handle
// given to `fill` - which sets n, ranked, chunk_of_rank, tok and off, hands back the host postings and says false to
// refuse its arguments (CQS_HIP_ERR_INVALID) - then finish_create (device, wave ranges, range directories, scratch), and
// the handle is the caller's.  On every failure what exists so far is released.
using Fill = std::function<bool(cqs_hip_sparse_index* s, std::vector<cqs_sparse_build::Posting>* post)>;
int32_t create_handle(int32_t device, const Fill& fill, cqs_hip_sparse_index** out);

// sparse_index.hip.  ensure_batch: score rows, maxima and result keys for `b` queries (grown on demand).  search_locked:
// shared by the search entry points; the caller holds s->mu.  q_off [b + 1]: the terms of query q are q_tokens / q_weights
// [q_off[q], q_off[q + 1]).  allow (with a null keep_bitset; every chunk has a tag): the keep-bitset is the tag filter's,
// written into d_keep by tags_keep_kernel in front of the scoring launch instead of copied from the host.
int32_t ensure_batch(cqs_hip_sparse_index* s, uint32_t b);
int32_t search_locked(cqs_hip_sparse_index* s, const uint64_t* q_off, const uint32_t* q_tokens, const float* q_weights, uint32_t b,
                      uint32_t k, const uint32_t* keep_bitset, uint64_t* out_chunks, float* out_scores, uint32_t* out_counts,
                      const uint32_t* allow = nullptr);

// The tags follow an update that succeeded (sparse_index_tags.hip).  Caller holds mu; the stream is idle.  Memory that fails
// here drops the tags (reason in last_error), never the update.
void tags_after_remove(cqs_hip_sparse_index* s, const std::vector<uint32_t>& removed);   // distinct chunk indices, ascending
void tags_after_extend(cqs_hip_sparse_index* s);

}  // namespace cqs_sparse

#define S_TRY(s, expr)                                                                   \
    do {                                                                                 \
        const hipError_t he_ = (expr);                                                   \
        if (he_ != hipSuccess) return cqs_sparse::sfail((s), he_ == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, #expr, he_); \
    } while (0)
