// sparse_internal.h — the sparse index handle and the host helpers shared by its translation units (sparse_index.hip:
// constructors, persistence, search; sparse_index_update.hip: remove / extend in place).
// Internal to libcqs_hip.so (the public boundary is include/cqs_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cqs_hip.h"
#include "combine_queue.h"
#include "sparse_geometry.h"

namespace cqs {

constexpr uint32_t kUnscored = 0xFFFFFFFFu;    // LDS marker: `scores.entry(chunk)` does not exist yet (a NaN bit pattern: weights that
                                               // carry it are refused at build / search, a sum that lands on it is stored as 0x7FC00000)
constexpr uint32_t kMaxTerms = 1u << 16;        // per query
constexpr uint32_t kSparseMaxBatch = 64;       // queries per cqs_hip_sparse_index_search_batch call

struct SparseTerm {            // one query term, resolved on the host
    unsigned long long start;  // first posting of the token's list
    unsigned long long dir;    // first entry of the list's range directory (kNoDir: none - the wave bisects the list)
    uint32_t len;              // postings in the list
    float w;                   // query weight
};

}  // namespace cqs

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

// The tags follow an update that succeeded (sparse_index.hip).  Caller holds mu; the stream is idle.  Memory that fails
// here drops the tags (reason in last_error), never the update.
void tags_after_remove(cqs_hip_sparse_index* s, const std::vector<uint32_t>& removed);   // distinct chunk indices, ascending
void tags_after_extend(cqs_hip_sparse_index* s);

}  // namespace cqs_sparse

#define S_TRY(s, expr)                                                                   \
    do {                                                                                 \
        const hipError_t he_ = (expr);                                                   \
        if (he_ != hipSuccess) return cqs_sparse::sfail((s), he_ == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, #expr, he_); \
    } while (0)
