// sparse_update_host.h — the device-free part of cqs_hip_sparse_index_remove / _extend: the arguments
// checked, the chunk and rank renumbering, the new token table, and the rules that say where every posting of the updated
// index sits.  Plain C++ over the caller's arrays, no HIP, no handle: sparse_index_update.hip calls it under the handle's
// mutex and its kernels call the position rules; tests/sparse_update_host_driver.cpp runs all of it under ASAN + UBSan
// on the CPU.
//
// "Position" below is what a posting stores in .x: the chunk's rank in ascending id order on a ranked handle, the chunk
// index on an unranked one (chunk_of_rank empty = identity).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "sparse_build_host.h"
#include "sparse_geometry.h"

#if defined(__HIPCC__)
#define CQS_SU_HD __host__ __device__
#else
#define CQS_SU_HD
#endif

namespace cqs_sparse_update {

constexpr uint32_t kGone = 0xFFFFFFFFu;             // remap[] of a removed chunk's position; "no old list" of a new token
constexpr uint64_t kChunkLimit = cqs::kSparseMaxChunks;   // create refuses n >= this

using cqs_sparse_build::Posting;                    // {position, weight bits}: the layout of the device's uint2

enum class Plan : int32_t {
    Invalid = -1,   // CQS_HIP_ERR_INVALID; *why says which argument; nothing planned
    Nothing = 0,    // nothing to remove / to add: CQS_HIP_OK, the index stays as it is
    Update = 1,
};

// ---- the position rules (host and device) ------------------------------------------------------------------------------
// Entries of p[0 .. n) with .x < key; p ascending in .x.
template <class P>
CQS_SU_HD inline uint32_t count_below(const P* p, uint32_t n, uint32_t key) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2u;
        if (p[m].x < key) a = m + 1u; else b = m;
    }
    return a;
}

// The list that holds posting e: the largest t in [0, lists) with off[t] <= e (off ascending, off[0] = 0, e < off[lists]).
CQS_SU_HD inline uint32_t list_of(const uint64_t* off, uint32_t lists, uint64_t e) {
    uint32_t lo = 0, hi = lists;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// remove, kept old posting e of list t: new_off[slot(t)] + K(e) - K(off[t]), K = the global exclusive count of kept
// postings.  remove_token_table sets new_off[slot(t)] = K(off[t]) - the lists stay in token order and a dead list holds no
// kept posting - so the device passes K(e) alone (start terms 0); the driver checks the long form against it.
CQS_SU_HD inline uint64_t remove_position(uint64_t new_off_slot, uint64_t k_e, uint64_t k_start) {
    return new_off_slot + (k_e - k_start);
}
// extend, old posting e of list t: new_off[slot'(t)] + (e - off[t]) + #(added postings of t with final rank < lifted rank of e)
CQS_SU_HD inline uint64_t extend_old_position(uint64_t new_off_slot, uint64_t e_in_list, uint32_t added_below) {
    return new_off_slot + e_in_list + added_below;
}
// extend, j-th added posting of token t, final rank R: new_off[slot'(t)] + j + #(old postings of t with old rank < R - #(new ranks < R))
CQS_SU_HD inline uint64_t extend_added_position(uint64_t new_off_slot, uint64_t j, uint32_t old_below) {
    return new_off_slot + j + old_below;
}

// ---- remove ------------------------------------------------------------------------------------------------------------
struct RemovePlan {
    std::vector<uint32_t> removed;         // the distinct chunk indices, ascending
    std::vector<uint32_t> remap;           // [n] old position -> new position, kGone for a removed chunk's
    std::vector<uint32_t> chunk_of_rank;   // the new one (ranked handles; empty otherwise)
    uint64_t n_new = 0;
};

// cqs_hip_sparse_index_remove's arguments against an index of n chunks (chunk_of_rank: n entries, or empty = unranked).
inline Plan plan_remove(const uint64_t* chunks, uint64_t m, uint64_t n, const std::vector<uint32_t>& chunk_of_rank, RemovePlan* out,
                        const char** why) {
    *out = RemovePlan();
    out->n_new = n;
    if (m == 0) return Plan::Nothing;
    if (!chunks) { *why = "null chunks"; return Plan::Invalid; }
    for (uint64_t i = 0; i < m; ++i)
        if (chunks[i] >= n) { *why = "chunk index not in this index"; return Plan::Invalid; }
    out->removed.reserve(m);
    for (uint64_t i = 0; i < m; ++i) out->removed.push_back((uint32_t)chunks[i]);
    std::sort(out->removed.begin(), out->removed.end());
    out->removed.erase(std::unique(out->removed.begin(), out->removed.end()), out->removed.end());
    // survivors keep their relative chunk order and are renumbered densely (np.delete on the id list)
    std::vector<uint32_t> renum((size_t)n);
    {
        size_t j = 0;
        for (uint64_t c = 0; c < n; ++c) {
            if (j < out->removed.size() && out->removed[j] == c) { renum[c] = kGone; ++j; }
            else renum[c] = (uint32_t)(c - j);
        }
    }
    const bool ranked = !chunk_of_rank.empty();
    out->n_new = n - out->removed.size();
    out->remap.resize((size_t)n);
    if (ranked) out->chunk_of_rank.resize((size_t)out->n_new);
    uint32_t next = 0;                     // ... and so do their ranks
    for (uint64_t r = 0; r < n; ++r) {
        const uint32_t c = ranked ? chunk_of_rank[r] : (uint32_t)r;
        if (renum[c] == kGone) { out->remap[r] = kGone; continue; }
        if (ranked) out->chunk_of_rank[next] = renum[c];
        out->remap[r] = next++;
    }
    return Plan::Update;
}

// From K at the list starts (k[t] = kept postings before old posting off[t], k[lists] = all kept): the surviving tokens and
// their offsets.  A token whose every posting belonged to removed chunks is gone.
inline void remove_token_table(const std::vector<uint32_t>& tok, const std::vector<uint64_t>& k, std::vector<uint32_t>* new_tok,
                               std::vector<uint64_t>* new_off) {
    new_tok->clear();
    new_off->clear();
    for (size_t t = 0; t < tok.size(); ++t)
        if (k[t + 1] > k[t]) { new_tok->push_back(tok[t]); new_off->push_back(k[t]); }
    new_off->push_back(k.empty() ? 0 : k.back());
}

// ---- extend ------------------------------------------------------------------------------------------------------------
struct ExtendPlan {
    uint64_t n_total = 0;
    std::vector<uint32_t> lift;            // [n_old] old position -> final position
    std::vector<uint32_t> chunk_of_rank;   // the new one (ranked handles; empty otherwise)
    std::vector<uint32_t> tok;             // the merged token table ...
    std::vector<uint64_t> off;             // ... and its offsets [tok.size() + 1]
    std::vector<uint32_t> new_slot;        // [old lists] slot'(t): where old list t sits in `tok`
    std::vector<uint32_t> old_slot;        // [tok.size()] the old list of a merged list, kGone = a token the index never saw
    std::vector<uint64_t> add_off;         // [tok.size() + 1] the merged list's slice of `added`
    std::vector<Posting> added;            // the added postings {final position, weight bits}, sorted by (token, position), stable
    std::vector<uint32_t> added_slot;      // [added] the merged list each belongs to
    std::vector<uint32_t> added_thr;       // [added] old positions below this one sort in front of it: R - #(new ranks < R)
};

// cqs_hip_sparse_index_extend's arguments against an index of n_old chunks with token table (old_tok, old_off); ranked says
// whether the handle was created with id_rank (old_chunk_of_rank then has n_old entries).
inline Plan plan_extend(const uint64_t* doc_off, const uint32_t* tokens, const float* weights, uint64_t n_new, const uint32_t* new_rank,
                        uint64_t n_old, bool ranked, const std::vector<uint32_t>& old_chunk_of_rank, const std::vector<uint32_t>& old_tok,
                        const std::vector<uint64_t>& old_off, ExtendPlan* out, const char** why) {
    *out = ExtendPlan();
    out->n_total = n_old;
    if (n_new == 0) return Plan::Nothing;
    if (n_new >= kChunkLimit || n_old + n_new >= kChunkLimit) { *why = "too many chunks"; return Plan::Invalid; }   // (before doc_off[n_new] is read)
    if (!cqs_sparse_build::check_csr(doc_off, n_new, tokens, weights, why)) return Plan::Invalid;
    const uint64_t PA = doc_off[n_new];
    if (new_rank && !ranked) { *why = "new_rank on an index created without id_rank"; return Plan::Invalid; }
    const uint64_t n_total = n_old + n_new;
    // final position of every new chunk; the new ranks in ascending order
    std::vector<uint32_t> final_pos((size_t)n_new), by_rank((size_t)n_new);
    std::iota(by_rank.begin(), by_rank.end(), 0u);
    if (new_rank) {
        for (uint64_t i = 0; i < n_new; ++i)
            if (new_rank[i] >= n_total) { *why = "new_rank out of range"; return Plan::Invalid; }
        std::sort(by_rank.begin(), by_rank.end(), [&](uint32_t a, uint32_t b) { return new_rank[a] < new_rank[b]; });
        for (uint64_t j = 1; j < n_new; ++j)
            if (new_rank[by_rank[j]] == new_rank[by_rank[j - 1]]) { *why = "new_rank given twice"; return Plan::Invalid; }
        for (uint64_t i = 0; i < n_new; ++i) final_pos[i] = new_rank[i];
    } else {
        for (uint64_t i = 0; i < n_new; ++i) final_pos[i] = (uint32_t)(n_old + i);
    }
    // the old-rank threshold of every new chunk: with the new ranks sorted, the j-th one has `rank - j` old chunks below it
    std::vector<uint32_t> thr_of((size_t)n_new), thr_sorted((size_t)n_new);
    for (uint64_t j = 0; j < n_new; ++j) {
        thr_sorted[j] = final_pos[by_rank[j]] - (uint32_t)j;
        thr_of[by_rank[j]] = thr_sorted[j];
    }
    // hence the lift old_rank -> old_rank + #(thresholds <= old_rank)
    out->lift.resize((size_t)n_old);
    {
        uint64_t j = 0;
        for (uint64_t r = 0; r < n_old; ++r) {
            while (j < n_new && thr_sorted[j] <= r) ++j;
            out->lift[r] = (uint32_t)(r + j);
        }
    }
    if (ranked) {
        out->chunk_of_rank.resize((size_t)n_total);
        for (uint64_t r = 0; r < n_old; ++r) out->chunk_of_rank[out->lift[r]] = old_chunk_of_rank[r];
        for (uint64_t i = 0; i < n_new; ++i) out->chunk_of_rank[final_pos[i]] = (uint32_t)(n_old + i);
    }
    // the added postings by (token, final position); stable, so a chunk's repeated tokens keep document order
    std::vector<uint64_t> order((size_t)PA);
    std::vector<uint32_t> doc_of((size_t)PA);
    for (uint64_t i = 0; i < n_new; ++i)
        for (uint64_t e = doc_off[i]; e < doc_off[i + 1]; ++e) doc_of[e] = (uint32_t)i;
    std::iota(order.begin(), order.end(), (uint64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (tokens[a] != tokens[b]) return tokens[a] < tokens[b];
        return final_pos[doc_of[a]] < final_pos[doc_of[b]];
    });
    // the merged token table and offsets
    const size_t U = old_tok.size();
    out->new_slot.assign(U, kGone);
    out->added.resize((size_t)PA);
    out->added_slot.resize((size_t)PA);
    out->added_thr.resize((size_t)PA);
    out->off.push_back(0);
    out->add_off.push_back(0);
    size_t t = 0;
    uint64_t a = 0;
    while (t < U || a < PA) {
        const bool take_old = t < U && (a >= PA || old_tok[t] <= tokens[order[a]]);
        const uint32_t token = take_old ? old_tok[t] : tokens[order[a]];
        const uint32_t slot = (uint32_t)out->tok.size();
        uint64_t len = 0;
        if (take_old) { len = old_off[t + 1] - old_off[t]; out->new_slot[t] = slot; out->old_slot.push_back((uint32_t)t); ++t; }
        else out->old_slot.push_back(kGone);
        for (; a < PA && tokens[order[a]] == token; ++a, ++len) {
            const uint64_t e = order[a];
            uint32_t bits;
            memcpy(&bits, &weights[e], 4);
            out->added[a] = Posting{final_pos[doc_of[e]], bits};
            out->added_slot[a] = slot;
            out->added_thr[a] = thr_of[doc_of[e]];
        }
        if (len > 0xFFFFFFFFull) { *why = "a posting list would exceed 2^32 postings"; *out = ExtendPlan(); out->n_total = n_old; return Plan::Invalid; }
        out->tok.push_back(token);
        out->off.push_back(out->off.back() + len);
        out->add_off.push_back(a);
    }
    out->n_total = n_total;
    return Plan::Update;
}

}  // namespace cqs_sparse_update
