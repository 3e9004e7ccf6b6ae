// sparse_build_host.h — the device-free part of the sparse index's constructors and of its search: the arguments checked,
// the id-order permutation, the token table and the posting array of cqs_hip_sparse_index_create / _create_inverted, the
// host fill of the range directories, and the resolution of a batch's query terms.  Plain C++ over the caller's arrays, no
// HIP, no handle: sparse_index_create.hip and sparse_index.hip call it and only allocate, copy and launch;
// tests/sparse_build_host_driver.cpp runs all of it under ASAN + UBSan on the CPU.
//
// "Position" is what a posting stores in .x: the chunk's rank in ascending id order when the caller gave id_rank, the
// chunk index otherwise (chunk_of_rank empty = identity).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "sparse_geometry.h"

namespace cqs_sparse_build {

struct alignas(8) Posting { uint32_t x, y; };       // {position, weight bits}: the layout and alignment of the device's uint2

constexpr uint32_t kDenseTokenLimit = 1u << 24;     // token ids all below this: the token table by counting, else by sorting

struct Built {
    std::vector<uint32_t> tok;                      // sorted distinct token ids
    std::vector<uint64_t> off;                      // [tok.size() + 1]
    std::vector<Posting> post;                      // the lists back to back, each in ascending position
};

inline uint32_t weight_bits(float w) {
    uint32_t bits;
    memcpy(&bits, &w, 4);
    return bits;
}

// A CSR triple (offsets [n + 1], two payload arrays of off[n] entries, the second one weights) as the constructors and
// extend take it.  The words are those of the documents' form, the one caller (extend) that reports them.
inline bool check_csr(const uint64_t* off, uint64_t n, const uint32_t* a, const float* b, const char** why) {
    if (n == 0) return true;
    if (!off) { *why = "null doc_off"; return false; }
    if (off[0] != 0) { *why = "doc_off does not start at 0"; return false; }
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) { *why = "doc_off not ascending"; return false; }
    const uint64_t P = off[n];
    if (P && (!a || !b)) { *why = "null tokens / weights"; return false; }
    for (uint64_t e = 0; e < P; ++e)
        if (weight_bits(b[e]) == cqs::kUnscored) { *why = "reserved NaN payload in a weight"; return false; }   // the one NaN payload the kernel reserves
    return true;
}

// chunk_of_rank[r] = the chunk whose id is the r-th smallest (empty without id_rank).  false: id_rank is not a permutation
// of 0 .. n - 1.
inline bool rank_table(uint64_t n, const uint32_t* id_rank, std::vector<uint32_t>* chunk_of_rank) {
    chunk_of_rank->clear();
    if (!id_rank) return true;
    chunk_of_rank->assign((size_t)n, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < n; ++i) {
        if (id_rank[i] >= n || (*chunk_of_rank)[id_rank[i]] != 0xFFFFFFFFu) return false;
        (*chunk_of_rank)[id_rank[i]] = (uint32_t)i;
    }
    return true;
}

// cqs_hip_sparse_index_create's arrays from documents that passed check_csr.
inline Built from_documents(const uint64_t* doc_off, const uint32_t* tokens, const float* weights, uint64_t n,
                            const std::vector<uint32_t>& chunk_of_rank) {
    Built x;
    const uint64_t P = n ? doc_off[n] : 0;
    const bool ranked = !chunk_of_rank.empty();
    // the token table: sorted distinct ids; a dense counting pass when the ids are small (every real vocabulary), a sort otherwise
    uint32_t max_tok = 0;
    for (uint64_t e = 0; e < P; ++e) max_tok = std::max(max_tok, tokens[e]);
    std::vector<uint64_t> dense;                          // token -> slot + 1 (dense path)
    std::unordered_map<uint32_t, uint32_t> sparse_slot;   // (sort path)
    const bool use_dense = P && max_tok < kDenseTokenLimit;
    if (use_dense) {
        dense.assign((size_t)max_tok + 1, 0);
        for (uint64_t e = 0; e < P; ++e) dense[tokens[e]]++;
        for (uint32_t t = 0; t <= max_tok; ++t)
            if (dense[t]) { x.tok.push_back(t); x.off.push_back(dense[t]); }
    } else if (P) {
        std::vector<uint32_t> sorted(tokens, tokens + P);
        std::sort(sorted.begin(), sorted.end());
        for (uint64_t e = 0; e < P;) {
            uint64_t f = e;
            while (f < P && sorted[f] == sorted[e]) ++f;
            x.tok.push_back(sorted[e]);
            x.off.push_back(f - e);
            e = f;
        }
    }
    {   // counts -> offsets
        uint64_t run = 0;
        for (size_t t = 0; t < x.off.size(); ++t) { const uint64_t c = x.off[t]; x.off[t] = run; run += c; }
        x.off.push_back(run);
    }
    if (use_dense) {
        for (size_t t = 0; t < x.tok.size(); ++t) dense[x.tok[t]] = t + 1;
    } else {
        sparse_slot.reserve(x.tok.size());
        for (size_t t = 0; t < x.tok.size(); ++t) sparse_slot[x.tok[t]] = (uint32_t)t;
    }
    // the postings, list by list; inside a list ascending position (rank order = the order the documents are walked in)
    x.post.resize((size_t)P);
    std::vector<uint64_t> cur(x.off.begin(), x.off.end() - 1);
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t d = ranked ? chunk_of_rank[r] : r;
        for (uint64_t e = doc_off[d]; e < doc_off[d + 1]; ++e) {
            const size_t slot = use_dense ? (size_t)(dense[tokens[e]] - 1) : (size_t)sparse_slot[tokens[e]];
            x.post[cur[slot]++] = Posting{(uint32_t)r, weight_bits(weights[e])};
        }
    }
    return x;
}

// cqs_hip_sparse_index_create_inverted's arrays from the reference's map (token -> [(chunk, weight)] in push order), the
// lists having passed check_csr.  false: a key given twice (a map has each key once).
inline bool from_inverted(const uint32_t* token_ids, const uint64_t* list_off, const uint32_t* post_chunks, const float* post_weights,
                          uint64_t n_tokens, uint64_t n, const std::vector<uint32_t>& chunk_of_rank, Built* out) {
    *out = Built();
    // the HashMap's keys in ascending order
    std::vector<uint32_t> order((size_t)n_tokens);
    for (uint64_t t = 0; t < n_tokens; ++t) order[t] = (uint32_t)t;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return token_ids[x] < token_ids[y]; });
    for (uint64_t t = 1; t < n_tokens; ++t)
        if (token_ids[order[t]] == token_ids[order[t - 1]]) return false;
    const bool ranked = !chunk_of_rank.empty();
    std::vector<uint32_t> rank_of;                          // chunk -> position
    if (ranked) {
        rank_of.resize((size_t)n);
        for (uint64_t r = 0; r < n; ++r) rank_of[chunk_of_rank[r]] = (uint32_t)r;
    }
    std::vector<Posting>& post = out->post;
    post.reserve((size_t)(n_tokens ? list_off[n_tokens] : 0));
    out->off.push_back(0);
    for (uint64_t t = 0; t < n_tokens; ++t) {
        const uint32_t src = order[t];
        const size_t first = post.size();
        bool ascending = true;
        for (uint64_t e = list_off[src]; e < list_off[src + 1]; ++e) {
            const uint32_t c = post_chunks[e];
            if (c >= n) continue;                           // the search skips such a posting (index.rs:252): it never scores
            const uint32_t pos = ranked ? rank_of[c] : c;
            if (post.size() > first && pos < post.back().x) ascending = false;
            post.push_back(Posting{pos, weight_bits(post_weights[e])});
        }
        if (post.size() == first) continue;                 // nothing usable under this token: no list
        // ascending positions; postings of ONE chunk keep their order (the only order the sums depend on)
        if (!ascending) std::stable_sort(post.begin() + (ptrdiff_t)first, post.end(), [](const Posting& x, const Posting& y) { return x.x < y.x; });
        out->tok.push_back(token_ids[src]);
        out->off.push_back(post.size());
    }
    return true;
}

// The range directories of the lists that sparse_plan_directories gave one: dir[r] = postings of the list below position
// r * rw, r = 0 .. n_pad / rw.
inline void fill_directories(const Posting* post, const std::vector<uint64_t>& off, const std::vector<uint64_t>& dir_off,
                             const cqs::SparseGeometry& geo, std::vector<uint32_t>* dirs) {
    const uint64_t R1 = (uint64_t)(geo.n_pad / geo.rw) + 1;
    uint64_t used = 0;
    for (const uint64_t d : dir_off)
        if (d != cqs::kNoDir) used = std::max(used, d + R1);
    dirs->assign((size_t)used, 0u);
    for (size_t t = 0; t < dir_off.size(); ++t) {
        if (dir_off[t] == cqs::kNoDir) continue;
        const Posting* const pl = post + off[t];
        const uint32_t len = (uint32_t)(off[t + 1] - off[t]);
        uint32_t* const d = dirs->data() + dir_off[t];
        uint32_t pos = 0;
        for (uint64_t r = 0; r < R1; ++r) {
            const uint64_t edge = r * geo.rw;
            while (pos < len && pl[pos].x < edge) ++pos;
            d[r] = pos;
        }
    }
}

// A batch of b queries as the search entry points take it: the terms of query q are q_tokens / q_weights
// [q_off[q], q_off[q + 1]).  *why continues "sparse search: ".
inline bool check_queries(const uint64_t* q_off, const uint32_t* q_tokens, const float* q_weights, uint32_t b, const char** why) {
    if (b > cqs::kSparseMaxBatch) { *why = "more than 64 queries in a batch"; return false; }
    for (uint32_t q = 0; q < b; ++q) {
        if (q_off[q + 1] < q_off[q]) { *why = "query offsets not ascending"; return false; }
        if (q_off[q + 1] - q_off[q] > cqs::kMaxTerms) { *why = "too many query terms"; return false; }
    }
    if (q_off[b] - q_off[0] && (!q_tokens || !q_weights)) { *why = "null query"; return false; }
    return true;
}

// Resolves the terms of a checked batch (`self.postings.get(&token_id)`, index.rs:249): a token without a list scores
// nothing.  terms[qoff[q] .. qoff[q + 1]) are query q's, qoff[b] all of them (at most q_off[b] - q_off[0]: the caller's
// arrays hold that many); *touched = the postings they name.
inline bool resolve_terms(const std::vector<uint32_t>& tok, const std::vector<uint64_t>& off, const std::vector<uint64_t>& dir_off,
                          const uint64_t* q_off, const uint32_t* q_tokens, const float* q_weights, uint32_t b, cqs::SparseTerm* terms,
                          uint32_t* qoff, uint64_t* touched, const char** why) {
    uint32_t nt = 0;
    *touched = 0;
    for (uint32_t q = 0; q < b; ++q) {
        qoff[q] = nt;
        for (uint64_t i = q_off[q]; i < q_off[q + 1]; ++i) {
            if (weight_bits(q_weights[i]) == cqs::kUnscored) { *why = "reserved NaN payload in a query weight"; return false; }
            const auto it = std::lower_bound(tok.begin(), tok.end(), q_tokens[i]);
            if (it == tok.end() || *it != q_tokens[i]) continue;
            const size_t slot = (size_t)(it - tok.begin());
            const uint64_t len = off[slot + 1] - off[slot];
            if (len == 0) continue;
            if (len > 0xFFFFFFFFull) { *why = "posting list longer than 2^32"; return false; }
            terms[nt].start = off[slot];
            terms[nt].dir = dir_off[slot];
            terms[nt].len = (uint32_t)len;
            terms[nt].w = q_weights[i];
            ++nt;
            *touched += len;
        }
    }
    qoff[b] = nt;
    return true;
}

}  // namespace cqs_sparse_build
