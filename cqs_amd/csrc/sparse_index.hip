// sparse_index.hip — the SPLADE sparse retrieval leg on gfx950: `SpladeIndex` (src/splade/index.rs:177-306) behind the C ABI
// (include/cqs_hip.h, "sparse index" section).
//
// The reference keeps `postings: HashMap<u32, Vec<(usize, f32)>>` (token -> [(chunk_index, weight)], chunk order) and, per
// query, walks the posting list of every query term IN QUERY ORDER adding `query_weight * doc_weight` into a
// `HashMap<usize, f32>` (index.rs:248-258), then pushes every scored chunk through `BoundedScoreHeap` (:265-281).
//
// HBM layout here: ONE array of 8-byte postings {chunk, weight bits}, the lists of all tokens back to back, each list in
// ascending chunk order (= the reference's push order); the token -> (start, length) table stays on the host (a query
// names a few dozen tokens).  "chunk" is the chunk's RANK in ascending id order when the caller gives `id_rank`, so that
// the select's (score desc, position asc) order is BoundedScoreHeap's (score desc, id asc).
//
// One launch scores a query (sparse_accumulate_kernel; its comment has the details): every WAVE owns a contiguous range of
// chunks with their scores in LDS, finds its slice of each query term's list in the list's range directory (built at
// create: where the list crosses every range boundary) and streams the slices term after term, 64 postings per step, adding
// `s = s + qw * dw` with separate f32 multiply and add - every chunk's sum is built in exactly the reference's order, so
// the scores are bit-identical, not "close".  No global atomics, no barriers.  Bound by the touched postings' bytes (8 B
// each) + the score row (4 B per chunk); the exact top-k is the dense index's select_finish_kernel over that score row and
// its 64-chunk maxima, with bins laid over the row's own range of maxima (scan_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "scan_kernels.h"
#include "sparse_build_host.h"
#include "sparse_internal.h"
#include "tags_kernel.h"

namespace cqs {

constexpr size_t kQoffBytes = ((kSparseMaxBatch + 1) * 4 + 15) / 16 * 16;   // the offsets' share of the query block (terms follow, 16-byte aligned)

__device__ __forceinline__ uint32_t lower_bound_chunk(const uint2* __restrict__ p, uint32_t a, uint32_t b, uint32_t c) {
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (p[m].x < c) a = m + 1u; else b = m;
    }
    return a;
}

// (Round 4, first two forms of this file: (1) every wave bisecting every term's list and walking the terms one after the
// other - one dependent memory round trip per term and wave, 126 us at 64 terms; (2) a `sparse_slice_kernel` in front that
// walked the touched postings once and wrote where each list crosses the wave ranges into a [range][term] table - 12 us
// for the extra launch, the postings read twice (the table term-major instead: that launch 11.9 -> 10.0 us, the scoring
// launch 11.4 -> 14.2).  Now the crossings are precomputed at build time: the range directory.  Also tried on top of it and
// dropped: fetching the slices of 4 x 64 terms together (200 terms: 35.7 -> 38.2 us; the LDS rounds bound it, not the trips).)

// ---- the scoring launch ------------------------------------------------------------------------------------------------
// A wave owns `rw = 1 << sh` chunks and their scores in LDS.  64 terms at a time: lane t reads its term's slice - two
// adjacent entries of the list's range directory (dir[r] = postings of the list with position < r * rw; built once, at
// create), or two bisections for a list too short to have one - a wave
// prefix sum lays the slices end to end (term order, inside a term posting order = the order the reference adds in), and the
// wave streams that sequence 64 postings per step - every lane finds its term by a search over the 64 running counts in
// LDS, so all lanes carry a posting whatever the slices' lengths, and the loads of one step do not wait for the sums of the
// step before.  Two postings of a step may name the same chunk (different terms, or a token a document lists twice): each
// pending lane posts its lane number into claim[chunk] with an LDS minimum, the lowest lane (= the earlier posting) adds
// and clears the claim, the others go round again.  No barriers, no global atomics.
constexpr int kSpUnroll = 4;
// dynamic LDS per wave: rw scores + rw claims + 64 x (count, address lo, address hi, weight)
__host__ __device__ constexpr uint32_t sparse_wave_lds_words(uint32_t rw) { return 2u * rw + 4u * 64u; }

__global__ __launch_bounds__(256) void sparse_accumulate_kernel(const uint2* __restrict__ post, const SparseTerm* __restrict__ terms_all,
                                                                const uint32_t* __restrict__ q_term_off /*[queries + 1]*/, const uint32_t* __restrict__ dir,
                                                                uint32_t n, uint32_t n_pad, uint32_t sh,
                                                                const uint32_t* __restrict__ keep, const uint32_t* __restrict__ chunk_of_rank,
                                                                float* __restrict__ scores, float* __restrict__ gmax,
                                                                uint64_t* __restrict__ gaux, uint32_t group16) {
    extern __shared__ uint32_t sp_lds[];
    // blockIdx.y = the query of a batch: its terms, its score row, its maxima
    const SparseTerm* const terms = terms_all + q_term_off[blockIdx.y];
    const uint32_t n_terms = q_term_off[blockIdx.y + 1u] - q_term_off[blockIdx.y];
    scores += (size_t)blockIdx.y * n_pad;
    gmax += (size_t)blockIdx.y * (group16 ? n_pad >> 4 : n_pad >> 6);
    gaux += (size_t)blockIdx.y * (group16 ? n_pad >> 4 : n_pad >> 6);
    const uint32_t rw = 1u << sh;
    const int lane = threadIdx.x & 63;
    const uint32_t wid = threadIdx.x >> 6;
    const uint32_t range = blockIdx.x * 4u + wid;
    const uint32_t c0 = range << sh;
    if (c0 >= n_pad) return;                              // (wave-uniform; no barrier anywhere in this kernel)
    uint32_t* const my = sp_lds + wid * sparse_wave_lds_words(rw);
    uint32_t* const claim = my + rw;
    uint32_t* const t_cum = claim + rw;                   // [64] postings of this group's terms before term j (in this range)
    uint32_t* const t_alo = t_cum + 64;                   // [64] address of the slice's first posting, low / high word
    uint32_t* const t_ahi = t_alo + 64;
    uint32_t* const t_w = t_ahi + 64;
    for (uint32_t i = lane; i < rw; i += 64u) { my[i] = kUnscored; claim[i] = 0xFFFFFFFFu; }

    for (uint32_t t0 = 0; t0 < n_terms; t0 += 64u) {
        uint32_t len = 0u;
        unsigned long long addr = 0ull;
        float w = 0.f;
        if (t0 + (uint32_t)lane < n_terms) {
            const SparseTerm tm = terms[t0 + lane];
            uint32_t lo, hi;
            if (tm.dir != kNoDir) {
                lo = dir[tm.dir + range];
                hi = dir[tm.dir + range + 1u];
            } else {
                const uint2* const p = post + tm.start;
                lo = lower_bound_chunk(p, 0u, tm.len, c0);
                uint32_t b = tm.len;
                if (lo + rw < b && p[lo + rw].x >= c0 + rw) b = lo + rw;   // the usual case: no more than one posting per chunk
                hi = lower_bound_chunk(p, lo, b, c0 + rw);
            }
            len = hi - lo;
            addr = tm.start + lo;
            w = tm.w;
        }
        uint32_t cum = len;                               // inclusive wave prefix sum
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(cum, off, 64);
            if (lane >= off) cum += v;
        }
        const uint32_t total = __builtin_amdgcn_readlane(cum, 63);
        if (total == 0u) continue;
        t_cum[lane] = cum - len;
        t_alo[lane] = (uint32_t)addr;
        t_ahi[lane] = (uint32_t)(addr >> 32);
        t_w[lane] = __builtin_bit_cast(uint32_t, w);
        for (uint32_t g0 = 0; g0 < total; g0 += 64u * kSpUnroll) {
            uint2 e[kSpUnroll];
            float prod[kSpUnroll];
            bool pend[kSpUnroll];
#pragma unroll
            for (int u = 0; u < kSpUnroll; ++u) {
                const uint32_t g = g0 + 64u * u + (uint32_t)lane;
                pend[u] = g < total;
                e[u] = make_uint2(c0, 0u);
                prod[u] = 0.f;
                if (pend[u]) {
                    uint32_t a = 0u, b = 64u;             // the last term whose running count <= g
#pragma unroll
                    for (int step = 0; step < 6; ++step) {
                        const uint32_t m = (a + b) >> 1;
                        if (t_cum[m] <= g) a = m; else b = m;
                    }
                    const unsigned long long at = ((unsigned long long)t_ahi[a] << 32 | t_alo[a]) + (g - t_cum[a]);
#if defined(CQS_SP_ABLATE_NOLOAD)      // timing experiment (wrong results): no posting is read
                    e[u] = make_uint2(c0 + ((uint32_t)at & (rw - 1u)), 0x3f800000u);
#else
                    e[u] = post[at];
#endif
                    prod[u] = __fmul_rn(__builtin_bit_cast(float, t_w[a]), __builtin_bit_cast(float, e[u].y));
                }
            }
#pragma unroll
            for (int u = 0; u < kSpUnroll; ++u) {
                if (g0 + 64u * u >= total) break;         // (wave-uniform)
                const uint32_t at = e[u].x - c0;
                bool pending = pend[u];
#if defined(CQS_SP_ABLATE_NORMW)       // timing experiment (wrong results): the loads alone
                if (pending && prod[u] == 12345.678f) my[at] = 1u;
                pending = false;
#endif
                while (__builtin_amdgcn_ballot_w64(pending) != 0ull) {
                    // (compiler barriers: the other lanes' LDS stores are invisible to the single-thread view the optimiser
                    // reasons in - no load of a score or a claim may move across a round)
                    asm volatile("" ::: "memory");
                    if (pending) atomicMin(&claim[at], (uint32_t)lane);
                    asm volatile("" ::: "memory");
                    if (pending && *(volatile uint32_t*)&claim[at] == (uint32_t)lane) {
                        const uint32_t s = *(volatile uint32_t*)&my[at];
                        const uint32_t sum = __builtin_bit_cast(uint32_t, __fadd_rn(s == kUnscored ? 0.f : __builtin_bit_cast(float, s), prod[u]));
                        // a NaN sum that happens to carry the marker's bits (the sign of a NaN result is the hardware's
                        // choice) is stored as the canonical NaN: still NaN for every later add, still dropped at the end
                        *(volatile uint32_t*)&my[at] = sum == kUnscored ? 0x7FC00000u : sum;
                        *(volatile uint32_t*)&claim[at] = 0xFFFFFFFFu;
                        pending = false;
                    }
                    asm volatile("" ::: "memory");
                }
            }
        }
    }
    // the score row + the maxima of its 64-chunk groups (what select_finish_kernel reads); a chunk that was never scored,
    // is filtered out, or whose score is not finite (BoundedScoreHeap refuses it, candidate.rs:245-247) = -inf
    for (uint32_t i = lane; i < rw; i += 64u) {
        const uint32_t r = c0 + i;
        const uint32_t s = my[i];
        float v = __builtin_bit_cast(float, s);
        bool ok = r < n && s != kUnscored && __builtin_isfinite(v);
        if (ok && keep) {
            const uint32_t c = chunk_of_rank ? chunk_of_rank[r] : r;
            ok = (keep[c >> 5] >> (c & 31u)) & 1u;
        }
        v = ok ? v : -INFINITY;
        scores[r] = v;
        float m = cqs::wave_max16(v);                     // (DPP: `__shfl_xor` is a ds_bpermute round trip per step on gfx950)
        // beside each maximum: the lane it sits in and the group's runner-up (select_finish_kernel, round 5: a group whose
        // runner-up misses the threshold contributes its maximum without its scores being read back)
        if (group16) {                                    // small indexes: maxima of 16 chunks (fewer than k groups of 64 would
            if ((lane & 15) == 0) gmax[r >> 4] = m;       // make every score a candidate and send the select down its radix path)
            const uint32_t seg = (uint32_t)(__ballot(v == m) >> (lane & 48)) & 0xFFFFu;   // my 16 lanes (no scored chunk: m = -inf, all match)
            const uint32_t arg = (uint32_t)__builtin_ctz(seg);
            const float sec = cqs::wave_max16(((uint32_t)(lane & 15) == arg) ? -INFINITY : v);
            if ((lane & 15) == 0) gaux[r >> 4] = ((uint64_t)arg << 32) | (uint64_t)__builtin_bit_cast(uint32_t, sec);
        } else {
            m = cqs::wave_max64(v);
            if (lane == 0) gmax[r >> 6] = m;
            const uint32_t arg = (uint32_t)__builtin_ctzll(__ballot(v == m));
            const float sec = cqs::wave_max64(((uint32_t)lane == arg) ? -INFINITY : v);
            if (lane == 0) gaux[r >> 6] = ((uint64_t)arg << 32) | (uint64_t)__builtin_bit_cast(uint32_t, sec);
        }
    }
}

}  // namespace cqs

using cqs::kMaxTerms;
using cqs::kSparseMaxBatch;
using cqs::kQoffBytes;
using cqs::kUnscored;
using cqs::sparse_accumulate_kernel;
using cqs::sparse_wave_lds_words;
using cqs::SparseTerm;

namespace {

using cqs_sparse::sfail;

int32_t ensure_terms(cqs_hip_sparse_index* s, uint32_t t) {
    if (t <= s->terms_cap) return CQS_HIP_OK;
    const uint32_t cap = std::max(256u, t + t / 2u);
    // ONE block per side: [first-term offsets of the batch's queries: kQoffBytes][terms] - a search is one H2D copy
    // (round 4 sent the offsets and the terms in two)
    if (s->d_qoff) { (void)hipFree(s->d_qoff); s->d_qoff = nullptr; s->d_terms = nullptr; }
    if (s->h_qoff) { (void)hipHostFree(s->h_qoff); s->h_qoff = nullptr; s->h_terms = nullptr; }
    s->terms_cap = 0;
    S_TRY(s, hipMalloc((void**)&s->d_qoff, kQoffBytes + (size_t)cap * sizeof(SparseTerm)));
    S_TRY(s, hipHostMalloc((void**)&s->h_qoff, kQoffBytes + (size_t)cap * sizeof(SparseTerm), hipHostMallocDefault));
    s->d_terms = (SparseTerm*)((char*)s->d_qoff + kQoffBytes);
    s->h_terms = (SparseTerm*)((char*)s->h_qoff + kQoffBytes);
    s->terms_cap = cap;
    return CQS_HIP_OK;
}

}  // namespace

namespace cqs_sparse {

// score rows, maxima and result keys for `b` queries (grown on demand; one query's worth exists from create on)
int32_t ensure_batch(cqs_hip_sparse_index* s, uint32_t b) {
    if (b <= s->b_cap) return CQS_HIP_OK;
    for (void** p : {(void**)&s->d_scores, (void**)&s->d_gmax, (void**)&s->d_out_keys, (void**)&s->d_out_count})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (s->h_out_keys) { (void)hipHostFree(s->h_out_keys); s->h_out_keys = nullptr; s->h_out_keys_dev = nullptr; }
    s->b_cap = 0;
    const size_t groups = s->n_pad / (s->group16 ? 16u : 64u);
    S_TRY(s, hipMalloc((void**)&s->d_scores, (size_t)b * s->n_pad * 4));
    S_TRY(s, hipMalloc((void**)&s->d_gmax, (size_t)b * groups * 12));   // maxima, then (argmax, runner-up) pairs (groups % 4 == 0: 8-byte aligned)
    S_TRY(s, hipMalloc((void**)&s->d_out_keys, (size_t)b * cqs::kMaxK * 8));
    S_TRY(s, hipMalloc((void**)&s->d_out_count, (size_t)b * 4));
    // keys [b][k] then the b counts, in one pinned + device-visible block: the select writes there
    S_TRY(s, hipHostMalloc((void**)&s->h_out_keys, (size_t)b * (cqs::kMaxK + 1) * 8, hipHostMallocMapped));
    if (hipHostGetDevicePointer((void**)&s->h_out_keys_dev, s->h_out_keys, 0) != hipSuccess) s->h_out_keys_dev = nullptr;
    s->b_cap = b;
    return CQS_HIP_OK;
}

int32_t search_locked(cqs_hip_sparse_index* s, const uint64_t* q_off, const uint32_t* q_tokens, const float* q_weights, uint32_t b,
                      uint32_t k, const uint32_t* keep_bitset, uint64_t* out_chunks, float* out_scores, uint32_t* out_counts,
                      const uint32_t* allow) {
    for (uint32_t q = 0; q < b; ++q) out_counts[q] = 0;
    if (s->poisoned) return CQS_HIP_ERR_POISONED;
    if (k > cqs::kMaxK) return sfail(s, CQS_HIP_ERR_INVALID, "sparse search: k > CQS_HIP_MAX_K");
    const char* why = "";
    if (!cqs_sparse_build::check_queries(q_off, q_tokens, q_weights, b, &why)) return sfail(s, CQS_HIP_ERR_INVALID, std::string("sparse search: ") + why);
    const uint64_t total_terms = q_off[b] - q_off[0];
    s->last_ms = 0.f;
    s->last_touched = 0;
    if (total_terms == 0 || s->n == 0 || k == 0) return CQS_HIP_OK;    // index.rs:237-239; BoundedScoreHeap::new(0) keeps nothing
    if (!out_chunks || !out_scores) return sfail(s, CQS_HIP_ERR_INVALID, "sparse search: null output");
    S_TRY(s, hipSetDevice(s->device));
    int32_t rc = ensure_terms(s, (uint32_t)total_terms);
    if (rc != CQS_HIP_OK) return rc;
    if ((rc = ensure_batch(s, b)) != CQS_HIP_OK) return rc;
    // resolve the terms, straight into the pinned block the copy below sends
    uint64_t touched = 0;
    if (!cqs_sparse_build::resolve_terms(s->tok, s->off, s->dir_off, q_off, q_tokens, q_weights, b, s->h_terms, s->h_qoff, &touched, &why))
        return sfail(s, CQS_HIP_ERR_INVALID, std::string("sparse search: ") + why);
    const uint32_t nt = s->h_qoff[b];
    if (nt == 0) return CQS_HIP_OK;
    s->last_touched = touched;
    hipStream_t st = s->stream;
    S_TRY(s, hipMemcpyAsync(s->d_qoff, s->h_qoff, kQoffBytes + (size_t)nt * sizeof(SparseTerm), hipMemcpyHostToDevice, st));
    const uint32_t* d_keep = nullptr;
    if (keep_bitset) {
        const size_t words = (size_t)((s->n + 31) / 32);
        memcpy(s->h_keep, keep_bitset, words * 4);
        S_TRY(s, hipMemcpyAsync(s->d_keep, s->h_keep, words * 4, hipMemcpyHostToDevice, st));
        d_keep = s->d_keep;
    } else if (allow) {                                       // (n >= 1; d_keep holds n_pad / 32 >= ceil(n / 32) words)
        S_TRY(s, cqs::launch_tags_keep(s->d_tags, (uint32_t)s->n, allow, s->d_keep, nullptr, st));
        d_keep = s->d_keep;
    }
    const uint32_t waves = s->n_pad / s->rw;
    // the scoring launch is bracketed by events only once somebody has asked for its time (cqs_hip_sparse_index_last_search
    // with a non-NULL accumulate_ms): two event records are ~4 us of an 80 us call
    const bool timed = s->want_timing.load(std::memory_order_relaxed);
    if (timed) S_TRY(s, hipEventRecord(s->ev0, st));
    hipLaunchKernelGGL(sparse_accumulate_kernel, dim3((waves + 3u) / 4u, b), dim3(256), (size_t)4 * sparse_wave_lds_words(s->rw) * 4, st,
                       s->d_post, s->d_terms, s->d_qoff, s->d_dir, (uint32_t)s->n, s->n_pad, s->sh, d_keep,
                       s->ranked ? s->d_chunk_of_rank : nullptr, s->d_scores, s->d_gmax,
                       (uint64_t*)(s->d_gmax + (size_t)s->b_cap * (s->n_pad / (s->group16 ? 16u : 64u))), s->group16 ? 1u : 0u);
    S_TRY(s, hipGetLastError());
    if (timed) S_TRY(s, hipEventRecord(s->ev1, st));
    cqs::ScanArgs a{};
    a.n = (uint32_t)s->n;
    a.n_pad = s->n_pad;
    a.b = b;
    a.scores = s->d_scores;
    a.gmax = s->d_gmax;
    a.gaux = (uint64_t*)(s->d_gmax + (size_t)s->b_cap * (s->n_pad / (s->group16 ? 16u : 64u)));
    a.gemv_only = true;                                   // (not the matrix-core scan: the select reads gaux)
    a.tiers = s->group16 ? cqs::TaskTiers{0u, 0u, s->n_pad / 16u} : cqs::TaskTiers{s->n_pad / 64u, 0u, 0u};
    a.k = k;
    a.linear_bins = false;
    a.range_bins = true;
    a.work = s->d_work;
    a.n_cu = s->n_cu;
    a.dbg = s->d_dbg;
    uint32_t* const h_counts = (uint32_t*)(s->h_out_keys + (size_t)s->b_cap * cqs::kMaxK);     // after the key block
    if (s->h_out_keys_dev) {
        S_TRY(s, cqs::launch_select(a, 0u, s->h_out_keys_dev, (uint32_t*)(s->h_out_keys_dev + (size_t)s->b_cap * cqs::kMaxK), st));
    } else {
        S_TRY(s, cqs::launch_select(a, 0u, s->d_out_keys, s->d_out_count, st));
        S_TRY(s, hipMemcpyAsync(s->h_out_keys, s->d_out_keys, (size_t)b * k * 8, hipMemcpyDeviceToHost, st));
        S_TRY(s, hipMemcpyAsync(h_counts, s->d_out_count, (size_t)b * 4, hipMemcpyDeviceToHost, st));
    }
    S_TRY(s, hipStreamSynchronize(st));
    if (timed) (void)hipEventElapsedTime(&s->last_ms, s->ev0, s->ev1);
    if (s->d_dbg) {
        unsigned long long h[16];
        if (hipMemcpy(h, s->d_dbg, sizeof h, hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "[cqs_hip sparse] select phases (us): zero+range %.2f | histogram %.2f | decide %.2f | groups %.2f | gather %.2f | sort %.2f | out %.2f | groups=%llu candidates=%llu\n",
                    0.0, (h[1] - h[0]) * 0.01, (h[2] - h[1]) * 0.01, (h[3] - h[2]) * 0.01, (h[4] - h[3]) * 0.01, (h[5] - h[4]) * 0.01,
                    (h[6] - h[5]) * 0.01, h[8], h[9]);
    }
    for (uint32_t q = 0; q < b; ++q) {                     // the select packs query q's keys at [q * k, (q + 1) * k)
        uint32_t cnt = h_counts[q];
        if (cnt > k) cnt = k;
        uint64_t* const oc = out_chunks + (size_t)q * k;
        cqs_hip_unpack_keys(s->h_out_keys + (size_t)q * k, cnt, oc, out_scores + (size_t)q * k);
        if (s->ranked)
            for (uint32_t i = 0; i < cnt; ++i) oc[i] = s->chunk_of_rank[(size_t)oc[i]];
        out_counts[q] = cnt;
    }
    return CQS_HIP_OK;
}

}  // namespace cqs_sparse

using cqs_sparse::search_locked;

extern "C" {

namespace {

// ---- the combining queue (combine_queue.h) over the batched launches -----------------------------------------
// The reference's daemon calls `search_with_filter(&self)` from one thread per client on a shared index
// (src/cli/batch/view.rs:1621, src/search/query.rs:898-901).  An unfiltered single-query call parks its request; whoever
// leads next gathers the parked requests with the same k (oldest first, up to 64), takes the device mutex and runs them as
// one batch - every caller gets exactly the bits its own call would have produced (the kernels treat the queries of a
// batch independently).  Requests are validated BEFORE they park, so a batch can only fail for the device.
int32_t sparse_combine_search(cqs_hip_sparse_index* s, cqs_sparse_req& r) {
    const auto same_k = [](const cqs_sparse_req* a, const cqs_sparse_req* b) { return a->k == b->k; };
    return s->cq.search(r, same_k, [s](cqs_sparse_req* const* batch, uint32_t nb) {
        std::lock_guard<std::mutex> dev(s->mu);            // the device, for the batch alone
        int32_t rc = CQS_HIP_OK;
        const uint32_t k = batch[0]->k;
        std::vector<uint32_t> counts;
        std::vector<uint64_t> chunks;
        std::vector<float> scores;
        try {
            std::vector<uint64_t> q_off(nb + 1, 0);
            for (uint32_t i = 0; i < nb; ++i) q_off[i + 1] = q_off[i] + batch[i]->n_terms;
            std::vector<uint32_t> toks((size_t)q_off[nb]);
            std::vector<float> wts((size_t)q_off[nb]);
            for (uint32_t i = 0; i < nb; ++i) {
                if (batch[i]->n_terms == 0) continue;
                memcpy(toks.data() + q_off[i], batch[i]->q_tokens, (size_t)batch[i]->n_terms * 4);
                memcpy(wts.data() + q_off[i], batch[i]->q_weights, (size_t)batch[i]->n_terms * 4);
            }
            counts.assign(nb, 0u);
            chunks.resize((size_t)nb * k);
            scores.resize((size_t)nb * k);
            rc = search_locked(s, q_off.data(), toks.data(), wts.data(), nb, k, nullptr, chunks.data(), scores.data(), counts.data());
        } catch (const std::bad_alloc&) {
            rc = sfail(s, CQS_HIP_ERR_NOMEM, "sparse search: out of host memory");
        } catch (...) {
            rc = sfail(s, CQS_HIP_ERR_INVALID, "sparse search: unexpected C++ exception");
        }
        s->stat_passes.fetch_add(1, std::memory_order_relaxed);
        s->stat_queries.fetch_add(nb, std::memory_order_relaxed);
        if (rc == CQS_HIP_OK)
            for (uint32_t i = 0; i < nb; ++i) {
                memcpy(batch[i]->out_chunks, chunks.data() + (size_t)i * k, (size_t)counts[i] * 8);
                memcpy(batch[i]->out_scores, scores.data() + (size_t)i * k, (size_t)counts[i] * 4);
                *batch[i]->out_count = counts[i];
            }
        return cqs_combine::Outcome{rc, s->poisoned.load(std::memory_order_acquire)};
    });
}

}  // namespace

int32_t cqs_hip_sparse_index_search(cqs_hip_sparse_index* s, const uint32_t* q_tokens, const float* q_weights, uint32_t n_terms,
                                    uint32_t k, const uint32_t* keep_bitset, uint64_t* out_chunks, float* out_scores,
                                    uint32_t* out_count) CQS_ABI_TRY {
    if (!s) return CQS_HIP_ERR_INVALID;
    // One unfiltered query with its arguments in order: the combining queue.  Everything a batch could refuse for ONE of
    // its members is checked here, before the request parks.
    if (s->combine && !keep_bitset && out_count && out_chunks && out_scores && k >= 1 && k <= cqs::kMaxK && n_terms >= 1 &&
        n_terms <= kMaxTerms && q_tokens && q_weights && s->n != 0) {
        if (s->poisoned.load(std::memory_order_acquire)) { *out_count = 0; return CQS_HIP_ERR_POISONED; }
        bool reserved = false;
        for (uint32_t i = 0; i < n_terms; ++i) {
            uint32_t bits;
            memcpy(&bits, &q_weights[i], 4);
            reserved |= bits == kUnscored;
        }
        if (!reserved) {
            *out_count = 0;
            cqs_sparse_req r{q_tokens, q_weights, n_terms, k, out_chunks, out_scores, out_count};
            return sparse_combine_search(s, r);
        }
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (!out_count) return sfail(s, CQS_HIP_ERR_INVALID, "sparse search: null out_count");
    const uint64_t q_off[2] = {0, n_terms};
    return search_locked(s, q_off, q_tokens, q_weights, 1u, k, keep_bitset, out_chunks, out_scores, out_count);
} CQS_ABI_CATCH(s)

int32_t cqs_hip_sparse_index_search_batch(cqs_hip_sparse_index* s, const uint64_t* q_off, const uint32_t* q_tokens,
                                          const float* q_weights, uint32_t b, uint32_t k, const uint32_t* keep_bitset,
                                          uint64_t* out_chunks, float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    if (!s) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(s->mu);
    if (b == 0) return CQS_HIP_OK;
    if (!q_off || !out_counts) return sfail(s, CQS_HIP_ERR_INVALID, "sparse search: null offsets / counts");
    return search_locked(s, q_off, q_tokens, q_weights, b, k, keep_bitset, out_chunks, out_scores, out_counts);
} CQS_ABI_CATCH(s)

void cqs_hip_sparse_index_combine_stats(const cqs_hip_sparse_index* s, uint64_t* passes, uint64_t* queries) CQS_ABI_TRY {
    if (passes) *passes = s ? s->stat_passes.load(std::memory_order_relaxed) : 0;
    if (queries) *queries = s ? s->stat_queries.load(std::memory_order_relaxed) : 0;
} CQS_ABI_CATCH_VOID

int32_t cqs_hip_sparse_index_last_search(const cqs_hip_sparse_index* s, float* accumulate_ms, uint64_t* touched_postings) CQS_ABI_TRY {
    if (!s) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(const_cast<cqs_hip_sparse_index*>(s)->mu);
    if (accumulate_ms) {
        *accumulate_ms = s->last_ms;             // 0 for a search that ran before the first request
        const_cast<cqs_hip_sparse_index*>(s)->want_timing.store(true, std::memory_order_relaxed);
    }
    if (touched_postings) *touched_postings = s->last_touched;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_VAL(CQS_HIP_ERR_INVALID)

// Diagnostic (not in the header): combine_queue.h's client storm over the public single-query entry point (query q's
// terms: [q_off[q], q_off[q + 1])); results land in the query's own output slot.  Returns the wall time in seconds, < 0 on a failed call.  What bench.py's Python threads cannot
// show behind the interpreter lock.
double cqs_hip_debug_sparse_client_storm(cqs_hip_sparse_index* s, const uint64_t* q_off, const uint32_t* q_tokens, const float* q_weights,
                                         uint32_t n_queries, uint32_t k, uint32_t n_threads, uint32_t per_thread,
                                         uint64_t* out_chunks, float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    if (!s || !q_off || !q_tokens || !q_weights || !n_queries || !n_threads || !out_chunks || !out_scores || !out_counts) return -1.0;
    return cqs_combine::client_storm(n_threads, per_thread, n_queries, [=](uint32_t qi) {
        return cqs_hip_sparse_index_search(s, q_tokens + q_off[qi], q_weights + q_off[qi], (uint32_t)(q_off[qi + 1] - q_off[qi]), k, nullptr,
                                           out_chunks + (size_t)qi * k, out_scores + (size_t)qi * k, out_counts + qi);
    });
} CQS_ABI_CATCH_VAL(-1.0)

}  // extern "C"
