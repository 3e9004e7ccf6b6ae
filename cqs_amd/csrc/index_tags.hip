// index_tags.hip — row tags on the device: one u32 per row beside the corpus, and the filtered search that
// sends 128 bytes of allowed sets instead of a keep-bitset of n / 8 bytes.  The predicate the reference sends with every
// filtered and hybrid query - chunk type in / not in a set, language in a set, src/search/query.rs:860-900 - is a function
// of two small integers per chunk; its host loop over all n chunk ids (src/cagra.rs:747-757) becomes tags_keep_kernel,
// which writes the bitset the scans already read.  The scan, select and shadow kernels are untouched: search_tagged hands
// the device bitset to the host search's block runner (index.hip) where the staged host bitset would go, so the answer is
// the bytes of cqs_hip_index_search with the host bitset of the same predicate.  A block of queries with a filter EACH
// (search_tagged_multi, and the combining queue's blocks of single tagged callers; §3.14a) gets its bitsets from ONE pass
// over the tags, tags_keep_multi_kernel, written straight into the handle's bitset table, and then runs as the blocks of
// callers with a host bitset run (index.hip, answer_block).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "abi_guard.h"
#include "roctx.h"
#include "index_internal.h"
#include "search_host.h"
#include "tags_host.h"
#include "tags_kernel.h"

namespace cqs {

struct TagFilter { uint32_t w[cqs_tags::kAllowWords]; };   // the 128-byte filter, by value in the kernel arguments

// One row per lane, 256 rows per workgroup and step.  The filter goes to LDS once per workgroup (four dynamic-index lookups
// per row); a wave's 64 verdicts are one ballot = two words of the bitset, stored by lanes 0 and 32 (plain vector stores,
// the wave's 64 rows start on a word boundary).  Every lane of every wave reaches the ballot - no early return; a lane at
// or past n contributes 0, so the bits past n in the last word are 0 and a word wholly past n is not written.  The kept
// count is exact: each wave sums its ballots' popcounts, the workgroup adds them in LDS and stores its partial count at
// partials[blockIdx.x] (null: nobody asked); the host sums the <= 2048 partials.  (First form: one global atomicAdd per
// workgroup on one word - 2048 adds on one address made the launch 25.7 us at 1M rows, against about 5 us in-stream for
// the same kernel without a count)  Reads 4 B per row, writes n / 8 B.
__global__ __launch_bounds__(kTagThreads) void tags_keep_kernel(const uint32_t* __restrict__ tags, uint32_t n, TagFilter filter,
                                                                uint32_t* __restrict__ keep, uint32_t* __restrict__ partials) {
    __shared__ uint32_t allow[cqs_tags::kAllowWords];
    __shared__ uint32_t wg_kept;
    if (threadIdx.x < cqs_tags::kAllowWords) allow[threadIdx.x] = filter.w[threadIdx.x];
    if (threadIdx.x == 0) wg_kept = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_tiles = n / kTagThreads + (n % kTagThreads ? 1u : 0u);
    uint32_t kept = 0u;                                    // (wave-uniform)
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t row = tile * kTagThreads + threadIdx.x;        // (tile < n_tiles <= 2^24: no wrap)
        const bool in = row < n;
        const uint32_t tag = in ? tags[row] : 0u;
        const unsigned long long m = __ballot(in && cqs_tags::tag_kept(tag, allow));
        kept += (uint32_t)__popcll(m);
        const uint32_t row0 = row - lane;                  // the wave's first row: a multiple of 64
        if (lane == 0u && row0 < n) keep[row0 >> 5] = (uint32_t)m;
        if (lane == 32u && row < n) keep[row >> 5] = (uint32_t)(m >> 32);
    }
    if (!partials) return;                                 // (uniform over the grid)
    if (lane == 0u && kept) atomicAdd(&wg_kept, kept);
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = wg_kept;
}

hipError_t launch_tags_keep(const uint32_t* d_tags, uint32_t n, const uint32_t* allow, uint32_t* d_keep, uint32_t* d_partials,
                            hipStream_t st) {
    TagFilter f;
    memcpy(f.w, allow, sizeof f.w);
    tags_keep_kernel<<<tags_keep_blocks(n), kTagThreads, 0, st>>>(d_tags, n, f, d_keep, d_partials);
    return hipGetLastError();
}

// Up to 32 filters in one pass over the tags.  The filters arrive transposed (tags_host.h: bit j of
// tbl[field][value] = filter j allows it), 4 KB that go to LDS once per workgroup, so a row's verdicts under ALL the filters
// are four lookups and three ANDs: each tag is read once, whatever f.  A wave takes kTagMultiGroups = 4 consecutive 64-row
// groups per step (256 rows = 8 words of every bitset).  Per filter j (f is wave-uniform) it takes the four ballots of
// bit j; lane j keeps the words of groups 0 and 1, lane j + 32 those of groups 2 and 3, so that a lane ends up with four
// CONSECUTIVE words of table row j: one 16-byte store per lane where that is aligned and wholly below ceil(n / 32), single
// guarded words otherwise (the last step, or a table row that does not start on 16 bytes).  Lanes at or past n contribute
// 0 (bits past n are zero), a word wholly past n is not written, lanes j >= f store nothing (rows >= f stay untouched).
// Counts: a lane popcounts the words it stores; the workgroup adds them per filter in LDS and writes partials[block][j]
// for every j < f - no global atomics (tags_keep_kernel's note above).  Plain vector stores only.
__global__ __launch_bounds__(kTagThreads) void tags_keep_multi_kernel(const uint32_t* __restrict__ tags, uint32_t n,
                                                                      const uint32_t* __restrict__ tbl_g, uint32_t f,
                                                                      uint32_t* __restrict__ tab, uint32_t stride,
                                                                      uint32_t* __restrict__ partials) {
    __shared__ uint32_t tbl[cqs_tags::kTableWords];
    __shared__ uint32_t wg_kept[cqs_tags::kMaxFilters];
    for (uint32_t i = threadIdx.x; i < cqs_tags::kTableWords; i += kTagThreads) tbl[i] = tbl_g[i];
    if (threadIdx.x < cqs_tags::kMaxFilters) wg_kept[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t j = lane & 31u;                         // the filter whose words this lane keeps,
    const bool hi = lane >= 32u;                           // ... groups 0, 1 (lanes 0 .. 31) or 2, 3 (lanes 32 .. 63)
    const uint32_t n_words = n / 32u + (n % 32u ? 1u : 0u);
    const uint32_t n_tiles = n / kTagMultiRows + (n % kTagMultiRows ? 1u : 0u);
    uint32_t kept = 0u;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t row0 = (uint64_t)tile * kTagMultiRows + wave * (64u * kTagMultiGroups);   // the wave's first row: a multiple of 256
        if (row0 >= n) continue;                           // (wave-uniform; the loop holds no barrier)
        uint32_t tag[kTagMultiGroups], v[kTagMultiGroups];
#pragma unroll
        for (uint32_t g = 0; g < kTagMultiGroups; ++g) {
            const uint64_t row = row0 + 64u * g + lane;
            tag[g] = row < n ? tags[row] : 0u;
        }
#pragma unroll
        for (uint32_t g = 0; g < kTagMultiGroups; ++g) {
            const uint64_t row = row0 + 64u * g + lane;
            v[g] = row < n ? cqs_tags::tag_verdicts(tag[g], tbl) : 0u;
        }
        uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
        for (uint32_t jj = 0; jj < f; ++jj) {              // every lane reaches every ballot
            const unsigned long long m0 = __ballot((v[0] >> jj) & 1u), m1 = __ballot((v[1] >> jj) & 1u);
            const unsigned long long m2 = __ballot((v[2] >> jj) & 1u), m3 = __ballot((v[3] >> jj) & 1u);
            if (j == jj) {
                const unsigned long long a = hi ? m2 : m0, b = hi ? m3 : m1;
                w0 = (uint32_t)a; w1 = (uint32_t)(a >> 32); w2 = (uint32_t)b; w3 = (uint32_t)(b >> 32);
            }
        }
        if (j < f) {                                       // (the other lanes' words stayed 0; rows >= f are not touched)
            kept += (uint32_t)(__popc(w0) + __popc(w1) + __popc(w2) + __popc(w3));
            const uint32_t first = (uint32_t)(row0 >> 5) + (hi ? 4u : 0u);  // this lane's four words of table row j
            uint32_t* const p = tab + (size_t)j * stride + first;
            if (first + 4u <= n_words && ((uintptr_t)p & 15u) == 0u) {
                *reinterpret_cast<uint4*>(p) = make_uint4(w0, w1, w2, w3);
            } else {
                if (first < n_words) p[0] = w0;
                if (first + 1u < n_words) p[1] = w1;
                if (first + 2u < n_words) p[2] = w2;
                if (first + 3u < n_words) p[3] = w3;
            }
        }
    }
    if (j < f && kept) atomicAdd(&wg_kept[j], kept);       // (LDS: eight lanes per filter and workgroup)
    __syncthreads();
    if (threadIdx.x < f) partials[(size_t)blockIdx.x * f + threadIdx.x] = wg_kept[threadIdx.x];
}

hipError_t launch_tags_keep_multi(const uint32_t* d_tags, uint32_t n, const uint32_t* d_tbl, uint32_t f, uint32_t* d_tab,
                                  uint32_t stride_words, uint32_t* d_partials, uint32_t max_blocks, hipStream_t st) {
    if (n == 0 || f == 0 || f > cqs_tags::kMaxFilters || stride_words < n / 32u + (n % 32u ? 1u : 0u)) return hipErrorInvalidValue;
    tags_keep_multi_kernel<<<tags_keep_multi_blocks(n, max_blocks), kTagThreads, 0, st>>>(d_tags, n, d_tbl, f, d_tab, stride_words,
                                                                                         d_partials);
    return hipGetLastError();
}

}  // namespace cqs

namespace cqs_idx {

void tags_free(cqs_hip_index* x) {
    hipFree(x->d_tags);
    hipFree(x->d_tag_count);
    hipHostFree(x->h_tag_count);
    hipFree(x->d_tag_tbl);
    hipHostFree(x->h_tag_tbl);
    hipFree(x->d_tag_mcount);
    hipHostFree(x->h_tag_mcount);
    x->d_tags = nullptr; x->d_tag_count = nullptr; x->h_tag_count = nullptr;
    x->d_tag_tbl = nullptr; x->h_tag_tbl = nullptr; x->d_tag_mcount = nullptr; x->h_tag_mcount = nullptr;
    x->tags_cap = 0; x->tagged = 0;
}

void tags_regrow(cqs_hip_index* x) {
    if (!x->d_tags || x->tags_cap >= x->cap_rows) return;
    uint32_t* nd = nullptr;
    hipError_t e = hipMalloc(&nd, (size_t)x->cap_rows * sizeof(uint32_t));
    if (e == hipSuccess && x->tagged) e = hipMemcpyAsync(nd, x->d_tags, (size_t)x->tagged * sizeof(uint32_t), hipMemcpyDeviceToDevice, x->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        hipFree(nd);
        hipFree(x->d_tags);
        x->d_tags = nullptr; x->tags_cap = 0; x->tagged = 0;
        x->last_error = "extend: no memory to regrow the row tags; they are dropped (set_tags again)";
        return;
    }
    hipFree(x->d_tags);
    x->d_tags = nd;
    x->tags_cap = x->cap_rows;
}

// The checks every tagged call makes before anything else, under mu.  OK = a single-device handle, not poisoned, whose
// every row has a tag.  None of the refusals poisons.
int32_t tagged_ready(cqs_hip_index* x, const uint32_t* allow, const char* who) {
    char msg[160];
    if (!allow) { snprintf(msg, sizeof msg, "%s: null allow", who); return fail(x, CQS_HIP_ERR_INVALID, msg); }
    if (x->sh) { snprintf(msg, sizeof msg, "%s: not built for a row-sharded handle", who); return fail(x, CQS_HIP_ERR_INVALID, msg); }
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (x->tagged < x->n) {
        snprintf(msg, sizeof msg, "%s: tags cover %llu of %llu rows", who, (unsigned long long)x->tagged, (unsigned long long)x->n);
        return fail(x, CQS_HIP_ERR_INVALID, msg);
    }
    return CQS_HIP_OK;
}

namespace {

// The filter's bitset over the whole index into x->d_keep on x->stream, and the exact count of kept rows after one small
// wait.  Caller holds mu, has set the device; n >= 1, every row tagged.
int32_t tags_keep_locked(cqs_hip_index* x, const uint32_t* allow, uint64_t* kept) {
    const int32_t rc = ensure_keep(x, (x->n + 31) / 32);
    if (rc != CQS_HIP_OK) return rc;
    if (!x->d_tag_count) HIP_TRY(x, hipMalloc(&x->d_tag_count, cqs::kTagMaxBlocks * sizeof(uint32_t)));
    if (!x->h_tag_count) HIP_TRY(x, hipHostMalloc(&x->h_tag_count, cqs::kTagMaxBlocks * sizeof(uint32_t), hipHostMallocDefault));
    const uint32_t blocks = cqs::tags_keep_blocks((uint32_t)x->n);
    HIP_TRY(x, cqs::launch_tags_keep(x->d_tags, (uint32_t)x->n, allow, x->d_keep, x->d_tag_count, x->stream));
    HIP_TRY(x, hipMemcpyAsync(x->h_tag_count, x->d_tag_count, blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    uint64_t sum = 0;
    for (uint32_t i = 0; i < blocks; ++i) sum += x->h_tag_count[i];
    *kept = sum;
    return CQS_HIP_OK;
}

// The bitsets of `f` filters (allows [f * 32], host; 1 <= f <= kCombineCap) over the whole index into rows 0 .. f - 1 of
// d_tab (stride_words each) on x->stream, by ONE launch, and the exact kept rows of each after one copy and one wait.
// Caller holds mu, has set the device; n >= 1, every row tagged.
int32_t tags_keep_multi_locked(cqs_hip_index* x, const uint32_t* allows, uint32_t f, uint32_t max_blocks, uint32_t* d_tab,
                               uint32_t stride_words, uint64_t* kept) {
    constexpr size_t tbl_bytes = cqs_tags::kTableWords * sizeof(uint32_t);
    constexpr size_t cnt_bytes = (size_t)cqs::kTagMultiMaxBlocks * cqs_tags::kMaxFilters * sizeof(uint32_t);
    if (!x->d_tag_tbl) HIP_TRY(x, hipMalloc(&x->d_tag_tbl, tbl_bytes));
    if (!x->h_tag_tbl) HIP_TRY(x, hipHostMalloc(&x->h_tag_tbl, tbl_bytes, hipHostMallocDefault));
    if (!x->d_tag_mcount) HIP_TRY(x, hipMalloc(&x->d_tag_mcount, cnt_bytes));
    if (!x->h_tag_mcount) HIP_TRY(x, hipHostMalloc(&x->h_tag_mcount, cnt_bytes, hipHostMallocDefault));
    cqs_tags::transpose_filters(allows, f, x->h_tag_tbl);   // (the last block's copy of it has been waited for)
    const uint32_t blocks = cqs::tags_keep_multi_blocks((uint32_t)x->n, max_blocks);
    HIP_TRY(x, hipMemcpyAsync(x->d_tag_tbl, x->h_tag_tbl, tbl_bytes, hipMemcpyHostToDevice, x->stream));
    HIP_TRY(x, cqs::launch_tags_keep_multi(x->d_tags, (uint32_t)x->n, x->d_tag_tbl, f, d_tab, stride_words, x->d_tag_mcount,
                                           max_blocks, x->stream));
    HIP_TRY(x, hipMemcpyAsync(x->h_tag_mcount, x->d_tag_mcount, (size_t)blocks * f * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    for (uint32_t j = 0; j < f; ++j) kept[j] = 0;
    for (uint32_t blk = 0; blk < blocks; ++blk)
        for (uint32_t j = 0; j < f; ++j) kept[j] += x->h_tag_mcount[(size_t)blk * f + j];
    return CQS_HIP_OK;
}

// `b` queries under ONE filter, as cqs_hip_index_search_tagged has always run them: the bitset into d_keep, its exact
// count, then the shared-bitset kernels at k_eff.  Caller holds mu, has set the device and ordered x->stream.
int32_t tagged_shared_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k, const uint32_t* allow,
                             uint32_t mode, float threshold) {
    uint64_t included = 0;
    int32_t rc = tags_keep_locked(x, allow, &included);
    if (rc != CQS_HIP_OK) return rc;
    uint32_t k_eff = k;
    const cqs_search::Keep kept = cqs_tags::plan_keep_count(included, x->n, &k_eff);   // src/cagra.rs:760-775
    if (kept == cqs_search::Keep::Empty) return CQS_HIP_OK;
    // A lone query takes the kernels its host-bitset call takes: that call rides the combining queue, whose blocks
    // are gemv passes (index_combine.hip), unless the queue is off.
    const bool gemv_only = b == 1 && x->combine && x->combine_filtered;
    return search_blocks_locked(x, qs, b, k_eff, kept == cqs_search::Keep::Filtered ? x->d_keep : nullptr, mode, threshold, gemv_only);
}

}  // namespace

// `b` queries with one (k, mode, threshold) and a tag filter EACH (qs[i].allow): blocks of <= kCombineCap queries whose
// bitsets tags_keep_multi_kernel writes into the handle's table in one pass over the tags - no host bitset, no staging
// copy - and which then run exactly as search_filtered_locked's blocks run (index.hip): gemv passes that mask each query's
// scores with its own table row, at the callers' k, through the shadow copies under the rules of unfiltered blocks, the
// uncertified queries redone on the f32 scan with their own rows.  A query that keeps nothing or is not finite is answered
// with count 0 and takes no slot.  A block of one is the lone call (tagged_shared_locked); so is every query when there is
// no memory for the table.
int32_t search_tagged_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k, uint32_t mode, float threshold) {
    int32_t rc = injected_failure(x);
    if (rc != CQS_HIP_OK || x->n == 0 || k == 0) return rc;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, order_after_last(x, x->stream));
    if (b == 1 || !ensure_keep_tab(x)) {
        for (uint32_t i = 0; i < b; ++i)
            if ((rc = tagged_shared_locked(x, &qs[i], 1, k, qs[i].allow, mode, threshold)) != CQS_HIP_OK) return rc;
        return CQS_HIP_OK;
    }
    std::vector<const cqs_combine_req*> staged;
    std::vector<uint32_t> allows((size_t)kCombineCap * cqs_tags::kAllowWords);
    uint64_t kept[kCombineCap];
    uint8_t slot[kCombineCap];
    for (uint32_t done = 0; done < b;) {
        // the next block: filter i in table row i; the queries that have an answer in h_q rows 0 .., each with its row's slot
        const uint32_t nb = (b - done) < kCombineCap ? (b - done) : kCombineCap;
        if ((rc = ensure_scratch(x, nb, k)) != CQS_HIP_OK) return rc;
        for (uint32_t i = 0; i < nb; ++i)
            memcpy(allows.data() + (size_t)i * cqs_tags::kAllowWords, qs[done + i].allow, cqs_tags::kAllowWords * sizeof(uint32_t));
        if ((rc = tags_keep_multi_locked(x, allows.data(), nb, 0, x->d_keep_tab, (uint32_t)x->keep_tab_stride, kept)) != CQS_HIP_OK) return rc;
        staged.clear();
        for (uint32_t i = 0; i < nb; ++i) {
            const cqs_combine_req& r = qs[done + i];
            if (kept[i] == 0 || !cqs_search::query_finite(r.q, x->dim)) continue;   // src/cagra.rs:765-767, :464-470
            memcpy(x->h_q + staged.size() * x->dim, r.q, (size_t)x->dim * sizeof(float));
            slot[staged.size()] = (uint8_t)i;
            staged.push_back(&r);
        }
        done += nb;
        if (staged.empty()) continue;
        if ((rc = answer_block(x, staged, slot, k, nullptr, mode, threshold, /*gemv_only=*/true)) != CQS_HIP_OK) return rc;
    }
    return CQS_HIP_OK;
}

}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

int32_t cqs_hip_index_set_tags(cqs_hip_index* x, uint64_t first_row, const uint32_t* tags, uint64_t m) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->sh) return fail(x, CQS_HIP_ERR_INVALID, "set_tags: not built for a row-sharded handle");
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    uint64_t first = 0, new_tagged = 0;
    const char* why = "";
    const cqs_tags::Set plan = cqs_tags::plan_set_tags(first_row, tags, m, x->row_base, x->n, x->tagged, &first, &new_tagged, &why);
    if (plan == cqs_tags::Set::Invalid) return fail(x, CQS_HIP_ERR_INVALID, (std::string("set_tags: ") + why).c_str());
    if (plan == cqs_tags::Set::Nothing) return CQS_HIP_OK;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // (nothing in flight reads the column - tagged searches wait under mu - but a regrow may free it)
    if (!x->d_tags) {         // first call: the column, sized like the corpus (a borrowing handle's cap_rows is its n)
        const uint64_t cap = x->cap_rows > x->n ? x->cap_rows : x->n;
        HIP_TRY(x, hipMalloc(&x->d_tags, (size_t)cap * sizeof(uint32_t)));
        x->tags_cap = cap;
    }
    HIP_TRY(x, hipMemcpyAsync(x->d_tags + first, tags, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));   // (the caller's array is free on return)
    x->tagged = new_tagged;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

uint64_t cqs_hip_index_tagged_rows(const cqs_hip_index* x) CQS_ABI_TRY {
    if (!x || x->sh) return 0;
    std::lock_guard<std::mutex> g(x->mu);
    return x->tagged;
} CQS_ABI_CATCH_VAL(0)

int32_t cqs_hip_index_count_tagged(cqs_hip_index* x, const uint32_t* allow, uint64_t* out_kept) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    if (out_kept) *out_kept = 0;
    std::lock_guard<std::mutex> g(x->mu);
    int32_t rc = tagged_ready(x, allow, "count_tagged");
    if (rc != CQS_HIP_OK) return rc;
    if (!out_kept) return fail(x, CQS_HIP_ERR_INVALID, "count_tagged: null out_kept");
    if (x->n == 0) return CQS_HIP_OK;
    if (cqs_tags::all_pass(allow)) { *out_kept = x->n; return CQS_HIP_OK; }
    HIP_TRY(x, hipSetDevice(x->device));
    return tags_keep_locked(x, allow, out_kept);
} CQS_ABI_CATCH(x)

int32_t cqs_hip_index_search_tagged(cqs_hip_index* x, const float* queries, uint32_t b, uint32_t query_dim, uint32_t k,
                                    const uint32_t* allow, uint32_t mode, float threshold, uint64_t* out_rows,
                                    float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_search_tagged");
    if (!x) return CQS_HIP_ERR_INVALID;
    // One query under a filter that constrains something, arguments in order (the condition list of cqs_hip_index_search's
    // fast path), a single-device handle: the combining queue, in blocks of tagged callers only (index_combine.hip).
    // Every other call takes the path below, which is what it has always been.
    if (x->combine && x->combine_tagged && b == 1 && !x->sh && allow && !cqs_tags::all_pass(allow) && queries && out_counts &&
        out_rows && out_scores && query_dim == x->dim && k >= 1 && k <= cqs::kMaxK && mode <= CQS_HIP_MODE_PIPELINE) {
        // The pre-check, under mu when mu is free.  When it is not, a pass (or an extend, a save ...) holds it: waiting here
        // would keep this caller out of the queue until that pass ends - the callers a pass has just answered would queue on
        // mu instead of parking, and the next leader would seal its block without them (measured: 2.6 callers per block of
        // 8 threads instead of 7.9).  Such a caller parks unchecked; the sealed block repeats tagged_ready under mu and
        // hands every caller the same status and message.
        if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
        {
            std::unique_lock<std::mutex> g(x->mu, std::try_to_lock);
            if (g.owns_lock()) {
                const int32_t rc = tagged_ready(x, allow, "search_tagged");
                if (rc != CQS_HIP_OK) return rc;
            }
        }
        out_counts[0] = 0;
        if (!cqs_search::query_finite(queries, query_dim)) return CQS_HIP_OK;                    // src/cagra.rs:464-470
        cqs_combine_req r{queries, k, mode, threshold, out_rows, out_scores, out_counts};
        r.allow = allow;
        return combine_search(x, r);
    }
    {
        std::lock_guard<std::mutex> g(x->mu);
        int32_t rc = tagged_ready(x, allow, "search_tagged");
        if (rc != CQS_HIP_OK) return rc;
        if (!cqs_tags::all_pass(allow)) {
            const cqs_search::Args a{queries, b, query_dim, k, mode, out_rows, out_scores, out_counts};
            if (!search_planned(x, a, &rc)) return rc;
            const std::vector<cqs_combine_req> rq = requests(a, threshold);
            if ((rc = injected_failure(x)) != CQS_HIP_OK) return rc;
            HIP_TRY(x, hipSetDevice(x->device));
            HIP_TRY(x, order_after_last(x, x->stream));
            return tagged_shared_locked(x, rq.data(), b, k, allow, mode, threshold);
        }
    }
    // no field is constrained: the unfiltered search, no device work for the filter (and its single queries are combined)
    return cqs_hip_index_search(x, queries, b, query_dim, k, nullptr, mode, threshold, out_rows, out_scores, out_counts);
} CQS_ABI_CATCH(x)

// `b` queries with a tag filter each (allows [b * 32]): per query the bytes of cqs_hip_index_search_tagged(that query, 1,
// ..., that filter, ...).  Holds mu throughout; not the queue, so no combine counter moves.
int32_t cqs_hip_index_search_tagged_multi(cqs_hip_index* x, const float* queries, uint32_t b, uint32_t query_dim, uint32_t k,
                                          const uint32_t* allows, uint32_t mode, float threshold, uint64_t* out_rows,
                                          float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_search_tagged_multi");
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    int32_t rc = tagged_ready(x, allows, "search_tagged_multi");
    if (rc != CQS_HIP_OK) return rc;
    const cqs_search::Args a{queries, b, query_dim, k, mode, out_rows, out_scores, out_counts};
    if (!search_planned(x, a, &rc)) return rc;
    std::vector<cqs_combine_req> rq = requests(a, threshold);
    for (uint32_t i = 0; i < b; ++i) rq[i].allow = allows + (size_t)i * cqs_tags::kAllowWords;
    return search_tagged_locked(x, rq.data(), b, k, mode, threshold);
} CQS_ABI_CATCH(x)

// Test hook (not part of the public header): the bitset tags_keep_kernel builds for `allow` - also an all-pass one, which
// the public calls never launch - copied to out_words, ceil(len / 32) words.
int32_t cqs_hip_debug_index_tag_keep(cqs_hip_index* x, const uint32_t* allow, uint32_t* out_words) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    int32_t rc = tagged_ready(x, allow, "debug_tag_keep");
    if (rc != CQS_HIP_OK) return rc;
    if (!out_words) return fail(x, CQS_HIP_ERR_INVALID, "debug_tag_keep: null out_words");
    if (x->n == 0) return CQS_HIP_OK;
    HIP_TRY(x, hipSetDevice(x->device));
    uint64_t kept = 0;
    if ((rc = tags_keep_locked(x, allow, &kept)) != CQS_HIP_OK) return rc;
    HIP_TRY(x, hipMemcpy(out_words, x->d_keep, (size_t)((x->n + 31) / 32) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook (not part of the public header): tags_keep_multi_kernel for the f filters at allows [f * 32] (1 <= f <= 32;
// all-pass ones too) with the grid cap max_blocks (0 = default), into a scratch table of 32 rows of ceil(len / 32) + 2
// words pre-filled with 0xA5A5A5A5.  out_words [f * ceil(len / 32)] receives rows 0 .. f - 1, out_kept [f] the counts.
// CQS_HIP_ERR_INVALID ("... wrote outside its rows") when a word behind a row's ceil(len / 32) words, or any word of a
// row >= f, is no longer the fill.
int32_t cqs_hip_debug_index_tag_keep_multi(cqs_hip_index* x, const uint32_t* allows, uint32_t f, uint32_t max_blocks,
                                           uint32_t* out_words, uint64_t* out_kept) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    int32_t rc = tagged_ready(x, allows, "debug_tag_keep_multi");
    if (rc != CQS_HIP_OK) return rc;
    if (!out_words || !out_kept || f == 0 || f > kCombineCap) return fail(x, CQS_HIP_ERR_INVALID, "debug_tag_keep_multi: bad arguments");
    if (x->n == 0) return CQS_HIP_OK;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, order_after_last(x, x->stream));
    constexpr uint32_t fill = 0xA5A5A5A5u;
    const uint32_t words = (uint32_t)((x->n + 31) / 32), stride = words + 2;
    std::vector<uint32_t> h((size_t)kCombineCap * stride);
    uint32_t* d_tab = nullptr;
    HIP_TRY(x, hipMalloc(&d_tab, h.size() * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(d_tab, 0xA5, h.size() * sizeof(uint32_t), x->stream);
    if (e == hipSuccess) {
        uint64_t kept[kCombineCap];
        rc = tags_keep_multi_locked(x, allows, f, max_blocks, d_tab, stride, kept);
        for (uint32_t j = 0; rc == CQS_HIP_OK && j < f; ++j) out_kept[j] = kept[j];
        if (rc == CQS_HIP_OK) e = hipMemcpy(h.data(), d_tab, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    hipFree(d_tab);
    if (rc != CQS_HIP_OK) return rc;
    HIP_TRY(x, e);
    for (uint32_t j = 0; j < kCombineCap; ++j)
        for (uint32_t w = j < f ? words : 0u; w < stride; ++w)
            if (h[(size_t)j * stride + w] != fill) return fail(x, CQS_HIP_ERR_INVALID, "debug_tag_keep_multi: the kernel wrote outside its rows");
    for (uint32_t j = 0; j < f; ++j) memcpy(out_words + (size_t)j * words, h.data() + (size_t)j * stride, (size_t)words * sizeof(uint32_t));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

}  // extern "C"
