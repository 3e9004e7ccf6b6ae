// index_tags.hip — row tags on the device: one u32 per row beside the corpus, and the filtered search that
// sends 128 bytes of allowed sets instead of a keep-bitset of n / 8 bytes.  The predicate the reference sends with every
// filtered and hybrid query - chunk type in / not in a set, language in a set, src/search/query.rs:860-900 - is a function
// of two small integers per chunk; its host loop over all n chunk ids (src/cagra.rs:747-757) becomes tags_keep_kernel,
// which writes the bitset the scans already read.  The scan, select and shadow kernels are untouched: search_tagged hands
// the device bitset to the host search's block runner (index.hip) where the staged host bitset would go, so the answer is
// the bytes of cqs_hip_index_search with the host bitset of the same predicate.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

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

}  // namespace cqs

namespace cqs_idx {

void tags_free(cqs_hip_index* x) {
    hipFree(x->d_tags);
    hipFree(x->d_tag_count);
    hipHostFree(x->h_tag_count);
    x->d_tags = nullptr; x->d_tag_count = nullptr; x->h_tag_count = nullptr;
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

namespace {

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

}  // namespace
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
            uint64_t included = 0;
            if ((rc = tags_keep_locked(x, allow, &included)) != CQS_HIP_OK) return rc;
            uint32_t k_eff = k;
            const cqs_search::Keep kept = cqs_tags::plan_keep_count(included, x->n, &k_eff);   // src/cagra.rs:760-775
            if (kept == cqs_search::Keep::Empty) return CQS_HIP_OK;
            // A lone query takes the kernels its host-bitset call takes: that call rides the combining queue, whose blocks
            // are gemv passes (index_combine.hip), unless the queue is off.
            const bool gemv_only = b == 1 && x->combine && x->combine_filtered;
            return search_blocks_locked(x, rq.data(), b, k_eff, kept == cqs_search::Keep::Filtered ? x->d_keep : nullptr, mode,
                                        threshold, gemv_only);
        }
    }
    // no field is constrained: the unfiltered search, no device work for the filter (and its single queries are combined)
    return cqs_hip_index_search(x, queries, b, query_dim, k, nullptr, mode, threshold, out_rows, out_scores, out_counts);
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

}  // extern "C"
