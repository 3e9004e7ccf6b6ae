// index_remove.hip — cqs_hip_index_remove: rows leave the resident corpus in place.  The other half of "the GPU corpus
// never needs a periodic rebuild": the reference's tiered backend exists "to clean orphaned vectors and absorb deltas"
// (src/tiered.rs:13-17); extend absorbs, this cleans.  An order-preserving compaction of d_rows and of the shadow's
// per-row buffers through a bounded bounce buffer, planned on the host (remove_host.h), DESIGN.md §3.13.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "abi_guard.h"
#include "index_internal.h"
#include "remove_host.h"
#include "tags_host.h"

namespace cqs_idx {

// The bounce buffer: large enough that a pass moves >= 10 us of HBM traffic per launch (the launch gaps amortise), small
// enough that the buffer and everything a pass streams between writing one of its lines and reading it back (<= 2 x this)
// fit the 256 MiB Infinity Cache.  Allocated per call and freed before the call returns: remove is rare next to search,
// and an idle handle should not hold 64 MiB for it.
constexpr uint64_t kBounceBytes = 64ull << 20;
constexpr uint32_t kGatherThreads = 256;
constexpr uint32_t kRowsPerGroup = 4;    // consecutive destination rows one lane group gathers (one lookup, then it walks the runs)

// The runs as the device reads them: x = first source row, y = first destination row, one entry per run in order and a
// closing entry (old n, new n), so a run's rows are the next entry's y minus its own.
// The run that holds destination row d: the largest i in [0, n_runs) with runs[i].y <= d (runs[0].y <= d is the caller's).
__device__ __forceinline__ uint32_t find_run(const uint2* __restrict__ runs, uint32_t n_runs, uint32_t d) {
    uint32_t lo = 0, hi = n_runs;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (runs[mid].y <= d) lo = mid; else hi = mid;
    }
    return lo;
}

typedef uint32_t unit16 __attribute__((ext_vector_type(4)));   // 16 bytes as the compiler's own vector (stays in registers)

// One pass's gather: destination rows [d0, d0 + rows) of `src` (rows of `upr` units of T) into `bounce`, densely.  A group
// of `lanes` lanes (a power of two <= 64) takes kRowsPerGroup consecutive rows; lane `sub` of it moves units sub, sub +
// lanes, ... of each, four loads in flight before the first store.  T = unit16 for the three corpus copies (row bytes are a
// multiple of 16 in each), float for the int8 copy's row scales.  `src` and `bounce` never overlap; plain vector stores.
template <typename T>
__global__ __launch_bounds__(kGatherThreads) void remove_gather_kernel(const T* __restrict__ src, T* __restrict__ bounce,
                                                                     const uint2* __restrict__ runs, uint32_t n_runs,
                                                                     uint32_t d0, uint32_t rows, uint32_t upr, uint32_t lanes) {
    const uint32_t t = blockIdx.x * kGatherThreads + threadIdx.x;
    const uint32_t sub = t & (lanes - 1u);
    const uint32_t j0 = (t / lanes) * kRowsPerGroup;
    if (j0 >= rows) return;
    const uint32_t j1 = min(j0 + kRowsPerGroup, rows);
    uint32_t i = find_run(runs, n_runs, d0 + j0);
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t d = d0 + j;
        while (d >= runs[i + 1u].y) ++i;                  // (the closing entry ends the walk: d < new n)
        const T* __restrict__ sp = src + (size_t)(runs[i].x + (d - runs[i].y)) * upr;
        T* __restrict__ dp = bounce + (size_t)j * upr;
        for (uint32_t u = sub; u < upr; u += 4u * lanes) {
            T v[4];
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c)
                if (u + c * lanes < upr) v[c] = sp[u + c * lanes];
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c)
                if (u + c * lanes < upr) dp[u + c * lanes] = v[c];
        }
    }
}

namespace {

struct DeviceBuf {   // freed on every way out of remove_locked
    void* p = nullptr;
    ~DeviceBuf() { hipFree(p); }
};

// Compact one per-row buffer (rows of upr units of T) with the plan: per pass, in ascending row order on the handle's
// stream, the gather into the bounce buffer, then the stream-ordered copy of the bounce buffer to the pass's destination.
template <typename T>
int32_t compact(cqs_hip_index* x, T* base, uint32_t upr, const std::vector<cqs_remove::Pass>& passes, const uint2* d_runs, void* bounce) {
    uint32_t lanes = 1;
    while (lanes < 64u && lanes < upr) lanes *= 2u;
    for (const cqs_remove::Pass& p : passes) {
        const uint64_t groups = (p.rows + kRowsPerGroup - 1) / kRowsPerGroup;
        const uint32_t blocks = (uint32_t)((groups * lanes + kGatherThreads - 1) / kGatherThreads);
        remove_gather_kernel<T><<<blocks, kGatherThreads, 0, x->stream>>>(base, (T*)bounce, d_runs + p.run_first, (uint32_t)p.run_count,
                                                                       (uint32_t)p.dst, (uint32_t)p.rows, upr, lanes);
        HIP_TRY(x, hipGetLastError());
        HIP_TRY(x, hipMemcpyAsync(base + (size_t)p.dst * upr, bounce, (size_t)p.rows * upr * sizeof(T), hipMemcpyDeviceToDevice, x->stream));
    }
    return CQS_HIP_OK;
}

// The passes of a buffer whose rows are row_bytes long: the handle's test budget in rows, else what fits kBounceBytes.
std::vector<cqs_remove::Pass> passes_for(const cqs_hip_index* x, const std::vector<cqs_remove::Run>& runs, uint64_t row_bytes) {
    return cqs_remove::cut_passes(runs, x->remove_budget_rows ? x->remove_budget_rows : kBounceBytes / row_bytes);
}

uint64_t largest_pass(const std::vector<cqs_remove::Pass>& passes) {
    uint64_t r = 0;
    for (const cqs_remove::Pass& p : passes) r = std::max(r, p.rows);
    return r;
}

// Caller holds mu, has checked the handle and the plan.  An allocation that fails leaves the index untouched (NOMEM); any
// failure after the first pass is queued leaves the corpus half-moved: the handle is poisoned (HIP_TRY, fail).
int32_t remove_locked(cqs_hip_index* x, const std::vector<uint64_t>& removed, const std::vector<cqs_remove::Run>& runs) {
    if (x->inject_fail.exchange(0, std::memory_order_acq_rel) != 0)
        return fail(x, CQS_HIP_ERR_DEVICE, "remove: injected device failure (test hook)");
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // a search enqueued on a caller stream may still read the rows
    shadow_sweep_reset(x);
    const uint64_t n_new = x->n - removed.size();
    if (!runs.empty()) {
        const ShadowBuffers sb = shadow_buffers(x);
        const uint32_t dim = x->dim;
        const auto pf = passes_for(x, runs, (uint64_t)dim * sizeof(float));
        const auto pb = sb.bf16 ? passes_for(x, runs, (uint64_t)dim * sizeof(uint16_t)) : std::vector<cqs_remove::Pass>();
        const auto p8 = sb.i8 ? passes_for(x, runs, dim) : std::vector<cqs_remove::Pass>();
        const auto ps = sb.i8 ? passes_for(x, runs, sizeof(float)) : std::vector<cqs_remove::Pass>();
        const auto pt = x->d_tags ? passes_for(x, runs, sizeof(uint32_t)) : std::vector<cqs_remove::Pass>();
        const uint64_t bounce_bytes = std::max(std::max(std::max(largest_pass(pf) * dim * sizeof(float), largest_pass(pb) * dim * sizeof(uint16_t)),
                                                        std::max(largest_pass(p8) * dim, largest_pass(ps) * sizeof(float))),
                                               largest_pass(pt) * sizeof(uint32_t));
        std::vector<uint2> h_runs(runs.size() + 1);   // (row ids fit 32 bits: create / extend keep n + row_base below 2^32)
        for (size_t i = 0; i < runs.size(); ++i) h_runs[i] = make_uint2((uint32_t)runs[i].src, (uint32_t)runs[i].dst);
        h_runs[runs.size()] = make_uint2((uint32_t)x->n, (uint32_t)n_new);
        DeviceBuf bounce, d_runs;
        HIP_TRY(x, hipMalloc(&bounce.p, bounce_bytes));
        HIP_TRY(x, hipMalloc(&d_runs.p, h_runs.size() * sizeof(uint2)));
        HIP_TRY(x, hipMemcpyAsync(d_runs.p, h_runs.data(), h_runs.size() * sizeof(uint2), hipMemcpyHostToDevice, x->stream));
        const uint2* dr = (const uint2*)d_runs.p;
        int32_t rc = compact<unit16>(x, (unit16*)x->d_rows, dim / 4u, pf, dr, bounce.p);
        // The shadow's copies move with the same runs.  Its r / norm / r8 / norm8 stay: they are maxima over a superset of
        // the surviving rows, so the certificate stays valid and only gets looser (more fallbacks at worst), and answers stay
        // the f32 scan's bytes.  d_stats stays too: the certified / fallback counts survive a removal.
        if (rc == CQS_HIP_OK && sb.bf16) rc = compact<unit16>(x, (unit16*)sb.bf16, dim / 8u, pb, dr, bounce.p);
        if (rc == CQS_HIP_OK && sb.i8) rc = compact<unit16>(x, (unit16*)sb.i8, dim / 16u, p8, dr, bounce.p);
        if (rc == CQS_HIP_OK && sb.i8) rc = compact<float>(x, sb.i8_scale, 1u, ps, dr, bounce.p);
        // The tag column moves with the same runs, whole (rows past the tagged prefix hold nothing anybody reads; the column
        // is as long as the corpus's allocation).
        if (rc == CQS_HIP_OK && x->d_tags) rc = compact<uint32_t>(x, x->d_tags, 1u, pt, dr, bounce.p);
        if (rc != CQS_HIP_OK) { (void)hipStreamSynchronize(x->stream); return rc; }   // (h_runs and the buffers outlive the queue)
        HIP_TRY(x, hipStreamSynchronize(x->stream));
    }
    x->tagged = cqs_tags::tagged_after_remove(removed.data(), removed.size(), x->tagged);
    x->n = n_new;   // cap_rows stays: nothing is reallocated, the keep-bitset table's stride stays valid
    return CQS_HIP_OK;
}

}  // namespace
}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

int32_t cqs_hip_index_remove(cqs_hip_index* x, const uint64_t* rows, uint64_t m, uint64_t* out_removed) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    if (out_removed) *out_removed = 0;
    std::lock_guard<std::mutex> g(x->mu);
    // A row-sharded parent: its shard starts must stay multiples of 32 rows (sharded.hip slices the host bitset by words);
    // keeping that across a removal is not built.
    if (x->sh) return fail(x, CQS_HIP_ERR_INVALID, "remove: not supported on a row-sharded handle");
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (x->borrow) return fail(x, CQS_HIP_ERR_INVALID, "remove: index borrows its rows");
    std::vector<uint64_t> removed;
    std::vector<cqs_remove::Run> runs;
    const char* why = "";
    const cqs_remove::Plan plan = cqs_remove::plan_remove(rows, m, x->row_base, x->n, &removed, &runs, &why);
    if (plan == cqs_remove::Plan::Invalid) return fail(x, CQS_HIP_ERR_INVALID, (std::string("remove: ") + why).c_str());
    if (plan == cqs_remove::Plan::Nothing) return CQS_HIP_OK;
    const int32_t rc = remove_locked(x, removed, runs);
    if (rc == CQS_HIP_OK && out_removed) *out_removed = removed.size();
    return rc;
} CQS_ABI_CATCH(x)

// Test hook (not part of the public header): the next removals on this handle cut their passes at `rows` rows of every
// buffer instead of at the bounce buffer's byte budget (0 = the byte budget again).
void cqs_hip_debug_index_remove_budget(cqs_hip_index* x, uint64_t rows) CQS_ABI_TRY {
    if (!x) return;
    std::lock_guard<std::mutex> g(x->mu);
    x->remove_budget_rows = rows < (1ull << 22) ? rows : (1ull << 22);   // (keeps a pass's thread count in 32 bits)
} CQS_ABI_CATCH_VOID

}  // extern "C"
