// index_diff.hip — cqs_hip_index_diff: the reference's `semantic_diff` arithmetic (src/diff.rs:172-215) between two
// resident indexes.  The reference fetches both embeddings of every matched chunk from SQLite, a thousand at a time, and
// runs `full_cosine_similarity` (src/math.rs:35-67) on the CPU; here pair i is (stored row rows_a[i] of a, stored row
// rows_b[i] of b), both read where they lie in HBM: one wave per pair gathers the two rows and sums dot and both squared
// norms in f64, two small kernels compact the pairs below the threshold in pair order, and only the answer crosses the
// bus.  The plan, the passes and the arithmetic's restatement are diff_host.h; DESIGN.md §3.17.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "diff_host.h"
#include "index_internal.h"
#include "roctx.h"
#include "scan_device.h"
#include "wave_ops.h"

namespace cqs_idx {

struct DiffParams {
    const float* rows_a;     // a's corpus
    const float* rows_b;     // b's
    const uint32_t* la;      // [pairs] local row of a per pair ...
    const uint32_t* lb;      // ... and of b
    uint32_t pairs, dim;
    float threshold;
    float* sims;             // [pairs]
    uint32_t* cls;           // [pairs] class words (cqs_diff::kModified | kUndefined)
    uint2* tiles;            // [ceil(pairs / kTile)] (modified, undefined) of each tile of kTile pairs
    uint2* list;             // [pairs] the modified pairs' (pass-local index, sim bits), ascending: cqs_diff::ListEntry
    uint32_t* counts;        // [2] modified, undefined of the pass
};

constexpr uint32_t kDiffThreads = 256;
constexpr uint32_t kDiffWaves = kDiffThreads / 64u;

__device__ __forceinline__ void diff_piece(const cqs::f4& x, const cqs::f4& y, double& dot, double& na, double& nb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) cqs_diff::accumulate((double)x[e], (double)y[e], &dot, &na, &nb);
}

// The three lane sums to the pair's sim and class, stored by lane 0 (every lane holds the same bits after the butterfly).
__device__ __forceinline__ void diff_finish(const DiffParams& p, uint32_t pair, uint32_t lane, double dot, double na, double nb) {
    dot = cqs::wave_sum64_shfl(dot);
    na = cqs::wave_sum64_shfl(na);
    nb = cqs::wave_sum64_shfl(nb);
    uint32_t c;
    const float sim = cqs_diff::finish_pair(dot, na, nb, p.threshold, &c);
    if (lane == 0) {
        p.sims[pair] = sim;
        p.cls[pair] = c;
    }
}

// One wave per pair, four to a workgroup, one workgroup per four pairs: no grid-stride loop and no pair held ahead - the
// dispatcher keeps every CU's wave slots full, which measured faster than either.  Lane l takes the
// 16-byte pieces l, l + 64, ... of both rows (dim % 4 == 0, rows 16-byte aligned), four of each row in flight, each
// component converted to f64 and folded into three f64 sums in piece order, then the fixed xor-butterfly: the shape of the
// sum is a function of dim alone, so a pair's sim depends on nothing else - not on the grid, the pair's place in the list
// or the pass.
__global__ __launch_bounds__(kDiffThreads) void diff_score_kernel(DiffParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pair = blockIdx.x * kDiffWaves + (threadIdx.x >> 6);
    if (pair >= p.pairs) return;   // (whole waves)
    const float* __restrict__ ra = p.rows_a + (size_t)p.la[pair] * p.dim;
    const float* __restrict__ rb = p.rows_b + (size_t)p.lb[pair] * p.dim;
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (uint32_t c = lane * 4u; c < p.dim; c += 4u * 256u) {
        cqs::f4 x[4], y[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u)
            if (c + u * 256u < p.dim) { x[u] = *(const cqs::f4*)(ra + c + u * 256u); y[u] = *(const cqs::f4*)(rb + c + u * 256u); }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u)
            if (c + u * 256u < p.dim) diff_piece(x[u], y[u], dot, na, nb);
    }
    diff_finish(p, pair, lane, dot, na, nb);
}

// The class words of tile blockIdx.x, item j * 256 + thread of it per step: its ballots' bit counts land in LDS words by
// integer adds (any order gives the same sums).
constexpr uint32_t kTileSteps = cqs_diff::kTile / kDiffThreads;

// (modified, undefined) of every tile.
__global__ __launch_bounds__(kDiffThreads) void diff_count_kernel(DiffParams p) {
    __shared__ uint32_t total[2];
    if (threadIdx.x < 2u) total[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * cqs_diff::kTile;
    uint32_t mod = 0, undef = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTileSteps; ++j) {
        const uint32_t i = base + j * kDiffThreads + threadIdx.x;
        const uint32_t c = i < p.pairs ? p.cls[i] : 0u;
        mod += (uint32_t)__popcll(__ballot((c & cqs_diff::kModified) != 0));
        undef += (uint32_t)__popcll(__ballot((c & cqs_diff::kUndefined) != 0));
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&total[0], mod);
        atomicAdd(&total[1], undef);
    }
    __syncthreads();
    if (threadIdx.x == 0) p.tiles[blockIdx.x] = make_uint2(total[0], total[1]);
}

// Tile blockIdx.x's modified pairs into the list, behind those of the tiles before it (their counts summed here) and in
// pair order inside the tile: step by step, wave by wave, lane by lane.  The last tile's workgroup leaves the pass's counts.
__global__ __launch_bounds__(kDiffThreads) void diff_write_kernel(DiffParams p) {
    __shared__ uint32_t before[2];                       // modified / undefined of the tiles before this one
    __shared__ uint32_t part[kTileSteps * kDiffWaves];   // modified of each (step, wave) of this tile
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 2u) before[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mod = 0, undef = 0;
    for (uint32_t t = threadIdx.x; t < blockIdx.x; t += kDiffThreads) {
        const uint2 c = p.tiles[t];
        mod += c.x;
        undef += c.y;
    }
    if (mod) atomicAdd(&before[0], mod);
    if (undef) atomicAdd(&before[1], undef);
    const uint32_t base = blockIdx.x * cqs_diff::kTile;
    bool mine[kTileSteps];
    uint32_t rank[kTileSteps];                           // modified pairs of my (step, wave) in lanes below mine
#pragma unroll
    for (uint32_t j = 0; j < kTileSteps; ++j) {
        const uint32_t i = base + j * kDiffThreads + threadIdx.x;
        mine[j] = i < p.pairs && (p.cls[i] & cqs_diff::kModified) != 0;
        const unsigned long long b = __ballot(mine[j]);
        rank[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) part[j * kDiffWaves + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t at = before[0], own = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTileSteps; ++j) {
#pragma unroll
        for (uint32_t w = 0; w < kDiffWaves; ++w) {
            const uint32_t n = part[j * kDiffWaves + w];
            if (w == wave && mine[j]) {
                const uint32_t i = base + j * kDiffThreads + threadIdx.x;
                p.list[at + own + rank[j]] = make_uint2(i, __float_as_uint(p.sims[i]));
            }
            own += n;
        }
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) {
        const uint2 last = p.tiles[blockIdx.x];
        p.counts[0] = before[0] + last.x;
        p.counts[1] = before[1] + last.y;
    }
}

namespace {

// A pass of c pairs in the staging block: the two local row lists first (one copy in), then sims, class words, the
// compacted list (8-byte entries: 16 c is a multiple of 8), the tile counts and the pass's counts.
struct DiffStage {
    uint64_t c, tiles;
    explicit DiffStage(uint64_t pairs) : c(pairs), tiles((pairs + cqs_diff::kTile - 1) / cqs_diff::kTile) {}
    uint64_t total() const { return 24u * c + 8u * tiles + 16u; }
    uint32_t* la(void* base) const { return (uint32_t*)base; }
    uint32_t* lb(void* base) const { return (uint32_t*)((char*)base + 4u * c); }
    float* sims(void* base) const { return (float*)((char*)base + 8u * c); }
    uint32_t* cls(void* base) const { return (uint32_t*)((char*)base + 12u * c); }
    uint2* list(void* base) const { return (uint2*)((char*)base + 16u * c); }
    uint2* tile_counts(void* base) const { return (uint2*)((char*)base + 24u * c); }
    uint32_t* counts(void* base) const { return (uint32_t*)((char*)base + 24u * c + 8u * tiles); }
};

// The staging pair holds a pass of `pairs` pairs (regrown; a's stream is idle of earlier diffs: each ends with a wait).
// Nothing is touched on failure.
int32_t ensure_diff_stage(cqs_hip_index* a, uint64_t pairs) {
    if (pairs <= a->diff_pairs) return CQS_HIP_OK;
    diff_free(a);
    const uint64_t bytes = DiffStage(pairs).total();
    hipError_t e = hipHostMalloc(&a->diff_h, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&a->diff_d, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        diff_free(a);
        return fail(a, e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, "diff: staging buffer", e);
    }
    a->diff_pairs = pairs;
    return CQS_HIP_OK;
}

cqs_diff::Side side_of(const cqs_hip_index* x) {
    return cqs_diff::Side{true, x->sh != nullptr, x->device, x->dim, x->row_base, x->sh ? 0 : x->n};
}

bool is_poisoned(const cqs_hip_index* x) {
    return x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire);
}

// Caller holds both mutexes and has planned the call.  Everything runs on a's stream, ordered after the last search of
// each handle; every pass ends with a wait, so nothing of b is read once the call has returned.
int32_t diff_locked(cqs_hip_index* a, cqs_hip_index* b, const uint64_t* rows_a, const uint64_t* rows_b, uint64_t m,
                    float threshold, float* out_sims, uint64_t* out_mod_pairs, float* out_mod_sims, uint64_t* out_counts) {
    HIP_TRY(a, hipSetDevice(a->device));
    HIP_TRY(a, order_after_last(a, a->stream));
    if (b != a) HIP_TRY(a, order_after_last(b, a->stream));
    const uint64_t budget = a->diff_budget_pairs ? a->diff_budget_pairs : cqs_diff::kPassPairs;
    const std::vector<cqs_diff::Pass> passes = cqs_diff::cut_passes(m, budget);
    const int32_t rc = ensure_diff_stage(a, std::min(m, budget));
    if (rc != CQS_HIP_OK) return rc;
    uint64_t modified = 0, undefined = 0;
    for (const cqs_diff::Pass& ps : passes) {
        const DiffStage st(ps.count);
        cqs_diff::local_rows(rows_a, a->row_base, ps, st.la(a->diff_h));
        cqs_diff::local_rows(rows_b, b->row_base, ps, st.lb(a->diff_h));
        HIP_TRY(a, hipMemcpyAsync(a->diff_d, a->diff_h, 8u * ps.count, hipMemcpyHostToDevice, a->stream));
        DiffParams p;
        p.rows_a = a->d_rows;
        p.rows_b = b->d_rows;
        p.la = st.la(a->diff_d);
        p.lb = st.lb(a->diff_d);
        p.pairs = (uint32_t)ps.count;
        p.dim = a->dim;
        p.threshold = threshold;
        p.sims = st.sims(a->diff_d);
        p.cls = st.cls(a->diff_d);
        p.tiles = st.tile_counts(a->diff_d);
        p.list = st.list(a->diff_d);
        p.counts = st.counts(a->diff_d);
        hipLaunchKernelGGL(diff_score_kernel, dim3((uint32_t)((ps.count + kDiffWaves - 1) / kDiffWaves)), dim3(kDiffThreads), 0, a->stream, p);
        HIP_TRY(a, hipGetLastError());
        hipLaunchKernelGGL(diff_count_kernel, dim3((uint32_t)st.tiles), dim3(kDiffThreads), 0, a->stream, p);
        HIP_TRY(a, hipGetLastError());
        hipLaunchKernelGGL(diff_write_kernel, dim3((uint32_t)st.tiles), dim3(kDiffThreads), 0, a->stream, p);
        HIP_TRY(a, hipGetLastError());
        HIP_TRY(a, hipMemcpyAsync(st.counts(a->diff_h), st.counts(a->diff_d), 2u * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        if (out_sims) HIP_TRY(a, hipMemcpyAsync(st.sims(a->diff_h), st.sims(a->diff_d), 4u * ps.count, hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(a, hipStreamSynchronize(a->stream));
        const uint32_t n_mod = st.counts(a->diff_h)[0];
        if (n_mod > ps.count) return fail(a, CQS_HIP_ERR_DEVICE, "diff: a pass counted more modified pairs than it holds");
        if (out_sims) memcpy(out_sims + ps.first, st.sims(a->diff_h), 4u * ps.count);
        if (out_mod_pairs && n_mod) {
            HIP_TRY(a, hipMemcpyAsync(st.list(a->diff_h), st.list(a->diff_d), 8u * (uint64_t)n_mod, hipMemcpyDeviceToHost, a->stream));
            HIP_TRY(a, hipStreamSynchronize(a->stream));   // the next pass restages the same block
            cqs_diff::append_modified(ps, (const cqs_diff::ListEntry*)st.list(a->diff_h), n_mod, modified, out_mod_pairs, out_mod_sims);
        }
        modified += n_mod;
        undefined += st.counts(a->diff_h)[1];
    }
    out_counts[0] = modified;
    out_counts[1] = m - modified;
    out_counts[2] = undefined;
    return CQS_HIP_OK;
}

}  // namespace

void diff_free(cqs_hip_index* x) {
    if (x->diff_h) (void)hipHostFree(x->diff_h);
    if (x->diff_d) (void)hipFree(x->diff_d);
    x->diff_h = x->diff_d = nullptr;
    x->diff_pairs = 0;
}

}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

int32_t cqs_hip_index_diff(cqs_hip_index* a, const uint64_t* rows_a, cqs_hip_index* b, const uint64_t* rows_b, uint64_t m,
                           float threshold, float* out_sims, uint64_t* out_mod_pairs, float* out_mod_sims,
                           uint64_t* out_counts) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_diff");
    if (!a || !b) return CQS_HIP_ERR_INVALID;
    cqs_diff::PairLock<std::mutex> g(a->mu, b->mu);
    if (is_poisoned(a) || is_poisoned(b)) return CQS_HIP_ERR_POISONED;
    const cqs_diff::Args args{rows_a, rows_b, m, threshold, out_counts != nullptr, out_mod_pairs != nullptr, out_mod_sims != nullptr};
    std::string why;
    const cqs_diff::Plan plan = cqs_diff::plan_diff(side_of(a), side_of(b), args, &why);
    if (plan == cqs_diff::Plan::Invalid) return fail(a, CQS_HIP_ERR_INVALID, ("diff: " + why).c_str());
    if (plan == cqs_diff::Plan::Nothing) {
        if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = 0;
        return CQS_HIP_OK;
    }
    return diff_locked(a, b, rows_a, rows_b, m, threshold, out_sims, out_mod_pairs, out_mod_sims, out_counts);
} CQS_ABI_CATCH(a)

// Test hook (not part of the public header): the next diffs with this handle as `a` cut their passes at `pairs` pairs
// instead of at cqs_diff::kPassPairs (0, or anything past it: kPassPairs again).
void cqs_hip_debug_index_diff_budget(cqs_hip_index* a, uint64_t pairs) CQS_ABI_TRY {
    if (!a) return;
    std::lock_guard<std::mutex> g(a->mu);
    a->diff_budget_pairs = pairs > cqs_diff::kPassPairs ? 0 : pairs;
} CQS_ABI_CATCH_VOID

}  // extern "C"
