// index_knn.hip — cqs_hip_index_knn_graph: `find_neighbors` (src/cli/commands/search/neighbors.rs:86-132) for a range of
// stored rows in one call - the exact kNN graph of the resident corpus, what the reference's `cqs index --umap` has
// umap-learn approximate on the CPU from a stream of every embedding.  The corpus is cut into fixed tiles of T rows
// (knn_host.h); each tile the range touches runs as ONE block of enqueue_search whose queries are the tile's rows where
// they lie in d_rows, and knn_finish_kernel turns the block's packed keys into the asked targets' answers on the device:
// the target's own key dropped, the rest moved up (cqs_search::drop_self), rows and scores decoded, zeros past the count.
// One copy back and one wait per call.  DESIGN.md §3.16.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "index_internal.h"
#include "knn_host.h"
#include "roctx.h"

namespace cqs_idx {

struct KnnFinishParams {
    const uint64_t* keys;     // [tile rows, k1] the select's packed keys, descending
    const uint32_t* counts;   // [tile rows]
    uint32_t k1, limit;       // k1 <= limit + 1 <= 101
    uint32_t emit_first;      // first emitted query of the tile
    uint32_t emit_count;
    uint32_t first_global;    // global row of query 0 of the tile (row_base + tile_first; fits 32 bits as every packed row)
    uint64_t* out_rows;       // the call's staging arrays, at this tile's first target: [emit_count, limit] ...
    float* out_scores;
    uint32_t* out_counts;     // ... and [emit_count]
};

// One wave per emitted target, four to a workgroup.  k1 <= 101 and limit <= 100: lane l holds slots l and l + 64 of the
// target's key row and writes output slots l and l + 64.  The slot that names the target is found by ballot; every key
// goes to knn_host.h's dest_slot.  No LDS, no atomics; each output word is written by exactly one lane.
__global__ __launch_bounds__(256) void knn_finish_kernel(KnnFinishParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (e >= p.emit_count) return;   // (whole waves)
    const uint32_t q = p.emit_first + e;
    const uint64_t* __restrict__ keys = p.keys + (size_t)q * p.k1;
    const uint32_t have = p.counts[q];
    const uint32_t cnt = have < p.k1 ? have : p.k1;
    const uint32_t mark = cqs_knn::key_mark(p.first_global + q);
    uint64_t key[2];
    bool mine[2];
    for (uint32_t j = 0; j < 2u; ++j) {
        const uint32_t s = lane + 64u * j;
        key[j] = s < cnt ? keys[s] : 0ull;
        mine[j] = s < cnt && (uint32_t)key[j] == mark;
    }
    const unsigned long long b0 = __ballot(mine[0]), b1 = __ballot(mine[1]);
    const uint32_t self = b0 ? (uint32_t)__ffsll((long long)b0) - 1u : b1 ? 63u + (uint32_t)__ffsll((long long)b1) : cnt;
    const uint32_t count = cqs_knn::emitted(cnt, self < cnt, p.limit);
    uint64_t* __restrict__ orow = p.out_rows + (size_t)e * p.limit;
    float* __restrict__ oscore = p.out_scores + (size_t)e * p.limit;
    for (uint32_t j = 0; j < 2u; ++j) {
        const uint32_t s = lane + 64u * j;
        if (s < cnt && s != self) {
            const uint32_t d = cqs_knn::dest_slot(s, self);
            if (d < p.limit) {
                orow[d] = cqs_knn::key_row(key[j]);
                oscore[d] = __uint_as_float(cqs_knn::key_score_bits(key[j]));
            }
        }
        if (s >= count && s < p.limit) { orow[s] = 0ull; oscore[s] = 0.f; }   // (no key lands at or past `count`)
    }
    if (lane == 0) p.out_counts[e] = count;
}

namespace {

// The three staging arrays of a call of m targets at stride `limit`, in one block: rows (u64), scores, counts.
struct KnnStage {
    size_t rows_bytes, scores_bytes, counts_bytes;
    KnnStage(uint64_t m, uint32_t limit)
        : rows_bytes((size_t)m * limit * sizeof(uint64_t)), scores_bytes((size_t)m * limit * sizeof(float)),
          counts_bytes((size_t)m * sizeof(uint32_t)) {}
    size_t total() const { return rows_bytes + scores_bytes + counts_bytes; }
    uint64_t* rows(void* base) const { return (uint64_t*)base; }
    float* scores(void* base) const { return (float*)((char*)base + rows_bytes); }
    uint32_t* counts(void* base) const { return (uint32_t*)((char*)base + rows_bytes + scores_bytes); }
};

// The staging pair holds at least `bytes` (regrown; the stream is idle of earlier graph calls: each ends with a wait).
// Nothing is touched on failure.
int32_t ensure_knn_stage(cqs_hip_index* x, size_t bytes) {
    if (bytes <= x->knn_bytes) return CQS_HIP_OK;
    knn_free(x);
    hipError_t e = hipHostMalloc(&x->knn_h, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&x->knn_d, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        knn_free(x);
        return fail(x, e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, "knn_graph: staging buffer", e);
    }
    x->knn_bytes = bytes;
    return CQS_HIP_OK;
}

}  // namespace

void knn_free(cqs_hip_index* x) {
    if (x->knn_h) (void)hipHostFree(x->knn_h);
    if (x->knn_d) (void)hipFree(x->knn_d);
    x->knn_h = x->knn_d = nullptr;
    x->knn_bytes = 0;
}

}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

int32_t cqs_hip_index_knn_graph(cqs_hip_index* x, uint64_t first_row, uint64_t m, uint32_t limit, uint64_t* out_rows,
                                float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_knn_graph");
    cqs_knn::Planned pl;
    const char* why = "";
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    const cqs_knn::Handle h{true, x->sh != nullptr, x->row_base, x->sh ? cqs_sharded::len(x) : x->n,
                            x->sh ? 0u : max_query_block(x)};
    const cqs_knn::Plan plan = cqs_knn::plan_knn(h, first_row, m, limit, out_rows && out_scores && out_counts, &pl, &why);
    if (plan == cqs_knn::Plan::Invalid) return fail(x, CQS_HIP_ERR_INVALID, (std::string("knn_graph: ") + why).c_str());
    if (plan == cqs_knn::Plan::Nothing) return CQS_HIP_OK;
    const uint32_t L = pl.limit;
    if (pl.k1 == 0) {   // the target is the only row: it has no neighbour
        memset(out_rows, 0, (size_t)m * L * sizeof(uint64_t));
        memset(out_scores, 0, (size_t)m * L * sizeof(float));
        memset(out_counts, 0, (size_t)m * sizeof(uint32_t));
        return CQS_HIP_OK;
    }
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, order_after_last(x, x->stream));
    const std::vector<cqs_knn::Tile> tiles = cqs_knn::cut_tiles(pl.local_first, m, x->n, pl.tile);
    uint32_t widest = 0;
    for (const cqs_knn::Tile& t : tiles) widest = t.tile_rows > widest ? t.tile_rows : widest;
    int32_t rc = ensure_scratch(x, widest, pl.k1);   // (before the first enqueue: growing it moves d_out_keys)
    if (rc != CQS_HIP_OK) return rc;
    const KnnStage st(m, L);
    if ((rc = ensure_knn_stage(x, st.total())) != CQS_HIP_OK) return rc;
    // Tiles back to back on the handle's stream: stream order keeps a tile's finish ahead of the next tile's select, which
    // overwrites d_out_keys.
    for (const cqs_knn::Tile& t : tiles) {
        rc = enqueue_search(x, x->d_rows + (size_t)t.tile_first * x->dim, t.tile_rows, pl.k1, nullptr, CQS_HIP_MODE_RAW, 0.f,
                            x->d_out_keys, x->d_out_counts, x->stream);
        if (rc != CQS_HIP_OK) return rc;
        KnnFinishParams p;
        p.keys = x->d_out_keys;
        p.counts = x->d_out_counts;
        p.k1 = pl.k1;
        p.limit = L;
        p.emit_first = t.emit_first;
        p.emit_count = t.emit_count;
        p.first_global = (uint32_t)(x->row_base + t.tile_first);
        p.out_rows = st.rows(x->knn_d) + (size_t)t.out_offset * L;
        p.out_scores = st.scores(x->knn_d) + (size_t)t.out_offset * L;
        p.out_counts = st.counts(x->knn_d) + t.out_offset;
        hipLaunchKernelGGL(knn_finish_kernel, dim3((t.emit_count + 3u) / 4u), dim3(256), 0, x->stream, p);
        HIP_TRY(x, hipGetLastError());
        HIP_TRY(x, record_done(x, x->stream));   // the finish reads the scratch the next search, on any stream, overwrites
    }
    HIP_TRY(x, hipMemcpyAsync(x->knn_h, x->knn_d, st.total(), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    memcpy(out_rows, st.rows(x->knn_h), st.rows_bytes);
    memcpy(out_scores, st.scores(x->knn_h), st.scores_bytes);
    memcpy(out_counts, st.counts(x->knn_h), st.counts_bytes);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

}  // extern "C"
