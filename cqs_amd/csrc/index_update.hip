// index_update.hip — cqs_hip_index_update: stored rows of the resident corpus rewritten in place, the shadow's copies of
// them included.  The reference re-embeds chunks it already holds and writes the vectors back under the same ids
// (Store::update_embeddings_batch, src/store/chunks/crud.rs:349-480; upsert_chunks_batch's ON CONFLICT(id) DO UPDATE,
// src/store/chunks/async_helpers.rs:314-330); behind remove + extend that would move everything behind the first such row
// and renumber it.  Here the row stays where it is: the new vectors are staged in plan order (update_host.h), and one wave
// per row scatters each into d_rows and converts it into the copies the handle holds, with the build kernels' own per-row
// bodies (shadow_build_device.h).  DESIGN.md §3.15.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "abi_guard.h"
#include "index_internal.h"
#include "scan_i8.h"
#include "shadow_build_device.h"
#include "update_host.h"

namespace cqs_idx {

struct UpdateParams {
    const float* stage;      // [rows, dim] the new rows, in plan order
    const uint32_t* dst;     // [rows] the local row each of them replaces, ascending, no row twice
    uint32_t rows, dim;
    float* d_rows;           // the corpus
    uint16_t* bf16;          // the shadow's copies (null: the handle does not hold that one) ...
    int8_t* i8;
    float* i8_scale;
    double gamma, gamma8;    // ... and what their build kernels are launched with
    unsigned long long* stats;
    unsigned long long* stats8;
};

// One wave per updated row (grid-stride, as the two build kernels).  The row comes from the staging buffer, never from
// d_rows, so nothing here reads what it writes; no two waves share a destination (the plan refuses a row named twice).
// The f32 copy moves 16 bytes per lane and step (dim % 4 == 0, rows of both buffers 16-byte aligned); the shadow bodies
// mind their own tails (128 components a step for bf16, 256 for int8).  Which copies exist is uniform across the launch.
__global__ __launch_bounds__(256) void row_update_kernel(UpdateParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < p.rows; r += waves) {
        const float* __restrict__ xp = p.stage + (size_t)r * p.dim;
        const size_t d = p.dst[r];
        float* __restrict__ fp = p.d_rows + d * p.dim;
        for (uint32_t i = lane * 4u; i < p.dim; i += 256u) *(cqs::f4*)(fp + i) = *(const cqs::f4*)(xp + i);
        if (p.bf16) cqs::shadow_build_row(xp, p.bf16 + d * p.dim, p.dim, p.gamma, p.stats, (int)lane);
        if (p.i8) cqs::i8_build_row(xp, p.i8 + d * p.dim, p.i8_scale + d, p.dim, p.gamma8, p.stats8, lane);
    }
}

namespace {

// The staging pair holds at least `bytes` (regrown, never past what one pass may stage).  Nothing is touched on failure.
int32_t ensure_stage(cqs_hip_index* x, uint64_t bytes) {
    if (bytes <= x->upd_bytes) return CQS_HIP_OK;
    update_free(x);
    hipError_t e = hipHostMalloc(&x->upd_h, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&x->upd_d, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        update_free(x);
        return fail(x, e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, "update: staging buffer", e);
    }
    x->upd_bytes = bytes;
    return CQS_HIP_OK;
}

}  // namespace

void update_free(cqs_hip_index* x) {
    if (x->upd_h) (void)hipHostFree(x->upd_h);
    if (x->upd_d) (void)hipFree(x->upd_d);
    x->upd_h = x->upd_d = nullptr;
    x->upd_bytes = 0;
}

// Planned entries order[0, count) of one single-device index: vectors[order[j]] replaces its local row local[order[j]] -
// local_off.  Caller holds x->mu, has found the handle neither poisoned nor borrowing, and has checked the plan against
// this index.  An allocation that fails leaves the index untouched (NOMEM); any failure after the first pass is queued
// leaves some rows written: the handle is poisoned.
int32_t update_entries(cqs_hip_index* x, const uint32_t* local, uint64_t local_off, const uint64_t* order, uint64_t count,
                       const float* vectors) {
    if (count == 0) return CQS_HIP_OK;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // a search enqueued on a caller stream may still read the rows
    const uint32_t dim = x->dim;
    const size_t row_bytes = (size_t)dim * sizeof(float);
    const uint64_t budget = x->update_budget_rows ? x->update_budget_rows : cqs_update::budget_rows(dim);
    const std::vector<cqs_update::Pass> passes = cqs_update::cut_passes(count, budget);
    const int32_t rc = ensure_stage(x, std::min(count, budget) * (row_bytes + sizeof(uint32_t)));
    if (rc != CQS_HIP_OK) return rc;
    UpdateParams p{};
    p.dim = dim;
    p.d_rows = x->d_rows;
    const ShadowBuffers sb = shadow_buffers(x);
    p.bf16 = sb.bf16;
    p.i8 = sb.i8;
    p.i8_scale = sb.i8_scale;
    if (sb.bf16) {
        p.gamma = cqs::shadow_gamma(dim);
        p.gamma8 = cqs::i8_gamma(dim);
        const int32_t brc = shadow_update_begin(x, &p.stats, &p.stats8);
        if (brc != CQS_HIP_OK) return brc;
    }
    for (const cqs_update::Pass& ps : passes) {
        // the pass's rows, then its destination list, in one block: one copy, and the list stays 4-byte aligned
        float* hv = (float*)x->upd_h;
        uint32_t* hd = (uint32_t*)((char*)x->upd_h + ps.count * row_bytes);
        for (size_t j = 0; j < ps.count; ++j) {
            const uint64_t entry = order[ps.first + j];
            memcpy(hv + j * dim, vectors + entry * dim, row_bytes);
            hd[j] = (uint32_t)(local[entry] - local_off);
        }
        HIP_TRY(x, hipMemcpyAsync(x->upd_d, x->upd_h, ps.count * (row_bytes + sizeof(uint32_t)), hipMemcpyHostToDevice, x->stream));
        p.stage = (const float*)x->upd_d;
        p.dst = (const uint32_t*)((const char*)x->upd_d + ps.count * row_bytes);
        p.rows = (uint32_t)ps.count;
        const uint64_t blocks = (ps.count + 3u) / 4u;
        hipLaunchKernelGGL(row_update_kernel, dim3((uint32_t)(blocks < 8192u ? blocks : 8192u)), dim3(256), 0, x->stream, p);
        HIP_TRY(x, hipGetLastError());
        HIP_TRY(x, hipStreamSynchronize(x->stream));   // the next pass restages the same pinned block
    }
    return sb.bf16 ? shadow_update_end(x) : CQS_HIP_OK;
}

}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

int32_t cqs_hip_index_update(cqs_hip_index* x, const uint64_t* rows, const float* vectors, uint64_t m,
                             uint64_t* out_updated) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    if (out_updated) *out_updated = 0;
    if (x->sh) return cqs_sharded::update(x, rows, vectors, m, out_updated);
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (x->borrow) return fail(x, CQS_HIP_ERR_INVALID, "update: index borrows its rows");
    std::vector<uint32_t> local;
    std::vector<uint64_t> order;
    const char* why = "";
    const cqs_update::Plan plan = cqs_update::plan_update(rows, vectors, m, x->row_base, x->n, &local, &order, &why);
    if (plan == cqs_update::Plan::Invalid) return fail(x, CQS_HIP_ERR_INVALID, (std::string("update: ") + why).c_str());
    if (plan == cqs_update::Plan::Nothing) return CQS_HIP_OK;
    const int32_t rc = update_entries(x, local.data(), 0, order.data(), m, vectors);
    if (rc == CQS_HIP_OK && out_updated) *out_updated = m;
    return rc;
} CQS_ABI_CATCH(x)

// Test hook (not part of the public header): the next updates on this handle (on every shard of a row-sharded one) cut
// their passes at `rows` rows instead of at the staging buffer's byte budget (0 = the byte budget again).
void cqs_hip_debug_index_update_budget(cqs_hip_index* x, uint64_t rows) CQS_ABI_TRY {
    if (!x) return;
    std::lock_guard<std::mutex> g(x->mu);
    if (rows > cqs_update::budget_rows(x->dim)) rows = 0;   // (never past the byte budget: the staging buffer is sized by it)
    x->update_budget_rows = rows;
    if (x->sh) cqs_sharded::update_budget(x, rows);
} CQS_ABI_CATCH_VOID

}  // extern "C"
