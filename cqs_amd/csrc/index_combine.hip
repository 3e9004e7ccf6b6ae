// index_combine.hip — the combining queue of cqs_hip_index_search (index.hip parks its single-query callers here) and the
// debug / bench hooks that exercise it: cqs_hip_debug_index_fail_next and the native client storms.
//
// Concurrent single-query callers of cqs_hip_index_search (the daemon's client threads, src/cli/watch/daemon.rs:273,
// on one Arc<dyn VectorIndex>) used to queue on the handle mutex for one 0.5 ms pass EACH, although one pass scans up to
// 8 queries for 0.50-0.54 ms.  Now a caller parks its query; whoever leads next takes the device, gathers
// the parked queries with the same (k, mode, threshold) and runs them as ONE block of gemv passes; every caller gets
// exactly the bits a lone call would have produced (search_host_locked, gemv_only).  Callers with a bitset park too, on a
// single-device handle, and form blocks of their own (search_filtered_locked: one bitset per query); so do the single-query
// callers of cqs_hip_index_search_tagged (index_tags.hip; search_tagged_locked: one tag filter per query, the block's
// bitsets written by one kernel).  The three classes never share a block.  Multi-query blocks, and bitsets on a sharded
// handle, keep the serial path.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "abi_guard.h"
#include "index_internal.h"

namespace cqs_idx {

// May the two share a block: the same (k, mode, threshold) and the same class - unfiltered, host bitset or tag filter.
// A closure type, so that the queue's loops inline it.
static constexpr auto same_params = [](const cqs_combine_req* a, const cqs_combine_req* b) {
    return a->k == b->k && a->mode == b->mode && memcmp(&a->thr, &b->thr, sizeof(float)) == 0 && !a->keep == !b->keep &&
           !a->allow == !b->allow;
};

// One sealed block on a single-device handle: the device mutex is taken here, for the pass alone.
static int32_t combine_run_single(cqs_hip_index* x, cqs_combine_req* const* batch, uint32_t nb) {
    std::lock_guard<std::mutex> dev(x->mu);       // (other entry points - device API searches, extend, save - order with the pass here)
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    cqs_combine_req rq[kCombineCap];
    for (uint32_t i = 0; i < nb; ++i) rq[i] = *batch[i];
    // gemv passes only: each caller gets its lone call's bits.  CQS_HIP_COMBINE_BITS=relaxed (opt-in, read at create) lets a
    // block of >= 9 callers take the matrix-core kernel instead - 32 queries per corpus sweep instead of 8, scores in another
    // summation order (|delta| <= 2e-6 on unit vectors, inside the parity tolerance; the reference's GPU backend promises no
    // bit-reproducibility across calls either, src/cagra.rs:443-492)
    if (batch[0]->keep) return search_filtered_locked(x, rq, nb, batch[0]->k, batch[0]->mode, batch[0]->thr);
    if (batch[0]->allow) {
        // an extend between parking and this pass may have added rows without a tag: every caller of the block is refused
        // as a call that came after the extend is (INVALID, not poisoned)
        const int32_t rc = tagged_ready(x, batch[0]->allow, "search_tagged");
        return rc != CQS_HIP_OK ? rc : search_tagged_locked(x, rq, nb, batch[0]->k, batch[0]->mode, batch[0]->thr);
    }
    const bool gemv_only = !(x->combine_relaxed && nb >= cqs::kMfmaMinQueries);
    return search_host_locked(x, rq, nb, batch[0]->k, nullptr, batch[0]->mode, batch[0]->thr, gemv_only);
}

// The protocol - who leads, the wait for stragglers, the seal, who gets which return code - is combine_queue.h's.
int32_t combine_search(cqs_hip_index* x, cqs_combine_req& r) {
    return x->cq.search(r, same_params, [x](cqs_combine_req* const* batch, uint32_t nb) {
        int32_t rc = CQS_HIP_OK;
        try {
            rc = x->sh ? cqs_sharded::search_combined(x, batch, nb) : combine_run_single(x, batch, nb);
        } catch (const std::bad_alloc&) {
            rc = fail(x, CQS_HIP_ERR_NOMEM, "search: out of host memory");
        } catch (...) {
            rc = fail(x, CQS_HIP_ERR_INVALID, "search: unexpected C++ exception");
        }
        (batch[0]->keep ? x->stat_fpasses : batch[0]->allow ? x->stat_tpasses : x->stat_passes).fetch_add(1, std::memory_order_relaxed);
        (batch[0]->keep ? x->stat_fqueries : batch[0]->allow ? x->stat_tqueries : x->stat_queries).fetch_add(nb, std::memory_order_relaxed);
        const bool poisoned = x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire);
        return cqs_combine::Outcome{rc, poisoned};
    });
}

}  // namespace cqs_idx

extern "C" {

// Test hook (not part of the public header): the next host search on this handle fails as a device error would
// (the handle ends up poisoned) - how tests/test_threads_gpu.py reaches the combining queue's failure path.
void cqs_hip_debug_index_fail_next(cqs_hip_index* x) CQS_ABI_TRY {
    if (x) x->inject_fail.store(1, std::memory_order_release);
} CQS_ABI_CATCH_VOID

// Bench aid (not part of the public header): combine_queue.h's client storm over the PUBLIC blocking entry point
// cqs_hip_index_search, one query of the `n_queries` host rows per call.  out_rows / out_scores / out_counts
// [n_queries, k] / [n_queries] receive each query's last answer.  Returns wall seconds, < 0 on a failed call.
// keep_bitsets (nullable): the call for query qi passes keep_bitsets + qi * keep_stride_words.
static double client_storm(cqs_hip_index* x, const float* queries, uint32_t n_queries, uint32_t dim, uint32_t k,
                           const uint32_t* keep_bitsets, uint64_t keep_stride_words, uint32_t n_threads, uint32_t per_thread,
                           uint64_t* out_rows, float* out_scores, uint32_t* out_counts) {
    if (!x || !queries || !n_queries || !n_threads || !out_rows || !out_scores || !out_counts) return -1.0;
    return cqs_combine::client_storm(n_threads, per_thread, n_queries, [=](uint32_t qi) {
        return cqs_hip_index_search(x, queries + (size_t)qi * dim, 1, dim, k,
                                    keep_bitsets ? keep_bitsets + (size_t)qi * keep_stride_words : nullptr, CQS_HIP_MODE_RAW, 0.f,
                                    out_rows + (size_t)qi * k, out_scores + (size_t)qi * k, out_counts + qi);
    });
}

double cqs_hip_debug_client_storm(cqs_hip_index* x, const float* queries, uint32_t n_queries, uint32_t dim, uint32_t k,
                                  uint32_t n_threads, uint32_t per_thread, uint64_t* out_rows, float* out_scores,
                                  uint32_t* out_counts) CQS_ABI_TRY {
    return client_storm(x, queries, n_queries, dim, k, nullptr, 0, n_threads, per_thread, out_rows, out_scores, out_counts);
} CQS_ABI_CATCH_VAL(-1.0)

// The same storm with one bitset per query row.
double cqs_hip_debug_client_storm_filtered(cqs_hip_index* x, const float* queries, uint32_t n_queries, uint32_t dim, uint32_t k,
                                           const uint32_t* keep_bitsets, uint64_t keep_stride_words, uint32_t n_threads,
                                           uint32_t per_thread, uint64_t* out_rows, float* out_scores,
                                           uint32_t* out_counts) CQS_ABI_TRY {
    if (!keep_bitsets) return -1.0;
    return client_storm(x, queries, n_queries, dim, k, keep_bitsets, keep_stride_words, n_threads, per_thread, out_rows,
                        out_scores, out_counts);
} CQS_ABI_CATCH_VAL(-1.0)

// The same storm over the PUBLIC cqs_hip_index_search_tagged, one tag filter (32 words) per query row.
double cqs_hip_debug_client_storm_tagged(cqs_hip_index* x, const float* queries, uint32_t n_queries, uint32_t dim, uint32_t k,
                                         const uint32_t* allows, uint32_t n_threads, uint32_t per_thread, uint64_t* out_rows,
                                         float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    if (!x || !queries || !allows || !n_queries || !n_threads || !out_rows || !out_scores || !out_counts) return -1.0;
    return cqs_combine::client_storm(n_threads, per_thread, n_queries, [=](uint32_t qi) {
        return cqs_hip_index_search_tagged(x, queries + (size_t)qi * dim, 1, dim, k, allows + (size_t)qi * 32u, CQS_HIP_MODE_RAW, 0.f,
                                           out_rows + (size_t)qi * k, out_scores + (size_t)qi * k, out_counts + qi);
    });
} CQS_ABI_CATCH_VAL(-1.0)

}  // extern "C"
