// index_combine.hip — the combining queue of cqs_hip_index_search (index.hip parks its single-query callers here) and the
// debug / bench hooks that exercise it: cqs_hip_debug_index_fail_next and the native client storms.
//
// Concurrent single-query callers of cqs_hip_index_search (the daemon's client threads, src/cli/watch/daemon.rs:273,
// on one Arc<dyn VectorIndex>) used to queue on the handle mutex for one 0.5 ms pass EACH, although one pass scans up to
// 8 queries for 0.50-0.54 ms.  Now a caller parks its query; whoever leads next takes the device, gathers
// the parked queries with the same (k, mode, threshold) and runs them as ONE block of gemv passes; every caller gets
// exactly the bits a lone call would have produced (search_host_locked, gemv_only).  Callers with a bitset park too, on a
// single-device handle, and form blocks of their own (search_filtered_locked: one bitset per query).  Multi-query blocks,
// and bitsets on a sharded handle, keep the serial path.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <thread>

#include "abi_guard.h"
#include "index_internal.h"

namespace cqs_idx {

static bool same_params(const cqs_combine_req* a, const cqs_combine_req* b) {   // (callers with a bitset form blocks of their own)
    return a->k == b->k && a->mode == b->mode && memcmp(&a->thr, &b->thr, sizeof(float)) == 0 && !a->keep == !b->keep;
}
static uint32_t count_like_front(const cqs_hip_index* x) {
    uint32_t n = 0;
    for (const cqs_combine_req* r : x->pending) n += same_params(r, x->pending.front()) ? 1u : 0u;
    return n;
}

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
    const bool gemv_only = !(x->combine_relaxed && nb >= cqs::kMfmaMinQueries);
    return search_host_locked(x, rq, nb, batch[0]->k, nullptr, batch[0]->mode, batch[0]->thr, gemv_only);
}

// Lead one pass.  `lk` holds cmu on entry and on exit; x->leader is set by the caller.
static void combine_lead(cqs_hip_index* x, std::unique_lock<std::mutex>& lk) {
    // Stragglers: if recent passes carried more callers than are parked now, their threads are on their way back (a
    // caller needs some tens of microseconds between getting its answer and asking again).  Waiting for them costs a
    // little once; scanning without them costs them a whole pass.  The window is anchored at the END OF THE PREVIOUS
    // PASS (round 5), not at this leader's arrival: a caller that comes alone combine_wait_us or more after a burst does
    // not wait at all (round 4: it paid the full wait once), and a lone caller never waits (expect is 1).  No device
    // mutex is held meanwhile (round 4 spun inside x->mu): there is one leader at a time, so the device is only ever
    // contended by the other entry points, and those must not queue behind a spin.
    const uint32_t target = x->expect < kCombineCap ? x->expect : kCombineCap;
    if (x->combine_wait_us && count_like_front(x) < target) {
        const auto t_end = x->last_pass_end + std::chrono::microseconds(x->combine_wait_us);
        while (count_like_front(x) < target && std::chrono::steady_clock::now() < t_end) {
            lk.unlock();
            for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
            lk.lock();
        }
    }
    // seal the block: the oldest request and everything parked with its parameters, oldest first
    cqs_combine_req* batch[kCombineCap];
    uint32_t nb = 0, left_like = 0;
    {
        const cqs_combine_req head = *x->pending.front();
        std::deque<cqs_combine_req*> keep;
        for (cqs_combine_req* r : x->pending) {
            if (same_params(r, &head)) {
                if (nb < kCombineCap) { batch[nb++] = r; continue; }
                ++left_like;
            }
            keep.push_back(r);
        }
        x->pending.swap(keep);
        x->n_pending.store((uint32_t)x->pending.size(), std::memory_order_relaxed);
    }
    x->expect = nb + left_like;                    // what this pass saw (>= 1)
    lk.unlock();

    int32_t rc = CQS_HIP_OK;
    try {
        rc = x->sh ? cqs_sharded::search_combined(x, batch, nb) : combine_run_single(x, batch, nb);
    } catch (const std::bad_alloc&) {
        rc = fail(x, CQS_HIP_ERR_NOMEM, "search: out of host memory");
    } catch (...) {
        rc = fail(x, CQS_HIP_ERR_INVALID, "search: unexpected C++ exception");
    }
    (batch[0]->keep ? x->stat_fpasses : x->stat_passes).fetch_add(1, std::memory_order_relaxed);
    (batch[0]->keep ? x->stat_fqueries : x->stat_queries).fetch_add(nb, std::memory_order_relaxed);
    const bool poisoned = x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire);

    lk.lock();
    x->last_pass_end = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < nb; ++i) {
        // the call that met the failure reports it; whoever rode along on a handle that is now poisoned gets what
        // any later call gets (src/cagra.rs:486-490)
        batch[i]->rc = (rc != CQS_HIP_OK && i > 0 && poisoned) ? CQS_HIP_ERR_POISONED : rc;
        batch[i]->done = true;
    }
    if (poisoned) {                                // nobody stays parked on a dead handle
        for (cqs_combine_req* r : x->pending) { r->rc = CQS_HIP_ERR_POISONED; r->done = true; }
        x->pending.clear();
        x->n_pending.store(0, std::memory_order_relaxed);
    } else if (!x->pending.empty()) {
        // callers that arrived during this pass with the same parameters could have ridden along: tell the next leader
        uint32_t like = 0;
        for (const cqs_combine_req* r : x->pending) like += same_params(r, batch[0]) ? 1u : 0u;
        if (nb + like > x->expect) x->expect = nb + like;
    }
}

int32_t combine_search(cqs_hip_index* x, cqs_combine_req& r) {
    std::unique_lock<std::mutex> lk(x->cmu);
    x->pending.push_back(&r);
    x->n_pending.store((uint32_t)x->pending.size(), std::memory_order_relaxed);
    while (!r.done) {
        if (!x->leader) {
            x->leader = true;
            struct Reset {                             // whatever happens in there, the next caller can lead
                cqs_hip_index* x; std::unique_lock<std::mutex>& lk;
                ~Reset() { if (!lk.owns_lock()) lk.lock(); x->leader = false; x->ccv.notify_all(); }
            } reset{x, lk};
            combine_lead(x, lk);
        } else {
            x->ccv.wait(lk);
        }
    }
    return r.rc;
}

}  // namespace cqs_idx

extern "C" {

// Test hook (not part of the public header): the next host search on this handle fails as a device error would
// (the handle ends up poisoned) - how tests/test_threads_gpu.py reaches the combining queue's failure path.
void cqs_hip_debug_index_fail_next(cqs_hip_index* x) CQS_ABI_TRY {
    if (x) x->inject_fail.store(1, std::memory_order_release);
} CQS_ABI_CATCH_VOID

// Bench aid (not part of the public header): `n_threads` native threads, each calling the PUBLIC blocking entry point
// cqs_hip_index_search `per_thread` times with one query at a time (thread t asks queries t, t + n_threads, ... of the
// `n_queries` host rows, round and round) - what the reference's daemon does with one thread per client
// (src/cli/watch/daemon.rs:273), without a Python interpreter lock between the callers.  out_rows / out_scores /
// out_counts [n_queries, k] / [n_queries] receive each query's last answer.  Returns wall seconds, < 0 on a failed call.
// keep_bitsets (nullable): the call for query qi passes keep_bitsets + qi * keep_stride_words.
static double client_storm(cqs_hip_index* x, const float* queries, uint32_t n_queries, uint32_t dim, uint32_t k,
                           const uint32_t* keep_bitsets, uint64_t keep_stride_words, uint32_t n_threads, uint32_t per_thread,
                           uint64_t* out_rows, float* out_scores, uint32_t* out_counts) {
    if (!x || !queries || !n_queries || !n_threads || !out_rows || !out_scores || !out_counts) return -1.0;
    std::atomic<int32_t> bad{0};
    std::atomic<uint32_t> ready{0};
    std::atomic<bool> go{false};
    std::vector<std::thread> th;
    th.reserve(n_threads);
    for (uint32_t t = 0; t < n_threads; ++t)
        th.emplace_back([&, t]() {
            ready.fetch_add(1);
            while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
            uint32_t qi = t % n_queries;
            for (uint32_t i = 0; i < per_thread; ++i) {
                const int32_t rc = cqs_hip_index_search(x, queries + (size_t)qi * dim, 1, dim, k,
                                                        keep_bitsets ? keep_bitsets + (size_t)qi * keep_stride_words : nullptr,
                                                        CQS_HIP_MODE_RAW, 0.f, out_rows + (size_t)qi * k, out_scores + (size_t)qi * k,
                                                        out_counts + qi);
                if (rc != CQS_HIP_OK) { bad.store(rc); break; }
                qi = (qi + n_threads) % n_queries;
            }
        });
    while (ready.load() < n_threads) std::this_thread::yield();
    const auto t0 = std::chrono::steady_clock::now();
    go.store(true, std::memory_order_release);
    for (std::thread& t : th) t.join();
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return bad.load() ? -1.0 : el;
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

}  // extern "C"
