// combine_queue.h — the combining queue of the blocking single-query searches, and the client storm that exercises it.
// Concurrent callers park their requests; one of them leads: it seals a block of like requests, runs it as one pass and
// hands every caller its own answer.  The dense index (index_combine.hip) and the sparse index (sparse_index.hip) each
// supply the request type, the block size, which requests may share a block, and what running a block means.
// Plain C++ over the standard library, no HIP, no handle: tests/combine_queue_driver.cpp runs it under ThreadSanitizer
// and ASAN + UBSan (tests/test_combine_queue_cpu.py).
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/cqs_hip.h"

namespace cqs_combine {

struct Outcome { int32_t rc; bool poisoned; };     // of one sealed block: its return code, and whether the handle is dead now

// Req lives on its caller's stack and has `int32_t rc; bool done;` (both guarded by `mu`); Cap: requests per block.
template <class Req, uint32_t Cap>
struct Queue {
    std::mutex mu;                                  // orders the queue only; the device work runs under the handle's own mutex
    std::condition_variable cv;
    std::deque<Req*> pending;
    bool leader = false;                            // somebody is collecting / running a block
    uint32_t expect = 1;                            // like callers the next block should expect (what recent passes saw)
    uint32_t wait_us = 100;                         // how long after the END of a pass the next leader waits for the callers that pass carried
    std::chrono::steady_clock::time_point last_pass_end{};   // (epoch until the first pass: nobody waits)

    // Park r and return its answer.  same(a, b): may the two requests share a block.  run(batch, nb) -> Outcome: called
    // by the leader with `mu` released; takes whatever device lock it needs; does not throw.
    template <class Same, class Run>
    int32_t search(Req& r, Same same, Run run) {
        std::unique_lock<std::mutex> lk(mu);
        pending.push_back(&r);
        while (!r.done) {
            if (!leader) {
                leader = true;
                struct Reset {                      // whatever happens in there, the next caller can lead
                    Queue* q; std::unique_lock<std::mutex>& lk;
                    ~Reset() { if (!lk.owns_lock()) lk.lock(); q->leader = false; q->cv.notify_all(); }
                } reset{this, lk};
                lead(lk, same, run);
            } else {
                cv.wait(lk);
            }
        }
        return r.rc;
    }

    size_t parked() {                               // (tests)
        std::lock_guard<std::mutex> g(mu);
        return pending.size();
    }

private:
    template <class Same>
    uint32_t count_like(const Req* head, Same& same) const {
        uint32_t n = 0;
        for (const Req* r : pending) n += same(r, head) ? 1u : 0u;
        return n;
    }

    // Lead one pass.  `lk` holds mu on entry and on exit; `leader` is set by the caller.
    template <class Same, class Run>
    void lead(std::unique_lock<std::mutex>& lk, Same& same, Run& run) {
        // Stragglers: if recent passes carried more callers than are parked now, their threads are on their way back (a
        // caller needs some tens of microseconds between getting its answer and asking again).  Waiting for them costs a
        // little once; scanning without them costs them a whole pass.  The window is anchored at the END OF THE PREVIOUS
        // PASS (round 5), not at this leader's arrival: a caller that comes alone wait_us or more after a burst does
        // not wait at all (round 4: it paid the full wait once), and a lone caller never waits (expect is 1).  No device
        // mutex is held meanwhile (round 4 spun inside it): there is one leader at a time, so the device is only ever
        // contended by the other entry points, and those must not queue behind a spin.
        const uint32_t target = expect < Cap ? expect : Cap;
        if (wait_us && count_like(pending.front(), same) < target) {
            const auto t_end = last_pass_end + std::chrono::microseconds(wait_us);
            while (count_like(pending.front(), same) < target && std::chrono::steady_clock::now() < t_end) {
                lk.unlock();
                for (int i = 0; i < 64; ++i) __builtin_ia32_pause();
                lk.lock();
            }
        }
        // seal the block: the oldest request and everything parked that is like it, oldest first
        Req* batch[Cap];
        uint32_t nb = 0, left_like = 0;
        {
            const Req* head = pending.front();
            std::deque<Req*> keep;
            for (Req* r : pending) {
                if (same(r, head)) {
                    if (nb < Cap) { batch[nb++] = r; continue; }
                    ++left_like;
                }
                keep.push_back(r);
            }
            pending.swap(keep);
        }
        expect = nb + left_like;                    // what this pass saw (>= 1)
        lk.unlock();

        const Outcome o = run(batch, nb);

        lk.lock();
        last_pass_end = std::chrono::steady_clock::now();
        for (uint32_t i = 0; i < nb; ++i) {
            // the call that met the failure reports it; whoever rode along on a handle that is now poisoned gets what
            // any later call gets (src/cagra.rs:486-490)
            batch[i]->rc = (o.rc != CQS_HIP_OK && i > 0 && o.poisoned) ? CQS_HIP_ERR_POISONED : o.rc;
            batch[i]->done = true;
        }
        if (o.poisoned) {                           // nobody stays parked on a dead handle
            for (Req* r : pending) { r->rc = CQS_HIP_ERR_POISONED; r->done = true; }
            pending.clear();
        } else if (!pending.empty()) {
            // callers that arrived during this pass and are like its block could have ridden along: tell the next leader
            const uint32_t like = count_like(batch[0], same);
            if (nb + like > expect) expect = nb + like;
        }
    }
};

// CQS_HIP_COMBINE_WAIT_US (microseconds, read at create; 0 = never wait), `unset` when the variable is not there.
inline uint32_t wait_us_from_env(uint32_t unset = 100) {
    const char* e = getenv("CQS_HIP_COMBINE_WAIT_US");
    return e ? (uint32_t)strtoul(e, nullptr, 10) : unset;
}

// The client storm of the debug / bench entry points: n_threads native threads start together, and thread t calls
// one_call(qi) per_thread times with qi = t, t + n_threads, ... (mod n_queries), round and round - one thread per client
// as the reference's daemon has them (src/cli/watch/daemon.rs:273), without a Python interpreter lock between the
// callers.  A call that does not return CQS_HIP_OK ends its thread.  Returns wall seconds, < 0 after a failed call.
template <class Call>
double client_storm(uint32_t n_threads, uint32_t per_thread, uint32_t n_queries, Call one_call) {
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
                const int32_t rc = one_call(qi);
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

}  // namespace cqs_combine
