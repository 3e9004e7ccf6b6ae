// ticket_pool.h — the submit / collect bookkeeping of both transformer engines (embedder_run.hip, bert_run.hip): which
// submission slot a call gets, which execution context its ticket runs on, who may collect a ticket and when its slot is
// free again.  Header-only and device-free, so the engines and a CPU test (tests/ticket_pool_driver.cpp, under
// ThreadSanitizer and ASAN + UBSan) run the same functions.  The pool holds no payload: an engine keeps its pinned buffers
// and events in an array of its own, indexed by the slot numbers handed out here.  Every member is guarded by the ENGINE's
// mutex, which the caller holds around each call; only take_reserved gives it up, while it waits.
//   submit:  take / take_reserved -> (pack, enqueue) -> choose_context somewhere in between -> publish, LAST: a submit
//            that fails on the way leaves the slot with ticket 0, that is, free
//   collect: begin_collect -> wait for the device with the mutex released -> Collecting guard under the mutex again
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <mutex>

#include "batch_tables.h"

namespace cqs {

enum CollectCode { COLLECT_OK = 0, COLLECT_UNKNOWN, COLLECT_BUSY };

// N ticket slots (the public contract: up to N tickets in flight) + R slots reserved for blocking calls, which wait for one
// instead of failing when an index run holds every ticket.
template <int N, int R>
struct TicketPool {
    static constexpr int kNone = -1;
    struct Slot {
        uint64_t ticket = 0;       // 0 = free
        int kind = 0;              // what the ticket collects to (the engine's own numbering)
        int ctx = 0;               // execution context the ticket runs on
        bool collecting = false;   // a collect is waiting on this ticket: a second collector of the same ticket is refused
    };
    Slot slot[N + R];
    uint64_t next_ticket = 1;      // never reused
    int last_ctx = 1;              // context of the previous ticket (ties alternate)
    std::condition_variable cv;    // a slot was released

    int first_free(int lo, int hi) const {
        for (int i = lo; i < hi; ++i)
            if (slot[i].ticket == 0) return i;
        return kNone;
    }
    // A free ticket slot, or kNone: every one is in flight.
    int take() const { return first_free(0, N); }
    // A reserved slot, waiting (`lk`, the engine's mutex, released meanwhile) while other threads' blocking calls hold them.
    int take_reserved(std::unique_lock<std::mutex>& lk) {
        int i = kNone;
        cv.wait(lk, [&] { return (i = first_free(N, N + R)) != kNone; });
        return i;
    }

    struct Choice { int ctx; int load[2]; };   // load: tickets in flight per context before this one
    // The context slot i's ticket runs on: batch_tables.h's rule over the tickets in flight (slot i itself still has ticket
    // 0), or context 0 when the engine has a reason of its own (force0).
    Choice choose_context(int i, bool force0 = false) {
        Choice c{0, {0, 0}};
        for (const Slot& s : slot)
            if (s.ticket != 0) c.load[s.ctx]++;
        c.ctx = force0 ? 0 : pick_context(c.load[0], c.load[1], last_ctx);
        last_ctx = slot[i].ctx = c.ctx;
        return c;
    }

    uint64_t publish(int i, int kind) {
        slot[i].kind = kind;
        return slot[i].ticket = next_ticket++;
    }

    // One collector per ticket: the first gets the slot, a second one meanwhile is refused.
    CollectCode begin_collect(uint64_t ticket, int kind, int* i_out) {
        for (int i = 0; ticket != 0 && i < N + R; ++i)
            if (slot[i].ticket == ticket && slot[i].kind == kind) {
                if (slot[i].collecting) return COLLECT_BUSY;
                slot[i].collecting = true;
                *i_out = i;
                return COLLECT_OK;
            }
        return COLLECT_UNKNOWN;
    }
    void end_collect(int i) {
        slot[i].collecting = false;
        slot[i].ticket = 0;
        cv.notify_all();
    }
    // Whatever path leaves a collect: the slot is free again and waiters hear of it.  Made and destroyed under the mutex.
    struct Collecting {
        TicketPool& pool; int i;
        ~Collecting() { pool.end_collect(i); }
    };

    template <class F>
    void for_each_in_flight(F f) const {
        for (int i = 0; i < N + R; ++i)
            if (slot[i].ticket != 0) f(i);
    }
    int in_flight() const {
        int n = 0;
        for_each_in_flight([&](int) { ++n; });
        return n;
    }
};

}  // namespace cqs
