// Stand-alone driver for the ticket pool of the two transformer engines (cqs_amd/csrc/ticket_pool.h) over a toy payload, and
// for the weights' bf16 rounding (cqs_amd/csrc/engine_common.h, its device-free part).  Built once with -fsanitize=thread and
// once with -fsanitize=address,undefined and run on the CPU by tests/test_ticket_pool_cpu.py.  The toy engine is a mutex, a
// 3 + 1 pool and one payload per slot; a submit is take -> choose_context -> write the payload -> publish, a collect is
// begin_collect -> (the mutex released, as during the wait for the device) -> read the payload under the Collecting guard.
// Prints one line per scenario, fields separated by '|'.  argv[1]: rounds per thread of the storm (default 2000).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../cqs_amd/csrc/engine_common.h"
#include "../cqs_amd/csrc/ticket_pool.h"

using Clock = std::chrono::steady_clock;
using Pool = cqs::TicketPool<3, 1>;
using Lock = std::unique_lock<std::mutex>;
static const int TICKET = 1, BLOCKING = 2;          // the two kinds of the toy engine

struct Toy {
    std::mutex mu;                                  // the engine's mutex: guards the pool and the payloads
    Pool pool;
    struct { uint32_t thread, round; } payload[4];

    // kNone -> 0; otherwise the ticket.  `ctx`: the context it was given.
    uint64_t submit(Lock& lk, bool reserved, int kind, uint32_t thread, uint32_t round, int* ctx = nullptr, bool force0 = false, int* slot = nullptr) {
        const int i = reserved ? pool.take_reserved(lk) : pool.take();
        if (i == Pool::kNone) return 0;
        const int c = pool.choose_context(i, force0).ctx;
        if (ctx) *ctx = c;
        if (slot) *slot = i;
        payload[i] = {thread, round};
        return pool.publish(i, kind);
    }
    // Is the payload the ticket collects to (thread, round)?  -1: the collect was refused.
    int collect(uint64_t ticket, int kind, uint32_t thread, uint32_t round) {
        int i = 0;
        {
            Lock lk(mu);
            if (pool.begin_collect(ticket, kind, &i) != cqs::COLLECT_OK) return -1;
        }
        std::this_thread::yield();                  // (the wait for the device: others submit and collect meanwhile)
        Lock lk(mu);
        Pool::Collecting release{pool, i};
        return payload[i].thread == thread && payload[i].round == round;
    }
};

[[noreturn]] static void stuck(const char* what) {
    std::fprintf(stderr, "driver: gave up waiting for %s\n", what);
    std::exit(3);
}

static std::string join(const std::vector<uint64_t>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

static void fill_and_refuse() {
    Toy toy;
    Lock lk(toy.mu);
    std::vector<uint64_t> tickets;
    int slot_of_2 = -1, slot = -1;
    for (uint32_t r = 0; r < 3; ++r) {
        tickets.push_back(toy.submit(lk, false, TICKET, 0, r, nullptr, false, &slot));
        if (tickets.back() == 2) slot_of_2 = slot;
    }
    const int fourth = toy.pool.take();
    const int reserved = toy.pool.take_reserved(lk);               // free: does not wait
    lk.unlock();
    const int own = toy.collect(2, TICKET, 0, 1);
    lk.lock();
    const uint64_t next = toy.submit(lk, false, TICKET, 0, 3, nullptr, false, &slot);
    std::printf("fill|%s|%s|%d|%d|%llu|%d|%d\n", join(tickets).c_str(), fourth == Pool::kNone ? "none" : "slot", reserved, own,
                (unsigned long long)next, slot, slot_of_2);
}

static void context_sequences() {
    std::vector<uint64_t> a, b, c;
    int ctx = -1;
    {   // submit, submit, submit, collect the first, submit
        Toy toy;
        Lock lk(toy.mu);
        for (uint32_t r = 0; r < 3; ++r) { toy.submit(lk, false, TICKET, 0, r, &ctx); a.push_back((uint64_t)ctx); }
        lk.unlock();
        toy.collect(1, TICKET, 0, 0);
        lk.lock();
        toy.submit(lk, false, TICKET, 0, 3, &ctx); a.push_back((uint64_t)ctx);
    }
    {   // blocking calls, one at a time
        Toy toy;
        for (uint32_t r = 0; r < 4; ++r) {
            Lock lk(toy.mu);
            const uint64_t t = toy.submit(lk, true, BLOCKING, 0, r, &ctx); b.push_back((uint64_t)ctx);
            lk.unlock();
            toy.collect(t, BLOCKING, 0, r);
        }
    }
    {   // the engine forces context 0 for the second of three
        Toy toy;
        Lock lk(toy.mu);
        for (uint32_t r = 0; r < 3; ++r) { toy.submit(lk, false, TICKET, 0, r, &ctx, r == 1); c.push_back((uint64_t)ctx); }
    }
    std::printf("contexts|%s|%s|%s\n", join(a).c_str(), join(b).c_str(), join(c).c_str());
}

static void collect_rules() {
    Toy toy;
    Lock lk(toy.mu);
    const uint64_t t = toy.submit(lk, false, TICKET, 0, 0);
    static const char* name[] = {"ok", "unknown", "busy"};
    int i = -1;
    std::string s;
    s += name[toy.pool.begin_collect(0, TICKET, &i)];
    s += std::string(",") + name[toy.pool.begin_collect(t + 6, TICKET, &i)];      // never issued
    s += std::string(",") + name[toy.pool.begin_collect(t, BLOCKING, &i)];       // the other kind
    s += std::string(",") + name[toy.pool.begin_collect(t, TICKET, &i)];
    s += std::string(",") + name[toy.pool.begin_collect(t, TICKET, &i)];         // its first collector has not ended
    toy.pool.end_collect(i);
    s += std::string(",") + name[toy.pool.begin_collect(t, TICKET, &i)];
    std::printf("collect|%s|%d\n", s.c_str(), toy.pool.in_flight());
}

static void reserved_slot_two_threads() {
    Toy toy;
    uint64_t ta, tb = 0;
    { Lock lk(toy.mu); ta = toy.submit(lk, true, BLOCKING, 0, 0); }               // A holds the reserved slot: published, not collected
    std::atomic<bool> b_waits{false}, b_has_it{false};
    std::thread b([&] {
        Lock lk(toy.mu);
        b_waits.store(true);                                                     // (before the wait, under the mutex A needs to release the slot)
        tb = toy.submit(lk, true, BLOCKING, 1, 0);
        b_has_it.store(true);
    });
    // (polled, not cv.wait_for: older ThreadSanitizer runtimes do not know the timed wait's unlock and report a double lock)
    const auto give_up = Clock::now() + std::chrono::seconds(20);
    while (!b_waits.load()) {
        if (Clock::now() > give_up) stuck("thread B to reach the reserved slot");
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(50));
    const bool blocked = !b_has_it.load();
    const int own_a = toy.collect(ta, BLOCKING, 0, 0);                            // end_collect wakes B
    b.join();
    const int own_b = toy.collect(tb, BLOCKING, 1, 0);
    std::printf("reserved|%d|%llu|%llu|%d|%d|%d\n", blocked, (unsigned long long)ta, (unsigned long long)tb, own_a, own_b, toy.pool.in_flight());
}

static void storm(uint32_t rounds) {
    const uint32_t n_threads = 8;
    Toy toy;
    std::atomic<uint32_t> own{0}, ready{0};
    std::vector<std::vector<uint64_t>> tickets(n_threads);
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < n_threads; ++t)
        th.emplace_back([&, t] {
            ready.fetch_add(1);
            while (ready.load() < n_threads) std::this_thread::yield();          // everybody starts together
            const bool blocking = t % 2 == 0;                                    // even: the reserved slot, waited for; odd: a ticket slot, retried
            const int kind = blocking ? BLOCKING : TICKET;
            for (uint32_t r = 0; r < rounds; ++r) {
                uint64_t ticket = 0;
                while (ticket == 0) {
                    { Lock lk(toy.mu); ticket = toy.submit(lk, blocking, kind, t, r); }
                    if (ticket == 0) std::this_thread::yield();
                }
                tickets[t].push_back(ticket);
                own.fetch_add(toy.collect(ticket, kind, t, r) == 1 ? 1u : 0u);
            }
        });
    for (std::thread& t : th) t.join();
    std::set<uint64_t> distinct;
    for (const auto& v : tickets) distinct.insert(v.begin(), v.end());
    std::printf("storm|%u|%u|%zu|%d\n", n_threads * rounds, own.load(), distinct.size(), toy.pool.in_flight());
}

static void bf16_rounding() {
    const uint32_t in[] = {0x00000000u, 0x80000000u, 0x3F800000u, 0x3F808000u, 0x3F818000u, 0x7F800000u, 0x7FC00000u, 0x7F800001u};
    std::string s;
    for (uint32_t u : in) {
        float f;
        memcpy(&f, &u, 4);
        char hex[8];
        std::snprintf(hex, sizeof hex, "%04X", (unsigned)cqs::f32_to_bf16_bits(f));
        s += (s.empty() ? "" : ",") + std::string(hex);
    }
    std::printf("bf16|%s\n", s.c_str());
}

int main(int argc, char** argv) {
    fill_and_refuse();
    context_sequences();
    collect_rules();
    reserved_slot_two_threads();
    storm(argc > 1 ? (uint32_t)std::atoi(argv[1]) : 2000u);
    bf16_rounding();
    return 0;
}
