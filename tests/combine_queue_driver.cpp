// Stand-alone driver for the combining queue (cqs_amd/csrc/combine_queue.h) over a toy request.  Built once with
// -fsanitize=thread and once with -fsanitize=address,undefined and run on the CPU by tests/test_combine_queue_cpu.py.
// The fake `run` records every block it is given and answers payload * 3 + key; a latch can hold one run so that the main
// thread decides who is parked when the next block is sealed.  Prints one line per scenario, fields separated by '|'.
#include <cstdio>
#include <string>

#include "../cqs_amd/csrc/combine_queue.h"

using Clock = std::chrono::steady_clock;
using cqs_combine::Outcome;

struct Req { uint32_t key, payload; uint32_t* out; int32_t rc; bool done; };
using Queue = cqs_combine::Queue<Req, 4>;
static const uint32_t A = 1, B = 2, C = 3;

static bool same_key(const Req* a, const Req* b) { return a->key == b->key; }
static uint32_t answer(uint32_t key, uint32_t payload) { return payload * 3 + key; }
static int64_t micros(Clock::duration d) { return std::chrono::duration_cast<std::chrono::microseconds>(d).count(); }

static const char* rc_name(int32_t rc) {
    return rc == CQS_HIP_OK ? "OK" : rc == CQS_HIP_ERR_DEVICE ? "DEVICE" : rc == CQS_HIP_ERR_NOMEM ? "NOMEM"
         : rc == CQS_HIP_ERR_POISONED ? "POISONED" : "?";
}

[[noreturn]] static void stuck(const char* what) {
    std::fprintf(stderr, "driver: gave up waiting for %s\n", what);
    std::exit(3);
}

struct Block {
    std::vector<Req> members;       // copies, in the order the queue sealed them
    uint32_t expect;                // the queue's `expect` while the block runs
    Clock::time_point at;           // when `run` was entered
};

struct Rig {
    Queue q;
    std::mutex mu;                  // guards everything below
    std::condition_variable cv;
    std::vector<Block> blocks;
    bool hold_next = false, holding = false, released = false;
    uint32_t fail_key = 0;          // blocks of this key fail with `fail`
    Outcome fail{CQS_HIP_OK, false};

    Outcome run(Req* const* batch, uint32_t nb) {
        Block b{{}, 0, Clock::now()};
        for (uint32_t i = 0; i < nb; ++i) b.members.push_back(*batch[i]);
        { std::lock_guard<std::mutex> g(q.mu); b.expect = q.expect; }
        std::unique_lock<std::mutex> l(mu);
        blocks.push_back(b);
        if (hold_next) {
            hold_next = false;
            holding = true;
            cv.wait(l, [&] { return released; });
            released = holding = false;
        }
        if (fail_key && batch[0]->key == fail_key) return fail;
        for (uint32_t i = 0; i < nb; ++i) *batch[i]->out = answer(batch[i]->key, batch[i]->payload);
        return Outcome{CQS_HIP_OK, false};
    }
    int32_t call(uint32_t key, uint32_t payload, uint32_t* out) {
        Req r{key, payload, out, 0, false};
        return q.search(r, same_key, [this](Req* const* batch, uint32_t nb) { return run(batch, nb); });
    }
    // One caller that is held inside `run`: everybody who calls before release() parks behind it.
    std::thread hold(uint32_t key, uint32_t payload, uint32_t* out, int32_t* rc) {
        { std::lock_guard<std::mutex> g(mu); hold_next = true; }
        std::thread t([=] { *rc = call(key, payload, out); });
        // (polled, not cv.wait_for: older ThreadSanitizer runtimes do not know the timed wait's unlock and report a double lock)
        const auto give_up = Clock::now() + std::chrono::seconds(20);
        for (std::unique_lock<std::mutex> l(mu); !holding; l.lock()) {
            l.unlock();
            if (Clock::now() > give_up) stuck("the held run");
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        return t;
    }
    void release() {
        { std::lock_guard<std::mutex> g(mu); released = true; }
        cv.notify_all();
    }
    void wait_parked(size_t n) {
        const auto give_up = Clock::now() + std::chrono::seconds(20);
        while (q.parked() != n) {
            if (Clock::now() > give_up) stuck("a caller to park");
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
    }
    std::string blocks_text() {
        std::lock_guard<std::mutex> g(mu);
        std::string s;
        for (const Block& b : blocks) {
            if (!s.empty()) s += ';';
            for (size_t i = 0; i < b.members.size(); ++i)
                s += (i ? "," : "") + std::string(1, "?ABC"[b.members[i].key]) + std::to_string(b.members[i].payload);
        }
        return s;
    }
};

// A held first caller (payload 0), then one caller per key parked in that order (payloads 1, 2, ...), then the release.
struct Parked {
    std::vector<uint32_t> keys, out;
    std::vector<int32_t> rc;
    Parked(Rig& rig, uint32_t first_key, std::vector<uint32_t> parked_keys) : keys{first_key}, out(1 + parked_keys.size(), 0), rc(out.size(), 99) {
        keys.insert(keys.end(), parked_keys.begin(), parked_keys.end());
        std::vector<std::thread> th;
        th.push_back(rig.hold(first_key, 0, &out[0], &rc[0]));
        for (uint32_t i = 1; i < keys.size(); ++i) {
            th.emplace_back([&, i] { rc[i] = rig.call(keys[i], i, &out[i]); });
            rig.wait_parked(i);
        }
        rig.release();
        for (std::thread& t : th) t.join();
    }
    std::string rcs() const {
        std::string s;
        for (size_t i = 0; i < rc.size(); ++i) s += (i ? "," : "") + std::string(rc_name(rc[i]));
        return s;
    }
    bool answered(size_t i) const { return out[i] == answer(keys[i], (uint32_t)i); }
};

static void lone_caller() {
    Rig rig;
    rig.q.wait_us = 5000000;
    uint32_t out = 0;
    const auto t0 = Clock::now();
    const int32_t rc = rig.call(A, 7, &out);
    const int64_t us = micros(Clock::now() - t0);
    std::printf("lone|%s|%s|%d|%d\n", rig.blocks_text().c_str(), rc_name(rc), out == answer(A, 7), us < 1000000);
}

static void deterministic_seal() {
    Rig rig;
    rig.q.wait_us = 2000;
    Parked p(rig, A, {A, A, B, A, A, A, B, A});
    std::string expects;
    for (const Block& b : rig.blocks) expects += (expects.empty() ? "" : ",") + std::to_string(b.expect);
    uint32_t own = 0;
    for (size_t i = 0; i < p.out.size(); ++i) own += p.answered(i) && p.rc[i] == CQS_HIP_OK;
    std::printf("seal|%s|%s|%u|%zu\n", rig.blocks_text().c_str(), expects.c_str(), own, rig.q.parked());
}

static void storm() {
    const uint32_t n_threads = 8, per_thread = 2000;
    Queue q;
    q.wait_us = 100;
    std::atomic<uint32_t> own{0}, n_blocks{0}, members{0}, largest{0}, mixed{0}, ready{0};
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < n_threads; ++t)
        th.emplace_back([&, t] {
            ready.fetch_add(1);
            while (ready.load() < n_threads) std::this_thread::yield();   // everybody starts together
            uint32_t lcg = 12345u + t;
            for (uint32_t i = 0; i < per_thread; ++i) {
                lcg = lcg * 1664525u + 1013904223u;
                uint32_t out = 0;
                Req r{(lcg >> 16) & 1u ? A : B, t * per_thread + i, &out, 0, false};
                const int32_t rc = q.search(r, same_key, [&](Req* const* batch, uint32_t nb) {
                    n_blocks.fetch_add(1);
                    members.fetch_add(nb);
                    for (uint32_t seen = largest.load(); nb > seen && !largest.compare_exchange_weak(seen, nb);) {}
                    std::this_thread::yield();                              // a pass takes a while: the others park meanwhile
                    for (uint32_t j = 0; j < nb; ++j) {
                        mixed.fetch_add(same_key(batch[j], batch[0]) ? 0u : 1u);
                        *batch[j]->out = answer(batch[j]->key, batch[j]->payload);
                    }
                    return Outcome{CQS_HIP_OK, false};
                });
                own.fetch_add(rc == CQS_HIP_OK && out == answer(r.key, r.payload) ? 1u : 0u);
            }
        });
    for (std::thread& t : th) t.join();
    std::printf("storm|%u|%u|%u|%u|%u|%zu\n", own.load(), n_blocks.load(), members.load(), largest.load(), mixed.load(), q.parked());
}

static void failure(const char* name, Outcome o, std::vector<uint32_t> parked_keys) {
    Rig rig;
    rig.q.wait_us = 2000;
    rig.fail_key = A;
    rig.fail = o;
    Parked p(rig, C, parked_keys);
    std::string answered;
    for (size_t i = 0; i < p.out.size(); ++i) answered += p.answered(i) ? '1' : (p.out[i] == 0 ? '0' : 'x');
    bool leader;
    { std::lock_guard<std::mutex> g(rig.q.mu); leader = rig.q.leader; }
    std::printf("%s|%s|%s|%s|%zu|%d\n", name, rig.blocks_text().c_str(), p.rcs().c_str(), answered.c_str(), rig.q.parked(), leader);
}

static void straggler_window() {
    const uint32_t wait_us = 300000;
    Rig rig;
    rig.q.wait_us = wait_us;
    uint32_t out = 0;
    // a burst of 4 in one block, then a lone caller at once: it is sealed no earlier than the window's end
    Parked burst(rig, C, {A, A, A, A});
    Clock::time_point pass_end;
    uint32_t expect;
    { std::lock_guard<std::mutex> g(rig.q.mu); pass_end = rig.q.last_pass_end; expect = rig.q.expect; }
    rig.call(A, 50, &out);
    const int64_t waited = micros(rig.blocks.back().at - pass_end);
    // another burst, then a lone caller after the window has closed: it does not wait
    Parked burst2(rig, C, {A, A, A, A});
    uint32_t expect2;
    { std::lock_guard<std::mutex> g(rig.q.mu); expect2 = rig.q.expect; }
    std::this_thread::sleep_for(std::chrono::milliseconds(400));
    const auto parked_at = Clock::now();
    rig.call(A, 51, &out);
    const int64_t late = micros(rig.blocks.back().at - parked_at);
    std::printf("window|%s|%u|%lld|%u|%lld|%u\n", rig.blocks_text().c_str(), expect, (long long)waited, expect2, (long long)late, wait_us);
}

int main() {
    lone_caller();
    deterministic_seal();
    storm();
    failure("poison", Outcome{CQS_HIP_ERR_DEVICE, true}, {A, A, A, B, B});
    failure("nomem", Outcome{CQS_HIP_ERR_NOMEM, false}, {A, A, B});
    straggler_window();
    return 0;
}
