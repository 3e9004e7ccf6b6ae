// Stand-alone driver of cqs_amd/csrc/diff_host.h (tests/test_diff_host_cpu.py builds it with ASAN + UBSan, and a second
// time with TSan for the lock).  `diff_host_driver cases` reads lines from stdin:
//     plan name  a_present a_sharded a_device a_dim a_base a_len  b_present b_sharded b_device b_dim b_base b_len
//          m thr_bits has_rows_a has_rows_b has_counts has_mod_pairs has_mod_sims  rows_a[0..m) rows_b[0..m)
//       -> name|plan|why
//     passes name m budget
//       -> name|first:count,...
//     run name file budget thr_bits
//       -> name|sim bits,...|class words,...|mod pairs,...|mod sim bits,...|modified,unchanged,undefined
//   `file` holds u64 {n_a, n_b, dim, m, base_a, base_b}, then A [n_a, dim] f32, B [n_b, dim] f32, rows_a [m] u64, rows_b [m]
//   u64.  A run is the call's host restatement end to end: the plan, then per pass local_rows into arrays of exactly the
//   pass's size, pair_sim per pair, compact, append_modified - every array sized exactly, so a step outside is ASAN's.
// `diff_host_driver lock rounds` runs PairLock from three threads - (x, y), (y, x) and (x, x) - `rounds` times each over
// two plain counters that only the locks protect, and prints the counters.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../cqs_amd/csrc/diff_host.h"

using namespace cqs_diff;

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static bool read_side(std::istringstream& in, Side* s) {
    int present = 0, sharded = 0;
    if (!(in >> present >> sharded >> s->device >> s->dim >> s->row_base >> s->len)) return false;
    s->present = present != 0;
    s->sharded = sharded != 0;
    return true;
}

static void run_plan(std::istringstream& in) {
    std::string name;
    Side a{}, b{};
    uint64_t m = 0;
    uint32_t thr = 0;
    int has_a = 0, has_b = 0, has_counts = 0, has_pairs = 0, has_sims = 0;
    if (!(in >> name) || !read_side(in, &a) || !read_side(in, &b)) return;
    if (!(in >> m >> thr >> has_a >> has_b >> has_counts >> has_pairs >> has_sims)) return;
    std::vector<uint64_t> ra(m), rb(m);
    for (uint64_t i = 0; i < m; ++i) in >> ra[i];
    for (uint64_t i = 0; i < m; ++i) in >> rb[i];
    const Args g{has_a ? ra.data() : nullptr, has_b ? rb.data() : nullptr, m, from_bits(thr), has_counts != 0, has_pairs != 0, has_sims != 0};
    std::string why = "stale";
    const Plan plan = plan_diff(a, b, g, &why);
    std::cout << name << '|' << (int)plan << '|' << why << '\n';
}

static void run_passes(std::istringstream& in) {
    std::string name;
    uint64_t m = 0, budget = 0;
    if (!(in >> name >> m >> budget)) return;
    std::cout << name << '|';
    const std::vector<Pass> passes = cut_passes(m, budget);
    for (size_t i = 0; i < passes.size(); ++i) std::cout << (i ? "," : "") << passes[i].first << ':' << passes[i].count;
    std::cout << '\n';
}

template <class T>
static std::vector<T> read_array(std::ifstream& f, uint64_t count) {
    std::vector<T> v(count);
    f.read((char*)v.data(), (std::streamsize)(count * sizeof(T)));
    return v;
}

static void run_call(std::istringstream& in) {
    std::string name, path;
    uint64_t budget = 0;
    uint32_t thr_bits = 0;
    if (!(in >> name >> path >> budget >> thr_bits)) return;
    std::ifstream f(path, std::ios::binary);
    const std::vector<uint64_t> h = read_array<uint64_t>(f, 6);
    const uint64_t n_a = h[0], n_b = h[1], dim = h[2], m = h[3], base_a = h[4], base_b = h[5];
    const std::vector<float> A = read_array<float>(f, n_a * dim), B = read_array<float>(f, n_b * dim);
    const std::vector<uint64_t> ra = read_array<uint64_t>(f, m), rb = read_array<uint64_t>(f, m);
    if (!f) { std::cout << name << "|unreadable\n"; return; }
    const float thr = from_bits(thr_bits);
    const Side a{true, false, 0, (uint32_t)dim, base_a, n_a}, b{true, false, 0, (uint32_t)dim, base_b, n_b};
    std::string why;
    if (plan_diff(a, b, Args{ra.data(), rb.data(), m, thr, true, true, true}, &why) != Plan::Run) {
        std::cout << name << "|refused: " << why << '\n';
        return;
    }
    std::vector<float> sims(m), mod_sims;
    std::vector<uint32_t> classes(m);
    std::vector<uint64_t> mod_pairs;
    uint64_t modified = 0, undefined = 0;
    for (const Pass& ps : cut_passes(m, budget)) {
        std::vector<uint32_t> la(ps.count), lb(ps.count), cls(ps.count);
        std::vector<float> s(ps.count);
        std::vector<ListEntry> list(ps.count);
        local_rows(ra.data(), base_a, ps, la.data());
        local_rows(rb.data(), base_b, ps, lb.data());
        for (uint64_t j = 0; j < ps.count; ++j)
            s[j] = pair_sim(A.data() + (size_t)la[j] * dim, B.data() + (size_t)lb[j] * dim, (uint32_t)dim, thr, &cls[j]);
        uint32_t counts[2];
        compact(cls.data(), s.data(), (uint32_t)ps.count, list.data(), counts);
        mod_pairs.resize(modified + counts[0]);
        mod_sims.resize(modified + counts[0]);
        modified = append_modified(ps, list.data(), counts[0], modified, mod_pairs.data(), mod_sims.data());
        undefined += counts[1];
        for (uint64_t j = 0; j < ps.count; ++j) { sims[ps.first + j] = s[j]; classes[ps.first + j] = cls[j]; }
    }
    std::cout << name << '|';
    for (uint64_t i = 0; i < m; ++i) std::cout << (i ? "," : "") << to_bits(sims[i]);
    std::cout << '|';
    for (uint64_t i = 0; i < m; ++i) std::cout << (i ? "," : "") << classes[i];
    std::cout << '|';
    for (uint64_t i = 0; i < modified; ++i) std::cout << (i ? "," : "") << mod_pairs[i];
    std::cout << '|';
    for (uint64_t i = 0; i < modified; ++i) std::cout << (i ? "," : "") << to_bits(mod_sims[i]);
    std::cout << '|' << modified << ',' << m - modified << ',' << undefined << '\n';
}

static int run_lock(int rounds) {
    std::mutex x, y;
    long cx = 0, cy = 0;   // cx is x's, cy is y's: plain counters, so a hole in the locking is a data race
    std::thread t1([&] { for (int i = 0; i < rounds; ++i) { PairLock<std::mutex> g(x, y); ++cx; ++cy; } });
    std::thread t2([&] { for (int i = 0; i < rounds; ++i) { PairLock<std::mutex> g(y, x); ++cx; ++cy; } });
    std::thread t3([&] { for (int i = 0; i < rounds; ++i) { PairLock<std::mutex> g(x, x); ++cx; } });
    t1.join();
    t2.join();
    t3.join();
    std::printf("%ld %ld\n", cx, cy);
    return cx == 3L * rounds && cy == 2L * rounds ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::string(argv[1]) == "lock") return run_lock(std::atoi(argv[2]));
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "plan") run_plan(in);
        else if (kind == "passes") run_passes(in);
        else if (kind == "run") run_call(in);
    }
    return 0;
}
