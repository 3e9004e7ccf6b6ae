// Stand-alone driver of cqs_amd/csrc/update_host.h (tests/test_update_host_cpu.py builds it with ASAN + UBSan and feeds it
// its cases on stdin).  One case per line:
//     name n row_base budget_rows m vectors id_0 ... id_{m-1}
// (`vectors` is 1, or 0 for a null vector block; the single word `null` in place of the ids is a null id list.)
// One answer per line:
//     name|plan|why|local rows in list order|order|first:count,...|values|shards|checks
// "values": an array holding 0 .. n-1 updated exactly as the library does it - per pass the planned entries gathered into a
// staging block of the largest pass's size (entry i of the list carries the value 1000000 + i) with their destination
// list beside them, then one write per staged entry - so a pass that overruns its staging block is ASAN's to find.
// "shards": the entries of three near-equal row ranges (entries_in), as first:count.
// "checks": 1 when every pass holds 1 .. budget entries, the passes tile the order with no gap, every list entry is staged
// exactly once, the destinations ascend strictly over the whole sequence, and the three shard ranges tile the order.
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/update_host.h"

using namespace cqs_update;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name;
        uint64_t n = 0, row_base = 0, budget = 0, m = 0;
        int has_vectors = 1;
        if (!(in >> name >> n >> row_base >> budget >> m >> has_vectors)) continue;
        std::vector<uint64_t> ids;
        bool null_ids = false;
        std::string tok;
        while (in >> tok) {
            if (tok == "null") null_ids = true; else ids.push_back(std::stoull(tok));
        }
        const float some = 0.f;   // (the plan only asks whether the block is there)
        std::vector<uint32_t> local;
        std::vector<uint64_t> order;
        const char* why = "";
        const Plan plan = plan_update(null_ids ? nullptr : ids.data(), has_vectors ? &some : nullptr, m, row_base, n, &local, &order, &why);
        std::cout << name << '|' << (int)plan << '|' << why << '|';
        for (size_t i = 0; i < local.size(); ++i) std::cout << (i ? "," : "") << local[i];
        std::cout << '|';
        for (size_t i = 0; i < order.size(); ++i) std::cout << (i ? "," : "") << order[i];
        std::cout << '|';
        std::vector<uint64_t> v(n);
        for (uint64_t i = 0; i < n; ++i) v[i] = i;
        bool ok = true;
        std::ostringstream shards;
        if (plan == Plan::Update) {
            ok = ok && local.size() == m && order.size() == m;
            const std::vector<Pass> passes = cut_passes(m, budget);
            size_t largest = 0, next = 0;
            for (size_t i = 0; i < passes.size(); ++i) {
                std::cout << (i ? "," : "") << passes[i].first << ':' << passes[i].count;
                ok = ok && passes[i].count >= 1 && passes[i].count <= (budget ? budget : 1) && passes[i].first == next;
                next = passes[i].first + passes[i].count;
                if (passes[i].count > largest) largest = passes[i].count;
            }
            ok = ok && next == m;
            std::vector<uint64_t> stage(largest);
            std::vector<uint32_t> dst(largest);
            std::vector<uint32_t> staged(m, 0);
            int64_t last_dst = -1;
            for (const Pass& p : passes) {
                for (size_t j = 0; j < p.count; ++j) {
                    const uint64_t entry = order.at(p.first + j);
                    stage.at(j) = 1000000u + entry;
                    dst.at(j) = local.at(entry);
                    ++staged.at(entry);
                }
                for (size_t j = 0; j < p.count; ++j) {
                    ok = ok && (int64_t)dst[j] > last_dst;
                    last_dst = dst[j];
                    v.at(dst[j]) = stage[j];
                }
            }
            for (uint64_t i = 0; i < m; ++i) ok = ok && staged[i] == 1u;
            size_t tiled = 0;
            for (uint64_t s = 0; s < 3; ++s) {
                size_t first = 0;
                const size_t count = entries_in(local, order, n * s / 3, n * (s + 1) / 3, &first);
                shards << (s ? "," : "") << first << ':' << count;
                ok = ok && first == tiled;
                for (size_t j = 0; j < count; ++j)
                    ok = ok && local[order[first + j]] >= n * s / 3 && local[order[first + j]] < n * (s + 1) / 3;
                tiled += count;
            }
            ok = ok && tiled == m;
        }
        std::cout << '|';
        for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? "," : "") << v[i];
        std::cout << '|' << shards.str() << '|' << (ok ? 1 : 0) << '\n';
    }
    return 0;
}
