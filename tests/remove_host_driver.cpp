// Stand-alone driver of cqs_amd/csrc/remove_host.h (tests/test_remove_host_cpu.py builds it with ASAN + UBSan and feeds it
// its cases on stdin).  One case per line:
//     name n row_base budget_rows m id_0 ... id_{m-1}        (or the single word `null` for a null id list)
// One answer per line:
//     name|plan|why|removed|src:dst:rows,...|dst:rows:run_first:run_count,...|surviving values|checks
// "surviving values": an array holding 0 .. n-1 compacted in place exactly as the device does it - per pass a gather into a
// bounce buffer of the largest pass's rows through the run table with its closing entry (the kernel's lookup: a binary
// search in the pass's runs, then a walk), then the copy to the pass's destination - and cut to its new length.
// "checks": 1 when every pass fits the budget, satisfies pass_overlap_ok, passes tile the runs' destinations in order,
// and no row below the first removed row was written.
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/remove_host.h"

using namespace cqs_remove;

struct Entry { uint64_t src, dst; };

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name;
        uint64_t n = 0, row_base = 0, budget = 0, m = 0;
        if (!(in >> name >> n >> row_base >> budget >> m)) continue;
        std::vector<uint64_t> ids;
        bool null_ids = false;
        std::string tok;
        while (in >> tok) {
            if (tok == "null") null_ids = true; else ids.push_back(std::stoull(tok));
        }
        std::vector<uint64_t> removed;
        std::vector<Run> runs;
        const char* why = "";
        const Plan plan = plan_remove(null_ids ? nullptr : ids.data(), m, row_base, n, &removed, &runs, &why);
        std::cout << name << '|' << (int)plan << '|' << why << '|' << removed.size() << '|';
        for (size_t i = 0; i < runs.size(); ++i) std::cout << (i ? "," : "") << runs[i].src << ':' << runs[i].dst << ':' << runs[i].rows;
        std::cout << '|';
        std::vector<uint64_t> v(n);
        for (uint64_t i = 0; i < n; ++i) v[i] = i;
        bool ok = true;
        if (plan == Plan::Remove) {
            const std::vector<Pass> passes = cut_passes(runs, budget);
            for (size_t i = 0; i < passes.size(); ++i)
                std::cout << (i ? "," : "") << passes[i].dst << ':' << passes[i].rows << ':' << passes[i].run_first << ':' << passes[i].run_count;
            const uint64_t n_new = n - removed.size();
            std::vector<Entry> table;
            for (const Run& r : runs) table.push_back(Entry{r.src, r.dst});
            table.push_back(Entry{n, n_new});
            uint64_t largest = 0, next_dst = removed[0];
            for (size_t i = 0; i < passes.size(); ++i) {
                const Pass& p = passes[i];
                ok = ok && p.rows >= 1 && p.rows <= (budget ? budget : 1) && p.dst == next_dst && pass_overlap_ok(runs, passes, i);
                ok = ok && p.run_first + p.run_count <= runs.size() && runs[p.run_first].dst <= p.dst;
                next_dst = p.dst + p.rows;
                if (p.rows > largest) largest = p.rows;
            }
            ok = ok && next_dst == n_new;
            std::vector<uint64_t> bounce(largest);
            for (const Pass& p : passes) {
                const Entry* t = table.data() + p.run_first;
                size_t lo = 0, hi = p.run_count;
                while (hi - lo > 1) {
                    const size_t mid = lo + (hi - lo) / 2;
                    if (t[mid].dst <= p.dst) lo = mid; else hi = mid;
                }
                for (uint64_t j = 0; j < p.rows; ++j) {
                    const uint64_t d = p.dst + j;
                    while (d >= t[lo + 1].dst) ++lo;
                    const uint64_t s = t[lo].src + (d - t[lo].dst);
                    ok = ok && s == source_of(runs, d) && s > d && s < n;
                    bounce[j] = v.at(s);
                }
                for (uint64_t j = 0; j < p.rows; ++j) {
                    ok = ok && p.dst + j >= removed[0];
                    v.at(p.dst + j) = bounce[j];
                }
            }
            v.resize(n_new);
        }
        std::cout << '|';
        for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? "," : "") << v[i];
        std::cout << '|' << (ok ? 1 : 0) << '\n';
    }
    return 0;
}
