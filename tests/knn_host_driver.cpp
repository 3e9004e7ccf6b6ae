// Stand-alone driver of cqs_amd/csrc/knn_host.h (tests/test_knn_host_cpu.py builds it with ASAN + UBSan and feeds it its
// cases on stdin).  Two kinds of line:
//     plan name present sharded row_base len max_block first_row m limit outputs
//     finish name limit target cnt key_0 ... key_{cnt-1}
// A plan line answers
//     name|plan|why|L|k1|T|local_first|tile_first:tile_rows:emit_first:emit_count:out_offset,...|checks
// "checks": 1 when every tile is a whole fixed tile of the corpus (starts at a multiple of T, has min(T, len - start)
// rows), its emitted targets lie inside it, and - replayed on an array of exactly m counters, so an emit outside the
// request is ASAN's to find - every asked target is emitted exactly once, at the output row that is its distance from
// first_row, in ascending order.
// A finish line runs the finish rule (finish_target) into arrays of exactly `limit` slots and, beside it, the host path it
// stands for: cqs_search::unpack_keys + cqs_search::drop_self.  It answers
//     name|count|rows|score bits|drop_self count|its rows|its score bits
// with all `limit` slots of the first pair (zeros past the count) and the drop_self pair cut at its count.
#include <cstdint>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/knn_host.h"

using namespace cqs_knn;

static void run_plan(std::istringstream& in) {
    std::string name;
    int present = 0, sharded = 0, outputs = 0;
    uint64_t row_base = 0, len = 0, first_row = 0, m = 0;
    uint32_t max_block = 0, limit = 0;
    if (!(in >> name >> present >> sharded >> row_base >> len >> max_block >> first_row >> m >> limit >> outputs)) return;
    const Handle h{present != 0, sharded != 0, row_base, len, max_block};
    Planned pl;
    const char* why = "";
    const Plan plan = plan_knn(h, first_row, m, limit, outputs != 0, &pl, &why);
    std::cout << name << '|' << (int)plan << '|' << why << '|' << pl.limit << '|' << pl.k1 << '|' << pl.tile << '|'
              << pl.local_first << '|';
    bool ok = true;
    if (plan == Plan::Run) {
        const std::vector<Tile> tiles = cut_tiles(pl.local_first, m, len, pl.tile);
        std::vector<uint32_t> emitted_times(m, 0);
        uint64_t next_out = 0;
        for (size_t i = 0; i < tiles.size(); ++i) {
            const Tile& t = tiles[i];
            std::cout << (i ? "," : "") << t.tile_first << ':' << t.tile_rows << ':' << t.emit_first << ':' << t.emit_count
                      << ':' << t.out_offset;
            const uint64_t whole = len - t.tile_first < pl.tile ? len - t.tile_first : pl.tile;
            ok = ok && t.tile_first % pl.tile == 0 && t.tile_first < len && t.tile_rows == whole && t.emit_count >= 1 &&
                 (uint64_t)t.emit_first + t.emit_count <= t.tile_rows && t.out_offset == next_out;
            for (uint32_t j = 0; j < t.emit_count; ++j) {
                ++emitted_times.at(t.out_offset + j);
                ok = ok && t.tile_first + t.emit_first + j == pl.local_first + t.out_offset + j;
            }
            next_out += t.emit_count;
        }
        ok = ok && next_out == m;
        for (uint64_t i = 0; i < m; ++i) ok = ok && emitted_times[i] == 1u;
    }
    std::cout << '|' << (ok ? 1 : 0) << '\n';
}

static void run_finish(std::istringstream& in) {
    std::string name;
    uint32_t limit = 0, target = 0, cnt = 0;
    if (!(in >> name >> limit >> target >> cnt)) return;
    std::vector<uint64_t> keys(cnt);
    for (uint32_t i = 0; i < cnt; ++i) in >> keys[i];
    std::vector<uint64_t> rows(limit, ~0ull), ds_rows(limit, ~0ull), all_rows(cnt);
    std::vector<float> scores(limit, -1.f), ds_scores(limit, -1.f), all_scores(cnt);
    const uint32_t count = finish_target(keys.data(), cnt, target, limit, rows.data(), scores.data());
    cqs_search::unpack_keys(keys.data(), cnt, all_rows.data(), all_scores.data());
    const uint32_t ds = cqs_search::drop_self(all_rows.data(), all_scores.data(), cnt, target, limit, ds_rows.data(), ds_scores.data());
    const auto bits = [](float f) { uint32_t b; memcpy(&b, &f, 4); return b; };
    std::cout << name << '|' << count << '|';
    for (uint32_t i = 0; i < limit; ++i) std::cout << (i ? "," : "") << rows[i];
    std::cout << '|';
    for (uint32_t i = 0; i < limit; ++i) std::cout << (i ? "," : "") << bits(scores[i]);
    std::cout << '|' << ds << '|';
    for (uint32_t i = 0; i < ds; ++i) std::cout << (i ? "," : "") << ds_rows[i];
    std::cout << '|';
    for (uint32_t i = 0; i < ds; ++i) std::cout << (i ? "," : "") << bits(ds_scores[i]);
    std::cout << '\n';
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "plan") run_plan(in);
        else if (kind == "finish") run_finish(in);
    }
    return 0;
}
