// Stand-alone driver of the multi-filter part of cqs_amd/csrc/tags_host.h (tests/test_tags_multi_host_cpu.py builds it with
// ASAN + UBSan and feeds it its cases on stdin).  One case per line, one answer per line:
//   multi name f n tag_0 .. tag_{n-1} allow_0 .. allow_{32 f - 1}        (tags and allow words in hex)
//       -> name|disagreements|table words with a bit >= f|verdicts_0,..,verdicts_{n-1}
//     (the f filters through transpose_filters into a table of exactly 1024 words, every tag through tag_verdicts;
//     `disagreements` counts the (tag, j < f) pairs where bit j of the verdicts is not tag_kept(tag, filter j))
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/tags_host.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, name;
        if (!(in >> cmd >> name) || cmd != "multi") continue;
        uint32_t f = 0;
        uint64_t n = 0;
        in >> f >> n;
        std::vector<uint32_t> tags(n), allows((size_t)f * cqs_tags::kAllowWords);
        in >> std::hex;
        for (uint32_t& t : tags) in >> t;
        for (uint32_t& a : allows) in >> a;
        std::vector<uint32_t> tbl(cqs_tags::kTableWords, 0xFFFFFFFFu);   // (heap, exact size: ASAN sees a write past it)
        cqs_tags::transpose_filters(allows.data(), f, tbl.data());
        uint64_t high = 0, bad = 0;
        for (uint32_t w : tbl) high += (f < 32 && (w >> f)) ? 1 : 0;
        std::cout << name << '|';
        std::ostringstream verdicts;
        verdicts << std::hex;
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t v = cqs_tags::tag_verdicts(tags[i], tbl.data());
            for (uint32_t j = 0; j < f; ++j)
                bad += (((v >> j) & 1u) != 0u) != cqs_tags::tag_kept(tags[i], allows.data() + (size_t)cqs_tags::kAllowWords * j) ? 1 : 0;
            verdicts << (i ? "," : "") << v;
        }
        std::cout << bad << '|' << high << '|' << verdicts.str() << '\n';
    }
    return 0;
}
