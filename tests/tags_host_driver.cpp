// Stand-alone driver of cqs_amd/csrc/tags_host.h (tests/test_tags_host_cpu.py builds it with ASAN + UBSan and feeds it its
// cases on stdin).  One case per line, one answer per line:
//   keep name n k tag_0 .. tag_{n-1} allow_0 .. allow_31
//       -> name|kept|word_0,..|all_pass|count rule: keep:k_eff|plan_keep on that bitset: keep:k_eff
//     (the per-row rule through keep_words; the count-taking keep rule beside search_host.h's plan_keep on the bitset the
//     words are; tags and allow words in hex)
//   set name first_row m|null row_base len tagged       (m tags, or `null <m>` for a null array of m)
//       -> name|plan|why|first_local|new_tagged
//   rm name n row_base tagged m id_0 .. id_{m-1}
//       -> name|plan|new_tagged|survivors below the old prefix
//     (the ids through remove_host.h's plan_remove, as index_remove.hip does, then tagged_after_remove; the last field
//     counts, on an array compacted with std::remove_if, the surviving rows that had a tag)
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/remove_host.h"
#include "../cqs_amd/csrc/tags_host.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, name;
        if (!(in >> cmd >> name)) continue;
        if (cmd == "keep") {
            uint64_t n = 0;
            uint32_t k = 0;
            in >> n >> k;
            std::vector<uint32_t> tags(n), allow(cqs_tags::kAllowWords);
            in >> std::hex;
            for (uint32_t& t : tags) in >> t;
            for (uint32_t& a : allow) in >> a;
            std::vector<uint32_t> words((n + 31) / 32);
            const uint64_t kept = cqs_tags::keep_words(tags.data(), n, allow.data(), words.data());
            std::cout << name << '|' << kept << '|' << std::hex;
            for (size_t i = 0; i < words.size(); ++i) std::cout << (i ? "," : "") << words[i];
            std::cout << std::dec << '|' << (cqs_tags::all_pass(allow.data()) ? 1 : 0);
            uint32_t k_count = k, k_bits = k;
            const cqs_search::Keep by_count = cqs_tags::plan_keep_count(kept, n, &k_count);
            const cqs_search::Keep by_bits = cqs_search::plan_keep(words.data(), n, &k_bits);
            std::cout << '|' << (int)by_count << ':' << k_count << '|' << (int)by_bits << ':' << k_bits << '\n';
        } else if (cmd == "set") {
            uint64_t first_row = 0, m = 0, row_base = 0, len = 0, tagged = 0;
            std::string ms;
            in >> first_row >> ms;
            const bool null_tags = ms == "null";
            if (null_tags) in >> m; else m = std::stoull(ms);
            in >> row_base >> len >> tagged;
            std::vector<uint32_t> tags(null_tags ? 0 : std::min<uint64_t>(m, 4096), 7u);   // (a Write plan has m <= len, small here)
            uint64_t first_local = 99, new_tagged = 99;
            const char* why = "";
            // (an empty vector's data() may be null: m == 0 must not look at it)
            const cqs_tags::Set plan = cqs_tags::plan_set_tags(first_row, null_tags ? nullptr : tags.data(), m, row_base, len, tagged,
                                                               &first_local, &new_tagged, &why);
            if (plan == cqs_tags::Set::Write) {          // what set_tags then does: the copy stays inside a column of len entries
                std::vector<uint32_t> column(len);
                for (uint64_t i = 0; i < m; ++i) column.at(first_local + i) = tags[i];
            }
            std::cout << name << '|' << (int)plan << '|' << why << '|' << first_local << '|' << new_tagged << '\n';
        } else if (cmd == "rm") {
            uint64_t n = 0, row_base = 0, tagged = 0, m = 0;
            in >> n >> row_base >> tagged >> m;
            std::vector<uint64_t> ids(m);
            for (uint64_t& i : ids) in >> i;
            std::vector<uint64_t> removed;
            std::vector<cqs_remove::Run> runs;
            const char* why = "";
            const cqs_remove::Plan plan = cqs_remove::plan_remove(ids.data(), m, row_base, n, &removed, &runs, &why);
            uint64_t new_tagged = tagged, below = 0;
            if (plan == cqs_remove::Plan::Remove) {
                new_tagged = cqs_tags::tagged_after_remove(removed.data(), removed.size(), tagged);
                std::vector<uint64_t> v(n);
                for (uint64_t i = 0; i < n; ++i) v[i] = i;
                v.erase(std::remove_if(v.begin(), v.end(), [&](uint64_t r) { return std::binary_search(removed.begin(), removed.end(), r); }), v.end());
                for (uint64_t r : v) below += r < tagged ? 1 : 0;
            }
            std::cout << name << '|' << (int)plan << '|' << new_tagged << '|' << below << '\n';
        }
    }
    return 0;
}
