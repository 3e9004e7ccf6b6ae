// Stand-alone driver of cqs_amd/csrc/match_host.h (tests/test_match_host_cpu.py builds it with ASAN + UBSan).
// `match_host_driver` reads lines from stdin:
//     plan name  a_present a_sharded a_device a_dim a_base a_len  b_present b_sharded b_device b_dim b_base b_len
//          m_a m_b has_rows_a has_rows_b has_best_a has_score_a has_best_b has_score_b  n_a rows_a[0..n_a) n_b rows_b[0..n_b)
//       -> name|plan|why|local rows of a,...|local rows of b,...          (the local rows only when the plan is Run)
//        (n_a / n_b: how many rows the line carries - m_a / m_b, or 0 where the plan must answer before it reads them;
//         the arrays are sized exactly, so a read past them is ASAN's)
//     key name score_bits position
//       -> name|key|best|score bits                                        (pack, then unpack)
//     merge name file block reverse
//       -> name|best_a,...|score_a bits,...|best_b,...|score_b bits,...
//        file: u64 {m_a, m_b}, S [m_a, m_b] f32.  Each side's answer is built block by block of the OTHER side's list
//        (blocks of `block` positions, last to first when `reverse`): a block's answer is the maximum of pack() over its
//        positions, unpacked, moved to global positions and folded in with merge_best.
//     mutual name file thr_bits
//       -> name|i:j,...                                                    (bests by one block over S, then mutual_pairs)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/match_host.h"

using namespace cqs_match;

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static bool read_side(std::istringstream& in, Side* s) {
    int present = 0, sharded = 0;
    if (!(in >> present >> sharded >> s->device >> s->dim >> s->row_base >> s->len)) return false;
    s->present = present != 0;
    s->sharded = sharded != 0;
    return true;
}

template <class T>
static void print_list(const std::vector<T>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? "," : "") << v[i];
}

static void run_plan(std::istringstream& in) {
    std::string name;
    Side a{}, b{};
    uint32_t m_a = 0, m_b = 0;
    int has[6] = {0, 0, 0, 0, 0, 0};
    if (!(in >> name) || !read_side(in, &a) || !read_side(in, &b)) return;
    if (!(in >> m_a >> m_b >> has[0] >> has[1] >> has[2] >> has[3] >> has[4] >> has[5])) return;
    uint64_t n_a = 0, n_b = 0;
    in >> n_a;
    std::vector<uint64_t> ra(n_a);
    for (uint64_t i = 0; i < n_a; ++i) in >> ra[i];
    in >> n_b;
    std::vector<uint64_t> rb(n_b);
    for (uint64_t i = 0; i < n_b; ++i) in >> rb[i];
    const Args g{has[0] ? ra.data() : nullptr, m_a, has[1] ? rb.data() : nullptr, m_b, has[2] != 0, has[3] != 0, has[4] != 0, has[5] != 0};
    std::string why = "stale";
    const Plan plan = plan_match(a, b, g, &why);
    std::cout << name << '|' << (int)plan << '|' << why << '|';
    if (plan == Plan::Run) {
        std::vector<uint32_t> la(m_a), lb(m_b);
        local_rows(ra.data(), a.row_base, m_a, la.data());
        local_rows(rb.data(), b.row_base, m_b, lb.data());
        print_list(la);
        std::cout << '|';
        print_list(lb);
    } else {
        std::cout << '|';
    }
    std::cout << '\n';
}

static void run_key(std::istringstream& in) {
    std::string name;
    uint32_t score_bits = 0, position = 0;
    if (!(in >> name >> score_bits >> position)) return;
    const uint64_t key = pack(from_bits(score_bits), position);
    uint64_t best = 1;
    float score = 1.f;
    unpack(key, &best, &score);
    std::cout << name << '|' << key << '|' << best << '|' << to_bits(score) << '\n';
}

struct Matrix {
    uint64_t m_a = 0, m_b = 0;
    std::vector<float> s;
    bool ok = false;
};

static Matrix read_matrix(const std::string& path) {
    Matrix x;
    std::ifstream f(path, std::ios::binary);
    uint64_t h[2] = {0, 0};
    f.read((char*)h, sizeof h);
    x.m_a = h[0];
    x.m_b = h[1];
    x.s.resize(x.m_a * x.m_b);
    f.read((char*)x.s.data(), (std::streamsize)(x.s.size() * sizeof(float)));
    x.ok = (bool)f;
    return x;
}

// One side's answers, block by block of the other side's list.  at(i, j): the entry of row i of this side and position j
// of the other.
template <class At>
static void side_by_blocks(uint64_t rows, uint64_t others, uint64_t block, bool reverse, At at, std::vector<uint64_t>* best,
                           std::vector<float>* score) {
    best->assign(rows, kNone);
    score->assign(rows, 0.0f);
    std::vector<uint64_t> starts;
    for (uint64_t j0 = 0; j0 < others; j0 += block) starts.push_back(j0);
    if (reverse) std::reverse(starts.begin(), starts.end());
    for (uint64_t j0 : starts) {
        const uint64_t j1 = std::min(others, j0 + block);
        for (uint64_t i = 0; i < rows; ++i) {
            uint64_t key = 0;
            for (uint64_t j = j0; j < j1; ++j) key = std::max(key, pack(at(i, j), (uint32_t)(j - j0)));
            uint64_t b = 0;
            float s = 0.f;
            unpack(key, &b, &s);
            if (b != kNone) b += j0;
            merge_best(&(*best)[i], &(*score)[i], b, s);
        }
    }
}

static void bests(const Matrix& x, uint64_t block, bool reverse, std::vector<uint64_t>* ba, std::vector<float>* sa, std::vector<uint64_t>* bb,
                  std::vector<float>* sb) {
    side_by_blocks(x.m_a, x.m_b, block, reverse, [&](uint64_t i, uint64_t j) { return x.s[i * x.m_b + j]; }, ba, sa);
    side_by_blocks(x.m_b, x.m_a, block, reverse, [&](uint64_t j, uint64_t i) { return x.s[i * x.m_b + j]; }, bb, sb);
}

static void run_merge(std::istringstream& in) {
    std::string name, path;
    uint64_t block = 0;
    int reverse = 0;
    if (!(in >> name >> path >> block >> reverse) || block == 0) return;
    const Matrix x = read_matrix(path);
    if (!x.ok) { std::cout << name << "|unreadable\n"; return; }
    std::vector<uint64_t> ba, bb;
    std::vector<float> sa, sb;
    bests(x, block, reverse != 0, &ba, &sa, &bb, &sb);
    std::vector<uint32_t> sa_bits(sa.size()), sb_bits(sb.size());
    for (size_t i = 0; i < sa.size(); ++i) sa_bits[i] = to_bits(sa[i]);
    for (size_t i = 0; i < sb.size(); ++i) sb_bits[i] = to_bits(sb[i]);
    std::cout << name << '|';
    print_list(ba);
    std::cout << '|';
    print_list(sa_bits);
    std::cout << '|';
    print_list(bb);
    std::cout << '|';
    print_list(sb_bits);
    std::cout << '\n';
}

static void run_mutual(std::istringstream& in) {
    std::string name, path;
    uint32_t thr_bits = 0;
    if (!(in >> name >> path >> thr_bits)) return;
    const Matrix x = read_matrix(path);
    if (!x.ok) { std::cout << name << "|unreadable\n"; return; }
    std::vector<uint64_t> ba, bb;
    std::vector<float> sa, sb;
    bests(x, std::max<uint64_t>(1, std::max(x.m_a, x.m_b)), false, &ba, &sa, &bb, &sb);
    const auto pairs = mutual_pairs(ba.data(), sa.data(), x.m_a, bb.data(), x.m_b, from_bits(thr_bits));
    std::cout << name << '|';
    for (size_t i = 0; i < pairs.size(); ++i) std::cout << (i ? "," : "") << pairs[i].first << ':' << pairs[i].second;
    std::cout << '\n';
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "plan") run_plan(in);
        else if (kind == "key") run_key(in);
        else if (kind == "merge") run_merge(in);
        else if (kind == "mutual") run_mutual(in);
    }
    return 0;
}
