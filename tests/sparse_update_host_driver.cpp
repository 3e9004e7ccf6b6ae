// sparse_update_host_driver.cpp — cqs_amd/csrc/sparse_update_host.h as a stand-alone CPU program (built with ASAN + UBSan
// by tests/test_sparse_update_host_cpu.py): for every case on stdin, the canonical arrays of the index built from the
// documents by the library's own host builder (sparse_build_host.h: what cqs_hip_sparse_index_create builds), the plan of
// a remove or an extend, and the position rules the kernels implement replayed over host arrays.  Prints the resulting index; the test compares it with its own
// from-scratch build of the resulting documents.
//
// One case per line, fields separated by '|', lists of integers separated by spaces, "null" = a NULL pointer:
//   name|remove|n|doc_off|tokens|weight bits|id_rank|chunks|m
//   name|extend|n|doc_off|tokens|weight bits|id_rank|n_new|doc_off|tokens|weight bits|new_rank
// Output: name|plan|why|chunks|tokens|offsets|postings position:bits|chunk_of_rank|checks
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/sparse_update_host.h"

namespace su = cqs_sparse_update;

struct List {
    bool null = false;
    std::vector<uint64_t> v;
};

static List parse_list(const std::string& s) {
    List l;
    if (s == "null") { l.null = true; return l; }
    std::istringstream in(s);
    uint64_t x;
    while (in >> x) l.v.push_back(x);
    return l;
}

static std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    std::string cur;
    for (char c : s) {
        if (c == sep) { out.push_back(cur); cur.clear(); } else cur += c;
    }
    out.push_back(cur);
    return out;
}

template <class T>
static std::vector<T> narrow(const List& l) {
    std::vector<T> v;
    for (uint64_t x : l.v) v.push_back((T)x);
    return v;
}

struct Index {
    uint64_t n = 0;
    bool ranked = false;
    std::vector<uint32_t> tok;
    std::vector<uint64_t> off;
    std::vector<su::Posting> post;
    std::vector<uint32_t> chunk_of_rank;
};

// cqs_hip_sparse_index_create's arrays, by the library's own builder (sparse_build_host.h).
static Index build(uint64_t n, const std::vector<uint64_t>& doc_off, const std::vector<uint32_t>& tokens, const std::vector<uint32_t>& wbits,
                   const List& id_rank) {
    Index x;
    x.n = n;
    x.ranked = !id_rank.null;
    const std::vector<uint32_t> rank = narrow<uint32_t>(id_rank);
    std::vector<float> w(wbits.size());
    if (!wbits.empty()) memcpy(w.data(), wbits.data(), wbits.size() * 4);
    const char* why = "";
    if (!cqs_sparse_build::check_csr(doc_off.data(), n, tokens.data(), w.data(), &why) ||
        !cqs_sparse_build::rank_table(n, x.ranked ? rank.data() : nullptr, &x.chunk_of_rank)) {
        fprintf(stderr, "bad case index: %s\n", why);
        exit(2);
    }
    cqs_sparse_build::Built b = cqs_sparse_build::from_documents(doc_off.data(), tokens.data(), w.data(), n, x.chunk_of_rank);
    x.tok.swap(b.tok);
    x.off.swap(b.off);
    x.post.swap(b.post);
    return x;
}

static void print(const std::string& name, int plan, const char* why, const Index& x, bool checks) {
    std::cout << name << '|' << plan << '|' << why << '|' << x.n << '|';
    for (size_t i = 0; i < x.tok.size(); ++i) std::cout << (i ? " " : "") << x.tok[i];
    std::cout << '|';
    for (size_t i = 0; i < x.off.size(); ++i) std::cout << (i ? " " : "") << x.off[i];
    std::cout << '|';
    for (size_t i = 0; i < x.post.size(); ++i) std::cout << (i ? " " : "") << x.post[i].x << ':' << x.post[i].y;
    std::cout << '|';
    for (size_t i = 0; i < x.chunk_of_rank.size(); ++i) std::cout << (i ? " " : "") << x.chunk_of_rank[i];
    std::cout << '|' << (checks ? 1 : 0) << '\n';
}

static const uint32_t kUnwritten = 0xFFFFFFFEu;

static void run_remove(const std::string& name, const Index& old, const List& chunks, uint64_t m) {
    su::RemovePlan plan;
    const char* why = "";
    const su::Plan p = su::plan_remove(chunks.null ? nullptr : chunks.v.data(), m, old.n, old.chunk_of_rank, &plan, &why);
    if (p != su::Plan::Update) {
        const bool nothing_planned = plan.removed.empty() && plan.remap.empty() && plan.chunk_of_rank.empty() && plan.n_new == old.n;
        print(name, (int)p, why, old, nothing_planned);
        return;
    }
    bool ok = true;
    const uint64_t P = old.post.size();
    // K: the global exclusive count of kept postings
    std::vector<uint64_t> K(P + 1, 0);
    for (uint64_t e = 0; e < P; ++e) K[e + 1] = K[e] + (plan.remap[old.post[e].x] != su::kGone ? 1 : 0);
    std::vector<uint64_t> k_start(old.tok.size() + 1);
    for (size_t t = 0; t <= old.tok.size(); ++t) k_start[t] = K[old.off[t]];
    Index nw;
    nw.n = plan.n_new;
    nw.ranked = old.ranked;
    su::remove_token_table(old.tok, k_start, &nw.tok, &nw.off);
    nw.chunk_of_rank = plan.chunk_of_rank;
    nw.post.assign(nw.off.back(), su::Posting{kUnwritten, 0});
    size_t slot = 0;                        // slot(t) of the surviving lists, in order
    for (size_t t = 0; t < old.tok.size(); ++t) {
        if (k_start[t + 1] == k_start[t]) continue;
        ok = ok && slot < nw.tok.size() && nw.tok[slot] == old.tok[t];
        for (uint64_t e = old.off[t]; e < old.off[t + 1]; ++e) {
            const uint32_t r = plan.remap[old.post[e].x];
            if (r == su::kGone) continue;
            ok = ok && su::list_of(old.off.data(), (uint32_t)old.tok.size(), e) == t;
            const uint64_t pos = su::remove_position(nw.off[slot], K[e], k_start[t]);
            ok = ok && pos == su::remove_position(0, K[e], 0);          // the form the device uses
            if (pos >= nw.post.size() || nw.post[pos].x != kUnwritten) { ok = false; continue; }
            nw.post[pos] = su::Posting{r, old.post[e].y};
        }
        ++slot;
    }
    ok = ok && slot == nw.tok.size();
    for (const su::Posting& q : nw.post) ok = ok && q.x != kUnwritten;
    print(name, (int)p, why, nw, ok);
}

static void run_extend(const std::string& name, const Index& old, uint64_t n_new, const List& doc_off, const List& tokens, const List& wbits,
                       const List& new_rank) {
    const std::vector<uint32_t> tk = narrow<uint32_t>(tokens), wb = narrow<uint32_t>(wbits), nr = narrow<uint32_t>(new_rank);
    std::vector<float> w(wb.size());
    if (!wb.empty()) memcpy(w.data(), wb.data(), wb.size() * 4);
    su::ExtendPlan plan;
    const char* why = "";
    const su::Plan p = su::plan_extend(doc_off.null ? nullptr : doc_off.v.data(), tokens.null ? nullptr : tk.data(), wbits.null ? nullptr : w.data(),
                                       n_new, new_rank.null ? nullptr : nr.data(), old.n, old.ranked, old.chunk_of_rank, old.tok, old.off, &plan,
                                       &why);
    if (p != su::Plan::Update) {
        const bool nothing_planned = plan.lift.empty() && plan.tok.empty() && plan.off.empty() && plan.added.empty() &&
                                     plan.chunk_of_rank.empty() && plan.n_total == old.n;
        print(name, (int)p, why, old, nothing_planned);
        return;
    }
    bool ok = true;
    Index nw;
    nw.n = plan.n_total;
    nw.ranked = old.ranked;
    nw.tok = plan.tok;
    nw.off = plan.off;
    nw.chunk_of_rank = plan.chunk_of_rank;
    nw.post.assign(nw.off.back(), su::Posting{kUnwritten, 0});
    const uint32_t old_lists = (uint32_t)old.tok.size();
    for (uint64_t e = 0; e < old.post.size(); ++e) {                      // extend_move_kernel
        const uint32_t t = su::list_of(old.off.data(), old_lists, e);
        const uint32_t u = plan.new_slot[t];
        const uint32_t lifted = plan.lift[old.post[e].x];
        const uint64_t a0 = plan.add_off[u];
        const uint32_t below = su::count_below(plan.added.data() + a0, (uint32_t)(plan.add_off[u + 1] - a0), lifted);
        const uint64_t pos = su::extend_old_position(nw.off[u], e - old.off[t], below);
        if (pos >= nw.post.size() || nw.post[pos].x != kUnwritten) { ok = false; continue; }
        nw.post[pos] = su::Posting{lifted, old.post[e].y};
    }
    for (uint64_t a = 0; a < plan.added.size(); ++a) {                    // extend_place_kernel
        const uint32_t u = plan.added_slot[a];
        const uint32_t t = plan.old_slot[u];
        uint32_t below = 0;
        if (t != su::kGone) below = su::count_below(old.post.data() + old.off[t], (uint32_t)(old.off[t + 1] - old.off[t]), plan.added_thr[a]);
        const uint64_t pos = su::extend_added_position(nw.off[u], a - plan.add_off[u], below);
        if (pos >= nw.post.size() || nw.post[pos].x != kUnwritten) { ok = false; continue; }
        nw.post[pos] = plan.added[a];
    }
    for (const su::Posting& q : nw.post) ok = ok && q.x != kUnwritten;
    print(name, (int)p, why, nw, ok);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const std::vector<std::string> f = split(line, '|');
        if (f.size() < 9) { fprintf(stderr, "bad case line\n"); return 2; }
        const uint64_t n = std::stoull(f[2]);
        const List doc_off = parse_list(f[3]);
        const Index old = build(n, doc_off.v, narrow<uint32_t>(parse_list(f[4])), narrow<uint32_t>(parse_list(f[5])), parse_list(f[6]));
        if (f[1] == "remove") {
            run_remove(f[0], old, parse_list(f[7]), std::stoull(f[8]));
        } else if (f[1] == "extend" && f.size() >= 12) {
            run_extend(f[0], old, std::stoull(f[7]), parse_list(f[8]), parse_list(f[9]), parse_list(f[10]), parse_list(f[11]));
        } else {
            fprintf(stderr, "bad case kind\n");
            return 2;
        }
    }
    return 0;
}
