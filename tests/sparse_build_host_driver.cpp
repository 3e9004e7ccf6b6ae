// sparse_build_host_driver.cpp — cqs_amd/csrc/sparse_build_host.h and sparse_file_host.h as a stand-alone CPU program (built
// with ASAN + UBSan by tests/test_sparse_build_host_cpu.py): the constructors' host builders, the directory fill, the term
// resolution of a search and the file's writer and reader, each over the arrays of one case; the test compares what is
// printed with its own restatement in Python.
//
// One case per line, fields separated by '|', lists of integers separated by spaces, "null" = a NULL pointer:
//   name|docs|n|doc_off|tokens|weight bits|id_rank
//   name|inverted|n|n_tokens|token_ids|list_off|chunks|weight bits|id_rank
//   name|dirs|n|n_cu|doc_off|tokens|weight bits
//   name|resolve|n|doc_off|tokens|weight bits|b|q_off|q_tokens|q weight bits
//   name|write|path|ranked|n|generation|tokens|offsets|postings position:bits|chunk_of_rank
//   name|read|path|expected_chunks|generation
// Output: name|status|why|... (see each run_* below)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/sparse_build_host.h"
#include "../cqs_amd/csrc/sparse_file_host.h"

namespace sb = cqs_sparse_build;
namespace sf = cqs_sparse_file;

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

// An argument array exactly as long as the case says (so that a read past its end is ASAN's to find); nullptr for "null".
template <class T>
struct Arg {
    bool null;
    std::vector<T> v;
    explicit Arg(const List& l) : null(l.null) { for (uint64_t x : l.v) v.push_back((T)x); }
    const T* p() const { return null ? nullptr : v.data(); }
};
struct Weights {                                    // from bit patterns: a NaN's payload survives
    bool null;
    std::vector<float> v;
    explicit Weights(const List& l) : null(l.null), v(l.v.size()) {
        for (size_t i = 0; i < l.v.size(); ++i) { const uint32_t b = (uint32_t)l.v[i]; memcpy(&v[i], &b, 4); }
    }
    const float* p() const { return null ? nullptr : v.data(); }
};

template <class V>
static void put(const V& v) {
    for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? " " : "") << v[i];
    std::cout << '|';
}
static void put(const std::vector<sb::Posting>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? " " : "") << v[i].x << ':' << v[i].y;
    std::cout << '|';
}

// name|status|why|n|tokens|offsets|postings|chunk_of_rank|
static void print_index(const std::string& name, const char* status, const char* why, uint64_t n, const sb::Built& x,
                        const std::vector<uint32_t>& cor) {
    std::cout << name << '|' << status << '|' << why << '|' << n << '|';
    put(x.tok); put(x.off); put(x.post); put(cor);
    std::cout << '\n';
}

// The order of cqs_hip_sparse_index_create: the CSR, then the id order, then the build.
static void run_docs(const std::vector<std::string>& f) {
    const uint64_t n = std::stoull(f[2]);
    const Arg<uint64_t> off(parse_list(f[3]));
    const Arg<uint32_t> tok(parse_list(f[4])), rank(parse_list(f[6]));
    const Weights w(parse_list(f[5]));
    const char* why = "";
    std::vector<uint32_t> cor;
    if (!sb::check_csr(off.p(), n, tok.p(), w.p(), &why)) return print_index(f[0], "csr", why, n, sb::Built(), cor);
    if (!sb::rank_table(n, rank.p(), &cor)) return print_index(f[0], "rank", why, n, sb::Built(), {});
    print_index(f[0], "ok", why, n, sb::from_documents(off.p(), tok.p(), w.p(), n, cor), cor);
}

static void run_inverted(const std::vector<std::string>& f) {
    const uint64_t n = std::stoull(f[2]), n_tokens = std::stoull(f[3]);
    const Arg<uint32_t> ids(parse_list(f[4])), chunks(parse_list(f[6])), rank(parse_list(f[8]));
    const Arg<uint64_t> off(parse_list(f[5]));
    const Weights w(parse_list(f[7]));
    const char* why = "";
    std::vector<uint32_t> cor;
    sb::Built x;
    if (!sb::check_csr(off.p(), n_tokens, chunks.p(), w.p(), &why)) return print_index(f[0], "csr", why, n, sb::Built(), cor);
    if (!sb::rank_table(n, rank.p(), &cor)) return print_index(f[0], "rank", why, n, sb::Built(), {});
    if (!sb::from_inverted(ids.p(), off.p(), chunks.p(), w.p(), n_tokens, n, cor, &x)) return print_index(f[0], "twice", why, n, sb::Built(), cor);
    print_index(f[0], "ok", why, n, x, cor);
}

static void put_dir_off(const std::vector<uint64_t>& dir_off) {
    for (size_t i = 0; i < dir_off.size(); ++i) {
        std::cout << (i ? " " : "");
        if (dir_off[i] == cqs::kNoDir) std::cout << "-"; else std::cout << dir_off[i];
    }
    std::cout << '|';
}

// name|ok||rw|n_pad|planned entries|dir_off ("-" = none)|dirs|offsets|postings|
static void run_dirs(const std::vector<std::string>& f) {
    const uint64_t n = std::stoull(f[2]);
    const Arg<uint64_t> off(parse_list(f[4]));
    const Arg<uint32_t> tok(parse_list(f[5]));
    const Weights w(parse_list(f[6]));
    const sb::Built x = sb::from_documents(off.p(), tok.p(), w.p(), n, {});
    const cqs::SparseGeometry geo = cqs::sparse_geometry(n, (uint32_t)std::stoul(f[3]));
    std::vector<uint64_t> dir_off;
    const uint64_t used = cqs::sparse_plan_directories(x.off, geo, &dir_off);
    std::vector<uint32_t> dirs;
    sb::fill_directories(x.post.data(), x.off, dir_off, geo, &dirs);
    std::cout << f[0] << "|ok||" << geo.rw << '|' << geo.n_pad << '|' << used << '|';
    put_dir_off(dir_off); put(dirs); put(x.off); put(x.post);
    std::cout << '\n';
}

// The order of search_locked: the batch checked, then its terms resolved into arrays that hold exactly the batch's terms.
// name|status|why|first terms|terms start:dir:len:weight bits|touched|tokens|offsets|dir_off|
static void run_resolve(const std::vector<std::string>& f) {
    const uint64_t n = std::stoull(f[2]);
    const Arg<uint64_t> off(parse_list(f[3])), q_off(parse_list(f[7]));
    const Arg<uint32_t> tok(parse_list(f[4])), q_tok(parse_list(f[8]));
    const Weights w(parse_list(f[5])), q_w(parse_list(f[9]));
    const uint32_t b = (uint32_t)std::stoul(f[6]);
    const sb::Built x = sb::from_documents(off.p(), tok.p(), w.p(), n, {});
    std::vector<uint64_t> dir_off;
    cqs::sparse_plan_directories(x.off, cqs::sparse_geometry(n, 256u), &dir_off);
    const char* why = "";
    const char* status = "ok";
    std::vector<cqs::SparseTerm> terms;
    std::vector<uint32_t> qoff;
    uint64_t touched = 0;
    if (!sb::check_queries(q_off.p(), q_tok.p(), q_w.p(), b, &why)) {
        status = "queries";
    } else {
        terms.resize((size_t)(q_off.v[b] - q_off.v[0]));
        qoff.assign((size_t)b + 1, 0xFFFFFFFFu);
        if (!sb::resolve_terms(x.tok, x.off, dir_off, q_off.p(), q_tok.p(), q_w.p(), b, terms.data(), qoff.data(), &touched, &why)) {
            status = "terms";
            qoff.clear();
        }
        terms.resize(qoff.empty() ? 0 : qoff[b]);
    }
    std::cout << f[0] << '|' << status << '|' << why << '|';
    put(qoff);
    for (size_t i = 0; i < terms.size(); ++i) {
        std::cout << (i ? " " : "") << terms[i].start << ':';
        if (terms[i].dir == cqs::kNoDir) std::cout << "-"; else std::cout << terms[i].dir;
        std::cout << ':' << terms[i].len << ':' << sb::weight_bits(terms[i].w);
    }
    std::cout << '|' << touched << '|';
    put(x.tok); put(x.off); put_dir_off(dir_off);
    std::cout << '\n';
}

// name|status||checksum|
static void run_write(const std::vector<std::string>& f) {
    const Arg<uint32_t> tok(parse_list(f[6])), cor(parse_list(f[9]));
    const Arg<uint64_t> off(parse_list(f[7]));
    std::vector<sb::Posting> post;
    for (const std::string& p : split(f[8], ' ')) {
        if (p.empty()) continue;
        const size_t c = p.find(':');
        post.push_back(sb::Posting{(uint32_t)std::stoul(p.substr(0, c)), (uint32_t)std::stoul(p.substr(c + 1))});
    }
    sf::SparseFileHeader h = sf::make_header(f[3] == "1", std::stoull(f[4]), tok.v.size(), post.size(), std::stoull(f[5]));
    const void* const sections[4] = {tok.v.data(), off.v.data(), post.data(), cor.v.data()};
    uint64_t checksum = 0;
    const int fd = open(f[2].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    const bool ok = fd >= 0 && sf::write_file(fd, h, sections, &checksum);
    if (fd >= 0) close(fd);
    std::cout << f[0] << '|' << (ok ? "ok" : "failed") << "||" << checksum << "|\n";
}

// name|ok / header / sections / structure / open||ranked|n|tokens|offsets|postings|chunk_of_rank|
static void run_read(const std::vector<std::string>& f) {
    static const char* const kStage[] = {"ok", "header", "sections", "structure"};
    sf::SparseFileHeader h{};
    sb::Built x;
    std::vector<uint32_t> cor;
    const int fd = open(f[2].c_str(), O_RDONLY);
    const char* status = "open";
    if (fd >= 0) {
        status = kStage[(int)sf::read_file(fd, std::stoull(f[3]), std::stoull(f[4]), &h, &x.tok, &x.off, &x.post, &cor)];
        close(fd);
    }
    if (strcmp(status, "ok") != 0) { x = sb::Built(); cor.clear(); h = sf::SparseFileHeader{}; }
    std::cout << f[0] << '|' << status << "||" << h.ranked << '|' << h.chunks << '|';
    put(x.tok); put(x.off); put(x.post); put(cor);
    std::cout << '\n';
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const std::vector<std::string> f = split(line, '|');
        const std::string kind = f.size() > 1 ? f[1] : "";
        if (kind == "docs" && f.size() == 7) run_docs(f);
        else if (kind == "inverted" && f.size() == 9) run_inverted(f);
        else if (kind == "dirs" && f.size() == 7) run_dirs(f);
        else if (kind == "resolve" && f.size() == 10) run_resolve(f);
        else if (kind == "write" && f.size() == 10) run_write(f);
        else if (kind == "read" && f.size() == 5) run_read(f);
        else { fprintf(stderr, "bad case line\n"); return 2; }
    }
    return 0;
}
