// Stand-alone driver of cqs_amd/csrc/umap_host.h (tests/test_umap_host_cpu.py builds it with ASAN + UBSan and feeds it its
// cases on stdin).  Kinds of line and their answers:
//     plan name out params arrays n_declared n_real stride a b lr repulsion neg n_epochs seed counts[n_real] rows[n_real*stride]
//         name|ok|why|n_epochs      the arrays hold n_real vertices exactly (heap: a read past them is ASAN's to find);
//                                   n_declared is what the plan is told, so n > 2^31 needs no such arrays
//     adj name n stride counts[n] rows[n*stride] score_bits[n*stride]
//         name|offsets|nbrs|distance bits
//     active name p_bits e_max          name|one 0/1 per epoch 1 .. e_max
//     hash name seed epoch vertex slot draw n      name|hash|drawn vertex
//     init name seed vertex             name|bits of x|bits of y
//     alpha name lr_bits e E            name|bits
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/umap_host.h"

using namespace cqs_umap;

static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float float_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static float read_float(std::istringstream& in) { std::string s; in >> s; return strtof(s.c_str(), nullptr); }

static void run_plan(std::istringstream& in) {
    std::string name;
    int out = 0, params = 0, arrays = 0;
    uint64_t n_declared = 0, n_real = 0;
    uint32_t stride = 0;
    in >> name >> out >> params >> arrays >> n_declared >> n_real >> stride;
    cqs_hip_layout_params p;
    p.a = read_float(in); p.b = read_float(in); p.learning_rate = read_float(in); p.repulsion = read_float(in);
    in >> p.negative_samples >> p.n_epochs >> p.seed;
    // exact-size heap arrays (non-null even where empty)
    const size_t slots = (size_t)n_real * stride;
    std::unique_ptr<uint32_t[]> counts(new uint32_t[n_real]);
    std::unique_ptr<uint64_t[]> rows(new uint64_t[slots]);
    std::unique_ptr<float[]> scores(new float[slots]);
    for (size_t i = 0; i < n_real; ++i) in >> counts[i];
    for (size_t i = 0; i < slots; ++i) { in >> rows[i]; scores[i] = 0.5f; }
    Planned pl;
    char why[192];
    const bool ok = plan_layout(out != 0, n_declared, stride, arrays ? rows.get() : nullptr, arrays ? scores.get() : nullptr,
                                arrays ? counts.get() : nullptr, params ? &p : nullptr, &pl, why, sizeof why);
    std::cout << name << '|' << (ok ? 1 : 0) << '|' << why << '|' << pl.n_epochs << '\n';
}

static void run_adj(std::istringstream& in) {
    std::string name;
    uint64_t n = 0;
    uint32_t stride = 0;
    in >> name >> n >> stride;
    std::vector<uint32_t> counts(n);
    std::vector<uint64_t> rows(n * stride);
    std::vector<float> scores(n * stride);
    for (auto& c : counts) in >> c;
    for (auto& r : rows) in >> r;
    for (auto& s : scores) { uint32_t b; in >> b; s = float_of(b); }
    Adjacency adj;
    build_adjacency(n, stride, rows.data(), scores.data(), counts.data(), &adj);
    std::cout << name << '|';
    for (size_t i = 0; i < adj.off.size(); ++i) std::cout << (i ? "," : "") << adj.off[i];
    std::cout << '|';
    for (size_t i = 0; i < adj.nbr.size(); ++i) std::cout << (i ? "," : "") << adj.nbr[i];
    std::cout << '|';
    for (size_t i = 0; i < adj.dist.size(); ++i) std::cout << (i ? "," : "") << bits_of(adj.dist[i]);
    std::cout << '\n';
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, name;
        if (!(in >> kind)) continue;
        if (kind == "plan") run_plan(in);
        else if (kind == "adj") run_adj(in);
        else if (kind == "active") {
            uint32_t pb = 0, e_max = 0;
            in >> name >> pb >> e_max;
            std::cout << name << '|';
            for (uint32_t e = 1; e <= e_max; ++e) std::cout << (active(e, float_of(pb)) ? '1' : '0');
            std::cout << '\n';
        } else if (kind == "hash") {
            uint64_t seed = 0, n = 0;
            uint32_t epoch = 0, vertex = 0, slot = 0, draw = 0;
            in >> name >> seed >> epoch >> vertex >> slot >> draw >> n;
            const uint32_t h = hash5(seed, epoch, vertex, slot, draw);
            std::cout << name << '|' << h << '|' << draw_vertex(h, n) << '\n';
        } else if (kind == "init") {
            uint64_t seed = 0;
            uint32_t vertex = 0;
            in >> name >> seed >> vertex;
            std::cout << name << '|' << bits_of(initial_coord(seed, vertex, 0)) << '|' << bits_of(initial_coord(seed, vertex, 1)) << '\n';
        } else if (kind == "alpha") {
            uint32_t lb = 0, e = 0, E = 0;
            in >> name >> lb >> e >> E;
            std::cout << name << '|' << bits_of(alpha_of(float_of(lb), e, E)) << '\n';
        }
    }
    return 0;
}
