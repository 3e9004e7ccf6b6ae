// Stand-alone driver of cqs_amd/csrc/umap_transform_host.h (tests/test_umap_transform_host_cpu.py builds it with ASAN +
// UBSan and feeds it its cases on stdin).  Kinds of line and their answers:
//     plan name params arrays anchors out n m_declared m_real stride a b lr repulsion neg n_epochs id_base counts[m_real] rows[m_real*stride]
//         name|ok|why|nothing|n_epochs      the arrays hold m_real vertices exactly (heap: a read past them is ASAN's to
//                                           find); m_declared is what the plan is told
//     epochs name m                     name|default E for m
//     run name epochs E                 name|epochs the call runs
//     alpha name lr_bits e E            name|bits
//     target name c                     name|bits of log2f(c)
//     place name n c score_bits[c] ids[c] xy_bits[2n]
//         name|sigma bits|weight bits, comma separated|bits of x|bits of y|placed
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/umap_transform_host.h"

using namespace cqs_umap;

static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static float float_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static float read_float(std::istringstream& in) { std::string s; in >> s; return strtof(s.c_str(), nullptr); }

static void run_plan(std::istringstream& in) {
    std::string name;
    int params = 0, arrays = 0, anchors = 0, out = 0;
    uint64_t n = 0, m_declared = 0, m_real = 0, id_base = 0;
    uint32_t stride = 0;
    in >> name >> params >> arrays >> anchors >> out >> n >> m_declared >> m_real >> stride;
    cqs_hip_layout_params p;
    p.a = read_float(in); p.b = read_float(in); p.learning_rate = read_float(in); p.repulsion = read_float(in);
    in >> p.negative_samples >> p.n_epochs >> id_base;
    p.seed = 42;
    const size_t slots = (size_t)m_real * stride;
    std::unique_ptr<uint32_t[]> counts(new uint32_t[m_real]);
    std::unique_ptr<uint64_t[]> rows(new uint64_t[slots]);
    std::unique_ptr<float[]> scores(new float[slots]);
    for (size_t i = 0; i < m_real; ++i) in >> counts[i];
    for (size_t i = 0; i < slots; ++i) { in >> rows[i]; scores[i] = 0.5f; }
    TransformPlanned pl;
    char why[192];
    const bool ok = plan_transform(n, anchors != 0, m_declared, stride, arrays ? rows.get() : nullptr, arrays ? scores.get() : nullptr,
                                   arrays ? counts.get() : nullptr, params ? &p : nullptr, p.n_epochs, id_base, out != 0, &pl, why,
                                   sizeof why);
    std::cout << name << '|' << (ok ? 1 : 0) << '|' << why << '|' << (pl.nothing ? 1 : 0) << '|' << pl.n_epochs << '\n';
}

static void run_place(std::istringstream& in) {
    std::string name;
    uint64_t n = 0;
    uint32_t c = 0;
    in >> name >> n >> c;
    std::vector<float> scores(c), xy(2 * n), w(c);
    std::vector<uint64_t> ids(c);
    for (auto& s : scores) { uint32_t b; in >> b; s = float_of(b); }
    for (auto& i : ids) in >> i;
    for (auto& v : xy) { uint32_t b; in >> b; v = float_of(b); }
    const float sigma = transform_weights(scores.data(), c, w.data());
    float x = 7.f, y = 7.f;
    const bool placed = transform_initial(w.data(), ids.data(), c, xy.data(), &x, &y);
    std::cout << name << '|' << bits_of(sigma) << '|';
    for (size_t i = 0; i < w.size(); ++i) std::cout << (i ? "," : "") << bits_of(w[i]);
    std::cout << '|' << bits_of(x) << '|' << bits_of(y) << '|' << (placed ? 1 : 0) << '\n';
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, name;
        if (!(in >> kind)) continue;
        if (kind == "plan") run_plan(in);
        else if (kind == "place") run_place(in);
        else if (kind == "epochs") {
            uint64_t m = 0;
            in >> name >> m;
            std::cout << name << '|' << transform_default_epochs(m) << '\n';
        } else if (kind == "run") {
            uint32_t epochs = 0, E = 0;
            in >> name >> epochs >> E;
            std::cout << name << '|' << transform_epochs_to_run(epochs, E) << '\n';
        } else if (kind == "alpha") {
            uint32_t lb = 0, e = 0, E = 0;
            in >> name >> lb >> e >> E;
            std::cout << name << '|' << bits_of(transform_alpha(float_of(lb), e, E)) << '\n';
        } else if (kind == "target") {
            uint32_t c = 0;
            in >> name >> c;
            std::cout << name << '|' << bits_of(transform_target(c)) << '\n';
        }
    }
    return 0;
}
