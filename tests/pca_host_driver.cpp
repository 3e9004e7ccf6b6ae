// Runs cqs_amd/csrc/pca_host.h on the CPU (built with ASAN + UBSan by tests/test_pca_host_cpu.py).  Commands on stdin, one
// per line; one answer line each, fields separated by '|':
//   plan NAME present sharded row_base len dim n_components n_passes outputs      -> NAME|ok|why|p|passes
//   proj NAME present sharded row_base len dim mean_axes output n_components first m -> NAME|plan|why|local_first
//   start NAME seed dim                                                             -> NAME|bits of V0 [dim][8]
//   jitter NAME seed n                                                              -> NAME|bits [n][2]
//   scale NAME seed n nc bits[n*nc]                                                 -> NAME|ok|bits [n][2]
//   gs NAME dim p values[dim*8]                                                     -> NAME|replaced|values [dim][8]
//   eig NAME p values[p*p]                                                          -> NAME|lambda [p]|w [p][p]
//   sign NAME dim bits[dim]                                                         -> NAME|bits [dim]
//   finish NAME dim p n nc v[dim*8] y[dim*8]                                        -> NAME|ok|axes bits|variance bits
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/pca_host.h"

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static double read_double(std::istream& in) {   // (operator>> does not read "nan" / "inf")
    std::string tok;
    in >> tok;
    return strtod(tok.c_str(), nullptr);
}

static void print_bits(const float* v, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%s%" PRIu32, i ? "," : "", bits_of(v[i]));
}
static void print_doubles(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%s%.17g", i ? "," : "", v[i]);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, name;
        in >> cmd >> name;
        if (cmd.empty()) continue;
        printf("%s|", name.c_str());
        if (cmd == "plan") {
            int present, sharded, outputs;
            uint64_t row_base, len;
            uint32_t dim, nc, passes;
            in >> present >> sharded >> row_base >> len >> dim >> nc >> passes >> outputs;
            cqs_pca::Planned pl;
            const char* why = "";
            const bool ok = cqs_pca::plan_pca(cqs_pca::Handle{present != 0, sharded != 0, row_base, len, dim}, nc, passes, outputs != 0, &pl, &why);
            printf("%d|%s|%u|%u\n", ok ? 1 : 0, why, pl.p, pl.passes);
        } else if (cmd == "proj") {
            int present, sharded, mean_axes, output;
            uint64_t row_base, len, first, m, local = 0;
            uint32_t dim, nc;
            in >> present >> sharded >> row_base >> len >> dim >> mean_axes >> output >> nc >> first >> m;
            const char* why = "";
            const cqs_pca::Plan plan = cqs_pca::plan_project(cqs_pca::Handle{present != 0, sharded != 0, row_base, len, dim}, mean_axes != 0,
                                                             output != 0, nc, first, m, &local, &why);
            printf("%d|%s|%" PRIu64 "\n", (int)plan, why, local);
        } else if (cmd == "start") {
            uint64_t seed;
            uint32_t dim;
            in >> seed >> dim;
            std::vector<float> v((size_t)dim * cqs_pca::kBlock);
            for (uint32_t d = 0; d < dim; ++d)
                for (uint32_t j = 0; j < cqs_pca::kBlock; ++j) v[(size_t)d * cqs_pca::kBlock + j] = cqs_pca::start_entry(seed, d, j);
            print_bits(v.data(), v.size());
            printf("\n");
        } else if (cmd == "jitter") {
            uint64_t seed, n;
            in >> seed >> n;
            std::vector<float> v((size_t)n * 2);
            for (uint64_t i = 0; i < n; ++i)
                for (uint32_t c = 0; c < 2; ++c) v[2 * i + c] = cqs_pca::jitter(seed, (uint32_t)i, c);
            print_bits(v.data(), v.size());
            printf("\n");
        } else if (cmd == "scale") {
            uint64_t seed, n;
            uint32_t nc;
            in >> seed >> n >> nc;
            std::vector<float> proj((size_t)n * nc), xy((size_t)n * 2, 7.0f);
            for (float& f : proj) { uint32_t u; in >> u; f = float_of(u); }
            const bool ok = cqs_pca::noisy_scale_coords(proj.data(), n, nc, seed, xy.data());
            printf("%d|", ok ? 1 : 0);
            print_bits(xy.data(), xy.size());
            printf("\n");
        } else if (cmd == "gs") {
            uint32_t dim, p;
            in >> dim >> p;
            std::vector<double> a((size_t)dim * cqs_pca::kBlock);
            for (double& d : a) d = read_double(in);
            const uint32_t replaced = cqs_pca::gram_schmidt(a.data(), dim, p);
            printf("%u|", replaced);
            print_doubles(a.data(), a.size());
            printf("\n");
        } else if (cmd == "eig") {
            uint32_t p;
            in >> p;
            double h[64] = {0}, lambda[8] = {0}, w[64];
            for (uint32_t i = 0; i < p; ++i)
                for (uint32_t j = 0; j < p; ++j) h[i * cqs_pca::kBlock + j] = read_double(in);
            cqs_pca::jacobi_eigen(h, p, lambda, w);
            print_doubles(lambda, p);
            printf("|");
            for (uint32_t i = 0; i < p; ++i) {
                if (i) printf(",");
                print_doubles(w + i * cqs_pca::kBlock, p);
            }
            printf("\n");
        } else if (cmd == "sign") {
            uint32_t dim;
            in >> dim;
            std::vector<float> a(dim);
            for (float& f : a) { uint32_t u; in >> u; f = float_of(u); }
            cqs_pca::fix_sign(a.data(), dim);
            print_bits(a.data(), a.size());
            printf("\n");
        } else if (cmd == "finish") {
            uint32_t dim, p, nc;
            uint64_t n;
            in >> dim >> p >> n >> nc;
            std::vector<double> v((size_t)dim * cqs_pca::kBlock), y((size_t)dim * cqs_pca::kBlock);
            for (double& d : v) d = read_double(in);
            for (double& d : y) d = read_double(in);
            std::vector<float> axes((size_t)nc * dim, 7.0f), var(nc, 7.0f);
            const bool ok = cqs_pca::finish(v.data(), y.data(), dim, p, n, nc, axes.data(), var.data());
            printf("%d|", ok ? 1 : 0);
            print_bits(axes.data(), axes.size());
            printf("|");
            print_bits(var.data(), var.size());
            printf("\n");
        } else {
            printf("?\n");
            return 2;
        }
    }
    return 0;
}
