// Stand-alone driver of cqs_amd/csrc/batch_tables.h (tests/test_batch_tables_cpu.py builds it with ASAN + UBSan and runs it).
// Reads one case per line on stdin and answers with one line each:
//   shape K MAXLEN B len..                          -> shape CODE B M NBLK VTCOLS WORDS        (batch_shape alone: nothing allocated)
//   fill  K MAXLEN VOCAB TYPEVOCAB B len.. tok.. [ty..]  -> fill CODE B M NBLK VTCOLS WORDS w..  (the block, word by word; ty.. for K = 1)
//   mask  B L MAXSEQ m..                            -> mask CODE len..
//   ctx                                             -> ctx then pick_context for load0, load1 in 0..4, last in 0..1 (50 digits)
//   rounds NCU MMAX                                 -> rounds then exact_rounds for M = 1..MMAX (MMAX digits)
//   props SEED N                                    -> props ok N     (monotone table_words, carve inside / disjoint / tok == base)
// A filled block lives in an allocation of exactly table_words int32, so ASAN guards its end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cqs_amd/csrc/batch_tables.h"

using namespace cqs;

static void die(const char* what) { fprintf(stderr, "batch_tables_driver: %s\n", what); exit(2); }

// every non-null table inside [base, base + words), pairwise disjoint, in the order carved, ending at base + words
static void check_carve(BatchKind k, const BatchShape& s, const int32_t* base) {
    const BatchTables<const int32_t> t = carve(k, base, s);
    const size_t words = table_words(k, s);
    struct { const int32_t* p; size_t n; } tabs[] = {{t.tok, s.M}, {t.pos, s.M}, {t.tt, s.M}, {t.seq_start, s.B}, {t.seq_len, s.B},
                                                     {t.vt_start, s.B}, {t.blk, (size_t)2 * s.nblk}, {t.row_seq, s.M}};
    if (t.tok != base) die("tok is not the block's start");
    if ((k == BATCH_BERT) != (t.tt != nullptr) || (k == BATCH_BERT) != (t.row_seq != nullptr) || (k == BATCH_GEMMA) != (t.vt_start != nullptr))
        die("a kind carves a table it lacks, or lacks one it has");
    size_t sum = 0;
    for (const auto& a : tabs) {
        if (!a.p) continue;
        if (a.p < base || a.p + a.n > base + words) die("a table leaves the block");
        for (const auto& b : tabs)
            if (b.p && &a != &b && a.p < b.p + b.n && b.p < a.p + a.n) die("two tables overlap");
        sum += a.n;
    }
    if (sum != words) die("the tables do not add up to table_words");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "shape" || cmd == "fill") {
            int kind; uint32_t max_len, B; int64_t vocab = 0, type_vocab = 0;
            in >> kind >> max_len;
            if (cmd == "fill") in >> vocab >> type_vocab;
            in >> B;
            const BatchKind k = kind ? BATCH_BERT : BATCH_GEMMA;
            std::vector<uint32_t> lens(B);
            for (uint32_t& l : lens) in >> l;
            BatchShape s;
            const BatchCode code = batch_shape(k, lens.data(), B, max_len, &s);
            if (code != BATCH_OK) { printf("%s %d\n", cmd.c_str(), (int)code); continue; }
            const size_t words = table_words(k, s);
            printf("%s %d %u %u %u %u %zu", cmd.c_str(), (int)code, s.B, s.M, s.nblk, s.vt_cols, words);
            if (cmd == "shape") { printf("\n"); continue; }
            std::vector<int64_t> tok(s.M), ty(s.M, 0);
            for (int64_t& v : tok) in >> v;
            if (k == BATCH_BERT) for (int64_t& v : ty) in >> v;
            if (!in) die("short fill line");
            // the Gemma kind fetches by (sequence, position) from a padded matrix, the BERT kind by packed row: both argument forms run
            uint32_t L = 1;
            for (uint32_t l : lens) L = l > L ? l : L;
            std::vector<int64_t> padded((size_t)B * L, -99);
            for (uint32_t b = 0, m = 0; b < B; m += lens[b++])
                for (uint32_t j = 0; j < lens[b]; ++j) padded[(size_t)b * L + j] = tok[m + j];
            int32_t* block = new int32_t[words];                       // exactly table_words: ASAN guards the end
            for (size_t i = 0; i < words; ++i) block[i] = -7;
            check_carve(k, s, block);
            const BatchTables<int32_t> t = carve(k, block, s);
            const BatchCode fc = k == BATCH_GEMMA
                ? fill_tables(k, t, s, lens.data(), [&](uint32_t b, uint32_t j, uint32_t) { return padded[(size_t)b * L + j]; }, NoTypes{}, vocab, type_vocab)
                : fill_tables(k, t, s, lens.data(), [&](uint32_t, uint32_t, uint32_t row) { return tok[row]; },
                              [&](uint32_t, uint32_t, uint32_t row) { return ty[row]; }, vocab, type_vocab);
            if (fc != BATCH_OK) printf(" refused %d", (int)fc);
            else for (size_t i = 0; i < words; ++i) printf(" %d", block[i]);
            printf("\n");
            delete[] block;
        } else if (cmd == "mask") {
            uint32_t B, L, max_seq;
            in >> B >> L >> max_seq;
            int64_t* mask = new int64_t[(size_t)B * L];
            for (size_t i = 0; i < (size_t)B * L; ++i) in >> mask[i];
            uint32_t* lens = new uint32_t[B];
            const BatchCode code = prefix_lens(mask, B, L, max_seq, lens);
            printf("mask %d", (int)code);
            if (code == BATCH_OK) for (uint32_t b = 0; b < B; ++b) printf(" %u", lens[b]);
            printf("\n");
            delete[] mask; delete[] lens;
        } else if (cmd == "ctx") {
            printf("ctx ");
            for (int a = 0; a <= 4; ++a) for (int b = 0; b <= 4; ++b) for (int last = 0; last <= 1; ++last) printf("%d", pick_context(a, b, last));
            printf("\n");
        } else if (cmd == "rounds") {
            uint32_t n_cu, m_max;
            in >> n_cu >> m_max;
            std::string out(m_max, '0');
            for (uint32_t M = 1; M <= m_max; ++M) out[M - 1] = exact_rounds(M, n_cu) ? '1' : '0';
            printf("rounds %s\n", out.c_str());
        } else if (cmd == "props") {
            uint64_t st; uint32_t n;
            in >> st >> n;
            auto rnd = [&st](uint32_t mod) { st = st * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 33) % mod; };
            for (uint32_t i = 0; i < n; ++i)
                for (BatchKind k : {BATCH_GEMMA, BATCH_BERT}) {
                    const BatchShape s1{rnd(40) + 1, rnd(5000), rnd(200), rnd(6000)};
                    const BatchShape s2{s1.B + rnd(40), s1.M + rnd(5000), s1.nblk + rnd(200), s1.vt_cols + rnd(100)};
                    if (table_words(k, s1) > table_words(k, s2)) die("table_words is not monotone");
                    std::vector<int32_t> cap(table_words(k, s2) + 1);   // (+ 1: never an empty vector)
                    check_carve(k, s1, cap.data());
                    check_carve(k, s2, cap.data());
                    if (carve<const int32_t>(k, cap.data(), s1).tok != carve<const int32_t>(k, cap.data(), s2).tok) die("capacity and batch shape disagree on tok");
                }
            printf("props ok %u\n", n);
        } else die("unknown command");
    }
    return 0;
}
