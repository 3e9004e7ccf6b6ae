// batch_tables.h — the packed int32 tables a batch travels to the device in, and the rule that picks a ticket's execution
// context, for both transformer engines (embedder_run.hip, bert_run.hip).  Header-only and device-free, so the engines and
// a CPU test (tests/batch_tables_driver.cpp) run the same functions.  One block per batch, pinned on the host and copied as it
// is to the device:
//   Gemma kind: [tok M][pos M][seq_start B][seq_len B][vt_start B][blk 2 nblk]                 (attention blocks of 128 rows)
//   BERT kind:  [tok M][pos M][tt M][seq_start B][seq_len B][blk 2 nblk][row_seq M]            (attention blocks of 64 rows)
// M = packed tokens, B = sequences, nblk = attention row blocks; blk holds (sequence, block in the sequence) pairs, vt_start
// the sequence's first column of V^T (lengths padded to 32), row_seq the sequence of a packed row.  carve() is the only place
// where an offset is computed.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cqs {

enum BatchKind { BATCH_GEMMA = 0, BATCH_BERT = 1 };
enum BatchCode { BATCH_OK = 0, BATCH_TOO_LONG, BATCH_TOO_MANY_TOKENS, BATCH_BAD_TOKEN, BATCH_BAD_TYPE, BATCH_MASK_NOT_PREFIX };

constexpr uint32_t batch_block_rows(BatchKind k) { return k == BATCH_GEMMA ? 128u : 64u; }

struct BatchShape { uint32_t B = 0, M = 0, nblk = 0, vt_cols = 0; };   // vt_cols: columns of V^T (Gemma kind; 0 otherwise)

inline BatchCode batch_shape(BatchKind k, const uint32_t* lens, uint32_t B, uint32_t max_len, BatchShape* s) {
    uint64_t M = 0, nblk = 0;
    uint32_t vcols = 0;
    for (uint32_t b = 0; b < B; ++b) {
        if (lens[b] > max_len) return BATCH_TOO_LONG;
        M += lens[b];
        nblk += (lens[b] + batch_block_rows(k) - 1u) / batch_block_rows(k);
        vcols += (lens[b] + 31u) / 32u * 32u;
    }
    if (M > 0x7FFFFFFFull) return BATCH_TOO_MANY_TOKENS;
    s->B = B; s->M = (uint32_t)M; s->nblk = (uint32_t)nblk; s->vt_cols = k == BATCH_GEMMA ? vcols + 32u : 0u;
    return BATCH_OK;
}

// int32 words of a batch's block.  Monotone in each of M, B and nblk: a block sized from capacities holds every batch within them.
inline size_t table_words(BatchKind k, const BatchShape& s) {
    return (size_t)(k == BATCH_GEMMA ? 2 : 4) * s.M + (size_t)(k == BATCH_GEMMA ? 3 : 2) * s.B + (size_t)2 * s.nblk;
}

template <class I>   // int32_t or const int32_t; tables a kind lacks are null
struct BatchTables { I *tok = nullptr, *pos = nullptr, *tt = nullptr, *seq_start = nullptr, *seq_len = nullptr, *vt_start = nullptr, *blk = nullptr, *row_seq = nullptr; };

// The same call carves the pinned host block and the device block (tok == base for both kinds).
template <class I>
BatchTables<I> carve(BatchKind k, I* base, const BatchShape& s) {
    const bool bert = k == BATCH_BERT;
    auto take = [&base](bool has, size_t n) -> I* { I* p = has ? base : nullptr; if (has) base += n; return p; };
    BatchTables<I> t;
    t.tok = take(true, s.M); t.pos = take(true, s.M); t.tt = take(bert, s.M);
    t.seq_start = take(true, s.B); t.seq_len = take(true, s.B); t.vt_start = take(!bert, s.B);
    t.blk = take(true, (size_t)2 * s.nblk); t.row_seq = take(bert, s.M);
    return t;
}

struct NoTypes { int64_t operator()(uint32_t, uint32_t, uint32_t) const { return 0; } };

// Fill a block carved at `s` (= batch_shape of the same lens).  tok_at / type_at (sequence, position in it, packed row) fetch
// one id; ids outside [0, vocab) / [0, type_vocab) are refused (the type ids only where the kind has tt).
template <class TokAt, class TypeAt>
BatchCode fill_tables(BatchKind k, const BatchTables<int32_t>& t, const BatchShape& s, const uint32_t* lens, TokAt tok_at, TypeAt type_at,
                      int64_t vocab, int64_t type_vocab) {
    uint32_t m = 0, vcols = 0, nb = 0;
    for (uint32_t b = 0; b < s.B; ++b) {
        const uint32_t len = lens[b];
        t.seq_start[b] = (int32_t)m; t.seq_len[b] = (int32_t)len;
        if (t.vt_start) t.vt_start[b] = (int32_t)vcols;
        for (uint32_t j = 0; j < len; ++j) {
            const int64_t id = tok_at(b, j, m + j);
            if (id < 0 || id >= vocab) return BATCH_BAD_TOKEN;
            t.tok[m + j] = (int32_t)id; t.pos[m + j] = (int32_t)j;
            if (t.tt) {
                const int64_t ty = type_at(b, j, m + j);
                if (ty < 0 || ty >= type_vocab) return BATCH_BAD_TYPE;
                t.tt[m + j] = (int32_t)ty; t.row_seq[m + j] = (int32_t)b;
            }
        }
        for (uint32_t q = 0; q * batch_block_rows(k) < len; ++q) { t.blk[2 * nb] = (int32_t)b; t.blk[2 * nb + 1] = (int32_t)q; ++nb; }
        m += len;
        vcols += (len + 31u) / 32u * 32u;
    }
    return BATCH_OK;
}

// Lengths of a padded [B, L] batch whose mask rows must be 1...10...0, none longer than max_seq.
inline BatchCode prefix_lens(const int64_t* mask, uint32_t B, uint32_t L, uint32_t max_seq, uint32_t* lens) {
    for (uint32_t b = 0; b < B; ++b) {
        const int64_t* row = mask + (size_t)b * L;
        uint32_t len = 0;
        while (len < L && row[len] != 0) ++len;
        for (uint32_t j = len; j < L; ++j)
            if (row[j] != 0) return BATCH_MASK_NOT_PREFIX;
        if (len > max_seq) return BATCH_TOO_LONG;
        lens[b] = len;
    }
    return BATCH_OK;
}

// The context with fewer tickets in flight; ties alternate - so pipelined callers interleave two kernel chains on the device,
// while ONE blocking call at a time always lands on context 0: the same activation scratch (and the same captured query
// graphs) call after call instead of two sets taking turns in L2 / the Infinity Cache.
constexpr int pick_context(int load0, int load1, int last_ctx) {
    return load0 == load1 ? (load0 == 0 ? 0 : 1 - last_ctx) : (load0 < load1 ? 0 : 1);
}

// Gemma engine: a batch whose kernels are EXACT rounds of the CUs stays on context 0 whatever pick_context says.
// Such a batch (16 384 or 32 768 tokens on 256 CUs: 128 / 256 row blocks x 2 workgroups) leaves a second chain nothing to fill -
// side by side the two only contend.  Tickets in flight, chunks/s, two contexts | one | blocking calls (a round-4 sweep script,
// since deleted, same box): 12 288 tokens 6 370 | 5 480 | 5 510; 14 336: 6 530 | 6 175 | 6 130; 16 384: 6 220-6 450 | 6 400 | 6 440;
// 18 432: 5 975-6 300 | 4 845 | 4 820; 24 576: 6 050 | 5 690 | 5 740; 32 768: 6 340 | 6 530 | 6 600; 49 152: 6 220 | 6 110 | 6 200;
// 65 536: 6 100 | 5 970 | 6 060.  So: those two sizes stay on context 0, everything else alternates.
// The rule is the geometry, not the two bench shapes: the fused projections launch two workgroups per 128 token
// rows; a batch is "exact rounds" when it fills at least one round and the last round of those workgroups is full or within
// 1/32 of full (16 384 - 100 and 32 768 - 500 tokens still are; 14 336 and 18 432 - 7/8 and 9/8 of a round - are not, and
// measured faster on two contexts above; fewer workgroups than CUs never are: 16 384 - 500 tokens, 250 workgroups, alternate).
constexpr bool exact_rounds(uint32_t M, uint32_t n_cu) {
    const uint32_t wgs = (M + 127u) / 128u * 2u, last = wgs % n_cu;
    return wgs >= n_cu && (last == 0u || last * 32u >= n_cu * 31u);
}

}  // namespace cqs
