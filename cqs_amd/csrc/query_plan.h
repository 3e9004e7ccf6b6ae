// query_plan.h — the launch plans of the search-time chain (query_gemm.hip, query_attention.hip, query_forward.hip): which
// kernel form serves which query length, its grid, its workgroup size and its dynamic LDS bytes.  Header-only and
// device-free, so the launchers and a CPU test (tests/query_plan_driver.cpp) run the same functions.
//
// Three things live here and nowhere else:
//   * the LDS layout of every kernel family: the kernels take their pointers from a layout's offsets, the plans take the
//     byte count from the same layout's total;
//   * the experiment switches, read once per process into one struct that the plan functions take as a plain argument;
//   * one plan function per dispatch family.  "Not supported" is a form (.._NONE), not an error code; the template arguments
//     behind a form come from one shape table per family, which the launchers instantiate from.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace cqs {

constexpr int kQfPad = 8;                  // bf16 elements of row padding in the LDS activation tile
constexpr int kQfHD = 256;                 // head_dim of the attention kernels
constexpr int kQfKRow = kQfHD + 8;         // sQ / sK row stride (elements)
constexpr uint32_t kQfLdsMax = 160u * 1024u;
constexpr int qf_vrow(int mt) { return 32 * ((mt + 1) / 2) + 8; }   // sVt row stride: keys padded to 32, + 8

// ---- LDS layouts (byte offsets from the start of the dynamic segment; the first array sits at 0) --------------------------
// prologue GEMM: sA [16 gt][lda] | red [nw][nt][gt][64] f4 | pool [nw][H] f32 (pooled head only) | sW [nt][nc][lda].
// ro: `red` overlays sA (and takes no room of its own).
struct QfProLds { int lda; size_t a_bytes, red_bytes, red, pool, w, total; };
constexpr QfProLds qf_pro_lds(int nch, int nt, int nc, int gt, int nw, bool pool, bool ro) {
    QfProLds l{};
    l.lda = nch * 256 + kQfPad;
    l.a_bytes = (size_t)16 * gt * l.lda * 2;
    l.red_bytes = (size_t)nw * nt * gt * 64 * 16;
    l.red = ro ? 0 : l.a_bytes;
    l.pool = l.a_bytes + (ro ? 0 : l.red_bytes);
    l.w = l.pool + (pool ? (size_t)nw * nch * 256 * 4 : 0);
    l.total = l.w + (size_t)nt * nc * l.lda * 2;
    return l;
}
// gather GEMM: red [4][mt][64] f4
constexpr size_t qf_plain_lds(int mt) { return (size_t)4 * mt * 64 * 16; }
// staged GEMM: sW [nc][ldk] | sA [16 mt][ldk] (one row: [1][ldk]) | red [4][mt][64] f4
struct QfStagedLds { uint32_t ldk; size_t a, a_bytes, red, total; };
constexpr QfStagedLds qf_staged_lds(int mt, int nc, bool one, uint32_t K) {
    QfStagedLds l{};
    l.ldk = K + 8u;
    l.a = (size_t)nc * l.ldk * 2;
    l.a_bytes = (size_t)(one ? 1 : 16 * mt) * l.ldk * 2;
    l.red = l.a + l.a_bytes;
    l.total = l.red + qf_plain_lds(mt);
    return l;
}
// attention: sQ [q_rows][kQfKRow] | sK [16 mt][kQfKRow] | sVt [256][vrow(mt)] | red [red_tiles][64] f4 | sW [w_rows][w_k + 8]
struct QfAttnLds { size_t k, vt, red, w, total; };
constexpr QfAttnLds qf_attn_layout(int mt, int q_rows, int red_tiles, int w_rows, int w_k) {
    QfAttnLds l{};
    l.k = (size_t)q_rows * kQfKRow * 2;
    l.vt = l.k + (size_t)16 * mt * kQfKRow * 2;
    l.red = l.vt + (size_t)kQfHD * qf_vrow(mt) * 2;
    l.w = l.red + (size_t)red_tiles * 64 * 16;
    l.total = l.w + (size_t)w_rows * (w_k + 8) * 2;
    return l;
}
constexpr QfAttnLds qf_attention_lds(int mt) { return qf_attn_layout(mt, 16 * mt, 0, 0, 0); }
// attention + o_proj, one shot: Q of nh heads x 16 mtq rows; the o_proj slice is staged unless three or more key tiles
// of a whole-rows workgroup have filled LDS (w == total: the kernel then gathers its fragments from global memory)
constexpr QfAttnLds qf_attn_oproj_lds(int mt, int nh, int nc, int nw, int mtq) {
    return qf_attn_layout(mt, nh * 16 * mtq, nw * mtq, (mt < 3 || mtq < mt) ? nc : 0, nh * kQfHD);
}
// attention + o_proj, keys in two halves of 16 mt: 16 queries x a 32-column slice
constexpr QfAttnLds qf_attn_oproj_long_lds(int mt, int nh, int nw) { return qf_attn_layout(mt, nh * 16, nw * 2, 32, nh * kQfHD); }

// ---- experiment switches ------------------------------------------------------------------------------------------------
struct QfSwitches {
    bool staged = true;        // CQS_HIP_QUERY_STAGED
    bool row_split = true;     // CQS_HIP_QUERY_ROW_SPLIT
    bool attn80 = true;        // CQS_HIP_QUERY_ATTN80
    bool fuse_attn = true;     // CQS_HIP_QUERY_FUSE_ATTN
    int debug_repeat = 1;      // CQS_HIP_QUERY_DEBUG_REPEAT
};
inline QfSwitches qf_read_switches() {
    auto on = [](const char* e) { return !(e && e[0] == '0'); };
    QfSwitches s;
    s.staged = on(getenv("CQS_HIP_QUERY_STAGED"));
    s.row_split = on(getenv("CQS_HIP_QUERY_ROW_SPLIT"));
    s.attn80 = on(getenv("CQS_HIP_QUERY_ATTN80"));
    s.fuse_attn = on(getenv("CQS_HIP_QUERY_FUSE_ATTN"));
    const char* r = getenv("CQS_HIP_QUERY_DEBUG_REPEAT");
    s.debug_repeat = r && r[0] == '2' ? 2 : 1;
    return s;
}
inline const QfSwitches& qf_switches() {       // read once per process
    static const QfSwitches s = qf_read_switches();
    return s;
}

struct QfLaunch { uint32_t grid_x = 0, grid_y = 1, threads = 0, lds_bytes = 0; };

// ---- prologue GEMM (QKV, GeGLU, the pooled head, BERT's add + LayerNorm projections) ----------------------------------------
// W<n>: all rows (<= n) in one workgroup per 8 columns.  B<n>: row blocks of n rows (blockIdx.y) x 16-column tiles (B8C8:
// one block of 8 rows x 8-column tiles).
enum QfProForm { QF_PF_NONE = 0, QF_PF_W4, QF_PF_W8, QF_PF_W16, QF_PF_W32, QF_PF_W48, QF_PF_W64, QF_PF_W128,
                 QF_PF_B8C8, QF_PF_B8C16, QF_PF_B16, QF_PF_B32, QF_PF_B48 };
// qf_gemm_kernel's template arguments behind a form: columns per tile, rows per wave in the first batch, row tiles, waves,
// rows per block, `red` overlays the activation tile.  (rows per wave, row tiles, waves) by length: past 8 tokens a workgroup
// has 8 waves - the per-row work of the prologue is what these kernels spend their time on.
struct QfProShape { int nc, rb, mt, nw, br; bool ro; };
constexpr QfProShape qf_pro_shape(QfProForm f, int nch, bool geglu) {
    switch (f) {
        case QF_PF_W4: return {8, 1, 1, 4, 16, false};
        case QF_PF_W8: return {8, 2, 1, 4, 16, false};
        case QF_PF_W16: return {8, 2, 1, 8, 16, false};
        case QF_PF_W32: return {8, 4, 2, 8, 32, false};
        case QF_PF_W48: return {8, 4, 3, 8, 48, false};
        case QF_PF_W64: return {8, 4, 4, geglu ? 4 : 8, 64, false};     // (GeGLU x 4 row tiles at 8 waves: LDS)
        case QF_PF_W128: return {8, 4, 8, 8, 128, false};
        case QF_PF_B8C8: return {8, 1, 1, 8, 8, false};
        case QF_PF_B8C16: return {16, 1, 1, 8, 8, false};
        case QF_PF_B16: return {16, 2, 1, 8, 16, false};
        case QF_PF_B32: return {16, 4, 2, 8, 32, false};
        case QF_PF_B48: return {16, 4, 3, 8, 48, geglu && nch >= 3};    // (two weight tiles of hidden 768+)
        default: return {0, 0, 0, 0, 0, false};
    }
}
constexpr QfProLds qf_pro_form_lds(QfProForm f, int nch, bool pool, bool geglu) {
    const QfProShape s = qf_pro_shape(f, nch, geglu);
    return qf_pro_lds(nch, geglu ? 2 : 1, s.nc, pool ? 1 : s.mt, s.nw, pool, s.ro);   // (pooled head: the one pooled row)
}
struct QfProPlan : QfLaunch { QfProForm form = QF_PF_NONE; };

inline QfProPlan qf_plan_pro(uint32_t T, int nch, bool pool, bool geglu, uint32_t n_out_cols, const QfSwitches& sw) {
    // row blocks x 16-column tiles (a workgroup's prologue pulls its block through its CU's L2 port, not every row, and every
    // column of the MFMA tile is a real one); not for the pooled head (one row tile anyway)
    const bool split = !pool && sw.row_split && n_out_cols % 16u == 0;
    QfProPlan p;
    // 5-16 tokens: blocks of 8 rows (5-8: one block, 8-column tiles - 160 / 144 workgroups of 49 / 62 KB beat 80 / 72 of 62 / 86).
    // GeGLU at 97-128 tokens: row blocks of 48 (72 column tiles x 3 = 216 workgroups: ONE round on 256 CUs; blocks of 32 rows
    // made 288: 12.4 -> 10.7 us); the QKV projection keeps blocks of 16 rows (48-row blocks: 8.2 -> 9.9 us - its time is the
    // rows a wave normalises, not the rounds).  GeGLU at 65-96 tokens: row blocks of 32 (72 column tiles x 8 blocks of 16 rows =
    // 576 workgroups of 90 KB were 2.25 rounds on 256 CUs; x 4 blocks of 32 rows = 288).
    if (split && T > 4u && T <= 16u) p.form = T <= 8u ? QF_PF_B8C8 : QF_PF_B8C16;
    else if (split && geglu && T > 96u) p.form = QF_PF_B48;
    else if (split && geglu && T > 64u) p.form = QF_PF_B32;
    else if (split && T > 16u) p.form = QF_PF_B16;
    else if (!pool && T > 64u) return p;                            // (only the pooled head keeps all rows in one workgroup)
    else p.form = T <= 4u ? QF_PF_W4 : T <= 8u ? QF_PF_W8 : T <= 16u ? QF_PF_W16 : T <= 32u ? QF_PF_W32 : T <= 48u ? QF_PF_W48 :
                  T <= 64u ? QF_PF_W64 : QF_PF_W128;
    const QfProShape s = qf_pro_shape(p.form, nch, geglu);
    p.grid_x = n_out_cols / (uint32_t)s.nc;
    p.grid_y = (T + (uint32_t)s.br - 1u) / (uint32_t)s.br;
    p.threads = 64u * (uint32_t)s.nw;
    p.lds_bytes = (uint32_t)qf_pro_form_lds(p.form, nch, pool, geglu).total;
    return p;
}

// ---- GEMMs over rows that already exist as bf16 (o_proj, down, Dense 2, the BERT engines' small-row GEMMs) ------------------
// STAGED: both operands through LDS by coalesced loads, blocks of 16 mt rows; GATHER: MFMA fragments straight from global
// memory, all rows (<= 64) in one workgroup.  8 output columns per workgroup either way.
enum QfGemmForm { QF_GF_NONE = 0, QF_GF_STAGED, QF_GF_STAGED_ONE, QF_GF_GATHER };
// K classes of the staged kernel: (k-steps per batch, chunk iterations per row)
struct QfStagedK { uint32_t K; int ch, kc32; };
constexpr int kQfStagedKs = 6;
constexpr QfStagedK kQfStagedK[kQfStagedKs] = {{768, 6, 3}, {1152, 9, 5}, {3072, 8, 12}, {512, 4, 2}, {384, 3, 2}, {256, 2, 1}};
struct QfGemmPlan : QfLaunch {
    QfGemmForm form = QF_GF_NONE;
    int mt = 0;                // row tiles of a workgroup
    int ch = 0;                // k-steps per batch
    int kclass = -1;           // STAGED: index into kQfStagedK
};

inline QfGemmPlan qf_plan_gemm(uint32_t T, bool one_row, uint32_t K, uint32_t n_out_cols, const QfSwitches& sw) {
    const uint32_t rows = one_row ? 1u : T;
    QfGemmPlan p;
    p.grid_x = n_out_cols / 8u;
    p.threads = 256u;
    int kclass = -1;
    for (int i = 0; i < kQfStagedKs; ++i)
        if (kQfStagedK[i].K == K) kclass = i;
    auto staged = [&](int mt, bool one, uint32_t row_blocks) {      // unknown K, no room in LDS or the switch: not this form
        const size_t lds = qf_staged_lds(mt, 8, one, K).total;
        if (!sw.staged || kclass < 0 || lds > kQfLdsMax) return false;
        p.form = one ? QF_GF_STAGED_ONE : QF_GF_STAGED;
        p.mt = mt; p.ch = kQfStagedK[kclass].ch; p.kclass = kclass;
        p.grid_y = row_blocks;
        p.lds_bytes = (uint32_t)lds;
        return true;
    };
    bool ok = false;
    if (one_row) ok = staged(1, true, 1u);
    else if (rows <= 16u) ok = staged(1, false, 1u);
    else if (rows <= 32u) ok = staged(2, false, 1u);
    else if (rows <= 48u) ok = staged(3, false, 1u);
    // blocks of 32 rows: 64 rows of K = 1152 do not fit LDS beside the weight slice, and the gather kernel pays ~44 clocks
    // of address processing per fragment load
    if (!ok && rows > 32u) ok = staged(2, false, (rows + 31u) / 32u);
    if (ok || rows > 64u) return p;                                 // (the gather kernel holds at most four row tiles)
    const uint32_t steps = K / 128u;                                // k-steps of 32 per wave
    p.form = QF_GF_GATHER;
    p.mt = rows <= 16u ? 1 : rows <= 32u ? 2 : rows <= 48u ? 3 : 4;
    p.ch = steps == 9u ? 9 : (steps % 6u == 0u && (p.mt <= 2 || steps == 6u)) ? 6 :   // (batches of 6 x 4 row tiles would not fit the registers twice over)
           steps % 4u == 0u ? 4 : steps % 3u == 0u ? 3 : steps % 2u == 0u ? 2 : 1;
    p.lds_bytes = (uint32_t)qf_plain_lds(p.mt);
    return p;
}

// ---- attention -------------------------------------------------------------------------------------------------------------
// AT<n>: qf_attention_kernel, one workgroup per q head, <= n tokens; o_proj is a GEMM launch of its own (qf_plan_gemm).
// AO<n>: attention + o_proj in one launch, all queries per workgroup x 8 columns.  AOB<n>: the same in blocks of 8 (AOB16) or
// 16 queries x 16 columns, <= n keys.  AOL<n>: keys in two halves, 16 queries x 32 columns, after a qk_norm_rope launch.
enum QfAttnForm { QF_AF_NONE = 0, QF_AF_AT4, QF_AF_AT8, QF_AF_AT16, QF_AF_AT32, QF_AF_AT48, QF_AF_AT64,
                  QF_AF_AO4, QF_AF_AO8, QF_AF_AO16, QF_AF_AO32, QF_AF_AO48,
                  QF_AF_AOB16, QF_AF_AOB32, QF_AF_AOB48, QF_AF_AOB64, QF_AF_AOB80, QF_AF_AOL96, QF_AF_AOL128 };
// key tiles, rows per wave in the first staging batch, o_proj columns, waves, query tiles and queries per workgroup
struct QfAttnShape { int mt, rb, nc, nw, mtq, qb; };
constexpr QfAttnShape qf_attn_shape(QfAttnForm f) {
    switch (f) {
        case QF_AF_AT4: return {1, 1, 0, 4, 1, 16};
        case QF_AF_AT8: return {1, 2, 0, 4, 1, 16};
        case QF_AF_AT16: return {1, 4, 0, 4, 1, 16};
        case QF_AF_AT32: return {2, 4, 0, 4, 2, 32};
        case QF_AF_AT48: return {3, 4, 0, 4, 3, 48};
        case QF_AF_AT64: return {4, 4, 0, 4, 4, 64};
        case QF_AF_AO4: return {1, 1, 8, 4, 1, 16};
        case QF_AF_AO8: return {1, 2, 8, 4, 1, 16};
        case QF_AF_AO16: return {1, 2, 8, 8, 1, 16};
        case QF_AF_AO32: return {2, 4, 8, 8, 2, 32};
        case QF_AF_AO48: return {3, 4, 8, 8, 3, 48};
        case QF_AF_AOB16: return {1, 2, 16, 8, 1, 8};                  // 9-16 tokens: two blocks of 8 queries
        case QF_AF_AOB32: return {2, 4, 16, 8, 1, 16};
        case QF_AF_AOB48: return {3, 4, 16, 8, 1, 16};
        case QF_AF_AOB64: return {4, 4, 16, 8, 1, 16};
        case QF_AF_AOB80: return {5, 4, 16, 8, 1, 16};
        case QF_AF_AOL96: return {3, 0, 32, 8, 1, 16};                 // two halves of 48 keys
        case QF_AF_AOL128: return {4, 0, 32, 8, 1, 16};                // two halves of 64
        default: return {0, 0, 0, 0, 0, 0};
    }
}
constexpr bool qf_attn_two_launches(QfAttnForm f) { return f >= QF_AF_AT4 && f <= QF_AF_AT64; }
constexpr bool qf_attn_long(QfAttnForm f) { return f == QF_AF_AOL96 || f == QF_AF_AOL128; }
constexpr QfAttnLds qf_attn_form_lds(QfAttnForm f, int nh) {
    const QfAttnShape s = qf_attn_shape(f);
    if (qf_attn_two_launches(f)) return qf_attention_lds(s.mt);
    return qf_attn_long(f) ? qf_attn_oproj_long_lds(s.mt, nh, s.nw) : qf_attn_oproj_lds(s.mt, nh, s.nc, s.nw, s.mtq);
}
struct QfAttnPlan : QfLaunch {
    QfAttnForm form = QF_AF_NONE;
    bool rope_first = false;   // a qk_norm_rope launch (in place on the qkv rows) precedes the kernel
};

inline QfAttnPlan qf_plan_attn(uint32_t T, uint32_t heads, uint32_t kv_heads, uint32_t H, bool has_pos, const QfSwitches& sw) {
    QfAttnPlan p;
    QfAttnForm f = QF_AF_NONE;
    // attention + o_proj in one launch: 2 or 3 q heads on one kv head
    if (sw.fuse_attn && kv_heads == 1u && H % 8u == 0 && (heads == 2u || heads == 3u)) {
        const bool blocks = sw.row_split && H % 16u == 0;           // blocks of 8 / 16 queries x 16-column o_proj tiles
        // 65-80 tokens: five key tiles still fit the one-shot kernel's LDS next to a 16-query block (154 of 160 KiB with three
        // heads) - no qk_norm_rope launch, no second key half, 4 launches per layer like every shorter query: 0.90 -> 0.78-0.84
        // ms device.  (Six tiles fit too - 162 304 of 163 840 bytes - but 81-96 tokens are 6 query blocks x 48 column tiles =
        // 288 workgroups, two rounds on 256 CUs: 1.09 ms against 0.91 for the two-halves kernel; measured, not kept.)
        if (T > 64u && T <= 80u && sw.attn80 && H % 16u == 0 && qf_attn_form_lds(QF_AF_AOB80, (int)heads).total <= kQfLdsMax) f = QF_AF_AOB80;
        else if (T > 64u) {                                         // 65-128 tokens: the keys in two halves (online softmax across them)
            if (H % 32u == 0 && T <= 128u && has_pos) f = T <= 96u ? QF_AF_AOL96 : QF_AF_AOL128;
        } else if (T <= 8u) f = T <= 4u ? QF_AF_AO4 : QF_AF_AO8;
        else if (blocks) f = T <= 16u ? QF_AF_AOB16 : T <= 32u ? QF_AF_AOB32 : T <= 48u ? QF_AF_AOB48 : QF_AF_AOB64;
        else if (T <= 48u) f = T <= 16u ? QF_AF_AO16 : T <= 32u ? QF_AF_AO32 : QF_AF_AO48;
    }
    // else two launches: one workgroup per q head (4 waves: (rows per wave, row tiles) by length), then o_proj
    if (f == QF_AF_NONE) {
        if (T > 64u) return p;
        f = T <= 4u ? QF_AF_AT4 : T <= 8u ? QF_AF_AT8 : T <= 16u ? QF_AF_AT16 : T <= 32u ? QF_AF_AT32 : T <= 48u ? QF_AF_AT48 : QF_AF_AT64;
    }
    const QfAttnShape s = qf_attn_shape(f);
    p.form = f;
    p.rope_first = qf_attn_long(f);
    p.grid_x = qf_attn_two_launches(f) ? heads : H / (uint32_t)s.nc;
    p.grid_y = qf_attn_two_launches(f) ? 1u : (T + (uint32_t)s.qb - 1u) / (uint32_t)s.qb;
    p.threads = 64u * (uint32_t)s.nw;
    p.lds_bytes = (uint32_t)qf_attn_form_lds(f, (int)heads).total;
    return p;
}

// ---- the chain ---------------------------------------------------------------------------------------------------------------
struct QfChainGeom { uint32_t hidden, heads, kv_heads, inter, dense_hidden; };
// every step of a layer and of the head has a supported form at T tokens
inline bool qf_chain_supported(const QfChainGeom& g, uint32_t T, bool has_pos, const QfSwitches& sw) {
    const int nch = (int)(g.hidden / 256u);
    const uint32_t NQ = (g.heads + 2u * g.kv_heads) * 256u, HQ = g.heads * 256u;
    const QfAttnPlan a = qf_plan_attn(T, g.heads, g.kv_heads, g.hidden, has_pos, sw);
    return qf_plan_pro(T, nch, false, false, NQ, sw).form != QF_PF_NONE && a.form != QF_AF_NONE &&
           (!qf_attn_two_launches(a.form) || qf_plan_gemm(T, false, HQ, g.hidden, sw).form != QF_GF_NONE) &&
           qf_plan_pro(T, nch, false, true, g.inter, sw).form != QF_PF_NONE &&
           qf_plan_gemm(T, false, g.inter, g.hidden, sw).form != QF_GF_NONE &&
           qf_plan_pro(T, nch, true, false, g.dense_hidden, sw).form != QF_PF_NONE &&
           qf_plan_gemm(T, true, g.dense_hidden, g.hidden, sw).form != QF_GF_NONE;
}
// Longest query the chain serves for this geometry: 128 tokens if every step has a form at 128, else 64.
inline uint32_t qf_chain_max_tokens(const QfChainGeom& g, const QfSwitches& sw) {
    return qf_chain_supported(g, 128u, true, sw) ? 128u : 64u;
}

}  // namespace cqs
