// Stand-alone driver of cqs_amd/csrc/query_plan.h (no HIP, no GPU): sweeps the three plan functions of the search-time
// chain and checks every plan against the kernels' own LDS layouts and tiling rules; prints the lengths at which a form
// changes and the form of every step for the two test geometries (tests/test_query_plan_cpu.py compares them with
// query_state.BREAKS and tests/golden/query_plan_forms.json).  Built with -fsanitize=address,undefined.
#include <stdio.h>

#include <set>
#include <string>

#include "../cqs_amd/csrc/query_plan.h"

using namespace cqs;

static long g_checks = 0;
#define CHECK(c, ...)                                      \
    do {                                                   \
        ++g_checks;                                        \
        if (!(c)) {                                        \
            printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #c); \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
            exit(1);                                       \
        }                                                  \
    } while (0)

static const uint32_t kKs[8] = {128, 256, 384, 512, 640, 768, 1152, 3072};

static QfSwitches switches(unsigned mask) {                // bit set = switch off
    QfSwitches s;
    s.staged = !(mask & 1u); s.row_split = !(mask & 2u); s.attn80 = !(mask & 4u); s.fuse_attn = !(mask & 8u);
    return s;
}

// what every supported plan obeys: LDS, workgroup size, column tiles cover the output exactly, row blocks cover the rows
// with no empty block, a block fits the form's row tiles
static void check_launch(const QfLaunch& l, uint32_t n_out_cols, uint32_t col_tile, uint32_t rows, uint32_t row_block, uint32_t row_cap,
                         size_t layout_total, uint32_t waves, const char* what, uint32_t T) {
    CHECK(l.lds_bytes <= 160u * 1024u, "%s T=%u lds=%u", what, T, l.lds_bytes);
    CHECK(l.threads == 256u || l.threads == 512u, "%s T=%u threads=%u", what, T, l.threads);
    CHECK(l.threads == 64u * waves, "%s T=%u threads=%u waves=%u", what, T, l.threads, waves);
    CHECK(l.grid_x * col_tile == n_out_cols, "%s T=%u grid_x=%u tile=%u cols=%u", what, T, l.grid_x, col_tile, n_out_cols);
    CHECK(l.grid_y >= 1u && l.grid_y * row_block >= rows && (l.grid_y - 1u) * row_block < rows, "%s T=%u grid_y=%u block=%u rows=%u", what, T,
          l.grid_y, row_block, rows);
    CHECK(row_cap >= (rows < row_block ? rows : row_block), "%s T=%u cap=%u block=%u", what, T, row_cap, row_block);
    CHECK(l.lds_bytes == layout_total, "%s T=%u lds=%u layout=%zu", what, T, l.lds_bytes, layout_total);
}

static void check_pro(const QfProPlan& p, uint32_t T, int nch, bool pool, bool geglu, uint32_t n) {
    if (p.form == QF_PF_NONE) return;
    const QfProShape s = qf_pro_shape(p.form, nch, geglu);
    const size_t total = qf_pro_lds(nch, geglu ? 2 : 1, s.nc, pool ? 1 : s.mt, s.nw, pool, s.ro).total;
    check_launch(p, n, (uint32_t)s.nc, T, (uint32_t)s.br, 16u * (uint32_t)s.mt, total, (uint32_t)s.nw, pool ? "pool" : geglu ? "geglu" : "qkv", T);
    const QfProLds l = qf_pro_lds(nch, geglu ? 2 : 1, s.nc, pool ? 1 : s.mt, s.nw, pool, s.ro);
    CHECK(!s.ro || l.red_bytes <= l.a_bytes, "overlay T=%u", T);
}

static void check_gemm(const QfGemmPlan& p, uint32_t T, bool one_row, uint32_t K, uint32_t n) {
    if (p.form == QF_GF_NONE) return;
    const uint32_t rows = one_row ? 1u : T;
    const bool staged = p.form != QF_GF_GATHER;
    CHECK((p.form == QF_GF_STAGED_ONE) == (staged && one_row), "one-row form T=%u", T);
    CHECK(p.ch > 0 && (K / 128u) % (uint32_t)p.ch == 0, "k-steps per batch K=%u ch=%d", K, p.ch);
    if (staged) CHECK(p.kclass >= 0 && p.kclass < kQfStagedKs && kQfStagedK[p.kclass].K == K && kQfStagedK[p.kclass].ch == p.ch, "K class K=%u", K);
    const size_t total = staged ? qf_staged_lds(p.mt, 8, one_row, K).total : qf_plain_lds(p.mt);
    check_launch(p, n, 8u, rows, 16u * (uint32_t)p.mt, 16u * (uint32_t)p.mt, total, 4u, staged ? "staged" : "gather", T);
    if (!staged) CHECK(p.grid_y == 1u && p.mt <= 4, "gather T=%u", T);
}

static void check_attn(const QfAttnPlan& p, uint32_t T, uint32_t heads, uint32_t H) {
    if (p.form == QF_AF_NONE) return;
    const QfAttnShape s = qf_attn_shape(p.form);
    const bool two = qf_attn_two_launches(p.form), lng = qf_attn_long(p.form);
    const size_t total = two ? qf_attention_lds(s.mt).total : lng ? qf_attn_oproj_long_lds(s.mt, (int)heads, s.nw).total :
                                                                    qf_attn_oproj_lds(s.mt, (int)heads, s.nc, s.nw, s.mtq).total;
    if (two) check_launch(p, heads, 1u, T, (uint32_t)s.qb, 16u * (uint32_t)s.mtq, total, (uint32_t)s.nw, "attention", T);
    else check_launch(p, H, (uint32_t)s.nc, T, (uint32_t)s.qb, 16u * (uint32_t)s.mtq, total, (uint32_t)s.nw, "attn+oproj", T);
    CHECK(16u * (uint32_t)s.mt * (lng ? 2u : 1u) >= T, "key tiles T=%u mt=%d", T, s.mt);
    CHECK(p.rope_first == lng, "rope T=%u", T);
}

// ---- the chain's steps as (name of the instantiation, launch) -----------------------------------------------------------------
struct Step { std::string name; QfLaunch l; bool ok; };
static std::string pro_name(const QfProPlan& p, int nch, int pro, bool geglu) {
    const QfProShape s = qf_pro_shape(p.form, nch, geglu);
    char b[128];
    snprintf(b, sizeof b, "qf_gemm_kernel<%d,%d,%d,%d,%d,%d,%d,%d,%s>", nch, pro, geglu ? 1 : 0, s.nc, s.rb, s.mt, s.nw, s.br, s.ro ? "true" : "false");
    return b;
}
static std::string gemm_name(const QfGemmPlan& p, int epi) {
    char b[128];
    if (p.form == QF_GF_GATHER) snprintf(b, sizeof b, "qf_gemm_plain_kernel<%d,%d,%d,8>", p.mt, p.ch, epi);
    else snprintf(b, sizeof b, "qf_gemm_staged_kernel<%d,%d,%d,%d,8,%d>", p.mt, p.ch, p.kclass >= 0 ? kQfStagedK[p.kclass].kc32 : 0, epi, p.form == QF_GF_STAGED_ONE ? 1 : 0);
    return b;
}
static std::string attn_name(const QfAttnPlan& p, uint32_t heads) {
    const QfAttnShape s = qf_attn_shape(p.form);
    char b[128];
    if (qf_attn_two_launches(p.form)) snprintf(b, sizeof b, "qf_attention_kernel<%d,%d>", s.mt, s.rb);
    else if (qf_attn_long(p.form)) snprintf(b, sizeof b, "qf_attn_oproj_long_kernel<%d,%u,%d>", s.mt, heads, s.nw);
    else snprintf(b, sizeof b, "qf_attn_oproj_kernel<%d,%d,%u,%d,%d,%d,%d>", s.mt, s.rb, heads, s.nc, s.nw, s.mtq, s.qb);
    return b;
}

struct Chain { QfProPlan qkv, geglu, pool; QfAttnPlan attn; QfGemmPlan oproj, down, dense2; };
static Chain plan_chain(const QfChainGeom& g, uint32_t T, const QfSwitches& sw) {
    const int nch = (int)(g.hidden / 256u);
    Chain c;
    c.qkv = qf_plan_pro(T, nch, false, false, (g.heads + 2u * g.kv_heads) * 256u, sw);
    c.attn = qf_plan_attn(T, g.heads, g.kv_heads, g.hidden, true, sw);
    c.oproj = qf_plan_gemm(T, false, g.heads * 256u, g.hidden, sw);
    c.geglu = qf_plan_pro(T, nch, false, true, g.inter, sw);
    c.down = qf_plan_gemm(T, false, g.inter, g.hidden, sw);
    c.pool = qf_plan_pro(T, nch, true, false, g.dense_hidden, sw);
    c.dense2 = qf_plan_gemm(T, true, g.dense_hidden, g.hidden, sw);
    return c;
}
static bool chain_ok(const Chain& c) {
    return c.qkv.form != QF_PF_NONE && c.attn.form != QF_AF_NONE && (!qf_attn_two_launches(c.attn.form) || c.oproj.form != QF_GF_NONE) &&
           c.geglu.form != QF_PF_NONE && c.down.form != QF_GF_NONE && c.pool.form != QF_PF_NONE && c.dense2.form != QF_GF_NONE;
}
// the forms of a chain as one comparable key (the template instantiations, not the grids)
static std::string chain_key(const Chain& c, const QfChainGeom& g) {
    const int nch = (int)(g.hidden / 256u);
    return pro_name(c.qkv, nch, 2, false) + attn_name(c.attn, g.heads) + (qf_attn_two_launches(c.attn.form) ? gemm_name(c.oproj, 0) : "") +
           pro_name(c.geglu, nch, 2, true) + gemm_name(c.down, 0) + pro_name(c.pool, nch, 3, false) + gemm_name(c.dense2, 2);
}

static void print_step(const char* geom, const char* cfg, uint32_t T, const char* step, const std::string& name, const QfLaunch& l) {
    printf("g|%s/%s/%u|%s|%s|%u|%u|%u\n", geom, cfg, T, step, name.c_str(), l.grid_x, l.grid_y, l.threads);
}

int main() {
    // ---- 1. every plan of every geometry, length and switch subset ----
    for (uint32_t hidden : {256u, 768u})
        for (uint32_t heads = 1; heads <= 4; ++heads)
            for (uint32_t kv = 1; kv <= 2; ++kv) {
                if (heads % kv) continue;
                for (unsigned mask = 0; mask < 16u; ++mask) {
                    const QfSwitches sw = switches(mask);
                    const int nch = (int)(hidden / 256u);
                    for (uint32_t T = 1; T <= 128u; ++T) {
                        check_pro(qf_plan_pro(T, nch, false, false, (heads + 2u * kv) * 256u, sw), T, nch, false, false, (heads + 2u * kv) * 256u);
                        check_attn(qf_plan_attn(T, heads, kv, hidden, true, sw), T, heads, hidden);
                        CHECK(qf_plan_attn(T, heads, kv, hidden, false, sw).rope_first == false, "no positions, no rope launch T=%u", T);
                        for (uint32_t K : kKs) {
                            check_pro(qf_plan_pro(T, nch, false, true, K, sw), T, nch, false, true, K);
                            check_pro(qf_plan_pro(T, nch, true, false, K, sw), T, nch, true, false, K);
                            check_gemm(qf_plan_gemm(T, false, K, hidden, sw), T, false, K, hidden);
                            check_gemm(qf_plan_gemm(T, true, K, hidden, sw), T, true, K, hidden);
                        }
                    }
                    // the chain: every step has a form up to the longest length, and a 64-token geometry lacks one at 65
                    for (uint32_t inter : kKs)
                        for (uint32_t dense : kKs) {
                            const QfChainGeom g{hidden, heads, kv, inter, dense};
                            const uint32_t M = qf_chain_max_tokens(g, sw);
                            CHECK(M == 64u || M == 128u, "max tokens %u", M);
                            for (uint32_t T = 1; T <= M; ++T) {
                                CHECK(qf_chain_supported(g, T, true, sw), "hidden=%u heads=%u kv=%u inter=%u dense=%u mask=%u T=%u", hidden, heads, kv, inter, dense, mask, T);
                                CHECK(chain_ok(plan_chain(g, T, sw)) , "chain T=%u", T);
                            }
                            if (M == 64u) CHECK(!qf_chain_supported(g, 65u, true, sw), "hidden=%u heads=%u kv=%u inter=%u dense=%u mask=%u", hidden, heads, kv, inter, dense, mask);
                        }
                }
            }
    // the BERT engines' add + LayerNorm projections (hidden 1024 too), <= 64 rows.  (Hidden 1024 with CQS_HIP_QUERY_ROW_SPLIT=0
    // is left out: 49-64 rows in one workgroup are 181 376 bytes of LDS, a launch the runtime refuses - as before the plans.)
    for (int nch : {1, 3, 4})
        for (unsigned mask = 0; mask < 16u; ++mask)
            for (uint32_t T = 1; T <= 64u; ++T)
                for (uint32_t n : {768u, 1024u, 3072u, 4096u}) {
                    if (nch == 4 && (mask & 2u)) continue;
                    const QfProPlan p = qf_plan_pro(T, nch, false, false, n, switches(mask));
                    CHECK(p.form != QF_PF_NONE, "addln T=%u", T);
                    check_pro(p, T, nch, false, false, n);
                }
    printf("checks ok %ld\n", g_checks);

    // ---- 2. the lengths at which a form of the full geometry changes, all switches on ----
    const QfChainGeom full{768, 3, 1, 1152, 3072}, small{256, 2, 1, 384, 512};
    {
        std::set<uint32_t> br = {1u, 128u};
        const QfSwitches sw = switches(0);
        for (uint32_t T = 2; T <= 128u; ++T)
            if (chain_key(plan_chain(full, T, sw), full) != chain_key(plan_chain(full, T - 1u, sw), full)) { br.insert(T - 1u); br.insert(T); }
        printf("breaks");
        for (uint32_t b : br) printf(" %u", b);
        printf("\n");
    }

    // ---- 3. the form of every step, both test geometries (3 and 24 layers), all switches on and each one off ----
    const char* cfgs[5] = {"all", "staged0", "split0", "attn80_0", "fuse0"};
    const unsigned masks[5] = {0u, 1u, 2u, 4u, 8u};
    for (int gi = 0; gi < 2; ++gi) {
        const QfChainGeom& g = gi ? full : small;
        const char* gname = gi ? "full" : "small";
        const uint32_t layers = gi ? 24u : 3u;
        const int nch = (int)(g.hidden / 256u);
        for (int ci = 0; ci < 5; ++ci) {
            const QfSwitches sw = switches(masks[ci]);
            const uint32_t M = qf_chain_max_tokens(g, sw);
            for (uint32_t T = 1; T <= 128u; ++T) {
                if (T > M) { printf("g|%s/%s/%u|unsupported\n", gname, cfgs[ci], T); continue; }
                const Chain c = plan_chain(g, T, sw);
                const bool two = qf_attn_two_launches(c.attn.form);
                print_step(gname, cfgs[ci], T, "qkv0", pro_name(c.qkv, nch, 1, false), c.qkv);
                print_step(gname, cfgs[ci], T, "qkv", pro_name(c.qkv, nch, 2, false), c.qkv);
                if (c.attn.rope_first) printf("g|%s/%s/%u|rope\n", gname, cfgs[ci], T);
                print_step(gname, cfgs[ci], T, "attn", attn_name(c.attn, g.heads), c.attn);
                if (two) print_step(gname, cfgs[ci], T, "oproj", gemm_name(c.oproj, 0), c.oproj);
                print_step(gname, cfgs[ci], T, "geglu", pro_name(c.geglu, nch, 2, true), c.geglu);
                print_step(gname, cfgs[ci], T, "down", gemm_name(c.down, 0), c.down);
                print_step(gname, cfgs[ci], T, "pool", pro_name(c.pool, nch, 3, false), c.pool);
                print_step(gname, cfgs[ci], T, "dense2", gemm_name(c.dense2, 2), c.dense2);
                printf("g|%s/%s/%u|launches|%u\n", gname, cfgs[ci], T, layers * (4u + (c.attn.rope_first ? 1u : 0u) + (two ? 1u : 0u)) + 2u);
            }
        }
    }
    printf("all ok\n");
    return 0;
}
