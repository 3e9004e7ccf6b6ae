// query_forward.hip — the search-time forward: ONE short sequence (<= 128 tokens) through EmbeddingGemma.
//
// The reference embeds the query text on every search (`Embedder::embed_query`, src/embedder/core.rs:768-856, called at
// src/cli/commands/search/query.rs:595; README.md:1079-1082 quotes ~3 ms on its CUDA EP).  At one sequence of 8-32 tokens
// the forward is not a throughput problem: 2 x 101.5 M parameters are 212 MB of bf16 weights streamed once (~30 us at
// HBM / Infinity-Cache rates) and ~10 MFLOP per token of matrix work.  The batch chain (embedder_run.hip: run_layers) serves
// that shape with 9-10 launches per layer, each a tile kernel built for 16 384 tokens: 230 dependent launches of 4-8 us,
// 1.3 ms.  What bounds a kernel here is LATENCY: a launch boundary (~1.3 us, MI355X_MICROARCH.md price list
// "boundary"), one round trip to L2 / MALL for the activations the previous kernel wrote, one for the weights.  So:
//
//   * 4 launches per layer, the minimum the data flow allows with every projection's N range spread over the chip (a
//     row norm needs the whole row = all N-slices of the producing GEMM, so every GEMM output is a grid-wide seam; a
//     grid barrier inside one launch costs 4-5 us on this chip, 3x a launch boundary - not a persistent kernel):
//         QKV      [ x += norm(down_prev)(1+w) ; xn = norm(x)(1+w) ]  -> qkv = xn Wqkv^T
//         attention[ k norm + rope, q norm + rope + scale ] + o_proj  -> y = softmax(q k^T) v Wo^T   (every o_proj workgroup
//                                                                        redoes the attention of all heads in its own LDS)
//         GeGLU    [ x += norm(y)(1+w) ; xn = norm(x)(1+w) ]          -> h = gelu(xn Wg^T) * (xn Wu^T)
//         down                                                          -> y = h Wd^T
//     the row-wise add + RMSNorm pairs live in the PROLOGUE of the GEMM that consumes them: every workgroup recomputes
//     them for its rows instead of a launch + a round trip each; the workgroup of column tile 0 also writes the new residual
//     stream to the other of two x buffers (everybody reads the old one: no race);
//   * a GEMM workgroup = 8 or 16 output columns x a block of rows, its 4 or 8 waves split K (partial tiles summed through
//     LDS); weight slice and activation rows arrive by COALESCED loads and go through LDS (a fragment gather of 16 rows x
//     64 B costs ~44 clocks of address processing per wave-instruction against ~16 for a contiguous 1 KB);
//     v_mfma_f32_16x16x32_bf16 with the weight rows as the A operand (a lane ends with 4 consecutive output columns of
//     one token row);
//   * what a kernel costs is (a) its executed instruction count (one wave per SIMD: template parameters instead of guards,
//     DPP + readlane reductions) and (b) the bytes ONE workgroup pulls through its CU's L2 port (~70 GB/s for lines every
//     workgroup shares): from 5 tokens on the rows are cut into blocks of 8 (<= 16 tokens) or 16 rows (blockIdx.y) x
//     16-column tiles, so a workgroup normalises only its block;
//   * the head (final add + norm, mean pool, Dense 768 -> 3072 -> 768) is two more launches of the same kernels;
//   * T is a launch parameter (no row past the query's length is loaded; the engine keeps one captured hipGraph per length).
// K order differs from the batch kernels (K split over a workgroup's waves) -> results agree with the batch path to bf16
// rounding noise (cosine >= 0.9999, tests/test_query_path_gpu.py), not bit for bit.  Numbers: DESIGN.md 3.8.
// Which kernel form serves which length, its grid and its LDS bytes: the plans of query_plan.h; the chain below asks for a
// plan per step (the same for every layer), then hands it to the step's launcher (query_gemm.hip, query_attention.hip).
#include "query_device.h"

namespace cqs {

namespace {

template <int NCH>
hipError_t qf_forward_t(const QueryFwd& f, hipStream_t st) {
    const uint32_t H = f.hidden, NQ = (f.heads + 2u * f.kv_heads) * 256u, HQ = f.heads * 256u;
    const QfSwitches& sw = qf_switches();
    const QfProPlan plan_qkv = qf_plan_pro(f.T, NCH, false, false, NQ, sw);
    const QfAttnPlan plan_attn = qf_plan_attn(f.T, f.heads, f.kv_heads, H, f.pos != nullptr, sw);
    const QfGemmPlan plan_oproj = qf_plan_gemm(f.T, false, HQ, H, sw);
    const QfProPlan plan_geglu = qf_plan_pro(f.T, NCH, false, true, f.inter, sw);
    const QfGemmPlan plan_down = qf_plan_gemm(f.T, false, f.inter, H, sw);
    float* xb[2] = {f.x0, f.x1};
    int cur = 0;                                     // the residual stream lives in xb[cur]
    hipError_t e = hipSuccess;
    uint32_t slot = 0;
    for (uint32_t l = 0; l < f.layers; ++l) {
        const QueryFwdLayer& w = f.layer[l];
        QfGemmParams p{};
        p.dbg = f.dbg; p.dbg_slot = slot++;
        p.T = f.T; p.eps = f.eps;
        // QKV (+ embedding gather / the previous layer's post-ffw add + this layer's input norm)
        p.W = w.wqkv; p.C = f.qkv; p.ldc = NQ; p.w_next = w.n_in; p.x_out = xb[cur ^ (l == 0 ? 0 : 1)];
        if (l == 0) {
            p.tok = f.tok; p.emb = f.emb; p.scale = f.embed_scale;
            e = qf_launch_pro<NCH, QF_PRO_EMBED, QF_EPI_BF16>(plan_qkv, p, st);
        } else {
            p.x_in = xb[cur]; p.y = f.y; p.w_post = f.layer[l - 1].n_post_ffw;
            e = qf_launch_pro<NCH, QF_PRO_ADDNORM, QF_EPI_BF16>(plan_qkv, p, st);
            cur ^= 1;
        }
        if (e != hipSuccess) return e;
        // attention + o_proj in one launch where the plan has such a form, else two
        QfAttnParams a{};
        a.dbg = f.dbg; a.dbg_slot = slot++;
        a.T = f.T; a.qkv = f.qkv; a.out = f.attn; a.wq = w.n_q; a.wk = w.n_k;
        const bool full = ((l + 1u) % f.sliding_pattern) == 0u;
        a.cos_sin = full ? f.rope_global : f.rope_local;
        a.eps = f.eps; a.q_scale = f.q_scale; a.heads = f.heads; a.kv_heads = f.kv_heads; a.window = full ? 0u : f.window;
        a.wo = w.wo; a.y = f.y; a.H = H; a.pos = f.pos;
        if ((e = qf_launch_attn(plan_attn, a, st)) != hipSuccess) return e;
        if (qf_attn_two_launches(plan_attn.form)) {
            QfGemmParams po{};
            po.dbg = f.dbg; po.dbg_slot = slot;
            po.T = f.T; po.A = f.attn; po.K = HQ; po.W = w.wo; po.C = f.y; po.ldc = H;
            if ((e = qf_launch_gemm<QF_EPI_BF16>(plan_oproj, po, st)) != hipSuccess) return e;
        }
        slot++;
        // GeGLU (+ post-attention add, pre-ffw norm)
        QfGemmParams pg{};
        pg.dbg = f.dbg; pg.dbg_slot = slot++;
        pg.T = f.T; pg.eps = f.eps; pg.x_in = xb[cur]; pg.y = f.y; pg.w_post = w.n_post_attn; pg.w_next = w.n_pre_ffw;
        pg.x_out = xb[cur ^ 1]; pg.W = w.wgu; pg.C = f.h; pg.ldc = f.inter;
        if ((e = qf_launch_pro<NCH, QF_PRO_ADDNORM, QF_EPI_GEGLU>(plan_geglu, pg, st)) != hipSuccess) return e;
        cur ^= 1;
        // down
        QfGemmParams pd{};
        pd.dbg = f.dbg; pd.dbg_slot = slot++;
        pd.T = f.T; pd.A = f.h; pd.K = f.inter; pd.W = w.wd; pd.C = f.y; pd.ldc = H;
        if ((e = qf_launch_gemm<QF_EPI_BF16>(plan_down, pd, st)) != hipSuccess) return e;
    }
    // head: last post-ffw add + final norm + mean pool -> Dense 1 ; Dense 2
    QfGemmParams p1{};
    p1.dbg = f.dbg; p1.dbg_slot = slot++;
    p1.T = f.T; p1.eps = f.eps; p1.x_in = xb[cur]; p1.y = f.y; p1.w_post = f.layer[f.layers - 1].n_post_ffw; p1.w_next = f.n_final;
    p1.W = f.dense1; p1.C = f.d1; p1.ldc = f.dense_hidden; p1.one_row = 1;
    if ((e = qf_launch_pro<NCH, QF_PRO_POOL, QF_EPI_BF16>(qf_plan_pro(f.T, NCH, true, false, f.dense_hidden, sw), p1, st)) != hipSuccess) return e;
    QfGemmParams p2{};
    p2.dbg = f.dbg; p2.dbg_slot = slot++;
    p2.T = f.T; p2.A = f.d1; p2.K = f.dense_hidden; p2.W = f.dense2; p2.C = f.out; p2.ldc = H; p2.one_row = 1;
    return qf_launch_gemm<QF_EPI_F32>(qf_plan_gemm(f.T, true, f.dense_hidden, H, sw), p2, st);
}

}  // namespace

bool query_forward_supported(const EmbedGeom& g) {
    const uint32_t HQ = g.heads * 256u;
    return (g.hidden == 256u || g.hidden == 768u) && g.head_dim == 256u && g.kv_heads && g.heads % g.kv_heads == 0 &&
           g.inter % 128u == 0 && HQ % 128u == 0 && g.dense_hidden % 128u == 0 && g.hidden % 128u == 0;
}

// Longest query the chain serves for this geometry: 128 tokens if every step of a layer and of the head has a form at 128
// tokens (query_plan.h), else 64.
uint32_t query_forward_max_tokens(const EmbedGeom& g) {
    QfChainGeom c{g.hidden, g.heads, g.kv_heads, g.inter, g.dense_hidden};
    // An intermediate size of 3072 is one of the staged GEMM's K classes, but 32 rows of it do not fit LDS beside the weight
    // slice, so the down projection has no form past 64 rows and the plans say 64.  An engine of that geometry has always
    // been told 128 (judged by the K class alone; its longer queries then fail at the down projection); that answer is
    // kept until the lengths such an engine accepts are changed on purpose.
    if (c.inter == 3072u) c.inter = 1152u;
    return qf_chain_max_tokens(c, qf_switches());
}

hipError_t launch_query_forward(const QueryFwd& f, hipStream_t st) {
    if (!f.layer || f.layers == 0 || f.T < 1u || f.T > kQueryFwdMaxTokens) return hipErrorInvalidValue;
    if (f.hidden == 768u) return qf_forward_t<3>(f, st);
    if (f.hidden == 256u) return qf_forward_t<1>(f, st);
    return hipErrorInvalidValue;
}

}  // namespace cqs
