// query_attention.hip — the attention kernels of the search-time chain (query_forward.hip) and their launcher.  Which form
// serves which length: query_plan.h.
#include "query_device.h"

#include <cmath>

namespace cqs {

namespace {

// ---- attention over <= 64 keys ------------------------------------------------------------------------------------------
// Staging (one WAVE per token row; lane owns dims [4 lane, 4 lane + 4), rotate_half partner = lane ^ 32 - the arithmetic
// of qk_norm_rope_block): per row the k head and the NH q heads are RMS-normalised, rotated (q also scaled) and written
// to LDS as bf16 rows, V is written transposed.  S^T = K Q^T with keys on MFMA rows (softmax lane-local + two
// cross-lane steps), O^T = V^T P^T with the S^T accumulators as the B operand (embed_attention.hip's key permutation: lane
// group g holds keys {4g..4g+3} of each 16-key tile, so the 8 slots of a 32-key step are keys {4g.., 16 + 4g..} and V^T
// is read in that order).  Two users: qf_attention_kernel (one workgroup per q head; queries of 49-64 tokens) and
// qf_attn_oproj_kernel (every o_proj workgroup redoes the attention of all heads in its own LDS: one launch and one
// round trip through memory less per layer; the redundant work is ~100 MFMAs per workgroup at 8-16 tokens).

// Stage rows [0, T) of kv head g and q heads [h0, h0 + NH): sQ [NH][16 MTQ][kQfKRow], sK [16 MT][kQfKRow], sVt [256][vrow].
// MTQ < MT: only the query rows [qrow0, qrow0 + 16 MTQ) are staged (a workgroup that owns one row block of the queries
// still needs every key / value row); a row's q heads are then neither loaded nor rotated outside that window.
template <int MT, int RB, int NH, int NW, int MTQ = MT, int QB = 16 * MTQ>
__device__ __forceinline__ void qf_attn_stage(const QfAttnParams& p, uint32_t h0, uint32_t g, bf16_t* sQ, bf16_t* sK, bf16_t* sVt,
                                              int wid, int lane, uint32_t qrow0 = 0u) {
    constexpr int VR = qf_vrow(MT);
    auto inq = [&](uint32_t row) { return (MTQ == MT && QB == 16 * MTQ) || (row >= qrow0 && row < qrow0 + (uint32_t)QB); };   // (wave-uniform)
    const uint32_t T = p.T, last = T - 1u;
    const uint32_t ld = (p.heads + 2u * p.kv_heads) * (uint32_t)kQfHD;
    const bf16_t* qb = p.qkv + (size_t)h0 * kQfHD + lane * 4;
    const bf16_t* kb = p.qkv + (size_t)(p.heads + g) * kQfHD + lane * 4;
    const bf16_t* vb = p.qkv + (size_t)(p.heads + p.kv_heads + g) * kQfHD + lane * 4;
    const float* csb = p.cos_sin + (uint32_t)(lane & 31) * 8u;
    struct Row { bf4 q[NH], k, v; f4 c0, c1; };
    auto load = [&](uint32_t row, Row& r) {
        if (inq(row)) {
#pragma unroll
            for (int h = 0; h < NH; ++h) r.q[h] = *(const bf4*)(qb + (size_t)row * ld + h * kQfHD);
        }
        r.k = *(const bf4*)(kb + (size_t)row * ld);
        r.v = *(const bf4*)(vb + (size_t)row * ld);
        r.c0 = *(const f4*)(csb + (size_t)row * 256u);
        r.c1 = *(const f4*)(csb + (size_t)row * 256u + 4);
    };
    f4 wq1, wk1;
    auto rot = [&](const bf4& in, const f4& w1, const Row& r, float scale) -> bf4 {
        const float c4[4] = {r.c0[0], r.c0[2], r.c1[0], r.c1[2]};
        const float s4[4] = {r.c0[1], r.c0[3], r.c1[1], r.c1[3]};
        float x[4];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { x[i] = (float)in[i]; ss += x[i] * x[i]; }
        const float inv = rsqrtf(wave_sum64_readlane(ss) / (float)kQfHD + p.eps);
        bf4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float n = x[i] * inv * w1[i];
            const float other = xor32_value(n, lane);                    // rotate_half partner: dim +/- 128
            o[i] = (bf16_t)(((lane < 32) ? (n * c4[i] - other * s4[i]) : (n * c4[i] + other * s4[i])) * scale);
        }
        return o;
    };
    auto put = [&](uint32_t row, const Row& r) {
        if (inq(row)) {
#pragma unroll
            for (int h = 0; h < NH; ++h)
                *(bf4*)(sQ + ((size_t)h * 16 * MTQ + (row - qrow0)) * kQfKRow + lane * 4) = rot(r.q[h], wq1, r, p.q_scale);
        }
        *(bf4*)(sK + (size_t)row * kQfKRow + lane * 4) = rot(r.k, wk1, r, 1.0f);
#pragma unroll
        for (int i = 0; i < 4; ++i) sVt[(size_t)(lane * 4 + i) * VR + row] = r.v[i];
    };
    Row rows[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
        const uint32_t r = (uint32_t)wid + (uint32_t)NW * (uint32_t)b;
        load(r < T ? r : last, rows[b]);                              // a slot past T re-does row T - 1
    }
    wq1 = *(const f4*)(p.wq + lane * 4) + 1.0f;
    wk1 = *(const f4*)(p.wk + lane * 4) + 1.0f;
    if (MT == 1) {
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const uint32_t r = (uint32_t)wid + (uint32_t)NW * (uint32_t)b;
            put(r < T ? r : last, rows[b]);
        }
    } else {                                                          // RB = 4: 16 rows per pass of the workgroup
        for (uint32_t r0 = (uint32_t)wid;;) {
#pragma unroll
            for (int b = 0; b < RB; ++b) {
                const uint32_t r = r0 + (uint32_t)NW * (uint32_t)b;
                put(r < T ? r : last, rows[b]);
            }
            r0 += (uint32_t)(NW * RB);
            if (r0 >= T) break;
#pragma unroll
            for (int b = 0; b < RB; ++b) {
                const uint32_t r = r0 + (uint32_t)NW * (uint32_t)b;
                load(r < T ? r : last, rows[b]);
            }
        }
    }
    // V^T columns [T, 32 ceil(MT / 2)) multiply P = 0 in the last 32-key step: zeros (K rows past T may hold anything:
    // their scores are replaced, not multiplied).  Thread = one head dim.
    if (threadIdx.x < (uint32_t)kQfHD) {
        bf16_t* vz = sVt + (size_t)threadIdx.x * VR;
        for (uint32_t key = T; key < 32u * ((MT + 1) / 2); ++key) vz[key] = (bf16_t)0.f;
    }
}

// One (q head, 16-query tile) unit on one wave: o[j][r] = O[query 16 qt + l15][dim 16 (dt0 + j) + 4 lg + r], unnormalised;
// returns 1 / sum.  sQh = the head's Q rows.
template <int MT, int NDT>
__device__ __forceinline__ float qf_attn_unit(const QfAttnParams& p, const bf16_t* sQh, const bf16_t* sK, const bf16_t* sVt,
                                              uint32_t qt, uint32_t dt0, int l15, int lg, f4 (&o)[NDT], uint32_t qrow0 = 0u) {
    constexpr int VR = qf_vrow(MT);
    const uint32_t T = p.T;
    const uint32_t ql = 16u * qt + (uint32_t)l15;              // row of sQh (local to the staged query window)
    const uint32_t q = qrow0 + ql;                             // the query's position
    f4 sc[MT];
#pragma unroll
    for (int kt = 0; kt < MT; ++kt) sc[kt] = (f4)(0.f);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const bf8 qf = *(const bf8*)(sQh + (size_t)ql * kQfKRow + 32 * s + 8 * lg);
#pragma unroll
        for (int kt = 0; kt < MT; ++kt) {
            const bf8 kf = *(const bf8*)(sK + (size_t)(16 * kt + l15) * kQfKRow + 32 * s + 8 * lg);
            sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, sc[kt], 0, 0, 0);
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < MT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t key = (uint32_t)(16 * kt + 4 * lg + r);
            const uint32_t dist = key > q ? key - q : q - key;
            const bool ok = key < T && (p.window == 0u || dist < p.window);
            sc[kt][r] = ok ? sc[kt][r] : -INFINITY;
            mx = fmaxf(mx, sc[kt][r]);
        }
    mx = xor16_max(mx);
    mx = xor32_max(mx);
    float sum = 0.f;
    constexpr int KT2 = 2 * ((MT + 1) / 2);
    bf4 pb[KT2];
#pragma unroll
    for (int kt = 0; kt < KT2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = kt < MT ? __expf(sc[kt < MT ? kt : 0][r] - mx) : 0.f;   // masked: exp(-inf) = 0 (a live query sees itself: mx is finite)
            pb[kt][r] = (bf16_t)e;
            sum += (float)pb[kt][r];                                   // the rounded weights are what multiplies V
        }
    sum = xor16_sum(sum);
    sum = xor32_sum(sum);
#pragma unroll
    for (int j = 0; j < NDT; ++j) o[j] = (f4)(0.f);
#pragma unroll
    for (int kb = 0; kb < (MT + 1) / 2; ++kb) {
        bf8 pf;
#pragma unroll
        for (int r = 0; r < 4; ++r) { pf[r] = pb[2 * kb][r]; pf[4 + r] = pb[2 * kb + 1][r]; }
#pragma unroll
        for (int j = 0; j < NDT; ++j) {
            const bf16_t* vr = sVt + (size_t)(16u * (dt0 + (uint32_t)j) + (uint32_t)l15) * VR + 32 * kb + 4 * lg;
            const bf4 v0 = *(const bf4*)vr, v1 = *(const bf4*)(vr + 16);
            bf8 vf;
#pragma unroll
            for (int r = 0; r < 4; ++r) { vf[r] = v0[r]; vf[4 + r] = v1[r]; }
            o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[j], 0, 0, 0);
        }
    }
    return 1.0f / sum;
}

// Standalone: one workgroup per q head.  Up to 16 queries the 4 waves split the 16 output tiles of the one query tile
// (each recomputes S and the softmax: 8 MFMAs); 17-32 queries: 2 waves per query tile; more: one wave per tile.
template <int MT, int RB>
__global__ __launch_bounds__(256) void qf_attention_kernel(const QfAttnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qf_smem[];
    constexpr QfAttnLds L = qf_attention_lds(MT);
    bf16_t* const sQ = (bf16_t*)qf_smem;
    bf16_t* const sK = (bf16_t*)(qf_smem + L.k);
    bf16_t* const sVt = (bf16_t*)(qf_smem + L.vt);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    QF_STAMP(p, 0);
    const uint32_t h = blockIdx.x, g = h / (p.heads / p.kv_heads);
    qf_attn_stage<MT, RB, 1, 4>(p, h, g, sQ, sK, sVt, wid, lane);
    __syncthreads();
    QF_STAMP(p, 1);
    constexpr int G = MT == 1 ? 4 : (MT == 2 ? 2 : 1);                    // waves per query tile
    constexpr int NDT = 16 / G;
    const uint32_t qt = (uint32_t)wid / G, dgrp = (uint32_t)wid % G;
    if (qt >= (uint32_t)MT) return;
    f4 o[NDT];
    const float rinv = qf_attn_unit<MT, NDT>(p, sQ, sK, sVt, qt, dgrp * (uint32_t)NDT, l15, lg, o);
    QF_STAMP(p, 2);
    const uint32_t q = 16u * qt + (uint32_t)l15;
    if (q >= p.T) return;
    bf16_t* orow = p.out + (size_t)q * (p.heads * (uint32_t)kQfHD) + (size_t)h * kQfHD + 4 * lg + 16u * dgrp * (uint32_t)NDT;
#pragma unroll
    for (int j = 0; j < NDT; ++j) {
        bf4 ob;
#pragma unroll
        for (int r = 0; r < 4; ++r) ob[r] = (bf16_t)(o[j][r] * rinv);
        *(bf4*)(orow + 16 * j) = ob;
    }
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QF_STAMP(p, 3); }
}

// Fused: attention of ALL heads (NH = heads, one kv head) in the workgroup's LDS, then y[:, NC columns] = attn Wo^T.
// The attention output of (head, query tile) overwrites that tile's Q rows (the unit's own wave is their only reader).
// MTQ < MT (17-32 tokens: MT = 2 key tiles, MTQ = 1): blockIdx.y = the workgroup's block of 16 MTQ query rows; it stages
// every key / value row but only its own queries (and their cos / sin rows), runs NH MTQ attention units and multiplies
// 16 MTQ rows of o_proj against an NC = 16 column slice - less to pull through the CU's L2 port, half the units per workgroup.
template <int MT, int RB, int NH, int NC, int NW, int MTQ = MT, int QB = 16 * MTQ>
__global__ __launch_bounds__(64 * NW) void qf_attn_oproj_kernel(const QfAttnParams p) {
    constexpr int K = NH * kQfHD, kw = K / NW, S = kw / 32;          // o_proj's K = heads x 256; this wave's K range and k-steps
    static_assert(K % (32 * NW) == 0, "the waves split K in whole 32-deep steps");
    extern __shared__ __attribute__((aligned(16))) unsigned char qf_smem[];
    constexpr QfAttnLds L = qf_attn_oproj_lds(MT, NH, NC, NW, MTQ);
    bf16_t* const sQ = (bf16_t*)qf_smem;                               // [NH][16 MTQ][kQfKRow]: Q, then O
    bf16_t* const sK = (bf16_t*)(qf_smem + L.k);
    bf16_t* const sVt = (bf16_t*)(qf_smem + L.vt);
    float* const red = (float*)(qf_smem + L.red);                      // [NW waves][MTQ][64 lanes] f4
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    QF_STAMP(p, 0);
    static_assert(QB <= 16 * MTQ, "a query block fits the staged query tiles");
    const uint32_t qrow0 = blockIdx.y * (uint32_t)QB;               // (QB < 16: 9-16 tokens as two blocks of 8 queries)
    // o_proj's weight slice (NC consecutive rows: one contiguous block) first, by coalesced loads (thread = row tid / 32,
    // 16-byte chunks tid % 32 + 32 j); it lands while the attention runs and goes through LDS (sW [NC][K + 8]) - except
    // at 3 row tiles, where LDS is full and the fragments are gathered from global memory as before
    static_assert(NC == 8 || NC == 16, "an 8- or 16-row weight slice per workgroup");
    static_assert(NC <= 2 * NW, "one slice row per 32-thread group");
    constexpr bool kStageW = L.total > L.w;                          // (a block of the queries leaves LDS room at any key count)
    constexpr int LDW = K + 8;
    bf16_t* const sW = (bf16_t*)(qf_smem + L.w);
    const uint32_t wg = (uint32_t)tid >> 5, wl32 = (uint32_t)tid & 31u;
    u4 wreg[NH];
    bf8 wf[S];
    if (kStageW) {
        if (wg < (uint32_t)NC) {
            const bf16_t* src = p.wo + (size_t)(blockIdx.x * (uint32_t)NC + wg) * K + wl32 * 8u;
#pragma unroll
            for (int j = 0; j < NH; ++j) wreg[j] = *(const u4*)(src + 256 * j);
        }
    } else {
        const bf16_t* wp = p.wo + (size_t)(blockIdx.x * (uint32_t)NC + (uint32_t)(l15 % NC)) * K + wid * kw + 8 * lg;
#pragma unroll
        for (int s = 0; s < S; ++s) wf[s] = *(const bf8*)(wp + 32 * s);
    }
    qf_attn_stage<MT, RB, NH, NW, MTQ, QB>(p, 0u, 0u, sQ, sK, sVt, wid, lane, qrow0);
    __syncthreads();
    QF_STAMP(p, 1);
    for (uint32_t u = (uint32_t)wid; u < (uint32_t)(NH * MTQ); u += (uint32_t)NW) {   // (head, query tile) units over the waves
        const uint32_t h = u / (uint32_t)MTQ, qt = u % (uint32_t)MTQ;
        bf16_t* sQh = sQ + (size_t)h * 16 * MTQ * kQfKRow;
        f4 o[16];
        const float rinv = qf_attn_unit<MT, 16>(p, sQh, sK, sVt, qt, 0u, l15, lg, o, qrow0);
        bf16_t* orow = sQh + (size_t)(16u * qt + (uint32_t)l15) * kQfKRow + 4 * lg;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            bf4 ob;
#pragma unroll
            for (int r = 0; r < 4; ++r) ob[r] = (bf16_t)(o[j][r] * rinv);
            *(bf4*)(orow + 16 * j) = ob;
        }
    }
    if (kStageW && wg < (uint32_t)NC) {
#pragma unroll
        for (int j = 0; j < NH; ++j) *(u4*)(sW + (size_t)wg * LDW + wl32 * 8u + 256 * j) = wreg[j];
    }
    __syncthreads();
    QF_STAMP(p, 2);
    if (kStageW) {
#pragma unroll
        for (int s = 0; s < S; ++s) wf[s] = *(const bf8*)(sW + (size_t)(l15 % NC) * LDW + wid * kw + 8 * lg + 32 * s);
    }
    // y tile: B operand (attention rows) from LDS: row 16 m + l15, k = wid kw + 32 s + 8 lg -> head k / 256, dim k % 256
    f4 acc[MTQ];
#pragma unroll
    for (int m = 0; m < MTQ; ++m) acc[m] = (f4)(0.f);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int k = wid * kw + 32 * s;                               // wave-uniform; a 32-wide step never straddles a head
        const bf16_t* src = sQ + (size_t)(k / kQfHD) * 16 * MTQ * kQfKRow + (k % kQfHD) + 8 * lg;
#pragma unroll
        for (int m = 0; m < MTQ; ++m) {
            const bf8 a = *(const bf8*)(src + (size_t)(16 * m + l15) * kQfKRow);
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], a, acc[m], 0, 0, 0);
        }
    }
#pragma unroll
    for (int m = 0; m < MTQ; ++m) *(f4*)(red + ((size_t)(wid * MTQ + m) * 64 + lane) * 4) = acc[m];
    __syncthreads();
    if (wid >= MTQ) return;
    f4 v = *(const f4*)(red + ((size_t)wid * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < NW; ++w) v += *(const f4*)(red + ((size_t)(w * MTQ + wid) * 64 + lane) * 4);
    const uint32_t lrow = 16u * (uint32_t)wid + (uint32_t)l15, row = qrow0 + lrow;
    if (lrow >= (uint32_t)QB || row >= p.T || 4 * lg >= NC) return;
    bf4 ob;
#pragma unroll
    for (int r = 0; r < 4; ++r) ob[r] = (bf16_t)v[r];
    *(bf4*)(p.y + (size_t)row * p.H + blockIdx.x * (uint32_t)NC + 4u * (uint32_t)lg) = ob;
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QF_STAMP(p, 3); }
}

// ---- attention + o_proj for 65-128 tokens: the keys in TWO halves ----------------------------------------------------------
// At > 64 keys the one-shot layout above does not fit LDS (K rows + V^T + Q of three heads + the o_proj slice: 195 KB at 128
// keys), and 48 column tiles x 8 query blocks = 384 workgroups of > 80 KB are two rounds on 256 CUs.  Here:
//   * q and k heads are normalised / rotated ONCE per layer by a launch of their own (qk_norm_rope_kernel, in place on the
//     qkv rows: 128 rows x 4 heads) instead of by every workgroup (each pulled 128 KB of cos / sin rows for that, as much as
//     K and V together); the workgroups below only copy rows;
//   * a workgroup = 16 queries x a 32-column o_proj tile (24 x 8 = 192 workgroups: one round), 8 waves; it stages the keys
//     in two halves of 16 MT rows and runs an online softmax across them (running maximum m, per-lane partial sum l, O
//     rescaled by exp(m_old - m_new) between the halves): LDS = what 16 MT keys need (154 KB at MT = 4);
//   * one (head, query tile) unit per wave (waves 0 .. NH - 1); its O accumulators live in registers across the second staging.
template <int MT, int NH, int NW>
__global__ __launch_bounds__(64 * NW) void qf_attn_oproj_long_kernel(const QfAttnParams p) {
    constexpr int NC = 32;                                            // o_proj columns per workgroup = two 16-row weight tiles
    constexpr int K = NH * kQfHD, kw = K / NW, S = kw / 32;
    constexpr int VR = qf_vrow(MT);
    constexpr int LDW = K + 8;
    static_assert(K % (32 * NW) == 0 && NH <= NW && NC == 4 * NW, "two o_proj weight rows per 32-thread group");
    extern __shared__ __attribute__((aligned(16))) unsigned char qf_smem[];
    bf16_t* const sQ = (bf16_t*)qf_smem;                               // [NH][16][kQfKRow]: Q, then O
    constexpr QfAttnLds L = qf_attn_oproj_long_lds(MT, NH, NW);
    bf16_t* const sK = (bf16_t*)(qf_smem + L.k);                       // [16 MT][kQfKRow]
    bf16_t* const sVt = (bf16_t*)(qf_smem + L.vt);                     // [256][VR]
    float* const red = (float*)(qf_smem + L.red);                      // [NW][2][64] f4
    bf16_t* const sW = (bf16_t*)(qf_smem + L.w);                       // [NC][LDW]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    QF_STAMP(p, 0);
    const uint32_t T = p.T, last = T - 1u;
    const uint32_t qrow0 = blockIdx.y * 16u;
    const uint32_t wg = (uint32_t)tid >> 5, wl32 = (uint32_t)tid & 31u;   // 16 groups of 32 threads: slice rows wg and wg + 16
    u4 wreg[2][NH];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const bf16_t* src = p.wo + (size_t)(blockIdx.x * (uint32_t)NC + wg + 16u * (uint32_t)t) * K + wl32 * 8u;
#pragma unroll
        for (int j = 0; j < NH; ++j) wreg[t][j] = *(const u4*)(src + 256 * j);
    }
    const uint32_t ld = (p.heads + 2u * p.kv_heads) * (uint32_t)kQfHD;
    // ---- Q of the workgroup's 16 queries (already normalised, rotated, scaled): row lr = tid / 32, 16-byte chunks tid % 32 ----
    {
        const uint32_t lr = wg;
        const uint32_t row = qrow0 + lr < T ? qrow0 + lr : last;
        u4 q[NH];
#pragma unroll
        for (int h = 0; h < NH; ++h) q[h] = *(const u4*)(p.qkv + (size_t)row * ld + (size_t)h * kQfHD + wl32 * 8u);
#pragma unroll
        for (int h = 0; h < NH; ++h) *(u4*)(sQ + ((size_t)h * 16 + lr) * kQfKRow + wl32 * 8u) = q[h];
    }
    // ---- the two key halves ----
    f4 o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] = (f4)(0.f);
    float m_run = -INFINITY, l_run = 0.f;
    const uint32_t ql = (uint32_t)l15, qpos = qrow0 + ql;             // this lane's query (row of the staged window / position)
    const bf16_t* const kb = p.qkv + (size_t)p.heads * kQfHD;                          // (one kv head)
    const bf16_t* const vb = p.qkv + (size_t)(p.heads + p.kv_heads) * kQfHD + lane * 4;
    // K rows: plain copies, 16 rows per pass (thread = row tid / 32, chunk tid % 32); V rows: one wave per row, written
    // transposed.  The second half's rows are requested BEFORE the first half's units run (32 registers): their latency
    // hides behind the units instead of following the barrier.
    constexpr int KP = MT;                                            // passes of 16 rows
    constexpr int VP = 16 * MT / NW;                                  // V rows per wave
    u4 kk[KP];
    bf4 vv[VP];
    auto fetch = [&](uint32_t key0, uint32_t kend) {
#pragma unroll
        for (int b = 0; b < KP; ++b) {
            const uint32_t r = key0 + wg + 16u * (uint32_t)b;
            kk[b] = *(const u4*)(kb + (size_t)(r < kend ? r : kend - 1u) * ld + wl32 * 8u);   // a slot past the half re-does its last row
        }
#pragma unroll
        for (int b = 0; b < VP; ++b) {
            const uint32_t r = key0 + (uint32_t)wid + (uint32_t)NW * (uint32_t)b;
            vv[b] = *(const bf4*)(vb + (size_t)(r < kend ? r : kend - 1u) * ld);
        }
    };
    fetch(0u, T < (uint32_t)(16 * MT) ? T : (uint32_t)(16 * MT));
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const uint32_t key0 = (uint32_t)(half * 16 * MT);
        const uint32_t kend = T < key0 + (uint32_t)(16 * MT) ? T : key0 + (uint32_t)(16 * MT);   // keys [key0, kend) (T > key0 by the launcher)
        if (half) __syncthreads();                                    // every unit is done with the first half's K / V^T
#pragma unroll
        for (int b = 0; b < KP; ++b) {
            const uint32_t r = key0 + wg + 16u * (uint32_t)b;
            *(u4*)(sK + (size_t)((r < kend ? r : kend - 1u) - key0) * kQfKRow + wl32 * 8u) = kk[b];
        }
#pragma unroll
        for (int b = 0; b < VP; ++b) {
            const uint32_t r = key0 + (uint32_t)wid + (uint32_t)NW * (uint32_t)b;
            const uint32_t lrow = (r < kend ? r : kend - 1u) - key0;
#pragma unroll
            for (int i = 0; i < 4; ++i) sVt[(size_t)(lane * 4 + i) * VR + lrow] = vv[b][i];
        }
        if (half == 0) fetch((uint32_t)(16 * MT), T < (uint32_t)(32 * MT) ? T : (uint32_t)(32 * MT));
        // V^T columns past the half's last key multiply P = 0: zeros (K rows past it hold anything: their scores are replaced)
        if (threadIdx.x < (uint32_t)kQfHD) {
            bf16_t* vz = sVt + (size_t)threadIdx.x * VR;
            for (uint32_t key = kend - key0; key < 32u * ((MT + 1) / 2); ++key) vz[key] = (bf16_t)0.f;
        }
        __syncthreads();
        if (wid < NH) {                                               // unit = head `wid`, the workgroup's one query tile
            const bf16_t* sQh = sQ + (size_t)wid * 16 * kQfKRow;
            f4 sc[MT];
#pragma unroll
            for (int kt = 0; kt < MT; ++kt) sc[kt] = (f4)(0.f);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const bf8 qf = *(const bf8*)(sQh + (size_t)ql * kQfKRow + 32 * s + 8 * lg);
#pragma unroll
                for (int kt = 0; kt < MT; ++kt) {
                    const bf8 kf = *(const bf8*)(sK + (size_t)(16 * kt + l15) * kQfKRow + 32 * s + 8 * lg);
                    sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, sc[kt], 0, 0, 0);
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < MT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t key = key0 + (uint32_t)(16 * kt + 4 * lg + r);
                    const uint32_t dist = key > qpos ? key - qpos : qpos - key;
                    const bool ok = key < T && (p.window == 0u || dist < p.window);
                    sc[kt][r] = ok ? sc[kt][r] : -INFINITY;
                    mx = fmaxf(mx, sc[kt][r]);
                }
            mx = xor32_max(xor16_max(mx));
            const float m_new = fmaxf(m_run, mx);
            const float mb = m_new == -INFINITY ? 0.f : m_new;        // no attendable key so far: every weight is exp(-inf) = 0
            if (half) {                                               // O and the row sum of the first half shrink by exp(m_old - m_new)
                const float a = m_run == -INFINITY ? 0.f : __expf(m_run - mb);
                l_run *= a;
#pragma unroll
                for (int j = 0; j < 16; ++j) o[j] *= a;
            }
            m_run = m_new;
            constexpr int KT2 = 2 * ((MT + 1) / 2);
            bf4 pb[KT2];
#pragma unroll
            for (int kt = 0; kt < KT2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = kt < MT ? __expf(sc[kt < MT ? kt : 0][r] - mb) : 0.f;
                    pb[kt][r] = (bf16_t)e;
                    l_run += (float)pb[kt][r];                        // the rounded weights are what multiplies V
                }
#pragma unroll
            for (int kbk = 0; kbk < (MT + 1) / 2; ++kbk) {
                bf8 pf;
#pragma unroll
                for (int r = 0; r < 4; ++r) { pf[r] = pb[2 * kbk][r]; pf[4 + r] = pb[2 * kbk + 1][r]; }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const bf16_t* vr = sVt + (size_t)(16u * (uint32_t)j + (uint32_t)l15) * VR + 32 * kbk + 4 * lg;
                    const bf4 v0 = *(const bf4*)vr, v1 = *(const bf4*)(vr + 16);
                    bf8 vf;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { vf[r] = v0[r]; vf[4 + r] = v1[r]; }
                    o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[j], 0, 0, 0);
                }
            }
        }
    }
    QF_STAMP(p, 1);
    if (wid < NH) {                                                   // O / sum over the head's Q rows (this wave is their only reader)
        const float sum = xor32_sum(xor16_sum(l_run));
        const float rinv = 1.0f / sum;                                // (a live query sees itself: sum > 0; rows past T are never stored)
        bf16_t* orow = sQ + ((size_t)wid * 16 + (uint32_t)l15) * kQfKRow + 4 * lg;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            bf4 ob;
#pragma unroll
            for (int r = 0; r < 4; ++r) ob[r] = (bf16_t)(o[j][r] * rinv);
            *(bf4*)(orow + 16 * j) = ob;
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < NH; ++j) *(u4*)(sW + (size_t)(wg + 16u * (uint32_t)t) * LDW + wl32 * 8u + 256 * j) = wreg[t][j];
    __syncthreads();
    QF_STAMP(p, 2);
    // ---- y tile = attention rows x the 32-column o_proj slice (two weight tiles); the waves split K ----
    f4 acc[2];
    acc[0] = (f4)(0.f); acc[1] = (f4)(0.f);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int k = wid * kw + 32 * s;                              // wave-uniform; a 32-wide step never straddles a head
        const bf16_t* src = sQ + (size_t)(k / kQfHD) * 16 * kQfKRow + (k % kQfHD) + 8 * lg;
        const bf8 a = *(const bf8*)(src + (size_t)l15 * kQfKRow);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bf8 wf = *(const bf8*)(sW + (size_t)(16 * t + l15) * LDW + k + 8 * lg);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, a, acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) *(f4*)(red + ((size_t)(wid * 2 + t) * 64 + lane) * 4) = acc[t];
    __syncthreads();
    if (wid >= 2) return;                                             // wave t finishes weight tile t
    f4 v = *(const f4*)(red + ((size_t)wid * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < NW; ++w) v += *(const f4*)(red + ((size_t)(w * 2 + wid) * 64 + lane) * 4);
    const uint32_t row = qrow0 + (uint32_t)l15;
    if (row >= T) return;
    bf4 ob;
#pragma unroll
    for (int r = 0; r < 4; ++r) ob[r] = (bf16_t)v[r];
    *(bf4*)(p.y + (size_t)row * p.H + blockIdx.x * (uint32_t)NC + 16u * (uint32_t)wid + 4u * (uint32_t)lg) = ob;
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QF_STAMP(p, 3); }
}

// ---- launchers: a plan (query_plan.h) -> the one instantiation of its form, with the LDS bytes of the kernel's layout -------
template <QfAttnForm F>
hipError_t qf_launch_attention_form(const QfAttnPlan& pl, const QfAttnParams& a, hipStream_t st) {
    constexpr QfAttnShape s = qf_attn_shape(F);
    static DynLdsOnce once;
    return qf_launch(qf_attention_kernel<s.mt, s.rb>, once, a, pl, qf_attn_form_lds(F, 1).total, st);
}
template <int NH, QfAttnForm F>
hipError_t qf_launch_attn_oproj_form(const QfAttnPlan& pl, const QfAttnParams& a, hipStream_t st) {
    constexpr QfAttnShape s = qf_attn_shape(F);
    static DynLdsOnce once;
    if constexpr (qf_attn_long(F))
        return qf_launch(qf_attn_oproj_long_kernel<s.mt, NH, s.nw>, once, a, pl, qf_attn_form_lds(F, NH).total, st);
    else
        return qf_launch(qf_attn_oproj_kernel<s.mt, s.rb, NH, s.nc, s.nw, s.mtq, s.qb>, once, a, pl, qf_attn_form_lds(F, NH).total, st);
}
template <int NH>
hipError_t qf_launch_attn_oproj(const QfAttnPlan& pl, const QfAttnParams& a, hipStream_t st) {
    switch (pl.form) {
        case QF_AF_AO4: return qf_launch_attn_oproj_form<NH, QF_AF_AO4>(pl, a, st);
        case QF_AF_AO8: return qf_launch_attn_oproj_form<NH, QF_AF_AO8>(pl, a, st);
        case QF_AF_AO16: return qf_launch_attn_oproj_form<NH, QF_AF_AO16>(pl, a, st);
        case QF_AF_AO32: return qf_launch_attn_oproj_form<NH, QF_AF_AO32>(pl, a, st);
        case QF_AF_AO48: return qf_launch_attn_oproj_form<NH, QF_AF_AO48>(pl, a, st);
        case QF_AF_AOB16: return qf_launch_attn_oproj_form<NH, QF_AF_AOB16>(pl, a, st);
        case QF_AF_AOB32: return qf_launch_attn_oproj_form<NH, QF_AF_AOB32>(pl, a, st);
        case QF_AF_AOB48: return qf_launch_attn_oproj_form<NH, QF_AF_AOB48>(pl, a, st);
        case QF_AF_AOB64: return qf_launch_attn_oproj_form<NH, QF_AF_AOB64>(pl, a, st);
        case QF_AF_AOB80: return qf_launch_attn_oproj_form<NH, QF_AF_AOB80>(pl, a, st);
        case QF_AF_AOL96: return qf_launch_attn_oproj_form<NH, QF_AF_AOL96>(pl, a, st);
        case QF_AF_AOL128: return qf_launch_attn_oproj_form<NH, QF_AF_AOL128>(pl, a, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t qf_launch_attn(const QfAttnPlan& pl, const QfAttnParams& a, hipStream_t st) {
    if (pl.rope_first) {
        // q / k heads normalised + rotated (q scaled) once, in place on the qkv rows: the workgroups of the kernel only copy them
        const hipError_t e = launch_qk_norm_rope(const_cast<bf16_t*>(a.qkv), a.pos, a.wq, a.wk, a.cos_sin, a.eps, a.q_scale, a.T, a.heads,
                                                 a.kv_heads, 0, st);
        if (e != hipSuccess) return e;
    }
    switch (pl.form) {
        case QF_AF_NONE: return hipErrorNotSupported;
        case QF_AF_AT4: return qf_launch_attention_form<QF_AF_AT4>(pl, a, st);
        case QF_AF_AT8: return qf_launch_attention_form<QF_AF_AT8>(pl, a, st);
        case QF_AF_AT16: return qf_launch_attention_form<QF_AF_AT16>(pl, a, st);
        case QF_AF_AT32: return qf_launch_attention_form<QF_AF_AT32>(pl, a, st);
        case QF_AF_AT48: return qf_launch_attention_form<QF_AF_AT48>(pl, a, st);
        case QF_AF_AT64: return qf_launch_attention_form<QF_AF_AT64>(pl, a, st);
        default: break;                                               // attention + o_proj in one launch: 2 or 3 q heads
    }
    if (a.heads == 3u) return qf_launch_attn_oproj<3>(pl, a, st);
    if (a.heads == 2u) return qf_launch_attn_oproj<2>(pl, a, st);
    return hipErrorInvalidValue;
}

}  // namespace cqs
