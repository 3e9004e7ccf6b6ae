// query_gemm.hip — the GEMM kernels of the search-time chain (query_forward.hip) and their launchers; also the small-row
// GEMM entry points of the BERT engines.  Which form serves which shape: query_plan.h.
#include "query_device.h"

namespace cqs {

namespace {

// What these kernels are built around (measured with QF_STAMP, then read off the ISA): at one wave per SIMD a
// wave issues one instruction per ~4-5 clocks and every launch runs its code exactly once, so a kernel's time is its
// EXECUTED INSTRUCTION COUNT.  The first versions (runtime row / tile counts behind guards inside unrolled loops) were
// 10-16 KB of straight-line code, 2 000 instructions of which ~1 100 were register copies at the guards' joins: 3-5 us
// per kernel whatever the bytes.  Hence: row-tile count MT, rows per wave RB and k-steps per batch CH are TEMPLATE
// parameters (no guards, no copies), dead slots re-do a real row instead of being predicated (same address: no extra
// bytes; same value stored to the same place), weight rows past NC repeat a real row (their output columns are never
// stored).

// ---- C = A W^T for activations that already exist as bf16 rows (o_proj, down, Dense 2) -------------------------------
// One workgroup = NC output columns x all rows; its 4 waves split K; a wave walks its K range in `nb` batches of CH
// k-steps, every load of a batch in flight before the first MFMA (K <= 1152: one batch).
template <int MT, int CH, int EPI, int NC>
__global__ __launch_bounds__(256) void qf_gemm_plain_kernel(const QfGemmParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qf_smem[];
    float* const red = (float*)qf_smem;                            // [4 waves][MT][64 lanes] f4
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    QF_STAMP(p, 0);
    const uint32_t rows = p.one_row ? 1u : p.T;
    const uint32_t K = p.K, kw = K / 4u, nb = kw / (32u * (uint32_t)CH);
    const uint32_t koff = (uint32_t)wid * kw + 8u * (uint32_t)lg;
    const bf16_t* wp = p.W + (size_t)(blockIdx.x * (uint32_t)NC + (uint32_t)(l15 % NC)) * K + koff;
    const bf16_t* ap[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const uint32_t r = 16u * (uint32_t)m + (uint32_t)l15;
        ap[m] = p.A + (size_t)(r < rows ? r : rows - 1u) * K + koff;
    }
    f4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f4)(0.f);
    for (uint32_t b = 0; b < nb; ++b) {
        bf8 wf[CH], af[MT][CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            wf[u] = *(const bf8*)(wp + 32 * u);
#pragma unroll
            for (int m = 0; m < MT; ++m) af[m][u] = *(const bf8*)(ap[m] + 32 * u);
        }
#pragma unroll
        for (int u = 0; u < CH; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], af[m][u], acc[m], 0, 0, 0);
        wp += 32 * CH;
#pragma unroll
        for (int m = 0; m < MT; ++m) ap[m] += 32 * CH;
    }
    QF_STAMP(p, 1);
    // sum the four K-quarters through LDS; wave w finishes m-tile w.  acc[m][r] = C[row 16 m + l15][col 4 lg + r]
#pragma unroll
    for (int m = 0; m < MT; ++m) *(f4*)(red + ((size_t)(wid * MT + m) * 64 + lane) * 4) = acc[m];
    __syncthreads();
    QF_STAMP(p, 2);
    if (wid >= MT) return;
    f4 v = *(const f4*)(red + ((size_t)wid * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *(const f4*)(red + ((size_t)(w * MT + wid) * 64 + lane) * 4);
    const uint32_t row = 16u * (uint32_t)wid + (uint32_t)l15;
    if (row >= rows || 4 * lg >= NC) return;                       // columns 4 lg .. 4 lg + 3 of the tile: real iff < NC
    const size_t off = (size_t)row * p.ldc + blockIdx.x * (uint32_t)NC + 4u * (uint32_t)lg;
    v = qf_bias_act(v, p.bias, p.act, blockIdx.x * (uint32_t)NC + 4u * (uint32_t)lg);
    if (EPI == QF_EPI_F32) {
        *(f4*)((float*)p.C + off) = v;
    } else {
        bf4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16_t)v[r];
        *(bf4*)((bf16_t*)p.C + off) = o;
    }
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QF_STAMP(p, 3); }
}

// ---- the same with both operands staged through LDS by COALESCED loads -----------------------------------------------------
// The kernel above feeds the MFMA straight from global memory: every fragment load is a gather of 16 rows x 64 B, ~44
// clocks of address processing per wave-instruction against ~16 for a contiguous 1 KB (measured with the stamps: with
// the same number of loads made contiguous - wrong data, timing only - `down` went from 2.05 to 1.05 us at 8 tokens, 3.3 to
// 2.0 at 32).  Here thread (row group rg = tid / 32, l32 = tid % 32) copies 16-byte chunks l32, l32 + 32, ... of rows rg,
// rg + 8, ... of the weight slice (NC consecutive rows = one contiguous block) and of the activation rows: a wave-instruction
// covers 2 rows x 512 contiguous bytes.  LDS rows are padded by 16 B (K % 128 == 0: consecutive rows land 4 banks apart).
// Chunks / rows past the end re-copy the last real one (same data to the same place: no guards in the unrolled code).
// KC32 = ceil(K / 8 / 32) chunk iterations per row, CH k-steps per batch (CH x batches = K / 4 / 32), ONE: the activations
// are one row (Dense 2).
template <int MT, int CH, int KC32, int EPI, int NC, int ONE>
__global__ __launch_bounds__(256) void qf_gemm_staged_kernel(const QfGemmParams p) {
    static_assert(NC == 8, "one 8-row weight slice per workgroup");
    extern __shared__ __attribute__((aligned(16))) unsigned char qf_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    QF_STAMP(p, 0);
    // blockIdx.y = block of 16 MT rows (33-64 tokens run as two blocks of 32: 64 rows of K = 1152 do not fit LDS beside the
    // weight slice, and the gather kernel they used to take pays ~44 clocks of address processing per fragment load)
    const uint32_t row0 = ONE ? 0u : blockIdx.y * (uint32_t)(16 * MT);
    const uint32_t rows = ONE ? 1u : (p.T - row0 < (uint32_t)(16 * MT) ? p.T - row0 : (uint32_t)(16 * MT));
    const uint32_t K = p.K, kc = K / 8u, kw = K / 4u, nb = kw / (32u * (uint32_t)CH);
    const QfStagedLds L = qf_staged_lds(MT, NC, ONE, K);
    const uint32_t ldk = L.ldk;                                    // LDS row stride (elements)
    bf16_t* const sW = (bf16_t*)qf_smem;                           // [NC][ldk]
    bf16_t* const sA = (bf16_t*)(qf_smem + L.a);                   // [16 MT][ldk]  (ONE: [1][ldk])
    float* const red = (float*)((unsigned char*)sA + L.a_bytes);   // [4 waves][MT][64 lanes] f4, at L.red

    const uint32_t rg = (uint32_t)tid >> 5, l32 = (uint32_t)tid & 31u;
    constexpr int AI = ONE ? 0 : 2 * MT;                           // activation row iterations of 8 rows
    u4 wreg[KC32], areg[AI > 0 ? AI : 1][KC32], oreg[ONE ? (KC32 + 7) / 8 : 1];
    const bf16_t* wsrc = p.W + (size_t)(blockIdx.x * (uint32_t)NC + rg) * K;
#pragma unroll
    for (int j = 0; j < KC32; ++j) {
        const uint32_t c = l32 + 32u * (uint32_t)j < kc ? l32 + 32u * (uint32_t)j : kc - 1u;
        wreg[j] = *(const u4*)(wsrc + c * 8u);
    }
    if (ONE) {                                                      // the one activation row: chunk tid, tid + 256, ...
#pragma unroll
        for (int j = 0; j < (KC32 + 7) / 8; ++j) {
            const uint32_t c = (uint32_t)tid + 256u * (uint32_t)j < kc ? (uint32_t)tid + 256u * (uint32_t)j : kc - 1u;
            oreg[j] = *(const u4*)(p.A + c * 8u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const uint32_t r = 8u * (uint32_t)i + rg;
            const bf16_t* asrc = p.A + (size_t)(row0 + (r < rows ? r : rows - 1u)) * K;
#pragma unroll
            for (int j = 0; j < KC32; ++j) {
                const uint32_t c = l32 + 32u * (uint32_t)j < kc ? l32 + 32u * (uint32_t)j : kc - 1u;
                areg[i][j] = *(const u4*)(asrc + c * 8u);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KC32; ++j) {
        const uint32_t c = l32 + 32u * (uint32_t)j < kc ? l32 + 32u * (uint32_t)j : kc - 1u;
        *(u4*)(sW + (size_t)rg * ldk + c * 8u) = wreg[j];
    }
    if (ONE) {
#pragma unroll
        for (int j = 0; j < (KC32 + 7) / 8; ++j) {
            const uint32_t c = (uint32_t)tid + 256u * (uint32_t)j < kc ? (uint32_t)tid + 256u * (uint32_t)j : kc - 1u;
            *(u4*)(sA + c * 8u) = oreg[j];
        }
    } else {
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const uint32_t r = 8u * (uint32_t)i + rg;
            const uint32_t rr = r < rows ? r : rows - 1u;
#pragma unroll
            for (int j = 0; j < KC32; ++j) {
                const uint32_t c = l32 + 32u * (uint32_t)j < kc ? l32 + 32u * (uint32_t)j : kc - 1u;
                *(u4*)(sA + (size_t)rr * ldk + c * 8u) = areg[i][j];
            }
        }
    }
    __syncthreads();
    QF_STAMP(p, 1);
    // fragments: weight row l15 % NC (rows past NC repeat real rows: their output columns are never stored), activation
    // row 16 m + l15 (rows past `rows` hold whatever LDS held: they only feed output columns that are never stored)
    const uint32_t koff = (uint32_t)wid * kw + 8u * (uint32_t)lg;
    const bf16_t* wp = sW + (size_t)(l15 % NC) * ldk + koff;
    const bf16_t* ap = sA + (size_t)(ONE ? 0 : l15) * ldk + koff;
    f4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f4)(0.f);
    for (uint32_t b = 0; b < nb; ++b) {
        bf8 wf[CH], af[MT][CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            wf[u] = *(const bf8*)(wp + 32 * u);
#pragma unroll
            for (int m = 0; m < MT; ++m) af[m][u] = *(const bf8*)(ap + (size_t)(ONE ? 0 : 16 * m) * ldk + 32 * u);
        }
#pragma unroll
        for (int u = 0; u < CH; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], af[m][u], acc[m], 0, 0, 0);
        wp += 32 * CH;
        ap += 32 * CH;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) *(f4*)(red + ((size_t)(wid * MT + m) * 64 + lane) * 4) = acc[m];
    __syncthreads();
    QF_STAMP(p, 2);
    if (wid >= MT) return;
    f4 v = *(const f4*)(red + ((size_t)wid * 64 + lane) * 4);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *(const f4*)(red + ((size_t)(w * MT + wid) * 64 + lane) * 4);
    const uint32_t row = 16u * (uint32_t)wid + (uint32_t)l15;
    if (row >= rows || 4 * lg >= NC) return;
    const size_t off = (size_t)(row0 + row) * p.ldc + blockIdx.x * (uint32_t)NC + 4u * (uint32_t)lg;
    v = qf_bias_act(v, p.bias, p.act, blockIdx.x * (uint32_t)NC + 4u * (uint32_t)lg);
    if (EPI == QF_EPI_F32) {
        *(f4*)((float*)p.C + off) = v;
    } else {
        bf4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16_t)v[r];
        *(bf4*)((bf16_t*)p.C + off) = o;
    }
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QF_STAMP(p, 3); }
}

// ---- GEMMs whose activations are made on the way in: embedding gather / add + RMSNorm pair (/ + mean pool) ---------
// NCH = H / 256, K = H.  Rows: one WAVE per row, wave w takes rows w, w + 4, ... in batches of RB rows (RB = 1, 2, 4
// by T for T <= 16: one batch; longer queries loop over batches of 4, the next batch's loads issued before the current
// one is reduced).  A batch slot past T re-does row T - 1.
// RO: the K-split reduction buffer `red` OVERLAYS the activation tile (one more barrier between the fragment reads and the
// partial sums) - 48-row blocks with two weight tiles then fit LDS.
template <int NCH, int PRO, int EPI, int NC, int RB, int MT, int NW, int BR = 16 * MT, bool RO = false>
__global__ __launch_bounds__(64 * NW) void qf_gemm_kernel(const QfGemmParams p) {
    constexpr int H = NCH * 256;
    constexpr int NT = EPI == QF_EPI_GEGLU ? 2 : 1;               // weight tiles per workgroup
    constexpr int GT = PRO == QF_PRO_POOL ? 1 : MT;                // row tiles of the GEMM (POOL: the one pooled row)
    constexpr QfProLds L = qf_pro_lds(NCH, NT, NC, GT, NW, PRO == QF_PRO_POOL, RO);
    constexpr int LDA = L.lda;                                     // LDS activation row stride (elements)
    extern __shared__ __attribute__((aligned(16))) unsigned char qf_smem[];
    bf16_t* const sA = (bf16_t*)qf_smem;                           // [16 GT][LDA]
    static_assert(!RO || L.red_bytes <= L.a_bytes, "red fits inside the activation tile");
    float* const red = (float*)(qf_smem + L.red);                  // [NW waves][NT][GT][64 lanes] f4
    float* const pool = (float*)(qf_smem + L.pool);                // POOL: [NW waves][H] column sums
    bf16_t* const sW = (bf16_t*)(qf_smem + L.w);                   // [NT][NC][LDA] weight slice

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    QF_STAMP(p, 0);
    // blockIdx.y = row block (17-32 tokens: two blocks of 16 rows x 16-column tiles - a workgroup then pulls 16 rows of
    // x / y through its CU's L2 port instead of all 32: the prologue is bound by exactly that); rows are
    // local to the block from here on, `T` = how many of them are real
    // (BR < 16: 9-16 tokens as two blocks of 8 rows - half the MFMA tile's rows idle, but 8 rows less to pull and one row
    // per wave in the prologue)
    static_assert(BR <= 16 * MT, "a row block fits the workgroup's row tiles");
    const uint32_t row0 = blockIdx.y * (uint32_t)BR;
    const uint32_t T = p.T - row0 < (uint32_t)BR ? p.T - row0 : (uint32_t)BR;
    constexpr uint32_t kw = H / NW;                                // this wave's K range: [wid kw, (wid + 1) kw)
    constexpr int S = H / NW / 32;                                 // k-steps of 32 per wave
    static_assert(H % (32 * NW) == 0, "the waves split K in whole 32-deep steps");

    // weight rows of the workgroup's tile(s).  GeGLU: W rows are interleaved per 64 (32 gate rows, then the same
    // channels' 32 up rows; embedder.hip set_tensor) -> channels [NC b, NC b + NC) = gate rows 64 (c / 32) + c % 32.
    uint32_t wrow0 = blockIdx.x * (uint32_t)NC;
    if (EPI == QF_EPI_GEGLU) wrow0 = 64u * (wrow0 >> 5) + (wrow0 & 31u);
    // The weight slice (NC consecutive rows per tile = one contiguous block) is requested first, with COALESCED loads
    // (thread = row tid / 32 of the slice, 16-byte chunks tid % 32 + 32 j: a wave-instruction covers 2 rows x 512 B; a
    // fragment gather of 16 rows x 64 B costs ~44 clocks of address processing per instruction against ~16), lands while
    // the rows are normalised and goes through LDS: sW [NT][NC][LDA].
    static_assert(NC == 8 || NC == 16, "an 8- or 16-row weight slice per tile");
    // slice row i = NC tile + r (i < NT NC) is copied by the 32-thread group i % (2 NW), pass i / (2 NW)
    constexpr int WG32 = 2 * NW;                                   // 32-thread groups of the workgroup
    constexpr int WL = (NT * NC + WG32 - 1) / WG32;                // slice rows per group
    const uint32_t wg = (uint32_t)tid >> 5, wl32 = (uint32_t)tid & 31u;
    u4 wreg[WL][NCH];
#pragma unroll
    for (int t = 0; t < WL; ++t) {
        const uint32_t i = wg + (uint32_t)(WG32 * t);
        const uint32_t ic = i < (uint32_t)(NT * NC) ? i : (uint32_t)(NT * NC - 1);     // (a group past the slice re-copies its last row)
        const bf16_t* src = p.W + (size_t)(wrow0 + 32u * (ic / (uint32_t)NC) + ic % (uint32_t)NC) * H + wl32 * 8u;
#pragma unroll
        for (int j = 0; j < NCH; ++j) wreg[t][j] = *(const u4*)(src + 256 * j);
    }

    // lane owns 4 consecutive floats of each 256-chunk of a row
    f4 wn1[NCH], wp1[NCH];                                         // 1 + w
    const uint32_t c0 = (uint32_t)lane * 4u;
    auto load_row = [&](uint32_t row, f4 (&xv)[NCH], f4 (&yv)[NCH]) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (PRO == QF_PRO_EMBED) {
                const bf4 e = *(const bf4*)(p.emb + (size_t)(uint32_t)p.tok[row0 + row] * H + c * 256 + c0);
#pragma unroll
                for (int i = 0; i < 4; ++i) xv[c][i] = (float)e[i] * p.scale;
            } else if (PRO == QF_PRO_ADDLN) {
                const bf4 xb = *(const bf4*)(p.xb_in + (size_t)(row0 + row) * H + c * 256 + c0);
                const bf4 yb = *(const bf4*)(p.y + (size_t)(row0 + row) * H + c * 256 + c0);
#pragma unroll
                for (int i = 0; i < 4; ++i) xv[c][i] = (float)xb[i] + (float)yb[i];
            } else {
                xv[c] = *(const f4*)(p.x_in + (size_t)(row0 + row) * H + c * 256 + c0);
                const bf4 yb = *(const bf4*)(p.y + (size_t)(row0 + row) * H + c * 256 + c0);
#pragma unroll
                for (int i = 0; i < 4; ++i) yv[c][i] = (float)yb[i];
            }
        }
    };
    f4 psum[NCH];                                                  // POOL: this wave's column sums
#pragma unroll
    for (int c = 0; c < NCH; ++c) psum[c] = (f4)(0.f);
    auto finish_row = [&](uint32_t row, bool count, f4 (&xv)[NCH], f4 (&yv)[NCH]) {
        if (PRO == QF_PRO_ADDLN) {
            // LayerNorm of v = x + y (bert_add_ln_kernel's arithmetic: mean, then the biased variance around it, two passes
            // over the registers); wp1 = gamma, wn1 = beta
            float sm = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) sm += xv[c][i];
            const float mean = wave_sum64_readlane(sm) / (float)H;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) { const float a = xv[c][i] - mean; q += a * a; }
            const float inv = rsqrtf(wave_sum64_readlane(q) / (float)H + p.eps);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                bf4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (bf16_t)((xv[c][i] - mean) * inv * wp1[c][i] + wn1[c][i]);
                *(bf4*)(sA + (size_t)row * LDA + c * 256 + c0) = o;
                if (blockIdx.x == 0) *(bf4*)(p.xb_out + (size_t)(row0 + row) * H + c * 256 + c0) = o;
            }
            return;
        }
        if (PRO != QF_PRO_EMBED) {                                   // x += norm(y) (1 + w_post)   (add_norm_kernel's arithmetic)
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) ss += yv[c][i] * yv[c][i];
            const float invy = rsqrtf(wave_sum64_readlane(ss) / (float)H + p.eps);
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) xv[c][i] += yv[c][i] * invy * wp1[c][i];
        }
        float sx = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) sx += xv[c][i] * xv[c][i];
        const float invx = rsqrtf(wave_sum64_readlane(sx) / (float)H + p.eps);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (PRO == QF_PRO_POOL) {
                if (count) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) psum[c][i] += xv[c][i] * invx * wn1[c][i];     // f32 hidden state, summed
                }
            } else {
                bf4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (bf16_t)(xv[c][i] * invx * wn1[c][i]);
                *(bf4*)(sA + (size_t)row * LDA + c * 256 + c0) = o;
                if (blockIdx.x == 0) *(f4*)(p.x_out + (size_t)(row0 + row) * H + c * 256 + c0) = xv[c];
            }
        }
    };
    f4 xv[RB][NCH], yv[RB][NCH];
    const uint32_t last = T - 1u;
#pragma unroll
    for (int b = 0; b < RB; ++b) {
        const uint32_t r = (uint32_t)wid + (uint32_t)NW * (uint32_t)b;
        load_row(r < T ? r : last, xv[b], yv[b]);
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const f4 a = *(const f4*)(p.w_next + c * 256 + c0);
        if (PRO == QF_PRO_ADDLN) {                                   // beta, gamma as they are
            wn1[c] = a;
            wp1[c] = *(const f4*)(p.w_post + c * 256 + c0);
            continue;
        }
        wn1[c] = a + 1.0f;
        if (PRO != QF_PRO_EMBED) wp1[c] = *(const f4*)(p.w_post + c * 256 + c0) + 1.0f;
    }
    if (MT == 1) {
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const uint32_t r = (uint32_t)wid + (uint32_t)NW * (uint32_t)b;
            finish_row(r < T ? r : last, r < T, xv[b], yv[b]);
        }
    } else {                                                        // RB = 4; 16 rows per pass of the workgroup, passes one after
        for (uint32_t r0 = (uint32_t)wid;;) {                        // the other (a second set of rows in flight spills the registers)
#pragma unroll
            for (int b = 0; b < RB; ++b) {
                const uint32_t r = r0 + (uint32_t)NW * (uint32_t)b;
                finish_row(r < T ? r : last, r < T, xv[b], yv[b]);
            }
            r0 += (uint32_t)(NW * RB);
            if (r0 >= T) break;
#pragma unroll
            for (int b = 0; b < RB; ++b) {
                const uint32_t r = r0 + (uint32_t)NW * (uint32_t)b;
                load_row(r < T ? r : last, xv[b], yv[b]);
            }
        }
    }
    if (PRO == QF_PRO_POOL) {
        // masked mean pool (src/embedder/pooling.rs:87-128) of the final-norm rows -> ONE activation row (bf16, as
        // mean_pool_kernel hands it to the Dense head)
#pragma unroll
        for (int c = 0; c < NCH; ++c) *(f4*)(pool + (size_t)wid * H + c * 256 + c0) = psum[c];
        __syncthreads();
        for (uint32_t col = (uint32_t)tid; col < (uint32_t)H; col += (uint32_t)(64 * NW)) {
            float sm = pool[col];
#pragma unroll
            for (int w = 1; w < NW; ++w) sm += pool[(size_t)w * H + col];
            sA[col] = (bf16_t)(sm / (float)T);
        }
        // (rows 1..15 of the m-tile stay whatever LDS held: an activation row only feeds its own output column of the
        // MFMA, and columns past the real rows are never stored)
    }
    // rows [T, 16 MT) of the tile are not initialised either, for the same reason
#pragma unroll
    for (int t = 0; t < WL; ++t) {
        const uint32_t i = wg + (uint32_t)(WG32 * t);
        const uint32_t ic = i < (uint32_t)(NT * NC) ? i : (uint32_t)(NT * NC - 1);
#pragma unroll
        for (int j = 0; j < NCH; ++j) *(u4*)(sW + (size_t)ic * LDA + wl32 * 8u + 256 * j) = wreg[t][j];
    }
    __syncthreads();
    QF_STAMP(p, 1);
    // ---- multiply: B operand (activations) from LDS: lane feeds row 16 m + l15, k = wid kw + 32 s + 8 lg .. + 7 ----
    bf8 wf[NT][S];                                                 // weight row l15 % NC (rows past NC repeat real rows)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < S; ++s) wf[t][s] = *(const bf8*)(sW + (size_t)(t * NC + l15 % NC) * LDA + (uint32_t)wid * kw + 8u * (uint32_t)lg + 32 * s);
    f4 acc[NT][GT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int m = 0; m < GT; ++m) acc[t][m] = (f4)(0.f);
    const bf16_t* la = sA + (size_t)l15 * LDA + (uint32_t)wid * kw + 8u * (uint32_t)lg;
#pragma unroll
    for (int m = 0; m < GT; ++m)
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const bf8 a = *(const bf8*)(la + (size_t)(16 * m) * LDA + 32 * s);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][s], a, acc[t][m], 0, 0, 0);
        }
    // ---- sum the four K-quarters through LDS; wave w finishes m-tile w.  acc[t][m][r] = C[row 16 m + l15][col 4 lg + r] ----
    if (RO) __syncthreads();                                        // everybody's fragment reads of the tile `red` overlays are done
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int m = 0; m < GT; ++m) *(f4*)(red + ((size_t)((wid * NT + t) * GT + m) * 64 + lane) * 4) = acc[t][m];
    __syncthreads();
    QF_STAMP(p, 2);
    if (wid >= GT) return;
    f4 v[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        v[t] = *(const f4*)(red + ((size_t)((0 * NT + t) * GT + wid) * 64 + lane) * 4);
#pragma unroll
        for (int w = 1; w < NW; ++w) v[t] += *(const f4*)(red + ((size_t)((w * NT + t) * GT + wid) * 64 + lane) * 4);
    }
    const uint32_t rows = PRO == QF_PRO_POOL ? 1u : T;
    const uint32_t row = 16u * (uint32_t)wid + (uint32_t)l15;
    if (row >= rows || 4 * lg >= NC) return;                       // columns 4 lg .. 4 lg + 3 of the tile: real iff < NC
    const size_t off = (size_t)(row0 + row) * p.ldc + blockIdx.x * (uint32_t)NC + 4u * (uint32_t)lg;
    bf4 o;
    if (EPI == QF_EPI_GEGLU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16_t)(gelu_tanh(v[0][r]) * v[NT - 1][r]);
    } else {
        if (PRO == QF_PRO_ADDLN) v[0] = qf_bias_act(v[0], p.bias, p.act, blockIdx.x * (uint32_t)NC + 4u * (uint32_t)lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16_t)v[0][r];
    }
    *(bf4*)((bf16_t*)p.C + off) = o;
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); QF_STAMP(p, 3); }
}

// ---- launchers: a plan (query_plan.h) -> the one instantiation of its form, with the LDS bytes of the kernel's layout -------
template <int NCH, int PRO, int EPI, QfProForm F>
hipError_t qf_launch_pro_form(const QfProPlan& pl, const QfGemmParams& p, hipStream_t st) {
    constexpr QfProShape s = qf_pro_shape(F, NCH, EPI == QF_EPI_GEGLU);
    static DynLdsOnce once;
    return qf_launch(qf_gemm_kernel<NCH, PRO, EPI, s.nc, s.rb, s.mt, s.nw, s.br, s.ro>, once, p, pl,
                     qf_pro_form_lds(F, NCH, PRO == QF_PRO_POOL, EPI == QF_EPI_GEGLU).total, st);
}

template <int MT, int EPI, int ONE, int KI>
hipError_t qf_launch_staged_k(const QfGemmPlan& pl, const QfGemmParams& p, hipStream_t st) {
    if (p.K != kQfStagedK[KI].K) return hipErrorInvalidValue;
    static DynLdsOnce once;
    return qf_launch(qf_gemm_staged_kernel<MT, kQfStagedK[KI].ch, kQfStagedK[KI].kc32, EPI, 8, ONE>, once, p, pl,
                     qf_staged_lds(MT, 8, ONE, p.K).total, st);
}
template <int MT, int EPI, int ONE>
hipError_t qf_launch_staged(const QfGemmPlan& pl, const QfGemmParams& p, hipStream_t st) {
    switch (pl.kclass) {
        case 0: return qf_launch_staged_k<MT, EPI, ONE, 0>(pl, p, st);
        case 1: return qf_launch_staged_k<MT, EPI, ONE, 1>(pl, p, st);
        case 2: return qf_launch_staged_k<MT, EPI, ONE, 2>(pl, p, st);
        case 3: return qf_launch_staged_k<MT, EPI, ONE, 3>(pl, p, st);
        case 4: return qf_launch_staged_k<MT, EPI, ONE, 4>(pl, p, st);
        case 5: return qf_launch_staged_k<MT, EPI, ONE, 5>(pl, p, st);
        default: return hipErrorInvalidValue;
    }
}

template <int MT, int CH, int EPI>
hipError_t qf_launch_gather_ch(const QfGemmPlan& pl, const QfGemmParams& p, hipStream_t st) {
    if (p.K % (128u * CH)) return hipErrorInvalidValue;             // a wave walks its K quarter in whole batches of CH k-steps
    static DynLdsOnce once;
    return qf_launch(qf_gemm_plain_kernel<MT, CH, EPI, 8>, once, p, pl, qf_plain_lds(MT), st);
}
template <int MT, int EPI>
hipError_t qf_launch_gather(const QfGemmPlan& pl, const QfGemmParams& p, hipStream_t st) {
    switch (pl.ch) {
        case 9: return qf_launch_gather_ch<MT, 9, EPI>(pl, p, st);
        case 6: return qf_launch_gather_ch<MT, 6, EPI>(pl, p, st);
        case 4: return qf_launch_gather_ch<MT, 4, EPI>(pl, p, st);
        case 3: return qf_launch_gather_ch<MT, 3, EPI>(pl, p, st);
        case 2: return qf_launch_gather_ch<MT, 2, EPI>(pl, p, st);
        case 1: return qf_launch_gather_ch<MT, 1, EPI>(pl, p, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// Weight-tile width by projection (8 columns: EmbeddingGemma's QKV 160, o_proj / down 96, GeGLU 144, Dense 1 384, Dense 2 96
// workgroups): the kernels are instruction-bound, not byte-bound - a narrower tile adds workgroups, not speed.
template <int NCH, int PRO, int EPI>
hipError_t qf_launch_pro(const QfProPlan& pl, const QfGemmParams& p, hipStream_t st) {
    // a form that no plan gives this kind of projection is not instantiated for it
    constexpr bool kPool = PRO == QF_PRO_POOL, kGeglu = EPI == QF_EPI_GEGLU;
    switch (pl.form) {
        case QF_PF_W4: return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_W4>(pl, p, st);
        case QF_PF_W8: return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_W8>(pl, p, st);
        case QF_PF_W16: return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_W16>(pl, p, st);
        case QF_PF_W32: return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_W32>(pl, p, st);
        case QF_PF_W48: return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_W48>(pl, p, st);
        case QF_PF_W64: return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_W64>(pl, p, st);
        case QF_PF_W128: if constexpr (kPool) return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_W128>(pl, p, st); break;
        case QF_PF_B8C8: if constexpr (!kPool) return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_B8C8>(pl, p, st); break;
        case QF_PF_B8C16: if constexpr (!kPool) return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_B8C16>(pl, p, st); break;
        case QF_PF_B16: if constexpr (!kPool) return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_B16>(pl, p, st); break;
        case QF_PF_B32: if constexpr (kGeglu) return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_B32>(pl, p, st); break;
        case QF_PF_B48: if constexpr (kGeglu) return qf_launch_pro_form<NCH, PRO, EPI, QF_PF_B48>(pl, p, st); break;
        case QF_PF_NONE: break;
    }
    return hipErrorNotSupported;
}
template hipError_t qf_launch_pro<1, QF_PRO_EMBED, QF_EPI_BF16>(const QfProPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_pro<1, QF_PRO_ADDNORM, QF_EPI_BF16>(const QfProPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_pro<1, QF_PRO_ADDNORM, QF_EPI_GEGLU>(const QfProPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_pro<1, QF_PRO_POOL, QF_EPI_BF16>(const QfProPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_pro<3, QF_PRO_EMBED, QF_EPI_BF16>(const QfProPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_pro<3, QF_PRO_ADDNORM, QF_EPI_BF16>(const QfProPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_pro<3, QF_PRO_ADDNORM, QF_EPI_GEGLU>(const QfProPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_pro<3, QF_PRO_POOL, QF_EPI_BF16>(const QfProPlan&, const QfGemmParams&, hipStream_t);

template <int EPI>
hipError_t qf_launch_gemm(const QfGemmPlan& pl, const QfGemmParams& p, hipStream_t st) {
    switch (pl.form) {
        case QF_GF_STAGED_ONE: return qf_launch_staged<1, EPI, 1>(pl, p, st);
        case QF_GF_STAGED:
            switch (pl.mt) {
                case 1: return qf_launch_staged<1, EPI, 0>(pl, p, st);
                case 2: return qf_launch_staged<2, EPI, 0>(pl, p, st);
                case 3: return qf_launch_staged<3, EPI, 0>(pl, p, st);
                default: return hipErrorInvalidValue;
            }
        case QF_GF_GATHER:
            switch (pl.mt) {
                case 1: return qf_launch_gather<1, EPI>(pl, p, st);
                case 2: return qf_launch_gather<2, EPI>(pl, p, st);
                case 3: return qf_launch_gather<3, EPI>(pl, p, st);
                case 4: return qf_launch_gather<4, EPI>(pl, p, st);
                default: return hipErrorInvalidValue;
            }
        case QF_GF_NONE: break;
    }
    return hipErrorNotSupported;
}
template hipError_t qf_launch_gemm<QF_EPI_BF16>(const QfGemmPlan&, const QfGemmParams&, hipStream_t);
template hipError_t qf_launch_gemm<QF_EPI_F32>(const QfGemmPlan&, const QfGemmParams&, hipStream_t);

// C[M, N] = act(A[M, K] W[N, K]^T + bias) for M <= 64 rows (a search-time SPLADE query, a rerank of one short passage):
// the search-time GEMM kernels above - 8 output columns per workgroup, K split over its 4 waves, both operands staged
// through LDS by coalesced loads where they fit - instead of one wave walking all of K per 32 x 32 tile.
// hipErrorNotSupported: shape outside what those kernels take (the caller falls back).
hipError_t launch_gemm_small_rows(const bf16_t* A, const bf16_t* W, const float* bias, void* C, uint32_t M, uint32_t N,
                                  uint32_t K, uint32_t ldc, GemmOut out, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (M > 64u || N % 8u || K % 128u || K < 128u) return hipErrorNotSupported;   // (the BERT engines' search-time shapes; the Gemma chain itself goes to 128 rows)
    if (out != GEMM_OUT_BF16 && out != GEMM_OUT_BF16_GELU && out != GEMM_OUT_F32) return hipErrorNotSupported;
    QfGemmParams p{};
    p.T = M; p.A = A; p.K = K; p.W = W; p.C = C; p.ldc = ldc; p.bias = bias; p.act = out == GEMM_OUT_BF16_GELU ? 1 : 0;
    const QfGemmPlan pl = qf_plan_gemm(M, false, K, N, qf_switches());
    return out == GEMM_OUT_F32 ? qf_launch_gemm<QF_EPI_F32>(pl, p, st) : qf_launch_gemm<QF_EPI_BF16>(pl, p, st);
}

// The same with the producer's residual add + LayerNorm in the prologue (BERT's post-LN layers):
//   x_out = bf16(LayerNorm(x + y) gamma + beta);  C = act(x_out W^T + bias)
// for M <= 64 rows, K = H in {256, 768, 1024}; x_out != x (every workgroup reads x, column tile 0 writes x_out).
hipError_t launch_gemm_small_rows_addln(const bf16_t* x, const bf16_t* y, const float* gamma, const float* beta, float eps,
                                        bf16_t* x_out, const bf16_t* W, const float* bias, void* C, uint32_t M, uint32_t N,
                                        uint32_t H, uint32_t ldc, GemmOut out, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (M > 64u || N % 16u || x == x_out || (out != GEMM_OUT_BF16 && out != GEMM_OUT_BF16_GELU)) return hipErrorNotSupported;
    QfGemmParams p{};
    p.T = M; p.xb_in = x; p.y = y; p.w_post = gamma; p.w_next = beta; p.eps = eps; p.xb_out = x_out;
    p.W = W; p.C = C; p.ldc = ldc; p.bias = bias; p.act = out == GEMM_OUT_BF16_GELU ? 1 : 0;
    const QfProPlan pl = qf_plan_pro(M, (int)(H / 256u), false, false, N, qf_switches());
    if (H == 768u) return qf_launch_pro<3, QF_PRO_ADDLN, QF_EPI_BF16>(pl, p, st);
    if (H == 1024u) return qf_launch_pro<4, QF_PRO_ADDLN, QF_EPI_BF16>(pl, p, st);
    if (H == 256u) return qf_launch_pro<1, QF_PRO_ADDLN, QF_EPI_BF16>(pl, p, st);
    return hipErrorNotSupported;
}

}  // namespace cqs

