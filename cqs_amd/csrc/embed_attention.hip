// embed_attention.hip — the two attention kernels of the EmbeddingGemma forward (embed_rows.hip has the file family's
// introduction), the plan that picks one, and every attention ablation switch.
#include "embed_kernels.h"

#include <cstdlib>
#include <type_traits>

namespace cqs {

// ---- attention --------------------------------------------------------------------------
// S^T = K Q^T (keys on rows, queries on lanes: softmax is lane-local), O^T += V^T P^T with the
// S^T accumulator used directly as the B operand (no LDS round trip for P).
// LDS tiles are split by the MFMA lane group g = lane >> 4 so that a fragment read's bank only depends
// on its row:  sK[g][key][8 k-steps x 8 dims + 8 pad]  (row stride 144 B: 16 rows -> 16 distinct 16-B slots)
//              sV[g][dim][8 keys = the group's B-operand slots]  (row stride 16 B: 16 rows = one 256-B bank row)
constexpr int kKRow = 64 + 8;               // elements per sK row
constexpr int kKSub = 32 * kKRow;           // elements per lane-group sub-tile (4608 B = 18 x 256 B)
constexpr int kVSub = kHD * 8;              // elements per lane-group sub-tile of sV

// One workgroup = 8 waves (2 per SIMD: one wave's MFMAs overlap the other's softmax VALU) = 128
// consecutive queries of ONE q-head of one sequence, 16 queries per wave (16x16x32 MFMA tiles keep the
// wave at ~150 VGPRs: O^T 64 + Q 32 + S 8, no accumulator spills into AGPRs).  The K / V^T tiles of
// the head's kv group are staged once per 32-key block for all eight waves.
//   S^T (32 keys x 16 q)  = K (A: 16 keys x 32 dims per tile) x Q^T (B, registers)     16 MFMAs
//   O^T (256 d x 16 q)   += V^T (A: 16 dims x 32 keys) x P^T (B = the S^T registers)    16 MFMAs
// C layout of 16x16: col = lane&15 (query), row = 4*(lane>>4) + reg.  So lane group g = lane>>4 owns
// keys {4g..4g+3} of each 16-key tile; used as the B operand its 8 slots are keys
// {4g..4g+3, 16+4g..16+4g+3} of the block, and the V^T fragment is read in the same order.
constexpr float kRescaleThr = 8.0f;  // defer the O rescale while the running max grows by < e^8 (P stays < 2981)

// Q^T fragments (B operand of S^T = K Q^T): lane feeds Q[q = lane & 15][dims 32s + 8 lg + 0..7], s = 0..7.
// With q_norm_w: q-head RMSNorm * (1 + w), RoPE and the 1/sqrt(query_pre_attn_scalar) scale on the wave's own
// fragments (what qk_norm_rope_kernel does for the k heads): the query's 256 dims live in this lane (64 of them) and
// in lanes ^16, ^32, ^48; rotate_half pairs dim d with d +/- 128 = fragments s and s + 4 of the SAME lane.
__device__ __forceinline__ void load_q_fragments(bf8 (&qf)[8], const bf16_t* __restrict__ qrow /*token row + head*/, int lg,
                                                 const float* __restrict__ q_norm_w, const float* __restrict__ cs /*[128][2] of the position*/,
                                                 float eps, float q_scale) {
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *(const bf8*)(qrow + 32 * s + 8 * lg);
    if (!q_norm_w) return;
    float ss = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float v = (float)qf[s][j]; ss += v * v; }
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    const float inv = rsqrtf(ss / (float)kHD + eps);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t d0 = (uint32_t)(32 * s + 8 * lg);    // dims d0 .. d0+7 (< 128) and their partners d0 + 128
        f4 c[4], wlo[2], whi[2];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = *(const f4*)(cs + 2u * d0 + 4u * (uint32_t)u);   // (cos,sin) x 2 dims each
#pragma unroll
        for (int u = 0; u < 2; ++u) { wlo[u] = *(const f4*)(q_norm_w + d0 + 4 * u); whi[u] = *(const f4*)(q_norm_w + 128u + d0 + 4 * u); }
        bf8 lo, hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float co = c[j >> 1][2 * (j & 1)], si = c[j >> 1][2 * (j & 1) + 1];
            const float nlo = (float)qf[s][j] * inv * (1.0f + wlo[j >> 2][j & 3]);
            const float nhi = (float)qf[s + 4][j] * inv * (1.0f + whi[j >> 2][j & 3]);
            lo[j] = (bf16_t)((nlo * co - nhi * si) * q_scale);      // d < 128: n cos - x[d+128] sin
            hi[j] = (bf16_t)((nhi * co + nlo * si) * q_scale);      // d >= 128: n cos + x[d-128] sin
        }
        qf[s] = lo;
        qf[s + 4] = hi;
    }
}

template <int WAVES, int G>
__global__ __launch_bounds__(64 * WAVES) void attention_kernel(const bf16_t* __restrict__ qkv,
                                                        const bf16_t* __restrict__ vt,
                                                        bf16_t* __restrict__ out,
                                                        const int32_t* __restrict__ blk,
                                                        const int32_t* __restrict__ seq_start,
                                                        const int32_t* __restrict__ seq_len,
                                                        const int32_t* __restrict__ vt_start, uint32_t vt_ld,
                                                        uint32_t heads, uint32_t kv_heads, uint32_t window,
                                                        const float* __restrict__ q_norm_w,
                                                        const float* __restrict__ cos_sin, float eps, float q_scale) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[4 * kKSub + 4 * kVSub];
    bf16_t* sK = smem;
    bf16_t* sV = smem + 4 * kKSub;
    // The workgroup owns TQ = WAVES / G tiles of 16 consecutive queries for ALL G q-heads of one kv head:
    // wave -> (query tile wid / G, head wid % G), so one staged K / V^T tile serves G heads.
    constexpr int T = 64 * WAVES;                   // threads
    constexpr int TQ = WAVES / G;                   // query tiles
    constexpr uint32_t kParts = 128 / (16 * TQ);    // workgroups per 128-query super-block of the blk list
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const uint32_t sblk = blockIdx.x / kParts, part = blockIdx.x % kParts;
    const uint32_t b = (uint32_t)blk[2 * sblk], sb = (uint32_t)blk[2 * sblk + 1];
    // blockIdx.y counts groups of G consecutive q-heads (G = heads / kv_heads: one kv head; G = 1: one q-head)
    const uint32_t head = blockIdx.y * (uint32_t)G + (uint32_t)(wid % G);
    const uint32_t g = head / (heads / kv_heads);
    const uint32_t s0 = (uint32_t)seq_start[b], L = (uint32_t)seq_len[b], v0 = (uint32_t)vt_start[b];
    const uint32_t ld = (heads + 2u * kv_heads) * kHD;
    const uint32_t koff = (heads + g) * kHD;
    const uint32_t qbase = sb * 128u + part * (16u * TQ);      // the workgroup's first query
    if (qbase >= L) return;                                    // (uniform: before any barrier)
    const uint32_t q0 = qbase + (uint32_t)(wid / G) * 16u;     // this wave's first query
    const bool wave_live = q0 < L;                          // waves past the sequence only help staging
    const uint32_t qi = q0 + (uint32_t)l15;                 // this lane's query

    const uint32_t qclamp = qi < L ? qi : L - 1u;           // position in the sequence (rows past the end: any real row)
    bf8 qf[8];
    load_q_fragments(qf, qkv + (size_t)(s0 + qclamp) * ld + head * kHD, lg, q_norm_w, cos_sin + (size_t)qclamp * 256u, eps, q_scale);

    f4 o[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d] = (f4)(0.f);
    float m_run = -INFINITY, l_run = 0.f;

    // key blocks that can hold an attendable key: workgroup range (staging) and this wave's own range
    const uint32_t nkb = (L + 31u) / 32u;
    uint32_t kb_lo = 0, kb_hi = nkb, wkb_lo = 0, wkb_hi = nkb;
    if (window) {
        const uint32_t glo = qbase, ghi = glo + 16u * TQ - 1u;     // workgroup's queries
        kb_lo = (glo + 1u > window) ? (glo + 1u - window) / 32u : 0u;
        kb_hi = (ghi + window - 1u) / 32u + 1u;
        if (kb_hi > nkb) kb_hi = nkb;
        const uint32_t qhi = q0 + 15u;                              // this wave's queries
        wkb_lo = (q0 + 1u > window) ? (q0 + 1u - window) / 32u : 0u;
        wkb_hi = (qhi + window - 1u) / 32u + 1u;
    }

    // K / V^T tiles go through registers one key block ahead (kU + kU x 16 B per thread)
    constexpr int kU = (1024 + T - 1) / T;
    u4 rk[kU], rv[kU];
    auto stage_load = [&](uint32_t kb) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = u * T + tid;
            if (1024 % T != 0 && i >= 1024) break;
            const uint32_t kr = (uint32_t)i / (kHD / 8), c = ((uint32_t)i % (kHD / 8)) * 8u;
            uint32_t key = kb * 32u + kr;
            key = key < L ? key : L - 1u;   // rows past the sequence: any finite row, masked later
            rk[u] = *(const u4*)(qkv + (size_t)(s0 + key) * ld + koff + c);
            const uint32_t d = (uint32_t)i / 4u, cv = ((uint32_t)i % 4u) * 8u;
            rv[u] = *(const u4*)(vt + ((size_t)g * kHD + d) * vt_ld + v0 + kb * 32u + cv);
        }
    };
    auto stage_write = [&]() {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = u * T + tid;
            if (1024 % T != 0 && i >= 1024) break;
            // K: 16-B chunk cc of key row kr = dims 8cc..8cc+7 = k-step cc/4, lane group cc%4
            const uint32_t kr = (uint32_t)i / (kHD / 8), cc = (uint32_t)i % (kHD / 8);
            *(u4*)(sK + (cc & 3u) * kKSub + kr * kKRow + (cc >> 2) * 8u) = rk[u];
            // V^T: chunk a of dim row d = keys 8a..8a+7: keys 8a+0..3 are slots 4(a/2)..+3 of lane group
            // 2(a%2), keys 8a+4..7 the same slots of lane group 2(a%2)+1
            const uint32_t d = (uint32_t)i / 4u, a = (uint32_t)i % 4u;
            bf16_t* vd = sV + (2u * (a & 1u)) * kVSub + d * 8u + 4u * (a >> 1);
            *(u2*)vd = (u2){rv[u][0], rv[u][1]};
            *(u2*)(vd + kVSub) = (u2){rv[u][2], rv[u][3]};
        }
    };
    if (kb_lo < kb_hi) stage_load(kb_lo);
    for (uint32_t kb = kb_lo; kb < kb_hi; ++kb) {
        __syncthreads();  // previous tile fully consumed
        stage_write();
        __syncthreads();
#ifndef CQS_ATT_ABLATE_NOLOAD
        if (kb + 1u < kb_hi) stage_load(kb + 1u);
#endif
        if (!wave_live || kb < wkb_lo || kb >= wkb_hi) continue;   // wave-uniform
#ifdef CQS_ATT_ABLATE_NOCOMPUTE
        if (kb != kb_lo) continue;
#endif

        // S^T tiles: keys [0,16) and [16,32) of the block x this wave's 16 queries.  Fragment reads are
        // issued 8 at a time AHEAD of their MFMAs (left alone, hipcc emits read -> wait -> MFMA pairs and
        // every MFMA eats a full LDS round trip).
        f4 sc[2];
        sc[0] = (f4)(0.f);
        sc[1] = (f4)(0.f);
        // kRA fragment reads in flight ahead of their MFMAs: 8 with two waves per SIMD; 4 for the 12-wave layout
        // (three waves per SIMD hide the rest, and 8 spilled 13 registers to scratch at its 168-VGPR budget)
        constexpr int kRA = WAVES >= 12 ? 4 : 8;
#pragma unroll
        for (int grp = 0; grp < 16 / kRA; ++grp) {
            bf8 kf[kRA];
#pragma unroll
            for (int u = 0; u < kRA; ++u) {
                const int i = grp * kRA + u, st = i >> 1, kt = i & 1;
                kf[u] = *(const bf8*)(sK + lg * kKSub + (kt * 16 + l15) * kKRow + 8 * st);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < kRA; ++u) {
                const int i = grp * kRA + u, st = i >> 1, kt = i & 1;
                sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[u], qf[st], sc[kt], 0, 0, 0);
            }
        }
        // mask (only on blocks that touch the sequence end or the window edge) + online softmax over this
        // lane's 8 keys; the query's other 24 keys live in lanes ^16, ^32, ^48
        const uint32_t k_first = kb * 32u, k_last = k_first + 31u;
        const bool interior = k_last < L && (!window || ((q0 + 15u < k_first + window) && (k_last < q0 + window)));
        float mloc = -INFINITY;
        if (interior) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) mloc = fmaxf(mloc, sc[kt][r]);
        } else {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t key = k_first + (uint32_t)(kt * 16 + 4 * lg + r);
                    bool ok = key < L;
                    if (window) {
                        const uint32_t dist = key > qi ? key - qi : qi - key;
                        ok = ok && dist < window;
                    }
                    sc[kt][r] = ok ? sc[kt][r] : -INFINITY;
                    mloc = fmaxf(mloc, sc[kt][r]);
                }
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        // Deferred rescale: the running max only moves when the block max exceeds it by more than
        // kRescaleThr; until then P = exp(s - m_run) <= e^8, exact in f32 and fine in bf16.
        const bool need = mloc > m_run + kRescaleThr || (m_run == -INFINITY && mloc != -INFINITY);
        if (__any(need)) {
            const float m_new = need ? mloc : m_run;
            const float a = need ? ((m_run == -INFINITY) ? 0.f : __expf(m_run - m_new)) : 1.f;
            l_run *= a;
#pragma unroll
            for (int d = 0; d < 16; ++d) o[d] *= a;
            m_run = m_new;
        }
        const float m_use = (m_run == -INFINITY) ? 0.f : m_run;   // no attendable key yet: every p = 0
        float lsum = 0.f;
        bf8 pf;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = __expf(sc[kt][r] - m_use);   // exp(-inf) = 0 for masked keys
                lsum += pv;
                pf[kt * 4 + r] = (bf16_t)pv;                    // slot (lg, 4kt + r) <-> key 16kt + 4lg + r
            }
        lsum += __shfl_xor(lsum, 16, 64);
        lsum += __shfl_xor(lsum, 32, 64);
        l_run += lsum;
        // slots 0..3 = keys 4lg + 0..3, slots 4..7 = keys 16 + 4lg + 0..3: one 16-B read per dim tile,
        // again kRA reads ahead of their MFMAs
#pragma unroll
        for (int grp = 0; grp < 16 / kRA; ++grp) {
            bf8 vf[kRA];
#pragma unroll
            for (int u = 0; u < kRA; ++u) vf[u] = *(const bf8*)(sV + lg * kVSub + ((grp * kRA + u) * 16 + l15) * 8);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < kRA; ++u)
                o[grp * kRA + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u], pf, o[grp * kRA + u], 0, 0, 0);
        }
    }

    // O^T[d][q]: lane <-> query l15, register r of tile d <-> dim 16d + 4lg + r
    if (wave_live && qi < L) {
        const float invl = l_run > 0.f ? 1.0f / l_run : 0.f;
        bf16_t* op = out + (size_t)(s0 + qi) * (heads * kHD) + head * kHD;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            bf4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (bf16_t)(o[d][e] * invl);
            *(bf4*)(op + 16 * d + 4 * lg) = w;
        }
    }
}

// ---- attention, second generation: 64-key blocks, LDS-DMA double buffer ---------------------------------
// Same math and wave layout as attention_kernel (wave = 16 queries of one q-head; S^T = K Q^T, O^T += V^T P^T), but
// the K / V tiles never pass through registers: each 64-key block (K and V rows as they lie in the qkv buffer, 64 x 256
// each = 32 KiB) is fetched by `global_load_lds_dwordx4` into the buffer the previous block is not using, ONE barrier
// per 64 keys (attention_kernel: two per 32, plus 6 ds_write per thread), the softmax's cross-lane steps use
// v_permlane{16,32}_swap instead of ds_bpermute (which queues behind the fragment reads), and the PV product's V^T
// fragments come from the ROW-major V image through `ds_read_b64_tr_b16` (hardware transpose: no V^T buffer, no
// v_transpose launch on this path).
// LDS images are unpadded; the bank swizzle is applied to the DMA's SOURCE address (the destination is lane-linear):
//   K [key row 0..63][32 chunks of 8 dims]   chunk c of row r lives at c ^ fK(r), fK(r) = 4 ((r >> 3) & 3) + (r & 3)
//   V [key row 0..63][32 chunks of 8 dims]   chunk c of row r lives at c ^ fV(r), fV(r) = 2 (r & 3) + 8 ((r >> 3) & 1)
// The S^T tile (t, kt) takes its 16 key rows in the order row(i) = 32 t + 8 (i >> 2) + 4 kt + (i & 3), so that lane
// group lg's C registers of tiles kt = 0, 1 hold the 8 CONSECUTIVE keys 32 t + 8 lg + 0..7 = k-indices 8 lg + 0..7 of
// the PV product, and fK(row(i)) = i.  A transposed read serves, per 16-lane group, 4 key rows x 16 dims: lane 4q + p
// supplies the address of (key 8 lg + 4 h + q, dims 16 dt + 4 p ..+3) and lane i receives dim 16 dt + i of the 4 keys;
// h = 0, 1 give the 8 k-indices.  fV makes the 8 rows a 32-lane half touches land in 8 distinct 32-byte bank slots.
constexpr int kABlk = 64;                    // keys per block
constexpr int kABuf = kABlk * kHD;           // elements of one K (or V^T) buffer: 32 KiB
constexpr size_t kAttDmaLds = (size_t)4 * kABuf * sizeof(bf16_t);   // [2] K + [2] V^T = 128 KiB

template <int WAVES, int G, int KRA_F>   // KRA_F: fragment reads in flight ahead of their MFMAs
__global__ __launch_bounds__(64 * WAVES) void attention_dma_kernel(const bf16_t* __restrict__ qkv,
                                                        const bf16_t* __restrict__ vt,
                                                        bf16_t* __restrict__ out,
                                                        const int32_t* __restrict__ blk,
                                                        const int32_t* __restrict__ seq_start,
                                                        const int32_t* __restrict__ seq_len,
                                                        const int32_t* __restrict__ vt_start, uint32_t vt_ld,
                                                        uint32_t heads, uint32_t kv_heads, uint32_t window,
                                                        const float* __restrict__ q_norm_w,
                                                        const float* __restrict__ cos_sin, float eps, float q_scale) {
    extern __shared__ __attribute__((aligned(16))) bf16_t asmem[];   // K[2][64 x 256] | V^T[2][256 x 64]
    constexpr int TQ = WAVES / G;                   // query tiles
    constexpr uint32_t kParts = 128 / (16 * TQ);    // workgroups per 128-query super-block of the blk list
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    // Workgroups go to the 8 XCDs round-robin by blockIdx.x; give each XCD one CONTIGUOUS run of the (sequence, query
    // block) list, so the workgroups that share a sequence's K / V^T share an L2 (blockIdx.x-order put them on 8
    // different XCDs: PMC showed 143 MB fetched per launch for 42 MB of q/k/v, every L2 streaming every sequence).
    const uint32_t nwg = gridDim.x, xcd = blockIdx.x % 8u, q8 = nwg / 8u, r8 = nwg % 8u;
    const uint32_t wg = (xcd < r8 ? xcd * (q8 + 1u) : r8 * (q8 + 1u) + (xcd - r8) * q8) + blockIdx.x / 8u;
    const uint32_t sblk = wg / kParts, part = wg % kParts;
    const uint32_t b = (uint32_t)blk[2 * sblk], sb = (uint32_t)blk[2 * sblk + 1];
    const uint32_t head = blockIdx.y * (uint32_t)G + (uint32_t)(wid % G);
    const uint32_t g = head / (heads / kv_heads);
    const uint32_t s0 = (uint32_t)seq_start[b], L = (uint32_t)seq_len[b];   // (vt / vt_start / vt_ld: unused here)
    const uint32_t ld = (heads + 2u * kv_heads) * kHD;
    const uint32_t koff = (heads + g) * kHD;
    const uint32_t qbase = sb * 128u + part * (16u * TQ);      // the workgroup's first query
    if (qbase >= L) return;                                    // (uniform: before any barrier)
    const uint32_t q0 = qbase + (uint32_t)(wid / G) * 16u;     // this wave's first query
    const bool wave_live = q0 < L;                          // waves past the sequence only help staging
    const uint32_t qi = q0 + (uint32_t)l15;                 // this lane's query

    // 64-key blocks that can hold an attendable key: workgroup range (staging) and this wave's own range
    const uint32_t nkb = (L + (uint32_t)kABlk - 1u) / (uint32_t)kABlk;
    uint32_t kb_lo = 0, kb_hi = nkb, wkb_lo = 0, wkb_hi = nkb;
    if (window) {
        const uint32_t glo = qbase, ghi = glo + 16u * TQ - 1u;     // workgroup's queries
        kb_lo = (glo + 1u > window) ? (glo + 1u - window) / (uint32_t)kABlk : 0u;
        kb_hi = (ghi + window - 1u) / (uint32_t)kABlk + 1u;
        if (kb_hi > nkb) kb_hi = nkb;
        const uint32_t qhi = q0 + 15u;                              // this wave's queries
        wkb_lo = (q0 + 1u > window) ? (q0 + 1u - window) / (uint32_t)kABlk : 0u;
        wkb_hi = (qhi + window - 1u) / (uint32_t)kABlk + 1u;
    }

    // LDS-DMA of one block: 32 K instructions + 32 V instructions of 2 key rows (512 B each), instruction i by wave
    // i % WAVES.  M0 = LDS byte address of the instruction's 1 KiB; lane l lands at byte 16 l.  Rows past the sequence
    // read its last key (finite; masked / multiplied by P = 0 later).
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) bf16_t*)asmem;
    const char* const gK = (const char*)(qkv + (size_t)s0 * ld + koff);
    const uint32_t vrel = kv_heads * (uint32_t)kHD * 2u;          // byte distance from a token's k head to its v head
    auto dma = [&](const char* sbase, uint32_t voff, uint32_t lds_byte) {
        asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                     :: "s"(lds_byte), "v"(voff), "s"(sbase) : "memory");
    };
    constexpr int NI = (32 + WAVES - 1) / WAVES;
    auto stage = [&](uint32_t kb, uint32_t p) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const uint32_t i = (uint32_t)wid + (uint32_t)(WAVES * j);
            if (32 % WAVES != 0 && i >= 32u) break;                 // wave-uniform
            const uint32_t r = 2u * i + (uint32_t)(lane >> 5);
            uint32_t key = kb * (uint32_t)kABlk + r;
            key = key < L ? key : L - 1u;
            const uint32_t kc = (uint32_t)(lane & 31) ^ (4u * ((r >> 3) & 3u) + (r & 3u));
            const uint32_t vc = (uint32_t)(lane & 31) ^ (2u * (r & 3u) + 8u * ((r >> 3) & 1u));
            dma(gK, (key * ld + kc * 8u) * 2u, lds0 + p * (uint32_t)(kABuf * 2) + i * 1024u);
            dma(gK, (key * ld + vc * 8u) * 2u + vrel, lds0 + (uint32_t)(2 * kABuf * 2) + p * (uint32_t)(kABuf * 2) + i * 1024u);
        }
    };
    if (kb_lo < kb_hi) stage(kb_lo, 0u);      // in flight under the Q prologue
#ifdef CQS_ATT2_NO_QNORM
    q_norm_w = nullptr;
#endif

    const uint32_t qclamp = qi < L ? qi : L - 1u;
    bf8 qf[8];
    load_q_fragments(qf, qkv + (size_t)(s0 + qclamp) * ld + head * kHD, lg, q_norm_w, cos_sin + (size_t)qclamp * 256u, eps, q_scale);
    // Pin the fragments here: with their loads still "pending" at the loop head (the q_norm_w == NULL path), hipcc
    // places its s_waitcnt vmcnt(n..0) inside the loop body, where it would drain the next block's DMA every iteration.
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(qf[s]));

    // fragment addresses (elements, buffer 0).  K: row(i = l15) of tile (t, kt) = 32 t + 4 kt + 8 (l15 >> 2) + (l15 & 3),
    // chunk (4 st + lg) ^ l15 = 16 (st >> 2) + 4 ((st & 3) ^ (l15 >> 2)) + (lg ^ (l15 & 3)): four lane-dependent bases.
    const bf16_t* kp[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
        kp[s] = asmem + (uint32_t)(8 * (l15 >> 2) + (l15 & 3)) * (uint32_t)kHD +
                (uint32_t)(4 * (s ^ (l15 >> 2)) + (lg ^ (l15 & 3))) * 8u;
    // V (transposed reads): lane 16 lg + 4 q + p addresses key row 8 lg + q (+ 4 h + 32 t), chunk 2 dt + (p >> 1), half
    // (p & 1); the chunk's position is 2 (dt ^ xq) + (p >> 1) with xq = q + 4 (lg & 1): eight lane-dependent bases by dt & 7.
    typedef short tr4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) tr4* lds_tr4;
    const int tq = (lane >> 2) & 3, tp = lane & 3, xq = tq + 4 * (lg & 1);
    uint32_t vb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        vb[j] = lds0 + (uint32_t)(2 * kABuf * 2) + (uint32_t)(8 * lg + tq) * (uint32_t)(kHD * 2) +
                (uint32_t)(2 * (j ^ xq) + (tp >> 1)) * 16u + (uint32_t)(tp & 1) * 8u;

    f4 o[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d] = (f4)(0.f);
    float m_run = -INFINITY, l_run = 0.f;

#ifdef CQS_ATT2_NO_LOOP
    kb_hi = kb_lo + 1u;
#endif
    // One 64-key block out of buffer P (compile-time: the buffer offset rides in the ds_read immediates, no per-block
    // pointer arithmetic and no second set of address registers)
    auto block = [&](uint32_t kb, auto par_c) {
        constexpr uint32_t p = (uint32_t)decltype(par_c)::value;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of block kb has landed
        __syncthreads();                                       // everyone's has; block kb - 1 is fully consumed
#ifndef CQS_ATT2_NO_DMA
        if (kb + 1u < kb_hi) stage(kb + 1u, p ^ 1u);
#endif
        if (!wave_live || kb < wkb_lo || kb >= wkb_hi) return;     // wave-uniform
#ifdef CQS_ATT2_NO_COMPUTE
        if (kb != kb_lo) return;
#endif
        constexpr uint32_t pofs = p * (uint32_t)kABuf;
        const uint32_t kb_first = kb * (uint32_t)kABlk;
        using FencedRA = std::integral_constant<int, KRA_F>;
        // S^T tiles kt = 0, 1 of half t: 16 MFMAs, fragment reads KRA ahead.  `fenced`: keep each read group ahead of its
        // MFMA group (left alone, hipcc emits read -> wait -> MFMA pairs and every MFMA eats a full LDS round trip);
        // unfenced, the caller lays the schedule down with sched_group_barrier.
        auto s_phase = [&](int t, f4 (&sc)[2], auto ra_c) {
            constexpr int RA = decltype(ra_c)::value;      // > 0: fenced groups of RA reads; < 0: unfenced, -RA
            constexpr bool fenced = RA > 0;
            constexpr int KRA = RA > 0 ? RA : -RA;
            sc[0] = (f4)(0.f);
            sc[1] = (f4)(0.f);
#pragma unroll
            for (int grp = 0; grp < 16 / KRA; ++grp) {
                bf8 kf[KRA];
#pragma unroll
                for (int u = 0; u < KRA; ++u) {
                    const int i = grp * KRA + u, st = i >> 1, kt = i & 1;
#if defined(CQS_ATT2_NO_LDSREAD)
                    kf[u] = qf[(st + kt) & 7];
#else
                    kf[u] = *(const bf8*)(kp[st & 3] + pofs + (uint32_t)((32 * t + 4 * kt) * kHD + (st >> 2) * 128));
#endif
                }
                if (fenced) __builtin_amdgcn_sched_barrier(0);
#ifndef CQS_ATT2_NO_S
#pragma unroll
                for (int u = 0; u < KRA; ++u) {
                    const int i = grp * KRA + u, st = i >> 1, kt = i & 1;
                    sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[u], qf[st], sc[kt], 0, 0, 0);
                }
#else
#pragma unroll
                for (int u = 0; u < KRA; ++u) sc[u & 1][0] += (float)kf[u][0];
#endif
            }
        };
        // O^T += V^T P^T over half t: 16 dim tiles, one 16-byte fragment each
        auto pv_phase = [&](int t, const bf8& pf, auto ra_c) {
            constexpr int RA = decltype(ra_c)::value;
            constexpr bool fenced = RA > 0;
            constexpr int KRA = RA > 0 ? RA : -RA;
#pragma unroll
            for (int grp = 0; grp < 16 / KRA; ++grp) {
                bf8 vf[KRA];
#pragma unroll
#if defined(CQS_ATT2_NO_LDSREAD)
                for (int u = 0; u < KRA; ++u) vf[u] = qf[(grp + u) & 7];
#else
                for (int u = 0; u < KRA; ++u) {
                    const int dt = grp * KRA + u;
                    const uint32_t ad = vb[dt & 7] + pofs * 2u + (uint32_t)(t * 32 * kHD * 2 + (dt >> 3) * 256);
                    const tr4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr4)(uintptr_t)ad);
                    const tr4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr4)(uintptr_t)(ad + (uint32_t)(4 * kHD * 2)));
                    vf[u] = __builtin_bit_cast(bf8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                }
#endif
                if (fenced) __builtin_amdgcn_sched_barrier(0);
#ifndef CQS_ATT2_NO_PV
#pragma unroll
                for (int u = 0; u < KRA; ++u)
                    o[grp * KRA + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u], pf, o[grp * KRA + u], 0, 0, 0);
#else
#pragma unroll
                for (int u = 0; u < KRA; ++u) o[grp * KRA + u][0] += (float)vf[u][0] * (float)pf[0];
#endif
            }
        };
        // Online softmax of one half (this lane: 8 keys of query qi; the other 24 live in lanes ^16, ^32, ^48), branch-free
        // up to the (rare) rescale: sc[kt][r] = score of key k_first + 8 lg + 4 kt + r; returns P as the PV product's B
        // fragment (k-index 8 lg + 4 kt + r).  Deferred rescale: the running max only moves when the half's max exceeds it
        // by more than kRescaleThr; until then P = exp(s - m_run) <= e^8, exact in f32 and fine in bf16.
        constexpr float kLog2e = 1.4426950408889634f;
        auto softmax = [&](const f4 (&sc)[2], float mloc, bf8& pf, float& m_old, float& lsum) -> bool {
            // (branch-free on purpose: one basic block with the MFMAs it is interleaved with; the caller applies the
            // rescale of the lanes that return true - `need` - in a separate, rarely taken block)
            mloc = xor32_max(xor16_max(mloc));
            const bool need = (mloc > m_run + kRescaleThr) | ((m_run == -INFINITY) & (mloc != -INFINITY));   // (no short-circuit: no branch)
            m_old = m_run;
            m_run = need ? mloc : m_run;
            const float mb = (m_run == -INFINITY) ? 0.f : m_run * kLog2e;   // no attendable key yet: every p = 0
            lsum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#ifdef CQS_ATT2_NO_EXP
                    const float pv = sc[kt][r] - mb;
#else
                    const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kt][r], kLog2e, -mb));   // exp(-inf) = 0 for masked keys
#endif
                    lsum += pv;
                    pf[kt * 4 + r] = (bf16_t)pv;
                }
            return need;
        };
        // lanes with `need` moved their running max from m_old to m_run: O and the row sum shrink by exp(m_old - m_run)
        // (0 when there was no max yet: exp2(-inf))
        auto rescale = [&](bool need, float m_old) {
            const float a = need ? __builtin_amdgcn_exp2f((m_old - m_run) * kLog2e) : 1.f;
            l_run *= a;
#pragma unroll
            for (int d = 0; d < 16; ++d) o[d] *= a;
        };
        auto max8 = [&](const f4 (&sc)[2]) {
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, sc[kt][r]);
            return m;
        };

        // Edge blocks (sequence end or a window edge inside them) mask key by key; a half without any attendable key
        // just yields P = 0.  (Measured and dropped: half 1's S^T MFMAs issued between half 0's softmax VALU, half 0's
        // PV MFMAs between half 1's softmax - sched_group_barrier interleave, 2 reads ahead to stay in 168 VGPRs:
        // 44.9 us vs 42.5.  The loop is co-bound: per 32 keys the CU's 12 waves need 1536 clk of MFMA per SIMD, 1536 clk
        // of LDS fragment reads and ~1000 clk of VALU, and removing any ONE of them leaves the time unchanged.)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t k_first = kb_first + 32u * (uint32_t)t, k_last = k_first + 31u;
            if (k_first >= L) break;                               // wave-uniform: the half lies past the sequence
            if (window && (k_last + window <= q0 || k_first >= q0 + 15u + window)) continue;   // no query of the wave sees it
            f4 sc[2];
            s_phase(t, sc, FencedRA{});
            // sc[kt][r] = score of key k_first + 8 lg + 4 kt + r for query qi
            const bool interior = k_last < L && (!window || ((q0 + 15u < k_first + window) && (k_last < q0 + window)));
            if (!interior) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t key = k_first + (uint32_t)(8 * lg + 4 * kt + r);
                        bool ok = key < L;
                        if (window) {
                            const uint32_t dist = key > qi ? key - qi : qi - key;
                            ok = ok && dist < window;
                        }
                        sc[kt][r] = ok ? sc[kt][r] : -INFINITY;
                    }
            }
            bf8 pf;
            float m_old, lsum;
            const bool need = softmax(sc, max8(sc), pf, m_old, lsum);
            if (__any(need)) rescale(need, m_old);
            l_run += lsum;              // per-lane partial of the row sum; reduced over the lane groups at the end
            pv_phase(t, pf, FencedRA{});
        }
    };
    for (uint32_t kb = kb_lo; kb < kb_hi; kb += 2u) {
        block(kb, std::integral_constant<int, 0>{});
        if (kb + 1u < kb_hi) block(kb + 1u, std::integral_constant<int, 1>{});
    }

    // O^T[d][q]: lane <-> query l15, register r of tile d <-> dim 16d + 4lg + r.  Through the wave's own 8 KiB of LDS
    // (the K buffers are dead after the barrier) so that the global stores are whole 512-byte head rows, 16 B per lane:
    // direct 8-byte stores (16 rows x 32 B per instruction) cost 7.5 us of this kernel's 48.
    l_run = xor32_sum(xor16_sum(l_run));
    __syncthreads();
    {
        const float invl = l_run > 0.f ? 1.0f / l_run : 0.f;
        // row q (512 B = 32 chunks of 8 dims): dims 16d + 4lg + 0..3 = half (lg & 1) of chunk 2d + (lg >> 1), stored at
        // chunk position c ^ (q & 7) ... 8-byte writes: lanes l15 = 0..15 hit distinct rows (stride 512 B = same bank
        // group) -> the XOR spreads them over 8 of the 16 slots; 2-way on a write costs nothing extra.
        bf16_t* const so = asmem + (uint32_t)wid * (16u * kHD);
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            bf4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (bf16_t)(o[d][e] * invl);
            const uint32_t c = (uint32_t)(2 * d + (lg >> 1)) ^ (uint32_t)(l15 & 7) ^ (uint32_t)((l15 >> 3) << 3);
            *(bf4*)(so + (uint32_t)l15 * kHD + c * 8u + (uint32_t)(lg & 1) * 4u) = w;
        }
        // (same wave wrote and reads: no barrier, the compiler's lgkmcnt wait orders the LDS accesses)
        const uint32_t rr = (uint32_t)(lane >> 5), cc = (uint32_t)(lane & 31);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t q = 2u * (uint32_t)i + rr;                      // query row of the wave's tile
            const uint32_t c = cc ^ (q & 7u) ^ ((q >> 3) << 3);
            const u4 v = *(const u4*)(so + q * kHD + c * 8u);
            if (wave_live && q0 + q < L)
                *(u4*)(out + (size_t)(s0 + q0 + q) * (heads * kHD) + head * kHD + cc * 8u) = v;
        }
    }
}

// Which attention kernel a batch gets.  With several q-heads per kv head: head-sharing workgroups on the 64-key LDS-DMA
// kernel (row-major V, no V^T), from ~1.5k tokens on - rounds 1-2 kept one q-head per workgroup on the register-staged
// kernel (which reads V^T) below one head-sharing workgroup per CU ("more, thinner workgroups fill the chip better": +6 %
// against round 1's head-sharing kernel); against the LDS-DMA kernel that rule lost 2-7 % of the whole forward at 4-48
// ragged sequences (tools/embed_att_layout_sweep.sh, round 3).  CQS_HIP_ATT_KERNEL=reg keeps the register-staged kernel,
// CQS_HIP_ATT_LAYOUT=shared / per-head forces a layout (test hooks: every combination is checked against the oracle).
struct AttPlan { bool share, dma; };
static AttPlan att_plan(uint32_t nblk, uint32_t heads, uint32_t kv_heads) {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
            n_cu = 256;
    }
    const uint32_t ratio = kv_heads ? heads / kv_heads : 0u;
    bool share = ratio > 1u && nblk * 2u * kv_heads >= 24u;      // (under ~1.5k tokens - one sequence - the thin workgroups are as fast or faster)
    (void)n_cu;
    if (const char* f = getenv("CQS_HIP_ATT_LAYOUT")) {
        if (f[0] == 's') share = ratio > 1u;
        else if (f[0] == 'p') share = false;
    }
    bool dma = share && ratio >= 2u && ratio <= 4u;
    if (const char* f = getenv("CQS_HIP_ATT_KERNEL")) dma = dma && f[0] != 'r';
    return {share, dma};
}
bool attention_reads_vt(uint32_t nblk, uint32_t heads, uint32_t kv_heads) { return !att_plan(nblk, heads, kv_heads).dma; }

hipError_t launch_attention(const bf16_t* qkv, const bf16_t* vt, bf16_t* out, const int32_t* blk, uint32_t nblk,
                            const int32_t* seq_start, const int32_t* seq_len, const int32_t* vt_start, uint32_t vt_ld,
                            uint32_t heads, uint32_t kv_heads, uint32_t window, const float* q_norm_w,
                            const float* cos_sin, float eps, float q_scale, hipStream_t st) {
    if (nblk == 0) return hipSuccess;
    if (kv_heads == 0 || heads % kv_heads) return hipErrorInvalidValue;
#ifndef CQS_ATT_TQ
#define CQS_ATT_TQ 4
#endif
    // One workgroup = CQS_ATT_TQ tiles of 16 queries x all q-heads of a kv head (EmbeddingGemma: 4 x 3 = 12
    // waves, 64 queries): the staged K / V^T tiles serve 192 query-heads instead of 128 (8 waves x 1 head),
    // and 32 x 512-token sequences make 256 workgroups = one per CU in one round instead of 384.
    // (4 q-heads per kv head: 2 tiles, or the 16 waves would be held to 128 VGPRs and spill)
#define CQS_ATT(GV, TQV)                                                                                           \
    hipLaunchKernelGGL((attention_kernel<TQV * GV, GV>), dim3(nblk * (128 / (16 * TQV)), heads / GV),             \
                       dim3(64 * TQV * GV), 0, st, qkv, vt, out, blk, seq_start, seq_len, vt_start, vt_ld, heads,   \
                       kv_heads, window, q_norm_w, cos_sin, eps, q_scale)
    const uint32_t ratio = heads / kv_heads;
    const AttPlan plan = att_plan(nblk, heads, kv_heads);
    const bool share = plan.share, use_dma = plan.dma;
    if (!share) { CQS_ATT(1, 8); return hipGetLastError(); }
#define CQS_ATT_DMA(GV, TQV, KRAV)                                                                                  \
    do {                                                                                                            \
        auto kern = attention_dma_kernel<TQV * GV, GV, KRAV>;                                                       \
        static std::atomic<uint64_t> attr_devices{0};                                                               \
        {                                                                                                           \
            const hipError_t e = set_max_dynamic_lds((const void*)kern, kAttDmaLds, attr_devices);                  \
            if (e != hipSuccess) return e;                                                                          \
        }                                                                                                           \
        hipLaunchKernelGGL(kern, dim3(nblk * (128 / (16 * TQV)), heads / GV), dim3(64 * TQV * GV), kAttDmaLds, st,  \
                           qkv, vt, out, blk, seq_start, seq_len, vt_start, vt_ld, heads, kv_heads, window,         \
                           q_norm_w, cos_sin, eps, q_scale);                                                        \
    } while (0)
    if (use_dma) {
        switch (ratio) {
            case 2: CQS_ATT_DMA(2, 4, 8); break;
            case 3: CQS_ATT_DMA(3, CQS_ATT_TQ, 4); break;
            case 4: CQS_ATT_DMA(4, 2, 8); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
#undef CQS_ATT_DMA
    switch (ratio) {
        case 2: CQS_ATT(2, 4); break;
        case 3: CQS_ATT(3, CQS_ATT_TQ); break;
        case 4: CQS_ATT(4, 2); break;
        default: return hipErrorInvalidValue;
    }
#undef CQS_ATT
    return hipGetLastError();
}

}  // namespace cqs
