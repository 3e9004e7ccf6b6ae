// scan_bf16.hip — gfx950 kernels of the dense index's bf16 shadow.
//
//  shadow_build_kernel   one pass over the f32 rows: bf16 copy (v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN)
//                        and the index-wide error bound R.
//  shadow_bound_kernel   one wave per query: B_q = ||q|| R (shadow_query_bound) into a device buffer, so that a search
//                        enqueued without a host sync can certify.
//  scan_bf16_kernel      HBM-streaming dot of every bf16 row with 1..8 f32 queries: half the bytes of scan_gemv_kernel.
//                        Same tasks / work queue / score + gmax (+ gaux) layout, so the unchanged select_finish_kernel
//                        takes each query's top k' + 1 approximate keys.
//  rescore_certify_kernel  one launch for a block's tail.  One wave per candidate: the exact f32 score, bit for bit what
//                        scan_gemv_kernel computes; one wave per query: B_q, unless an earlier launch computed it; the
//                        last workgroup of each query to arrive: top k of the rescored candidates (the select's rank
//                        sort) and the certificate that no row outside them can enter the top k.
//
// Wave = 64 lanes.  gfx950 only.
#include "scan_bf16.h"
#include "scan_i8.h"
#include "f32_score.h"
#include "launch_util.h"
#include "rank_sort.h"
#include "scan_gemv_device.h"
#include "select_device.h"
#include "shadow_build_device.h"
#include "tail_plan.h"
#include "tail_prefix.h"

namespace cqs {

static_assert(kShadowKMax == kMaxK, "shadow k' policy and the select agree on max k");

__device__ __forceinline__ float key_score(uint64_t key) {                                        // inverse of okey
    const uint32_t ok = (uint32_t)(key >> 32);
    return __uint_as_float((ok & 0x80000000u) ? (ok ^ 0x80000000u) : ~ok);
}

// ---- build ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void shadow_build_kernel(const float* __restrict__ rows, uint16_t* __restrict__ shadow,
                                                           uint64_t row0, uint64_t n_rows, uint32_t dim, double gamma,
                                                           unsigned long long* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        shadow_build_row(rows + (row0 + r) * dim, shadow + (row0 + r) * dim, dim, gamma, stats, lane);
    }
}

hipError_t launch_shadow_build(const float* rows, uint16_t* shadow, uint64_t row0, uint64_t n_rows, uint32_t dim,
                               double gamma, unsigned long long* stats, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    const uint64_t blocks = (n_rows + 3u) / 4u;
    hipLaunchKernelGGL(shadow_build_kernel, dim3((uint32_t)(blocks < 8192u ? blocks : 8192u)), dim3(256), 0, st, rows,
                       shadow, row0, n_rows, dim, gamma, stats);
    return hipGetLastError();
}

// ---- per-query bound ----------------------------------------------------------------------------------------------
// ||q||^2 as an f64 sum (the squares of f32 components are exact in f64; the order differs from a host loop, which the
// 2^-40 slack of shadow_query_bound covers), then the same bound function the host compiles: wave_shadow_bound, which the
// fused rescore + certify kernel shares.  Stand-alone for PIPELINE searches (the scan's drop rule reads B_q) and the
// debug hooks.
__global__ __launch_bounds__(64) void shadow_bound_kernel(const float* __restrict__ q, uint32_t dim, double r_max,
                                                          double norm_max, float* __restrict__ bq) {
    const uint32_t lane = threadIdx.x;
    const float v = wave_shadow_bound(q + (size_t)blockIdx.x * dim, dim, r_max, norm_max, lane);
    if (lane == 0) bq[blockIdx.x] = v;
}

hipError_t launch_shadow_bound(const float* q, uint32_t b, uint32_t dim, double r_max, double norm_max, float* bq,
                               hipStream_t st) {
    if (b == 0) return hipSuccess;
    if (b > kShadowMaxQ) return hipErrorInvalidValue;
    hipLaunchKernelGGL(shadow_bound_kernel, dim3(b), dim3(64), 0, st, q, dim, r_max, norm_max, bq);
    return hipGetLastError();
}

// ---- approximate scan -------------------------------------------------------------------------------------------
struct Bf16ScanParams {
    const uint16_t* rows;   // [n, dim] bf16
    uint32_t n, n_pad, dim;
    const float* q;
    float* scores;
    const uint32_t* keep;
    uint32_t mode;
    float thr;
    uint32_t nq;            // queries present (<= BQ)
    uint32_t* work;
    TaskTiers tiers;
    uint32_t n_tasks;
    float* gmax;
    uint64_t* gaux;         // nullable
    const float* bq;        // [nq] B_q of each query of the pass (device)
    uint32_t keep_stride;   // PQ: `keep` is a table of bitsets, this many words per row ...
    uint8_t slot[kMaxGemvQ];// ... and query b of the pass is filtered by row slot[b] (ScanArgs::keep_tab)
};

// NCH = ceil(dim / 512): 1-KiB bf16 chunks per row; lane owns components [c*512 + lane*8, +8) of chunk c (one 16-byte load).
// A partial last chunk (FULL = false, 768-d: lanes 32..63 of chunk 1) reads a clamped in-row address against a zero query
// fragment, as scan_gemv_kernel does.  Batch by batch (loads, then math); occupancy keeps the HBM busy.
// PQ: one keep-bitset per query, as in scan_gemv_kernel.
template <int NCH, int BQ, int RI, bool NT, bool FULL, bool PQ>
__global__ __launch_bounds__(256) void scan_bf16_kernel(const Bf16ScanParams p) {
    constexpr int NV = RI * BQ;
    constexpr int LPV = 64 / NV;
    const int lane = threadIdx.x & 63;
    const uint32_t n = p.n, dim = p.dim;

    uint32_t coff[NCH];
    f4 qa[BQ][NCH], qb[BQ][NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t idx = (uint32_t)c * 512u + (uint32_t)lane * 8u;
        const bool in = FULL || idx < dim;
        coff[c] = in ? idx : dim - 8u;
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            const float* qp = p.q + (size_t)((uint32_t)b < p.nq ? b : 0) * dim + coff[c];
            const f4 va = *(const f4*)qp, vb = *(const f4*)(qp + 4);
            qa[b][c] = in ? va : (f4)(0.f);
            qb[b][c] = in ? vb : (f4)(0.f);
        }
    }

    const uint32_t last = n - 1u;
    const uint32_t nwords = (n + 31u) / 32u;
    const uint32_t n_tasks = p.n_tasks;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t total_waves = gridDim.x * wpb;
    const uint32_t wave_id = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + (threadIdx.x >> 6)));
    const bool use_queue = n_tasks > total_waves;
    const uint32_t zero = opaque_zero();   // (keeps the dequeue a plain returning atomic)

    const char* const rows_b = (const char*)p.rows;
    const uint32_t row_bytes = dim * 2u;
    auto load_rows = [&](uint32_t base, int j, u4 (&x)[RI][NCH]) {
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            uint32_t row = base + (uint32_t)(RI * j + r);
            row = row > last ? last : row;
            const char* rp = rows_b + (uint64_t)row * row_bytes;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const u4* src = (const u4*)(rp + coff[c] * 2u);
                if (NT) x[r][c] = __builtin_nontemporal_load(src);
                else x[r][c] = *src;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto reduce_rows = [&](int j, u4 (&x)[RI][NCH], float (&sc)[BQ]) {
        f2 acc2[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc2[i] = (f2)(0.f);
#pragma unroll
        for (int r = 0; r < RI; ++r)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const u4 w = x[r][c];
                const f2 x0 = {bf_lo(w.x), bf_hi(w.x)}, x1 = {bf_lo(w.y), bf_hi(w.y)};
                const f2 x2 = {bf_lo(w.z), bf_hi(w.z)}, x3 = {bf_lo(w.w), bf_hi(w.w)};
#pragma unroll
                for (int b = 0; b < BQ; ++b) {
                    f2 a = acc2[b * RI + r];
                    a = __builtin_elementwise_fma(x0, __builtin_shufflevector(qa[b][c], qa[b][c], 0, 1), a);
                    a = __builtin_elementwise_fma(x1, __builtin_shufflevector(qa[b][c], qa[b][c], 2, 3), a);
                    a = __builtin_elementwise_fma(x2, __builtin_shufflevector(qb[b][c], qb[b][c], 0, 1), a);
                    a = __builtin_elementwise_fma(x3, __builtin_shufflevector(qb[b][c], qb[b][c], 2, 3), a);
                    acc2[b * RI + r] = a;
                }
            }
        float acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = acc2[i].x + acc2[i].y;
        treduce<NV>(acc, lane);
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            const float t = __shfl(acc[0], (b * RI + (lane % RI)) * LPV, 64);
            if (lane / RI == j) sc[b] = t;
        }
    };
    uint64_t qmask[PQ ? BQ : 1];   // PQ: the rows of the task each query keeps (task_mask)
    // The f32 epilogue's drop rules, made one-sided: a row is dropped only if its exact score is dropped too.  No clamp on
    // the stored score (bin_of clamps; the select only needs a monotone map).
    auto epilogue = [&](uint32_t cur, uint32_t base, uint32_t trows, uint64_t mask, float (&sc)[BQ]) {
        const uint32_t row = base + (uint32_t)lane;
        const bool live_all = (uint32_t)lane < trows && ((mask >> lane) & 1ull);
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            const bool live = PQ ? (uint32_t)lane < trows && ((qmask[PQ ? b : 0] >> lane) & 1ull) : live_all;
            float s = sc[b];
            if (!live || !(__builtin_fabsf(s) <= 3.4028234664e38f)) s = -INFINITY;
            else if (p.mode == 1u && (uint32_t)b < p.nq) {
                // s <= s~ + B_q, rounding is monotone and the clamp too: clamp(s) >= thr implies clamp(s~ + B_q) >= thr
                float t = s + p.bq[b];
                t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
                if (!(t >= p.thr)) s = -INFINITY;
            }
            if ((uint32_t)b >= p.nq) continue;
            if ((uint32_t)lane < trows && row < p.n_pad) p.scores[(size_t)b * p.n_pad + row] = s;
            const float gm = wave_max64(s);
            if (lane == 0) p.gmax[(size_t)b * n_tasks + cur] = gm;
            if (p.gaux) {
                const uint32_t arg = (uint32_t)__builtin_ctzll(__ballot(s == gm));
                const float sec = wave_max64(((uint32_t)lane == arg) ? -INFINITY : s);
                if (lane == 0) p.gaux[(size_t)b * n_tasks + cur] = ((uint64_t)arg << 32) | (uint64_t)__float_as_uint(sec);
            }
        }
    };
    auto task_mask = [&](uint32_t base, uint32_t trows) -> uint64_t {
        const uint64_t all = trows == 64u ? ~0ull : ((1ull << trows) - 1ull);
        uint64_t mask = all;
        if (base + trows > n) mask = (base >= n) ? 0ull : (all >> (trows - (n - base)));
        if constexpr (PQ) {   // (scan_gemv_kernel's: read what any query of the pass keeps, qmask[b] = what query b keeps)
            const uint32_t w = base / 32u;
            uint64_t any = 0ull;
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                uint64_t m = 0ull;
                if ((uint32_t)b < p.nq) {
                    // (constant address space: nothing writes the table during the launch, so the uniform address is
                    // enough for scalar loads; the shared bitset's plain loads are vector loads behind the row stores)
                    const kc32* kp = (const kc32*)(p.keep + (size_t)p.slot[b] * p.keep_stride);
                    const uint32_t w0 = (w < nwords) ? kp[w] : 0u;
                    const uint32_t w1 = (w + 1u < nwords) ? kp[w + 1u] : 0u;
                    m = mask & ((((uint64_t)w1 << 32) | (uint64_t)w0) >> (base & 31u));
                }
                const uint32_t mlo = __builtin_amdgcn_readfirstlane((uint32_t)m);
                const uint32_t mhi = __builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
                qmask[b] = ((uint64_t)mhi << 32) | mlo;
                any |= qmask[b];
            }
            return any;
        }
        if (p.keep) {
            const uint32_t w = base / 32u;
            const uint32_t w0 = (w < nwords) ? p.keep[w] : 0u;
            const uint32_t w1 = (w + 1u < nwords) ? p.keep[w + 1u] : 0u;
            mask &= (((uint64_t)w1 << 32) | (uint64_t)w0) >> (base & 31u);
        }
        const uint32_t mlo = __builtin_amdgcn_readfirstlane((uint32_t)mask);
        const uint32_t mhi = __builtin_amdgcn_readfirstlane((uint32_t)(mask >> 32));
        return ((uint64_t)mhi << 32) | mlo;
    };

    u4 x[RI][NCH];
    uint32_t cur = wave_id;
    while (cur < n_tasks) {
        uint32_t trows;
        const uint32_t base = p.tiers.locate(cur, trows);
        const uint64_t mask = task_mask(base, trows);
        uint32_t ticket = 0;
        if (use_queue && lane == 0) ticket = atomicAdd(p.work + zero, 1u);
        float sc[BQ];
#pragma unroll
        for (int b = 0; b < BQ; ++b) sc[b] = -INFINITY;
        const int nb = (int)(trows / (uint32_t)RI);
        for (int j = 0; j < nb; ++j) {
            const uint32_t m = (uint32_t)(mask >> (RI * j)) & ((1u << RI) - 1u);
            if (m == 0u) continue;   // all RI rows filtered out / past the end: skip their reads
            load_rows(base, j, x);
            reduce_rows(j, x, sc);
        }
        epilogue(cur, base, trows, mask, sc);
        cur = use_queue ? total_waves + (uint32_t)__builtin_amdgcn_readfirstlane(ticket) : n_tasks;
    }
}

#ifndef CQS_BF16_ONE_SHOT
#define CQS_BF16_ONE_SHOT 24u   // one task per wave up to this many tasks per SIMD; beyond: persistent grid + queue
#endif
#ifndef CQS_BF16_BLOCKS_PER_CU
#define CQS_BF16_BLOCKS_PER_CU 2u
#endif

template <int NCH, int BQ, int RI, bool PQ>
static hipError_t launch_bf16(const ScanArgs& a, const uint16_t* shadow, const float* bq, uint32_t q0, uint32_t nq,
                              uint32_t work_slot, hipStream_t st) {
    Bf16ScanParams p;
    fill_gemv_pass(p, a, q0, nq, PQ);
    p.rows = shadow;
    p.work = a.work + work_slot;
    p.bq = bq + q0;
    const bool one_shot = p.n_tasks <= a.n_cu * 4u * CQS_BF16_ONE_SHOT;
    const uint32_t wpb = 4u;
    const uint32_t blocks = one_shot ? (p.n_tasks + wpb - 1u) / wpb : a.n_cu * CQS_BF16_BLOCKS_PER_CU;
    const dim3 grid(blocks), block(64u * wpb);
    const bool full = (a.dim == (uint32_t)NCH * 512u);
    for_nt_full(a.nontemporal, full, [&](auto nt_c, auto full_c) {
        hipLaunchKernelGGL((scan_bf16_kernel<NCH, BQ, RI, decltype(nt_c)::value, decltype(full_c)::value, PQ>), grid, block, 0, st, p);
    });
    return hipGetLastError();
}

template <int NCH, bool PQ>
static hipError_t launch_bf16_groups(const ScanArgs& a, const uint16_t* shadow, const float* bq, hipStream_t st) {
    uint32_t done = 0, slot = 0;
    while (done < a.b) {
        const uint32_t left = a.b - done;
        hipError_t e;
        uint32_t g;
        if constexpr (NCH <= 2) {   // (5..7 queries ride the 8-query pass, as in the f32 scan)
            if (left >= 5) { g = left < 8u ? left : 8u; e = launch_bf16<NCH, 8, 2, PQ>(a, shadow, bq, done, g, slot, st); }
            else if (left >= 4) { g = 4; e = launch_bf16<NCH, 4, 4, PQ>(a, shadow, bq, done, g, slot, st); }
            else if (left >= 2) { g = 2; e = launch_bf16<NCH, 2, 8, PQ>(a, shadow, bq, done, g, slot, st); }
            else { g = 1; e = launch_bf16<NCH, 1, 16, PQ>(a, shadow, bq, done, g, slot, st); }
        } else {
            if (left >= 2) { g = 2; e = launch_bf16<NCH, 2, 4, PQ>(a, shadow, bq, done, g, slot, st); }
            else { g = 1; e = launch_bf16<NCH, 1, 8, PQ>(a, shadow, bq, done, g, slot, st); }
        }
        if (e != hipSuccess) return e;
        done += g;
        slot = (slot + 1u) % kWorkWords;   // (<= 32 queries: at most 32 passes, the heads never wrap)
    }
    return hipSuccess;
}

hipError_t launch_scan_bf16(const ScanArgs& a, const uint16_t* shadow, const float* bq, hipStream_t st) {
    if (a.b == 0 || a.n == 0) return hipSuccess;
    if (a.b > kShadowMaxQ || a.dim % 8u != 0u || a.dim > kShadowMaxDim || a.group_tasks != 1u) return hipErrorInvalidValue;
    if (a.keep_tab && !keep_tab_ok(a)) return hipErrorInvalidValue;
    switch ((a.dim + 511u) / 512u) {
        case 1: return a.keep_tab ? launch_bf16_groups<1, true>(a, shadow, bq, st) : launch_bf16_groups<1, false>(a, shadow, bq, st);
        case 2: return a.keep_tab ? launch_bf16_groups<2, true>(a, shadow, bq, st) : launch_bf16_groups<2, false>(a, shadow, bq, st);
        case 3: return a.keep_tab ? launch_bf16_groups<3, true>(a, shadow, bq, st) : launch_bf16_groups<3, false>(a, shadow, bq, st);
        case 4: return a.keep_tab ? launch_bf16_groups<4, true>(a, shadow, bq, st) : launch_bf16_groups<4, false>(a, shadow, bq, st);
        default: return hipErrorInvalidValue;
    }
}

// ---- select + rescore + certify ---------------------------------------------------------------------------------
struct TailParams {
    const float* rows;
    const float* q;
    uint32_t dim, k, kprime, mode, row_base;
    float thr;
    const float* scores;       // [b, n_pad]   the shadow scan's output (an earlier launch): approximate scores,
    const float* gmax;         // [b, n_groups] maxima of the scan's groups (GroupMap{tiers, group_tasks}),
    const uint64_t* gaux;      // nullable [b, n_groups] (argmax, runner-up)
    uint32_t n_pad;
    TaskTiers tiers;
    uint32_t group_tasks;      // ScanArgs::group_tasks: 1, or 4 behind the int8 scan's workgroup maxima
    uint32_t bins;             // select_body's `linear`
    uint32_t* work;            // [kWorkWords] the scans' work-queue heads: zeroed here, as the select launch did
    uint64_t* ekeys;           // [b, k']: exact key of candidate i, 0 = dropped by the f32 epilogue.  Handed from the
                               // rescoring waves to the finishing workgroup inside the launch (agent-scope accesses only)
    float* bq;                 // [b] B_q; bound != 0: computed here and handed over like ekeys
    uint32_t* tickets;         // [b] arrivals of each query's workgroups: 0 on entry, 0 again on exit
    uint32_t bound;            // 0: bq holds the block's bounds (an earlier launch), 1: the bf16 copy's, 2: the int8 copy's
    double r_max, norm_max;    // of that copy
    uint64_t* out_keys;        // [b, k]
    uint32_t* out_counts;      // [b]
    uint32_t* cert;            // [b]
    unsigned long long* counters;   // nullable [2]: certified, not certified
    unsigned long long* counters2;  // nullable [2]: the same again (the int8 copy's own counts)
    uint32_t prefix;           // 1: the finisher sorts a prefix first (tail_prefix.h), 0: all candidates at once
    unsigned long long* prefix_counts;   // nullable [2]: queries certified on the prefix, queries that went on to sort all
    unsigned long long* dbg;   // CQS_HIP_DEBUG_STAMPS (DBG instantiations only): [0, 16) phase stamps of query 0's tail, and
                               // kDbgTailSlow words further on the slow path's three
    uint32_t first;            // tail_plan_first: tier 1's candidates (implies prefix), 0: no tiers
};

// One launch for a block's tail.  blockIdx.y = query; the query's waves are numbered w = blockIdx.x * 16 + wave and take
// the slots w, w + #waves, ... of 0 .. min(count, lim), lim = k' candidates, or tier 1's j1 (tail_plan.h).
//  every workgroup  the select of its query for the top lim + 1 approximate keys (select_body on the scan's scores / gmax /
//                   gaux, as select_finish_kernel runs it): nobody can wait for a select workgroup, so each does the
//                   select itself.  All of them read the same words an earlier launch wrote and run the same code, so all
//                   hold the same sorted list and nothing is handed between workgroups before the ticket below.
//  slot 0           B_q of the query into bq (bound != 0), beside the rescoring waves, off their path.
//  slot i + 1       candidate i < min(count, lim): its exact f32 score, scan_gemv_kernel's for this (row, query): lane owns
//                   floats [c*256 + lane*4, +4) of chunk c (clamped address and zero query fragment past a partial last
//                   chunk), an (even, odd) packed-FMA chain over the chunks in order, even + odd, then the xor butterfly at
//                   distances 32 -> 1 - the tree treduce builds for every RI x BQ (each node adds the same two partial
//                   sums; IEEE addition commutes) - and that kernel's epilogue.
//  last workgroup   of the query to arrive certifies: top k of the rescored candidates (the select's rank sort) into
//                   out_keys / out_counts, and cert = 1 when no row outside them can enter the top k.
//  workgroup (0, 0) zeroes the work-queue heads for the next scan (visible at the kernel boundary; the scan that advanced
//                   them is an earlier launch).
// Nobody waits for anybody: a workgroup adds one to the query's ticket when its waves have stored, and the one whose add
// returns gridDim.x - 1 knows that every other has.  It puts the ticket back to 0 for the next search.
// Prefix first (p.first = j1 != 0): the select is exact and its keys totally ordered, so the first min(count, j1 + 1) keys of a
// select at j1 + 1 are those of the select at k' + 1.  With j1 + 1 keys returned the finisher holds what the prefix
// certificate reads - candidates 0 .. j1 - 1 rescored and key j1 - and a query it certifies is done at half the slots and a
// select of 161 keys, not 351 (k = 20).  Where it does not certify, the finisher alone goes round again: the select at
// k' + 1, its 16 waves rescore candidates j1 .. nc - 1 into LDS behind the prefix's keys, then one sort and the rules on all
// of them - the verdict the tail without tiers reaches, and still nobody waits.  Fewer than j1 + 1 keys returned: every valid row was a
// candidate and was rescored, rule (a).
// Visibility (per-XCD L2s are not coherent, a CU's L1 is never refreshed): every word handed over (ekeys, bq) is stored
// write-through by an agent-scope atomic store, each wave drains its stores before the workgroup's barrier, one lane then
// adds to the ticket, and the finisher reads those words by agent-scope atomic loads only, after the add has returned and a
// barrier that the adding wave joins.  scores / gmax / gaux come from an earlier launch and are read plainly.
// DBG: phase stamps of query 0's tail (s_memrealtime) into p.dbg: [0, 6) the first select_body's, 6 / 7 first rows issued /
// reduced (lane 0 of workgroup 0's wave 1), 10 workgroup 0's ticket returned, 14 the finisher's, 11 / 12 / 13 the finisher's
// keys listed / sorted (the last sort) / outputs stored; kDbgTailSlow + 0 / 1 / 2 the finisher's prefix refused / second select
// done / remaining rows' keys in LDS.
// TIER is a property of the instantiation, not a branch: without it (p.first == 0: the bf16 copy, CQS_HIP_TAIL_PREFIX=0, the tier
// switched off or ruled out) the kernel holds one select, no slow path, and is the code it was before there were tiers.
template <int NCH, bool DBG, bool TIER>
__global__ __launch_bounds__(1024) void rescore_certify_kernel(const TailParams p) {
    __shared__ uint64_t s_keys[kShadowKMax];
    __shared__ uint64_t s_sorted[kShadowKMax];
    __shared__ __attribute__((aligned(16))) uint32_t s_ok[kShadowKMax + 4];
    __shared__ uint32_t s_cnt, s_flag, s_last;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.y;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t wave = blockIdx.x * kTailWaves + wib;
    const uint32_t n_waves = gridDim.x * kTailWaves;
    const uint32_t dim = p.dim;
    const float* qp = p.q + (size_t)qi * dim;
    unsigned long long* const dbg = DBG && qi == 0u ? p.dbg : nullptr;
#define CQS_TAIL_STAMP(i, who) do { if (DBG && dbg && (who)) dbg[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
    if (threadIdx.x == 0) s_cnt = 0u;
    if (qi == 0u && blockIdx.x == 0u)
        for (uint32_t i = threadIdx.x; i < kWorkWords; i += 1024u) p.work[i] = 0u;
    const GroupMap map{p.tiers, p.group_tasks};
    const uint32_t n_groups = map.total();
    const uint32_t first = TIER ? p.first : 0u;
    uint32_t lim = TIER ? first : p.kprime;   // candidates of this select; it returns one key more where there is one
    uint32_t found, ac, nc;
    uint64_t key_next;
    const uint64_t* akeys;
    // the approximate top lim + 1, sorted: what select_finish_kernel wrote to akeys / acounts when it was a launch of its own
    auto run_select = [&](unsigned long long* stamps) {
        akeys = select_body(p.scores + (size_t)qi * p.n_pad, p.gmax + (size_t)qi * n_groups,
                            p.gaux ? p.gaux + (size_t)qi * n_groups : nullptr, p.n_pad, map, lim + 1u, p.row_base, p.bins,
                            stamps, found);
        found = (uint32_t)__builtin_amdgcn_readfirstlane((int)found);   // (workgroup-uniform: a scalar from here on)
        ac = found < lim + 1u ? found : lim + 1u;
        nc = ac < lim ? ac : lim;
        key_next = ac > lim ? akeys[lim] : 0ull;   // the (lim + 1)-th approximate key (the finisher's)
    };
    run_select(DBG ? dbg : nullptr);

    // top k of the m kept exact keys in s_keys, the outputs, the verdict: what the last workgroup to arrive does
    auto write_out = [&](uint32_t m, bool ok) {
        const uint32_t k = p.k;
        const uint32_t outc = m < k ? m : k;
        for (uint32_t i = threadIdx.x; i < k; i += 1024u) p.out_keys[(size_t)qi * k + i] = (i < outc) ? s_sorted[i] : 0ull;
        if (threadIdx.x == 0) {
            p.out_counts[qi] = outc;
            p.cert[qi] = ok ? 1u : 0u;   // (before the kernel ends: the gated f32 launches that follow read it at entry)
            if (p.counters) atomicAdd(&p.counters[ok ? 0 : 1], 1ull);
            if (p.counters2) atomicAdd(&p.counters2[ok ? 0 : 1], 1ull);
        }
    };
    // the rules on all min(count, k') candidates, m of them kept (ac, key_next: of a select that was asked for k' + 1 keys,
    // or of tier 1's where it returned no more than j1 <= k')
    auto full_verdict = [&](uint32_t m, float bq) {
        bool ok = false;
        if (__builtin_fabsf(bq) <= 3.4028234664e38f) {
            if (ac <= p.kprime) ok = true;   // (a) every row the approximate rules keep was rescored
            else if (m >= p.k) {             // (b) every outsider j: s_j <= s~_j + B_q <= s~_(k'+1) + B_q < s_(k)
                float t = key_score(key_next) + bq;
                if (p.mode == 1u) t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
                ok = t < key_score(s_sorted[p.k - 1u]);
            }
        }
        return ok;
    };

    for (uint32_t slot = wave; slot <= nc; slot += n_waves) {
        if (slot == 0u) {
            if (p.bound != 0u) {
                const float v = p.bound == 2u ? wave_i8_bound(qp, dim, p.r_max, p.norm_max, lane)
                                              : wave_shadow_bound(qp, dim, p.r_max, p.norm_max, lane);
                if (lane == 0u)
                    __hip_atomic_store((uint32_t*)p.bq + qi, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            continue;
        }
        const uint32_t i = slot - 1u;
        const uint64_t key = akeys[i];
        const uint32_t grow = 0xFFFFFFFFu - (uint32_t)key;
        const float* rp = p.rows + (size_t)(grow - p.row_base) * dim;
        // the exact score and scan_gemv_kernel's epilogue: f32_score.h, shared with the one-launch f32 fallback
        f4 x[NCH], qv[NCH];
        if constexpr (TIER) f32_fragments_batched<NCH>(rp, qp, dim, lane, x, qv);
        else f32_fragments<NCH>(rp, qp, dim, lane, x, qv);
        CQS_TAIL_STAMP(6, slot == 1u && threadIdx.x == 64u);
        float s = f32_dot_chain<NCH>(x, qv);
        const bool keep = f32_emit(s, p.mode, p.thr);
        if (lane == 0u)
            __hip_atomic_store(p.ekeys + (size_t)qi * p.kprime + i, keep ? pack_key(okey(s), grow) : 0ull, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        CQS_TAIL_STAMP(7, slot == 1u && threadIdx.x == 64u);
    }
    // hand-off: every wave drains its stores, the barrier, then one lane signals for the workgroup
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = __hip_atomic_fetch_add(p.tickets + qi, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == gridDim.x - 1u;
        if (last) __hip_atomic_store(p.tickets + qi, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // armed for the next search
        s_last = last ? 1u : 0u;
        CQS_TAIL_STAMP(10, blockIdx.x == 0u);
        CQS_TAIL_STAMP(14, last);
    }
    __syncthreads();
    if (s_last == 0u) return;   // (workgroup-uniform) not the last to arrive: done

    // the finisher: every other workgroup of the query has stored, drained and signalled.  The certificate holds for any
    // prefix of the candidates (tail_prefix_first), and the rank sort is quadratic in what it sorts: first the prefix alone;
    // the rest only if the prefix does not certify, and then the rules on all of them.  Tier 1 rescored the prefix alone:
    // it is a proper one whenever the select returned a key past it.
    const uint32_t j1 = p.prefix ? tail_prefix_first(p.k, nc) : nc;
    const bool proper = TIER ? found > first : j1 < nc;   // (workgroup-uniform) candidate j1 is the first row outside the prefix
    if (threadIdx.x < j1) {
        const uint64_t key = __hip_atomic_load(p.ekeys + (size_t)qi * p.kprime + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (key != 0ull) s_keys[atomicAdd(&s_cnt, 1u)] = key;
    }
    __syncthreads();
    CQS_TAIL_STAMP(11, threadIdx.x == 0u);
    uint32_t m = s_cnt;
    float bq = 0.f;   // (asked for ahead of the sort: the prefix's verdict stands between the sort and the outputs)
    if (threadIdx.x == 0) bq = __uint_as_float(__hip_atomic_load((uint32_t*)p.bq + qi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    // a proper prefix is short (6k + 40 keys): all 1024 threads rank it; every candidate at once is the sort it always was
    if (proper) rank_sort_keys_wide(s_keys, m, s_sorted, s_ok, &s_flag);
    else rank_sort_keys(s_keys, m, s_sorted, s_ok, &s_flag);
    if (proper) {
        if (threadIdx.x == 0) {
            bool ok = false;
            if (__builtin_fabsf(bq) <= 3.4028234664e38f && m >= p.k)
                ok = tail_prefix_certifies(akeys[j1], bq, p.mode, key_score(s_sorted[p.k - 1u]));
            s_last = ok ? 2u : 1u;
            if (p.prefix_counts) atomicAdd(&p.prefix_counts[ok ? 0 : 1], 1ull);
        }
        __syncthreads();
        if (s_last == 2u) {
            CQS_TAIL_STAMP(12, threadIdx.x == 0u);
            write_out(m, true);
            CQS_TAIL_STAMP(13, threadIdx.x == 0u);
            return;
        }
        if constexpr (!TIER) {   // the other workgroups rescored the rest too
            if (threadIdx.x >= j1 && threadIdx.x < nc) {
                const uint64_t key = __hip_atomic_load(p.ekeys + (size_t)qi * p.kprime + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (key != 0ull) s_keys[atomicAdd(&s_cnt, 1u)] = key;
            }
        } else {
            // the slow path, this workgroup alone: the whole select, then candidates first .. nc - 1, a wave taking kRU
            // neighbours at a time with their loads in flight together (kRU * NCH + NCH f4 registers per lane; only NCH = 3 was
            // timed).  The kept keys go behind the prefix's in s_keys, which the sort left as they were.
            CQS_TAIL_STAMP(kDbgTailSlow + 0u, threadIdx.x == 0u);
            lim = p.kprime;
            run_select(nullptr);
            CQS_TAIL_STAMP(kDbgTailSlow + 1u, threadIdx.x == 0u);
            constexpr int kRU = NCH <= 3 ? 4 : (NCH <= 4 ? 3 : (NCH <= 6 ? 2 : 1));
            f4 qv[NCH];
            f32_query_fragments<NCH>(qp, dim, lane, qv);
            for (uint32_t i0 = first + wib * (uint32_t)kRU; i0 < nc; i0 += kTailWaves * (uint32_t)kRU) {
                f4 x[kRU][NCH];
                uint32_t grow[kRU];
#pragma unroll
                for (int u = 0; u < kRU; ++u) {
                    const uint32_t i = i0 + (uint32_t)u < nc ? i0 + (uint32_t)u : nc - 1u;
                    grow[u] = 0xFFFFFFFFu - (uint32_t)akeys[i];
                    f32_row_fragments<NCH>(p.rows + (size_t)(grow[u] - p.row_base) * dim, dim, lane, x[u]);
                }
                __builtin_amdgcn_sched_barrier(0);   // (the kRU rows' loads are issued before the first is waited for)
#pragma unroll
                for (int u = 0; u < kRU; ++u) {
                    float s = f32_dot_chain<NCH>(x[u], qv);
                    const bool keep = f32_emit(s, p.mode, p.thr);
                    if (lane == 0u && i0 + (uint32_t)u < nc && keep) s_keys[atomicAdd(&s_cnt, 1u)] = pack_key(okey(s), grow[u]);
                }
            }
        }
        __syncthreads();
        if constexpr (TIER) CQS_TAIL_STAMP(kDbgTailSlow + 2u, threadIdx.x == 0u);
        m = s_cnt;
        rank_sort_keys(s_keys, m, s_sorted, s_ok, &s_flag);
    }
    CQS_TAIL_STAMP(12, threadIdx.x == 0u);
    bool ok = false;
    if (threadIdx.x == 0) ok = full_verdict(m, bq);
    write_out(m, ok);
    CQS_TAIL_STAMP(13, threadIdx.x == 0u);
#undef CQS_TAIL_STAMP
}

#ifndef CQS_TAIL_MAX_BLOCKS_PER_CU
#define CQS_TAIL_MAX_BLOCKS_PER_CU 1u   // the select's LDS leaves room for one workgroup per CU: the grid stays one round
#endif

template <int NCH>
static void launch_tail(dim3 grid, dim3 block, hipStream_t st, const TailParams& tp) {
    if (tp.first != 0u) {
        if (tp.dbg) hipLaunchKernelGGL((rescore_certify_kernel<NCH, true, true>), grid, block, 0, st, tp);
        else hipLaunchKernelGGL((rescore_certify_kernel<NCH, false, true>), grid, block, 0, st, tp);
    } else {
        if (tp.dbg) hipLaunchKernelGGL((rescore_certify_kernel<NCH, true, false>), grid, block, 0, st, tp);
        else hipLaunchKernelGGL((rescore_certify_kernel<NCH, false, false>), grid, block, 0, st, tp);
    }
}

hipError_t launch_rescore_certify(const ScanArgs& a, uint32_t row_base, uint32_t k, uint32_t kprime, uint32_t bound,
                                  double r_max, double norm_max, float* bq, uint32_t* tickets, uint64_t* ekeys,
                                  uint64_t* out_keys, uint32_t* out_counts, uint32_t* cert, unsigned long long* counters,
                                  unsigned long long* counters2, bool prefix, bool prefix_first, unsigned long long* prefix_counts,
                                  unsigned long long* dbg, hipStream_t st) {
    const uint32_t b = a.b, dim = a.dim;
    if (b == 0) return hipSuccess;
    if (b > kShadowMaxQ || k == 0 || kprime < k || kprime >= kShadowKMax || a.k != kprime + 1u || dim % 8u != 0u ||
        dim > kShadowMaxDim || bound > 2u || (a.group_tasks != 1u && a.group_tasks != kMaxGroupTasks))
        return hipErrorInvalidValue;
    const uint32_t first = tail_plan_first(k, kprime, prefix, prefix_first);
    const TailParams tp{a.rows, a.q, dim, k, kprime, a.mode, row_base, a.threshold, a.scores, a.gmax, a.gaux, a.n_pad, a.tiers, a.group_tasks,
                        a.range_bins ? 2u : (a.linear_bins ? 1u : 0u), a.work, ekeys, bq, tickets, bound, r_max, norm_max,
                        out_keys, out_counts, cert, counters, counters2, prefix ? 1u : 0u, prefix_counts, dbg, first};
    // One wave per slot (B_q + the candidates of the first select: tier 1's, or k') while the block's workgroups fit the
    // device in one round; beyond that (b * ceil((k' + 1) / 16) > CUs: from b = 4 at k = 500) fewer workgroups whose waves
    // take several slots each, because every workgroup repeats the select's front end and a second round would repeat it
    // behind the first.
    const dim3 grid(tail_plan_workgroups(tail_plan_slots(kprime, first), b, a.n_cu, CQS_TAIL_MAX_BLOCKS_PER_CU), b), block(64u * kTailWaves);
    switch ((dim + 255u) / 256u) {
        case 1: launch_tail<1>(grid, block, st, tp); break;
        case 2: launch_tail<2>(grid, block, st, tp); break;
        case 3: launch_tail<3>(grid, block, st, tp); break;
        case 4: launch_tail<4>(grid, block, st, tp); break;
        case 5: launch_tail<5>(grid, block, st, tp); break;
        case 6: launch_tail<6>(grid, block, st, tp); break;
        case 7: launch_tail<7>(grid, block, st, tp); break;
        case 8: launch_tail<8>(grid, block, st, tp); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace cqs
