// scan_kernels.hip — gfx950 (MI355X) kernels for the cqs brute-force scan.
//
//  scan_gemv_kernel   HBM-streaming fp32 dot of every corpus row with 1..8 queries.
//                     One wave = one task of 64 (32, 16) rows; up to ~1.5M rows every task gets
//                     its own wave and the hardware dispatcher does the scheduling, beyond that
//                     a persistent grid continues from a global work queue.  A row is read as
//                     dim/256 fully coalesced 1-KiB wave loads (16 B/lane) issued 8 rows at a
//                     time, double-buffered; the query lives in registers; lane partials are
//                     reduced with a transposed butterfly so that RI rows x BQ queries cost ~1
//                     cross-lane op per dot.  Besides the score row it emits one maximum per
//                     task: the pruning index of the top-k select.
//                     Replaces the per-row simsimd dot of the reference's brute-force loop
//                     (src/math.rs:11-28 called from src/search/query.rs:469-481) and
//                     cuVS' search for the exact backend (src/cagra.rs:605).
//  select_finish      exact top-k in ONE workgroup per query: threshold bin from the group-
//                     maxima histogram -> the few groups that can hold a top-k entry ->
//                     their scores -> bitonic sort (exact one-block radix fallback for ties).
//                     Replaces BoundedScoreHeap (candidate.rs:162-330): same comparator
//                     (score desc under total order, id asc) on a packed 64-bit key.
//
// Wave = 64 lanes.  gfx950 only.
#include "scan_kernels.h"
#include "launch_util.h"
#include "scan_gemv_device.h"
#include "select_device.h"

namespace cqs {


// ---- scan ------------------------------------------------------------------
struct ScanParams {
    const float* rows;
    uint32_t n, n_pad, dim;
    const float* q;
    float* scores;
    const uint32_t* keep;
    uint32_t mode;
    float thr;
    uint32_t nq;        // queries actually present (<= BQ: the pass may be padded; extra slots are never stored)
    uint32_t* work;     // work-queue head of this launch
    TaskTiers tiers;    // task t -> (first row, 64 / 32 / 16 rows)
    uint32_t n_tasks;   // tiers.total()
    float* gmax;        // [BQ][n_tasks] maximum valid score of each task's rows (-inf if none)
    uint64_t* gaux;     // nullable, [BQ][n_tasks]: (lane of that maximum << 32) | bits of the largest score of the task's OTHER rows
    unsigned long long* dbg;  // CQS_HIP_DEBUG_STAMPS: [16 + 2*wave] = start / end realtime of each wave
    const uint32_t* gate;     // nullable, [gate_n]: skip the launch when all are 1 (ScanArgs::gate)
    uint32_t gate_n;
    uint32_t keep_stride;     // PQ: `keep` is a table of bitsets, this many words per row ...
    uint8_t slot[kMaxGemvQ];  // ... and query b of the pass is filtered by row slot[b] (ScanArgs::keep_tab)
};

// NCH = ceil(dim / 256): 1-KiB chunks per row.  BQ queries, RI rows per batch (RI*BQ partial
// sums are reduced together).  FULL: dim == NCH*256.
// PIPE: 0 = batch by batch: loads -> math (many-query variants: the register file is full of query
//           fragments); 1 = two batches in flight while a third is reduced (tasks whose rows are partly
//           filtered out still go batch by batch, skipping the empty ones).
// OCC:  workgroups per CU the register allocation must leave room for.  The pipelined single-query
//       variant wants > 256 VGPRs (one wave per SIMD); corpora with fewer tasks than 2 waves per SIMD
//       use an OCC = 2 build instead so that every task is resident at once.
// PQ:   one keep-bitset per query (ScanParams::slot).  A batch is read when ANY query of the pass keeps one of its rows, the
//       pipelined path runs when together they keep the whole task; each query's own mask decides, in the epilogue, which
//       rows it scores.  Every mask is wave-uniform and lives in a scalar register pair.  The arithmetic is untouched: a
//       query's scores are those of a pass of its own with its bitset shared.
template <int NCH, int BQ, int RI, bool NT, bool FULL, int PIPE, int OCC, bool PQ>
__global__ __launch_bounds__(256, OCC) void scan_gemv_kernel(const ScanParams p) {
    if (p.gate && gate_closed(p.gate, p.gate_n)) return;   // the bf16 shadow certified the block (before any load or dequeue)
    constexpr int NV = RI * BQ;
    constexpr int LPV = 64 / NV;  // lanes per reduced value
    const int lane = threadIdx.x & 63;
    const uint32_t n = p.n, dim = p.dim;

    // per-lane column offsets: lane owns floats [c*256 + lane*4, +4) of every chunk c.
    // A partial last chunk is read from a clamped in-row address against a zero query
    // fragment, so the row loads stay unconditional (no branch, no early wait).
    uint32_t coff[NCH];
    f4 qv[BQ][NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t idx = (uint32_t)c * 256u + (uint32_t)lane * 4u;
        const bool in = FULL || idx < dim;
        coff[c] = in ? idx : dim - 4u;
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            const f4 v = *(const f4*)(p.q + (size_t)((uint32_t)b < p.nq ? b : 0) * dim + coff[c]);
            qv[b][c] = in ? v : (f4)(0.f);
        }
    }

    const uint32_t last = n - 1u;
    const uint32_t nwords = (n + 31u) / 32u;
    const uint32_t n_tasks = p.n_tasks;
    const uint32_t wpb = blockDim.x >> 6;  // waves per workgroup
    const uint32_t total_waves = gridDim.x * wpb;
    // (readfirstlane: tell the compiler the wave index - and every task index derived from it - is uniform)
    const uint32_t wave_id = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + (threadIdx.x >> 6)));
    // A wave's first task is its own index (no atomic).  A one-shot grid covers every task that way and
    // the hardware dispatcher does the scheduling; a persistent grid (huge corpora) continues from the
    // shared queue, whose tickets count from #waves.  (One queue word sustains only ~88 dequeues/us: a
    // start-up burst from every wave would cost 10-25 us.)
    const bool use_queue = n_tasks > total_waves;
    const uint32_t zero = opaque_zero();   // (keeps the dequeue a plain returning atomic)
    if (p.dbg && lane == 0 && wave_id < kDbgWaves) p.dbg[16u + 2u * wave_id] = __builtin_amdgcn_s_memrealtime();

    // issue the RI*NCH row loads of batch j of the task at `base` back to back (all in flight together).
    // Address = uniform row pointer (SGPR pair, scalar ALU) + the lane's fixed 32-bit byte offset (+ the
    // chunk as an immediate): no per-row vector address registers.
    const char* const rows_b = (const char*)p.rows;
    const uint32_t row_bytes = dim * 4u;
    uint32_t lane_off[NCH];  // FULL: only [0] is used, chunks go into the immediate offset
#pragma unroll
    for (int c = 0; c < NCH; ++c) lane_off[c] = coff[c] * 4u;
    auto load_rows = [&](uint32_t base, int j, f4 (&x)[RI][NCH]) {
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            uint32_t row = base + (uint32_t)(RI * j + r);
            row = row > last ? last : row;
            const char* rp = rows_b + (uint64_t)row * row_bytes;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const f4* src = FULL ? (const f4*)(rp + lane_off[0]) + c * 64 : (const f4*)(rp + lane_off[c]);
                if (NT) x[r][c] = __builtin_nontemporal_load(src);
                else x[r][c] = *src;
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the math that follows
    };
    // dot the batch with the queries; lane L = RI*j + r receives row r's score of query b in sc[b]
    auto reduce_rows = [&](int j, f4 (&x)[RI][NCH], float (&sc)[BQ]) {
        // packed f32 math (v_pk_fma_f32: two FMAs per instruction): every dot product keeps an (even, odd)
        // pair of partial sums over the lane's float pairs, folded once per batch
        f2 acc2[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc2[i] = (f2)(0.f);
#pragma unroll
        for (int r = 0; r < RI; ++r)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const f2 xlo = __builtin_shufflevector(x[r][c], x[r][c], 0, 1);
                const f2 xhi = __builtin_shufflevector(x[r][c], x[r][c], 2, 3);
#pragma unroll
                for (int b = 0; b < BQ; ++b) {
                    f2 a = acc2[b * RI + r];
                    a = __builtin_elementwise_fma(xlo, __builtin_shufflevector(qv[b][c], qv[b][c], 0, 1), a);
                    a = __builtin_elementwise_fma(xhi, __builtin_shufflevector(qv[b][c], qv[b][c], 2, 3), a);
                    acc2[b * RI + r] = a;
                }
            }
        float acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = acc2[i].x + acc2[i].y;
        treduce<NV>(acc, lane);
        // value (b, r) now sits in lanes [(b*RI+r)*LPV, +LPV); lane L = RI*j + r wants it
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            const float t = __shfl(acc[0], (b * RI + (lane % RI)) * LPV, 64);
            if (lane / RI == j) sc[b] = t;
        }
    };

    uint64_t qmask[PQ ? BQ : 1];   // PQ: the rows of the current task each query keeps (task_mask)
    // emit the scores of task `cur` (lane <-> row base+lane, lanes < trows): one coalesced store per
    // query and the task maximum for the select's pruning index
    auto epilogue = [&](uint32_t cur, uint32_t base, uint32_t trows, uint64_t mask, float (&sc)[BQ]) {
        const uint32_t row = base + (uint32_t)lane;
        bool live = (uint32_t)lane < trows && ((mask >> lane) & 1ull);
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            float s = sc[b];
            if constexpr (PQ) live = (uint32_t)lane < trows && ((qmask[b] >> lane) & 1ull);
            // non-finite scores are never emitted (src/math.rs:23-27, src/cagra.rs:649-651)
            if (!live || !(__builtin_fabsf(s) <= 3.4028234664e38f)) s = -INFINITY;
            else if (p.mode == 1u) {
                // candidate.rs:550 clamp(0,1) (Rust clamp keeps -0.0), :513-519 `>= threshold`
                s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
                if (!(s >= p.thr)) s = -INFINITY;
            }
            if ((uint32_t)b >= p.nq) continue;  // padding slot of a 5..7-query pass
            if ((uint32_t)lane < trows && row < p.n_pad) p.scores[(size_t)b * p.n_pad + row] = s;
            const float gm = wave_max64(s);
            if (lane == 0) p.gmax[(size_t)b * n_tasks + cur] = gm;
            if (p.gaux) {
                // Round 5: WHERE the maximum sits and the best score among the task's other rows.  A task whose runner-up
                // is below the select's threshold contributes exactly one candidate - (gm, base + arg) - without its score
                // row being read back (select_finish_kernel: 500 x 256 B of gather through ONE CU were 11 of its 28 us).
                // Rows tied at the maximum: only lane `arg` is masked, so the runner-up equals gm and the task is read.
                const uint32_t arg = (uint32_t)__builtin_ctzll(__ballot(s == gm));   // (no valid row: gm = -inf, every lane matches)
                const float sec = wave_max64(((uint32_t)lane == arg) ? -INFINITY : s);
                if (lane == 0) p.gaux[(size_t)b * n_tasks + cur] = ((uint64_t)arg << 32) | (uint64_t)__float_as_uint(sec);
            }
        }
    };
    // ticket -> task index
    auto claimed = [&](uint32_t ticket) -> uint32_t {
        return use_queue ? total_waves + (uint32_t)__builtin_amdgcn_readfirstlane(ticket) : n_tasks;
    };

    // wave-uniform mask of the rows of a task this wave must score: inside the corpus, kept by the filter
    // (PQ: by the filter of at least one query of the pass; qmask[b] = the rows query b keeps, none for a padding slot)
    auto task_mask = [&](uint32_t base, uint32_t trows) -> uint64_t {
        const uint64_t all = trows == 64u ? ~0ull : ((1ull << trows) - 1ull);
        uint64_t mask = all;
        if (base + trows > n) mask = (base >= n) ? 0ull : (all >> (trows - (n - base)));
        if constexpr (PQ) {
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
        // uniform by construction; tell the compiler so the loop branches become scalar
        const uint32_t mlo = __builtin_amdgcn_readfirstlane((uint32_t)mask);
        const uint32_t mhi = __builtin_amdgcn_readfirstlane((uint32_t)(mask >> 32));
        return ((uint64_t)mhi << 32) | mlo;
    };
    f4 xa[RI][NCH], xb[RI][NCH];
    // batch by batch, skipping batches with no row to score
    auto sparse_task = [&](uint32_t t, uint32_t base, uint32_t trows, uint64_t mask) {
        float sc[BQ];
#pragma unroll
        for (int b = 0; b < BQ; ++b) sc[b] = -INFINITY;
        const int nb = (int)(trows / (uint32_t)RI);
        for (int j = 0; j < nb; ++j) {
            const uint32_t m = (uint32_t)(mask >> (RI * j)) & ((1u << RI) - 1u);
            if (m == 0u) continue;  // all RI rows filtered out / past the end: skip their HBM reads
            load_rows(base, j, xb);
            reduce_rows(j, xb, sc);
        }
        epilogue(t, base, trows, mask, sc);
    };

    uint32_t cur = wave_id;
    while (cur < n_tasks) {
        uint32_t trows;
        const uint32_t base = p.tiers.locate(cur, trows);
        const uint64_t mask = task_mask(base, trows);
        const uint64_t all = trows == 64u ? ~0ull : ((1ull << trows) - 1ull);
        uint32_t ticket = 0;  // lane 0: the dequeue drawn during this task
        if (PIPE == 1 && mask == all) {
            float sc[BQ];
#pragma unroll
            for (int b = 0; b < BQ; ++b) sc[b] = -INFINITY;
            const int steps = (int)(trows / (2u * (uint32_t)RI));
            load_rows(base, 0, xa);
            for (int s = 0; s < steps; ++s) {
                load_rows(base, 2 * s + 1, xb);
                // the dequeue goes out behind row loads already in flight: vmcnt retires in issue
                // order, so an atomic issued ahead of them would stall the first reduction
                if (s == 0 && use_queue && lane == 0) ticket = atomicAdd(p.work + zero, 1u);
                reduce_rows(2 * s, xa, sc);
                if (s + 1 < steps) load_rows(base, 2 * s + 2, xa);
                reduce_rows(2 * s + 1, xb, sc);
            }
            epilogue(cur, base, trows, mask, sc);
        } else {
            if (use_queue && lane == 0) ticket = atomicAdd(p.work + zero, 1u);
            sparse_task(cur, base, trows, mask);
        }
        cur = claimed(ticket);
    }
    if (p.dbg && lane == 0 && wave_id < kDbgWaves) p.dbg[17u + 2u * wave_id] = __builtin_amdgcn_s_memrealtime();
}

// ---- select: one workgroup per query (the body: select_device.h) ---------------
__global__ __launch_bounds__(1024) void select_finish_kernel(const float* __restrict__ scores,
                                                             const float* __restrict__ gmax,
                                                             const uint64_t* __restrict__ gaux, uint32_t n_pad,
                                                             const TaskTiers tiers, uint32_t slot_log2, uint32_t k,
                                                             uint32_t row_base, uint32_t linear,
                                                             uint64_t* __restrict__ out_keys,
                                                             uint32_t* __restrict__ out_counts,
                                                             uint32_t* __restrict__ work,
                                                             unsigned long long* __restrict__ dbg,
                                                             const uint32_t* __restrict__ gate, uint32_t gate_n) {
    if (gate && gate_closed(gate, gate_n)) return;   // (same words, same decision as the gated scan; before any barrier)
    const uint32_t qi = blockIdx.x;
    const uint32_t n_tasks = tiers.total();
    uint32_t count;
    const uint64_t* sorted = select_body(scores + (size_t)qi * n_pad, gmax + (size_t)qi * n_tasks,
                                         gaux ? gaux + (size_t)qi * n_tasks : nullptr, n_pad, GroupMap{tiers, 1u}, k, row_base, linear, dbg,
                                         count);
    const uint32_t outc = count < k ? count : k;
    for (uint32_t i = threadIdx.x; i < k; i += 1024u) out_keys[(size_t)qi * k + i] = (i < outc) ? sorted[i] : 0ull;
    if (threadIdx.x == 0) out_counts[qi] = outc;
    // re-arm the scan work-queue heads for the next search (visible at the kernel boundary)
    if (qi == 0) for (uint32_t i = threadIdx.x; i < kWorkWords; i += 1024u) work[i] = 0u;
    if (dbg && threadIdx.x == 0 && blockIdx.x == 0) dbg[6] = __builtin_amdgcn_s_memrealtime();
}

// ---- launchers -------------------------------------------------------------
// dim <= 2048: up to 8 chunks per row, 1..8 queries per pass.  2052..4096 (the reference's presets reach 2560 and 4096,
// src/embedder/models.rs:515,572): 9..16 chunks per row - a row is 9..16 KiB, so ONE row per batch already keeps as many
// bytes in flight as eight 768-d rows; one query per pass (16 chunks x 4 registers of query + two row buffers = 192 VGPRs).
bool scan_dim_supported(uint32_t dim) { return dim >= 4 && dim % 4 == 0 && dim <= 4096; }

#ifndef CQS_SCAN_PIPE
#define CQS_SCAN_PIPE 1
#endif
#ifndef CQS_SCAN_RI1
#define CQS_SCAN_RI1 8   // rows per batch of the single-query scan
#endif
#ifndef CQS_SCAN_CAP_OCCUPANCY
#define CQS_SCAN_CAP_OCCUPANCY 1
#endif
#ifndef CQS_SCAN_ONE_SHOT
#define CQS_SCAN_ONE_SHOT 24u   // one task per wave up to this many tasks per SIMD; beyond: persistent grid + queue
#endif
#ifndef CQS_SCAN_BLOCK_WAVES
#define CQS_SCAN_BLOCK_WAVES 2u   // waves per workgroup of the one-shot launch (64-row tasks)
#endif
#ifndef CQS_SCAN_BLOCK_WAVES_SMALL
#define CQS_SCAN_BLOCK_WAVES_SMALL 1u   // ... of 16-row tasks
#endif
#ifndef CQS_SCAN_BLOCKS_PER_CU
#define CQS_SCAN_BLOCKS_PER_CU 2u   // persistent grid
#endif

static uint32_t tier_slot_log2(const TaskTiers& t) { return t.nA ? 6u : (t.nB ? 5u : 4u); }

template <int NCH, int BQ, int RI, bool PQ>
static hipError_t launch_gemv(const ScanArgs& a, uint32_t q0, uint32_t nq, uint32_t work_slot, hipStream_t st) {
    constexpr int PIPE = (BQ <= 2) ? CQS_SCAN_PIPE : 0;
    ScanParams p;
    fill_gemv_pass(p, a, q0, nq, PQ);
    p.rows = a.rows;
    p.work = a.work + work_slot;
    p.dbg = (unsigned long long*)a.dbg;
    p.gate = a.gate;
    p.gate_n = a.b;
    // One-shot grid (one task per wave, the hardware dispatcher schedules: beats a persistent grid up to
    // ~1.5M rows) or, for huge corpora, a persistent grid that continues from the work queue (beats the
    // one-shot grid by 3 % at 10M rows).
    const bool small = a.tiers.nA == 0u && a.tiers.nB == 0u;  // 16-row tasks only
    // A gated launch (the f32 fallback behind a certified shadow search) finds its gate closed in almost every search, and
    // then costs what it takes to dispatch its workgroups: it takes the persistent grid wherever that is the smaller one
    // (1M rows: 256 workgroups instead of 7.8k; an open gate pays the ~4 % the one-shot grid wins at that size).
    const uint32_t wpb1 = small ? CQS_SCAN_BLOCK_WAVES_SMALL : CQS_SCAN_BLOCK_WAVES;
    const uint32_t blocks1 = (p.n_tasks + wpb1 - 1u) / wpb1;
    const uint32_t blocks_p = (PIPE == 1 && CQS_SCAN_CAP_OCCUPANCY) ? a.n_cu   // (one resident workgroup per CU, see below)
                                                                    : a.n_cu * CQS_SCAN_BLOCKS_PER_CU;
    const bool one_shot = p.n_tasks <= a.n_cu * 4u * CQS_SCAN_ONE_SHOT && !(a.gate && blocks1 > blocks_p);
    const uint32_t wpb = one_shot ? wpb1 : 4u, blocks = one_shot ? blocks1 : blocks_p;
    const dim3 grid(blocks), block(64u * wpb);
    // Streaming a corpus far larger than the caches runs best with ONE wave per SIMD (each with two
    // 8-row batches in flight): a second wave per SIMD costs 2-3 % of the HBM rate (DRAM page
    // locality of the extra streams).  The pipelined kernel fits 2 waves per SIMD in registers, so
    // the launch asks for enough (unused) LDS to hold the CU at 4 waves.
    const bool huge = a.n_pad / 64u >= 6u * a.n_cu * 4u;  // >= ~393k rows (mid-size corpora prefer the extra waves)
    const size_t occ_lds = (PIPE == 1 && huge && CQS_SCAN_CAP_OCCUPANCY) ? (wpb == 4u ? 96u : 160u / (4u / wpb) - 16u) * 1024u : 0u;
    const bool full = (a.dim == (uint32_t)NCH * 256u);
#ifdef CQS_SCAN_FORCE_NT
    const bool nt = CQS_SCAN_FORCE_NT;
#else
    const bool nt = a.nontemporal;
#endif
    auto launch = [&](auto nt_c, auto full_c, auto occ_c) -> hipError_t {
        auto kern = scan_gemv_kernel<NCH, BQ, RI, decltype(nt_c)::value, decltype(full_c)::value, PIPE, decltype(occ_c)::value, PQ>;
        if (occ_lds > 64u * 1024u) {
            static DynLdsOnce once;   // per instantiation: the attribute is set once per device, not per launch
            hipError_t e = once.ensure((const void*)kern, occ_lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, block, occ_lds, st, p);
        return hipGetLastError();
    };
    // small corpora never stream past the caches: their OCC = 2 variant is built without nt loads only
    if (small && PIPE == 1) {
        const std::integral_constant<int, 2> occ2;
        return full ? launch(std::false_type{}, std::true_type{}, occ2) : launch(std::false_type{}, std::false_type{}, occ2);
    }
    return for_nt_full(nt, full, [&](auto nt_c, auto full_c) { return launch(nt_c, full_c, std::integral_constant<int, 1>{}); });
}

template <int NCH, bool PQ>
static hipError_t launch_gemv_groups(const ScanArgs& a, hipStream_t st) {
    uint32_t done = 0, slot = 0;
    while (done < a.b) {
        const uint32_t left = a.b - done;
        hipError_t e;
        uint32_t g;
        // register budget ~ 4*NCH*(BQ + RI) + BQ*RI VGPRs: wide rows take fewer queries per pass
        if constexpr (NCH <= 4) {
            // 5..7 queries ride the 8-query pass (0.50 ms at 1M x 768; 4 + 1..3 would be two or three passes)
            if (left >= 5) { g = left < 8u ? left : 8u; e = launch_gemv<NCH, 8, 2, PQ>(a, done, g, slot, st); }
            else if (left >= 4) { g = 4; e = launch_gemv<NCH, 4, 4, PQ>(a, done, g, slot, st); }
            else if (left >= 2) { g = 2; e = launch_gemv<NCH, 2, 4, PQ>(a, done, g, slot, st); }
            else { g = 1; e = launch_gemv<NCH, 1, CQS_SCAN_RI1, PQ>(a, done, g, slot, st); }
        } else if constexpr (NCH <= 8) {
            if (left >= 2) { g = 2; e = launch_gemv<NCH, 2, 2, PQ>(a, done, g, slot, st); }
            else { g = 1; e = launch_gemv<NCH, 1, 2, PQ>(a, done, g, slot, st); }
        } else {
            g = 1; e = launch_gemv<NCH, 1, 1, PQ>(a, done, g, slot, st);
        }
        if (e != hipSuccess) return e;
        done += g;
        slot = (slot + 1u) % kWorkWords;
        if (slot == 0 && done < a.b) {  // queue heads exhausted: recycle them (rare: > 64 launches)
            e = hipMemsetAsync(a.work, 0, kWorkWords * sizeof(uint32_t), st);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_scan(const ScanArgs& a, hipStream_t st) {
    if (a.b == 0 || a.n == 0) return hipSuccess;
    if (a.group_tasks != 1u) return hipErrorInvalidValue;   // (one maximum per task: groups of tasks are the int8 scan's)
    if (a.gate && (a.b > 64u || (!a.gemv_only && use_mfma(a.b, a.dim)))) return hipErrorInvalidValue;   // gemv passes only
    if (!a.gemv_only && use_mfma(a.b, a.dim)) {
        if (a.keep_tab) return hipErrorInvalidValue;   // (per-query bitsets: gemv passes only)
        uint32_t slot = 0;
        for (uint32_t q0 = 0; q0 < a.b; q0 += 256u) {
            const uint32_t nq = (a.b - q0) < 256u ? (a.b - q0) : 256u;
            hipError_t e = launch_scan_mfma(a, q0, nq, slot, st);
            if (e != hipSuccess) return e;
            slot = (slot + 1u) % kWorkWords;
            if (slot == 0 && q0 + 256u < a.b) {
                e = hipMemsetAsync(a.work, 0, kWorkWords * sizeof(uint32_t), st);
                if (e != hipSuccess) return e;
            }
        }
        return hipSuccess;
    }
    const uint32_t nch = (a.dim + 255u) / 256u;
    if (a.keep_tab) {   // one bitset per query: the PQ instantiations (gemv passes only; the matrix-core kernel has none)
        if (!keep_tab_ok(a)) return hipErrorInvalidValue;
        switch (nch) {
#define CQS_PQ_CASE(N) case N: return launch_gemv_groups<N, true>(a, st);
            CQS_PQ_CASE(1) CQS_PQ_CASE(2) CQS_PQ_CASE(3) CQS_PQ_CASE(4) CQS_PQ_CASE(5) CQS_PQ_CASE(6) CQS_PQ_CASE(7) CQS_PQ_CASE(8)
            CQS_PQ_CASE(9) CQS_PQ_CASE(10) CQS_PQ_CASE(11) CQS_PQ_CASE(12) CQS_PQ_CASE(13) CQS_PQ_CASE(14) CQS_PQ_CASE(15) CQS_PQ_CASE(16)
#undef CQS_PQ_CASE
            default: return hipErrorInvalidValue;
        }
    }
    switch (nch) {
        case 1: return launch_gemv_groups<1, false>(a, st);
        case 2: return launch_gemv_groups<2, false>(a, st);
        case 3: return launch_gemv_groups<3, false>(a, st);
        case 4: return launch_gemv_groups<4, false>(a, st);
        case 5: return launch_gemv_groups<5, false>(a, st);
        case 6: return launch_gemv_groups<6, false>(a, st);
        case 7: return launch_gemv_groups<7, false>(a, st);
        case 8: return launch_gemv_groups<8, false>(a, st);
        case 9: return launch_gemv_groups<9, false>(a, st);
        case 10: return launch_gemv_groups<10, false>(a, st);
        case 11: return launch_gemv_groups<11, false>(a, st);
        case 12: return launch_gemv_groups<12, false>(a, st);
        case 13: return launch_gemv_groups<13, false>(a, st);
        case 14: return launch_gemv_groups<14, false>(a, st);
        case 15: return launch_gemv_groups<15, false>(a, st);
        case 16: return launch_gemv_groups<16, false>(a, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_select(const ScanArgs& a, uint32_t row_base, uint64_t* out_keys, uint32_t* out_counts,
                         hipStream_t st) {
    if (a.b == 0 || a.k == 0) return hipSuccess;
    if ((a.gate && a.b > 64u) || a.group_tasks != 1u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_finish_kernel, dim3(a.b), dim3(1024), 0, st, a.scores, a.gmax,
                       (!a.gemv_only && use_mfma(a.b, a.dim)) ? nullptr : a.gaux, a.n_pad,
                       a.tiers, tier_slot_log2(a.tiers), a.k, row_base,
                       a.range_bins ? 2u : (a.linear_bins ? 1u : 0u), out_keys, out_counts, a.work,
                       (unsigned long long*)a.dbg, a.gate, a.b);
    return hipGetLastError();
}

}  // namespace cqs
