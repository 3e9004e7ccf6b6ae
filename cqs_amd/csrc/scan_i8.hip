// scan_i8.hip — gfx950 kernels of the int8 copy of the dense index's shadow (scan_i8.h).
//
//  i8_build_kernel   one wave per f32 row, the row held in registers: scale = max|x_i| / 127, the codes, and the copy's
//                    index-wide error bound R from the stored codes and scale.
//  scan_i8_kernel    HBM-streaming dot of every int8 row with 1..4 f32 queries, times the row's scale: a quarter of the
//                    bytes of scan_gemv_kernel.  scan_bf16_kernel's tasks, score + gmax (+ gaux) layout and one-sided
//                    epilogue, so the unchanged select, rescore and certify follow it; one wave per task at every size.
//                    ScanArgs::group_tasks = 4: the four waves of a workgroup publish ONE (maximum, argmax, runner-up)
//                    triple for their four consecutive tasks (group_map.h), a quarter of the maxima for the select to walk.
//
// Wave = 64 lanes.  gfx950 only.
#include "scan_i8.h"
#include "i8_sweep.h"
#include "launch_util.h"
#include "scan_gemv_device.h"
#include "shadow_build_device.h"

namespace cqs {

// byte i of w as a signed code, converted (exact)
template <int I>
__device__ __forceinline__ float code_f32(uint32_t w) { return (float)(int)(int8_t)(w >> (8 * I)); }

// ---- build ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void i8_build_kernel(const float* __restrict__ rows, int8_t* __restrict__ codes,
                                                       float* __restrict__ scales, uint64_t row0, uint64_t n_rows,
                                                       uint32_t dim, double gamma, unsigned long long* __restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        i8_build_row(rows + (row0 + r) * dim, codes + (row0 + r) * dim, scales + row0 + r, dim, gamma, stats, lane);
    }
}

hipError_t launch_i8_build(const float* rows, int8_t* codes, float* scales, uint64_t row0, uint64_t n_rows, uint32_t dim,
                           double gamma, unsigned long long* stats, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    if (!i8_dim_ok(dim)) return hipErrorInvalidValue;
    const uint64_t blocks = (n_rows + 3u) / 4u;
    hipLaunchKernelGGL(i8_build_kernel, dim3((uint32_t)(blocks < 8192u ? blocks : 8192u)), dim3(256), 0, st, rows, codes,
                       scales, row0, n_rows, dim, gamma, stats);
    return hipGetLastError();
}

// ---- per-query bound ----------------------------------------------------------------------------------------------
// shadow_bound_kernel with the int8 copy's bound function (wave_i8_bound, which the fused rescore + certify kernel shares).
__global__ __launch_bounds__(64) void i8_bound_kernel(const float* __restrict__ q, uint32_t dim, double r_max,
                                                      double norm_max, float* __restrict__ bq) {
    const uint32_t lane = threadIdx.x;
    const float v = wave_i8_bound(q + (size_t)blockIdx.x * dim, dim, r_max, norm_max, lane);
    if (lane == 0) bq[blockIdx.x] = v;
}

hipError_t launch_i8_bound(const float* q, uint32_t b, uint32_t dim, double r_max, double norm_max, float* bq, hipStream_t st) {
    if (b == 0) return hipSuccess;
    if (b > kShadowMaxQ) return hipErrorInvalidValue;
    hipLaunchKernelGGL(i8_bound_kernel, dim3(b), dim3(64), 0, st, q, dim, r_max, norm_max, bq);
    return hipGetLastError();
}

// ---- approximate scan -------------------------------------------------------------------------------------------
struct I8ScanParams {
    const int8_t* rows;     // [n, dim] codes
    const float* scales;    // [n]
    uint32_t n, n_pad, dim;
    const float* q;
    float* scores;
    const uint32_t* keep;
    uint32_t mode;
    float thr;
    uint32_t nq;            // queries present (<= BQ)
    TaskTiers tiers;
    uint32_t n_tasks;
    float* gmax;
    uint64_t* gaux;         // nullable
    const float* bq;        // [nq] B_q of each query of the pass (device)
    uint32_t keep_stride;   // PQ: `keep` is a table of bitsets, this many words per row ...
    uint8_t slot[kMaxGemvQ];// ... and query b of the pass is filtered by row slot[b] (ScanArgs::keep_tab)
    uint32_t group_tasks;   // 1: gmax / gaux hold one entry per task.  kI8BlockWaves: one per workgroup = group of that many
    uint32_t n_groups;      // consecutive tasks (GroupMap{tiers, group_tasks}), and this is their per-query stride
    uint32_t rev;           // 1: workgroup blockIdx.x takes the tasks of workgroup n_wg - 1 - blockIdx.x: the sweep runs
    uint32_t n_wg;          // backwards (i8_sweep.h).  n_wg = ceil(n_tasks / kI8BlockWaves) workgroups
    uint32_t plain_lo, plain_hi;   // NT: workgroups (after the mapping) below plain_lo or from plain_hi on load plainly
};

constexpr uint32_t kI8BlockWaves = 4;   // waves = consecutive tasks of a workgroup (= kMaxGroupTasks: the grouped form's G)
static_assert(kI8BlockWaves == kMaxGroupTasks, "a workgroup of the int8 scan is one group of the select's map");

// NCH = ceil(dim / 1024): 1-KiB chunks per row; lane owns components [c*1024 + lane*16, +16) of chunk c (one 16-byte load).
// A partial last chunk (FULL = false, 768-d: lanes 48..63) reads a clamped in-row address against a zero query fragment, as
// scan_bf16_kernel does: the same quarter of the lane-loads of a 768-d row.  Per lane and chunk: 16 converts and 8 packed
// FMAs, (even, odd) accumulators; the row's scale multiplies the reduced sum once, in the epilogue.
// One task per wave at every size, no persistent grid + work queue: with the queue a search took 0.26 ms against 0.158 at
// 1M rows and 2.11 against 1.24 at 10M - both about 14 ns per dequeued task, whatever the blocks per CU,
// which points at the one returning atomic per task on an address every XCD shares; this scan needs a task every 8 ns.
// PQ: one keep-bitset per query, as in scan_gemv_kernel.
// group_tasks = 4 (a uniform branch on the kernarg; 1 keeps the per-task stores as they were): each wave leaves its triple
// per query in LDS and adds one to an arrival counter (workgroup scope, acq_rel); the wave whose add completes the count -
// min(4, n_tasks - 4 blockIdx.x): waves past the last task leave at entry - combines the slots (combine_triples) and stores
// the group's gmax / gaux entry.  Which group a workgroup is, and so every index below, comes from sweep_group (i8_sweep.h):
// a reversed sweep writes the same values to the same places in another order in time.  Nobody waits at the end; the
// counter is zeroed behind the one barrier at entry, which stands before the early return.  The stores are plain: their
// reader is the next launch.
template <int NCH, int BQ, int RI, bool NT, bool FULL, bool PQ>
__global__ __launch_bounds__(256) void scan_i8_kernel(const I8ScanParams p) {
    constexpr int NV = RI * BQ;
    constexpr int LPV = 64 / NV;
    __shared__ float s_gmx[kI8BlockWaves][BQ], s_gsec[kI8BlockWaves][BQ];
    __shared__ uint32_t s_garg[kI8BlockWaves][BQ], s_goff[kI8BlockWaves], s_arrive;
    const int lane = threadIdx.x & 63;
    const uint32_t n = p.n, dim = p.dim;
    const bool grouped = p.group_tasks > 1u;
    if (grouped) {
        if (threadIdx.x == 0) s_arrive = 0u;
        __syncthreads();
    }

    uint32_t coff[NCH];
    f4 qv[BQ][NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t idx = (uint32_t)c * 1024u + (uint32_t)lane * 16u;
        const bool in = FULL || idx < dim;
        coff[c] = in ? idx : dim - 16u;
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            const float* qp = p.q + (size_t)((uint32_t)b < p.nq ? b : 0) * dim + coff[c];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const f4 t = *(const f4*)(qp + 4 * w);
                qv[b][c][w] = in ? t : (f4)(0.f);
            }
        }
    }

    const uint32_t last = n - 1u;
    const uint32_t nwords = (n + 31u) / 32u;
    const uint32_t n_tasks = p.n_tasks;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wib = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t wg = sweep_group(blockIdx.x, p.n_wg, p.rev);   // (uniform: the workgroup whose tasks this one takes)
    const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)(wg * wpb + (threadIdx.x >> 6)));
    if (cur >= n_tasks) return;

    const char* const rows_b = (const char*)p.rows;
    auto load_rows = [&](auto nt_c, uint32_t base, int j, u4 (&x)[RI][NCH]) {
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            uint32_t row = base + (uint32_t)(RI * j + r);
            row = row > last ? last : row;
            const char* rp = rows_b + (uint64_t)row * dim;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const u4* src = (const u4*)(rp + coff[c]);
                if (decltype(nt_c)::value) x[r][c] = __builtin_nontemporal_load(src);
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
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint32_t u = x[r][c][w];
                    const f2 lo = {code_f32<0>(u), code_f32<1>(u)}, hi = {code_f32<2>(u), code_f32<3>(u)};
#pragma unroll
                    for (int b = 0; b < BQ; ++b) {
                        const f4 qq = qv[b][c][w];
                        f2 a = acc2[b * RI + r];
                        a = __builtin_elementwise_fma(lo, __builtin_shufflevector(qq, qq, 0, 1), a);
                        a = __builtin_elementwise_fma(hi, __builtin_shufflevector(qq, qq, 2, 3), a);
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
    // scan_bf16_kernel's epilogue after the scale: the f32 drop rules made one-sided with this copy's B_q.  A row with a
    // non-finite component has a NaN scale, so its score is dropped here as the f32 scan drops it.
    auto epilogue = [&](uint32_t cur, uint32_t base, uint32_t trows, uint64_t mask, float scale, float (&sc)[BQ]) {
        const uint32_t row = base + (uint32_t)lane;
        const bool live_all = (uint32_t)lane < trows && ((mask >> lane) & 1ull);
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            const bool live = PQ ? (uint32_t)lane < trows && ((qmask[PQ ? b : 0] >> lane) & 1ull) : live_all;
            float s = sc[b] * scale;
            if (!live || !(__builtin_fabsf(s) <= 3.4028234664e38f)) s = -INFINITY;
            else if (p.mode == 1u && (uint32_t)b < p.nq) {
                float t = s + p.bq[b];
                t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
                if (!(t >= p.thr)) s = -INFINITY;
            }
            if ((uint32_t)b >= p.nq) continue;
            if ((uint32_t)lane < trows && row < p.n_pad) p.scores[(size_t)b * p.n_pad + row] = s;
            const float gm = wave_max64(s);
            if (grouped) {   // this wave's triple of query b into its LDS slot (no gaux: the maximum alone matters)
                uint32_t arg = 0u;
                float sec = -INFINITY;
                if (p.gaux) {
                    arg = (uint32_t)__builtin_ctzll(__ballot(s == gm));
                    sec = wave_max64(((uint32_t)lane == arg) ? -INFINITY : s);
                }
                if (lane == 0) { s_gmx[wib][b] = gm; s_garg[wib][b] = arg; s_gsec[wib][b] = sec; }
                continue;
            }
            if (lane == 0) p.gmax[(size_t)b * n_tasks + cur] = gm;
            if (p.gaux) {
                const uint32_t arg = (uint32_t)__builtin_ctzll(__ballot(s == gm));
                const float sec = wave_max64(((uint32_t)lane == arg) ? -INFINITY : s);
                if (lane == 0) p.gaux[(size_t)b * n_tasks + cur] = ((uint64_t)arg << 32) | (uint64_t)__float_as_uint(sec);
            }
        }
        if (!grouped) return;
        // the hand-off: lane 0 has stored this wave's slots; its acq_rel add releases them and, for the wave that completes
        // the count, acquires every other wave's
        const uint32_t g = wg;   // (= cur / kI8BlockWaves: the launch puts consecutive tasks into a workgroup)
        uint32_t gr;
        const uint32_t gbase = p.tiers.locate(g * kI8BlockWaves, gr);
        uint32_t t = 0u;
        if (lane == 0) {
            s_goff[wib] = base - gbase;
            t = __hip_atomic_fetch_add(&s_arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        const uint32_t left = n_tasks - g * kI8BlockWaves;
        const uint32_t expect = left < kI8BlockWaves ? left : kI8BlockWaves;
        if (t + 1u != expect) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // (every lane that reads the slots below)
        if ((uint32_t)lane < p.nq) {   // lane b combines query b
            MaxTriple w[kI8BlockWaves];
            uint32_t off[kI8BlockWaves];
#pragma unroll
            for (uint32_t i = 0; i < kI8BlockWaves; ++i) {   // (a missing wave: -inf, which never wins and never raises the runner-up)
                const bool there = i < expect;
                w[i] = MaxTriple{there ? s_gmx[i][lane] : -INFINITY, there ? s_garg[i][lane] : 0u, there ? s_gsec[i][lane] : -INFINITY};
                off[i] = there ? s_goff[i] : 0u;
            }
            const MaxTriple m = combine_triples(w, off, kI8BlockWaves);
            p.gmax[(size_t)lane * p.n_groups + g] = m.max;
            if (p.gaux) p.gaux[(size_t)lane * p.n_groups + g] = ((uint64_t)m.arg << 32) | (uint64_t)__float_as_uint(m.sec);
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
    uint32_t trows;
    const uint32_t base = p.tiers.locate(cur, trows);
    const uint64_t mask = task_mask(base, trows);
    const uint32_t srow = base + (uint32_t)lane;
    const float scale = p.scales[srow > last ? last : srow];
    float sc[BQ];
#pragma unroll
    for (int b = 0; b < BQ; ++b) sc[b] = -INFINITY;
    const int nb = (int)(trows / (uint32_t)RI);
    // NT: the load policy is the workgroup's (uniform).  The ends of the copy, where one search stops and the next one
    // starts, load plainly and so are found in the Infinity Cache; the rest streams.  Each arm is the whole batch loop.
    if (NT && wg >= p.plain_lo && wg < p.plain_hi) {
        for (int j = 0; j < nb; ++j) {
            const uint32_t m = (uint32_t)(mask >> (RI * j)) & ((1u << RI) - 1u);
            if (m == 0u) continue;   // all RI rows filtered out / past the end: skip their reads
            load_rows(std::true_type{}, base, j, x);
            reduce_rows(j, x, sc);
        }
    } else {
        for (int j = 0; j < nb; ++j) {
            const uint32_t m = (uint32_t)(mask >> (RI * j)) & ((1u << RI) - 1u);
            if (m == 0u) continue;
            load_rows(std::false_type{}, base, j, x);
            reduce_rows(j, x, sc);
        }
    }
    epilogue(cur, base, trows, mask, scale, sc);
}

constexpr int kI8RowsPerBatch = 16;   // of the single-query pass (divides the 16-row task); 8 measured 3 % slower

template <int NCH, int BQ, int RI, bool PQ>
static hipError_t launch_i8(const ScanArgs& a, const int8_t* codes, const float* scales, const float* bq, uint32_t q0,
                            uint32_t nq, hipStream_t st) {
    I8ScanParams p;
    fill_gemv_pass(p, a, q0, nq, PQ);
    p.rows = codes; p.scales = scales;
    p.bq = bq + q0;
    p.group_tasks = a.group_tasks;
    p.n_groups = (p.n_tasks + a.group_tasks - 1u) / a.group_tasks;
    if (a.group_tasks != 1u) {   // one entry per workgroup: the rows of gmax / gaux are that much shorter
        p.gmax = a.gmax + (size_t)q0 * p.n_groups;
        p.gaux = a.gaux ? a.gaux + (size_t)q0 * p.n_groups : nullptr;
    }
    const uint32_t wpb = kI8BlockWaves;
    const dim3 grid((p.n_tasks + wpb - 1u) / wpb), block(64u * wpb);
    p.n_wg = grid.x;
    p.rev = a.sweep_rev;
    const PlainWindow pw = a.nontemporal ? plain_window(GroupMap{p.tiers, kI8BlockWaves}, p.n, p.dim, a.plain_bytes) : PlainWindow{0u, p.n_wg};
    p.plain_lo = pw.lo; p.plain_hi = pw.hi;
    const bool full = (a.dim == (uint32_t)NCH * 1024u);
    for_nt_full(a.nontemporal, full, [&](auto nt_c, auto full_c) {
        hipLaunchKernelGGL((scan_i8_kernel<NCH, BQ, RI, decltype(nt_c)::value, decltype(full_c)::value, PQ>), grid, block, 0, st, p);
    });
    return hipGetLastError();
}

template <int NCH, bool PQ>
static hipError_t launch_i8_groups(const ScanArgs& a, const int8_t* codes, const float* scales, const float* bq, hipStream_t st) {
    uint32_t done = 0;
    while (done < a.b) {
        const uint32_t left = a.b - done;
        hipError_t e;
        uint32_t g;
        if (left >= 3) { g = left < 4u ? left : 4u; e = launch_i8<NCH, 4, 4, PQ>(a, codes, scales, bq, done, g, st); }   // (3 ride the 4-query pass)
        else if (left >= 2) { g = 2; e = launch_i8<NCH, 2, 8, PQ>(a, codes, scales, bq, done, g, st); }
        else { g = 1; e = launch_i8<NCH, 1, kI8RowsPerBatch, PQ>(a, codes, scales, bq, done, g, st); }
        if (e != hipSuccess) return e;
        done += g;
    }
    return hipSuccess;
}

hipError_t launch_scan_i8(const ScanArgs& a, const int8_t* codes, const float* scales, const float* bq, hipStream_t st) {
    if (a.b == 0 || a.n == 0) return hipSuccess;
    if (a.b > kShadowMaxQ || !i8_dim_ok(a.dim) || (a.group_tasks != 1u && a.group_tasks != kI8BlockWaves)) return hipErrorInvalidValue;
    if (a.keep_tab && !keep_tab_ok(a)) return hipErrorInvalidValue;
    switch ((a.dim + 1023u) / 1024u) {
        case 1: return a.keep_tab ? launch_i8_groups<1, true>(a, codes, scales, bq, st) : launch_i8_groups<1, false>(a, codes, scales, bq, st);
        case 2: return a.keep_tab ? launch_i8_groups<2, true>(a, codes, scales, bq, st) : launch_i8_groups<2, false>(a, codes, scales, bq, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace cqs
