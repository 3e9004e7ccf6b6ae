// select_device.h — the body of the exact top-k select as device functions, shared by select_finish_kernel
// (scan_kernels.hip) and the tail kernel of the shadow search (scan_bf16.hip), whose every workgroup selects for itself.
// Device code only; internal to libcqs_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_sort.h"
#include "scan_device.h"
#include "scan_kernels.h"

namespace cqs {

// Histogram bin of a valid score; monotone non-decreasing in the score.
// linear: 4096 bins of width 2^-11 over [-1,1] (cosine / clamped scores: fine
// resolution exactly where the top-k threshold lives); else the top 12 bits of
// the ordered key (log-spaced, any range: raw dot products).
__device__ __forceinline__ uint32_t bin_of(float s, bool linear) {
    if (linear) {
        const float t = (s + 1.0f) * 2048.0f;
        const int b = (int)t;  // t >= 0 for s >= -1; negatives truncate toward 0 and clamp below
        return (uint32_t)(b < 0 ? 0 : (b > 4095 ? 4095 : b));
    }
    return okey(s) >> 20;
}
// Third form (select mode 2, the sparse index): linear bins over the range the GROUP MAXIMA of this very row span - sums of
// SPLADE products crowd into two or three octaves, where the log-spaced bins above put thousands of groups into the
// threshold bin.  Any monotone map is correct (the candidates are re-ranked on their full keys); this one is sharp where
// the top-k lives.  Scores below `lo` fall into bin 0.
__device__ __forceinline__ uint32_t bin_of_range(float s, float lo, float scale) {
    if (!(scale > 0.f)) return 0u;                        // degenerate range: one bin
    const float t = (s - lo) * scale;
    if (!(t < 4095.0f)) return 4095u;                     // (also an overflowed difference)
    return t > 0.f ? (uint32_t)(int)t : 0u;
}
__device__ __forceinline__ uint32_t bin_any(float s, uint32_t mode, float lo, float scale) {
    return mode == 2u ? bin_of_range(s, lo, scale) : bin_of(s, mode != 0u);
}

// ---- block-wide "find the bin holding the k-th largest" ---------------------
// hist: kHistBins counters (global or LDS).  Finds T = the highest bin such
// that count(bins >= T) >= k_rem.  res[0]=T res[1]=count(bins > T) res[2]=hist[T]
// res[3]=total count.  If total < k_rem: T = 0, res[1] = total - hist[0].
template <int THREADS>
__device__ void block_decide(const uint32_t* hist, uint32_t k_rem, uint32_t* s_part /*>= THREADS/64*/,
                             uint32_t* res /*4, LDS*/) {
    constexpr int BPT = kHistBins / THREADS;
    constexpr int NW = THREADS / 64;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t h[BPT];
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        h[i] = hist[t * BPT + i];
        sum += h[i];
    }
    // inclusive suffix scan over threads (thread THREADS-1 owns the top bins):
    // shuffles inside a wave, then the totals of the higher waves through LDS
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_down(incl, off, 64);
        if (lane + off < 64) incl += v;
    }
    if (lane == 0) s_part[w] = incl;
    __syncthreads();
    for (int ww = w + 1; ww < NW; ++ww) incl += s_part[ww];
    uint32_t above = incl - sum;  // count in bins owned by higher threads
    if (t == 0) {
        res[3] = incl;
        if (incl < k_rem) {  // fewer entries than requested: take them all
            res[0] = 0;
            res[1] = incl - h[0];
            res[2] = h[0];
        }
    }
    if (above < k_rem && incl >= k_rem) {  // exactly one thread
#pragma unroll
        for (int i = BPT - 1; i >= 0; --i) {
            if (above < k_rem && above + h[i] >= k_rem) {
                res[0] = (uint32_t)(t * BPT + i);
                res[1] = above;
                res[2] = h[i];
            }
            above += h[i];
        }
    }
    __syncthreads();
}

// ---- one-block exact select (fallback for heavy ties / crowded bins) --------
// Radix select on the full 64-bit packed key (score bits then row bits: all
// keys distinct), 12-bit digits, streaming the whole score row per pass.
// Leaves <= kCandCap candidates in s_keys and returns their count.
static __device__ uint32_t slow_select(const float* __restrict__ s, uint32_t n_pad, uint32_t k, uint32_t row_base,
                                uint64_t* s_keys, uint32_t* s_hist, uint32_t* s_part, uint32_t* s_res,
                                uint32_t* s_cnt) {
    uint64_t prefix = 0;  // digits decided so far (top bits of the key)
    int bits_done = 0;
    uint32_t k_rem = k, sel_above = 0;
    uint64_t lb = 0;
    while (bits_done < 64) {
        const int w = (64 - bits_done) >= 12 ? 12 : (64 - bits_done);
        for (int i = threadIdx.x; i < (int)kHistBins; i += 1024) s_hist[i] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_pad; i += 1024u) {
            const uint32_t kk = okey(s[i]);
            if (kk <= kInvalidKey) continue;
            const uint64_t key = pack_key(kk, row_base + i);
            if (bits_done == 0 || (key >> (64 - bits_done)) == prefix)
                atomicAdd(&s_hist[(uint32_t)(key >> (64 - bits_done - w)) & ((1u << w) - 1u)], 1u);
        }
        __syncthreads();
        block_decide<1024>(s_hist, k_rem, s_part, s_res);
        const uint32_t T = s_res[0], above = s_res[1], cnt = s_res[2], total = s_res[3];
        __syncthreads();
        if (bits_done == 0 && total <= k) { lb = 0; break; }
        prefix = (prefix << w) | T;
        bits_done += w;
        sel_above += above;
        k_rem -= above;
        lb = prefix << (64 - bits_done);
        if (sel_above + cnt <= kCandCap) break;
    }
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_pad; i += 1024u) {
        const uint32_t kk = okey(s[i]);
        if (kk <= kInvalidKey) continue;
        const uint64_t key = pack_key(kk, row_base + i);
        if (key >= lb) {
            const uint32_t slot = atomicAdd(s_cnt, 1u);
            if (slot < kCandCap) s_keys[slot] = key;
        }
    }
    __syncthreads();
    const uint32_t c = *s_cnt;
    return c < kCandCap ? c : kCandCap;
}

// ---- select: one workgroup per query -----------------------------------------
// Two-level exact top-k.  The scan left (a) every score and (b) the maximum of each
// 64-row group.  The workgroup histograms the group maxima (LDS), takes T = the highest
// bin with at least k maxima at or above it - then at least k scores have bin >= T, so
// every top-k entry has bin >= T and lives in a group whose maximum has bin >= T - reads
// back only those groups (about k of them), and sorts their entries with bin >= T
// (bitonic, packed keys).  Global loads are issued GB per thread at a time so the phases
// are bandwidth- not latency-paced.
constexpr uint32_t kGroupCap = 8192;
constexpr int kGB = 16;  // independent loads in flight per thread
constexpr int kGBShort = 4;  // ... where the maxima are one per group of several tasks (GroupMap::G > 1) and 4 096 slots hold them

#define CQS_STAMP(i) do { if (dbg && threadIdx.x == 0 && blockIdx.x == 0) dbg[i] = __builtin_amdgcn_s_memrealtime(); } while (0)

// Phases 1 and 2 of select_body at GB slots per thread and trip: the histogram of the n_groups maxima gm[], the threshold
// bin T (returned), and the list of the groups whose maximum reaches it (s_groups, their number in *s_ng).  Every slot is
// a load, an LDS atomic, a ballot and an mbcnt whether or not a group stands behind it, so GB follows the number of groups
// (select_body): 16 for a row of up to 16 384 task maxima, 4 where 4 096 groups cover it.
template <int GB>
__device__ __forceinline__ uint32_t select_front(const float* __restrict__ gm, uint32_t n_groups, uint32_t k, uint32_t linear,
                                                 float r_lo, float r_scale, uint32_t* s_hist, uint32_t* s_part, uint32_t* s_res,
                                                 uint32_t* s_ng, uint32_t* s_groups, unsigned long long* __restrict__ dbg) {
    const int lane = threadIdx.x & 63;
    // phase 1: histogram of the group maxima
    float m[GB];
    const bool one_pass = n_groups <= 1024u * GB;  // the maxima then stay in registers for phase 2
    for (uint32_t t0 = 0; t0 < n_groups; t0 += 1024u * GB) {
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            const uint32_t t = t0 + (uint32_t)u * 1024u + threadIdx.x;
            const float v = gm[t < n_groups ? t : n_groups - 1u];  // unconditional load, clamped
            m[u] = t < n_groups ? v : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < GB; ++u)
            if (m[u] != -INFINITY) atomicAdd(&s_hist[bin_any(m[u], linear, r_lo, r_scale)], 1u);
    }
    __syncthreads();
    CQS_STAMP(1);
    block_decide<1024>(s_hist, k, s_part, s_res);
    const uint32_t T = (s_res[3] < k) ? 0u : s_res[0];  // fewer groups than k: every valid score is a candidate
    __syncthreads();
    CQS_STAMP(2);

    // phase 2: groups whose maximum reaches the threshold bin
    for (uint32_t t0 = 0; t0 < n_groups; t0 += 1024u * GB) {
        if (!one_pass) {
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const uint32_t t = t0 + (uint32_t)u * 1024u + threadIdx.x;
                const float v = gm[t < n_groups ? t : n_groups - 1u];
                m[u] = t < n_groups ? v : -INFINITY;
            }
        }
        // list positions by ballot + mbcnt, one LDS atomic per wave (round 5; until then a 6-step shuffle scan over 16 flags)
        bool take[GB];
        uint64_t mk[GB];
        uint32_t pre[GB], tot = 0;
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            take[u] = (m[u] != -INFINITY) && (bin_any(m[u], linear, r_lo, r_scale) >= T);
            mk[u] = __ballot(take[u]);
            pre[u] = tot;
            tot += (uint32_t)__popcll(mk[u]);
        }
        uint32_t base = 0;
        if (tot) {                                       // wave-uniform
            if (lane == 0) base = atomicAdd(s_ng, tot);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        }
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            const uint32_t slot = base + pre[u] + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk[u], 0u));
            if (take[u] && slot < kGroupCap) s_groups[slot] = t0 + (uint32_t)u * 1024u + threadIdx.x;
        }
    }
    __syncthreads();
    CQS_STAMP(3);
    return T;
}

// The select of one query by one workgroup of 1024 threads, up to the sorted candidates: s = the query's score row
// [n_pad], gm / ga = its rows of the scan's gmax / gaux (ga nullable), one entry per group of `map` (G = 1: per task; the
// int8 scan's G = 4: per workgroup of four tasks).  Returns the candidates sorted descending (LDS,
// valid until the workgroup's next use of this function) and their number in `count`, which may exceed k: the first
// min(count, k) are the query's top k.  The LDS it needs is declared here, so every kernel that calls it carries it.
// Every thread of the workgroup must call it (barriers inside); it writes nothing but LDS and the debug stamps.
__device__ __forceinline__ const uint64_t* select_body(const float* __restrict__ s, const float* __restrict__ gm,
                                                       const uint64_t* __restrict__ ga, uint32_t n_pad,
                                                       const GroupMap& map, uint32_t k, uint32_t row_base,
                                                       uint32_t linear, unsigned long long* __restrict__ dbg,
                                                       uint32_t& count_out) {
    __shared__ uint64_t s_keys[kCandCap];
    __shared__ uint32_t s_groups[kGroupCap];
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[kHistBins];
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_res[4];
    __shared__ uint32_t s_cnt, s_ng, s_ng2;
    const TaskTiers& tiers = map.tiers;
    const uint32_t G = map.G;
    const uint32_t n_groups = map.total();
    const int lane = threadIdx.x & 63;
    float r_lo = 0.f, r_scale = 0.f;                       // mode 2: the bins' range (see bin_of_range)

    CQS_STAMP(0);
    for (uint32_t i = threadIdx.x; i < kHistBins; i += 1024u) s_hist[i] = 0u;
    if (threadIdx.x == 0) { s_cnt = 0; s_ng = 0; s_ng2 = 0; }
    __syncthreads();
    if (linear == 2u) {                                    // phase 0: smallest and largest finite group maximum
        float lo = INFINITY, hi = -INFINITY;
        for (uint32_t t0 = 0; t0 < n_groups; t0 += 1024u * kGB) {   // kGB unconditional loads in flight (a conditional one per trip waited for each)
            float v[kGB];
#pragma unroll
            for (int u = 0; u < kGB; ++u) {
                const uint32_t t = t0 + (uint32_t)u * 1024u + threadIdx.x;
                v[u] = gm[t < n_groups ? t : n_groups - 1u];
            }
#pragma unroll
            for (int u = 0; u < kGB; ++u)
                if (v[u] != -INFINITY) { lo = fminf(lo, v[u]); hi = fmaxf(hi, v[u]); }   // (a clamped repeat of the last group changes neither)
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, off, 64));
            hi = fmaxf(hi, __shfl_xor(hi, off, 64));
        }
        float* const f_part = reinterpret_cast<float*>(s_part);
        if (lane == 0) { f_part[threadIdx.x >> 6] = lo; f_part[16 + (threadIdx.x >> 6)] = hi; }
        __syncthreads();
        lo = f_part[0]; hi = f_part[16];
        for (int w = 1; w < 16; ++w) { lo = fminf(lo, f_part[w]); hi = fmaxf(hi, f_part[16 + w]); }
        __syncthreads();                                   // s_part is reused by block_decide
        r_lo = lo;
        r_scale = (hi > lo) ? 4096.0f / (hi - lo) : 0.f;   // (no finite maximum at all: nothing is histogrammed below)
        if (!(r_scale < INFINITY)) r_scale = 0.f;          // a range narrower than 4096 ulps of a subnormal: one bin, the exact path sorts it out
    }

    // phases 1 and 2: the threshold bin and the groups that reach it, at as many slots per thread as the groups need.  Only
    // a map of G > 1 has few enough groups for the short form to pay; G = 1 callers keep the code they had.
    const uint32_t T = (G > 1u && n_groups <= 1024u * kGBShort)
                           ? select_front<kGBShort>(gm, n_groups, k, linear, r_lo, r_scale, s_hist, s_part, s_res, &s_ng, s_groups, dbg)
                           : select_front<kGB>(gm, n_groups, k, linear, r_lo, r_scale, s_hist, s_part, s_res, &s_ng, s_groups, dbg);
    const uint32_t ng = s_ng;
    uint32_t count = kCandCap + 1u;
    if (ng <= kGroupCap) {
        // phase 3: their scores (L2 / Infinity Cache hits: the scan just wrote them).  Round 5: ONE WAVE PER GROUP -
        // lane <-> row of the group, so a group is one coalesced load at a wave-uniform base (no per-element
        // slot -> (group, offset) arithmetic), kGU groups in flight per wave, and the survivors are appended with
        // ballot + mbcnt ranks and ONE LDS atomic per kGU groups.  (Round 4 spread group x slot over all threads:
        // 2 rounds of 16 loads per thread with a 6-step shuffle scan each - 11 us of one CU's issue slots at k = 500.)
        // Round 5, producers that also left `gaux` (the gemv scan, the sparse index): a selected group whose runner-up
        // misses the threshold bin IS its maximum - the candidate (gm, base + arg) goes straight to the list and the
        // group's rows are never read; only groups with a second entry at or above the threshold (a few per cent at
        // k = 500, all of them under heavy ties) are gathered.
        const uint32_t* glist = s_groups;
        uint32_t n2 = ng;
        if (ga) {
            uint32_t* const s_list2 = s_hist;              // the histogram is dead (T lives in a register)
            for (uint32_t i0 = 0; i0 < ng; i0 += 1024u) {
                const uint32_t i = i0 + threadIdx.x;
                const bool valid = i < ng;
                const uint32_t t = s_groups[valid ? i : ng - 1u];
                const uint64_t ax = ga[t];
                const float mx = gm[t];
                const float sec = __uint_as_float((uint32_t)ax);
                const bool need = valid && (sec != -INFINITY) && (bin_any(sec, linear, r_lo, r_scale) >= T);
                const bool direct = valid && !need;
                // a group to gather appends its (up to G) tasks: task j of every such group by one ballot, one LDS atomic per wave
                const uint32_t ntk = need ? map.tasks(t) : 0u;
                const uint64_t md = __ballot(direct);
                uint64_t mn[kMaxGroupTasks];
                uint32_t pn[kMaxGroupTasks], totn = 0;
#pragma unroll
                for (uint32_t j = 0; j < kMaxGroupTasks; ++j) {
                    mn[j] = (j < G) ? __ballot(need && (j == 0u || j < ntk)) : 0ull;
                    pn[j] = totn;
                    totn += (uint32_t)__popcll(mn[j]);
                }
                uint32_t bn = 0, bd = 0;
                if (lane == 0) {
                    if (totn) bn = atomicAdd(&s_ng2, totn);
                    if (md) bd = atomicAdd(&s_cnt, (uint32_t)__popcll(md));
                }
                bn = (uint32_t)__builtin_amdgcn_readfirstlane((int)bn);
                bd = (uint32_t)__builtin_amdgcn_readfirstlane((int)bd);
#pragma unroll
                for (uint32_t j = 0; j < kMaxGroupTasks; ++j) {
                    if (j < G && need && (j == 0u || j < ntk)) {
                        const uint32_t slot = bn + pn[j] + __builtin_amdgcn_mbcnt_hi((uint32_t)(mn[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mn[j], 0u));
                        if (slot < kHistBins) s_list2[slot] = G * t + j;
                    }
                }
                if (direct) {
                    const uint32_t slot = bd + __builtin_amdgcn_mbcnt_hi((uint32_t)(md >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)md, 0u));
                    if (slot < kCandCap) s_keys[slot] = pack_key(okey(mx), row_base + map.base(t) + (uint32_t)(ax >> 32));
                }
            }
            __syncthreads();
            if (s_ng2 <= kHistBins) { glist = s_list2; n2 = s_ng2; }
            else {                                         // more tasks to read than the second list holds: read every listed group
                __syncthreads();
                if (threadIdx.x == 0) s_cnt = 0;
                __syncthreads();
            }
        }
        // one wave per TASK: 64 / 32 / 16 rows.  The second list holds tasks; the group list (no gaux, or the second list
        // overflowed) holds groups, each standing for its G tasks (entry e: task e % G of group e / G; G is a power of two)
        const bool by_group = glist == s_groups;
        const uint32_t gsh = (uint32_t)__builtin_ctz(G), n_tasks = tiers.total();
        if (by_group) n2 = ng << gsh;
        constexpr int kGU = 8;
        const uint32_t wv = threadIdx.x >> 6;
        for (uint32_t g0 = wv * kGU; g0 < n2; g0 += 16u * kGU) {
            float v[kGU];
            uint32_t idx[kGU];
            bool in[kGU];
#pragma unroll
            for (int u = 0; u < kGU; ++u) {
                const uint32_t g = g0 + (uint32_t)u;
                uint32_t grows;
                const uint32_t e = g < n2 ? g : n2 - 1u;
                uint32_t task = (uint32_t)__builtin_amdgcn_readfirstlane((int)glist[by_group ? e >> gsh : e]);
                bool there = true;
                if (G > 1u && by_group) {                  // (a partial last group has fewer than G tasks)
                    task = (task << gsh) + (e & (G - 1u));
                    there = task < n_tasks;
                    task = there ? task : n_tasks - 1u;
                }
                const uint32_t gbase = tiers.locate(task, grows);
                in[u] = g < n2 && there && (uint32_t)lane < grows;
                idx[u] = gbase + (in[u] ? (uint32_t)lane : 0u);
            }
#pragma unroll
            for (int u = 0; u < kGU; ++u) v[u] = s[idx[u]];
            uint64_t mask[kGU];
            uint32_t pre[kGU], tot = 0;
            bool take[kGU];
#pragma unroll
            for (int u = 0; u < kGU; ++u) {
                take[u] = in[u] && (v[u] != -INFINITY) && (bin_any(v[u], linear, r_lo, r_scale) >= T);
                mask[u] = __ballot(take[u]);
                pre[u] = tot;
                tot += (uint32_t)__popcll(mask[u]);
            }
            uint32_t base = 0;
            if (tot) {                                   // wave-uniform
                if (lane == 0) base = atomicAdd(&s_cnt, tot);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            }
#pragma unroll
            for (int u = 0; u < kGU; ++u) {
                const uint32_t slot = base + pre[u] +
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(mask[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask[u], 0u));
                if (take[u] && slot < kCandCap) s_keys[slot] = pack_key(okey(v[u]), row_base + idx[u]);
            }
        }
        __syncthreads();
        count = s_cnt;
    }
    if (count > kCandCap)  // heavy ties / crowded threshold bin: exact radix select over the whole row
        count = slow_select(s, n_pad, k, row_base, s_keys, s_hist, s_part, s_res, &s_cnt);

    CQS_STAMP(4);
    if (dbg && threadIdx.x == 0 && blockIdx.x == 0) { dbg[8] = ng; dbg[9] = count; }
    const uint64_t* sorted = s_keys;
    if (count <= 1024u) {
        uint64_t* s_sorted = reinterpret_cast<uint64_t*>(s_groups);  // group list is dead by now
        uint32_t* s_ok = s_hist;                                      // histogram is dead by now (slow_select included)
        rank_sort_keys(s_keys, count, s_sorted, s_ok, s_res);         // (rank_sort.h, shared with the bf16 certify kernel)
        sorted = s_sorted;
    } else {
        // Bitonic sort, descending (slow path sizes: up to kCandCap).
        uint32_t P = 2048;
        while (P < count) P <<= 1;
        for (uint32_t i = count + threadIdx.x; i < P; i += 1024u) s_keys[i] = 0ull;
        __syncthreads();
        for (uint32_t size = 2; size <= P; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t t = threadIdx.x; t < P / 2; t += 1024u) {
                    const uint32_t i = 2u * t - (t & (stride - 1u));  // lower index of the pair
                    const uint32_t j = i + stride;
                    const uint64_t a = s_keys[i], b = s_keys[j];
                    const bool desc = ((i & size) == 0u);
                    if ((a < b) == desc) {
                        s_keys[i] = b;
                        s_keys[j] = a;
                    }
                }
                __syncthreads();
            }
        }
    }

    CQS_STAMP(5);
#undef CQS_STAMP
    count_out = count;
    return sorted;
}

}  // namespace cqs
