// index_match.hip — cqs_hip_index_match: for two lists of stored rows, one of each of two resident indexes, the best
// partner of every row on the other side.  `semantic_diff` (src/diff.rs:43-53) matches chunks by (file, name, chunk_type),
// so a moved or renamed function is one `removed` and one unrelated `added` entry; its comment at :45-47 stops at line
// moves because the host has no cheap way to compare every removed chunk with every added one.  Here that is the cross
// similarity of two row lists already in HBM, reduced to one candidate per row of either side before anything is stored:
// the [m_a, m_b] matrix never exists.  The plan, the key and the merge rules are match_host.h; DESIGN.md §3.17a.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "abi_guard.h"
#include "diff_host.h"
#include "index_internal.h"
#include "match_host.h"
#include "roctx.h"
#include "scan_device.h"
#include "wave_ops.h"

namespace cqs_idx {

typedef float match_f16v __attribute__((ext_vector_type(16)));

// ---- S = A B^T, reduced as it is made -------------------------------------------------------------------------------------
// The cross form of gram_gather_kernel (mmr.hip): one wave per 32 x 32 tile of [m_a, m_b], the whole K range, through
// v_mfma_f32_32x32x2_f32.  An entry is the exact f32 fma chain
//     over k in the order  32 it + 8 u + c, 32 it + 8 u + 4 + c   (it = 0 .., u = 0..3, c = 0..3)
// of its two rows and of nothing else - the loop below is that kernel's, trip for trip, so S[i][j] is the bits
// cqs_hip_index_pairwise gives for the two rows, whichever side either came from (the products commute).  Lane l feeds
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]: per step of 8 floats it loads 16 bytes of its row of either
// tile, four steps in flight while the previous four multiply.  A lane whose row is past its list or whose floats are past
// dim holds zeros and does not read.
//
// A workgroup is four waves on ONE tile row ti and a span of B tiles: wave w takes tiles first + w, first + w + 4, ... of
// the span, so the four read the same 32 A rows at about the same time (the second to fourth find them in the CU's L1).
// Accumulator register r of lane l is S[A row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][B row l & 31] of the tile.  A candidate is
// the library's key (okey(score) << 32) | (0xFFFFFFFF - position): greater score under the f32 total order, then lower
// position; a non-finite score and an entry past either list are key 0, "none", below every real candidate.
//     B side   per tile: the lane's 16 registers are 16 A rows of ONE B row - a lane-local maximum, one exchange with the
//              other half-wave (the other 16 A rows), one atomicMax per B row of the tile.
//     A side   register r stays one A row for every tile of the wave: the lane keeps a running maximum per register over
//              its B rows of all those tiles, and only after the last tile the 32 lanes of a half-wave reduce each
//              (four DPP steps and a row swap), one atomicMax per A row of the wave.
// The best arrays are zeroed before the launch; the maximum of a total order is order-free, so the answer does not depend
// on the span, the grid or the order in which workgroups run.  A plain-looking (relaxed) read of the current best skips
// the atomic where the candidate cannot win: the value only grows, so a stale read only skips less.
constexpr int kMatchU = 4;            // 8-float steps per loop trip
constexpr uint32_t kMatchWaves = 4;   // waves of a workgroup
constexpr uint32_t kMatchThreads = 64u * kMatchWaves;

struct MatchParams {
    const float* rows_a;          // a's corpus
    const float* rows_b;          // b's
    const uint32_t* la;           // [m_a] local row of a per position ...
    const uint32_t* lb;           // [m_b] ... and of b
    uint32_t m_a, m_b, dim;
    uint32_t tiles_b;             // ceil(m_b / 32)
    uint32_t span;                // B tiles per workgroup (a multiple of kMatchWaves)
    unsigned long long* best_a;   // [m_a] packed bests, zeroed
    unsigned long long* best_b;   // [m_b]
};

__device__ __forceinline__ uint64_t match_key(float s, bool inside, uint32_t position) {
    const bool finite = (__float_as_uint(s) & 0x7F800000u) != 0x7F800000u;
    return (inside && finite) ? cqs::pack_key(cqs::okey(s), position) : 0ull;
}
__device__ __forceinline__ uint64_t match_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
template <int CTRL>
__device__ __forceinline__ uint64_t match_key_dpp(uint64_t k) {
    const uint32_t lo = __float_as_uint(cqs::wave_dpp<CTRL>(__uint_as_float((uint32_t)k)));
    const uint32_t hi = __float_as_uint(cqs::wave_dpp<CTRL>(__uint_as_float((uint32_t)(k >> 32))));
    return ((uint64_t)hi << 32) | lo;
}
// The maximum over the 32 lanes of this lane's half-wave, in all of them: the four DPP steps of a 16-lane row, then the
// row pair (mmr.hip's wave_max_key without its last step).
__device__ __forceinline__ uint64_t match_half_max(uint64_t k) {
    k = match_max(k, match_key_dpp<0xB1>(k));
    k = match_max(k, match_key_dpp<0x4E>(k));
    k = match_max(k, match_key_dpp<0x141>(k));
    k = match_max(k, match_key_dpp<0x140>(k));
    const cqs::lane_u2 lo = cqs::swap16_self((uint32_t)k), hi = cqs::swap16_self((uint32_t)(k >> 32));
    return match_max(((uint64_t)hi[0] << 32) | lo[0], ((uint64_t)hi[1] << 32) | lo[1]);
}
// max(lanes 0-31, lanes 32-63) of the same lane & 31, in both.
__device__ __forceinline__ uint64_t match_halves_max(uint64_t k) {
    const cqs::lane_u2 lo = cqs::swap32_self((uint32_t)k), hi = cqs::swap32_self((uint32_t)(k >> 32));
    return match_max(((uint64_t)hi[0] << 32) | lo[0], ((uint64_t)hi[1] << 32) | lo[1]);
}
__device__ __forceinline__ void match_offer(unsigned long long* slot, uint64_t key) {
    if (key > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, (unsigned long long)key);
}

__global__ __launch_bounds__(kMatchThreads) void match_cross_kernel(const MatchParams p) {
    const uint32_t lane = threadIdx.x & 63u, l31 = lane & 31u, lh = lane >> 5;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ti = blockIdx.y;
    const uint32_t ra = ti * 32u + l31;
    const float* pa = nullptr;
    if (ra < p.m_a) pa = p.rows_a + (size_t)p.la[ra] * p.dim + 4u * lh;
    const uint32_t kend = p.dim - 4u * lh;      // this lane's floats of a step at k0 exist while k0 < kend (dim % 4 == 0)

    auto load = [&](const float* row, uint32_t k0, cqs::f4 (&v)[kMatchU]) {
#pragma unroll
        for (int u = 0; u < kMatchU; ++u) {
            const uint32_t k = k0 + 8u * (uint32_t)u;
            v[u] = (row && k < kend) ? *(const cqs::f4*)(row + k) : cqs::f4{0.f, 0.f, 0.f, 0.f};
        }
    };

    uint64_t run[16];                           // the best B position so far of this lane's B rows, per register's A row
#pragma unroll
    for (int r = 0; r < 16; ++r) run[r] = 0ull;

    const uint32_t first = blockIdx.x * p.span;
    const uint32_t last = min(p.tiles_b, first + p.span);
    for (uint32_t tj = first + wave; tj < last; tj += kMatchWaves) {      // (uniform over the wave)
        const uint32_t gj = tj * 32u + l31;
        const float* pb = nullptr;
        if (gj < p.m_b) pb = p.rows_b + (size_t)p.lb[gj] * p.dim + 4u * lh;
        match_f16v acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        cqs::f4 a[kMatchU], b[kMatchU], an[kMatchU], bn[kMatchU];
        load(pa, 0u, a);
        load(pb, 0u, b);
        for (uint32_t k0 = 0; k0 < p.dim; k0 += 8u * kMatchU) {
            load(pa, k0 + 8u * kMatchU, an);     // (past dim: zeros, no read)
            load(pb, k0 + 8u * kMatchU, bn);
#pragma unroll
            for (int u = 0; u < kMatchU; ++u)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][c], b[u][c], acc, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < kMatchU; ++u) { a[u] = an[u]; b[u] = bn[u]; }
        }
        uint64_t col = 0ull;                     // the best A position of B row gj among this lane's 16 A rows
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t gi = ti * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * lh;
            const bool inside = gi < p.m_a && gj < p.m_b;
            col = match_max(col, match_key(acc[r], inside, gi));
            run[r] = match_max(run[r], match_key(acc[r], inside, gj));
        }
        col = match_halves_max(col);
        if (lh == 0u && col != 0ull) match_offer(p.best_b + gj, col);      // (col != 0 only where gj < m_b)
    }

    uint64_t mine = 0ull;                        // lane l31 = r of either half-wave ends with register r's row
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint64_t k = match_half_max(run[r]);
        if (l31 == (uint32_t)r) mine = k;
    }
    const uint32_t gi = ti * 32u + ((l31 & 3u) + 8u * ((l31 >> 2) & 3u)) + 4u * lh;
    if (l31 < 16u && mine != 0ull) match_offer(p.best_a + gi, mine);      // (mine != 0 only where gi < m_a)
}

namespace {

// A call of r = m_a + m_b rows in the staging block: the packed bests first (a's, then b's: one clear, one copy back),
// then the two local row lists (one copy in).
struct MatchStage {
    uint64_t m_a, m_b;
    MatchStage(uint64_t ma, uint64_t mb) : m_a(ma), m_b(mb) {}
    static uint64_t total(uint64_t rows) { return 12u * rows; }
    uint64_t key_bytes() const { return 8u * (m_a + m_b); }
    uint64_t list_bytes() const { return 4u * (m_a + m_b); }
    unsigned long long* best_a(void* base) const { return (unsigned long long*)base; }
    unsigned long long* best_b(void* base) const { return (unsigned long long*)base + m_a; }
    uint32_t* la(void* base) const { return (uint32_t*)((char*)base + key_bytes()); }
    uint32_t* lb(void* base) const { return la(base) + m_a; }
};

// The staging pair holds a call of `rows` rows (regrown; a's stream is idle of earlier matches: each ends with a wait).
// Nothing is touched on failure.
int32_t ensure_match_stage(cqs_hip_index* a, uint64_t rows) {
    if (rows <= a->match_rows) return CQS_HIP_OK;
    match_free(a);
    const uint64_t bytes = MatchStage::total(rows);
    hipError_t e = hipHostMalloc(&a->match_h, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&a->match_d, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        match_free(a);
        return fail(a, e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, "match: staging buffer", e);
    }
    a->match_rows = rows;
    return CQS_HIP_OK;
}

cqs_match::Side match_side_of(const cqs_hip_index* x) {
    return cqs_match::Side{true, x->sh != nullptr, x->device, x->dim, x->row_base, x->sh ? 0 : x->n};
}

bool match_poisoned(const cqs_hip_index* x) {
    return x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire);
}

// B tiles per workgroup: the longest span that still leaves the device a thousand workgroups, so that a short list does
// not idle the chip and a long one makes few atomics on the A side.
uint32_t match_span(uint32_t tiles_a, uint32_t tiles_b) {
    uint32_t span = 64;
    while (span > kMatchWaves && (uint64_t)tiles_a * ((tiles_b + span - 1) / span) < 1024u) span /= 2;
    return span;
}

// Caller holds both mutexes and has planned the call; both lists have rows.  Everything runs on a's stream, ordered
// after the last search of each handle, and ends with a wait: nothing of b is read once the call has returned.
int32_t match_locked(cqs_hip_index* a, cqs_hip_index* b, const uint64_t* rows_a, uint32_t m_a, const uint64_t* rows_b, uint32_t m_b,
                     uint64_t* out_best_a, float* out_score_a, uint64_t* out_best_b, float* out_score_b) {
    HIP_TRY(a, hipSetDevice(a->device));
    HIP_TRY(a, order_after_last(a, a->stream));
    if (b != a) HIP_TRY(a, order_after_last(b, a->stream));
    const int32_t rc = ensure_match_stage(a, (uint64_t)m_a + m_b);
    if (rc != CQS_HIP_OK) return rc;
    const MatchStage st(m_a, m_b);
    cqs_match::local_rows(rows_a, a->row_base, m_a, st.la(a->match_h));
    cqs_match::local_rows(rows_b, b->row_base, m_b, st.lb(a->match_h));
    HIP_TRY(a, hipMemcpyAsync(st.la(a->match_d), st.la(a->match_h), st.list_bytes(), hipMemcpyHostToDevice, a->stream));
    HIP_TRY(a, hipMemsetAsync(a->match_d, 0, st.key_bytes(), a->stream));
    MatchParams p;
    p.rows_a = a->d_rows;
    p.rows_b = b->d_rows;
    p.la = st.la(a->match_d);
    p.lb = st.lb(a->match_d);
    p.m_a = m_a;
    p.m_b = m_b;
    p.dim = a->dim;
    const uint32_t tiles_a = (m_a + 31u) / 32u;
    p.tiles_b = (m_b + 31u) / 32u;
    p.span = match_span(tiles_a, p.tiles_b);
    p.best_a = st.best_a(a->match_d);
    p.best_b = st.best_b(a->match_d);
    hipLaunchKernelGGL(match_cross_kernel, dim3((p.tiles_b + p.span - 1u) / p.span, tiles_a), dim3(kMatchThreads), 0, a->stream, p);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, hipMemcpyAsync(a->match_h, a->match_d, st.key_bytes(), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(a, hipStreamSynchronize(a->stream));
    const unsigned long long* ka = st.best_a(a->match_h);
    const unsigned long long* kb = st.best_b(a->match_h);
    for (uint32_t i = 0; i < m_a; ++i) cqs_match::unpack(ka[i], &out_best_a[i], &out_score_a[i]);
    for (uint32_t j = 0; j < m_b; ++j) cqs_match::unpack(kb[j], &out_best_b[j], &out_score_b[j]);
    return CQS_HIP_OK;
}

}  // namespace

void match_free(cqs_hip_index* x) {
    if (x->match_h) (void)hipHostFree(x->match_h);
    if (x->match_d) (void)hipFree(x->match_d);
    x->match_h = x->match_d = nullptr;
    x->match_rows = 0;
}

}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

int32_t cqs_hip_index_match(cqs_hip_index* a, const uint64_t* rows_a, uint32_t m_a, cqs_hip_index* b, const uint64_t* rows_b,
                            uint32_t m_b, uint64_t* out_best_a, float* out_score_a, uint64_t* out_best_b,
                            float* out_score_b) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_match");
    if (!a || !b) return CQS_HIP_ERR_INVALID;
    cqs_diff::PairLock<std::mutex> g(a->mu, b->mu);
    if (match_poisoned(a) || match_poisoned(b)) return CQS_HIP_ERR_POISONED;
    const cqs_match::Args args{rows_a, m_a, rows_b, m_b, out_best_a != nullptr, out_score_a != nullptr, out_best_b != nullptr,
                               out_score_b != nullptr};
    std::string why;
    const cqs_match::Plan plan = cqs_match::plan_match(match_side_of(a), match_side_of(b), args, &why);
    if (plan == cqs_match::Plan::Invalid) return fail(a, CQS_HIP_ERR_INVALID, ("match: " + why).c_str());
    if (plan == cqs_match::Plan::Nothing) return CQS_HIP_OK;
    if (m_a == 0 || m_b == 0) {                  // an empty other side: no entry, so no finite entry, and no device work
        for (uint32_t i = 0; i < m_a; ++i) cqs_match::unpack(0, &out_best_a[i], &out_score_a[i]);
        for (uint32_t j = 0; j < m_b; ++j) cqs_match::unpack(0, &out_best_b[j], &out_score_b[j]);
        return CQS_HIP_OK;
    }
    return match_locked(a, b, rows_a, m_a, rows_b, m_b, out_best_a, out_score_a, out_best_b, out_score_b);
} CQS_ABI_CATCH(a)

}  // extern "C"
