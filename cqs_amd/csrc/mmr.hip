// mmr.hip — pairwise similarities of stored rows and the MMR re-rank of a candidate pool, on the device.
//
// The reference diversifies its top-K pool with `mmr_rerank` (src/search/mmr.rs:59-126) over a surface-feature similarity
// because it drops the embeddings after scoring (mmr.rs:30-37, src/search/query.rs:540-542: "embedding-MMR is a
// follow-up").  Here every candidate's row is still resident behind the handle that produced the candidates, so the
// similarity is the dot of the two stored rows (the cosine on a COSINE index):
//     gram_gather_kernel   G = X X^T of the m gathered rows, exact f32 on the matrix cores, upper triangle + mirror
//     mmr_greedy_kernel    mmr_rerank's loop over G: one workgroup, one thread per candidate, `limit` steps
// and only `limit` indices cross the bus.  The device-free part (argument checks, the answers mmr.rs:64-69 gives without
// a loop) is mmr_host.h.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>

#include "abi_guard.h"
#include "roctx.h"
#include "index_internal.h"
#include "mmr_host.h"
#include "scan_device.h"

using namespace cqs_idx;
using cqs::f4;

namespace cqs_mmr {

typedef float f16v __attribute__((ext_vector_type(16)));

// ---- G = X X^T -------------------------------------------------------------------------------------------------------
// One wave per 32 x 32 output tile (ti <= tj) of the upper triangle, the whole K range: v_mfma_f32_32x32x2_f32 is an exact
// f32 fma chain, so an entry is
//     fma over k in the order  32 it + 8 u + c, 32 it + 8 u + 4 + c   (it = 0 .., u = 0..3, c = 0..3)
// of its two rows and of nothing else: not of m, not of the tile, not of which of the two rows came first (the products
// commute).  G[i][j] and G[j][i] are one register written twice; a row listed twice gives entries equal to its diagonal's.
// Lane l feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]: per step of 8 floats it loads 16 bytes of its row
// of either tile (floats 4 (l >> 5) .. + 4 of the step), four steps in flight while the previous four multiply.  A lane
// whose row is past m or whose floats are past dim holds zeros and does not read.
constexpr int kGramU = 4;   // 8-float steps per loop trip

struct GramParams {
    const float* rows;      // [*, dim]
    const uint32_t* idx;    // [m] row of candidate i (null: i)
    uint32_t m, dim, tiles; // tiles = ceil(m / 32)
    float* gram;            // [m, m]
};

__global__ __launch_bounds__(64) void gram_gather_kernel(const GramParams p) {
    const uint32_t lane = threadIdx.x, l31 = lane & 31u, lh = lane >> 5;
    uint32_t ti = 0, rem = blockIdx.x;
    while (rem >= p.tiles - ti) { rem -= p.tiles - ti; ++ti; }     // (uniform: at most 32 trips)
    const uint32_t tj = ti + rem;
    const bool diag = ti == tj;
    const uint32_t ra = ti * 32u + l31, rb = tj * 32u + l31;
    const float* pa = nullptr;
    const float* pb = nullptr;
    if (ra < p.m) pa = p.rows + (size_t)(p.idx ? p.idx[ra] : ra) * p.dim + 4u * lh;
    if (rb < p.m) pb = p.rows + (size_t)(p.idx ? p.idx[rb] : rb) * p.dim + 4u * lh;
    const uint32_t kend = p.dim - 4u * lh;      // this lane's floats of a step at k0 exist while k0 < kend (dim % 4 == 0)

    auto load = [&](const float* row, uint32_t k0, f4 (&v)[kGramU]) {
#pragma unroll
        for (int u = 0; u < kGramU; ++u) {
            const uint32_t k = k0 + 8u * (uint32_t)u;
            v[u] = (row && k < kend) ? *(const f4*)(row + k) : f4{0.f, 0.f, 0.f, 0.f};
        }
    };
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f4 a[kGramU], b[kGramU], an[kGramU], bn[kGramU];
    load(nullptr, 0u, b);                        // (a diagonal tile multiplies a by a; b stays zero, unused)
    load(nullptr, 0u, bn);
    load(pa, 0u, a);
    if (!diag) load(pb, 0u, b);
    for (uint32_t k0 = 0; k0 < p.dim; k0 += 8u * kGramU) {
        load(pa, k0 + 8u * kGramU, an);          // (past dim: zeros, no read)
        if (!diag) load(pb, k0 + 8u * kGramU, bn);
#pragma unroll
        for (int u = 0; u < kGramU; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][c], diag ? a[u][c] : b[u][c], acc, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < kGramU; ++u) { a[u] = an[u]; b[u] = bn[u]; }
    }
    // register r <-> A row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), lane & 31 <-> B row
    const uint32_t gj = tj * 32u + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t gi = ti * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * lh;
        if (gi < p.m && gj < p.m && (!diag || gi <= gj)) {
            p.gram[(size_t)gi * p.m + gj] = acc[r];
            p.gram[(size_t)gj * p.m + gi] = acc[r];
        }
    }
}

// A shard's candidates into a dense block: one 16-byte piece per thread.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* rows, const uint32_t* idx, uint32_t mc, uint32_t dim,
                                                          float* out) {
    const uint32_t per = dim / 4u;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)mc * per) return;
    const uint32_t i = (uint32_t)(t / per), c = (uint32_t)(t % per);
    ((f4*)out)[t] = *(const f4*)(rows + (size_t)idx[i] * dim + 4u * c);
}

// ---- the greedy loop ---------------------------------------------------------------------------------------------------
// mmr.rs:92: `lambda * cand.score - (1.0 - lambda) * max_sim`, every operation rounded on its own (Rust never contracts).
// Written as plain operators under `fp contract(off)`: this toolchain's __fmul_rn / __fsub_rn are `x * y` / `x - y` inline
// functions of a header compiled with contraction on, and hipcc fused them into one v_fma_f32 here (seen in the ISA).
__device__ __forceinline__ float mmr_value(float lambda, float one_minus, float score, float max_sim) {
#pragma clang fp contract(off)
    const float rel = lambda * score;
    const float div = one_minus * max_sim;
    return rel - div;
}

template <int CTRL>
__device__ __forceinline__ uint64_t key_dpp(uint64_t k) {
    const uint32_t lo = __float_as_uint(cqs::wave_dpp<CTRL>(__uint_as_float((uint32_t)k)));
    const uint32_t hi = __float_as_uint(cqs::wave_dpp<CTRL>(__uint_as_float((uint32_t)(k >> 32))));
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t key_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
// cqs::wave_max64 for packed keys: the same four DPP steps and two lane swaps, both halves of the key moved alike.
__device__ __forceinline__ uint64_t wave_max_key(uint64_t k) {
    k = key_max(k, key_dpp<0xB1>(k));
    k = key_max(k, key_dpp<0x4E>(k));
    k = key_max(k, key_dpp<0x141>(k));
    k = key_max(k, key_dpp<0x140>(k));
    {
        const cqs::lane_u2 lo = cqs::swap16_self((uint32_t)k), hi = cqs::swap16_self((uint32_t)(k >> 32));
        k = key_max(((uint64_t)hi[0] << 32) | lo[0], ((uint64_t)hi[1] << 32) | lo[1]);
    }
    const cqs::lane_u2 lo = cqs::swap32_self((uint32_t)k), hi = cqs::swap32_self((uint32_t)(k >> 32));
    return key_max(((uint64_t)hi[0] << 32) | lo[0], ((uint64_t)hi[1] << 32) | lo[1]);
}

// `mmr_rerank`'s loop (mmr.rs:74-123) for 0 < limit < m <= 1024 and lambda in [0, 1): thread i is candidate i.
//   max_sim   the fold of f32::max over the selected from 0.0 (mmr.rs:83-90), kept as a running maximum: each step folds
//             the LAST pick's Gram row in.  `max` over the values is exact and order-free, so this is the re-fold's value;
//             fmaxf drops a NaN operand as f32::max does.
//   winner    greatest mmr under f32::total_cmp, lowest index among equals (mmr.rs:107-111) = the maximum of
//             (okey(mmr) << 32) | (0xFFFFFFFF - i): one `max` per pair.  A selected or absent thread holds key 0, below
//             every live key (a live key's low word is >= 0xFFFFFFFF - 1023).
// picks[0] = the count, picks[1 ..] the indices in pick order.
__global__ __launch_bounds__(1024) void mmr_greedy_kernel(const float* gram, const float* scores, uint32_t m, uint32_t limit,
                                                          float lambda, uint32_t* picks) {
    __shared__ uint64_t s_key[2][16];
    const uint32_t i = threadIdx.x, lane = i & 63u, wid = i >> 6, nw = (blockDim.x + 63u) >> 6;
    const bool live = i < m;
    const float score = live ? scores[i] : 0.f;
    const float one_minus = 1.0f - lambda;
    float max_sim = 0.f;
    bool selected = false;
    uint32_t last = 0;
    for (uint32_t t = 0; t < limit; ++t) {
        if (t && live && !selected && last < m) max_sim = fmaxf(max_sim, gram[(size_t)last * m + i]);
        const uint64_t mine = (live && !selected) ? cqs::pack_key(cqs::okey(mmr_value(lambda, one_minus, score, max_sim)), i) : 0ull;
        const uint64_t wmax = wave_max_key(mine);
        if (lane == 0) s_key[t & 1u][wid] = wmax;
        __syncthreads();      // (one barrier per step: step t + 2 reuses this half only after every wave has passed step t + 1's)
        uint64_t best = 0ull;
        for (uint32_t w = 0; w < nw; ++w) best = key_max(best, s_key[t & 1u][w]);
        last = 0xFFFFFFFFu - (uint32_t)best;
        if (i == last) selected = true;
        if (i == 0) picks[1u + t] = last;
    }
    if (i == 0) picks[0] = limit;
}

// ---- scratch ---------------------------------------------------------------------------------------------------------
// Made on the first call, sized for the largest pool seen so far, freed with the handle.
struct Scratch {
    uint32_t m_cap = 0;
    uint32_t* d_idx = nullptr;     // [m_cap] row of each candidate
    float* d_scores = nullptr;     // [m_cap]
    float* d_gram = nullptr;       // [m_cap, m_cap] (4 MB at 1024)
    uint32_t* d_picks = nullptr;   // [1 + m_cap] count, picks
    uint32_t* h_io = nullptr;      // pinned [3 m_cap + 1]: idx | scores | count, picks
    // row-sharded handles: a shard's gathered candidates / the parent's staging block, [block_cap, dim], and the shard's
    // candidates' local rows (device, pinned twin)
    uint32_t block_cap = 0;
    float* d_block = nullptr;
    uint32_t* d_bidx = nullptr;
    uint32_t* h_bidx = nullptr;
};

static void release(Scratch* s) {
    (void)hipFree(s->d_idx); (void)hipFree(s->d_scores); (void)hipFree(s->d_gram); (void)hipFree(s->d_picks);
    (void)hipHostFree(s->h_io);
    s->d_idx = nullptr; s->d_scores = nullptr; s->d_gram = nullptr; s->d_picks = nullptr; s->h_io = nullptr;
    s->m_cap = 0;
}

void free_scratch(cqs_hip_index* x) {
    if (!x->mmr) return;
    (void)hipSetDevice(x->device);
    release(x->mmr);
    (void)hipFree(x->mmr->d_block); (void)hipFree(x->mmr->d_bidx); (void)hipHostFree(x->mmr->h_bidx);
    delete x->mmr;
    x->mmr = nullptr;
}

static int32_t ensure(cqs_hip_index* x, hipStream_t st, uint32_t m) {
    if (!x->mmr) {
        x->mmr = new (std::nothrow) Scratch();
        if (!x->mmr) return fail(x, CQS_HIP_ERR_NOMEM, "mmr: out of host memory");
    }
    Scratch* s = x->mmr;
    if (m <= s->m_cap) return CQS_HIP_OK;
    HIP_TRY(x, hipStreamSynchronize(st));
    release(s);
    HIP_TRY(x, hipMalloc(&s->d_idx, (size_t)m * sizeof(uint32_t)));
    HIP_TRY(x, hipMalloc(&s->d_scores, (size_t)m * sizeof(float)));
    HIP_TRY(x, hipMalloc(&s->d_gram, (size_t)m * m * sizeof(float)));
    HIP_TRY(x, hipMalloc(&s->d_picks, ((size_t)m + 1) * sizeof(uint32_t)));
    HIP_TRY(x, hipHostMalloc((void**)&s->h_io, (3 * (size_t)m + 1) * sizeof(uint32_t), hipHostMallocDefault));
    s->m_cap = m;
    return CQS_HIP_OK;
}

static int32_t ensure_block(cqs_hip_index* x, hipStream_t st, uint32_t rows) {
    if (!x->mmr) {
        x->mmr = new (std::nothrow) Scratch();
        if (!x->mmr) return fail(x, CQS_HIP_ERR_NOMEM, "mmr: out of host memory");
    }
    Scratch* s = x->mmr;
    if (rows <= s->block_cap) return CQS_HIP_OK;
    if (st) HIP_TRY(x, hipStreamSynchronize(st));
    else HIP_TRY(x, hipDeviceSynchronize());
    (void)hipFree(s->d_block); (void)hipFree(s->d_bidx); (void)hipHostFree(s->h_bidx);
    s->d_block = nullptr; s->d_bidx = nullptr; s->h_bidx = nullptr; s->block_cap = 0;
    HIP_TRY(x, hipMalloc(&s->d_block, (size_t)rows * x->dim * sizeof(float)));
    HIP_TRY(x, hipMalloc(&s->d_bidx, (size_t)rows * sizeof(uint32_t)));
    HIP_TRY(x, hipHostMalloc((void**)&s->h_bidx, (size_t)rows * sizeof(uint32_t), hipHostMallocDefault));
    s->block_cap = rows;
    return CQS_HIP_OK;
}

int32_t run(cqs_hip_index* x, hipStream_t st, const float* src, const uint32_t* h_idx, const float* h_scores, uint32_t m,
            uint32_t limit, float lambda, float* out_gram, uint32_t* out_picks) {
    int32_t rc = ensure(x, st, m);
    if (rc != CQS_HIP_OK) return rc;
    Scratch* s = x->mmr;
    uint32_t* const h_idx_pin = s->h_io;
    float* const h_scores_pin = (float*)(s->h_io + s->m_cap);
    uint32_t* const h_picks_pin = s->h_io + 2 * (size_t)s->m_cap;
    if (h_idx) {
        for (uint32_t i = 0; i < m; ++i) h_idx_pin[i] = h_idx[i];
        HIP_TRY(x, hipMemcpyAsync(s->d_idx, h_idx_pin, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    GramParams p;
    p.rows = src; p.idx = h_idx ? s->d_idx : nullptr; p.m = m; p.dim = x->dim; p.tiles = (m + 31u) / 32u; p.gram = s->d_gram;
    hipLaunchKernelGGL(gram_gather_kernel, dim3(p.tiles * (p.tiles + 1u) / 2u), dim3(64), 0, st, p);
    HIP_TRY(x, hipGetLastError());
    if (out_gram) {
        HIP_TRY(x, hipMemcpyAsync(out_gram, s->d_gram, (size_t)m * m * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(x, hipStreamSynchronize(st));
        return CQS_HIP_OK;
    }
    for (uint32_t i = 0; i < m; ++i) h_scores_pin[i] = h_scores[i];
    HIP_TRY(x, hipMemcpyAsync(s->d_scores, h_scores_pin, (size_t)m * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mmr_greedy_kernel, dim3(1), dim3((m + 63u) / 64u * 64u), 0, st, s->d_gram, s->d_scores, m, limit, lambda,
                       s->d_picks);
    HIP_TRY(x, hipGetLastError());
    h_picks_pin[0] = 0xFFFFFFFFu;
    HIP_TRY(x, hipMemcpyAsync(h_picks_pin, s->d_picks, ((size_t)limit + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(x, hipStreamSynchronize(st));
    if (h_picks_pin[0] != limit) return fail(x, CQS_HIP_ERR_DEVICE, "mmr: the greedy kernel did not finish");
    for (uint32_t i = 0; i < limit; ++i) out_picks[i] = h_picks_pin[1 + i];
    return CQS_HIP_OK;
}

int32_t gather_rows(cqs_hip_index* c, const uint32_t* h_idx, uint32_t mc, const float** out_block) {
    const int32_t rc = ensure_block(c, c->stream, mc);
    if (rc != CQS_HIP_OK) return rc;
    Scratch* s = c->mmr;
    for (uint32_t i = 0; i < mc; ++i) s->h_bidx[i] = h_idx[i];
    HIP_TRY(c, hipMemcpyAsync(s->d_bidx, s->h_bidx, (size_t)mc * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const uint64_t pieces = (uint64_t)mc * (c->dim / 4u);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((uint32_t)((pieces + 255u) / 256u)), dim3(256), 0, c->stream, c->d_rows, s->d_bidx,
                       mc, c->dim, s->d_block);
    HIP_TRY(c, hipGetLastError());
    *out_block = s->d_block;
    return CQS_HIP_OK;
}

int32_t staging(cqs_hip_index* parent, uint32_t m, float** out_block) {
    const int32_t rc = ensure_block(parent, nullptr, m);
    if (rc == CQS_HIP_OK) *out_block = parent->mmr->d_block;
    return rc;
}

// The candidates' local rows (checked by mmr_host.h: every one inside the index).
static void local_rows(const cqs_hip_index* x, const uint64_t* cand_rows, uint32_t m, uint32_t* out) {
    for (uint32_t i = 0; i < m; ++i) out[i] = (uint32_t)(cand_rows[i] - x->row_base);
}

}  // namespace cqs_mmr

extern "C" {

// Pairwise dots of stored rows: the similarity `mmr_rerank` would use had the reference kept its embeddings
// (src/search/mmr.rs:30-37), as one [m, m] f32 matrix.
int32_t cqs_hip_index_pairwise(cqs_hip_index* x, const uint64_t* cand_rows, uint32_t m, float* out) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_pairwise");
    if (!x) return CQS_HIP_ERR_INVALID;
    if (x->sh) return cqs_sharded::pairwise(x, cand_rows, m, out);
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    const char* why = "";
    const cqs_mmr::Plan plan = cqs_mmr::check_rows(cand_rows, m, x->row_base, x->n, &why);
    if (plan == cqs_mmr::Plan::Invalid) return fail(x, CQS_HIP_ERR_INVALID, why);
    if (plan == cqs_mmr::Plan::Empty) return CQS_HIP_OK;
    if (!out) return fail(x, CQS_HIP_ERR_INVALID, "pairwise: null output buffer");
    uint32_t idx[CQS_HIP_MMR_MAX];
    cqs_mmr::local_rows(x, cand_rows, m, idx);
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, order_after_last(x, x->stream));
    const int32_t rc = cqs_mmr::run(x, x->stream, x->d_rows, idx, nullptr, m, 0, 0.f, out, nullptr);
    if (rc != CQS_HIP_OK) return rc;
    HIP_TRY(x, record_done(x, x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// `mmr_rerank` (src/search/mmr.rs:59-126) with similarity(i, j) = the dot of stored rows cand_rows[i], cand_rows[j].
int32_t cqs_hip_index_mmr(cqs_hip_index* x, const uint64_t* cand_rows, const float* cand_scores, uint32_t m, uint32_t limit,
                          float lambda, uint32_t* out_picks, uint32_t* out_count) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_mmr");
    if (!x || !out_count) return CQS_HIP_ERR_INVALID;
    if (x->sh) return cqs_sharded::mmr(x, cand_rows, cand_scores, m, limit, lambda, out_picks, out_count);
    std::lock_guard<std::mutex> g(x->mu);
    *out_count = 0;
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    const char* why = "";
    const cqs_mmr::Plan plan = cqs_mmr::plan_mmr(cand_rows, cand_scores, m, x->row_base, x->n, &limit, &lambda, &why);
    if (plan == cqs_mmr::Plan::Invalid) return fail(x, CQS_HIP_ERR_INVALID, why);
    if (plan == cqs_mmr::Plan::Empty) return CQS_HIP_OK;                       // mmr.rs:64-66
    if (!out_picks) return fail(x, CQS_HIP_ERR_INVALID, "mmr: null output buffer");
    if (plan == cqs_mmr::Plan::Identity) {                                     // mmr.rs:67-69
        for (uint32_t i = 0; i < limit; ++i) out_picks[i] = i;
        *out_count = limit;
        return CQS_HIP_OK;
    }
    uint32_t idx[CQS_HIP_MMR_MAX];
    cqs_mmr::local_rows(x, cand_rows, m, idx);
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, order_after_last(x, x->stream));
    const int32_t rc = cqs_mmr::run(x, x->stream, x->d_rows, idx, cand_scores, m, limit, lambda, nullptr, out_picks);
    if (rc != CQS_HIP_OK) return rc;
    HIP_TRY(x, record_done(x, x->stream));
    *out_count = limit;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

}  // extern "C"
