// sparse_index_update.hip — cqs_hip_sparse_index_remove / cqs_hip_sparse_index_extend: chunks leave and join the resident
// sparse index without a rebuild from the documents, so the sparse leg of a hybrid query follows the dense leg's
// remove / extend through a watch loop (the reference's reason for in-place updates: "clean orphaned vectors and absorb
// deltas", src/tiered.rs:13-17).  DESIGN.md §3.10a.
//
// The host plans (sparse_update_host.h): renumbering, token table, and the rule that gives every posting its place.  The
// device rewrites the posting array ONCE into a new array beside the old one - every posting read once and written once,
// a chunk's postings in their old order inside every list, so every score is still summed in the reference's order - then
// fills the range directories from the new array, and the handle swaps its arrays under `mu`.  Until the swap nothing of
// the handle changes: a refused argument or a failed allocation leaves the index as it was.
//
// Plain streaming kernels: vector loads and stores, wave ballots, one block scan.  Hand-offs between them are kernel
// boundaries on the handle's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "scan_kernels.h"
#include "sparse_internal.h"
#include "sparse_update_host.h"

namespace cqs {

namespace su = cqs_sparse_update;

constexpr uint32_t kUpdThreads = 256;
constexpr uint32_t kUpdTile = 2u * kUpdThreads;       // postings per tile: two per lane, one 16-byte load
constexpr uint32_t kUpdMaxBlocks = 256u * 16u;        // grid cap; the tiles beyond it are taken grid-stride
constexpr uint32_t kScanThreads = 1024;

// Postings e0 and e0 + 1 (e0 even, so the pair is 16-byte aligned); have_* says which exist.
__device__ __forceinline__ void load_pair(const uint2* __restrict__ post, uint64_t P, uint64_t e0, uint2& a, uint2& b, bool& have_a,
                                          bool& have_b) {
    have_a = e0 < P;
    have_b = e0 + 1u < P;
    a = b = make_uint2(0u, 0u);
    if (have_b) {
        const uint4 v = *reinterpret_cast<const uint4*>(post + e0);
        a = make_uint2(v.x, v.y);
        b = make_uint2(v.z, v.w);
    } else if (have_a) {
        a = post[e0];
    }
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---- remove --------------------------------------------------------------------------------------------------------------
// Pass 1: every posting read once; remap[] (4 B per chunk, cache-resident) says whether its chunk stays.  Kept postings
// per tile.
__global__ __launch_bounds__(kUpdThreads) void remove_count_kernel(const uint2* __restrict__ post, uint64_t P, const uint32_t* __restrict__ remap,
                                                                 uint64_t n_tiles, uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_w[kUpdThreads / 64];
    const int lane = threadIdx.x & 63;
    const uint32_t wid = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint2 a, b;
        bool ha, hb;
        load_pair(post, P, tile * kUpdTile + 2u * threadIdx.x, a, b, ha, hb);
        const bool ka = ha && remap[a.x] != su::kGone, kb = hb && remap[b.x] != su::kGone;
        const uint32_t c = (uint32_t)__popcll(__ballot(ka)) + (uint32_t)__popcll(__ballot(kb));
        if (lane == 0) s_w[wid] = c;
        __syncthreads();
        if (threadIdx.x == 0) tile_count[tile] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// prefix[i] = kept postings in tiles 0 .. i - 1, prefix[n_tiles] = all of them.  One workgroup walks the counts 1024 at a
// time (188 k tiles at 96 M postings: 184 steps).
__global__ __launch_bounds__(kScanThreads) void tile_scan_kernel(const uint32_t* __restrict__ tile_count, uint64_t n_tiles,
                                                               unsigned long long* __restrict__ prefix) {
    __shared__ uint32_t s_w[kScanThreads / 64];
    __shared__ unsigned long long s_carry;
    const int lane = threadIdx.x & 63;
    const uint32_t wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0ull;
    __syncthreads();
    for (uint64_t base = 0; base < n_tiles; base += kScanThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < n_tiles ? tile_count[i] : 0u;
        uint32_t x = v;                                    // inclusive scan inside the wave (1024 tiles hold < 2^20 postings)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[wid] = x;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
            if (w < wid) before += s_w[w];
            total += s_w[w];
        }
        const unsigned long long carry = s_carry;
        if (i < n_tiles) prefix[i] = carry + before + (x - v);
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) prefix[n_tiles] = s_carry;
}

// K at the list starts: k[t] = kept postings before old posting off[t], t = 0 .. lists (off[lists] = P).  The tile prefix
// plus a walk over the start's own tile (< kUpdTile postings).  The host makes the new token table from these.
__global__ void remove_starts_kernel(const uint2* __restrict__ post, const uint32_t* __restrict__ remap, const uint64_t* __restrict__ off,
                                     uint32_t lists, const unsigned long long* __restrict__ prefix, unsigned long long* __restrict__ k) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > lists) return;
    const uint64_t e = off[t];
    const uint64_t tile = e / kUpdTile;                    // (e = P on a tile boundary: prefix[n_tiles], nothing to walk)
    unsigned long long c = prefix[tile];
    for (uint64_t i = tile * kUpdTile; i < e; ++i) c += remap[post[i].x] != su::kGone ? 1u : 0u;
    k[t] = c;
}

// Pass 2: every kept posting, with its new position, to its place in the new array.  Its place is K(e) (remove_position):
// the tile's prefix, the kept postings of the waves in front (LDS), and of the lanes in front (ballot + mbcnt).
__global__ __launch_bounds__(kUpdThreads) void remove_write_kernel(const uint2* __restrict__ post, uint64_t P, const uint32_t* __restrict__ remap,
                                                                 uint64_t n_tiles, const unsigned long long* __restrict__ prefix,
                                                                 uint2* __restrict__ out) {
    __shared__ uint32_t s_w[kUpdThreads / 64];
    const int lane = threadIdx.x & 63;
    const uint32_t wid = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint2 a, b;
        bool ha, hb;
        load_pair(post, P, tile * kUpdTile + 2u * threadIdx.x, a, b, ha, hb);
        const uint32_t ra = ha ? remap[a.x] : su::kGone, rb = hb ? remap[b.x] : su::kGone;
        const bool ka = ra != su::kGone, kb = rb != su::kGone;
        const uint64_t ma = __ballot(ka), mb = __ballot(kb);
        if (lane == 0) s_w[wid] = (uint32_t)__popcll(ma) + (uint32_t)__popcll(mb);
        __syncthreads();
        uint32_t before = lanes_below(ma) + lanes_below(mb);
        for (uint32_t w = 0; w < wid; ++w) before += s_w[w];
        const uint64_t k_e = prefix[tile] + before;
        if (ka) out[su::remove_position(0ull, k_e, 0ull)] = make_uint2(ra, a.y);
        if (kb) out[su::remove_position(0ull, k_e + (ka ? 1u : 0u), 0ull)] = make_uint2(rb, b.y);
        __syncthreads();
    }
}

// ---- extend --------------------------------------------------------------------------------------------------------------
// The per-list tables of an extend, all on the device: the old offsets, where every old list sits in the merged table,
// the merged offsets, every merged list's slice of the added postings and its old list.
struct ExtendTables {
    const uint64_t* off_old;      // [old_lists + 1]
    const uint32_t* new_slot;     // [old_lists]
    const uint64_t* new_off;      // [lists + 1]
    const uint64_t* add_off;      // [lists + 1]
    const uint32_t* old_slot;     // [lists]
    const uint2* added;           // [add_off[lists]] {final position, weight bits}
    uint32_t old_lists;
};

__device__ __forceinline__ void place_old(const ExtendTables& x, const uint32_t* __restrict__ lift, uint64_t e, uint2 p, uint32_t t,
                                          uint2* __restrict__ out) {
    const uint32_t u = x.new_slot[t];
    const uint32_t lifted = lift[p.x];
    const uint64_t a0 = x.add_off[u];
    const uint32_t below = su::count_below(x.added + a0, (uint32_t)(x.add_off[u + 1u] - a0), lifted);
    out[su::extend_old_position(x.new_off[u], e - x.off_old[t], below)] = make_uint2(lifted, p.y);
}

// The old postings move: lifted position, plus the added postings of their list that sort in front.  The list of a lane's
// first posting by bisection of the offsets (the lanes of a wave walk the same few cache lines), of its second by a step.
__global__ __launch_bounds__(kUpdThreads) void extend_move_kernel(const uint2* __restrict__ post, uint64_t P, ExtendTables x,
                                                                const uint32_t* __restrict__ lift, uint64_t n_tiles, uint2* __restrict__ out) {
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t e0 = tile * kUpdTile + 2u * threadIdx.x;
        uint2 a, b;
        bool ha, hb;
        load_pair(post, P, e0, a, b, ha, hb);
        if (!ha) continue;
        uint32_t t = su::list_of(x.off_old, x.old_lists, e0);
        place_old(x, lift, e0, a, t, out);
        if (hb) {
            while (e0 + 1u >= x.off_old[t + 1u]) ++t;     // (e0 + 1 < P = off_old[old_lists] ends the walk)
            place_old(x, lift, e0 + 1u, b, t, out);
        }
    }
}

// The added postings take their places: behind the added postings of their list in front of them, and behind the old
// postings whose position is below their threshold.
__global__ __launch_bounds__(kUpdThreads) void extend_place_kernel(const uint2* __restrict__ post, ExtendTables x,
                                                                 const uint32_t* __restrict__ added_slot, const uint32_t* __restrict__ added_thr,
                                                                 uint64_t n_added, uint2* __restrict__ out) {
    for (uint64_t a = (uint64_t)blockIdx.x * kUpdThreads + threadIdx.x; a < n_added; a += (uint64_t)gridDim.x * kUpdThreads) {
        const uint32_t u = added_slot[a];
        const uint32_t t = x.old_slot[u];
        uint32_t below = 0u;
        if (t != su::kGone) {
            const uint64_t s0 = x.off_old[t];
            below = su::count_below(post + s0, (uint32_t)(x.off_old[t + 1u] - s0), added_thr[a]);
        }
        out[su::extend_added_position(x.new_off[u], a - x.add_off[u], below)] = x.added[a];
    }
}

// ---- range directories from the device's own postings ----------------------------------------------------------------------
// dir[r] of a list = its postings with position < r * rw.  One pass over the postings: posting i of a list, at position p
// with its predecessor at q, is the first at or above every edge q < r * rw <= p and writes dir[r] = i for those; the
// list's last posting also writes the entries behind it (= the list's length).  Every entry is written exactly once.
__global__ __launch_bounds__(kUpdThreads) void dir_fill_kernel(const uint2* __restrict__ post, uint64_t P, const uint64_t* __restrict__ off,
                                                             uint32_t lists, const uint64_t* __restrict__ dir_off, uint32_t sh, uint32_t R1,
                                                             uint32_t* __restrict__ dir) {
    for (uint64_t i = (uint64_t)blockIdx.x * kUpdThreads + threadIdx.x; i < P; i += (uint64_t)gridDim.x * kUpdThreads) {
        const uint32_t t = su::list_of(off, lists, i);
        const uint64_t d0 = dir_off[t];
        if (d0 == kNoDir) continue;
        const uint64_t s0 = off[t];
        const uint32_t li = (uint32_t)(i - s0);
        const uint32_t r_hi = post[i].x >> sh;             // (position < n <= n_pad: r_hi <= R1 - 2)
        uint32_t r = li ? (post[i - 1u].x >> sh) + 1u : 0u;
        for (; r <= r_hi; ++r) dir[d0 + r] = li;
        if (i + 1u == off[t + 1u])
            for (; r < R1; ++r) dir[d0 + r] = li + 1u;
    }
}

}  // namespace cqs

namespace {

namespace su = cqs_sparse_update;
using cqs_sparse::sfail;

struct DevBuf {       // freed on every way out unless handed to the handle
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T* as() const { return (T*)p; }
    template <class T> T* release() { T* r = (T*)p; p = nullptr; return r; }
};
struct StreamDrain {  // declared behind the buffers of a scope: whatever way out, the stream is idle before they are freed
    hipStream_t st;
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
};
struct PinBuf {
    void* p = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

// `bytes` of host memory into a fresh device buffer, on the handle's stream (the host memory outlives the next sync).
int32_t upload(cqs_hip_sparse_index* s, DevBuf& d, const void* src, size_t bytes) {
    S_TRY(s, hipMalloc(&d.p, std::max<size_t>(bytes, 8)));
    if (bytes) S_TRY(s, hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, s->stream));
    return CQS_HIP_OK;
}

uint32_t blocks_for(uint64_t items, uint32_t per_block) {
    const uint64_t b = (items + per_block - 1) / per_block;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(b, 1), cqs::kUpdMaxBlocks);
}

// The updated index, built beside the one the handle serves from.
struct NewIndex {
    uint64_t n = 0, P = 0;
    std::vector<uint32_t> tok;
    std::vector<uint64_t> off;
    std::vector<uint32_t> chunk_of_rank;
    DevBuf d_post, d_chunk_of_rank;
};

int32_t upload_chunk_of_rank(cqs_hip_sparse_index* s, NewIndex& nx) {
    if (!s->ranked) return CQS_HIP_OK;
    return upload(s, nx.d_chunk_of_rank, nx.chunk_of_rank.data(), nx.chunk_of_rank.size() * 4);
}

// Last step of both updates; the rewrite kernels are queued on the stream.  Geometry and directory plan for the new chunk
// count and list lengths by the constructors' own code (sparse_geometry.h), the directories filled on the device, the
// buffers whose size follows n_pad / the group size allocated anew - and only then, with nothing left that can refuse, the swap.
int32_t install(cqs_hip_sparse_index* s, NewIndex& nx) {
    const cqs::SparseGeometry geo = cqs::sparse_geometry(nx.n, s->n_cu);
    std::vector<uint64_t> dir_off;
    const uint64_t used = cqs::sparse_plan_directories(nx.off, geo, &dir_off);
    const uint32_t R1 = geo.n_pad / geo.rw + 1u;
    DevBuf d_dir, d_off, d_dir_off, d_keep, d_scores, d_gmax;
    PinBuf h_keep;
    StreamDrain drain{s->stream};
    S_TRY(s, hipMalloc(&d_dir.p, std::max<size_t>((size_t)used, 1) * 4));
    if (used) {
        int32_t rc = upload(s, d_off, nx.off.data(), nx.off.size() * 8);
        if (rc == CQS_HIP_OK) rc = upload(s, d_dir_off, dir_off.data(), dir_off.size() * 8);
        if (rc != CQS_HIP_OK) return rc;
        cqs::dir_fill_kernel<<<blocks_for(nx.P, cqs::kUpdThreads), cqs::kUpdThreads, 0, s->stream>>>(
            nx.d_post.as<uint2>(), nx.P, d_off.as<uint64_t>(), (uint32_t)nx.tok.size(), d_dir_off.as<uint64_t>(), geo.sh, R1, d_dir.as<uint32_t>());
        S_TRY(s, hipGetLastError());
    }
    const bool new_pad = geo.n_pad != s->n_pad;
    const bool new_rows = new_pad || geo.group16 != s->group16;
    if (new_pad) {
        S_TRY(s, hipMalloc(&d_keep.p, (size_t)(geo.n_pad / 32u) * 4));
        S_TRY(s, hipHostMalloc(&h_keep.p, (size_t)(geo.n_pad / 32u) * 4, hipHostMallocDefault));
    }
    if (new_rows && s->b_cap) {                            // the score rows and maxima of ensure_batch, for the queries it holds now
        const size_t groups = geo.n_pad / (geo.group16 ? 16u : 64u);
        S_TRY(s, hipMalloc(&d_scores.p, (size_t)s->b_cap * geo.n_pad * 4));
        S_TRY(s, hipMalloc(&d_gmax.p, (size_t)s->b_cap * groups * 12));
    }
    S_TRY(s, hipMemsetAsync(s->d_work, 0, cqs::kWorkWords * 4, s->stream));
    const hipError_t he = hipStreamSynchronize(s->stream);
    if (he != hipSuccess) return sfail(s, CQS_HIP_ERR_DEVICE, "sparse update: rewrite failed", he);
    // the swap: under mu, the stream idle
    (void)hipFree(s->d_post);
    (void)hipFree(s->d_dir);
    if (s->d_chunk_of_rank) (void)hipFree(s->d_chunk_of_rank);
    s->d_post = nx.d_post.release<uint2>();
    s->d_dir = d_dir.release<uint32_t>();
    s->d_chunk_of_rank = s->ranked ? nx.d_chunk_of_rank.release<uint32_t>() : nullptr;
    if (new_pad) {
        (void)hipFree(s->d_keep);
        (void)hipHostFree(s->h_keep);
        s->d_keep = d_keep.release<uint32_t>();
        s->h_keep = (uint32_t*)h_keep.p;
        h_keep.p = nullptr;
    }
    if (new_rows && s->b_cap) {
        (void)hipFree(s->d_scores);
        (void)hipFree(s->d_gmax);
        s->d_scores = d_scores.release<float>();
        s->d_gmax = d_gmax.release<float>();
    }
    s->n = nx.n;
    s->n_postings = nx.P;
    s->n_pad = geo.n_pad;
    s->rw = geo.rw;
    s->sh = geo.sh;
    s->group16 = geo.group16;
    s->tok.swap(nx.tok);
    s->off.swap(nx.off);
    s->chunk_of_rank.swap(nx.chunk_of_rank);
    s->dir_off.swap(dir_off);
    s->dir_entries = used;
    return CQS_HIP_OK;
}

// Caller holds mu and has checked the handle and the plan.
int32_t remove_locked(cqs_hip_sparse_index* s, su::RemovePlan& plan) {
    S_TRY(s, hipSetDevice(s->device));
    S_TRY(s, hipStreamSynchronize(s->stream));
    const uint64_t P = s->n_postings;
    const uint32_t lists = (uint32_t)s->tok.size();
    const uint64_t n_tiles = (P + cqs::kUpdTile - 1) / cqs::kUpdTile;
    std::vector<uint64_t> k((size_t)lists + 1, 0);
    DevBuf d_remap, d_count, d_prefix, d_off, d_k;
    NewIndex nx;
    StreamDrain drain{s->stream};
    if (P) {
        int32_t rc = upload(s, d_remap, plan.remap.data(), plan.remap.size() * 4);
        if (rc == CQS_HIP_OK) rc = upload(s, d_off, s->off.data(), s->off.size() * 8);
        if (rc != CQS_HIP_OK) return rc;
        S_TRY(s, hipMalloc(&d_count.p, (size_t)n_tiles * 4));
        S_TRY(s, hipMalloc(&d_prefix.p, ((size_t)n_tiles + 1) * 8));
        S_TRY(s, hipMalloc(&d_k.p, k.size() * 8));
        cqs::remove_count_kernel<<<blocks_for(n_tiles, 1), cqs::kUpdThreads, 0, s->stream>>>(s->d_post, P, d_remap.as<uint32_t>(), n_tiles,
                                                                                         d_count.as<uint32_t>());
        S_TRY(s, hipGetLastError());
        cqs::tile_scan_kernel<<<1, cqs::kScanThreads, 0, s->stream>>>(d_count.as<uint32_t>(), n_tiles, d_prefix.as<unsigned long long>());
        S_TRY(s, hipGetLastError());
        cqs::remove_starts_kernel<<<(lists + 1u + 255u) / 256u, 256, 0, s->stream>>>(s->d_post, d_remap.as<uint32_t>(), d_off.as<uint64_t>(), lists,
                                                                                  d_prefix.as<unsigned long long>(), d_k.as<unsigned long long>());
        S_TRY(s, hipGetLastError());
        // the call's only copy back: K at the list starts, (tokens + 1) x 8 B
        S_TRY(s, hipMemcpyAsync(k.data(), d_k.p, k.size() * 8, hipMemcpyDeviceToHost, s->stream));
        S_TRY(s, hipStreamSynchronize(s->stream));
    }
    nx.n = plan.n_new;
    su::remove_token_table(s->tok, k, &nx.tok, &nx.off);
    nx.P = nx.off.back();
    if (nx.P > P) return sfail(s, CQS_HIP_ERR_DEVICE, "sparse remove: kept more postings than the index holds");
    nx.chunk_of_rank.swap(plan.chunk_of_rank);
    S_TRY(s, hipMalloc(&nx.d_post.p, std::max<size_t>((size_t)nx.P, 1) * sizeof(uint2)));
    if (nx.P) {
        cqs::remove_write_kernel<<<blocks_for(n_tiles, 1), cqs::kUpdThreads, 0, s->stream>>>(
            s->d_post, P, d_remap.as<uint32_t>(), n_tiles, d_prefix.as<unsigned long long>(), nx.d_post.as<uint2>());
        S_TRY(s, hipGetLastError());
    }
    const int32_t rc = upload_chunk_of_rank(s, nx);
    if (rc != CQS_HIP_OK) return rc;
    return install(s, nx);
}

int32_t extend_locked(cqs_hip_sparse_index* s, su::ExtendPlan& plan) {
    S_TRY(s, hipSetDevice(s->device));
    S_TRY(s, hipStreamSynchronize(s->stream));
    const uint64_t P = s->n_postings, PA = plan.added.size();
    NewIndex nx;
    DevBuf d_off_old, d_new_slot, d_new_off, d_add_off, d_old_slot, d_added, d_added_slot, d_added_thr, d_lift;
    StreamDrain drain{s->stream};
    nx.n = plan.n_total;
    nx.tok.swap(plan.tok);
    nx.off.swap(plan.off);
    nx.P = nx.off.back();
    nx.chunk_of_rank.swap(plan.chunk_of_rank);
    int32_t rc = upload(s, d_off_old, s->off.data(), s->off.size() * 8);
    if (rc == CQS_HIP_OK) rc = upload(s, d_new_slot, plan.new_slot.data(), plan.new_slot.size() * 4);
    if (rc == CQS_HIP_OK) rc = upload(s, d_new_off, nx.off.data(), nx.off.size() * 8);
    if (rc == CQS_HIP_OK) rc = upload(s, d_add_off, plan.add_off.data(), plan.add_off.size() * 8);
    if (rc == CQS_HIP_OK) rc = upload(s, d_old_slot, plan.old_slot.data(), plan.old_slot.size() * 4);
    if (rc == CQS_HIP_OK) rc = upload(s, d_added, plan.added.data(), (size_t)PA * sizeof(su::Posting));
    if (rc == CQS_HIP_OK) rc = upload(s, d_added_slot, plan.added_slot.data(), (size_t)PA * 4);
    if (rc == CQS_HIP_OK) rc = upload(s, d_added_thr, plan.added_thr.data(), (size_t)PA * 4);
    if (rc == CQS_HIP_OK) rc = upload(s, d_lift, plan.lift.data(), plan.lift.size() * 4);
    if (rc != CQS_HIP_OK) return rc;
    S_TRY(s, hipMalloc(&nx.d_post.p, std::max<size_t>((size_t)nx.P, 1) * sizeof(uint2)));
    const cqs::ExtendTables x{d_off_old.as<uint64_t>(), d_new_slot.as<uint32_t>(), d_new_off.as<uint64_t>(), d_add_off.as<uint64_t>(),
                              d_old_slot.as<uint32_t>(), d_added.as<uint2>(), (uint32_t)s->tok.size()};
    if (P) {
        const uint64_t n_tiles = (P + cqs::kUpdTile - 1) / cqs::kUpdTile;
        cqs::extend_move_kernel<<<blocks_for(n_tiles, 1), cqs::kUpdThreads, 0, s->stream>>>(s->d_post, P, x, d_lift.as<uint32_t>(), n_tiles,
                                                                                        nx.d_post.as<uint2>());
        S_TRY(s, hipGetLastError());
    }
    if (PA) {
        cqs::extend_place_kernel<<<blocks_for(PA, cqs::kUpdThreads), cqs::kUpdThreads, 0, s->stream>>>(
            s->d_post, x, d_added_slot.as<uint32_t>(), d_added_thr.as<uint32_t>(), PA, nx.d_post.as<uint2>());
        S_TRY(s, hipGetLastError());
    }
    rc = upload_chunk_of_rank(s, nx);
    if (rc != CQS_HIP_OK) return rc;
    return install(s, nx);   // (synchronises the stream before the tables above go)
}

}  // namespace

extern "C" {

int32_t cqs_hip_sparse_index_remove(cqs_hip_sparse_index* s, const uint64_t* chunks, uint64_t m, uint64_t* out_removed) CQS_ABI_TRY {
    if (!s) return CQS_HIP_ERR_INVALID;
    if (out_removed) *out_removed = 0;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    su::RemovePlan plan;
    const char* why = "";
    const su::Plan p = su::plan_remove(chunks, m, s->n, s->chunk_of_rank, &plan, &why);
    if (p == su::Plan::Invalid) return sfail(s, CQS_HIP_ERR_INVALID, std::string("sparse remove: ") + why);
    if (p == su::Plan::Nothing) return CQS_HIP_OK;
    const int32_t rc = remove_locked(s, plan);   // (takes plan.chunk_of_rank; plan.removed stays)
    if (rc == CQS_HIP_OK) cqs_sparse::tags_after_remove(s, plan.removed);
    if (rc == CQS_HIP_OK && out_removed) *out_removed = plan.removed.size();
    return rc;
} CQS_ABI_CATCH(s)

int32_t cqs_hip_sparse_index_extend(cqs_hip_sparse_index* s, const uint64_t* doc_off, const uint32_t* tokens, const float* weights,
                                    uint64_t n_new, const uint32_t* new_rank) CQS_ABI_TRY {
    if (!s) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    su::ExtendPlan plan;
    const char* why = "";
    const su::Plan p = su::plan_extend(doc_off, tokens, weights, n_new, new_rank, s->n, s->ranked, s->chunk_of_rank, s->tok, s->off, &plan, &why);
    if (p == su::Plan::Invalid) return sfail(s, CQS_HIP_ERR_INVALID, std::string("sparse extend: ") + why);
    if (p == su::Plan::Nothing) return CQS_HIP_OK;
    const int32_t rc = extend_locked(s, plan);
    if (rc == CQS_HIP_OK) cqs_sparse::tags_after_extend(s);
    return rc;
} CQS_ABI_CATCH(s)

}  // extern "C"
