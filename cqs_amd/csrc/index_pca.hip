// index_pca.hip — cqs_hip_index_pca / cqs_hip_index_pca_project (include/cqs_hip.h "PCA of the stored rows", DESIGN.md
// §3.18b): the top principal axes of the resident corpus by block subspace iteration.  The host steps (Gram-Schmidt, the
// 8 x 8 eigen-solve, the refusals) are pca_host.h's; here are the launches between them:
//   moments_kernel  one pass: per slab of 1024 rows the column sums and the squared length of x - x_0 (x_0 = stored row 0), f64
//   pass_kernel     the hot path, once per pass: per slab Y = sum (x - x_0) (x) t and S = sum t, t = (x - x_0) V - c
//   reduce_kernel   the slab partials added in ascending slab order in f64
//   project_kernel  (x - mean) . axis_k per stored row
// No float atomics: every partial is written by one workgroup and added in an order fixed here, so the answer is a function
// of the stored rows, the seed and the pass count only.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "abi_guard.h"
#include "index_internal.h"
#include "pca_host.h"
#include "roctx.h"
#include "wave_ops.h"

namespace cqs_pca {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 256;                         // four waves a workgroup, in every kernel of this file
constexpr uint32_t kMomentTiles = 4;                      // 4096 / (4 * 256): the mean pass's workgroups per slab at the largest dim
constexpr uint32_t kMaxChunks = kTileDims / 16 / 4;        // 16-column chunks of the tile a wave accumulates (second product)

// LDS row stride of the staged batch, in floats: a multiple of 4 (the staging stores are 16 bytes) that is 20 mod 32, so
// the first product's reads (16 rows x 2 neighbouring columns per half-wave) fall on each bank at most twice.
__host__ __device__ inline uint32_t tile_stride(uint32_t tile_dims) { return tile_dims + ((20u + 32u - tile_dims % 32u) % 32u); }
inline size_t pass_lds_bytes(uint32_t tile_dims) { return ((size_t)kBatchRows * tile_stride(tile_dims) + 4u * 256u) * sizeof(float); }

// ---- the mean pass ----------------------------------------------------------------------------------------------------------
// Workgroup (slab, g): thread t owns the float4 column 256 g + t and adds x - x_0 and its squares over the slab's rows in
// row order, in f64 (the differences are exact there, and the f64 adds run at the f32 rate on this device).  The squares
// of the workgroup's threads are added in thread order.  part[slab][0 .. dim) = the column sums, part[slab][dim + g] = the
// squares of the columns of g.
__global__ __launch_bounds__(kThreads) void moments_kernel(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                           double* __restrict__ part) {
    __shared__ double squares[kThreads];
    const uint64_t row0 = (uint64_t)blockIdx.x * kSlabRows;
    const uint64_t row_end = row0 + kSlabRows < n ? row0 + kSlabRows : n;
    const uint32_t col = 4u * (blockIdx.y * kThreads + threadIdx.x);
    double* __restrict__ out = part + (size_t)blockIdx.x * (dim + kMomentTiles);
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0, sq = 0.0;
    if (col < dim) {
        const float4 x0 = *(const float4*)(rows + col);
#pragma unroll 8
        for (uint64_t r = row0; r < row_end; ++r) {
            const float4 v = *(const float4*)(rows + (size_t)r * dim + col);
            const double a = (double)v.x - (double)x0.x, b = (double)v.y - (double)x0.y, c = (double)v.z - (double)x0.z,
                         d = (double)v.w - (double)x0.w;
            sx += a; sy += b; sz += c; sw += d;
            sq += a * a; sq += b * b; sq += c * c; sq += d * d;
        }
        out[col] = sx; out[col + 1u] = sy; out[col + 2u] = sz; out[col + 3u] = sw;
    }
    squares[threadIdx.x] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (uint32_t t = 0; t < kThreads; ++t) s += squares[t];
        out[dim + blockIdx.y] = s;
    }
}

// ---- the pass ---------------------------------------------------------------------------------------------------------------
struct PassParams {
    const float* rows;   // [n][dim]
    uint64_t n;
    uint32_t dim;
    uint32_t tiles;      // ceil(dim / kTileDims) = gridDim.y
    const float* v;      // [dim][8] the block, f32
    const float* neg_c;  // [8] -(mu - x_0)^T V
    float* part;         // [slabs][dim * 8 + 8]: Y [dim][8], then S [8]
};

// The batch's rows of tile `tt`, minus x_0, into the LDS image: thread t owns the float4 column t of the tile.  `live` of
// the batch's 16 rows exist (the slab's last batch can be short); the others are staged as zeros.
__device__ __forceinline__ void stage_tile(const PassParams& p, float* tile, uint32_t stride, uint32_t tt, uint64_t first, uint32_t live) {
    const uint32_t dt0 = tt * kTileDims;
    const uint32_t tdt = p.dim - dt0 < kTileDims ? p.dim - dt0 : kTileDims;
    const uint32_t col = 4u * threadIdx.x;
    if (col >= tdt) return;
    const float4 x0 = *(const float4*)(p.rows + dt0 + col);
    const float* __restrict__ src = p.rows + (size_t)first * p.dim + dt0 + col;   // this thread's column of the batch's first row
    float* __restrict__ dst = tile + col;
    for (uint32_t half = 0; half < kBatchRows; half += 8u) {   // eight loads in flight a thread
        float4 x[8];
#pragma unroll
        for (uint32_t r = 0; r < 8u; ++r) x[r] = half + r < live ? *(const float4*)(src + (size_t)(half + r) * p.dim) : x0;
#pragma unroll
        for (uint32_t r = 0; r < 8u; ++r)
            *(float4*)(dst + (half + r) * stride) = half + r < live ? make_float4(x[r].x - x0.x, x[r].y - x0.y, x[r].z - x0.z, x[r].w - x0.w)
                                                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Workgroup (slab, g): the slab's rows in batches of 16, and the columns [1024 g, 1024 g + 1024) of Y.  Per batch the
// rows go to LDS once (minus x_0) and are used twice by the f32 matrix cores (v_mfma_f32_16x16x4_f32: a k-ordered fmaf
// chain, one rounding per product):
//   first product   T[16 rows][8] = X' V - c.  M = rows, N = the 8 columns (the other 8 of the tile are zero), K = the
//                   corpus columns in steps of 4; wave w runs the k-steps w, w + 4, ... in ascending order, wave 0's chain
//                   starting from -c, and the four chains are added as ((w0 + w1) + w2) + w3 through LDS.  dim > 1024:
//                   the tiles 0, 1, ... pass through the LDS image one after the other and the chains run on; every
//                   workgroup of a slab computes the same T.
//   second product  Y[16 columns][8] += X'^T T per 16-column chunk of the tile: M = columns, K = the batch's rows in steps
//                   of 4 ascending; wave w owns the chunks w, w + 4, ... and keeps their accumulators in registers for the
//                   whole slab, so a Y entry is one chain over the slab's rows in row order.
// S adds a row's t in the same row grouping: lane (k, j) adds rows k, k + 4, k + 8, k + 12 of each batch in turn, then
// ((k0 + k1) + k2) + k3.  Rows past the slab's end have t forced to 0.
__global__ __launch_bounds__(kThreads) void pass_kernel(const PassParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t li = lane & 15u, lk = lane >> 4;
    const uint32_t g = blockIdx.y;
    const uint32_t d0 = g * kTileDims;
    const uint32_t td = p.dim - d0 < kTileDims ? p.dim - d0 : kTileDims;
    const uint32_t stride = tile_stride(p.dim < kTileDims ? p.dim : kTileDims);
    float* tile = lds;
    float* tpart = lds + kBatchRows * stride;   // [4 waves][16 rows][16 columns]
    const uint64_t row0 = (uint64_t)blockIdx.x * kSlabRows;
    const uint64_t row_end = row0 + kSlabRows < p.n ? row0 + kSlabRows : p.n;

    const float c_start = (w == 0 && li < kBlock) ? p.neg_c[li] : 0.f;
    f32x4 yacc[kMaxChunks];
#pragma unroll
    for (uint32_t i = 0; i < kMaxChunks; ++i) yacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ssum[4] = {0.f, 0.f, 0.f, 0.f};

    for (uint64_t first = row0; first < row_end; first += kBatchRows) {
        f32x4 acc = f32x4{c_start, c_start, c_start, c_start};
        const uint32_t live = row_end - first < kBatchRows ? (uint32_t)(row_end - first) : kBatchRows;
        for (uint32_t tt = 0; tt < p.tiles; ++tt) {
            if (tt) __syncthreads();   // (the previous tile's reads)
            stage_tile(p, tile, stride, tt, first, live);
            __syncthreads();
            const uint32_t dt0 = tt * kTileDims;
            const uint32_t ksteps = (p.dim - dt0 < kTileDims ? p.dim - dt0 : kTileDims) / 4u;
            const float* __restrict__ vcol = p.v + (size_t)(dt0 + lk) * kBlock + (li & 7u);   // B operand: V[4 ks + lk][li], 0 for li >= 8
            for (uint32_t ks = w; ks < ksteps; ks += 4u) {
                const float vb = vcol[(size_t)ks * 4u * kBlock];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[li * stride + 4u * ks + lk], li < kBlock ? vb : 0.f, acc, 0, 0, 0);
            }
        }
        if (g + 1u != p.tiles) {       // the own tile back into the image (dim > 1024 only)
            __syncthreads();
            stage_tile(p, tile, stride, g, first, live);
        }
        // D of the first product: row 4 lk + reg, column li
#pragma unroll
        for (uint32_t reg = 0; reg < 4u; ++reg) tpart[w * 256u + (4u * lk + reg) * 16u + li] = acc[reg];
        __syncthreads();
        float tb[4];                   // B operand of the second product: lane holds t[row 4 kk + lk][li]
#pragma unroll
        for (uint32_t kk = 0; kk < 4u; ++kk) {
            const uint32_t row = 4u * kk + lk, at = row * 16u + li;
            const float t = ((tpart[at] + tpart[256u + at]) + tpart[512u + at]) + tpart[768u + at];
            tb[kk] = row < live ? t : 0.f;
            ssum[kk] += tb[kk];
        }
#pragma unroll
        for (uint32_t i = 0; i < kMaxChunks; ++i) {
            const uint32_t c = w + 4u * i;
            if (16u * c < td) {
                const uint32_t col = 16u * c + li;
#pragma unroll
                for (uint32_t kk = 0; kk < 4u; ++kk) {
                    const float a = col < td ? tile[(4u * kk + lk) * stride + col] : 0.f;
                    yacc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tb[kk], yacc[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();               // (before the next batch overwrites the image and tpart)
    }

    float* __restrict__ out = p.part + (size_t)blockIdx.x * ((size_t)p.dim * kBlock + kBlock);
#pragma unroll
    for (uint32_t i = 0; i < kMaxChunks; ++i) {
        const uint32_t c = w + 4u * i;
        if (16u * c < td) {
#pragma unroll
            for (uint32_t reg = 0; reg < 4u; ++reg) {
                const uint32_t col = 16u * c + 4u * lk + reg;
                if (col < td && li < kBlock) out[(size_t)(d0 + col) * kBlock + li] = yacc[i][reg];
            }
        }
    }
    if (w == 0) tpart[lane] = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
    __syncthreads();
    if (g == 0 && threadIdx.x < kBlock) {
        const uint32_t j = threadIdx.x;
        out[(size_t)p.dim * kBlock + j] = ((tpart[j] + tpart[16u + j]) + tpart[32u + j]) + tpart[48u + j];
    }
}

// out[e] = part[0][e] + part[1][e] + ... in f64, ascending slab order; one thread per entry.
template <class T>
__global__ __launch_bounds__(kThreads) void reduce_kernel(const T* __restrict__ part, uint64_t slabs, uint32_t width,
                                                          double* __restrict__ out) {
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= width) return;
    double s = 0.0;
#pragma unroll 16
    for (uint64_t sl = 0; sl < slabs; ++sl) s += (double)part[sl * width + e];   // (the loads ahead, the adds in order)
    out[e] = s;
}

// ---- the projection ---------------------------------------------------------------------------------------------------------
// One wave per row, four to a workgroup.  Lane l adds (x - mean) * axis over the float4 columns l, l + 64, ... in ascending
// order, x, y, z, w in turn, as fmaf chains; the lanes then add as v += v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.
template <uint32_t NC>
__global__ __launch_bounds__(kThreads) void project_kernel(const float* __restrict__ rows, uint64_t first, uint64_t m, uint32_t dim,
                                                           const float* __restrict__ mean, const float* __restrict__ axes,
                                                           float* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= m) return;   // (the whole wave)
    const float4* __restrict__ x = (const float4*)(rows + (size_t)(first + i) * dim);
    float s[NC];
#pragma unroll
    for (uint32_t k = 0; k < NC; ++k) s[k] = 0.f;
    for (uint32_t c4 = lane; c4 < dim / 4u; c4 += 64u) {
        const float4 v = x[c4], mu = ((const float4*)mean)[c4];
        const float a = v.x - mu.x, b = v.y - mu.y, c = v.z - mu.z, d = v.w - mu.w;
#pragma unroll
        for (uint32_t k = 0; k < NC; ++k) {
            const float4 ax = ((const float4*)(axes + (size_t)k * dim))[c4];
            s[k] = fmaf(a, ax.x, s[k]);
            s[k] = fmaf(b, ax.y, s[k]);
            s[k] = fmaf(c, ax.z, s[k]);
            s[k] = fmaf(d, ax.w, s[k]);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < NC; ++k) {
        const float t = cqs::wave_sum64_shfl(s[k]);
        if (lane == 0) out[i * NC + k] = t;
    }
}

namespace {

struct DeviceBlock {   // freed on every way out
    void* p = nullptr;
    ~DeviceBlock() { if (p) (void)hipFree(p); }
};

Handle handle_of(const cqs_hip_index* x) {
    if (!x) return Handle{false, false, 0, 0, 0};
    return Handle{true, x->sh != nullptr, x->row_base, x->sh ? cqs_sharded::len(x) : x->n, x->dim};
}

size_t round16(size_t bytes) { return (bytes + 15u) / 16u * 16u; }

}  // namespace
}  // namespace cqs_pca

using cqs_idx::fail;
using namespace cqs_pca;

extern "C" {

int32_t cqs_hip_index_pca(cqs_hip_index* x, uint32_t n_components, uint32_t n_passes, uint64_t seed, float* out_mean,
                          float* out_axes, float* out_variance, float* out_total_variance) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_pca");
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);   // held for the whole call: every pass sees the same rows
    if (x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    Planned pl;
    const char* why = "";
    if (!plan_pca(handle_of(x), n_components, n_passes, out_mean && out_axes && out_variance && out_total_variance, &pl, &why))
        return fail(x, CQS_HIP_ERR_INVALID, why);
    const uint64_t n = x->n;
    const uint32_t dim = x->dim;
    const uint64_t slabs = slabs_of(n);
    const uint32_t tiles = (dim + kTileDims - 1) / kTileDims;
    const uint32_t width = dim * kBlock + kBlock;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, cqs_idx::order_after_last(x, x->stream));
    // one block: V, -c, the slab partials (the mean pass's fit in the same space), the f64 sums
    const size_t v_bytes = round16((size_t)dim * kBlock * sizeof(float)), c_bytes = 64;
    const size_t part_bytes = round16((size_t)slabs * width * sizeof(float)), sum_bytes = (size_t)(width + kMomentTiles) * sizeof(double);
    DeviceBlock blk;
    HIP_TRY(x, hipMalloc(&blk.p, v_bytes + c_bytes + part_bytes + sum_bytes));
    float* d_v = (float*)blk.p;
    float* d_c = (float*)((char*)blk.p + v_bytes);
    float* d_part = (float*)((char*)blk.p + v_bytes + c_bytes);
    double* d_sum = (double*)((char*)blk.p + v_bytes + c_bytes + part_bytes);
    const size_t lds = pass_lds_bytes(dim < kTileDims ? dim : kTileDims);
    HIP_TRY(x, hipFuncSetAttribute((const void*)pass_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    // the mean pass (its f64 partials, [slabs][dim + 4], fit in the passes' space)
    const uint32_t mwidth = dim + kMomentTiles, mtiles = (dim / 4u + kThreads - 1) / kThreads;
    std::vector<double> sums(width > mwidth ? width : mwidth);
    std::vector<float> x0(dim);
    HIP_TRY(x, hipMemsetAsync(d_part, 0, (size_t)slabs * mwidth * sizeof(double), x->stream));
    hipLaunchKernelGGL(moments_kernel, dim3((uint32_t)slabs, mtiles), dim3(kThreads), 0, x->stream, x->d_rows, n, dim, (double*)d_part);
    HIP_TRY(x, hipGetLastError());
    hipLaunchKernelGGL(reduce_kernel<double>, dim3((mwidth + kThreads - 1) / kThreads), dim3(kThreads), 0, x->stream, (const double*)d_part, slabs, mwidth, d_sum);
    HIP_TRY(x, hipGetLastError());
    HIP_TRY(x, hipMemcpyAsync(sums.data(), d_sum, (size_t)mwidth * sizeof(double), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipMemcpyAsync(x0.data(), x->d_rows, (size_t)dim * sizeof(float), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    const double squares = ((sums[dim] + sums[dim + 1u]) + sums[dim + 2u]) + sums[dim + 3u];
    std::vector<double> shift_mean(dim);
    double mean_sq = 0.0;
    for (uint32_t d = 0; d < dim; ++d) {
        shift_mean[d] = sums[d] / (double)n;
        mean_sq += shift_mean[d] * shift_mean[d];
    }
    const double total = (squares - (double)n * mean_sq) / (double)(n - 1);

    // the passes
    std::vector<double> v((size_t)dim * kBlock), y((size_t)dim * kBlock);
    std::vector<float> v32((size_t)dim * kBlock), axes((size_t)n_components * dim);
    float neg_c[kBlock], variance[CQS_HIP_PCA_MAX_COMPONENTS];
    start_block(seed, dim, pl.p, v.data());
    PassParams pp;
    pp.rows = x->d_rows; pp.n = n; pp.dim = dim; pp.tiles = tiles; pp.v = d_v; pp.neg_c = d_c; pp.part = d_part;
    for (uint32_t pass = 0; pass <= pl.passes; ++pass) {
        device_block(v.data(), shift_mean.data(), dim, v32.data(), neg_c);
        HIP_TRY(x, hipMemcpyAsync(d_v, v32.data(), (size_t)dim * kBlock * sizeof(float), hipMemcpyHostToDevice, x->stream));
        HIP_TRY(x, hipMemcpyAsync(d_c, neg_c, sizeof neg_c, hipMemcpyHostToDevice, x->stream));
        hipLaunchKernelGGL(pass_kernel, dim3((uint32_t)slabs, tiles), dim3(kThreads), lds, x->stream, pp);
        HIP_TRY(x, hipGetLastError());
        hipLaunchKernelGGL(reduce_kernel<float>, dim3((width + kThreads - 1) / kThreads), dim3(kThreads), 0, x->stream, d_part, slabs, width, d_sum);
        HIP_TRY(x, hipGetLastError());
        HIP_TRY(x, hipMemcpyAsync(sums.data(), d_sum, (size_t)width * sizeof(double), hipMemcpyDeviceToHost, x->stream));
        HIP_TRY(x, hipStreamSynchronize(x->stream));
        for (size_t i = 0; i < (size_t)dim * kBlock; ++i) y[i] = sums[i];
        centre_pass(y.data(), sums.data() + (size_t)dim * kBlock, shift_mean.data(), dim);
        if (pass < pl.passes) {
            v = y;
            gram_schmidt(v.data(), dim, pl.p);
        }
    }
    // (the last pass ran on the f32 rounding of v: the Rayleigh values are those of the block the device saw)
    for (size_t i = 0; i < (size_t)dim * kBlock; ++i) v[i] = (double)v32[i];
    if (!std::isfinite((float)total) || !finish(v.data(), y.data(), dim, pl.p, n, n_components, axes.data(), variance))
        return fail(x, CQS_HIP_ERR_INVALID, "pca: non-finite rows");
    for (uint32_t d = 0; d < dim; ++d) out_mean[d] = (float)((double)x0[d] + shift_mean[d]);
    memcpy(out_axes, axes.data(), axes.size() * sizeof(float));
    memcpy(out_variance, variance, n_components * sizeof(float));
    *out_total_variance = (float)total;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

int32_t cqs_hip_index_pca_project(cqs_hip_index* x, const float* mean, const float* axes, uint32_t n_components,
                                  uint64_t first_row, uint64_t m, float* out) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_pca_project");
    if (!x) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    const char* why = "";
    uint64_t local = 0;
    const Plan plan = plan_project(handle_of(x), mean && axes, out != nullptr, n_components, first_row, m, &local, &why);
    if (plan == Plan::Invalid) return fail(x, CQS_HIP_ERR_INVALID, why);
    if (plan == Plan::Nothing) return CQS_HIP_OK;
    const uint32_t dim = x->dim;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, cqs_idx::order_after_last(x, x->stream));
    const uint64_t per = m < kProjectRowsPerLaunch ? m : kProjectRowsPerLaunch;
    const size_t vec_bytes = round16((size_t)dim * sizeof(float));
    DeviceBlock blk;
    HIP_TRY(x, hipMalloc(&blk.p, vec_bytes * (1u + n_components) + (size_t)per * n_components * sizeof(float)));
    float* d_mean = (float*)blk.p;
    float* d_axes = (float*)((char*)blk.p + vec_bytes);
    float* d_out = (float*)((char*)blk.p + vec_bytes * (1u + n_components));
    HIP_TRY(x, hipMemcpyAsync(d_mean, mean, (size_t)dim * sizeof(float), hipMemcpyHostToDevice, x->stream));
    HIP_TRY(x, hipMemcpyAsync(d_axes, axes, (size_t)dim * n_components * sizeof(float), hipMemcpyHostToDevice, x->stream));
    for (uint64_t at = 0; at < m; at += per) {
        const uint64_t cnt = m - at < per ? m - at : per;
        const dim3 grid((uint32_t)((cnt + 3u) / 4u)), block(kThreads);
        switch (n_components) {
            case 1: hipLaunchKernelGGL(project_kernel<1>, grid, block, 0, x->stream, x->d_rows, local + at, cnt, dim, d_mean, d_axes, d_out); break;
            case 2: hipLaunchKernelGGL(project_kernel<2>, grid, block, 0, x->stream, x->d_rows, local + at, cnt, dim, d_mean, d_axes, d_out); break;
            case 3: hipLaunchKernelGGL(project_kernel<3>, grid, block, 0, x->stream, x->d_rows, local + at, cnt, dim, d_mean, d_axes, d_out); break;
            default: hipLaunchKernelGGL(project_kernel<4>, grid, block, 0, x->stream, x->d_rows, local + at, cnt, dim, d_mean, d_axes, d_out); break;
        }
        HIP_TRY(x, hipGetLastError());
        HIP_TRY(x, hipMemcpyAsync(out + at * n_components, d_out, (size_t)cnt * n_components * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        HIP_TRY(x, hipStreamSynchronize(x->stream));
    }
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

}  // extern "C"
