// embed_gemm.hip — the first-generation GEMMs of the embedding side (128 x 128 tiles, few rows, skinny) and the planner
// that divides a projection between them and the 256-row kernel of gemm_kernels.hip.
#include "embed_kernels.h"
#include "activations.h"

#include <cstdlib>

namespace cqs {

// ---- GEMM (first generation; gemm_kernels.hip holds the 256-row ping-pong kernel that takes the full rounds) ----
// C[M,N] = A[M,K] W[N,K]^T, 128x128x64 tiles, 4 waves (2x2) of 64x64, 32x32x16 bf16 MFMA
// Measured alternatives at M=16384 (tools/gemm_bench.py), all 620-730 TF like this one: register-staged
// operands (ds_write_b128), a 256x128 tile with 4 waves of 128x64 and a 3-slot DMA ring (1 wave/SIMD: the
// ~100-cycle DMA issue cannot overlap the wave's own MFMAs: 1.5x slower), the same tile with 8 waves and
// staggered DMA issue (equal), BK = 32 with three workgroups per CU (620-670 TF: twice the barriers cost more than
// the third wave per SIMD gives back).  PMC on this kernel: waves issue 35 % of their cycles, are issue-stalled 41 %
// (mostly behind the other wave's MFMA) and parked at a waitcnt / barrier 24 %; the MFMA pipe is busy 36 %.
// The remaining gap to the matrix-core peak is per-K-step latency exposure
// (barrier + first fragment reads); closing it needs the phase-interleaved 256x256 schedule.
// LDS tile [128 rows][64 k] bf16, 16-B chunk c of row r stored at chunk c ^ ((r >> 1) & 7): the 16
// rows one ds_read_b128 lane group touches then hit 16 distinct 16-B slots of the 256-B bank row.
__device__ __forceinline__ uint32_t swz(uint32_t row, uint32_t chunk) { return row * 64u + ((chunk ^ ((row >> 1) & 7u)) * 8u); }

template <int OUT>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                        void* __restrict__ Cv, uint32_t M, uint32_t N, uint32_t K,
                                                        uint32_t ldc, const float* __restrict__ bias /*nullable; not GEGLU*/) {
    // ONE shared array (a second __shared__ object beside an LDS-DMA staging array can make hipcc
    // drain vmcnt before every ds_read): [buf][A|B][128 rows][64 k]
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * 2 * 128 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wid >> 1, wn = wid & 1;

    // XCD-aware tile order: workgroups b and b+8 share an XCD (round-robin dispatch); give each XCD
    // a contiguous run of tiles (n fastest) so the tiles sharing an A panel meet in one L2.
    const uint32_t nt = N / 128u, mt = (M + 127u) / 128u, total = nt * mt;
    const uint32_t bid = blockIdx.x, xcd = bid % 8u, q = total / 8u, r = total % 8u;
    const uint32_t tile = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + bid / 8u;
    const uint32_t m0 = (tile / nt) * 128u, n0 = (tile % nt) * 128u;

    // LDS-DMA staging (global_load_lds, 16 B per lane): one wave instruction fills 1 KiB = 8 tile
    // rows, lane l -> row (l >> 3), physical 16-B chunk (l & 7).  The swizzle therefore goes on the
    // SOURCE: the lane fetches logical chunk (l & 7) ^ ((row >> 1) & 7) of its row.  Each wave stages
    // 32 rows of A and 32 rows of B per K-step (4 + 4 instructions).
    const bf16_t* ga[4];
    const bf16_t* gb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t row = (uint32_t)(wid * 32 + u * 8 + (lane >> 3));
        const uint32_t c = (uint32_t)(lane & 7) ^ ((row >> 1) & 7u);
        uint32_t ar = m0 + row;
        ar = ar < M ? ar : M - 1u;
        ga[u] = A + (size_t)ar * K + c * 8u;
        gb[u] = W + (size_t)(n0 + row) * K + c * 8u;
    }
    auto stage = [&](uint32_t kt, int buf) {
        bf16_t* dA = smem + (size_t)buf * (2 * 128 * 64) + (size_t)(wid * 32) * 64;
        bf16_t* dB = dA + 128 * 64;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ga[u] + (size_t)kt * 64u),
                                             (__attribute__((address_space(3))) void*)(dA + u * 8 * 64), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gb[u] + (size_t)kt * 64u),
                                             (__attribute__((address_space(3))) void*)(dB + u * 8 * 64), 16, 0, 0);
        }
    };
    f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const uint32_t nk = K / 64u;
    stage(0, 0);
    for (uint32_t kt = 0; kt < nk; ++kt) {
        const int buf = (int)(kt & 1u);
        // one barrier per K-step: it drains this wave's DMA (tile kt has landed for everyone) and
        // proves every wave is done reading the other buffer, which the next stage overwrites
        __syncthreads();
        if (kt + 1u < nk) stage(kt + 1u, buf ^ 1);   // flies under this tile's MFMAs
        const bf16_t* sA = smem + (size_t)buf * (2 * 128 * 64);
        const bf16_t* sB = sA + 128 * 64;
        // fragments of k-step ks+1 are read while the MFMAs of k-step ks run (two register sets)
        bf8 af[2][2], bfr[2][2];
        auto read_frags = [&](int ks, int set) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t row = (uint32_t)(wm * 64 + i * 32 + l31);
                af[set][i] = *(const bf8*)(sA + swz(row, (uint32_t)(2 * ks + lh)));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t row = (uint32_t)(wn * 64 + j * 32 + l31);
                bfr[set][j] = *(const bf8*)(sB + swz(row, (uint32_t)(2 * ks + lh)));
            }
        };
        read_frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < 4) read_frags(ks + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[cur][i], bfr[cur][j], acc[i][j], 0, 0, 0);
        }
    }

    // epilogue: C tile element (row = (e&3) + 8(e>>2) + 4lh, col = l31) of acc[i][j]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const uint32_t row = m0 + (uint32_t)(wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh);
            if (row >= M) continue;
            if (OUT == GEMM_OUT_GEGLU) {
                // this wave's 64 columns = 32 gate channels (j = 0) + the same 32 channels' up (j = 1)
                const uint32_t ch = (n0 + (uint32_t)(wn * 64)) / 2u + (uint32_t)l31;
                const float v = gelu_tanh(acc[i][0][e]) * acc[i][1][e];
                ((bf16_t*)Cv)[(size_t)row * ldc + ch] = (bf16_t)v;
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t col = n0 + (uint32_t)(wn * 64 + j * 32 + l31);
                    float v = acc[i][j][e];
                    if (bias) v += bias[col];
                    if (OUT == GEMM_OUT_BF16_GELU) v = gelu_erf(v);
                    if (OUT == GEMM_OUT_F32) ((float*)Cv)[(size_t)row * ldc + col] = v;
                    else ((bf16_t*)Cv)[(size_t)row * ldc + col] = (bf16_t)v;
                }
            }
        }
}

// ---- few-rows GEMM: small batches (a query, a handful of chunks) ---------------------------------------------
// At M = 32 tokens the 128 x 128 kernel puts 6-18 workgroups on the chip and takes 12 us per projection (4 per layer:
// 70 % of a query's 1.6 ms).  Here ONE WAVE owns a 32 x 32 output tile (GeGLU: 32 x 64 = the gate and up halves of 32
// channels) and walks K by itself with operands straight from global memory / L2 (16 B per lane per 16-k step, 8
// steps in flight), no LDS, no barrier: N / 32 waves per 32 rows.  Same MFMA (32x32x16), same operand roles and the
// same K order as gemm_bf16_kernel, so the two kernels agree bit for bit and a chunk still embeds to the same bits
// alone or in a batch (test_padding_and_batch_invariance).

template <int OUT>
__global__ __launch_bounds__(64) void gemm_fewrows_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                          void* __restrict__ Cv, uint32_t M, uint32_t N, uint32_t K,
                                                          uint32_t ldc, const float* __restrict__ bias /*nullable; not GEGLU*/) {
    constexpr int NT = OUT == GEMM_OUT_GEGLU ? 2 : 1;          // 32-column tiles per wave
    const int lane = threadIdx.x, l31 = lane & 31, lh = lane >> 5;
    const uint32_t n0 = blockIdx.x * (uint32_t)(32 * NT), m0 = blockIdx.y * 32u;
    const uint32_t mr = m0 + (uint32_t)l31 < M ? m0 + (uint32_t)l31 : M - 1u;     // rows past M: any real row, never stored
    const bf16_t* ap = A + (size_t)mr * K + 8 * lh;
    const bf16_t* wp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) wp[j] = W + (size_t)(n0 + (uint32_t)(32 * j + l31)) * K + 8 * lh;
    f16v acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const uint32_t steps = K / 16u;                             // K % 64 == 0
    constexpr int U = 8;
    for (uint32_t s = 0; s < steps; s += U) {
        bf8 af[U], wf[NT][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t ss = s + (uint32_t)u < steps ? s + (uint32_t)u : steps - 1u;     // (tail: re-read, not accumulated)
            af[u] = *(const bf8*)(ap + (size_t)ss * 16u);
#pragma unroll
            for (int j = 0; j < NT; ++j) wf[j][u] = *(const bf8*)(wp[j] + (size_t)ss * 16u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (s + (uint32_t)u < steps) {
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[u], wf[j][u], acc[j], 0, 0, 0);
            }
    }
    // C tile element (row = (e & 3) + 8 (e >> 2) + 4 lh, col = l31), as in gemm_bf16_kernel
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const uint32_t row = m0 + (uint32_t)((e & 3) + 8 * (e >> 2) + 4 * lh);
        if (row >= M) continue;
        if (OUT == GEMM_OUT_GEGLU) {
            const float v = gelu_tanh(acc[0][e]) * acc[NT - 1][e];
            ((bf16_t*)Cv)[(size_t)row * ldc + n0 / 2u + (uint32_t)l31] = (bf16_t)v;
        } else {
            float v = acc[0][e];
            if (bias) v += bias[n0 + (uint32_t)l31];
            if (OUT == GEMM_OUT_BF16_GELU) v = gelu_erf(v);
            if (OUT == GEMM_OUT_F32) ((float*)Cv)[(size_t)row * ldc + n0 + (uint32_t)l31] = v;
            else ((bf16_t*)Cv)[(size_t)row * ldc + n0 + (uint32_t)l31] = (bf16_t)v;
        }
    }
}

static hipError_t launch_gemm_fewrows(const bf16_t* A, const bf16_t* W, const float* bias, void* C, uint32_t M, uint32_t N,
                                      uint32_t K, uint32_t ldc, GemmOut out, hipStream_t st) {
    if (N % 64u || K % 64u || (bias && out == GEMM_OUT_GEGLU)) return hipErrorInvalidValue;
    const dim3 fg(N / (out == GEMM_OUT_GEGLU ? 64u : 32u), (M + 31u) / 32u);
    switch (out) {
        case GEMM_OUT_BF16: hipLaunchKernelGGL(gemm_fewrows_kernel<GEMM_OUT_BF16>, fg, dim3(64), 0, st, A, W, C, M, N, K, ldc, bias); break;
        case GEMM_OUT_F32: hipLaunchKernelGGL(gemm_fewrows_kernel<GEMM_OUT_F32>, fg, dim3(64), 0, st, A, W, C, M, N, K, ldc, bias); break;
        case GEMM_OUT_GEGLU: hipLaunchKernelGGL(gemm_fewrows_kernel<GEMM_OUT_GEGLU>, fg, dim3(64), 0, st, A, W, C, M, N, K, ldc, bias); break;
        case GEMM_OUT_BF16_GELU: hipLaunchKernelGGL(gemm_fewrows_kernel<GEMM_OUT_BF16_GELU>, fg, dim3(64), 0, st, A, W, C, M, N, K, ldc, bias); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// One kernel for the whole [M, N] problem; tn = 0: the 128 x 128 kernel, 3..5: the 256 x (64 tn) ping-pong kernel.
static hipError_t launch_gemm_one(const bf16_t* A, const bf16_t* W, void* C, uint32_t M, uint32_t N, uint32_t K,
                                  uint32_t ldc, GemmOut out, int tn, hipStream_t st, const float* bias = nullptr) {
    if (tn) return launch_gemm_p8(A, W, C, M, N, K, ldc, out, tn, st, bias);
    static const uint32_t few_max = [] { const char* f = getenv("CQS_HIP_GEMM_FEWROWS"); return f ? (uint32_t)atoi(f) : 512u; }();
    if (M <= few_max && !getenv("CQS_HIP_GEMM_TILE"))           // small batch: one wave per 32 x 32 tile (bit-identical results)
        return launch_gemm_fewrows(A, W, bias, C, M, N, K, ldc, out, st);
    const dim3 grid((N / 128u) * ((M + 127u) / 128u)), block(256);
    switch (out) {
        case GEMM_OUT_BF16: hipLaunchKernelGGL(gemm_bf16_kernel<GEMM_OUT_BF16>, grid, block, 0, st, A, W, C, M, N, K, ldc, bias); break;
        case GEMM_OUT_F32: hipLaunchKernelGGL(gemm_bf16_kernel<GEMM_OUT_F32>, grid, block, 0, st, A, W, C, M, N, K, ldc, bias); break;
        case GEMM_OUT_GEGLU: hipLaunchKernelGGL(gemm_bf16_kernel<GEMM_OUT_GEGLU>, grid, block, 0, st, A, W, C, M, N, K, ldc, nullptr); break;
        case GEMM_OUT_BF16_GELU: hipLaunchKernelGGL(gemm_bf16_kernel<GEMM_OUT_BF16_GELU>, grid, block, 0, st, A, W, C, M, N, K, ldc, bias); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- skinny GEMM: a handful of rows (the pooled sentence vectors through the two Dense layers: M = sequences of
// the batch) against a big weight matrix.  The tiled kernels put 24 (or 6) workgroups on the chip for M = 32 and take
// 43 + 14 us; this one is a batch of GEMVs: one workgroup = one 16 x 16 output tile, its 4 waves split K (each streams
// its quarter of the 16 weight rows once, 16 B per lane, loads 8 k-steps deep), partial tiles summed through LDS.
template <int OUT>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                         void* __restrict__ Cv, uint32_t M, uint32_t N, uint32_t K,
                                                         uint32_t ldc, uint32_t lda /*row stride of A, elements*/,
                                                         const float* __restrict__ bias /*nullable*/, int act /*1: tanh*/,
                                                         const int32_t* __restrict__ row_index /*nullable: A row of output row m*/) {
    __shared__ __attribute__((aligned(16))) float red[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const uint32_t n0 = blockIdx.x * 16u, m0 = blockIdx.y * 16u;
    const uint32_t ksteps = K / 32u, per = (ksteps + 3u) / 4u;
    const uint32_t s_lo = (uint32_t)wid * per, s_hi = s_lo + per < ksteps ? s_lo + per : ksteps;
    const uint32_t mr = m0 + (uint32_t)l15 < M ? m0 + (uint32_t)l15 : M - 1u;    // rows past M: any real row, never stored
    const bf16_t* ap = A + (size_t)(row_index ? (uint32_t)row_index[mr] : mr) * lda + 8 * lg;
    const bf16_t* wp = W + (size_t)(n0 + (uint32_t)l15) * K + 8 * lg;
    f4 acc = (f4)(0.f);
    constexpr int U = 8;
    for (uint32_t s = s_lo; s < s_hi; s += U) {
        bf8 af[U], wf[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t ss = s + (uint32_t)u < s_hi ? s + (uint32_t)u : s_hi - 1u;   // (tail: re-read, not accumulated)
            af[u] = *(const bf8*)(ap + (size_t)ss * 32u);
            wf[u] = *(const bf8*)(wp + (size_t)ss * 32u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (s + (uint32_t)u < s_hi) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], af[u], acc, 0, 0, 0);
    }
    // acc[r] = C[m = m0 + l15][n = n0 + 4 lg + r] (weights as the A operand: a lane holds 4 consecutive columns)
    *(f4*)&red[wid][(l15 * 4 + lg) * 4] = acc;
    __syncthreads();
    if (wid == 0) {
        f4 v = *(const f4*)&red[0][(l15 * 4 + lg) * 4];
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *(const f4*)&red[w][(l15 * 4 + lg) * 4];
        const uint32_t m = m0 + (uint32_t)l15;
        if (bias) v += *(const f4*)(bias + n0 + 4 * lg);
        if (act == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = tanhf(v[r]);
        }
        if (m < M) {
            if (OUT == GEMM_OUT_F32) *(f4*)((float*)Cv + (size_t)m * ldc + n0 + 4 * lg) = v;
            else {
                bf4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (bf16_t)v[r];
                *(bf4*)((bf16_t*)Cv + (size_t)m * ldc + n0 + 4 * lg) = o;
            }
        }
    }
}

// Kernel plan of one [M, N, K] projection: n1 columns with tile kind tn1 (0 = the 128 x 128 kernel, 3..5 = 256 x 64 tn),
// the remaining N - n1 columns (if any) with tn2.
struct GemmPlan { uint32_t n1; int tn1, tn2; };
static GemmPlan plan_gemm(uint32_t M, uint32_t N, uint32_t K, GemmOut out) {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
            n_cu = 256;
    }
    // Kernel choice: rounds x measured cost of one round of tiles (microseconds at K = 768 on an MI355X, launch to
    // launch).  A round of the 256-row kernel costs ~8 us of prologue + epilogue on top of its K-steps and rounds of one
    // launch do not overlap (one workgroup per CU), so big tiles only pay when their rounds are FULL:
    //   128 x 128: 9 (GeGLU 8.2) | 256 x 192: 24 | 256 x 256: 25.5 | 256 x 320: 32.5   (GeGLU epilogue: + 1.5)
    // and a problem whose tile count is not a multiple of the CU count is cut in two launches along N: the part that
    // makes whole rounds of big tiles + the rest (N = 2304 at 16 384 rows: 2048 columns = 2 rounds of 256 x 256, then
    // 256 columns = one round of 128 x 128: 62 us instead of 73).
    const float kscale = (float)K / 768.f;
    const float geglu = out == GEMM_OUT_GEGLU ? 1.f : 0.f;
    static const uint32_t cu_env = [] { const char* f = getenv("CQS_HIP_GEMM_CUS"); const int v = f ? atoi(f) : 0; return v > 0 ? (uint32_t)v : 0u; }();
    const uint32_t cu = cu_env ? cu_env : (uint32_t)n_cu;      // (experiment hook: plan for part of the chip; read once)
    const bool fits = (uint64_t)M * K < (1ull << 31) && (uint64_t)N * K < (1ull << 31);
    const float cost[6] = {0.f, 0.f, 0.f, 24.f, 25.5f, 32.5f};
    auto one = [&](uint32_t n, int t) -> float {              // cost of n columns with one kernel; < 0: not applicable
        if (t == 0) return (float)(((n / 128u) * ((M + 127u) / 128u) + cu - 1u) / cu) * (3.f + (6.f - 0.8f * geglu) * kscale);
        if (!fits || n % (64u * (uint32_t)t)) return -1.f;
        return (float)(((n / (64u * (uint32_t)t)) * ((M + 255u) / 256u) + cu - 1u) / cu) * (8.f + 1.5f * geglu + (cost[t] - 8.f) * kscale);
    };
    auto best_one = [&](uint32_t n, int& t_out) -> float {
        float best = one(n, 0);
        t_out = 0;
        for (int t = 3; t <= 5; ++t) { const float c = one(n, t); if (c >= 0.f && c < best) { best = c; t_out = t; } }
        return best;
    };
    int tn1 = 0, tn2 = 0;
    uint32_t n1 = N;
    float best = best_one(N, tn1);
    const uint32_t mt = (M + 255u) / 256u;
    uint32_t g = mt, h = cu;
    while (h) { const uint32_t r = g % h; g = h; h = r; }      // g = gcd(mt, cu)
    for (int t = 3; t <= 5 && fits; ++t) {
        const uint32_t step = (cu / g) * 64u * (uint32_t)t;     // columns that make whole rounds of 256 x 64 t tiles
        for (uint32_t c1 = step; c1 < N; c1 += step) {
            if ((N - c1) % 128u) continue;
            int t2 = 0;
            const float c = one(c1, t) + best_one(N - c1, t2) + 2.f;   // + one kernel boundary
            if (c < best) { best = c; n1 = c1; tn1 = t; tn2 = t2; }
        }
    }
    if (const char* f = getenv("CQS_HIP_GEMM_TILE")) {  // test hook: "small" / "pp:<tn>" force one kernel (read per call: tests flip it)
        n1 = N;
        if (f[0] == 's') tn1 = 0;
        else if (f[0] == 'p') {
            const int t = f[2] == ':' ? atoi(f + 3) : 4;
            tn1 = (t >= 3 && t <= 5 && fits && N % (64u * (uint32_t)t) == 0) ? t : 0;
        }
    }
    return {n1, tn1, tn2};
}

int gemm_qkv_rope_tile(uint32_t M, uint32_t hidden, uint32_t heads, uint32_t kv_heads, uint32_t head_dim) {
    if (head_dim != 256u || kv_heads == 0u || hidden % 64u) return 0;
    const uint32_t N = (heads + 2u * kv_heads) * head_dim;
    const GemmPlan p = plan_gemm(M, N, hidden, GEMM_OUT_BF16);
    if (p.n1 != N) return 0;                              // the plain projection would be one launch of that tile too
    if (p.tn1 == 5 && heads == 3u * kv_heads) return 5;
    if (p.tn1 == 4) return 4;
    return 0;
}

hipError_t launch_gemm_bf16(const bf16_t* A, const bf16_t* W, void* C, uint32_t M, uint32_t N, uint32_t K,
                            uint32_t ldc, GemmOut out, hipStream_t st, const float* bias, const bf16_t* W_geglu4) {
    if (M == 0) return hipSuccess;
    if (N % 128u || K % 64u || (bias && out == GEMM_OUT_GEGLU)) return hipErrorInvalidValue;
    const GemmPlan pl = plan_gemm(M, N, K, out);
    const uint32_t n1 = pl.n1;
    const int tn1 = pl.tn1, tn2 = pl.tn2;
    if (out == GEMM_OUT_GEGLU && W_geglu4) {
        // parts the 256-row kernel takes read the per-4 interleave and pair gate / up in registers; a part on the 128 x 128 /
        // few-rows kernels keeps the per-32 order (cuts are multiples of 64 rows: the same channels on either side in both)
        const size_t coff = n1 / 2u;
        if (n1 == N) return launch_gemm_one(A, tn1 ? W_geglu4 : W, C, M, N, K, ldc, tn1 ? GEMM_OUT_GEGLU4 : GEMM_OUT_GEGLU, tn1, st, nullptr);
        if (n1 % 64u) return hipErrorInvalidValue;
        static const bool no_dual4 = getenv("CQS_HIP_GEMM_NO_DUAL") != nullptr;
        if (tn1 >= 3 && tn2 >= 3 && tn1 != tn2 && !no_dual4) {
            const hipError_t d = launch_gemm_p8_dual(A, W_geglu4, C, n1, tn1, W_geglu4 + (size_t)n1 * K, (bf16_t*)C + coff, N - n1, tn2, M, K, ldc, GEMM_OUT_GEGLU4, st);
            if (d != hipErrorNotSupported) return d;
        }
        hipError_t e = launch_gemm_one(A, tn1 ? W_geglu4 : W, C, M, n1, K, ldc, tn1 ? GEMM_OUT_GEGLU4 : GEMM_OUT_GEGLU, tn1, st, nullptr);
        if (e != hipSuccess) return e;
        return launch_gemm_one(A, (tn2 ? W_geglu4 : W) + (size_t)n1 * K, (bf16_t*)C + coff, M, N - n1, K, ldc, tn2 ? GEMM_OUT_GEGLU4 : GEMM_OUT_GEGLU, tn2, st, nullptr);
    }
    if (n1 == N) return launch_gemm_one(A, W, C, M, N, K, ldc, out, tn1, st, bias);
    const size_t coff = out == GEMM_OUT_GEGLU ? n1 / 2u : n1;    // output columns of the first part
    void* c2 = out == GEMM_OUT_F32 ? (void*)((float*)C + coff) : (void*)((bf16_t*)C + coff);
    static const bool no_dual = getenv("CQS_HIP_GEMM_NO_DUAL") != nullptr;                       // (read once)
    if (tn1 >= 3 && tn2 >= 3 && tn1 != tn2 && !bias && out != GEMM_OUT_BF16_GELU && !no_dual) {   // both parts in one launch
        const hipError_t d = launch_gemm_p8_dual(A, W, C, n1, tn1, W + (size_t)n1 * K, c2, N - n1, tn2, M, K, ldc, out, st);
        if (d != hipErrorNotSupported) return d;
    }
    hipError_t e = launch_gemm_one(A, W, C, M, n1, K, ldc, out, tn1, st, bias);
    if (e != hipSuccess) return e;
    return launch_gemm_one(A, W + (size_t)n1 * K, c2, M, N - n1, K, ldc, out, tn2, st, bias ? bias + n1 : nullptr);
}

hipError_t launch_gemm_bias(const bf16_t* A, const bf16_t* W, const float* bias, void* C, uint32_t M, uint32_t N,
                            uint32_t K, uint32_t ldc, GemmOut out, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (out == GEMM_OUT_GEGLU || K % 64u) return hipErrorInvalidValue;
    // small batches (a query, a rerank of a few dozen passages): one wave per 32 x 32 tile, no fixed cost of the 256-row
    // kernel's prologue / epilogue (13-50 us per projection at a few thousand tokens; measured crossover below)
    // Crossover measured on whole forwards (tools/bert_fewrows_sweep.py): few-rows wins up to ~900 tokens for BERT-base
    // (hidden 768), ~600 for BERT-large (1024), ~2000 for MiniLM (384) - for ALL of a layer's projections, the K = 4 x
    // hidden one included - i.e. tokens x hidden <~ 640 Ki; min(N, K) is the hidden size of every BERT projection.
    // up to 64 rows (a SPLADE query, one short passage): the search-time kernels - K split over a workgroup's waves, 96-384
    // workgroups - instead of 24-96 lone waves walking all of K (BERT-base FFN2 at 16 tokens: 25 us -> 3 us)
    if (M <= 64u) {
        const char* sr = getenv("CQS_HIP_GEMM_SMALL_ROWS");       // read per call: a test flips it inside one process
        if (!(sr && sr[0] == '0')) {
            const hipError_t e = launch_gemm_small_rows(A, W, bias, C, M, N, K, ldc, out, st);
            if (e != hipErrorNotSupported) return e;
        }
    }
    static const uint64_t few_mh = [] { const char* f = getenv("CQS_HIP_GEMM_BIAS_FEWROWS_MH"); return f ? (uint64_t)atoll(f) : 640ull * 1024ull; }();
    if ((uint64_t)M * (N < K ? N : K) <= few_mh && N % 64u == 0) return launch_gemm_fewrows(A, W, bias, C, M, N, K, ldc, out, st);
    // just above the few-rows range the 128 x 128 kernel still beats a mostly empty round of 256-row tiles (measured:
    // 1024 tokens of BERT-base 1.72 -> 1.62 ms, BERT-large 4.6 -> 4.15 ms; from ~2k tokens on the 256-row kernel wins)
    if (N % 128u == 0 && M <= 1536u) return launch_gemm_bf16(A, W, C, M, N, K, ldc, out, st, bias);
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
            n_cu = 256;
    }
    // (N not a multiple of 128) rounds x cost of a round (launch_gemm_bf16's table), over the tile widths that divide N
    const float cost[6] = {0.f, 0.f, 0.f, 24.f, 25.5f, 32.5f};
    int best_t = 0;
    float best = 0.f;
    for (int t = 3; t <= 5; ++t) {
        if (N % (64u * (uint32_t)t)) continue;
        const uint32_t tiles = (N / (64u * (uint32_t)t)) * ((M + 255u) / 256u);
        const float c = (float)((tiles + (uint32_t)n_cu - 1u) / (uint32_t)n_cu) * (8.f + (cost[t] - 8.f) * (float)K / 768.f);
        if (!best_t || c < best) { best = c; best_t = t; }
    }
    if (!best_t) return hipErrorInvalidValue;
    return launch_gemm_p8(A, W, C, M, N, K, ldc, out, best_t, st, bias);
}

// The Dense head's GEMMs (M = sequences of the batch).  Not chosen by launch_gemm_bf16 itself: its K split sums in a
// different order than the tiled kernels, and a token's activations must not depend on how many tokens share its
// batch (tests/test_embed_gpu.py::test_padding_and_batch_invariance) - the head, applied once per sequence, always
// takes this path up to 256 sequences, the tiled kernels beyond.
hipError_t launch_gemm_skinny(const bf16_t* A, const bf16_t* W, void* C, uint32_t M, uint32_t N, uint32_t K,
                              uint32_t ldc, GemmOut out, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (N % 16u || K % 32u || (out != GEMM_OUT_BF16 && out != GEMM_OUT_F32)) return hipErrorInvalidValue;
    if (M > 256u) return launch_gemm_bf16(A, W, C, M, N, K, ldc, out, st);
    return launch_gemm_rows(A, K, W, nullptr, 0, C, M, N, K, ldc, out, st, nullptr);
}

// The same kernel on strided rows with a bias and an optional tanh (the BERT pooler reads every sequence's first
// token out of the packed hidden states: lda = its stride; any M).
hipError_t launch_gemm_rows(const bf16_t* A, uint32_t lda, const bf16_t* W, const float* bias, int act_tanh, void* C,
                            uint32_t M, uint32_t N, uint32_t K, uint32_t ldc, GemmOut out, hipStream_t st,
                            const int32_t* row_index) {
    if (M == 0) return hipSuccess;
    if (N % 16u || K % 32u || (out != GEMM_OUT_BF16 && out != GEMM_OUT_F32)) return hipErrorInvalidValue;
    const dim3 grid(N / 16u, (M + 15u) / 16u);
    if (out == GEMM_OUT_F32)
        hipLaunchKernelGGL(gemm_skinny_kernel<GEMM_OUT_F32>, grid, dim3(256), 0, st, A, W, C, M, N, K, ldc, lda, bias, act_tanh, row_index);
    else
        hipLaunchKernelGGL(gemm_skinny_kernel<GEMM_OUT_BF16>, grid, dim3(256), 0, st, A, W, C, M, N, K, ldc, lda, bias, act_tanh, row_index);
    return hipGetLastError();
}

}  // namespace cqs
