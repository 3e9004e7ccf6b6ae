// embed_rows.hip — the row kernels of the EmbeddingGemma-300m forward (Gemma3 text encoder, bidirectional, +
// sentence-transformers pooling/dense head): embedding + norm, residual add + norm, q/k norm + RoPE, V transpose, mean
// pool, f32 -> bf16.  The attention is embed_attention.hip, the GEMMs embed_gemm.hip / gemm_kernels.hip /
// gemm_rowfuse.hip.  Together they replace the ONNX Runtime `session.run` of the reference
// (src/embedder/core.rs:1097; graph described in SURVEY.md §8a row A20).  Semantics follow oracle/gemma3_ref.py (which
// is pinned to transformers' Gemma3TextModel); bf16 operands on the matrix cores, f32 accumulation, f32 residual stream.
//
// Tokens are PACKED: padding never reaches a kernel (the reference pads every sequence to the
// longest of the batch, src/embedder/core.rs:1020-1035, and ORT computes on the pad).
#include "embed_kernels.h"

namespace cqs {

// ---- row kernels: one wave per token row, lane owns 4 consecutive floats of each 256-chunk ----
template <int NCH>
__global__ __launch_bounds__(256) void embed_norm_kernel(const int32_t* __restrict__ tok,
                                                         const bf16_t* __restrict__ emb, float scale,
                                                         const float* __restrict__ w_in, float eps,
                                                         float* __restrict__ x, bf16_t* __restrict__ xn, uint32_t M) {
    constexpr uint32_t H = NCH * 256;
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= M) return;
    const size_t src = (size_t)tok[row] * H;
    float v[NCH][4];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t col = (uint32_t)c * 256u + (uint32_t)lane * 4u;
        const bf4 e = *(const bf4*)(emb + src + col);
        f4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[c][i] = (float)e[i] * scale;
            o[i] = v[c][i];
            ss += v[c][i] * v[c][i];
        }
        *(f4*)(x + (size_t)row * H + col) = o;
    }
    const float inv = rsqrtf(wave_sum64_shfl(ss) / (float)H + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t col = (uint32_t)c * 256u + (uint32_t)lane * 4u;
        const f4 w = *(const f4*)(w_in + col);
        bf4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16_t)(v[c][i] * inv * (1.0f + w[i]));
        *(bf4*)(xn + (size_t)row * H + col) = o;
    }
}

// Row sums are taken HALF BY HALF (row_sum_of_halves, wave_ops.h): lane L owns, in half h = L >> 5, the columns
// (H / 2) h + 128 c + 4 (L & 31) + {0..3}, c = 0..NCH-1 - the split of the pair-split fused kernel (gemm_rowfuse.hip).
template <int NCH, int FINAL>
__global__ __launch_bounds__(256) void add_norm_kernel(float* __restrict__ x, const bf16_t* __restrict__ y,
                                                       const float* __restrict__ w_post,
                                                       const float* __restrict__ w_next, float eps,
                                                       bf16_t* __restrict__ xn, float* __restrict__ out, uint32_t M) {
    constexpr uint32_t H = NCH * 256;
    const int lane = threadIdx.x & 63;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= M) return;
    const uint32_t col0 = (uint32_t)(lane >> 5) * (H / 2u) + (uint32_t)(lane & 31) * 4u;
    f4 yv[NCH], xv[NCH];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t col = col0 + (uint32_t)c * 128u;
        const bf4 yb = *(const bf4*)(y + (size_t)row * H + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) yv[c][i] = (float)yb[i];
        xv[c] = *(const f4*)(x + (size_t)row * H + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) ss += yv[c][i] * yv[c][i];
    }
    const float invy = rsqrtf(row_sum_of_halves(ss) / (float)H + eps);
    float sx = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t col = col0 + (uint32_t)c * 128u;
        const f4 w = *(const f4*)(w_post + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xv[c][i] += yv[c][i] * invy * (1.0f + w[i]);
            sx += xv[c][i] * xv[c][i];
        }
        *(f4*)(x + (size_t)row * H + col) = xv[c];
    }
    const float invx = rsqrtf(row_sum_of_halves(sx) / (float)H + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const uint32_t col = col0 + (uint32_t)c * 128u;
        const f4 w = *(const f4*)(w_next + col);
        if (FINAL) {
            f4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = xv[c][i] * invx * (1.0f + w[i]);
            *(f4*)(out + (size_t)row * H + col) = o;
        } else {
            bf4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = (bf16_t)(xv[c][i] * invx * (1.0f + w[i]));
            *(bf4*)(xn + (size_t)row * H + col) = o;
        }
    }
}

// ---- q/k RMSNorm + RoPE, in place; one wave per token, all its q and k heads; lane owns dims [4l, 4l+4) ----
// (the token's cos/sin row - twice the bytes of one head - is fetched once for all heads, and the heads'
// loads are in flight together)
constexpr int kMaxQkHeads = 8;
__device__ __forceinline__ void qk_norm_rope_block(uint32_t bid, bf16_t* __restrict__ qkv, const int32_t* __restrict__ pos,
                                                   const float* __restrict__ wq, const float* __restrict__ wk,
                                                   const float* __restrict__ cos_sin, float eps, float q_scale,
                                                   uint32_t M, uint32_t heads, uint32_t kv_heads, uint32_t h_first) {
    // heads [h_first, heads + kv_heads) of the fused q | k | v row: h_first = 0 -> q and k heads, h_first = heads -> the
    // k heads only (the attention kernel then normalises / rotates its own Q fragments)
    const int lane = threadIdx.x & 63;
    const uint32_t nh = heads + kv_heads - h_first;
    const uint32_t m = bid * 4u + (threadIdx.x >> 6);
    if (m >= M) return;
    const uint32_t ld = (heads + 2u * kv_heads) * kHD;
    bf16_t* row = qkv + (size_t)m * ld + (size_t)h_first * kHD + lane * 4;
    bf4 in[kMaxQkHeads];
#pragma unroll
    for (int h = 0; h < kMaxQkHeads; ++h)
        if ((uint32_t)h < nh) in[h] = *(const bf4*)(row + (size_t)h * kHD);
    // rotate_half pairs dim d with d +/- 128: the partner lives in lane ^ 32, same element
    const float* cs = cos_sin + ((size_t)pos[m] * 128u + (uint32_t)(lane & 31) * 4u) * 2u;
    const f4 cs0 = *(const f4*)cs, cs1 = *(const f4*)(cs + 4);  // (cos,sin) x 4 dims
    const float c4[4] = {cs0[0], cs0[2], cs1[0], cs1[2]};
    const float s4[4] = {cs0[1], cs0[3], cs1[1], cs1[3]};
    const f4 wqv = *(const f4*)(wq + lane * 4), wkv = *(const f4*)(wk + lane * 4);
#pragma unroll
    for (int h = 0; h < kMaxQkHeads; ++h) {
        if ((uint32_t)h >= nh) break;
        const bool is_q = (uint32_t)h + h_first < heads;
        float v[4];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = (float)in[h][i];
            ss += v[i] * v[i];
        }
        const float inv = rsqrtf(wave_sum64_shfl(ss) / (float)kHD + eps);
        bf4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float n = v[i] * inv * (1.0f + (is_q ? wqv[i] : wkv[i]));
            const float other = __shfl_xor(n, 32, 64);
            // d < 128: n*cos - x[d+128]*sin ; d >= 128: n*cos + x[d-128]*sin
            float r = (lane < 32) ? (n * c4[i] - other * s4[i]) : (n * c4[i] + other * s4[i]);
            if (is_q) r *= q_scale;
            o[i] = (bf16_t)r;
        }
        *(bf4*)(row + (size_t)h * kHD) = o;
    }
}
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(bf16_t* __restrict__ qkv, const int32_t* __restrict__ pos,
                                                           const float* __restrict__ wq, const float* __restrict__ wk,
                                                           const float* __restrict__ cos_sin, float eps, float q_scale,
                                                           uint32_t M, uint32_t heads, uint32_t kv_heads, uint32_t h_first) {
    qk_norm_rope_block(blockIdx.x, qkv, pos, wq, wk, cos_sin, eps, q_scale, M, heads, kv_heads, h_first);
}

// ---- V transpose: vt[g][d][vt_start[seq] + pos] = v[token][g][d] -------------------------------------
// One workgroup = 64 positions (half a 128-position super-block of the attention's blk list) x 64 head
// dims of one kv head, through LDS.  In: 16-B loads along d.  Out: 16-B stores of 8 consecutive
// positions of one head dim (V^T columns of a sequence start at a multiple of 32, so they are aligned);
// 8 lanes cover one dim's 64 positions = one full 128-B line.  Positions past the sequence end are
// written as zeros (the attention multiplies them by P = 0; they must stay finite).
__device__ __forceinline__ void v_transpose_block(uint32_t bx, uint32_t by, const bf16_t* __restrict__ qkv,
                                                  bf16_t* __restrict__ vt, const int32_t* __restrict__ blk,
                                                  const int32_t* __restrict__ seq_start,
                                                  const int32_t* __restrict__ seq_len,
                                                  const int32_t* __restrict__ vt_start, uint32_t heads,
                                                  uint32_t kv_heads, uint32_t vt_ld) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[64][64 + 8];
    const uint32_t g = by >> 2, d0 = (by & 3u) * 64u;
    const uint32_t sblk = bx >> 1, half = bx & 1u;
    const uint32_t seq = (uint32_t)blk[2 * sblk], sb = (uint32_t)blk[2 * sblk + 1];
    const uint32_t len = (uint32_t)seq_len[seq], m_seq = (uint32_t)seq_start[seq], c_seq = (uint32_t)vt_start[seq];
    const uint32_t cols = (len + 31u) & ~31u;  // the sequence's padded V^T columns
    const uint32_t p0 = sb * 128u + half * 64u;
    if (p0 >= cols) return;
    const uint32_t ld = (heads + 2u * kv_heads) * kHD;
    const uint32_t voff = (heads + kv_heads + g) * kHD + d0;
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const uint32_t i = (uint32_t)(u * 256 + tid), t = i >> 3, c = (i & 7u) * 8u;
        bf8 v = (bf8)(0.f);
        if (p0 + t < len) v = *(const bf8*)(qkv + (size_t)(m_seq + p0 + t) * ld + voff + c);
        *(bf8*)&tile[t][c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const uint32_t i = (uint32_t)(u * 256 + tid), d = i >> 3, t0 = (i & 7u) * 8u;
        if (p0 + t0 >= cols) continue;
        bf8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = tile[t0 + e][d];
        *(bf8*)(vt + ((size_t)g * kHD + d0 + d) * vt_ld + c_seq + p0 + t0) = o;
    }
}
__global__ __launch_bounds__(256) void v_transpose_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ vt,
                                                          const int32_t* __restrict__ blk,
                                                          const int32_t* __restrict__ seq_start,
                                                          const int32_t* __restrict__ seq_len,
                                                          const int32_t* __restrict__ vt_start, uint32_t heads,
                                                          uint32_t kv_heads, uint32_t vt_ld) {
    v_transpose_block(blockIdx.x, blockIdx.y, qkv, vt, blk, seq_start, seq_len, vt_start, heads, kv_heads, vt_ld);
}

// ---- k-head norm + RoPE and the V transpose in ONE launch (two 6-7 us latency-bound kernels with nothing in common
// but their input row: workgroups [0, n_rope) take 4 tokens each, the rest one V^T tile each) -------------------------
__global__ __launch_bounds__(256) void kv_prep_kernel(bf16_t* __restrict__ qkv, bf16_t* __restrict__ vt,
                                                      const int32_t* __restrict__ pos, const float* __restrict__ wq,
                                                      const float* __restrict__ wk, const float* __restrict__ cos_sin,
                                                      float eps, float q_scale, uint32_t M, uint32_t heads,
                                                      uint32_t kv_heads, uint32_t n_rope, const int32_t* __restrict__ blk,
                                                      uint32_t nblk, const int32_t* __restrict__ seq_start,
                                                      const int32_t* __restrict__ seq_len,
                                                      const int32_t* __restrict__ vt_start, uint32_t vt_ld) {
    if (blockIdx.x < n_rope) {
        qk_norm_rope_block(blockIdx.x, qkv, pos, wq, wk, cos_sin, eps, q_scale, M, heads, kv_heads, heads);
    } else {
        const uint32_t b2 = blockIdx.x - n_rope;
        v_transpose_block(b2 % (nblk * 2u), b2 / (nblk * 2u), qkv, vt, blk, seq_start, seq_len, vt_start, heads, kv_heads, vt_ld);
    }
}

// ---- masked mean pool: block = (sequence, 256 hidden dims); 16 waves split the tokens, 4 loads in flight each ----
// (96 workgroups for 32 sequences x 768 dims: the parallelism has to come from inside the workgroup)
__global__ __launch_bounds__(1024) void mean_pool_kernel(const float* __restrict__ hidden,
                                                         const int32_t* __restrict__ seq_start,
                                                         const int32_t* __restrict__ seq_len,
                                                         bf16_t* __restrict__ pooled, uint32_t H) {
    __shared__ f4 part[16][64];
    const uint32_t b = blockIdx.x, lane = threadIdx.x & 63u, col = blockIdx.y * 256u + lane * 4u;
    const uint32_t s0 = (uint32_t)seq_start[b], L = (uint32_t)seq_len[b];
    const uint32_t w = threadIdx.x >> 6;
    const float* base = hidden + (size_t)s0 * H + col;
    f4 acc = (f4)(0.f);
    uint32_t t = w;
    for (; t + 48u < L; t += 64u) {   // 4 independent loads per trip
        const f4 a0 = *(const f4*)(base + (size_t)t * H), a1 = *(const f4*)(base + (size_t)(t + 16u) * H);
        const f4 a2 = *(const f4*)(base + (size_t)(t + 32u) * H), a3 = *(const f4*)(base + (size_t)(t + 48u) * H);
        acc += (a0 + a1) + (a2 + a3);
    }
    for (; t < L; t += 16u) acc += *(const f4*)(base + (size_t)t * H);
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        f4 sum = part[0][lane];
#pragma unroll
        for (int i = 1; i < 16; ++i) sum += part[i][lane];
        const float inv = L ? 1.0f / (float)L : 0.f;   // zero mask -> zero vector (src/embedder/pooling.rs:113-119)
        bf4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (bf16_t)(sum[i] * inv);
        *(bf4*)(pooled + (size_t)b * H + col) = o;
    }
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = (bf16_t)in[i];
}

// ---- launchers ---------------------------------------------------------------------------
hipError_t launch_embed_norm(const int32_t* tok, const bf16_t* emb, float scale, const float* w_in, float eps,
                             float* x, bf16_t* xn, uint32_t M, uint32_t H, hipStream_t st) {
    if (M == 0) return hipSuccess;
    const dim3 grid((M + 3u) / 4u), block(256);
    switch (H / 256u) {
        case 1: hipLaunchKernelGGL(embed_norm_kernel<1>, grid, block, 0, st, tok, emb, scale, w_in, eps, x, xn, M); break;
        case 2: hipLaunchKernelGGL(embed_norm_kernel<2>, grid, block, 0, st, tok, emb, scale, w_in, eps, x, xn, M); break;
        case 3: hipLaunchKernelGGL(embed_norm_kernel<3>, grid, block, 0, st, tok, emb, scale, w_in, eps, x, xn, M); break;
        case 4: hipLaunchKernelGGL(embed_norm_kernel<4>, grid, block, 0, st, tok, emb, scale, w_in, eps, x, xn, M); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int FINAL>
static hipError_t launch_add_norm_t(float* x, const bf16_t* y, const float* w_post, const float* w_next, float eps,
                                    bf16_t* xn, float* out, uint32_t M, uint32_t H, hipStream_t st) {
    const dim3 grid((M + 3u) / 4u), block(256);
    switch (H / 256u) {
        case 1: hipLaunchKernelGGL((add_norm_kernel<1, FINAL>), grid, block, 0, st, x, y, w_post, w_next, eps, xn, out, M); break;
        case 2: hipLaunchKernelGGL((add_norm_kernel<2, FINAL>), grid, block, 0, st, x, y, w_post, w_next, eps, xn, out, M); break;
        case 3: hipLaunchKernelGGL((add_norm_kernel<3, FINAL>), grid, block, 0, st, x, y, w_post, w_next, eps, xn, out, M); break;
        case 4: hipLaunchKernelGGL((add_norm_kernel<4, FINAL>), grid, block, 0, st, x, y, w_post, w_next, eps, xn, out, M); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_add_norm(float* x, const bf16_t* y, const float* w_post, const float* w_next, float eps,
                           bf16_t* xn, float* out, int final, uint32_t M, uint32_t H, hipStream_t st) {
    if (M == 0) return hipSuccess;
    return final ? launch_add_norm_t<1>(x, y, w_post, w_next, eps, xn, out, M, H, st)
                 : launch_add_norm_t<0>(x, y, w_post, w_next, eps, xn, out, M, H, st);
}

hipError_t launch_qk_norm_rope(bf16_t* qkv, const int32_t* pos, const float* wq, const float* wk,
                               const float* cos_sin, float eps, float q_scale, uint32_t M, uint32_t heads,
                               uint32_t kv_heads, int k_only, hipStream_t st) {
    if (M == 0) return hipSuccess;
    if (heads + kv_heads > (uint32_t)kMaxQkHeads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qk_norm_rope_kernel, dim3((M + 3u) / 4u), dim3(256), 0, st, qkv, pos, wq, wk, cos_sin, eps,
                       q_scale, M, heads, kv_heads, k_only ? heads : 0u);
    return hipGetLastError();
}

hipError_t launch_kv_prep(bf16_t* qkv, bf16_t* vt, const int32_t* pos, const float* wq, const float* wk,
                          const float* cos_sin, float eps, float q_scale, uint32_t M, uint32_t heads, uint32_t kv_heads,
                          const int32_t* blk, uint32_t nblk, const int32_t* seq_start, const int32_t* seq_len,
                          const int32_t* vt_start, uint32_t vt_ld, int with_vt, hipStream_t st) {
    if (M == 0 || nblk == 0) return hipSuccess;
    if (kv_heads > (uint32_t)kMaxQkHeads) return hipErrorInvalidValue;
    const uint32_t n_rope = (M + 3u) / 4u, n_vt = with_vt ? nblk * 2u * kv_heads * 4u : 0u;
    hipLaunchKernelGGL(kv_prep_kernel, dim3(n_rope + n_vt), dim3(256), 0, st, qkv, vt, pos, wq, wk, cos_sin, eps, q_scale, M,
                       heads, kv_heads, n_rope, blk, nblk, seq_start, seq_len, vt_start, vt_ld);
    return hipGetLastError();
}

hipError_t launch_v_transpose(const bf16_t* qkv, bf16_t* vt, const int32_t* blk, uint32_t nblk,
                              const int32_t* seq_start, const int32_t* seq_len, const int32_t* vt_start, uint32_t heads,
                              uint32_t kv_heads, uint32_t vt_ld, hipStream_t st) {
    if (nblk == 0) return hipSuccess;
    hipLaunchKernelGGL(v_transpose_kernel, dim3(nblk * 2u, kv_heads * 4u), dim3(256), 0, st, qkv, vt, blk, seq_start, seq_len,
                       vt_start, heads, kv_heads, vt_ld);
    return hipGetLastError();
}

hipError_t launch_mean_pool(const float* hidden, const int32_t* seq_start, const int32_t* seq_len, bf16_t* pooled,
                            uint32_t B, uint32_t H, hipStream_t st) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(mean_pool_kernel, dim3(B, H / 256u), dim3(1024), 0, st, hidden, seq_start, seq_len, pooled, H);
    return hipGetLastError();
}

hipError_t launch_f32_to_bf16(const float* in, bf16_t* out, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, in, out, n);
    return hipGetLastError();
}

}  // namespace cqs
