// sparse_index_create.hip — the sparse index's constructors (from the documents, from the reference's postings map), destroy
// and the accessors.  What a constructor decides without the device - arguments, id order, token table, postings, range
// directories - is sparse_build_host.h; here the handle is allocated, filled and handed over.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "abi_guard.h"
#include "scan_kernels.h"
#include "sparse_build_host.h"
#include "sparse_internal.h"

namespace sb = cqs_sparse_build;

namespace {

void release(cqs_hip_sparse_index* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (void* p : {(void*)s->d_tags, (void*)s->d_post, (void*)s->d_chunk_of_rank, (void*)s->d_scores, (void*)s->d_gmax, (void*)s->d_work,
                    (void*)s->d_keep, (void*)s->d_qoff, (void*)s->d_dir, (void*)s->d_out_keys, (void*)s->d_out_count, (void*)s->d_dbg})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)s->h_keep, (void*)s->h_out_keys, (void*)s->h_qoff})      // (d_terms / h_terms point into the qoff blocks)
        if (p) (void)hipHostFree(p);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

// Second half of every constructor: `s->tok` / `s->off` and the host posting array are final; device, wave ranges, range
// directories, scratch.  On failure create_handle releases the handle.
int32_t finish_create(cqs_hip_sparse_index* s, const std::vector<sb::Posting>& post, int32_t device) {
    const uint64_t n = s->n, P = s->n_postings;
    auto dfail = [&](hipError_t he) -> int32_t {           // (the caller's guard releases)
        return he == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE;
    };
    hipError_t he = hipSetDevice(device);
    if (he != hipSuccess) return dfail(he);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cu = (uint32_t)prop.multiProcessorCount;
    // n_pad, the waves' ranges, the select's group size and which lists get a range directory: sparse_geometry.h (shared
    // with the in-place updates)
    const cqs::SparseGeometry geo = cqs::sparse_geometry(n, s->n_cu);
    s->n_pad = geo.n_pad;
    s->rw = geo.rw;
    s->sh = geo.sh;
    s->group16 = geo.group16;
    {
        s->dir_entries = cqs::sparse_plan_directories(s->off, geo, &s->dir_off);
        std::vector<uint32_t> dirs;
        sb::fill_directories(post.data(), s->off, s->dir_off, geo, &dirs);
        if ((he = hipMalloc((void**)&s->d_dir, std::max<size_t>(dirs.size(), 1) * 4)) != hipSuccess) return dfail(he);
        if (!dirs.empty() && (he = hipMemcpy(s->d_dir, dirs.data(), dirs.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return dfail(he);
    }
    if ((he = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)) != hipSuccess) return dfail(he);
    if ((he = hipEventCreate(&s->ev0)) != hipSuccess || (he = hipEventCreate(&s->ev1)) != hipSuccess) return dfail(he);
    if ((he = hipMalloc((void**)&s->d_post, std::max<size_t>((size_t)P, 1) * sizeof(uint2))) != hipSuccess) return dfail(he);
    if (P && (he = hipMemcpy(s->d_post, post.data(), (size_t)P * sizeof(uint2), hipMemcpyHostToDevice)) != hipSuccess) return dfail(he);
    if (s->ranked) {
        if ((he = hipMalloc((void**)&s->d_chunk_of_rank, std::max<size_t>((size_t)n, 1) * 4)) != hipSuccess) return dfail(he);
        if (n && (he = hipMemcpy(s->d_chunk_of_rank, s->chunk_of_rank.data(), (size_t)n * 4, hipMemcpyHostToDevice)) != hipSuccess) return dfail(he);
    }
    if ((he = hipMalloc((void**)&s->d_work, cqs::kWorkWords * 4)) != hipSuccess) return dfail(he);
    if ((he = hipMemset(s->d_work, 0, cqs::kWorkWords * 4)) != hipSuccess) return dfail(he);
    if ((he = hipMalloc((void**)&s->d_keep, (size_t)(s->n_pad / 32u) * 4)) != hipSuccess) return dfail(he);
    if ((he = hipHostMalloc((void**)&s->h_keep, (size_t)(s->n_pad / 32u) * 4, hipHostMallocDefault)) != hipSuccess) return dfail(he);
    {
        const int32_t rc = cqs_sparse::ensure_batch(s, 1u);
        if (rc != CQS_HIP_OK) return rc;
    }
    if (const char* e = getenv("CQS_HIP_DEBUG_STAMPS"); e && *e == '1')
        if (hipMalloc((void**)&s->d_dbg, 16 * 8) == hipSuccess) (void)hipMemset(s->d_dbg, 0, 16 * 8);
    if (const char* e = getenv("CQS_HIP_COMBINE")) s->combine = !(e[0] == '0');
    s->cq.wait_us = cqs_combine::wait_us_from_env();
    return CQS_HIP_OK;
}

}  // namespace

int32_t cqs_sparse::create_handle(int32_t device, const Fill& fill, cqs_hip_sparse_index** out) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return CQS_HIP_ERR_NO_DEVICE;
    struct Guard {                                         // an exception or an early return frees what exists so far
        cqs_hip_sparse_index* p;
        ~Guard() { if (p) release(p); }
    } guard{new cqs_hip_sparse_index()};
    cqs_hip_sparse_index* const s = guard.p;
    s->device = device;
    std::vector<sb::Posting> post;
    if (!fill(s, &post)) return CQS_HIP_ERR_INVALID;
    s->n_postings = post.size();
    const int32_t rc = finish_create(s, post, device);
    if (rc != CQS_HIP_OK) return rc;
    guard.p = nullptr;
    *out = s;
    return CQS_HIP_OK;
}

extern "C" {

int32_t cqs_hip_sparse_index_create(const uint64_t* doc_off, const uint32_t* tokens, const float* weights, uint64_t n,
                                    const uint32_t* id_rank, int32_t device, cqs_hip_sparse_index** out) CQS_ABI_TRY {
    if (!out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    const char* why = "";
    if (n >= cqs::kSparseMaxChunks || !sb::check_csr(doc_off, n, tokens, weights, &why)) return CQS_HIP_ERR_INVALID;
    return cqs_sparse::create_handle(device, [&](cqs_hip_sparse_index* s, std::vector<sb::Posting>* post) {
        if (!sb::rank_table(n, id_rank, &s->chunk_of_rank)) return false;   // id_rank is not a permutation of 0 .. n - 1
        s->n = n;
        s->ranked = id_rank != nullptr;
        sb::Built x = sb::from_documents(doc_off, tokens, weights, n, s->chunk_of_rank);
        s->tok.swap(x.tok);
        s->off.swap(x.off);
        post->swap(x.post);
        return true;
    }, out);
} CQS_ABI_CATCH_NOHANDLE

int32_t cqs_hip_sparse_index_create_inverted(const uint32_t* token_ids, const uint64_t* list_off, const uint32_t* post_chunks,
                                             const float* post_weights, uint64_t n_tokens, uint64_t n, const uint32_t* id_rank,
                                             int32_t device, cqs_hip_sparse_index** out) CQS_ABI_TRY {
    if (!out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    const char* why = "";
    if (n >= cqs::kSparseMaxChunks || n_tokens > 0xFFFFFFFFull || (n_tokens && !token_ids)) return CQS_HIP_ERR_INVALID;
    if (!sb::check_csr(list_off, n_tokens, post_chunks, post_weights, &why)) return CQS_HIP_ERR_INVALID;
    return cqs_sparse::create_handle(device, [&](cqs_hip_sparse_index* s, std::vector<sb::Posting>* post) {
        if (!sb::rank_table(n, id_rank, &s->chunk_of_rank)) return false;
        s->n = n;
        s->ranked = id_rank != nullptr;
        sb::Built x;
        if (!sb::from_inverted(token_ids, list_off, post_chunks, post_weights, n_tokens, n, s->chunk_of_rank, &x)) return false;
        s->tok.swap(x.tok);
        s->off.swap(x.off);
        post->swap(x.post);
        return true;
    }, out);
} CQS_ABI_CATCH_NOHANDLE

void cqs_hip_sparse_index_destroy(cqs_hip_sparse_index* s) CQS_ABI_TRY {
    release(s);
} CQS_ABI_CATCH_VOID

uint64_t cqs_hip_sparse_index_len(const cqs_hip_sparse_index* s) CQS_ABI_TRY {
    return s ? s->n : 0;
} CQS_ABI_CATCH_VAL(0)

uint64_t cqs_hip_sparse_index_unique_tokens(const cqs_hip_sparse_index* s) CQS_ABI_TRY {
    return s ? (uint64_t)s->tok.size() : 0;
} CQS_ABI_CATCH_VAL(0)

uint64_t cqs_hip_sparse_index_postings(const cqs_hip_sparse_index* s) CQS_ABI_TRY {
    return s ? s->n_postings : 0;
} CQS_ABI_CATCH_VAL(0)

int32_t cqs_hip_sparse_index_poisoned(const cqs_hip_sparse_index* s) CQS_ABI_TRY {
    if (!s) return 0;
    return s->poisoned.load(std::memory_order_acquire) ? 1 : 0;
} CQS_ABI_CATCH_VAL(0)

size_t cqs_hip_sparse_index_last_error(const cqs_hip_sparse_index* s, char* buf, size_t cap) CQS_ABI_TRY {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<cqs_hip_sparse_index*>(s)->mu);
    if (buf && cap) {
        const size_t m = std::min(cap - 1, s->last_error.size());
        memcpy(buf, s->last_error.data(), m);
        buf[m] = 0;
    }
    return s->last_error.size();
} CQS_ABI_CATCH_VAL(0)

}  // extern "C"
