// index.hip — host side of libcqs_hip.so: the exact GPU index behind the C ABI
// of include/cqs_hip.h.  Shape follows the reference's GPU backend exemplar
// `CagraIndex` (src/cagra.rs:255-277): a flat [n, dim] f32 dataset resident on
// the device, device work serialised behind one mutex (src/cagra.rs:263), a
// poisoned flag instead of panics (src/cagra.rs:472-489), stream sync before
// teardown (src/cagra.rs:289-302).  The id_map (row -> chunk id) stays with
// the caller (the Rust shim), as rows are addressed by integer here.  This file: scratch, create / extend / destroy, the
// block runner of the host search and the search entry points.  The device-free rules those apply are search_host.h's,
// the blob format is index_persist.hip's, the combining queue index_combine.hip's, the shadow scans index_shadow.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "abi_guard.h"
#include "roctx.h"
#include "index_internal.h"
#include "scan_bf16.h"
#include "scan_i8.h"
#include "search_host.h"

using cqs::kMaxK;
using cqs::kRowsPerBlock;

namespace cqs_idx {

uint64_t pad_rows(uint64_t n) { return (n + kRowsPerBlock - 1) / kRowsPerBlock * kRowsPerBlock; }

int32_t fail(cqs_hip_index* idx, int32_t code, const char* what, hipError_t e) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(buf, sizeof buf, "%s", what);
    if (idx) {
        idx->last_error = buf;
        if (code == CQS_HIP_ERR_DEVICE) idx->poisoned.store(true, std::memory_order_release);
    }
    return code;
}

void free_scratch(cqs_hip_index* x) {
    hipFree(x->d_q); hipFree(x->d_scores); hipFree(x->d_gmax); hipFree(x->d_work); hipFree(x->d_gaux);
    x->d_work = nullptr; x->d_gaux = nullptr;
    hipFree(x->d_out_keys); hipFree(x->d_out_counts);
    hipHostFree(x->h_q); hipHostFree(x->h_out_keys); hipHostFree(x->h_out_counts);
    x->d_q = x->d_scores = nullptr; x->d_gmax = nullptr;
    x->d_out_keys = nullptr; x->d_out_counts = nullptr;
    x->h_q = nullptr; x->h_out_keys = nullptr; x->h_out_counts = nullptr;
    x->h_out_keys_dev = nullptr; x->h_out_counts_dev = nullptr;
    x->q_cap = 0; x->k_cap = 0; x->scr_n_pad = 0;
}

// Make the scratch hold `b` queries at top-`k` for the current n.
int32_t ensure_scratch(cqs_hip_index* x, uint32_t b, uint32_t k) {
    const uint64_t n_pad = pad_rows(x->n);
    if (b <= x->q_cap && k <= x->k_cap && n_pad == x->scr_n_pad) return CQS_HIP_OK;
    HIP_TRY(x, hipDeviceSynchronize());  // searches may be in flight on caller streams
    uint32_t qc = x->q_cap > b ? x->q_cap : b;
    uint32_t kc = x->k_cap > k ? x->k_cap : k;
    free_scratch(x);
    // query block, padded with zero rows to the MFMA query tile (<= 256 past the last chunk)
    HIP_TRY(x, hipMalloc(&x->d_q, ((size_t)qc + 256) * x->dim * sizeof(float)));
    HIP_TRY(x, hipMalloc(&x->d_scores, (size_t)qc * n_pad * sizeof(float)));
    HIP_TRY(x, hipMalloc(&x->d_work, cqs::kWorkWords * sizeof(uint32_t)));
    // work-queue heads must be zero on entry; every search re-zeroes them
    HIP_TRY(x, hipMemset(x->d_work, 0, cqs::kWorkWords * sizeof(uint32_t)));
    HIP_TRY(x, hipMalloc(&x->d_gmax, (size_t)qc * (n_pad / cqs::kTaskRowsSmall) * sizeof(float)));
    // (argmax, runner-up) per task: gemv blocks only (<= kGauxQueries queries; larger blocks run on the matrix cores or,
    // gemv_only, without it)
    HIP_TRY(x, hipMalloc(&x->d_gaux, (size_t)(qc < kGauxQueries ? qc : kGauxQueries) * (n_pad / cqs::kTaskRowsSmall) * sizeof(uint64_t)));
    HIP_TRY(x, hipMalloc(&x->d_out_keys, (size_t)qc * kc * sizeof(uint64_t)));
    HIP_TRY(x, hipMalloc(&x->d_out_counts, (size_t)qc * sizeof(uint32_t)));
    HIP_TRY(x, hipHostMalloc(&x->h_q, (size_t)qc * x->dim * sizeof(float), hipHostMallocDefault));
    HIP_TRY(x, hipHostMalloc(&x->h_out_keys, (size_t)qc * kc * sizeof(uint64_t), hipHostMallocDefault));
    HIP_TRY(x, hipHostMalloc(&x->h_out_counts, (size_t)qc * sizeof(uint32_t), hipHostMallocDefault));
    // device-visible addresses of the two result buffers (small blocks: the select kernel writes them directly);
    // a runtime that cannot map them leaves the pointers null and every block takes the copy path
    if (hipHostGetDevicePointer((void**)&x->h_out_keys_dev, x->h_out_keys, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&x->h_out_counts_dev, x->h_out_counts, 0) != hipSuccess) {
        (void)hipGetLastError();
        x->h_out_keys_dev = nullptr; x->h_out_counts_dev = nullptr;
    }
    x->q_cap = qc; x->k_cap = kc; x->scr_n_pad = n_pad;
    return CQS_HIP_OK;
}

// Largest query block whose score rows fit the scratch budget (score matrix
// is b * n_pad f32).  16 GiB default: 256 queries x 10M rows fit in one pass.
uint32_t max_query_block(const cqs_hip_index* x) {
    const uint64_t budget = 16ull << 30;
    const uint64_t per_q = pad_rows(x->n) * sizeof(float);
    uint64_t q = per_q ? budget / per_q : 1024;
    if (q < 1) q = 1;
    if (q > 1024) q = 1024;
    return (uint32_t)q;
}

cqs::ScanArgs scan_args(const cqs_hip_index* x, const float* d_q, uint32_t b, uint32_t k, const uint32_t* d_keep,
                        uint32_t mode, float thr, size_t elem_bytes, bool gemv_only, void* dbg, const uint32_t* gate,
                        const KeepTab* tab) {
    cqs::ScanArgs a;
    a.rows = x->d_rows;
    a.n = (uint32_t)x->n;
    a.n_pad = (uint32_t)pad_rows(x->n);
    a.dim = x->dim;
    a.q = d_q;
    a.b = b;
    a.scores = x->d_scores;
    a.keep = d_keep;
    a.mode = mode;
    a.threshold = thr;
    a.nontemporal = x->n * x->dim * elem_bytes > kNtBytes;
    a.linear_bins = (x->metric == CQS_HIP_METRIC_COSINE) || (mode == CQS_HIP_MODE_PIPELINE);
    a.k = k;
    a.gmax = x->d_gmax;
    a.gaux = (b <= kGauxQueries && k >= kGauxMinK) ? x->d_gaux : nullptr;
    a.work = x->d_work;
    a.n_cu = x->n_cu;
    a.dbg = dbg;
    a.gemv_only = gemv_only;
    a.tiers = cqs::plan_tiers(a.n_pad, x->n_cu, !gemv_only && cqs::uniform_groups(b, x->dim));
    a.gate = gate;
    if (tab) { a.keep_tab = tab->d_tab; a.keep_stride = tab->stride; a.keep_slot = tab->slot; }
    return a;
}

int32_t scan_select(cqs_hip_index* x, const cqs::ScanArgs& a, hipStream_t st, const ShadowRows* shadow,
                    uint64_t* out_keys, uint32_t* out_counts) {
    const bool timed = !a.gate && x->timing && x->ev_used + 2 <= kMaxTimingEvents;
    if (timed) {
        while (x->ev.size() < x->ev_used + 2) {
            hipEvent_t e = nullptr;
            HIP_TRY(x, hipEventCreate(&e));
            x->ev.push_back(e);
        }
        HIP_TRY(x, hipEventRecord(x->ev[x->ev_used], st));
    }
    if (shadow && shadow->bf16) HIP_TRY(x, cqs::launch_scan_bf16(a, shadow->bf16, shadow->bq, st));
    else if (shadow) HIP_TRY(x, cqs::launch_scan_i8(a, shadow->i8, shadow->i8_scale, shadow->bq, st));
    else HIP_TRY(x, cqs::launch_scan(a, st));
    if (timed) {
        HIP_TRY(x, hipEventRecord(x->ev[x->ev_used + 1], st));
        x->ev_used += 2;
    }
    if (out_keys) HIP_TRY(x, cqs::launch_select(a, (uint32_t)x->row_base, out_keys, out_counts, st));
    return CQS_HIP_OK;
}

// Enqueue scan + select for queries already on the device.  Caller holds mu.
int32_t enqueue_search(cqs_hip_index* x, const float* d_q, uint32_t b, uint32_t k, const uint32_t* d_keep,
                       uint32_t mode, float thr, uint64_t* d_out_keys, uint32_t* d_out_counts, hipStream_t st, bool gemv_only,
                       const uint32_t* gate, const KeepTab* tab) {
    HIP_TRY(x, order_after_last(x, st));   // the previous search may still be running on another stream and owns the same scratch
    if (!gemv_only && cqs::use_mfma(b, x->dim)) {
        // the matrix-core path reads whole query tiles: stage the block in d_q with a zero tail
        const size_t qbytes = (size_t)b * x->dim * sizeof(float);
        if (d_q != x->d_q) HIP_TRY(x, hipMemcpyAsync(x->d_q, d_q, qbytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(x, hipMemsetAsync((char*)x->d_q + qbytes, 0, (size_t)256 * x->dim * sizeof(float), st));
        d_q = x->d_q;
    }
    cqs::ScanArgs a = scan_args(x, d_q, b, k, d_keep, mode, thr, sizeof(float), gemv_only, x->d_dbg, gate, tab);
    static const bool use_gaux = [] { const char* e = getenv("CQS_HIP_SELECT_AUX"); return !(e && e[0] == '0'); }();   // A/B hook
    // The index only where the gather it replaces is long (scan_args): at k = 20 it costs what it saves (same-box A/B, 1M x 768,
    // scan + select per step: k = 20 0.4698 with / 0.4667 ms without; k = 500 0.4783 / 0.4825 - tools/ab_select_aux.sh).
    if (!use_gaux) a.gaux = nullptr;
    const int32_t rc = scan_select(x, a, st, nullptr, d_out_keys, d_out_counts);
    if (rc == CQS_HIP_OK) HIP_TRY(x, record_done(x, st));
    return rc;
}

// Wait (host) for the last enqueued search, whatever stream it ran on.  Caller holds mu.
hipError_t quiesce(cqs_hip_index* x) {
    hipError_t e = x->stream ? hipStreamSynchronize(x->stream) : hipSuccess;
    if (e == hipSuccess && x->done_valid) e = hipEventSynchronize(x->done);
    return e;
}

// Copy a host keep-bitset (`words` u32) into the handle's device copy on its stream.  Caller holds mu.
int32_t ensure_keep(cqs_hip_index* x, uint64_t words) {
    if (words <= x->keep_words_cap) return CQS_HIP_OK;
    HIP_TRY(x, quiesce(x));
    hipFree(x->d_keep);
    x->d_keep = nullptr;
    x->keep_words_cap = 0;
    HIP_TRY(x, hipMalloc(&x->d_keep, words * sizeof(uint32_t)));
    x->keep_words_cap = words;
    return CQS_HIP_OK;
}

int32_t stage_keep(cqs_hip_index* x, const uint32_t* host_words, uint64_t words) {
    const int32_t rc = ensure_keep(x, words);
    if (rc != CQS_HIP_OK) return rc;
    HIP_TRY(x, hipMemcpyAsync(x->d_keep, host_words, words * sizeof(uint32_t), hipMemcpyHostToDevice, x->stream));
    return CQS_HIP_OK;
}

void free_keep_tab(cqs_hip_index* x) {
    hipFree(x->d_keep_tab);
    hipHostFree(x->h_keep_tab);
    x->d_keep_tab = nullptr; x->h_keep_tab = nullptr; x->keep_tab_stride = 0;
}

bool ensure_keep_tab(cqs_hip_index* x) {
    const uint64_t cap = x->cap_rows > x->n ? x->cap_rows : x->n;
    const uint64_t stride = (cap + 31) / 32;
    if (x->d_keep_tab && x->keep_tab_stride >= stride) return true;
    if (stride > 0xFFFFFFFFull || quiesce(x) != hipSuccess) return false;   // (a search in flight may read the old table)
    free_keep_tab(x);
    const size_t bytes = (size_t)kCombineCap * stride * sizeof(uint32_t);
    if (hipMalloc(&x->d_keep_tab, bytes) != hipSuccess || hipHostMalloc(&x->h_keep_tab, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        free_keep_tab(x);
        return false;
    }
    x->keep_tab_stride = stride;
    return true;
}

void read_combine_env(cqs_hip_index* x) {                                              // read once per handle
    if (const char* ce = getenv("CQS_HIP_COMBINE")) x->combine = ce[0] != '0';
    if (const char* cf = getenv("CQS_HIP_COMBINE_FILTERED")) x->combine_filtered = cf[0] != '0';
    if (const char* ct = getenv("CQS_HIP_COMBINE_TAGGED")) x->combine_tagged = ct[0] != '0';
    x->cq.wait_us = cqs_combine::wait_us_from_env();
    if (const char* cb = getenv("CQS_HIP_COMBINE_BITS")) x->combine_relaxed = cb[0] == 'r';
}

int32_t create_common(uint64_t n, uint32_t dim, uint32_t metric, int32_t device, uint64_t row_base,
                      cqs_hip_index** out, cqs_hip_index** made) {
    if (!out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    if (!cqs::scan_dim_supported(dim) || metric > CQS_HIP_METRIC_DOT) return CQS_HIP_ERR_INVALID;
    if (n + row_base > 0xFFFFFFFEull) return CQS_HIP_ERR_INVALID;  // row ids are packed in 32 bits
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return CQS_HIP_ERR_NO_DEVICE;
    if (device < 0 || device >= cnt) return CQS_HIP_ERR_INVALID;
    cqs_hip_index* x = new (std::nothrow) cqs_hip_index();
    if (!x) return CQS_HIP_ERR_NOMEM;
    x->device = device; x->n = n; x->dim = dim; x->metric = metric; x->row_base = row_base;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&x->done, hipEventDisableTiming) != hipSuccess) {
        if (x->stream) hipStreamDestroy(x->stream);
        delete x;
        return CQS_HIP_ERR_DEVICE;
    }
    read_combine_env(x);
    if (getenv("CQS_HIP_DEBUG_STAMPS")) {
        const size_t bytes = (cqs::kDbgTailSlow + cqs::kDbgTailSlowWords) * sizeof(unsigned long long);
        if (hipMalloc(&x->d_dbg, bytes) == hipSuccess) (void)hipMemset(x->d_dbg, 0, bytes);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        x->n_cu = (uint32_t)prop.multiProcessorCount;
    *made = x;
    return CQS_HIP_OK;
}

}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

const char* cqs_hip_version(void) CQS_ABI_TRY { return "cqs-hip 0.1.0 (gfx950)"; } CQS_ABI_CATCH_VAL("cqs-hip")

int32_t cqs_hip_device_count(void) CQS_ABI_TRY {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
} CQS_ABI_CATCH_NOHANDLE

int32_t cqs_hip_device_mem(int32_t device, uint64_t* free_bytes, uint64_t* total_bytes) CQS_ABI_TRY {
    if (hipSetDevice(device) != hipSuccess) return CQS_HIP_ERR_NO_DEVICE;
    size_t f = 0, t = 0;
    if (hipMemGetInfo(&f, &t) != hipSuccess) return CQS_HIP_ERR_DEVICE;
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

}  // extern "C"

int32_t cqs_idx::create_owned(const float* rows, uint64_t n, uint32_t dim, uint32_t metric, int32_t device,
                              uint64_t row_base, cqs_hip_index** out) {
    if (n > 0 && !rows) return CQS_HIP_ERR_INVALID;
    cqs_hip_index* x = nullptr;
    int32_t rc = create_common(n, dim, metric, device, row_base, out, &x);
    if (rc != CQS_HIP_OK) return rc;
    x->cap_rows = n ? n : 1;
    hipError_t e = hipMalloc(&x->d_rows, (size_t)x->cap_rows * dim * sizeof(float));
    if (e == hipSuccess && n)
        e = hipMemcpyAsync(x->d_rows, rows, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
    if (e != hipSuccess) {
        cqs_hip_index_destroy(x);
        return e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE;
    }
    *out = x;
    return CQS_HIP_OK;
}

extern "C" {

int32_t cqs_hip_index_create(const float* rows, uint64_t n, uint32_t dim, uint32_t metric, int32_t device,
                             uint64_t row_base, cqs_hip_index** out) CQS_ABI_TRY {
    cqs_hip_index* x = nullptr;
    int32_t rc = create_owned(rows, n, dim, metric, device, row_base, &x);
    if (rc != CQS_HIP_OK) return rc;
    if ((rc = shadow_auto(x)) != CQS_HIP_OK) { cqs_hip_index_destroy(x); return rc; }
    *out = x;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

int32_t cqs_hip_index_create_device(const void* d_rows, uint64_t n, uint32_t dim, uint32_t metric, int32_t device,
                                    uint64_t row_base, int32_t borrow, cqs_hip_index** out) CQS_ABI_TRY {
    if (n > 0 && !d_rows) return CQS_HIP_ERR_INVALID;
    if (((uintptr_t)d_rows & 15u) != 0) return CQS_HIP_ERR_INVALID;  // 16-B row loads
    cqs_hip_index* x = nullptr;
    int32_t rc = create_common(n, dim, metric, device, row_base, out, &x);
    if (rc != CQS_HIP_OK) return rc;
    // The rows may still be in flight from the caller's own streams (torch's null stream, say), which the handle's
    // non-blocking stream does not order after: wait for the device before the copy or the shadow build reads them.
    if (n && hipDeviceSynchronize() != hipSuccess) { cqs_hip_index_destroy(x); return CQS_HIP_ERR_DEVICE; }
    if (borrow) {
        x->borrow = true;
        x->d_rows = (float*)d_rows;
        x->cap_rows = n;
    } else {
        x->cap_rows = n ? n : 1;
        hipError_t e = hipMalloc(&x->d_rows, (size_t)x->cap_rows * dim * sizeof(float));
        if (e == hipSuccess && n)
            e = hipMemcpyAsync(x->d_rows, d_rows, (size_t)n * dim * sizeof(float), hipMemcpyDeviceToDevice, x->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
        if (e != hipSuccess) {
            cqs_hip_index_destroy(x);
            return e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE;
        }
    }
    // borrowed: the shadow is a snapshot of the caller's rows, which the header requires to stay unmodified
    if ((rc = shadow_auto(x)) != CQS_HIP_OK) { cqs_hip_index_destroy(x); return rc; }
    *out = x;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

int32_t cqs_hip_index_extend(cqs_hip_index* x, const float* rows, uint64_t n_new) CQS_ABI_TRY {
    if (!x) return CQS_HIP_ERR_INVALID;
    if (x->sh) return cqs_sharded::extend(x, rows, n_new);
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (x->borrow) return fail(x, CQS_HIP_ERR_INVALID, "extend: index borrows its rows");
    if (n_new == 0) return CQS_HIP_OK;
    if (!rows) return fail(x, CQS_HIP_ERR_INVALID, "extend: null rows");
    if (x->n + n_new + x->row_base > 0xFFFFFFFEull) return fail(x, CQS_HIP_ERR_INVALID, "extend: row id overflow");
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // a search enqueued on a caller stream may still read d_rows
    const size_t row_bytes = (size_t)x->dim * sizeof(float);
    if (x->n + n_new > x->cap_rows) {  // grow geometrically, copy device-to-device
        uint64_t cap = x->cap_rows * 2;
        if (cap < x->n + n_new) cap = x->n + n_new;
        float* nd = nullptr;
        HIP_TRY(x, hipMalloc(&nd, cap * row_bytes));
        hipError_t e = hipMemcpyAsync(nd, x->d_rows, x->n * row_bytes, hipMemcpyDeviceToDevice, x->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
        if (e != hipSuccess) {
            hipFree(nd);
            return fail(x, CQS_HIP_ERR_DEVICE, "extend: copy", e);
        }
        hipFree(x->d_rows);
        x->d_rows = nd;
        x->cap_rows = cap;
        if (x->d_keep_tab) (void)ensure_keep_tab(x);   // (a failure leaves no table: filtered calls run one by one)
        if (x->d_tags) tags_regrow(x);                 // (a failure leaves no tags: search_tagged refuses until set_tags)
    }
    HIP_TRY(x, hipMemcpyAsync(x->d_rows + x->n * x->dim, rows, n_new * row_bytes, hipMemcpyHostToDevice, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    const uint64_t n_old = x->n;
    x->n += n_new;
    return shadow_extend(x, n_old);
} CQS_ABI_CATCH(x)

}  // extern "C"

extern "C" {

void cqs_hip_index_destroy(cqs_hip_index* x) CQS_ABI_TRY {
    if (!x) return;
    if (x->sh) { cqs_sharded::destroy(x); return; }
    hipSetDevice(x->device);
    (void)quiesce(x);  // src/cagra.rs:289-302 (incl. searches enqueued on caller streams)
    free_scratch(x);
    cqs_mmr::free_scratch(x);
    shadow_free(x);
    tags_free(x);
    update_free(x);
    knn_free(x);
    diff_free(x);
    match_free(x);
    hipFree(x->d_keep);
    free_keep_tab(x);
    hipFree(x->d_dbg);
    if (!x->borrow) hipFree(x->d_rows);
    for (hipEvent_t e : x->ev) hipEventDestroy(e);
    if (x->done) hipEventDestroy(x->done);
    if (x->stream) hipStreamDestroy(x->stream);
    delete x;
} CQS_ABI_CATCH_VOID

uint64_t cqs_hip_index_len(const cqs_hip_index* x) CQS_ABI_TRY { return x ? (x->sh ? cqs_sharded::len(x) : x->n) : 0; } CQS_ABI_CATCH_VAL(0)
uint32_t cqs_hip_index_dim(const cqs_hip_index* x) CQS_ABI_TRY { return x ? x->dim : 0; } CQS_ABI_CATCH_VAL(0)
uint32_t cqs_hip_index_metric(const cqs_hip_index* x) CQS_ABI_TRY { return x ? x->metric : 0; } CQS_ABI_CATCH_VAL(0)
uint32_t cqs_hip_index_max_k(const cqs_hip_index* x) CQS_ABI_TRY { (void)x; return kMaxK; } CQS_ABI_CATCH_VAL(0)
int32_t cqs_hip_index_poisoned(const cqs_hip_index* x) CQS_ABI_TRY {
    if (x && x->sh) return cqs_sharded::poisoned(x);
    return x && x->poisoned.load(std::memory_order_acquire) ? 1 : 0;
} CQS_ABI_CATCH_NOHANDLE
int32_t cqs_hip_index_device(const cqs_hip_index* x) CQS_ABI_TRY { return x ? x->device : -1; } CQS_ABI_CATCH_NOHANDLE
uint64_t cqs_hip_index_row_base(const cqs_hip_index* x) CQS_ABI_TRY { return x ? x->row_base : 0; } CQS_ABI_CATCH_VAL(0)

size_t cqs_hip_index_last_error(const cqs_hip_index* x, char* buf, size_t cap) CQS_ABI_TRY {
    if (!x || !buf || cap == 0) return 0;
    std::lock_guard<std::mutex> g(x->mu);   // (a row-sharded parent keeps its message on itself too)
    return cqs_search::copy_last_error(x->last_error.data(), x->last_error.size(), buf, cap);
} CQS_ABI_CATCH_VAL(0)

void cqs_hip_unpack_keys(const uint64_t* keys, size_t count, uint64_t* rows, float* scores) CQS_ABI_TRY {
    cqs_search::unpack_keys(keys, count, rows, scores);
} CQS_ABI_CATCH_VOID

size_t cqs_hip_merge_keys(const uint64_t* lists, const uint32_t* counts, size_t n_lists, size_t stride, size_t k,
                          uint64_t* out_keys) CQS_ABI_TRY {
    return cqs_search::merge_keys(lists, counts, n_lists, stride, k, out_keys);
} CQS_ABI_CATCH_VAL(0)

int32_t cqs_hip_index_search_device(cqs_hip_index* x, const float* d_queries, uint32_t b, uint32_t k,
                                    const uint32_t* d_keep_bitset, uint32_t mode, float threshold,
                                    uint64_t* d_out_keys, uint32_t* d_out_counts, void* stream) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_search_device");
    if (!x) return CQS_HIP_ERR_INVALID;
    if (x->sh) return CQS_HIP_ERR_INVALID;   // a row-sharded handle spans devices: host-buffer API only
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (b == 0) return CQS_HIP_OK;
    if (!d_queries || !d_out_keys || !d_out_counts) return fail(x, CQS_HIP_ERR_INVALID, "search_device: null buffer");
    if (k == 0 || k > kMaxK) return fail(x, CQS_HIP_ERR_INVALID, "search_device: k out of range");
    if (mode > CQS_HIP_MODE_PIPELINE) return fail(x, CQS_HIP_ERR_INVALID, "search_device: bad mode");
    if (b > max_query_block(x)) return fail(x, CQS_HIP_ERR_INVALID, "search_device: batch exceeds scratch budget");
    HIP_TRY(x, hipSetDevice(x->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the HIP null (legacy default) stream, e.g. torch's default stream
    if (x->n == 0) {
        HIP_TRY(x, hipMemsetAsync(d_out_counts, 0, (size_t)b * sizeof(uint32_t), st));
        return CQS_HIP_OK;
    }
    int32_t rc = ensure_scratch(x, b, k);
    if (rc != CQS_HIP_OK) return rc;
    // Through the bf16 shadow, no host sync: certify writes the answers into the caller's buffers and its verdicts into the
    // gate words.  The f32 scan + select that follow return at entry when every query is certified, else recompute the whole
    // block, which is harmless (gemv-pass scores do not depend on which queries share a pass; a certified answer is the f32
    // one).  `done` is recorded after the gated select, so the cross-stream hand-off covers the shadow's scratch too.
    // Where it applies the fallback is ONE gated launch instead (shadow_fallback: an exact brute-force top-k of the block).
    const uint32_t* gate = nullptr;
    if (shadow_takes(x, b, k, /*gemv_only=*/false)) {
        if ((rc = shadow_pass(x, d_queries, b, k, d_keep_bitset, mode, threshold, d_out_keys, d_out_counts, st, &gate)) != CQS_HIP_OK)
            return rc;
        bool taken = false;
        rc = shadow_fallback(x, d_queries, b, k, d_keep_bitset, mode, threshold, d_out_keys, d_out_counts, st, gate, &taken);
        if (rc != CQS_HIP_OK || taken) return rc;
    }
    return enqueue_search(x, d_queries, b, k, d_keep_bitset, mode, threshold, d_out_keys, d_out_counts, st, false, gate);
} CQS_ABI_CATCH(x)

}  // extern "C"

namespace cqs_idx {

// Debug print of the kernels' stamps (CQS_HIP_DEBUG_STAMPS=1).  Caller holds mu; the stream is idle.
static void print_debug_stamps(cqs_hip_index* x) {
    unsigned long long h[16];   // 100 MHz realtime counter: 10 ns ticks
    if (hipMemcpy(h, x->d_dbg, sizeof h, hipMemcpyDeviceToHost) == hipSuccess)
        fprintf(stderr, "[cqs_hip] select_finish us: zero %.2f hist %.2f decide %.2f groups %.2f scores %.2f sort %.2f emit %.2f | groups=%llu cand=%llu\n",
                0.0, (h[1] - h[0]) / 100.0, (h[2] - h[1]) / 100.0, (h[3] - h[2]) / 100.0, (h[4] - h[3]) / 100.0,
                (h[5] - h[4]) / 100.0, (h[6] - h[5]) / 100.0, h[8], h[9]);
    // scan waves: spread of start and end times relative to the first wave's start
    std::vector<unsigned long long> w(2 * cqs::kDbgWaves);
    if (hipMemcpy(w.data(), x->d_dbg + 16, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return;
    std::vector<double> st, en;
    unsigned long long t0 = ~0ull;
    for (uint32_t i = 0; i < cqs::kDbgWaves; ++i) if (w[2 * i] && w[2 * i] < t0) t0 = w[2 * i];
    for (uint32_t i = 0; i < cqs::kDbgWaves; ++i)
        if (w[2 * i] && w[2 * i + 1]) { st.push_back((w[2 * i] - t0) / 100.0); en.push_back((w[2 * i + 1] - t0) / 100.0); }
    if (!st.empty()) {
        std::sort(st.begin(), st.end());
        std::sort(en.begin(), en.end());
        auto pc = [](const std::vector<double>& v, double f) { return v[(size_t)(f * (v.size() - 1))]; };
        fprintf(stderr, "[cqs_hip] scan waves=%zu start us p0 %.1f p50 %.1f p90 %.1f p100 %.1f | end us p0 %.1f p10 %.1f p50 %.1f p90 %.1f p100 %.1f | select ends %.1f\n",
                st.size(), pc(st, 0), pc(st, .5), pc(st, .9), pc(st, 1), pc(en, 0), pc(en, .1), pc(en, .5), pc(en, .9), pc(en, 1),
                (h[6] - t0) / 100.0);
    }
    (void)hipMemset(x->d_dbg + 16, 0, w.size() * sizeof(unsigned long long));
}

// The nq queries staged in h_q (row i answers qs[i]; null: non-finite, a zero row, no answer), one wait: the f32 scan, or
// with redo the bf16 shadow, whose uncovered queries go to *redo, restaged in order in h_q[0, redo->size()).  Caller holds
// mu; x->stream is ordered after the last search.  slots (with a null d_keep): query i is filtered by row slots[i] of the
// handle's bitset table; the uncovered queries' slots are compacted with their rows of h_q.
static int32_t host_block(cqs_hip_index* x, const cqs_combine_req* const* qs, uint32_t nq, uint8_t* slots, uint32_t k,
                          const uint32_t* d_keep, uint32_t mode, float thr, bool gemv_only, std::vector<const cqs_combine_req*>* redo) {
    const KeepTab table{x->d_keep_tab, (uint32_t)x->keep_tab_stride, slots};
    const KeepTab* tab = slots ? &table : nullptr;
    HIP_TRY(x, hipMemcpyAsync(x->d_q, x->h_q, (size_t)nq * x->dim * sizeof(float), hipMemcpyHostToDevice, x->stream));
    // Small blocks: the select kernel writes keys and counts straight into the pinned host buffers (device-visible
    // addresses): no copy calls behind the kernels, one wait.  Large blocks keep the device buffers + two copies
    // (hundreds of KB of scattered 8-byte stores over PCIe would cost more than the copies).
    const bool direct = x->h_out_keys_dev && x->h_out_counts_dev && (size_t)nq * k <= kDirectOutKeys;
    uint64_t* const keys = direct ? x->h_out_keys_dev : x->d_out_keys;
    uint32_t* const counts = direct ? x->h_out_counts_dev : x->d_out_counts;
    int32_t rc = redo ? shadow_pass(x, x->d_q, nq, k, d_keep, mode, thr, keys, counts, x->stream, nullptr, tab)
                      : enqueue_search(x, x->d_q, nq, k, d_keep, mode, thr, keys, counts, x->stream, gemv_only, nullptr, tab);
    if (rc != CQS_HIP_OK) return rc;
    if (redo) HIP_TRY(x, record_done(x, x->stream));
    if (!direct) {
        HIP_TRY(x, hipMemcpyAsync(x->h_out_keys, x->d_out_keys, (size_t)nq * k * sizeof(uint64_t), hipMemcpyDeviceToHost, x->stream));
        HIP_TRY(x, hipMemcpyAsync(x->h_out_counts, x->d_out_counts, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    }
    const uint32_t* cert = nullptr;   // the shadow's verdicts
    if (redo) HIP_TRY(x, shadow_verdicts(x, nq, &cert));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    if (!redo && x->d_dbg) print_debug_stamps(x);
    if (redo) redo->clear();
    uint64_t certified = 0;
    for (uint32_t i = 0; i < nq; ++i) {
        if (!qs[i]) continue;
        if (cert && !cert[i]) {   // restaged for the f32 scan (ascending, so rows only move down)
            if (redo->size() != i) memcpy(x->h_q + redo->size() * x->dim, x->h_q + (size_t)i * x->dim, (size_t)x->dim * sizeof(float));
            if (slots) slots[redo->size()] = slots[i];
            redo->push_back(qs[i]);
            continue;
        }
        const uint32_t c = x->h_out_counts[i] < k ? x->h_out_counts[i] : k;
        cqs_search::unpack_keys(x->h_out_keys + (size_t)i * k, c, qs[i]->out_rows, qs[i]->out_scores);
        *qs[i]->out_count = c;
        certified += cert ? 1 : 0;
    }
    x->stat_certified.fetch_add(certified, std::memory_order_relaxed);
    if (redo) x->stat_fallbacks.fetch_add(redo->size(), std::memory_order_relaxed);
    if (redo && shadow_uses_i8(x, nq, k)) {   // (the decision shadow_pass took: same handle state, same (b, k))
        x->stat_i8_certified.fetch_add(certified, std::memory_order_relaxed);
        x->stat_i8_fallbacks.fetch_add(redo->size(), std::memory_order_relaxed);
    }
    return CQS_HIP_OK;
}

// One staged block to its answers: through the shadow copies first when shadow_takes the block (blocks that run as gemv
// passes; the matrix-core blocks keep their path, their scores are not the gemv kernel's), then the f32 scan over the
// queries the certificate did not cover - same call, same slots.  `staged` is left in an unspecified state.
int32_t answer_block(cqs_hip_index* x, std::vector<const cqs_combine_req*>& staged, uint8_t* slots, uint32_t k,
                     const uint32_t* d_keep, uint32_t mode, float thr, bool gemv_only) {
    int32_t rc;
    if (shadow_takes(x, (uint32_t)staged.size(), k, gemv_only)) {
        std::vector<const cqs_combine_req*> redo;
        if ((rc = host_block(x, staged.data(), (uint32_t)staged.size(), slots, k, d_keep, mode, thr, gemv_only, &redo)) != CQS_HIP_OK) return rc;
        staged.swap(redo);
    }
    if (staged.empty()) return CQS_HIP_OK;
    return host_block(x, staged.data(), (uint32_t)staged.size(), slots, k, d_keep, mode, thr, gemv_only, nullptr);
}

// The test hook (cqs_hip_debug_index_fail_next), consumed: an armed hook fails this one host search as a device error would.
int32_t injected_failure(cqs_hip_index* x) {
    if (x->inject_fail.exchange(0, std::memory_order_acq_rel) == 0) return CQS_HIP_OK;
    return fail(x, CQS_HIP_ERR_DEVICE, "search: injected device failure (test hook)");
}

// The host-buffer search proper: `b` queries with one (k, mode, threshold, bitset), scanned in blocks the scratch
// budget allows.  Caller holds mu, has checked the arguments and zeroed the counts.  `gemv_only`: every block goes
// through the HBM-streaming passes of <= 8 queries, whose scores do not depend on how many queries share a pass (same
// per-lane FMA chain, same butterfly) - what the combining queue needs to hand each caller the bits it would have got alone.
int32_t search_host_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k, const uint32_t* keep_bitset,
                           uint32_t mode, float threshold, bool gemv_only) {
    int32_t rc = injected_failure(x);
    if (rc != CQS_HIP_OK || x->n == 0 || k == 0) return rc;   // src/cagra.rs:445-447
    HIP_TRY(x, hipSetDevice(x->device));
    // a device-API search on a caller stream may still use the shared scratch this call is about to overwrite
    HIP_TRY(x, order_after_last(x, x->stream));
    const uint32_t* d_keep = nullptr;
    uint32_t k_eff = k;
    const cqs_search::Keep kept = cqs_search::plan_keep(keep_bitset, x->n, &k_eff);   // on the host, src/cagra.rs:747-775
    if (kept == cqs_search::Keep::Empty) return CQS_HIP_OK;
    if (kept == cqs_search::Keep::Filtered) {
        if ((rc = stage_keep(x, keep_bitset, (x->n + 31) / 32)) != CQS_HIP_OK) return rc;
        d_keep = x->d_keep;
    }
    return search_blocks_locked(x, qs, b, k_eff, d_keep, mode, threshold, gemv_only);
}

// The block loop behind it, over a bitset that is already on the device (search_tagged builds its own there): the scratch
// budget's blocks, staged and answered one after the other.
int32_t search_blocks_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k_eff, const uint32_t* d_keep,
                             uint32_t mode, float threshold, bool gemv_only) {
    int32_t rc;
    const uint32_t blk = max_query_block(x);
    std::vector<const cqs_combine_req*> staged;
    for (uint32_t done = 0; done < b;) {
        const uint32_t nb = (b - done) < blk ? (b - done) : blk;
        if ((rc = ensure_scratch(x, nb, k_eff)) != CQS_HIP_OK) return rc;
        // a non-finite query stays in the block as a zero row with no answer (nb, and with it the kernels chosen, do not move)
        staged.clear();
        for (uint32_t i = 0; i < nb; ++i)
            staged.push_back(cqs_search::stage_query(x->h_q + (size_t)i * x->dim, qs[done + i].q, x->dim) ? &qs[done + i] : nullptr);
        if ((rc = answer_block(x, staged, nullptr, k_eff, d_keep, mode, threshold, gemv_only)) != CQS_HIP_OK) return rc;
        done += nb;
    }
    return CQS_HIP_OK;
}

// `b` queries with one (k, mode, threshold) and a bitset EACH (qs[i].keep), every one answered with the bytes of
// search_host_locked(&qs[i], 1, k, qs[i].keep, ...): blocks of <= kCombineCap queries whose bitsets are staged in the
// handle's table, run as gemv passes that read a batch of rows when any query of the pass keeps one of them and mask each
// query's scores with its own row (scan_gemv_kernel, PQ).  The block runs at the callers' k: a query that keeps fewer rows
// gets them all, as its lone call at k = kept rows does (filtered-out rows are -inf and never candidates).  A query that
// keeps nothing or is not finite is answered with count 0 and takes no slot.  Through the shadow copies under the rules of
// unfiltered blocks; the uncertified queries are redone on the f32 scan with their own table rows.  Caller holds mu, has
// checked the arguments and zeroed the counts.
int32_t search_filtered_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k, uint32_t mode, float threshold) {
    int32_t rc = injected_failure(x);
    if (rc != CQS_HIP_OK) return rc;
    if (b == 1) return search_host_locked(x, qs, 1, k, qs[0].keep, mode, threshold, /*gemv_only=*/true);   // a lone call: the shared-bitset kernels
    if (x->n == 0 || k == 0) return CQS_HIP_OK;
    HIP_TRY(x, hipSetDevice(x->device));
    if (!ensure_keep_tab(x)) {   // no memory for the table: one by one over d_keep
        for (uint32_t i = 0; i < b; ++i)
            if ((rc = search_host_locked(x, &qs[i], 1, k, qs[i].keep, mode, threshold, true)) != CQS_HIP_OK) return rc;
        return CQS_HIP_OK;
    }
    HIP_TRY(x, order_after_last(x, x->stream));
    const uint64_t words = (x->n + 31) / 32;
    std::vector<const cqs_combine_req*> staged;
    uint8_t slot[kCombineCap];
    for (uint32_t done = 0; done < b;) {
        // the next block: up to kCombineCap queries that have an answer, query i in h_q row i and table row i
        staged.clear();
        if ((rc = ensure_scratch(x, (b - done) < kCombineCap ? (b - done) : kCombineCap, k)) != CQS_HIP_OK) return rc;
        for (; done < b && staged.size() < kCombineCap; ++done) {
            const cqs_combine_req& r = qs[done];
            if (!cqs_search::query_finite(r.q, x->dim) || cqs_search::popcount_bits(r.keep, 0, x->n) == 0) continue;   // src/cagra.rs:464-470, :765-767
            memcpy(x->h_q + staged.size() * x->dim, r.q, (size_t)x->dim * sizeof(float));
            memcpy(x->h_keep_tab + staged.size() * x->keep_tab_stride, r.keep, words * sizeof(uint32_t));
            slot[staged.size()] = (uint8_t)staged.size();
            staged.push_back(&r);
        }
        if (staged.empty()) continue;
        HIP_TRY(x, hipMemcpyAsync(x->d_keep_tab, x->h_keep_tab, ((staged.size() - 1u) * x->keep_tab_stride + words) * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, x->stream));
        if ((rc = answer_block(x, staged, slot, k, nullptr, mode, threshold, /*gemv_only=*/true)) != CQS_HIP_OK) return rc;
    }
    return CQS_HIP_OK;
}

// plan_search under the handle's mutex: true = there is device work, else *rc is the call's answer.
bool search_planned(cqs_hip_index* x, const cqs_search::Args& a, int32_t* rc) {
    const char* why = "";
    const cqs_search::Plan plan = cqs_search::plan_search(a, x->n, x->dim, kMaxK, &why);
    *rc = plan == cqs_search::Plan::Invalid ? fail(x, CQS_HIP_ERR_INVALID, why) : CQS_HIP_OK;
    if (plan == cqs_search::Plan::Empty && why[0]) x->last_error = why;   // (the dimension mismatch: an answer with a message, no failure)
    return plan == cqs_search::Plan::Run;
}

// One request per query of a planned call: its own output rows and, filtered, its own bitset.
std::vector<cqs_combine_req> requests(const cqs_search::Args& a, float thr) {
    std::vector<cqs_combine_req> rq(a.b);
    for (uint32_t i = 0; i < a.b; ++i) {
        rq[i] = cqs_combine_req{a.queries + (size_t)i * a.query_dim, a.k, a.mode, thr, a.out_rows + (size_t)i * a.k,
                                a.out_scores + (size_t)i * a.k, a.out_counts + i};
        if (a.filtered) rq[i].keep = a.keep_bitsets + (size_t)i * a.keep_stride_words;
    }
    return rq;
}

}  // namespace cqs_idx

extern "C" {

int32_t cqs_hip_index_search(cqs_hip_index* x, const float* queries, uint32_t b, uint32_t query_dim, uint32_t k,
                             const uint32_t* keep_bitset, uint32_t mode, float threshold, uint64_t* out_rows,
                             float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_search");
    if (!x) return CQS_HIP_ERR_INVALID;
    // One query, arguments in order: the combining queue (dim is immutable; everything else the locked
    // path would check is checked here or inside the pass).  Round 5: a row-sharded parent takes it too - what a
    // multi-GPU daemon binds - its block runs through every shard and the host merge (cqs_sharded::search_combined).
    if (x->combine && b == 1 && (!keep_bitset || (x->combine_filtered && !x->sh)) && queries && out_counts && out_rows && out_scores && query_dim == x->dim &&
        k >= 1 && k <= kMaxK && mode <= CQS_HIP_MODE_PIPELINE) {
        if (x->sh ? cqs_sharded::poisoned(x) != 0 : x->poisoned.load(std::memory_order_acquire))
            return CQS_HIP_ERR_POISONED;                                               // src/cagra.rs:486-490
        out_counts[0] = 0;
        if (!cqs_search::query_finite(queries, query_dim)) return CQS_HIP_OK;                     // src/cagra.rs:464-470
        cqs_combine_req r{queries, k, mode, threshold, out_rows, out_scores, out_counts};
        r.keep = keep_bitset;
        return combine_search(x, r);
    }
    if (x->sh) return cqs_sharded::search(x, queries, b, query_dim, k, keep_bitset, mode, threshold, out_rows, out_scores, out_counts);
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;  // src/cagra.rs:486-490
    const cqs_search::Args a{queries, b, query_dim, k, mode, out_rows, out_scores, out_counts};
    int32_t rc;
    if (!search_planned(x, a, &rc)) return rc;
    const std::vector<cqs_combine_req> rq = requests(a, threshold);
    return search_host_locked(x, rq.data(), b, k, keep_bitset, mode, threshold, /*gemv_only=*/false);
} CQS_ABI_CATCH(x)

// Combining-queue counters since the handle was made: passes run by the queue and the queries they carried (bench /
// tests; not in the Rust trait).  Either pointer may be NULL.
void cqs_hip_index_combine_stats(const cqs_hip_index* x, uint64_t* passes, uint64_t* queries) CQS_ABI_TRY {
    if (passes) *passes = x ? x->stat_passes.load(std::memory_order_relaxed) : 0;
    if (queries) *queries = x ? x->stat_queries.load(std::memory_order_relaxed) : 0;
} CQS_ABI_CATCH_VOID

// The same counters for the blocks of callers with a bitset (and nothing else: cqs_hip_index_search_filtered does not count).
void cqs_hip_index_combine_filter_stats(const cqs_hip_index* x, uint64_t* passes, uint64_t* queries) CQS_ABI_TRY {
    if (passes) *passes = x ? x->stat_fpasses.load(std::memory_order_relaxed) : 0;
    if (queries) *queries = x ? x->stat_fqueries.load(std::memory_order_relaxed) : 0;
} CQS_ABI_CATCH_VOID

// The same counters for the blocks of callers with a tag filter (cqs_hip_index_search_tagged_multi does not count).
void cqs_hip_index_combine_tagged_stats(const cqs_hip_index* x, uint64_t* passes, uint64_t* queries) CQS_ABI_TRY {
    if (passes) *passes = x ? x->stat_tpasses.load(std::memory_order_relaxed) : 0;
    if (queries) *queries = x ? x->stat_tqueries.load(std::memory_order_relaxed) : 0;
} CQS_ABI_CATCH_VOID

// `b` queries, each with its own keep-bitset: per query the bytes of cqs_hip_index_search(…, 1, …, that bitset, …).
int32_t cqs_hip_index_search_filtered(cqs_hip_index* x, const float* queries, uint32_t b, uint32_t query_dim, uint32_t k,
                                      const uint32_t* keep_bitsets, uint64_t keep_stride_words, uint32_t mode,
                                      float threshold, uint64_t* out_rows, float* out_scores, uint32_t* out_counts) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_search_filtered");
    if (!x) return CQS_HIP_ERR_INVALID;
    if (x->sh) {   // a row-sharded parent: correct, not combined - one by one through its filtered search (own early checks)
        if (b == 0) return CQS_HIP_OK;
        if (!queries || !out_counts || !keep_bitsets) return CQS_HIP_ERR_INVALID;
        for (uint32_t i = 0; i < b; ++i) out_counts[i] = 0;
        if (query_dim != x->dim) return CQS_HIP_OK;
        if (keep_stride_words < (cqs_sharded::len(x) + 31) / 32) return CQS_HIP_ERR_INVALID;
        for (uint32_t i = 0; i < b; ++i) {
            const int32_t rc = cqs_sharded::search(x, queries + (size_t)i * x->dim, 1, query_dim, k, keep_bitsets + (size_t)i * keep_stride_words,
                                                   mode, threshold, out_rows ? out_rows + (size_t)i * k : nullptr,
                                                   out_scores ? out_scores + (size_t)i * k : nullptr, out_counts + i);
            if (rc != CQS_HIP_OK) return rc;
        }
        return CQS_HIP_OK;
    }
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;  // src/cagra.rs:486-490
    const cqs_search::Args a{queries, b, query_dim, k, mode, out_rows, out_scores, out_counts, true, keep_bitsets, keep_stride_words};
    int32_t rc;
    if (!search_planned(x, a, &rc)) return rc;
    const std::vector<cqs_combine_req> rq = requests(a, threshold);
    return search_filtered_locked(x, rq.data(), b, k, mode, threshold);
} CQS_ABI_CATCH(x)

// `find_neighbors` (src/cli/commands/search/neighbors.rs:86-132) for a row of this index: the query is the
// target row where it already lies in HBM (no H2D), the scan asks for limit + 1 and the target itself is
// dropped from the answer: top-(limit+1) of all rows minus the target = top-limit of all rows but the target
// under the same total order (score desc, row asc; neighbors.rs:131), duplicates of the target included.
int32_t cqs_hip_index_neighbors(cqs_hip_index* x, uint64_t target_row, uint32_t limit, uint64_t* out_rows,
                                float* out_scores, uint32_t* out_count) CQS_ABI_TRY {
    CQS_ROCTX_RANGE("cqs_hip_index_neighbors");
    if (!x || !out_count) return CQS_HIP_ERR_INVALID;
    if (x->sh) return cqs_sharded::neighbors(x, target_row, limit, out_rows, out_scores, out_count);
    std::lock_guard<std::mutex> g(x->mu);
    *out_count = 0;
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    if (!out_rows || !out_scores) return fail(x, CQS_HIP_ERR_INVALID, "neighbors: null output buffer");
    if (target_row < x->row_base || target_row - x->row_base >= x->n)
        return fail(x, CQS_HIP_ERR_INVALID, "neighbors: target row not in this index");   // get_chunk_with_embedding fails, :98-106
    const uint32_t k = cqs_search::neighbors_k(&limit, x->n);   // limit clamped; <= CQS_HIP_NEIGHBORS_MAX + 1
    if (k == 0) return CQS_HIP_OK;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, order_after_last(x, x->stream));
    int32_t rc = ensure_scratch(x, 1, k);
    if (rc != CQS_HIP_OK) return rc;
    const float* d_target = x->d_rows + (size_t)(target_row - x->row_base) * x->dim;
    rc = enqueue_search(x, d_target, 1, k, nullptr, CQS_HIP_MODE_RAW, 0.f, x->d_out_keys, x->d_out_counts, x->stream);
    if (rc != CQS_HIP_OK) return rc;
    HIP_TRY(x, hipMemcpyAsync(x->h_out_keys, x->d_out_keys, (size_t)k * sizeof(uint64_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipMemcpyAsync(x->h_out_counts, x->d_out_counts, sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    const uint32_t c = x->h_out_counts[0] < k ? x->h_out_counts[0] : k;
    uint64_t rows[CQS_HIP_NEIGHBORS_MAX + 1];
    float scores[CQS_HIP_NEIGHBORS_MAX + 1];
    cqs_search::unpack_keys(x->h_out_keys, c, rows, scores);
    *out_count = cqs_search::drop_self(rows, scores, c, target_row, limit, out_rows, out_scores);
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

void cqs_hip_index_set_timing(cqs_hip_index* x, int32_t enable) CQS_ABI_TRY {
    if (!x) return;
    if (x->sh) { cqs_sharded::set_timing(x, enable); return; }
    std::lock_guard<std::mutex> g(x->mu);
    x->timing = enable != 0;
    x->ev_used = 0;
} CQS_ABI_CATCH_VOID

int32_t cqs_hip_index_scan_time(cqs_hip_index* x, uint32_t* launches, double* total_ms) CQS_ABI_TRY {
    if (!x || !launches || !total_ms) return CQS_HIP_ERR_INVALID;
    if (x->sh) return cqs_sharded::scan_time(x, launches, total_ms);
    std::lock_guard<std::mutex> g(x->mu);
    *launches = 0;
    *total_ms = 0.0;
    HIP_TRY(x, hipSetDevice(x->device));
    for (size_t i = 0; i + 1 < x->ev_used; i += 2) {
        HIP_TRY(x, hipEventSynchronize(x->ev[i + 1]));
        float ms = 0.f;
        HIP_TRY(x, hipEventElapsedTime(&ms, x->ev[i], x->ev[i + 1]));
        *total_ms += ms;
        *launches += 1;
    }
    x->ev_used = 0;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

}  // extern "C"
