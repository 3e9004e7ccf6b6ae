// index_shadow.hip — host side of the dense index's shadow: the bf16 copy and the optional int8 copy beside it (scan_bf16.h,
// scan_i8.h), behind one handle pointer.
#include <cstdlib>
#include <cstring>
#include <new>

#include "abi_guard.h"
#include "index_internal.h"
#include "scan_bf16.h"
#include "scan_fallback.h"
#include "i8_sweep.h"
#include "scan_i8.h"
#include "tail_plan.h"

namespace cqs_idx {

// bf16 shadow built automatically at create / load (CQS_HIP_SCAN_BF16 unset) from this f32 corpus size on: 4x the 256 MB
// Infinity Cache, where the f32 scan streams from HBM alone and half the bytes is close to half the time
constexpr uint64_t kShadowAutoBytes = 1ull << 30;
// ... and only if, once it is allocated, the device still has max(this, kShadowFreeFrac of its memory) free
constexpr uint64_t kShadowFreeMinBytes = 4ull << 30;
constexpr double kShadowFreeFrac = 0.10;
// Device counters behind the maxima of the two build passes: [3, 5) certified / fallback queries of the device-API
// searches, whichever copy served them; [8, 10) those of them the int8 copy served; [10, 12) queries of any search whose
// finisher certified on a prefix of the candidates / whose prefix failed (cqs_hip_debug_tail_verdicts).
constexpr uint32_t kStatWords = 12, kStatCounts = 3, kStatI8 = 5, kStatI8Counts = 8, kStatPrefix = 10;

// Built at create / load where it pays, CQS_HIP_SCAN_BF16, or cqs_hip_index_set_bf16_scan: searches of gemv blocks scan it
// first, rescore the candidates from the f32 rows and fall back to the f32 scan for any query the certificate does not
// cover (scan_bf16.h): host searches from the host, device-API searches through the gated f32 launches.  On a borrowed
// handle it is a snapshot of the caller's rows taken at create.
struct Shadow {
    uint16_t* d_bf16 = nullptr;           // [cap, dim] bf16
    uint64_t cap = 0;                     // rows the buffers hold (follows cap_rows)
    int8_t* d_i8 = nullptr;               // [cap, dim] int8 codes of the optional second copy (null: bf16 alone), which
    float* d_i8_scale = nullptr;          // [cap] searches of <= kI8MaxQ queries at an i8_k_ok k scan instead of the bf16 one
    double r8 = 0.0, norm8 = 0.0;         // r / norm of the int8 copy
    double r = 0.0;                       // max over the finite rows of ||x - x~|| + gamma (||x|| + ||x~||)
    double norm = 0.0;                    // max over the finite rows of max(||x||, ||x~||)
    unsigned long long* d_stats = nullptr;   // [kStatWords] the build pass's maxima (f64 bits) and outlier flag, the
                                             // device-API searches' certified / fallback counts (certify adds), then the
                                             // same five words of the int8 copy
    uint64_t* d_ekeys = nullptr;          // [kShadowMaxQ, kMaxK - 1] rescored keys
    uint32_t* d_cert = nullptr;           // [kShadowMaxQ] certified flags (device-API searches: the f32 gate; host searches:
                                          // when h_cert is not mappable)
    float* d_bq = nullptr;                // [kShadowMaxQ] B_q of each query of the block (the fused tail kernel; PIPELINE
                                          // searches: launch_shadow_bound / launch_i8_bound, ahead of the scan that reads it)
    uint32_t* d_tickets = nullptr;        // [kShadowMaxQ] arrival counts of the tail kernel's workgroups: zeroed here once,
                                          // put back to zero by every launch (launch_rescore_certify)
    uint64_t* d_fb_lists = nullptr;       // [kMaxGemvQ, n_cu, kFallbackMaxK] the one-launch f32 fallback's hand-off scratch
    uint32_t* d_fb_tickets = nullptr;     // [kMaxGemvQ] ... and its arrival counts: zeroed here once, put back to zero by every
                                          // launch (scan_fallback.h)
    bool fb_one_launch = true;            // CQS_HIP_FALLBACK_ONE_LAUNCH, read when the shadow is built: 0 = the device-API searches'
                                          // f32 fallback is always the gated scan + select pair
    bool tail_prefix = true;              // CQS_HIP_TAIL_PREFIX, read when the shadow is built: 0 = the tail kernel's finisher always
                                          // sorts every candidate at once (the A/B arm and the tests' reference; same answers)
    uint8_t tail_first = 2;               // CQS_HIP_TAIL_PREFIX_FIRST, read when the shadow is built: 0 = every tail workgroup selects and the
                                          // query's waves rescore all k' candidates (the A/B arm and the tests' reference); 1 = the prefix
                                          // first wherever a proper one exists; unset = where that pays (tail_prefix_first_default).  Same answers
    uint8_t i8_groups = 2;                // CQS_HIP_I8_GROUPS, read when the shadow is built: 0 = the int8 scan publishes one maximum per
                                          // task, as the other scans do (the A/B arm and the tests' reference); 1 = one per workgroup of
                                          // four tasks in every int8 block; unset = where that pays (shadow_group_tasks).  Same answers
    bool i8_serpentine = true;            // CQS_HIP_I8_SERPENTINE, read when the shadow is built: 0 = every int8 scan sweeps the copy forwards
                                          // and a streamed one loads nontemporally throughout (the A/B arm and the tests' reference;
                                          // same answers); w:<bytes> = on, with that plain-load window at any corpus size (tests)
    bool i8_force_window = false;         // (the w:<bytes> form: the int8 scan takes its nontemporal instantiation at any size)
    uint64_t i8_plain_bytes = cqs::kI8PlainBytes;   // bytes at each end of a streamed int8 copy that are loaded plainly (i8_sweep.h)
    uint32_t sweep_rev = 0;               // parity of the next int8 scan's sweep: flipped by shadow_pass after each one it
                                          // enqueues (host state, under the lock that serialises enqueues); extend, remove
                                          // and update put it back to 0 (shadow_sweep_reset)
    uint32_t* h_cert = nullptr;           // pinned [kShadowMaxQ]
    uint32_t* h_cert_dev = nullptr;       // its device-visible address (null: not mappable)
};

// Add what the device-API searches' certify launches counted (d_stats + first, two words) to *certified / *fallbacks,
// once every search has completed (quiesce).  Caller holds mu.
static void shadow_device_counts(cqs_hip_index* x, uint32_t first, uint64_t* certified, uint64_t* fallbacks) {
    unsigned long long c[2];
    if (!x->shadow || !x->shadow->d_stats || quiesce(x) != hipSuccess) return;
    hipError_t e = hipMemcpyAsync(c, x->shadow->d_stats + first, sizeof c, hipMemcpyDeviceToHost, x->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); return; }
    *certified += c[0];
    *fallbacks += c[1];
}

// Free the int8 copy alone; the bf16 copy then serves every block.  Its device counts stay in d_stats.
static void i8_free(Shadow* s) {
    hipFree(s->d_i8); hipFree(s->d_i8_scale);
    s->d_i8 = nullptr; s->d_i8_scale = nullptr;
}

void shadow_free(cqs_hip_index* x) {
    Shadow* s = x->shadow;
    if (!s) return;
    uint64_t c = 0, f = 0;   // the counts outlive the shadow
    shadow_device_counts(x, kStatCounts, &c, &f);
    x->stat_certified.fetch_add(c, std::memory_order_relaxed);
    x->stat_fallbacks.fetch_add(f, std::memory_order_relaxed);
    c = f = 0;
    shadow_device_counts(x, kStatI8Counts, &c, &f);
    x->stat_i8_certified.fetch_add(c, std::memory_order_relaxed);
    x->stat_i8_fallbacks.fetch_add(f, std::memory_order_relaxed);
    i8_free(s);
    hipFree(s->d_bf16); hipFree(s->d_stats); hipFree(s->d_ekeys);
    hipFree(s->d_cert); hipFree(s->d_bq); hipFree(s->d_tickets); hipFree(s->d_fb_lists); hipFree(s->d_fb_tickets);
    hipHostFree(s->h_cert);
    delete s;
    x->shadow = nullptr;
}

// The rows have changed (extend, remove, update): the next int8 scan sweeps forwards again.
void shadow_sweep_reset(cqs_hip_index* x) {
    if (x->shadow) x->shadow->sweep_rev = 0u;
}

ShadowBuffers shadow_buffers(const cqs_hip_index* x) {
    const Shadow* s = x->shadow;
    return s ? ShadowBuffers{s->d_bf16, s->d_i8, s->d_i8_scale} : ShadowBuffers{nullptr, nullptr, nullptr};
}

// Convert rows [row0, x->n) into the shadow and fold them into R.  Caller holds mu, the stream is idle.  *outlier: a finite
// row has a component of magnitude >= 2^64 (the shadow cannot certify against it).
static int32_t shadow_convert(cqs_hip_index* x, uint64_t row0, bool* outlier) {
    Shadow* s = x->shadow;
    HIP_TRY(x, hipMemsetAsync(s->d_stats + 2, 0, sizeof(unsigned long long), x->stream));
    HIP_TRY(x, cqs::launch_shadow_build(x->d_rows, s->d_bf16, row0, x->n - row0, x->dim, cqs::shadow_gamma(x->dim),
                                        s->d_stats, x->stream));
    unsigned long long st[3];
    HIP_TRY(x, hipMemcpyAsync(st, s->d_stats, sizeof st, hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    double r, m;
    memcpy(&r, &st[0], sizeof r);
    memcpy(&m, &st[1], sizeof m);
    s->r = r * (1.0 + 0x1p-30);      // (f64 sums of <= 2048 squares and three square roots: relative error < 2^-40)
    s->norm = m * (1.0 + 0x1p-30);
    *outlier = st[2] != 0;
    return CQS_HIP_OK;
}

// The same for the int8 copy (codes, scales, r8 / norm8); the outlier flag is shadow_convert's.
static int32_t i8_convert(cqs_hip_index* x, uint64_t row0) {
    Shadow* s = x->shadow;
    HIP_TRY(x, cqs::launch_i8_build(x->d_rows, s->d_i8, s->d_i8_scale, row0, x->n - row0, x->dim, cqs::i8_gamma(x->dim),
                                    s->d_stats + kStatI8, x->stream));
    unsigned long long st[2];
    HIP_TRY(x, hipMemcpyAsync(st, s->d_stats + kStatI8, sizeof st, hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    double r, m;
    memcpy(&r, &st[0], sizeof r);
    memcpy(&m, &st[1], sizeof m);
    s->r8 = r * (1.0 + 0x1p-30);
    s->norm8 = m * (1.0 + 0x1p-30);
    return CQS_HIP_OK;
}

int32_t shadow_update_begin(cqs_hip_index* x, unsigned long long** stats, unsigned long long** stats8) {
    Shadow* s = x->shadow;
    shadow_sweep_reset(x);
    HIP_TRY(x, hipMemsetAsync(s->d_stats + 2, 0, sizeof(unsigned long long), x->stream));
    *stats = s->d_stats;
    *stats8 = s->d_stats + kStatI8;
    return CQS_HIP_OK;
}

// d_stats[0..2] and [kStatI8, +2) hold the maxima over every row ever converted (the build passes never clear them), the
// rewritten rows' old contents among them: a superset of the rows now stored, so r / norm stay valid and at worst looser.
int32_t shadow_update_end(cqs_hip_index* x) {
    Shadow* s = x->shadow;
    unsigned long long st[kStatI8 + 2];
    HIP_TRY(x, hipMemcpyAsync(st, s->d_stats, sizeof st, hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    if (st[2] != 0) {
        shadow_free(x);
        x->last_error = "update: a new row has a component of magnitude >= 2^64; bf16 shadow turned off";
        return CQS_HIP_OK;
    }
    double v[4];
    memcpy(&v[0], &st[0], sizeof(double));
    memcpy(&v[1], &st[1], sizeof(double));
    memcpy(&v[2], &st[kStatI8], sizeof(double));
    memcpy(&v[3], &st[kStatI8 + 1], sizeof(double));
    s->r = v[0] * (1.0 + 0x1p-30);   // (the slack of shadow_convert / i8_convert)
    s->norm = v[1] * (1.0 + 0x1p-30);
    if (s->d_i8) {
        s->r8 = v[2] * (1.0 + 0x1p-30);
        s->norm8 = v[3] * (1.0 + 0x1p-30);
    }
    return CQS_HIP_OK;
}

static uint64_t i8_bytes(uint64_t cap, uint32_t dim) { return cap * dim + cap * sizeof(float); }

// Allocate and build the int8 copy over rows [0, n) beside a bf16 copy that is in place.  *built = false: no memory (freed again).
static int32_t i8_enable(cqs_hip_index* x, bool* built) {
    Shadow* s = x->shadow;
    *built = false;
    if (hipMalloc(&s->d_i8, (size_t)s->cap * x->dim) != hipSuccess ||
        hipMalloc(&s->d_i8_scale, (size_t)s->cap * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        i8_free(s);
        return CQS_HIP_OK;
    }
    const int32_t rc = i8_convert(x, 0);
    if (rc != CQS_HIP_OK) { i8_free(s); return rc; }
    *built = true;
    return CQS_HIP_OK;
}

// extend() on a handle with the shadow on: grow it with cap_rows, convert rows [n_old, n).  A failure here (no memory,
// an outlier row) turns the shadow off and leaves the f32 index as extended: the call still succeeds.
int32_t shadow_extend(cqs_hip_index* x, uint64_t n_old) {
    Shadow* s = x->shadow;
    if (!s) return CQS_HIP_OK;
    shadow_sweep_reset(x);
    if (x->cap_rows > s->cap) {
        uint16_t* nd = nullptr;
        if (hipMalloc(&nd, (size_t)x->cap_rows * x->dim * sizeof(uint16_t)) != hipSuccess) {
            (void)hipGetLastError();
            shadow_free(x);
            x->last_error = "extend: no device memory to grow the bf16 shadow; shadow turned off";
            return CQS_HIP_OK;
        }
        hipError_t e = hipMemcpyAsync(nd, s->d_bf16, (size_t)n_old * x->dim * sizeof(uint16_t), hipMemcpyDeviceToDevice, x->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
        if (e != hipSuccess) { hipFree(nd); return fail(x, CQS_HIP_ERR_DEVICE, "extend: shadow copy", e); }
        hipFree(s->d_bf16);
        s->d_bf16 = nd;
        if (s->d_i8) {   // the int8 copy grows with it, or goes (the bf16 copy then serves every block)
            int8_t* n8 = nullptr;
            float* ns = nullptr;
            if (hipMalloc(&n8, (size_t)x->cap_rows * x->dim) != hipSuccess || hipMalloc(&ns, (size_t)x->cap_rows * sizeof(float)) != hipSuccess) {
                (void)hipGetLastError();
                hipFree(n8);
                i8_free(s);
                x->last_error = "extend: no device memory to grow the int8 copy of the shadow; int8 copy turned off";
            } else {
                e = hipMemcpyAsync(n8, s->d_i8, (size_t)n_old * x->dim, hipMemcpyDeviceToDevice, x->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(ns, s->d_i8_scale, (size_t)n_old * sizeof(float), hipMemcpyDeviceToDevice, x->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
                if (e != hipSuccess) { hipFree(n8); hipFree(ns); return fail(x, CQS_HIP_ERR_DEVICE, "extend: int8 copy", e); }
                i8_free(s);
                s->d_i8 = n8;
                s->d_i8_scale = ns;
            }
        }
        s->cap = x->cap_rows;
    }
    bool outlier = false;
    int32_t rc = shadow_convert(x, n_old, &outlier);
    if (rc == CQS_HIP_OK && s->d_i8 && !outlier) rc = i8_convert(x, n_old);
    if (rc != CQS_HIP_OK) return rc;
    if (outlier) {
        shadow_free(x);
        x->last_error = "extend: a new row has a component of magnitude >= 2^64; bf16 shadow turned off";
    }
    return CQS_HIP_OK;
}

// The shadow's dim rule (16-byte loads of 8 components, up to kShadowMaxDim) and how last_error states it.
static bool dim_ok(uint32_t dim) { return dim % 8u == 0u && dim <= cqs::kShadowMaxDim; }
static const char* const kDimRule = ": dim must be a multiple of 8 and <= 2048";

// Allocate and build the shadow over rows [0, n) (no borrow check: the create policy snapshots borrowed rows too).  On
// failure the shadow is freed and `fail` has put `what: reason` in last_error.  Caller holds mu (or owns the new handle).
static int32_t shadow_enable(cqs_hip_index* x, const char* what) {
    std::string pre(what);
    if (!dim_ok(x->dim)) return fail(x, CQS_HIP_ERR_INVALID, (pre + kDimRule).c_str());
    if (x->shadow) return CQS_HIP_OK;
    auto oom = [&](hipError_t e) { (void)hipGetLastError(); shadow_free(x); return fail(x, CQS_HIP_ERR_NOMEM, (pre + ": allocation").c_str(), e); };
    Shadow* s = x->shadow = new (std::nothrow) Shadow();
    if (!s) return oom(hipErrorOutOfMemory);
    const uint64_t cap = x->cap_rows ? x->cap_rows : 1;
    hipError_t e;
    if ((e = hipMalloc(&s->d_bf16, (size_t)cap * x->dim * sizeof(uint16_t))) != hipSuccess) return oom(e);
    s->cap = cap;
    unsigned long long* stats = nullptr;   // zeroed before it is the shadow's: shadow_free reads its counts
    if ((e = hipMalloc(&stats, kStatWords * sizeof(unsigned long long))) != hipSuccess) return oom(e);
    if ((e = hipMemsetAsync(stats, 0, kStatWords * sizeof(unsigned long long), x->stream)) != hipSuccess) { hipFree(stats); return oom(e); }
    s->d_stats = stats;
    if ((e = hipMalloc(&s->d_ekeys, (size_t)cqs::kShadowMaxQ * (cqs::kMaxK - 1) * sizeof(uint64_t))) != hipSuccess) return oom(e);
    if ((e = hipMalloc(&s->d_cert, (size_t)cqs::kShadowMaxQ * sizeof(uint32_t))) != hipSuccess) return oom(e);
    if ((e = hipMalloc(&s->d_bq, (size_t)cqs::kShadowMaxQ * sizeof(float))) != hipSuccess) return oom(e);
    if ((e = hipMalloc(&s->d_tickets, (size_t)cqs::kShadowMaxQ * sizeof(uint32_t))) != hipSuccess) return oom(e);
    if ((e = hipMemsetAsync(s->d_tickets, 0, (size_t)cqs::kShadowMaxQ * sizeof(uint32_t), x->stream)) != hipSuccess) return oom(e);
    const char* fb_env = getenv("CQS_HIP_FALLBACK_ONE_LAUNCH");
    s->fb_one_launch = !(fb_env && fb_env[0] == '0');
    const char* tp_env = getenv("CQS_HIP_TAIL_PREFIX");
    s->tail_prefix = !(tp_env && tp_env[0] == '0');
    const char* tf_env = getenv("CQS_HIP_TAIL_PREFIX_FIRST");
    s->tail_first = tf_env && tf_env[0] == '0' ? 0 : (tf_env && tf_env[0] == '1' ? 1 : 2);
    const char* ig_env = getenv("CQS_HIP_I8_GROUPS");
    s->i8_groups = ig_env && ig_env[0] == '0' ? 0 : (ig_env && ig_env[0] == '1' ? 1 : 2);
    const char* sp_env = getenv("CQS_HIP_I8_SERPENTINE");
    s->i8_serpentine = !(sp_env && sp_env[0] == '0');
    if (sp_env && sp_env[0] == 'w' && sp_env[1] == ':') {
        s->i8_force_window = true;
        s->i8_plain_bytes = strtoull(sp_env + 2, nullptr, 10);
    }
    if ((e = hipMalloc(&s->d_fb_lists, cqs::f32_topk_fallback_words(x->n_cu) * sizeof(uint64_t))) != hipSuccess) return oom(e);
    if ((e = hipMalloc(&s->d_fb_tickets, (size_t)cqs::kMaxGemvQ * sizeof(uint32_t))) != hipSuccess) return oom(e);
    if ((e = hipMemsetAsync(s->d_fb_tickets, 0, (size_t)cqs::kMaxGemvQ * sizeof(uint32_t), x->stream)) != hipSuccess) return oom(e);
    if ((e = hipHostMalloc(&s->h_cert, (size_t)cqs::kShadowMaxQ * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess) return oom(e);
    if (hipHostGetDevicePointer((void**)&s->h_cert_dev, s->h_cert, 0) != hipSuccess) {
        (void)hipGetLastError();
        s->h_cert_dev = nullptr;
    }
    bool outlier = false;
    const int32_t rc = shadow_convert(x, 0, &outlier);
    if (rc != CQS_HIP_OK) { shadow_free(x); return rc; }
    if (outlier) {
        shadow_free(x);
        return fail(x, CQS_HIP_ERR_INVALID, (pre + ": a finite row has a component of magnitude >= 2^64").c_str());
    }
    return CQS_HIP_OK;
}

// The int8 copy's policy, once the bf16 copy is built (create / load policy and set_bf16_scan alike).  CQS_HIP_SCAN_I8, read
// here: unset = where it pays (f32 corpus >= kShadowAutoBytes), 0 = never, 1 = beside every bf16 copy; its own dim rule
// and the free-memory rule over both copies either way.  Never fails for the copy's sake: the bf16 copy then serves
// every block and last_error says why.  Returns an error only for a device fault.
static bool i8_dim_ok(uint32_t dim) { return cqs::i8_dim_ok(dim); }
static const char* const kI8DimRule = ": dim must be a multiple of 16 and <= 2048";
static int32_t i8_auto(cqs_hip_index* x) {
    Shadow* s = x->shadow;
    if (!s || s->d_i8) return CQS_HIP_OK;
    const char* env = getenv("CQS_HIP_SCAN_I8");
    if (env && env[0] == '0') return CQS_HIP_OK;
    if (!(env && env[0] == '1') && x->n * x->dim * sizeof(float) < kShadowAutoBytes) return CQS_HIP_OK;
    const std::string pre("int8 copy of the shadow not built (the bf16 copy serves every block)");
    if (!i8_dim_ok(x->dim)) { x->last_error = pre + kI8DimRule; return CQS_HIP_OK; }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        x->last_error = pre + ": hipMemGetInfo failed";
        return CQS_HIP_OK;
    }
    const uint64_t need = i8_bytes(s->cap, x->dim);
    const uint64_t frac = (uint64_t)(kShadowFreeFrac * (double)total_b);
    const uint64_t reserve = frac > kShadowFreeMinBytes ? frac : kShadowFreeMinBytes;
    bool built = false;
    if (free_b >= need && free_b - need >= reserve) {
        const int32_t rc = i8_enable(x, &built);
        if (rc != CQS_HIP_OK) return rc;
    }
    if (!built) x->last_error = pre + ": the device would keep less than max(4 GiB, 10 %) of its memory free with both copies";
    return CQS_HIP_OK;
}

// The shadow policy of create / create_device / load, for a single-device handle whose rows are in place.
// CQS_HIP_SCAN_BF16 (read here, at create): unset = where it pays (f32 corpus >= kShadowAutoBytes), 0 = never, 1 = at any
// size; dim, outlier and free-memory rules either way.  The create never fails for the shadow's sake: the handle then
// searches the f32 rows and last_error says why.  Returns an error only for a device fault (the handle is poisoned).
int32_t shadow_auto(cqs_hip_index* x) {
    const char* env = getenv("CQS_HIP_SCAN_BF16");
    if (env && env[0] == '0') return CQS_HIP_OK;
    const bool any_size = env && env[0] == '1';
    const uint64_t f32_bytes = x->n * x->dim * sizeof(float);
    if (!any_size && f32_bytes < kShadowAutoBytes) {
        x->last_error = "bf16 shadow not built: f32 corpus below 1 GiB (CQS_HIP_SCAN_BF16=1 builds it at any size)";
        return CQS_HIP_OK;
    }
    if (!dim_ok(x->dim)) {
        x->last_error = std::string("bf16 shadow not built") + kDimRule;
        return CQS_HIP_OK;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        x->last_error = "bf16 shadow not built: hipMemGetInfo failed";
        return CQS_HIP_OK;
    }
    const uint64_t cap = x->cap_rows ? x->cap_rows : 1;
    const uint64_t need = cap * x->dim * sizeof(uint16_t) + (cqs::kMaxK + 2ull) * cqs::kShadowMaxQ * sizeof(uint64_t) +
                          cqs::f32_topk_fallback_words(x->n_cu) * sizeof(uint64_t);
    const uint64_t frac = (uint64_t)(kShadowFreeFrac * (double)total_b);
    const uint64_t reserve = frac > kShadowFreeMinBytes ? frac : kShadowFreeMinBytes;
    if (free_b < need || free_b - need < reserve) {
        x->last_error = "bf16 shadow not built: the device would keep less than max(4 GiB, 10 %) of its memory free";
        return CQS_HIP_OK;
    }
    int32_t rc = shadow_enable(x, "bf16 shadow not built");
    if (rc == CQS_HIP_OK) rc = i8_auto(x);   // (free memory is read again: the bf16 copy is counted)
    return rc == CQS_HIP_ERR_DEVICE ? rc : CQS_HIP_OK;
}

// Blocks that run as gemv passes (the matrix-core blocks' scores are not the gemv kernel's) of up to kShadowMaxQ queries,
// at a k the shadow can certify (k' < k only at k = kMaxK).
bool shadow_takes(const cqs_hip_index* x, uint32_t b, uint32_t k, bool gemv_only) {
    return x->shadow && b <= cqs::kShadowMaxQ && (gemv_only || !cqs::use_mfma(b, x->dim)) && cqs::shadow_kprime(k) >= k;
}

// Which copy serves a block the shadow takes, from (b, k) alone: the int8 one where it exists, for blocks of <= kI8MaxQ
// queries at a k whose k'_8 fits the select; else the bf16 one.
bool shadow_uses_i8(const cqs_hip_index* x, uint32_t b, uint32_t k) {
    return x->shadow && x->shadow->d_i8 && b <= cqs::kI8MaxQ && cqs::i8_k_ok(k);
}

// Tasks per entry of the shadow scan's gmax / gaux (ScanArgs::group_tasks): 4, the int8 scan's workgroup maxima, where they
// pay.  They take 4 us off the select's walk over the maxima whatever k' is, and cost a gather that grows with k'^2 / n: a
// listed group of up to 256 rows holds a second entry at or above the threshold bin four times as often as a task of 64, and
// then all four of its tasks are read, 128 to a round trip - about 4 * 255 * (k' + 1)^2 / n tasks.  Measured at 1M rows
// ("Workgroup maxima"): -2.4 to -2.9 us per search at k' + 1 = 351, +8 at 1021; the rule keeps the estimate
// under two round trips.
static uint32_t shadow_group_tasks(const cqs_hip_index* x, bool i8, uint32_t kp) {
    const Shadow* s = x->shadow;
    if (!i8 || s->i8_groups == 0) return 1u;
    if (s->i8_groups == 1) return cqs::kMaxGroupTasks;
    const uint64_t kk = (uint64_t)kp + 1u;
    return 4u * kk * kk <= pad_rows(x->n) ? cqs::kMaxGroupTasks : 1u;
}

// The sweep of the int8 scan about to be enqueued with `a`: it starts where the last one stopped (the parity flips here, once
// per scan), and the ends of a streamed copy load plainly.  Caller holds mu.
static void sweep_args(Shadow* s, cqs::ScanArgs& a) {
    if (!s->i8_serpentine) return;
    a.sweep_rev = s->sweep_rev;
    s->sweep_rev ^= 1u;
    a.plain_bytes = s->i8_plain_bytes;
    if (s->i8_force_window) a.nontemporal = true;
}

// The shadow half of a gemv block on `st`: shadow scan -> one tail launch (select k' + 1, B_q, rescore, certify) into
// out_keys / out_counts.  PIPELINE searches alone launch the bound kernel first: only their scan reads B_q (its drop rule).
// device_gate (device-API searches): `st` is ordered after the last search here, certify counts outcomes on the device,
// *device_gate = the verdicts that must gate the f32 launches next.  Null: host searches (shadow_verdicts).
// The tail kernel's last workgroup writes the verdicts, and its first the zeroed work-queue heads, before the kernel ends,
// and nothing is launched between it and the gated f32 scan (gate_closed).  Both callers record `done` after the pass,
// which orders the next search, on any stream, after every user of d_bq, d_ekeys, d_cert and d_tickets.
int32_t shadow_pass(cqs_hip_index* x, const float* d_q, uint32_t nb, uint32_t k, const uint32_t* d_keep, uint32_t mode,
                    float threshold, uint64_t* out_keys, uint32_t* out_counts, hipStream_t st, const uint32_t** device_gate,
                    const KeepTab* tab) {
    Shadow* s = x->shadow;
    uint32_t* const cert = device_gate || !s->h_cert_dev ? s->d_cert : s->h_cert_dev;
    if (device_gate) *device_gate = cert;
    if (device_gate) HIP_TRY(x, order_after_last(x, st));
    // The same chain over either copy: its bound, its scan, its k'.  A query the int8 copy does not certify goes to the f32
    // scan like any other, not through the bf16 copy.
    const bool i8 = shadow_uses_i8(x, nb, k);
    const uint32_t kp = i8 ? cqs::i8_kprime(k) : cqs::shadow_kprime(k);
    const double r_max = i8 ? s->r8 : s->r, norm_max = i8 ? s->norm8 : s->norm;
    const bool bound_first = mode == CQS_HIP_MODE_PIPELINE;
    if (bound_first) {
        if (i8) HIP_TRY(x, cqs::launch_i8_bound(d_q, nb, x->dim, r_max, norm_max, s->d_bq, st));
        else HIP_TRY(x, cqs::launch_shadow_bound(d_q, nb, x->dim, r_max, norm_max, s->d_bq, st));
    }
    // gemv passes over the copy's rows (non-uniform tiers, no debug stamps), top k' + 1; the select's (argmax, runner-up)
    // index from kGauxMinK on whatever CQS_HIP_SELECT_AUX says (that A/B hook is the f32 select's)
    cqs::ScanArgs a = scan_args(x, d_q, nb, kp + 1u, d_keep, mode, threshold, i8 ? sizeof(int8_t) : sizeof(uint16_t), true, nullptr, nullptr, tab);
    a.group_tasks = shadow_group_tasks(x, i8, kp);   // (the scan publishes, the tail kernel's select walks: one maximum per that many tasks)
    if (i8) sweep_args(s, a);
    const ShadowRows rows{i8 ? nullptr : s->d_bf16, i8 ? s->d_i8 : nullptr, s->d_i8_scale, s->d_bq};
    const int32_t rc = scan_select(x, a, st, &rows, nullptr, nullptr);   // (the scan alone: the tail kernel selects)
    if (rc == CQS_HIP_OK)
        HIP_TRY(x, cqs::launch_rescore_certify(a, (uint32_t)x->row_base, k, kp, bound_first ? 0u : (i8 ? 2u : 1u), r_max, norm_max,
                                               s->d_bq, s->d_tickets, s->d_ekeys, out_keys, out_counts, cert,
                                               device_gate ? s->d_stats + kStatCounts : nullptr,
                                               device_gate && i8 ? s->d_stats + kStatI8Counts : nullptr, s->tail_prefix,
                                               s->tail_first == 2 ? cqs::tail_prefix_first_default(pad_rows(x->n), k) : s->tail_first == 1,
                                               s->d_stats + kStatPrefix, x->d_dbg, st));
    return rc;
}

// The f32 fallback of a device-API search behind shadow_pass on the same stream, gated by its verdicts.  One launch where
// that form takes the block (scan_fallback.h: b <= 8, k <= kFallbackMaxK, no per-query table) and the handle's switch is on;
// else *taken = false and the caller enqueues the gated scan + select pair.  Nothing is launched between the tail kernel and
// this launch (gate_closed), and `done` is recorded after it: the next search, on any stream, is ordered after every user of
// the hand-off scratch and its tickets.
int32_t shadow_fallback(cqs_hip_index* x, const float* d_q, uint32_t nb, uint32_t k, const uint32_t* d_keep, uint32_t mode,
                        float threshold, uint64_t* out_keys, uint32_t* out_counts, hipStream_t st, const uint32_t* gate,
                        bool* taken) {
    const Shadow* s = x->shadow;
    *taken = false;
    if (!s || !gate || !s->fb_one_launch) return CQS_HIP_OK;
    const cqs::ScanArgs a = scan_args(x, d_q, nb, k, d_keep, mode, threshold, sizeof(float), false, nullptr, gate);
    if (!cqs::f32_topk_fallback_takes(a)) return CQS_HIP_OK;
    HIP_TRY(x, cqs::launch_f32_topk_fallback(a, (uint32_t)x->row_base, gate, s->d_fb_lists, s->d_fb_tickets, out_keys, out_counts, st));
    HIP_TRY(x, record_done(x, st));
    *taken = true;
    return CQS_HIP_OK;
}

hipError_t shadow_verdicts(cqs_hip_index* x, uint32_t nb, const uint32_t** h_cert) {
    const Shadow* s = x->shadow;
    *h_cert = s->h_cert;
    return s->h_cert_dev ? hipSuccess : hipMemcpyAsync(s->h_cert, s->d_cert, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream);
}

}  // namespace cqs_idx

using namespace cqs_idx;

extern "C" {

// bf16 shadow of the corpus for `VectorIndex::search` (src/index.rs:146; the reference's GPU backend keeps its f32
// dataset resident, src/cagra.rs:255-277): host searches that run as gemv passes scan n x dim x 2 B instead of x 4 and
// return the f32 scan's bytes (scan_bf16.h).  Owned single-device handles only.
int32_t cqs_hip_index_set_bf16_scan(cqs_hip_index* x, int32_t enable) CQS_ABI_TRY {
    if (!x || x->sh) return CQS_HIP_ERR_INVALID;   // (a row-sharded parent: out of scope, header)
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // a search enqueued on a caller stream may still read the shadow
    if (!enable) { shadow_free(x); return CQS_HIP_OK; }
    // a borrowed handle gets its shadow at create or not at all: enabling it later would snapshot rows the caller may have
    // changed since (test_invalid_handles); disabling above works on every handle
    if (x->borrow) return fail(x, CQS_HIP_ERR_INVALID, "set_bf16_scan: index borrows its rows (they may change under the bound)");
    const int32_t rc = shadow_enable(x, "set_bf16_scan");
    return rc == CQS_HIP_OK ? i8_auto(x) : rc;   // (the int8 copy: under CQS_HIP_SCAN_I8's rule, as at create)
} CQS_ABI_CATCH(x)

void cqs_hip_index_bf16_stats(const cqs_hip_index* x, uint64_t* bytes, uint64_t* certified, uint64_t* fallbacks) CQS_ABI_TRY {
    uint64_t by = 0, c = 0, f = 0;
    if (x && !x->sh) {
        cqs_hip_index* m = const_cast<cqs_hip_index*>(x);   // (waits for the device-API searches whose counts it reads)
        std::lock_guard<std::mutex> g(m->mu);
        by = m->shadow ? m->shadow->cap * m->dim * sizeof(uint16_t) : 0;
        c = m->stat_certified.load(std::memory_order_relaxed);
        f = m->stat_fallbacks.load(std::memory_order_relaxed);
        if (m->shadow && hipSetDevice(m->device) == hipSuccess) shadow_device_counts(m, kStatCounts, &c, &f);
    }
    if (bytes) *bytes = by;
    if (certified) *certified = c;
    if (fallbacks) *fallbacks = f;
} CQS_ABI_CATCH_VOID

void cqs_hip_index_i8_stats(const cqs_hip_index* x, uint64_t* bytes, uint64_t* certified, uint64_t* fallbacks) CQS_ABI_TRY {
    uint64_t by = 0, c = 0, f = 0;
    if (x && !x->sh) {
        cqs_hip_index* m = const_cast<cqs_hip_index*>(x);
        std::lock_guard<std::mutex> g(m->mu);
        by = m->shadow && m->shadow->d_i8 ? i8_bytes(m->shadow->cap, m->dim) : 0;
        c = m->stat_i8_certified.load(std::memory_order_relaxed);
        f = m->stat_i8_fallbacks.load(std::memory_order_relaxed);
        if (m->shadow && hipSetDevice(m->device) == hipSuccess) shadow_device_counts(m, kStatI8Counts, &c, &f);
    }
    if (bytes) *bytes = by;
    if (certified) *certified = c;
    if (fallbacks) *fallbacks = f;
} CQS_ABI_CATCH_VOID

// Test hook (not part of the public header): B_q of `b` host queries [b, dim] as the device computes it for a device-API
// search (launch_shadow_bound) and as the host function computes it from a plain f64 loop (shadow_query_bound), both
// against this handle's shadow.  INVALID without a shadow or for b > kShadowMaxQ.
int32_t cqs_hip_debug_shadow_bound(cqs_hip_index* x, const float* queries, uint32_t b, float* out_device, float* out_host) CQS_ABI_TRY {
    if (!x || x->sh || !queries || !out_device || !out_host || b == 0) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    const Shadow* s = x->shadow;
    if (!s || b > cqs::kShadowMaxQ) return CQS_HIP_ERR_INVALID;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // d_bq belongs to the searches
    float* d_q = nullptr;
    HIP_TRY(x, hipMalloc(&d_q, (size_t)b * x->dim * sizeof(float)));
    hipError_t e = hipMemcpyAsync(d_q, queries, (size_t)b * x->dim * sizeof(float), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess) e = cqs::launch_shadow_bound(d_q, b, x->dim, s->r, s->norm, s->d_bq, x->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_device, s->d_bq, (size_t)b * sizeof(float), hipMemcpyDeviceToHost, x->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
    hipFree(d_q);
    HIP_TRY(x, e);
    for (uint32_t i = 0; i < b; ++i) {
        const float* q = queries + (size_t)i * x->dim;
        double s2 = 0.0;
        for (uint32_t d = 0; d < x->dim; ++d) s2 += (double)q[d] * (double)q[d];
        out_host[i] = cqs::shadow_query_bound(s2, s->r, s->norm, x->dim);
    }
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook: the same contract for the int8 copy's bound (launch_i8_bound against i8_query_bound with r8 / norm8).
// INVALID without an int8 copy or for b > kShadowMaxQ.
int32_t cqs_hip_debug_shadow_bound_i8(cqs_hip_index* x, const float* queries, uint32_t b, float* out_device, float* out_host) CQS_ABI_TRY {
    if (!x || x->sh || !queries || !out_device || !out_host || b == 0) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    const Shadow* s = x->shadow;
    if (!s || !s->d_i8 || b > cqs::kShadowMaxQ) return CQS_HIP_ERR_INVALID;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // d_bq belongs to the searches
    float* d_q = nullptr;
    HIP_TRY(x, hipMalloc(&d_q, (size_t)b * x->dim * sizeof(float)));
    hipError_t e = hipMemcpyAsync(d_q, queries, (size_t)b * x->dim * sizeof(float), hipMemcpyHostToDevice, x->stream);
    if (e == hipSuccess) e = cqs::launch_i8_bound(d_q, b, x->dim, s->r8, s->norm8, s->d_bq, x->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_device, s->d_bq, (size_t)b * sizeof(float), hipMemcpyDeviceToHost, x->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
    hipFree(d_q);
    HIP_TRY(x, e);
    for (uint32_t i = 0; i < b; ++i) {
        const float* q = queries + (size_t)i * x->dim;
        double s2 = 0.0;
        for (uint32_t d = 0; d < x->dim; ++d) s2 += (double)q[d] * (double)q[d];
        out_host[i] = cqs::i8_query_bound(s2, s->r8, s->norm8, x->dim);
    }
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook: out[0, b) = d_bq as the last search left it (B_q of its queries, whichever launch computed it), once every
// search has completed.  INVALID without a shadow or for b > kShadowMaxQ.
int32_t cqs_hip_debug_shadow_bq(cqs_hip_index* x, uint32_t b, float* out) CQS_ABI_TRY {
    if (!x || x->sh || !out || b == 0) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    const Shadow* s = x->shadow;
    if (!s || b > cqs::kShadowMaxQ) return CQS_HIP_ERR_INVALID;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));
    HIP_TRY(x, hipMemcpyAsync(out, s->d_bq, (size_t)b * sizeof(float), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook: out[0, b) = the tail kernel's ticket words as the last search left them (0 between searches), once every search
// has completed.  INVALID without a shadow or for b > kShadowMaxQ.
int32_t cqs_hip_debug_shadow_tickets(cqs_hip_index* x, uint32_t b, uint32_t* out) CQS_ABI_TRY {
    if (!x || x->sh || !out || b == 0) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    const Shadow* s = x->shadow;
    if (!s || b > cqs::kShadowMaxQ) return CQS_HIP_ERR_INVALID;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));
    HIP_TRY(x, hipMemcpyAsync(out, s->d_tickets, (size_t)b * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook: out[0, b) = the verdicts of the last device-API search's queries (d_cert: 1 = certified, 0 = the gated f32
// launches answered), out_prefix[0, 2) = queries since the shadow was built whose finisher certified on the prefix / whose
// prefix failed and that went on to sort every candidate; once every search has completed.  INVALID without a shadow.
int32_t cqs_hip_debug_tail_verdicts(cqs_hip_index* x, uint32_t b, uint32_t* out, uint64_t* out_prefix) CQS_ABI_TRY {
    if (!x || x->sh || !out || !out_prefix || b == 0) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    const Shadow* s = x->shadow;
    if (!s || b > cqs::kShadowMaxQ) return CQS_HIP_ERR_INVALID;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));
    HIP_TRY(x, hipMemcpyAsync(out, s->d_cert, (size_t)b * sizeof(uint32_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipMemcpyAsync(out_prefix, s->d_stats + kStatPrefix, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Diagnostic hook (CQS_HIP_DEBUG_STAMPS=1 handles; tools/tail_stamps.py): out[0, 16) = the phase stamps query 0 of the last
// shadow search left (select_body's and the tail kernel's, 10 ns ticks), out[16, 19) = those of its finisher's slow path (0:
// not taken), once every search has completed; the words are zeroed for the next search.  INVALID on a handle without the stamp buffer.
int32_t cqs_hip_debug_tail_stamps(cqs_hip_index* x, uint64_t* out) CQS_ABI_TRY {
    if (!x || x->sh || !out) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (!x->d_dbg) return CQS_HIP_ERR_INVALID;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));
    HIP_TRY(x, hipMemcpyAsync(out, x->d_dbg, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipMemcpyAsync(out + 16, x->d_dbg + cqs::kDbgTailSlow, cqs::kDbgTailSlowWords * sizeof(uint64_t), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(x, hipMemsetAsync(x->d_dbg, 0, 16 * sizeof(uint64_t), x->stream));
    HIP_TRY(x, hipMemsetAsync(x->d_dbg + cqs::kDbgTailSlow, 0, cqs::kDbgTailSlowWords * sizeof(uint64_t), x->stream));
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook: out[0..4) = r, norm, r8, norm8 as the handle holds them (after shadow_convert's factor; r8 = norm8 = 0 without an
// int8 copy).  INVALID without a shadow.
int32_t cqs_hip_debug_shadow_stats(cqs_hip_index* x, double* out) CQS_ABI_TRY {
    if (!x || x->sh || !out) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    const Shadow* s = x->shadow;
    if (!s) return CQS_HIP_ERR_INVALID;
    out[0] = s->r; out[1] = s->norm;
    out[2] = s->d_i8 ? s->r8 : 0.0; out[3] = s->d_i8 ? s->norm8 : 0.0;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook: the stored copy of rows [row0, row0 + rows).  copy 1: out = [rows, dim] bf16 words (out_scales ignored);
// copy 2: out = [rows, dim] int8 codes, out_scales = [rows] f32.  INVALID without that copy or past the index's rows.
int32_t cqs_hip_debug_shadow_rows(cqs_hip_index* x, uint32_t copy, uint64_t row0, uint64_t rows, void* out, float* out_scales) CQS_ABI_TRY {
    if (!x || x->sh || !out || (copy != 1u && copy != 2u) || (copy == 2u && !out_scales)) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    const Shadow* s = x->shadow;
    if (!s || (copy == 2u && !s->d_i8) || row0 > x->n || rows > x->n - row0) return CQS_HIP_ERR_INVALID;
    if (rows == 0) return CQS_HIP_OK;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));
    if (copy == 1u) {
        HIP_TRY(x, hipMemcpyAsync(out, s->d_bf16 + row0 * x->dim, (size_t)rows * x->dim * sizeof(uint16_t), hipMemcpyDeviceToHost, x->stream));
    } else {
        HIP_TRY(x, hipMemcpyAsync(out, s->d_i8 + row0 * x->dim, (size_t)rows * x->dim, hipMemcpyDeviceToHost, x->stream));
        HIP_TRY(x, hipMemcpyAsync(out_scales, s->d_i8_scale + row0, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, x->stream));
    }
    HIP_TRY(x, hipStreamSynchronize(x->stream));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

// Test hook: the score rows of one scan, before any select.  `b` host queries [b, dim] (b <= kMaxGemvQ; <= kI8MaxQ for the
// int8 copy), the search's k, an optional host keep-bitset, mode and threshold: the bound kernel of the copy a search of
// (b, k) would take (shadow_uses_i8), then exactly the scan launch of shadow_pass (copy 1 = bf16, 2 = int8: scan_args at
// k' + 1) or of enqueue_search (copy 0 = f32), on the handle's stream.  out_scores [b, n] (dropped rows are -inf), out_bq [b]
// (for copy 1 / 2 that copy's own B_q).  The work-queue heads are zeroed again, as the select leaves them.  INVALID without a
// shadow, for a copy the handle does not have, or for a (b, k) that copy does not serve.
int32_t cqs_hip_debug_shadow_scores(cqs_hip_index* x, uint32_t copy, const float* queries, uint32_t b, uint32_t k,
                                    const uint32_t* keep_bitset, uint32_t mode, float threshold, float* out_scores,
                                    float* out_bq) CQS_ABI_TRY {
    if (!x || x->sh || !queries || !out_scores || !out_bq || b == 0 || copy > 2u || mode > CQS_HIP_MODE_PIPELINE) return CQS_HIP_ERR_INVALID;
    if (k == 0 || k > cqs::kMaxK) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    Shadow* s = x->shadow;
    if (!s || x->n == 0 || b > cqs::kMaxGemvQ || !shadow_takes(x, b, k, /*gemv_only=*/false)) return CQS_HIP_ERR_INVALID;
    if (copy == 2u && !(s->d_i8 && b <= cqs::kI8MaxQ && cqs::i8_k_ok(k))) return CQS_HIP_ERR_INVALID;
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));   // the scratch belongs to the searches
    const bool i8 = copy == 2u || (copy == 0u && shadow_uses_i8(x, b, k));
    const uint32_t kp = copy == 2u ? cqs::i8_kprime(k) : cqs::shadow_kprime(k);
    const uint32_t k_scan = copy == 0u ? k : kp + 1u;
    int32_t rc = ensure_scratch(x, b, k_scan);
    if (rc != CQS_HIP_OK) return rc;
    const uint32_t* d_keep = nullptr;
    if (keep_bitset) {
        if ((rc = stage_keep(x, keep_bitset, (x->n + 31) / 32)) != CQS_HIP_OK) return rc;
        d_keep = x->d_keep;
    }
    hipStream_t st = x->stream;
    HIP_TRY(x, hipMemcpyAsync(x->d_q, queries, (size_t)b * x->dim * sizeof(float), hipMemcpyHostToDevice, st));
    if (i8) HIP_TRY(x, cqs::launch_i8_bound(x->d_q, b, x->dim, s->r8, s->norm8, s->d_bq, st));
    else HIP_TRY(x, cqs::launch_shadow_bound(x->d_q, b, x->dim, s->r, s->norm, s->d_bq, st));
    if (copy == 0u) {
        const cqs::ScanArgs a = scan_args(x, x->d_q, b, k, d_keep, mode, threshold, sizeof(float), false, x->d_dbg, nullptr);
        HIP_TRY(x, cqs::launch_scan(a, st));
    } else {
        cqs::ScanArgs a = scan_args(x, x->d_q, b, k_scan, d_keep, mode, threshold, i8 ? sizeof(int8_t) : sizeof(uint16_t), true, nullptr, nullptr);
        a.group_tasks = shadow_group_tasks(x, i8, kp);
        if (i8) sweep_args(s, a);   // (as shadow_pass: this scan takes the handle's parity and flips it)
        if (i8) HIP_TRY(x, cqs::launch_scan_i8(a, s->d_i8, s->d_i8_scale, s->d_bq, st));
        else HIP_TRY(x, cqs::launch_scan_bf16(a, s->d_bf16, s->d_bq, st));
    }
    HIP_TRY(x, hipMemsetAsync(x->d_work, 0, cqs::kWorkWords * sizeof(uint32_t), st));   // (what the select does after a scan)
    const size_t row_b = (size_t)x->n * sizeof(float);
    HIP_TRY(x, hipMemcpy2DAsync(out_scores, row_b, x->d_scores, (size_t)pad_rows(x->n) * sizeof(float), row_b, b, hipMemcpyDeviceToHost, st));
    HIP_TRY(x, hipMemcpyAsync(out_bq, s->d_bq, (size_t)b * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(x, hipStreamSynchronize(st));
    return CQS_HIP_OK;
} CQS_ABI_CATCH(x)

}  // extern "C"
