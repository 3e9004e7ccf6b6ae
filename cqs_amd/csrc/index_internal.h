// index_internal.h — the index handle and the host helpers shared by the index's translation units (index.hip,
// index_persist.hip, index_combine.hip, index_shadow.hip, index_remove.hip, index_update.hip, index_knn.hip, index_diff.hip,
// index_match.hip, mmr.hip, sharded.hip).
// Internal to libcqs_hip.so (the public boundary is include/cqs_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cqs_hip.h"
#include "combine_queue.h"
#include "scan_kernels.h"

namespace cqs_sharded { struct ShardSet; }
namespace cqs_idx {
struct Shadow;
constexpr uint32_t kCombineCap = 32;         // queries per combined block (4 passes of 8) = rows of the handle's bitset table
}
namespace cqs_mmr { struct Scratch; }
namespace cqs_search { struct Args; }

// One single-query host search: its query, parameters and output buffers (the caller's own).  The combining queue of
// cqs_hip_index_search (index_combine.hip) parks these on their callers' stacks; the host search runs blocks of them (index.hip).
struct cqs_combine_req {
    const float* q;          // [dim] host, validated (finite)
    uint32_t k, mode;
    float thr;
    uint64_t* out_rows;
    float* out_scores;
    uint32_t* out_count;
    int32_t rc = 0;
    bool done = false;
    const uint32_t* keep = nullptr;   // nullable host keep-bitset of this query, ceil(len/32) words (filtered blocks)
    const uint32_t* allow = nullptr;  // nullable tag filter of this query, 32 host words (tagged blocks; never beside keep)
};

struct cqs_hip_index {
    int device = 0;
    uint64_t n = 0;         // rows
    uint64_t cap_rows = 0;  // allocated rows (owning index)
    uint32_t dim = 0;
    uint32_t metric = 0;
    uint64_t row_base = 0;
    bool borrow = false;
    float* d_rows = nullptr;
    hipStream_t stream = nullptr;

    // scratch, grown on demand (never inside an enqueue-only path once warm)
    uint32_t q_cap = 0;        // queries the scratch can hold
    uint64_t scr_n_pad = 0;    // score-row stride the scratch was sized for
    uint32_t k_cap = 0;
    float* d_q = nullptr;
    float* d_scores = nullptr;
    uint32_t* d_work = nullptr;   // scan work-queue heads
    unsigned long long* d_dbg = nullptr;  // CQS_HIP_DEBUG_STAMPS=1: select_finish phase stamps
    uint32_t n_cu = 256;
    float* d_gmax = nullptr;      // [q_cap, <= n_pad/16] per-task maxima (stride = tiers.total())
    uint64_t* d_gaux = nullptr;   // [min(q_cap, kGauxQueries), <= n_pad/16] (argmax lane, runner-up) of each task (gemv blocks)
    uint64_t* d_out_keys = nullptr;
    uint32_t* d_out_counts = nullptr;
    uint32_t* d_keep = nullptr;
    uint64_t keep_words_cap = 0;
    // One bitset per query of a filtered block (index.hip, search_filtered_locked): kCombineCap rows of keep_tab_stride
    // words = ceil(cap_rows / 32), and the pinned twin the rows are staged in.  Made on first use; null = none (the
    // filtered calls then run one by one over d_keep).
    uint32_t* d_keep_tab = nullptr;
    uint32_t* h_keep_tab = nullptr;
    uint64_t keep_tab_stride = 0;
    // pinned host staging
    float* h_q = nullptr;
    uint64_t* h_out_keys = nullptr;
    uint32_t* h_out_counts = nullptr;
    uint64_t* h_out_keys_dev = nullptr;     // device-visible addresses of the two buffers above (null: not mappable)
    uint32_t* h_out_counts_dev = nullptr;

    // Searches share one scratch (d_scores, d_gmax, d_work, d_q): the handle orders them across streams.
    // Every enqueue records `done` on its stream; an enqueue on a DIFFERENT stream first waits on it.
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    bool done_valid = false;

    bool timing = false;
    std::vector<hipEvent_t> ev;  // pairs: [2i] before, [2i+1] after the scan launches
    size_t ev_used = 0;          // events recorded since the last read

    // Row-sharded parent (cqs_hip_index_create_sharded): the fields above are unused except dim / metric /
    // row_base; every entry point dispatches to sharded.hip.
    cqs_sharded::ShardSet* sh = nullptr;

    mutable std::mutex mu;
    std::atomic<bool> poisoned{false};
    std::string last_error;

    // Combining queue (combine_queue.h; index_combine.hip, cqs_hip_index_search): concurrent single-query callers park here and
    // ride ONE pass over the corpus (up to kMaxGemvQ queries share the HBM stream in registers).  cq.mu orders the queue only;
    // the device work itself still runs under `mu`.  The reference serialises its callers behind Mutex<GpuState>
    // (src/cagra.rs:263) one search at a time; the daemon calls `search` from one thread per client
    // (src/cli/watch/daemon.rs:273).  cq.wait_us is CQS_HIP_COMBINE_WAIT_US.
    cqs_combine::Queue<cqs_combine_req, cqs_idx::kCombineCap> cq;
    bool combine = true;                  // CQS_HIP_COMBINE=0: every caller takes the serial path
    bool combine_relaxed = false;         // CQS_HIP_COMBINE_BITS=relaxed: blocks of >= 9 callers may run on the matrix cores (32 queries per
                                          // sweep instead of 8): answers within the parity tolerance of the lone call's, not its bits
    bool combine_filtered = true;         // CQS_HIP_COMBINE_FILTERED=0: single-query callers with a bitset take the serial path
    std::atomic<uint64_t> stat_passes{0}, stat_queries{0};   // combined passes run / queries they carried (unfiltered callers)
    std::atomic<uint64_t> stat_fpasses{0}, stat_fqueries{0}; // the same for the blocks of callers with a bitset
    bool combine_tagged = true;           // CQS_HIP_COMBINE_TAGGED=0: single-query callers with a tag filter take the serial path
    std::atomic<uint64_t> stat_tpasses{0}, stat_tqueries{0}; // the same for the blocks of callers with a tag filter
    std::atomic<int32_t> inject_fail{0};  // test hook (cqs_hip_debug_index_fail_next): the next host search (or remove) fails as a device error
    uint64_t remove_budget_rows = 0;      // test hook (cqs_hip_debug_index_remove_budget): rows per pass of remove; 0 = the bounce buffer's byte budget
    uint64_t update_budget_rows = 0;      // test hook (cqs_hip_debug_index_update_budget): rows per pass of update; 0 = the staging buffer's byte budget
    uint64_t diff_budget_pairs = 0;       // test hook (cqs_hip_debug_index_diff_budget): pairs per pass of diff, on the `a` handle; 0 = cqs_diff::kPassPairs

    // Staging of cqs_hip_index_update (index_update.hip; null until the first update): a pass's new rows and their
    // destination list, pinned, and the device block they are copied into.  Kept between calls, freed at destroy.
    void* upd_h = nullptr;
    void* upd_d = nullptr;
    uint64_t upd_bytes = 0;

    // Staging of cqs_hip_index_knn_graph (index_knn.hip; null until the first such call): a call's rows, scores and counts
    // in one block on the device and its pinned twin.  Kept between calls, freed at destroy.
    void* knn_h = nullptr;
    void* knn_d = nullptr;
    size_t knn_bytes = 0;

    // Staging of cqs_hip_index_diff (index_diff.hip; null until the first such call with this handle as `a`): a pass's
    // local row lists, sims, class words, compacted list and counts in one block on the device and its pinned twin, sized
    // for diff_pairs pairs (the largest pass seen).  Kept between calls, freed at destroy.
    void* diff_h = nullptr;
    void* diff_d = nullptr;
    uint64_t diff_pairs = 0;

    // Staging of cqs_hip_index_match (index_match.hip; null until the first such call with this handle as `a`): the two
    // local row lists and the packed bests of both sides in one block on the device and its pinned twin, sized for
    // match_rows rows of the two lists together (the largest call seen).  Kept between calls, freed at destroy.
    void* match_h = nullptr;
    void* match_d = nullptr;
    uint64_t match_rows = 0;

    // bf16 shadow (index_shadow.hip; null = off).  Its certified / fallback counts outlive it: they live on the handle.
    cqs_idx::Shadow* shadow = nullptr;
    std::atomic<uint64_t> stat_certified{0}, stat_fallbacks{0};
    std::atomic<uint64_t> stat_i8_certified{0}, stat_i8_fallbacks{0};   // those of them that the int8 copy served

    // Scratch of cqs_hip_index_pairwise / cqs_hip_index_mmr (mmr.hip; null until the first such call on this handle).
    cqs_mmr::Scratch* mmr = nullptr;

    // Row tags (index_tags.hip; null until the first set_tags): one u32 per row beside the corpus, the
    // library's own also on a borrowing handle.  Local rows [0, tagged) have a tag.  tags_cap >= cap_rows whenever d_tags
    // is set (extend regrows it with the corpus, remove compacts it with the rows).
    uint32_t* d_tags = nullptr;
    uint64_t tags_cap = 0;
    uint64_t tagged = 0;
    uint32_t* d_tag_count = nullptr;      // the kept rows of the last tags_keep_kernel launch, one partial count per workgroup
    uint32_t* h_tag_count = nullptr;      // (kTagMaxBlocks words), and the pinned block they are read back into
    // tags_keep_multi_kernel (§3.14a): the transposed filters of a block (4 KB, staged pinned, copied on the stream) and
    // the partial counts [kTagMultiMaxBlocks][32] with their pinned twin.  Made by the first block of tagged queries.
    uint32_t* d_tag_tbl = nullptr;
    uint32_t* h_tag_tbl = nullptr;
    uint32_t* d_tag_mcount = nullptr;
    uint32_t* h_tag_mcount = nullptr;
};

namespace cqs_idx {

constexpr size_t kMaxTimingEvents = 8192;
constexpr uint64_t kNtBytes = 200ull << 20;  // corpus larger than this streams past L2/MALL
constexpr uint32_t kGauxQueries = 32;        // query blocks up to this size (every gemv block the host paths form) carry the select's (argmax, runner-up) index
constexpr uint32_t kGauxMinK = 100;          // ... and only from this k on (below it the gather it replaces is a few groups)
constexpr size_t kDirectOutKeys = 8192;      // host searches of up to this many result keys have them written straight to pinned host memory

uint64_t pad_rows(uint64_t n);
int32_t fail(cqs_hip_index* idx, int32_t code, const char* what, hipError_t e = hipSuccess);
void free_scratch(cqs_hip_index* x);
int32_t ensure_scratch(cqs_hip_index* x, uint32_t b, uint32_t k);
uint32_t max_query_block(const cqs_hip_index* x);
// One bitset per query of a gemv block: the device table, its row stride in words and the table row of each query (host
// [b]; ScanArgs::keep_tab).  Passed beside a null d_keep.
struct KeepTab { const uint32_t* d_tab; uint32_t stride; const uint8_t* slot; };
// Scan + select arguments over the handle's corpus.  elem_bytes (4 f32, 2 the bf16 shadow) sizes `nontemporal`.
cqs::ScanArgs scan_args(const cqs_hip_index* x, const float* d_q, uint32_t b, uint32_t k, const uint32_t* d_keep,
                        uint32_t mode, float thr, size_t elem_bytes, bool gemv_only, void* dbg, const uint32_t* gate,
                        const KeepTab* tab = nullptr);
// The rows a shadow scan reads: the bf16 copy, or (bf16 null) the int8 codes and their row scales; bq: B_q of the block.
struct ShadowRows { const uint16_t* bf16; const int8_t* i8; const float* i8_scale; const float* bq; };
// The scan of `a` on st (over `shadow` when set; timed unless a.gate: the shadow scan was), then the select (out_keys null:
// the scan alone - the shadow's tail kernel selects, and zeroes the work-queue heads as the select does).
int32_t scan_select(cqs_hip_index* x, const cqs::ScanArgs& a, hipStream_t st, const ShadowRows* shadow,
                    uint64_t* out_keys, uint32_t* out_counts);
// Searches share one scratch: order `st` after the last search / record `done` on `st` at the end of one.  Caller holds mu.
inline hipError_t order_after_last(cqs_hip_index* x, hipStream_t st) {
    return x->done_valid && x->done_stream != st ? hipStreamWaitEvent(st, x->done, 0) : hipSuccess;
}
inline hipError_t record_done(cqs_hip_index* x, hipStream_t st) {
    const hipError_t e = hipEventRecord(x->done, st);
    if (e == hipSuccess) { x->done_stream = st; x->done_valid = true; }
    return e;
}
// Enqueue scan + select for queries already on the device.  Caller holds mu.  gate: ScanArgs::gate (gemv blocks only).
int32_t enqueue_search(cqs_hip_index* x, const float* d_q, uint32_t b, uint32_t k, const uint32_t* d_keep,
                       uint32_t mode, float thr, uint64_t* d_out_keys, uint32_t* d_out_counts, hipStream_t st,
                       bool gemv_only = false, const uint32_t* gate = nullptr, const KeepTab* tab = nullptr);
hipError_t quiesce(cqs_hip_index* x);
// cqs_hip_index_create without the bf16 shadow policy (the shards of a row-sharded parent stay on f32)
int32_t create_owned(const float* rows, uint64_t n, uint32_t dim, uint32_t metric, int32_t device, uint64_t row_base,
                     cqs_hip_index** out);
int32_t stage_keep(cqs_hip_index* x, const uint32_t* host_words, uint64_t words);
// d_keep holds at least `words` u32 (regrown after a quiesce).  Caller holds mu.
int32_t ensure_keep(cqs_hip_index* x, uint64_t words);
// The handle's bitset table sized for cap_rows (made or regrown here; false = none: not enough memory).  Caller holds mu.
bool ensure_keep_tab(cqs_hip_index* x);
void free_keep_tab(cqs_hip_index* x);
int32_t create_common(uint64_t n, uint32_t dim, uint32_t metric, int32_t device, uint64_t row_base,
                      cqs_hip_index** out, cqs_hip_index** made);
void read_combine_env(cqs_hip_index* x);
// bf16 shadow (index_shadow.hip).  Caller holds mu (or owns the new handle).
int32_t shadow_auto(cqs_hip_index* x);
int32_t shadow_extend(cqs_hip_index* x, uint64_t n_old);
void shadow_free(cqs_hip_index* x);
void shadow_sweep_reset(cqs_hip_index* x);   // after extend / remove / update: the int8 scan's next sweep runs forwards
// The shadow's per-row buffers, which remove compacts beside d_rows (index_remove.hip); null: that copy is off.
struct ShadowBuffers { uint16_t* bf16; int8_t* i8; float* i8_scale; };
ShadowBuffers shadow_buffers(const cqs_hip_index* x);
// Around the launches of an update on a handle with the shadow on (index_update.hip), the stream idle: begin clears the
// outlier word and hands out the stats words the two build bodies fold into (*stats8: the int8 copy's); end reads the
// maxima back once and refreshes r / norm / r8 / norm8 as the build passes do.  An outlier row turns the shadow off as in
// extend (the call still succeeds).
int32_t shadow_update_begin(cqs_hip_index* x, unsigned long long** stats, unsigned long long** stats8);
int32_t shadow_update_end(cqs_hip_index* x);
// cqs_hip_index_update on one single-device index, planned (update_host.h): index_update.hip.  Caller holds x->mu.
int32_t update_entries(cqs_hip_index* x, const uint32_t* local, uint64_t local_off, const uint64_t* order, uint64_t count,
                       const float* vectors);
void update_free(cqs_hip_index* x);
void knn_free(cqs_hip_index* x);   // the staging of cqs_hip_index_knn_graph (index_knn.hip)
void diff_free(cqs_hip_index* x);  // the staging of cqs_hip_index_diff (index_diff.hip)
void match_free(cqs_hip_index* x); // the staging of cqs_hip_index_match (index_match.hip)
bool shadow_takes(const cqs_hip_index* x, uint32_t b, uint32_t k, bool gemv_only);
bool shadow_uses_i8(const cqs_hip_index* x, uint32_t b, uint32_t k);   // of a block shadow_takes: the int8 copy serves it
int32_t shadow_pass(cqs_hip_index* x, const float* d_q, uint32_t nb, uint32_t k, const uint32_t* d_keep, uint32_t mode,
                    float thr, uint64_t* out_keys, uint32_t* out_counts, hipStream_t st, const uint32_t** device_gate,
                    const KeepTab* tab = nullptr);
// The gated f32 fallback behind a device-API shadow_pass as one launch; *taken = false: not this block (the caller enqueues
// the gated scan + select).
int32_t shadow_fallback(cqs_hip_index* x, const float* d_q, uint32_t nb, uint32_t k, const uint32_t* d_keep, uint32_t mode,
                        float thr, uint64_t* out_keys, uint32_t* out_counts, hipStream_t st, const uint32_t* gate, bool* taken);
// The last host shadow pass's verdicts, pinned, valid after x->stream's wait (queues their copy when not mappable).
hipError_t shadow_verdicts(cqs_hip_index* x, uint32_t nb, const uint32_t** h_cert);

// plan_search (search_host.h) under the handle's mutex: true = there is device work, else *rc is the call's answer.
bool search_planned(cqs_hip_index* x, const cqs_search::Args& a, int32_t* rc);
// One request per query of a planned call: its own output rows and, filtered, its own bitset.
std::vector<cqs_combine_req> requests(const cqs_search::Args& a, float thr);
// The test hook (cqs_hip_debug_index_fail_next), consumed: an armed hook fails this one host search as a device error would.
int32_t injected_failure(cqs_hip_index* x);
// The block loop of the host search: `b` queries at k_eff over the rows d_keep keeps (device bitset of the whole index,
// ceil(n/32) words; null: every row).  Caller holds mu, has set the device and ordered x->stream after the last search.
int32_t search_blocks_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k_eff, const uint32_t* d_keep,
                             uint32_t mode, float threshold, bool gemv_only);
// One staged block to its answers (index.hip): queries staged[i] in h_q row i, through the shadow copies where they take
// the block, then the f32 scan for the rest.  slots (with a null d_keep): query i is filtered by row slots[i] of the handle's
// bitset table.  Caller holds mu; x->stream is ordered after the last search; ensure_scratch covers the block.
int32_t answer_block(cqs_hip_index* x, std::vector<const cqs_combine_req*>& staged, uint8_t* slots, uint32_t k,
                     const uint32_t* d_keep, uint32_t mode, float thr, bool gemv_only);
// Row tags (index_tags.hip).  Caller holds mu (or owns the handle).
void tags_free(cqs_hip_index* x);
// After extend regrew the corpus: the column regrown to cap_rows with its contents.  No memory for it: the tags are dropped
// (tagged = 0, reason in last_error) and the index stays usable.  The stream is idle.
void tags_regrow(cqs_hip_index* x);

// The host-buffer searches proper (index.hip).  Caller holds mu, has checked the arguments and zeroed the counts.
int32_t search_host_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k, const uint32_t* keep_bitset,
                           uint32_t mode, float threshold, bool gemv_only);
int32_t search_filtered_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k, uint32_t mode, float threshold);
// The tagged twin of search_filtered_locked (index_tags.hip): `b` queries with one (k, mode, threshold) and a tag filter
// EACH (qs[i].allow), every one answered with the bytes of cqs_hip_index_search_tagged(that query, 1, ..., that filter).
// Caller holds mu, has passed tagged_ready, checked the arguments and zeroed the counts.
int32_t search_tagged_locked(cqs_hip_index* x, const cqs_combine_req* qs, uint32_t b, uint32_t k, uint32_t mode, float threshold);
// The checks every tagged call makes before anything else, under mu: OK = a single-device handle, not poisoned, whose
// every row has a tag.  None of the refusals poisons; the reason goes to last_error as "<who>: ...".
int32_t tagged_ready(cqs_hip_index* x, const uint32_t* allow, const char* who);
// Park one single-query request on the combining queue and return its answer (index_combine.hip).
int32_t combine_search(cqs_hip_index* x, cqs_combine_req& r);

// persistence over one or more device segments in row order (index_persist.hip)
struct Segment { int device; float* d_rows; uint64_t rows; hipStream_t stream; };
int32_t save_segments(cqs_hip_index* err_owner, const std::vector<Segment>& segs, uint32_t dim, uint32_t metric,
                      const char* path, uint64_t* out_checksum);
int32_t open_blob(const char* path, uint32_t expected_dim, uint64_t expected_rows, int* fd_out, uint64_t* rows,
                  uint32_t* metric, uint64_t* checksum);
int32_t read_blob_into(int fd, uint64_t checksum, uint32_t dim, const std::vector<Segment>& segs);

}  // namespace cqs_idx

// Pairwise similarities and the MMR re-rank of a candidate pool (mmr.hip).  Caller holds the owner's mutex.
namespace cqs_mmr {
void free_scratch(cqs_hip_index* x);   // (sets the owner's device)
// G = X X^T over the m rows src[h_idx[i]] (h_idx null: rows 0 .. m-1 of src), then either the D2H of G (out_gram [m, m]) or
// the greedy loop and the D2H of its `limit` picks (out_gram null; 0 < limit < m, lambda in [0, 1)).  `src` lies on
// owner->device, the work runs on `st`; scratch and errors belong to `owner`.  Returns with the outputs written.
int32_t run(cqs_hip_index* owner, hipStream_t st, const float* src, const uint32_t* h_idx, const float* h_scores, uint32_t m,
            uint32_t limit, float lambda, float* out_gram, uint32_t* out_picks);
// A shard's part of a sharded pool: its mc candidates' rows (local indices h_idx) gathered on c->stream into the dense
// [mc, dim] block *out_block of c's own scratch.  Errors are left on c.
int32_t gather_rows(cqs_hip_index* c, const uint32_t* h_idx, uint32_t mc, const float** out_block);
// The parent's [m, dim] staging block on its first device.
int32_t staging(cqs_hip_index* parent, uint32_t m, float** out_block);
}  // namespace cqs_mmr

// Row-sharded parent handles (sharded.hip); each takes the parent handle and does its own locking.
namespace cqs_sharded {
int32_t pairwise(cqs_hip_index* parent, const uint64_t* cand_rows, uint32_t m, float* out);
int32_t mmr(cqs_hip_index* parent, const uint64_t* cand_rows, const float* cand_scores, uint32_t m, uint32_t limit,
            float lambda, uint32_t* out_picks, uint32_t* out_count);
void destroy(cqs_hip_index* parent);
int32_t search(cqs_hip_index* parent, const float* queries, uint32_t b, uint32_t query_dim, uint32_t k,
               const uint32_t* keep_bitset, uint32_t mode, float threshold, uint64_t* out_rows, float* out_scores,
               uint32_t* out_counts);
// One sealed block of the combining queue (index_combine.hip): nb single-query callers with the same (k, mode, threshold), every
// query finite and of the parent's dimension; takes the parent mutex for the block.  gemv passes only, so each caller gets
// the bits its lone call gets.
int32_t search_combined(cqs_hip_index* parent, cqs_combine_req* const* batch, uint32_t nb);
int32_t neighbors(cqs_hip_index* parent, uint64_t target_row, uint32_t limit, uint64_t* out_rows, float* out_scores,
                  uint32_t* out_count);
int32_t extend(cqs_hip_index* parent, const float* rows, uint64_t n_new);
int32_t update(cqs_hip_index* parent, const uint64_t* rows, const float* vectors, uint64_t m, uint64_t* out_updated);
void update_budget(cqs_hip_index* parent, uint64_t rows);   // (the test hook, handed to every shard; caller holds the parent's mutex)
int32_t save(cqs_hip_index* parent, const char* path, uint64_t* out_checksum);
uint64_t len(const cqs_hip_index* parent);
int32_t poisoned(const cqs_hip_index* parent);
void set_timing(cqs_hip_index* parent, int32_t enable);
int32_t scan_time(cqs_hip_index* parent, uint32_t* launches, double* total_ms);
}  // namespace cqs_sharded

#define HIP_TRY(idx, expr)                                                        \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess)                                                     \
            return cqs_idx::fail((idx), _e == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE, #expr, _e); \
    } while (0)
