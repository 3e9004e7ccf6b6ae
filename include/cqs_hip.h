/*
 * cqs_hip.h — C ABI of libcqs_hip.so, the MI355X (gfx950) implementation of the
 * cqs semantic-search hot path: exact brute-force dot/cosine scan + top-k over
 * an HBM-resident [n, dim] f32 corpus, and (embed section) the embedding
 * forward.  This is the drop-in boundary: plain pointers and sizes, opaque
 * handles, int32 status codes, no exceptions, no callbacks, no torch types.
 *
 * The reference (jamie8johnson/cqs, Rust) has no FFI for this path today; the
 * seams it would bind this library behind are cited per entry point
 * (file:line relative to the cqs repo root, v1.51.0).  INTEGRATION.md shows
 * the Rust `extern "C"` block + `impl VectorIndex` a maintainer would add.
 *
 * Threading: every entry point is safe to call concurrently on one handle
 * (the handle serialises device work behind an internal mutex, like
 * `CagraIndex.gpu: Mutex<GpuState>`, src/cagra.rs:263).  Searches of one handle share
 * one device scratch: `cqs_hip_index_search_device` returns with its kernels still in
 * flight, and the handle orders the NEXT search (any entry point, any stream) behind
 * them with an event, so calls on different streams serialise on the device instead of
 * racing; extend / remove / save / destroy wait for the last enqueued search first.  Device failures never
 * abort: they return a negative status, set the handle's poisoned flag
 * (src/index.rs:203-205, src/cagra.rs:472-489) and leave a message for
 * cqs_hip_index_last_error.
 */
#ifndef CQS_HIP_H
#define CQS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------- */
#define CQS_HIP_OK              0
#define CQS_HIP_ERR_INVALID    (-1)  /* bad argument (null, k > max_k, dim unsupported, ...) */
#define CQS_HIP_ERR_DEVICE     (-2)  /* HIP runtime error; handle is poisoned */
#define CQS_HIP_ERR_NOMEM      (-3)  /* device or host allocation failed */
#define CQS_HIP_ERR_POISONED   (-4)  /* handle was poisoned by an earlier device error */
#define CQS_HIP_ERR_NO_DEVICE  (-5)  /* no usable gfx950 device */

/* DistanceMetric (src/index.rs:45-56).  Both rank by the raw inner product;
 * COSINE additionally promises unit-norm rows so that score == cosine and
 * `index_scores_are_cosine()` (src/index.rs:236-238) may return true. */
#define CQS_HIP_METRIC_COSINE 0u
#define CQS_HIP_METRIC_DOT    1u

/* Score mode of a search.
 * RAW     : rank and return the raw dot product — the `VectorIndex::search`
 *           contract (src/index.rs:139-146; CAGRA's score at src/cagra.rs:656-662).
 * PIPELINE: rank on clamp(score,0,1) and drop scores < threshold — what the
 *           reference's brute-force scan ranks on with a default SearchFilter
 *           (src/search/scoring/candidate.rs:550 clamp, :513-519 ThresholdGate,
 *           loop at src/search/query.rs:469-481). */
#define CQS_HIP_MODE_RAW      0u
#define CQS_HIP_MODE_PIPELINE 1u

/* Largest k one search call serves (`VectorIndex::max_k`, src/index.rs:219-221;
 * production asks for candidate_count_for(limit) = max(5*limit, 500),
 * src/limits.rs:315-320). */
#define CQS_HIP_MAX_K 1024u

typedef struct cqs_hip_index cqs_hip_index;

/* ---- library / device ------------------------------------------------------ */
const char* cqs_hip_version(void);
/* Number of visible HIP devices (0 if none / runtime unusable).  Mirrors
 * `CagraIndex::gpu_available` (src/cagra.rs:336-376) for backend selection. */
int32_t cqs_hip_device_count(void);
/* Free + total HBM bytes of `device` (gpu_available_for sizing, src/cagra.rs:336-376). */
int32_t cqs_hip_device_mem(int32_t device, uint64_t* free_bytes, uint64_t* total_bytes);

/* ---- index lifetime -------------------------------------------------------- */
/* Build an exact index over `n` rows of `dim` f32 (host, row-major, rows in
 * rowid order = id_map order; replaces `CagraIndex::build_from_flat`,
 * src/cagra.rs:922-960).  The rows are copied to HBM.  Nothing is skipped:
 * the caller pre-filters zero / non-finite rows exactly like
 * `prepare_index_data` (src/hnsw/mod.rs:688-746) so len() and row->id agree.
 * `row_base` is added to every emitted row id (0 for a whole corpus; the shard
 * offset when the corpus is row-sharded over several GPUs/processes).
 * dim must be a multiple of 4 and <= 4096 (the reference's presets reach 4096, src/embedder/models.rs:572). */
int32_t cqs_hip_index_create(const float* rows, uint64_t n, uint32_t dim, uint32_t metric,
                             int32_t device, uint64_t row_base, cqs_hip_index** out);
/* Same, from rows already resident in `device`'s HBM.  borrow != 0: the index
 * uses the caller's buffer in place (caller keeps it alive and unmodified);
 * borrow == 0: the rows are copied device-to-device.
 * Every single-device create / create_device / load may build the bf16 shadow (see cqs_hip_index_set_bf16_scan).
 * On a borrowed handle the shadow is a snapshot of the rows taken here: rows written after create break the
 * "unmodified" contract, and searches may then return the old rows' answers or a mix of old and new ones.  A
 * caller that must write its rows disables the shadow first (cqs_hip_index_set_bf16_scan(idx, 0)). */
int32_t cqs_hip_index_create_device(const void* d_rows, uint64_t n, uint32_t dim, uint32_t metric,
                                    int32_t device, uint64_t row_base, int32_t borrow,
                                    cqs_hip_index** out);
/* Row-sharded index over several GPUs of ONE process (north_star): the reference's daemon is
 * one process holding an `Arc<dyn VectorIndex>` (src/cli/batch/context.rs:157, GPU state behind one mutex
 * src/cagra.rs:263), so the multi-GPU path sits behind the SAME handle type.  The n rows are cut in rowid order
 * into n_devices near-equal contiguous shards (shard starts are multiples of 256 rows), shard s lives on
 * devices[s]; every other entry point accepts the returned handle: `cqs_hip_index_search` broadcasts the query
 * block to every device, scans the shards concurrently, moves the per-shard packed (score,row) candidates with
 * ONE RCCL all-gather over xGMI (ncclGroupStart/End, communicators from ncclCommInitAll) and merges them on the
 * host with cqs_hip_merge_keys - the result contract is exactly the single-device one.  RCCL is bound at run time
 * (dlopen "librccl.so.1"); n_devices == 1 needs none.  A device may be named more than once (test hook for
 * one-GPU boxes): such a list cannot form an RCCL clique and gathers by device-to-device copies instead.
 * `cqs_hip_index_search_device` is not available on a sharded handle (-> CQS_HIP_ERR_INVALID); extend appends to
 * the last shard that holds rows; save writes one blob (rows of all shards in order), which either loader reads. */
int32_t cqs_hip_index_create_sharded(const float* rows, uint64_t n, uint32_t dim, uint32_t metric,
                                     const int32_t* devices, uint32_t n_devices, uint64_t row_base,
                                     cqs_hip_index** out);
int32_t cqs_hip_index_load_sharded(const char* path, uint32_t expected_dim, uint64_t expected_rows,
                                   const int32_t* devices, uint32_t n_devices, uint64_t row_base, cqs_hip_index** out);
/* Number of shards (1 for a single-device handle) and, per shard: its device, first global row, row count, and
 * whether its gathers go through RCCL (1) or device-to-device copies (0). */
uint32_t cqs_hip_index_shards(const cqs_hip_index* idx);
int32_t cqs_hip_index_shard_info(const cqs_hip_index* idx, uint32_t shard, int32_t* device, uint64_t* first_row,
                                 uint64_t* rows, int32_t* gathers_with_rccl);

/* Append rows (host) to an owning index — incremental add, the contract the
 * tiered backend's extend() exposes (src/tiered.rs:1-43).  Not valid on a
 * borrowing index. */
int32_t cqs_hip_index_extend(cqs_hip_index* idx, const float* rows, uint64_t n_new);
/* Remove rows from an owning index in place — the other half of the tiered backend's purpose, "to clean orphaned
 * vectors and absorb deltas" without a rebuild (src/tiered.rs:13-17).  `rows` are `m` global row ids (row_base
 * included, as cqs_hip_index_neighbors takes them), in any order; a duplicate counts once.  *out_removed (may be NULL)
 * = the distinct rows removed.  Afterwards len has dropped by that many, the surviving rows keep their relative order
 * and are renumbered densely from row_base, and the index is indistinguishable from one created from the surviving
 * rows: searches return the same bytes, save writes the same blob.  Nothing is reallocated.  The bf16 / int8 shadow
 * copies are compacted with the rows and keep their bounds (still valid, at worst looser) and their counts.  Removing
 * every row leaves an empty index that extend can refill.  m == 0 changes nothing.  CQS_HIP_ERR_INVALID, with the
 * index untouched and the reason in last_error: an id outside [row_base, row_base + len), NULL rows with m > 0, a
 * borrowing index (the rows are the caller's), a row-sharded handle.  Waits for the searches in flight, as extend does;
 * a device failure half-way leaves the rows half-moved and poisons the handle. */
int32_t cqs_hip_index_remove(cqs_hip_index* idx, const uint64_t* rows, uint64_t m, uint64_t* out_removed);
/* Rewrite stored rows of an owning index in place — what the reference's enrichment pass and its watch loop do to chunks
 * that keep their id (Store::update_embeddings_batch, src/store/chunks/crud.rs:349-480; upsert_chunks_batch's ON
 * CONFLICT(id) DO UPDATE, src/store/chunks/async_helpers.rs:314-330).  `rows` are `m` global row ids (row_base included,
 * as remove and neighbors take them), in any order, each at most once; `vectors` is [m, dim] f32, host, row-major, and
 * vectors[i] replaces stored row rows[i].  *out_updated (may be NULL) = m on success.  Afterwards len, row_base, the row
 * numbering, the tag column, capacity and every scratch buffer are what they were, and in every other respect the index
 * is indistinguishable from one created from the patched rows: searches return the same bytes, save writes the same
 * blob, the bf16 / int8 shadow copies hold the bytes a fresh build holds.  The shadow's bounds take the new rows in and
 * let nothing out (still valid, at worst looser, as after remove).  Rows are taken as extend takes them: none is skipped
 * or checked for finiteness; a finite row with a component of magnitude >= 2^64 turns the shadow off (last_error says so)
 * and the call still succeeds.  The new rows are staged through a buffer of at most 64 MiB, pinned and on the device,
 * which the handle keeps until destroy; larger updates run in passes.  m == 0 changes nothing.  Supported on a
 * row-sharded handle (shard starts do not move).  CQS_HIP_ERR_INVALID, with the index untouched, the handle not poisoned
 * and the reason in last_error: an id outside [row_base, row_base + len), an id named twice, NULL rows or vectors with
 * m > 0, a borrowing index (the rows are the caller's).  Waits for the searches in flight, as extend does; a device
 * failure half-way leaves some rows written and poisons the handle. */
int32_t cqs_hip_index_update(cqs_hip_index* idx, const uint64_t* rows, const float* vectors, uint64_t m,
                             uint64_t* out_updated);
/* Synchronises the index's streams, then frees everything (src/cagra.rs:289-302). */
void cqs_hip_index_destroy(cqs_hip_index* idx);

/* ---- persistence (the `index.cagra` + `.meta` pair of the reference, src/cagra.rs:973-1157,
 * 1174-1330) -----------------------------------------------------------------
 * save: writes `path` = 64-byte header {magic "CQSHIPF1", version, dim, metric, rows, checksum} +
 * the raw little-endian f32 rows, through `path.tmp` + rename (atomic like
 * save_blob_atomic_with_rollback, src/cagra.rs:1468-1592).  *out_checksum receives the 64-bit
 * content checksum for the caller's sidecar (the shim writes the CagraMeta-style JSON: magic,
 * version, dim, chunk_count, id_map, checksum, metric).  A poisoned index refuses to save.
 * load: validates magic / version / dim / rows (expected_rows 0 = any) / file size / checksum;
 * any mismatch -> CQS_HIP_ERR_INVALID and the caller deletes the files and rebuilds
 * (src/cagra.rs:1739-1750). */
int32_t cqs_hip_index_save(cqs_hip_index* idx, const char* path, uint64_t* out_checksum);
int32_t cqs_hip_index_load(const char* path, uint32_t expected_dim, uint64_t expected_rows, int32_t device,
                           uint64_t row_base, cqs_hip_index** out);

/* ---- index properties (VectorIndex, src/index.rs:139-239) ------------------ */
uint64_t cqs_hip_index_len(const cqs_hip_index* idx);       /* len()  :149 */
uint32_t cqs_hip_index_dim(const cqs_hip_index* idx);       /* dim()  :160 */
uint32_t cqs_hip_index_metric(const cqs_hip_index* idx);
uint32_t cqs_hip_index_max_k(const cqs_hip_index* idx);     /* max_k() :219 */
int32_t  cqs_hip_index_poisoned(const cqs_hip_index* idx);  /* is_poisoned() :203 */
int32_t  cqs_hip_index_device(const cqs_hip_index* idx);
uint64_t cqs_hip_index_row_base(const cqs_hip_index* idx);
/* Copies the last error / warning text (NUL-terminated, truncated to cap). */
size_t cqs_hip_index_last_error(const cqs_hip_index* idx, char* buf, size_t cap);

/* ---- search: host buffers --------------------------------------------------
 * `VectorIndex::search` / `search_with_filter` for a block of `b` queries
 * (src/index.rs:146,167; the CAGRA exemplar src/cagra.rs:443-672,727-820).
 *
 * queries   [b * query_dim] f32, host.
 * query_dim must equal dim(); a mismatch yields out_counts[*] = 0 and
 *           CQS_HIP_OK (reference: warn + empty Vec, src/cagra.rs:449-456).
 * k         0 -> counts 0; k > max_k -> CQS_HIP_ERR_INVALID (callers trim
 *           with cap_k_to_backend, src/search/query.rs:232-245).
 * keep_bitset nullable, host, ceil(len/32) words, bit (i%32) of word i/32 = keep
 *           local row i (src/cagra.rs:747-757).  All-pass == unfiltered, none ->
 *           counts 0, k is capped at the number of kept rows (src/cagra.rs:760-775).
 * mode/threshold: see CQS_HIP_MODE_*.
 * A query with a non-finite component yields count 0 (src/cagra.rs:464-470).
 *
 * Result per query q: out_rows[q*k .. q*k+out_counts[q]) (row_base + local row)
 * and out_scores likewise, ordered by (score desc under f32 total order, row
 * asc) — the reference's order (candidate.rs:327, neighbors.rs:131) with
 * integer ids.  Non-finite scores are never emitted (src/cagra.rs:649-651).
 * Slots past out_counts[q] are untouched.
 *
 * Concurrent callers (the daemon calls `search` from one thread per client on a shared
 * Arc<dyn VectorIndex>, src/cli/watch/daemon.rs:273; CAGRA serialises them behind
 * Mutex<GpuState>, src/cagra.rs:263): calls with b == 1 that meet on one handle are
 * COMBINED - a caller that finds the device busy parks its query, and whoever takes the
 * device next scans every parked query with the same (k, mode, threshold) in one pass over
 * the corpus (up to 8 queries share the HBM stream; more run as consecutive passes inside
 * the same hold of the device).  Each caller receives exactly the bytes a lone call would
 * have produced.  A lone caller pays two uncontended mutex operations.
 * Callers with a keep_bitset (what `search_with_filter` and the hybrid search send,
 * src/search/query.rs:860-888,1113-1132) are combined too, on a single-device handle: they
 * form blocks of their own - never mixed with unfiltered callers - in which every query
 * keeps its own bitset: a pass reads the rows that ANY of its queries keeps and scores each
 * query over the rows IT keeps (see cqs_hip_index_search_filtered).
 * CQS_HIP_COMBINE_FILTERED=0 (read at create) keeps them one after the other, as before.
 * A handle made by cqs_hip_index_create_sharded / _load_sharded combines its unfiltered
 * callers the same way (round 5): the block goes to every shard at once, one gather, one
 * host merge per query; its callers with a bitset run one after the other.
 * Calls with b > 1 run one after the other as before.
 * CQS_HIP_COMBINE_BITS=relaxed (read at create; default: exact) is an opt-in throughput mode: a block of >= 9 callers may
 * run on the matrix cores - 32 queries per corpus sweep instead of 8 (16 callers: 25 k q/s against 14 k) - and its answers
 * are then within the parity tolerance of the lone call's (scores <= 2e-6 apart on unit vectors, same ids outside
 * near-ties), not its bits.
 * If a pass fails, the call that led it returns the device error and every parked caller
 * returns CQS_HIP_ERR_POISONED.  CQS_HIP_COMBINE=0 (read at create) turns the queue off. */
int32_t cqs_hip_index_search(cqs_hip_index* idx, const float* queries, uint32_t b, uint32_t query_dim,
                             uint32_t k, const uint32_t* keep_bitset, uint32_t mode, float threshold,
                             uint64_t* out_rows, float* out_scores, uint32_t* out_counts);

/* ---- search: device buffers, asynchronous ----------------------------------
 * Same computation with every buffer in the index's device memory space and
 * no host synchronisation: work is enqueued on `stream` (a hipStream_t; NULL =
 * the HIP null stream, which is what PyTorch's default stream is) and the call
 * returns; results are ordered after it on that stream only.  Used by the bench (inputs
 * resident in HBM) and by the sharded multi-GPU path, whose per-shard
 * candidates feed an RCCL all-gather straight from HBM.
 * d_queries [b*dim] f32 must hold finite values (the caller checks; the host
 * entry point above does it for host queries).  d_keep_bitset nullable.
 * d_out_keys [b*k] u64 receives the packed candidates
 *     key = (ordered_u32(score) << 32) | (0xFFFFFFFF - global_row)
 * sorted descending (i.e. score desc, row asc), unused slots = 0.
 * d_out_counts [b] u32.  cqs_hip_unpack_keys decodes keys on the host. */
int32_t cqs_hip_index_search_device(cqs_hip_index* idx, const float* d_queries, uint32_t b, uint32_t k,
                                    const uint32_t* d_keep_bitset, uint32_t mode, float threshold,
                                    uint64_t* d_out_keys, uint32_t* d_out_counts, void* stream);

/* ---- neighbours of a stored row ----------------------------------------------
 * `find_neighbors` (src/cli/commands/search/neighbors.rs:86-132): exact kNN of a row that is already in the
 * index, the row itself excluded (:116-118), ordered (score desc, row asc) (:131), limit clamped to
 * [1, SIMILAR_LIMIT_MAX = 100] (:95, src/cli/limits.rs:40).  target_row is a GLOBAL row id (row_base + local).
 * out_rows / out_scores hold at least min(limit, 100) slots; *out_count <= min(limit, 100, len - 1).
 * target_row outside the index -> CQS_HIP_ERR_INVALID (the reference fails to load the target's embedding,
 * :98-106).  Scores are raw dots (the reference sums f32 left to right: equal to 1e-6 on unit vectors).
 * Rows with a non-finite score are dropped as in every search of this library; an index built through
 * `prepare_index_data` holds none. */
#define CQS_HIP_NEIGHBORS_MAX 100u
int32_t cqs_hip_index_neighbors(cqs_hip_index* idx, uint64_t target_row, uint32_t limit, uint64_t* out_rows,
                                float* out_scores, uint32_t* out_count);

/* ---- exact kNN graph of the stored rows ----------------------------------------
 * `find_neighbors` applied to each of the `m` stored rows first_row .. first_row + m - 1 (GLOBAL row ids) in one call:
 * what `cqs index --umap` needs before anything else (umap-learn accepts a precomputed graph), near-duplicate detection,
 * `neighbors` / `related` for a whole file's functions.  The rows are read where they lie in HBM; only the answer
 * crosses the bus, once.
 * Results: L = clamp(limit, 1, CQS_HIP_NEIGHBORS_MAX).  Target i owns out_rows[i*L .. i*L + out_counts[i]) and the same
 * range of out_scores (each [m * L], host; out_counts [m]), ordered (score desc under the f32 total order, row asc), the
 * target itself excluded, out_counts[i] <= min(L, len - 1).  Scores are raw dots (RAW mode); rows with a non-finite
 * score are never emitted; slots past the count are written as 0.  An index of one row gives count 0.
 * Tiles: T = min(256, the handle's largest query block) depends on len alone; local rows are cut into fixed tiles
 * [T*t, min(T*t + T, len)), and the call runs every tile its range touches as ONE block of T queries - all rows of the
 * tile - through the f32 scan and select every block of that size uses, at k1 = min(L + 1, len), then emits the targets
 * that were asked for.  So a target's answer depends on the corpus and the target only, not on how the caller cuts the
 * range into calls; it is byte for byte what cqs_hip_index_search returns for the block of its tile's rows at k1 with the
 * target dropped; and where its tile has at most 8 rows (the ragged last one can) it is byte for byte
 * cqs_hip_index_neighbors' answer.  Against the reference's find_neighbors: ids exact outside near-ties, scores to 1e-5.
 * Refused with CQS_HIP_ERR_INVALID, the outputs untouched, the handle not poisoned and the reason in last_error, in this
 * order: a NULL handle; a NULL output with m > 0; m > CQS_HIP_KNN_MAX_TARGETS; any part of the range outside the index;
 * a row-sharded handle.  m == 0 returns CQS_HIP_OK and touches nothing.  A poisoned handle -> CQS_HIP_ERR_POISONED; a
 * device failure poisons the handle.
 * The call holds the handle for its whole length: searches on the same handle wait for it, so a daemon that serves
 * queries meanwhile should pass a few tiles per call, not the corpus.  A first call grows the scratch to the 256-query
 * block's (256 * padded rows * 4 bytes of scores, as any 256-query search does) and a staging block of m * (12 L + 4)
 * bytes, pinned and on the device, which the handle keeps until destroy. */
#define CQS_HIP_KNN_MAX_TARGETS 65536u
int32_t cqs_hip_index_knn_graph(cqs_hip_index* idx, uint64_t first_row, uint64_t m, uint32_t limit,
                                uint64_t* out_rows, float* out_scores, uint32_t* out_counts);

/* ---- UMAP layout of a kNN graph ---------------------------------------------------
 * `cqs index --umap` (src/cli/commands/index/umap.rs) streams every embedding to a Python child that runs umap-learn with
 * n_neighbors = 15, min_dist = 0.1, metric = "cosine" and stores 2-D coordinates for the cluster view of `cqs serve`.
 * cqs_hip_index_knn_graph is the first half of that work; this is the second: the fuzzy-simplicial-set weights of the
 * graph and the epochs of force-directed layout, on the device.  The layout is its own handle: it takes a graph, not an
 * index, and never holds an index's mutex.  The rules below are umap-learn's published algorithm with the stated
 * departures; they are the specification.
 * Input: exactly what cqs_hip_index_knn_graph writes for the whole corpus of a handle with row_base 0.  Vertex i owns
 * knn_rows[i*stride .. i*stride + knn_counts[i]) and the same range of knn_scores (host; raw dots of unit rows; the target
 * itself excluded; a list names a vertex at most once).  The arrays are read during `create` only.
 * Distances: d = max(0, 1 - score) in f32.
 * Smooth-kNN, per vertex with c = its count:  rho = the smallest d > 0 of its list, 0 if there is none.  sigma by
 *   umap-learn's bisection in f32: lo = 0, hi = inf, mid = 1, at most 64 rounds of
 *     psum = sum over the list of (d - rho > 0 ? expf(-(d - rho) / mid) : 1);  stop when |psum - target| < 1e-5;
 *     psum > target: hi = mid, mid = (lo + hi) / 2;  else lo = mid, mid = hi infinite ? 2 mid : (lo + hi) / 2
 *   with target = log2f(c + 1) - umap-learn counts the point itself among its n_neighbors, so a graph of limit 14 is its
 *   n_neighbors = 15 - and sigma = the last mid.  Then sigma = max(sigma, 1e-3 * mean(d of the list)); stated departure:
 *   umap-learn uses the global mean where rho == 0.  c == 0: rho = sigma = 0, no forward edges.
 *   w(i->j) = 1 where d - rho <= 0 or sigma == 0, else expf(-(d - rho) / sigma).
 * Fuzzy union: s(i,j) = w(i->j) + w(j->i) - w(i->j) * w(j->i), 0 for an absent direction, the sum, the product and the
 *   difference each rounded.  The adjacency of i is its forward list in list order, then the vertices that list i and are
 *   not in i's list, in ascending id: every undirected edge is stored at both ends with the same weight bits.  w_max is
 *   the maximum over all entries.  This order is part of the contract: it is what cqs_hip_layout_graph returns and what
 *   "adjacency slot" means below.
 * Epoch e = 1 .. E (E = n_epochs, or 500 for n <= 10000 and 200 above where that is 0), on a snapshot - stated departure:
 *   umap-learn updates in place, edge by edge; here every vertex reads the previous epoch's coordinates and writes the
 *   next, so the result is a pure function of its inputs, without atomics or races.
 *     alpha = learning_rate * (1 - (e - 1) / E)
 *     an adjacency entry is active iff floorf(e * p) != floorf((e - 1) * p) with p = s / w_max: f32 operations, each
 *     rounded once
 *     for vertex i, the sum over its active entries (other end j, slot t) of
 *       2 * clip(ca * (y_i - y_j)),  ca = -2ab d2^(b-1) / (a d2^b + 1), d2 = |y_i - y_j|^2; 0 where d2 == 0  (twice:
 *         umap-learn lists the edge in both directions and each copy moves both ends)
 *       + for each draw k < negative_samples, of vertex q:  clip(cr * (y_i - y_q)),
 *         cr = 2 repulsion b / ((0.001 + d2) (a d2^b + 1)); 0 where q == i or d2 == 0
 *     clip is to [-4, 4] per coordinate;  y_i_new = y_i + alpha * sum.
 * Random draws: counter-based, from murmur3's 32-bit finaliser
 *     fmix(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *     hash(seed, epoch, vertex, slot, draw) = fmix(fmix(fmix(fmix(fmix(fmix(lo32(seed) ^ 0x9E3779B9) ^ hi32(seed)) ^ epoch)
 *                                             ^ vertex) ^ slot) ^ draw)
 *     q = (uint64(hash) * n) >> 32
 *   with slot = the entry's position in its vertex's adjacency.  Initial coordinates, unless cqs_hip_layout_set_coords
 *   replaces them, are uniform in [-10, 10): coordinate c of vertex i = float(hash(seed, 0, i, 0, c) >> 8) * (20 / 2^24)
 *   - 10 in f32, the product and the difference each rounded.  There is no device RNG state and nothing depends on the
 *   launch grid.
 * Determinism: the coordinates after epoch e are a function of the graph arrays, the parameters and the initial
 *   coordinates only.  run(50) and run(20); run(30) give the same bytes; two handles made from the same inputs give the
 *   same bytes.  A wave adds its terms in a fixed order that is not the sequential one: lane l of 64 adds the entries
 *   l, l + 64, ... in that order (attraction, then the draws 0, 1, ...), then the lanes add as v += v[lane ^ 32], ^ 16,
 *   ^ 8, ^ 4, ^ 2, ^ 1.
 * Degenerate sizes: n < 2 is valid: the coordinates are the origin, edges is 0 and `run` launches nothing.
 * create    refuses with CQS_HIP_ERR_INVALID, nothing left allocated, *out NULL, in this order: a NULL out, params or
 *           array; n > 2^31; stride == 0 or stride > CQS_HIP_NEIGHBORS_MAX; a count greater than stride; a neighbour id
 *           >= n or equal to its own vertex (the text names the vertex); a non-finite a, b, learning_rate or repulsion or
 *           a non-positive a or b; n_epochs > 10000.  The reason is this thread's create text: cqs_hip_layout_last_error
 *           with a NULL handle.  The adjacency is built on the host (the graph arrives from host memory anyway), the
 *           weights on the device.  Device memory: two coordinate buffers (16 n bytes) and the adjacency, 8 bytes per
 *           entry, at most 2 n stride entries, plus 20 n bytes of offsets, rho and sigma.
 * graph     the structure above, each output nullable: offsets [n + 1] u64, nbrs / weights [edges], rho / sigma [n],
 *           *w_max (0 where edges == 0).
 * set_coords / coords   xy [n * 2] f32, host: x then y of each vertex.  set_coords replaces the current coordinates and
 *           leaves the epoch counter alone.
 * run       the next `epochs` epochs, clamped at n_epochs; *epoch_after (nullable) = epochs done so far.  One launch per
 *           epoch on the layout's own stream, one wait per call.
 * A device failure poisons the layout handle only (CQS_HIP_ERR_POISONED afterwards).  Calls on one handle serialise. */
typedef struct cqs_hip_layout cqs_hip_layout;
typedef struct cqs_hip_layout_params {
    float a;                   /* 1.5769434603 with b = 0.8950608779: umap-learn's fit for min_dist 0.1, spread 1 */
    float b;
    float learning_rate;       /* 1.0 */
    float repulsion;           /* 1.0 */
    uint32_t negative_samples; /* 5 */
    uint32_t n_epochs;         /* 0: 500 for n <= 10000, 200 above */
    uint64_t seed;             /* 42 */
} cqs_hip_layout_params;
void cqs_hip_layout_params_default(cqs_hip_layout_params* params);
int32_t cqs_hip_layout_create(int32_t device, uint64_t n, uint32_t stride, const uint64_t* knn_rows,
                              const float* knn_scores, const uint32_t* knn_counts, const cqs_hip_layout_params* params,
                              cqs_hip_layout** out);
uint64_t cqs_hip_layout_len(const cqs_hip_layout* layout);
uint64_t cqs_hip_layout_edges(const cqs_hip_layout* layout);
uint32_t cqs_hip_layout_epochs(const cqs_hip_layout* layout);
int32_t cqs_hip_layout_graph(cqs_hip_layout* layout, uint64_t* offsets, uint32_t* nbrs, float* weights, float* rho,
                             float* sigma, float* w_max);
int32_t cqs_hip_layout_set_coords(cqs_hip_layout* layout, const float* xy);
int32_t cqs_hip_layout_coords(cqs_hip_layout* layout, float* xy);
int32_t cqs_hip_layout_run(cqs_hip_layout* layout, uint32_t epochs, uint32_t* epoch_after);
size_t cqs_hip_layout_last_error(const cqs_hip_layout* layout, char* buf, size_t cap);
void cqs_hip_layout_destroy(cqs_hip_layout* layout);
/* The two halves in one call, for a caller that has the index and wants the coordinates: cqs_hip_index_knn_graph at
 * limit n_neighbors - 1 (clamped to [1, CQS_HIP_NEIGHBORS_MAX]) over the whole corpus in calls of 4096 targets - the
 * index is held per call, not for the whole length - then a layout with the default parameters but n_epochs and seed,
 * run to its end on the index's device.  out_xy [len * 2] f32, host.  Fewer than 2 rows give the origin.  Refuses what
 * cqs_hip_index_knn_graph refuses (a row-sharded handle among it) and a handle whose row_base is not 0; the reason is in
 * the index's last_error. */
int32_t cqs_hip_index_umap_project(cqs_hip_index* idx, uint32_t n_neighbors, uint32_t n_epochs, uint64_t seed,
                                   float* out_xy);

/* ---- PCA of the stored rows ---------------------------------------------------------
 * The top principal axes of the resident corpus in a few streaming passes: the global picture of a corpus on its own (and
 * how anisotropic a model's embeddings are: variance / total_variance), and the initial coordinates of a UMAP layout that
 * umap-learn calls init="pca" (below).  The rules here are the specification.
 * Definition: X is the n stored f32 rows, mu their column mean, Z = X - 1 mu^T.  The axes are orthonormal eigenvectors of
 *   Z^T Z, largest eigenvalue first; out_variance[k] is the Rayleigh quotient a_k^T Z^T Z a_k / (n - 1) (sklearn's
 *   explained_variance_); out_total_variance = (sum |x_i|^2 - n |mu|^2) / (n - 1), the trace of the covariance.  Sign: the
 *   component of largest magnitude of each axis is positive, the lowest index on ties.
 * Shift: all sums are taken over x_i - x_0, x_0 the first stored row (the covariance does not change, the f32 sums lose
 *   less, and a corpus of identical rows gives exactly mean = x_0, Z = 0).  mu = x_0 + (sum (x_i - x_0)) / n; that sum and the
 *   squares of out_total_variance, evaluated as (sum |x_i - x_0|^2 - n |mu - x_0|^2) / (n - 1), are one pass in f64.
 * Method: block subspace iteration with p = min(8, dim) columns.
 *   Start: V0[d][j] = float(hash(seed, 0, d, 2, j) >> 8) * 2^-23 - 1 with the layout section's hash (slot 2: the initial
 *     coordinates use slot 0, the jitter below slot 1), orthonormalised on the host in f64.
 *   Gram-Schmidt (host, f64, column order): column j has its components along the columns before it subtracted one after
 *     the other, twice, and is divided by its norm.  Breakdown rule: a column whose norm before is 0 or not finite, or whose
 *     norm after is at most 1e-10 of the norm before, is replaced by the first unit basis vector e_d, d ascending, whose
 *     residual against the earlier columns has a squared norm of at least 1 / (2 dim); that residual is normalised.
 *   A pass (n_passes of them; 0 means 16; at most 64): V rounded to f32; on the device, per row, t = (x - x_0) V - c with
 *     c = (mu - x_0)^T V, Y += (x - x_0) (x) t, S += t, products and sums in f32; the host forms Z^T Z V = Y - (mu - x_0)
 *     (x) S in f64 and orthonormalises it into the next V.
 *   After the last pass one more gives H = V^T (Z^T Z V) for the f32 V the device saw; H is symmetrised and eigen-solved
 *     on the host (cyclic Jacobi, f64); the axes are V W's first n_components columns rounded to f32.
 * Determinism: the corpus is cut into slabs of 1024 rows by local row number.  A slab's partial Y [dim x 8] and S [8] are
 *   fmaf chains of the f32 matrix cores in an order fixed by the kernel (t: the columns in steps of 4, the steps dealt
 *   round-robin to four chains that are added as ((0 + 1) + 2) + 3; Y: the slab's rows in ascending order); the slab
 *   partials are added in ascending slab order in f64.  No float atomics.  The answer is a function of the stored rows,
 *   seed and n_passes only: not of the grid, the device's CU count, or whether the rows came by `create` or by `create` +
 *   `extend`; after `update` or `remove` it is that of a fresh index of the rows now stored.
 * cqs_hip_index_pca      out_mean [dim], out_axes [n_components * dim] (axis k at k * dim), out_variance [n_components],
 *   out_total_variance [1], host.  Holds the handle's mutex for the whole call, so that every pass sees the same rows:
 *   searches on the handle wait (DESIGN.md §3.18b has the measured length).  Device memory for the call: 32 dim + 4
 *   ceil(n / 1024) (8 dim + 8) bytes of partials, about 24 MB at 1M x 768; freed before it returns.
 * cqs_hip_index_pca_project   out[i * n_components + k] = (x_{first_row + i} - mean) . axes_k in f32 for the m stored rows
 *   from first_row (a GLOBAL row id) on: the subtraction first, then per lane an fmaf chain over the float4 columns lane,
 *   lane + 64, ..., then the lanes added as v += v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  Any m: launches of at most
 *   16 * CQS_HIP_KNN_MAX_TARGETS rows each, the handle held for the call.  mean / axes are the caller's (host), so rows
 *   can be projected onto the axes of another index.
 * Refused with CQS_HIP_ERR_INVALID, nothing written, the handle not poisoned and the reason in last_error, in this order -
 *   pca: a NULL handle; a NULL output; n_components == 0, > CQS_HIP_PCA_MAX_COMPONENTS or > dim; n_passes > 64; a
 *   row-sharded handle ("pca: not built for a row-sharded handle"); fewer than 2 rows; and, after the passes, a total variance,
 *   an entry of H or one of the p Rayleigh values that is not finite as f32 ("pca: non-finite rows").  pca_project: a NULL handle; (m == 0 returns CQS_HIP_OK here and touches nothing;)
 *   a NULL mean or axes; a NULL out; n_components as above; a row-sharded handle; any part of the range outside the index.
 *   A poisoned handle -> CQS_HIP_ERR_POISONED; a device failure poisons the handle. */
#define CQS_HIP_PCA_MAX_COMPONENTS 4
int32_t cqs_hip_index_pca(cqs_hip_index* idx, uint32_t n_components, uint32_t n_passes, uint64_t seed,
                          float* out_mean /*[dim]*/, float* out_axes /*[n_components * dim]*/,
                          float* out_variance /*[n_components]*/, float* out_total_variance /*1*/);
int32_t cqs_hip_index_pca_project(cqs_hip_index* idx, const float* mean, const float* axes, uint32_t n_components,
                                  uint64_t first_row, uint64_t m, float* out /*[m * n_components]*/);
/* cqs_hip_index_umap_project with a choice of initial coordinates.  init == CQS_HIP_UMAP_INIT_RANDOM: exactly the bytes of
 * cqs_hip_index_umap_project.  init == CQS_HIP_UMAP_INIT_PCA (umap-learn's init="pca"; where the clusters end up relative
 * to each other then follows the corpus, not the draw): cqs_hip_index_pca with 2 components (1 where dim == 1: y = 0), the
 * default passes and `seed`; cqs_hip_index_pca_project of all rows; then umap-learn's noisy_scale_coords on the host in
 * f32, each operation rounded once:
 *     coord = proj * (10 / max|proj|) + jitter,  jitter = (float(hash(seed, 0, i, 1, c) >> 8) * 2^-24 - 0.5) * 2e-4
 * (max over both coordinates of all rows; the jitter keeps duplicated rows from starting coincident, where the layout
 * gives them zero force), set as the layout's coordinates before its first epoch.  Where max|proj| is 0 (or so small
 * that the quotient overflows) or a projection is not finite the hashed uniform coordinates stay.  Fewer than 2 rows give
 * the origin as before.  Any other `init` is CQS_HIP_ERR_INVALID.  n_epochs > 10000 is refused before the passes, in the
 * layout's words; a refusal of pca or pca_project ("pca: non-finite rows", a row-sharded handle) or CQS_HIP_ERR_POISONED
 * from them is the call's, out_xy untouched.  The index is held per call of pca, pca_project and knn_graph, not across
 * them. */
#define CQS_HIP_UMAP_INIT_RANDOM 0
#define CQS_HIP_UMAP_INIT_PCA    1
int32_t cqs_hip_index_umap_project_init(cqs_hip_index* idx, uint32_t n_neighbors, uint32_t n_epochs, uint64_t seed,
                                        uint32_t init, float* out_xy);

/* ---- UMAP transform of new rows ----------------------------------------------------
 * The watch loop appends a few hundred chunks; this gives them coordinates in a layout that exists, without projecting the
 * corpus again: umap-learn's `transform`, restated in the conventions of the layout section above, departures stated.
 * The old coordinates - the anchors - do not move, so no new vertex depends on another: weights, initial position and all
 * epochs of a vertex are the private loop of one wave, and the whole call is ONE launch.
 * Input: n anchor coordinates Y [n * 2] f32 (x then y), fixed; for each of m new vertices a list of at most `stride` anchor
 *   ids (< n) with raw dot scores and a count: vertex i owns nbr_rows[i*stride .. i*stride + nbr_counts[i]) and the same
 *   range of nbr_scores (host) - what `search` of the new vectors at k = n_neighbors over the anchored rows returns.  There
 *   is no self entry: a new row is not an anchor.  Vertex i of the call has the id id_base + i, its future row number; the
 *   id is used only in the hash.  Anchor coordinates are NOT checked for finiteness: a non-finite anchor gives non-finite
 *   answers to the vertices that list or draw it.
 * Weights, per vertex with c = its count:  d = max(0, 1 - score);  rho = 0 (umap-learn's transform runs with
 *   local_connectivity - 1 = 0);  sigma from the layout's bisection with target = log2f(c) - c, not c + 1: the list holds
 *   all n_neighbors entries - then sigma = max(sigma, 1e-3 * mean(d));  w_t = 1 where d_t <= 0, else expf(-d_t / sigma).
 *   c == 0: the vertex is written as (0, 0) and never moves; so is one whose weights all underflow to 0 (scores far below
 *   -1: not unit rows).
 * Initial position: W = sum of w_t, q_t = w_t / W, y = sum of q_t * Y[j_t], each quotient and each product rounded once,
 *   the sums in the wave order below.
 * Epoch e = 1 .. E (E = n_epochs, or where that is 0, 100 for m <= 10000 and 30 above: umap-learn's transform defaults):
 *     alpha = (learning_rate / 4) * (1 - (e - 1) / E)
 *     entry t is active iff floorf(e * p) != floorf((e - 1) * p) with p = w_t / (the vertex's own largest w) - stated
 *       departure: umap-learn divides by the maximum over the whole batch; the per-vertex maximum makes a vertex's answer a
 *       function of the anchors, its own list and its id only, not of how the caller batches
 *     for each active entry, slot t and anchor j: clip(ca * (y - Y_j)) ONCE (the edge exists in one direction and only its
 *       head moves), then for each draw k < negative_samples, q = draw_vertex(hash(seed, e, id, t, k), n):
 *       clip(cr * (y - Y_q)).  ca, cr, clip and the hash are the layout's; a term is 0 where d2 == 0.
 *     y_new = y + alpha * sum, the sum taken at the epoch's starting y - stated departure, as in the layout: umap-learn
 *       re-reads y after every edge.
 * Order of addition (part of the contract): lane l of 64 holds the slots l and l + 64; it adds slot l's attraction, then
 *   slot l's draws 0, 1, .., then slot l + 64 likewise; the lanes then add as v += v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.
 * Determinism: a vertex's answer is a function of the anchors, its list, its id and the parameters.  One call of m and two
 *   calls cut anywhere with matching id_base give the same bytes.
 * `epochs` is how many of the E epochs to run, clamped at E: CQS_HIP_TRANSFORM_ALL runs all of them, 0 returns the initial
 *   positions.  out_xy [m * 2]; out_sigma [m] and out_weights [m * stride] (slots past a count written as 0) are nullable.
 * Refused with CQS_HIP_ERR_INVALID, the outputs untouched, in this order: NULL params, or out_xy, an array or the anchors
 *   NULL while m > 0; (m == 0 returns CQS_HIP_OK here;) n == 0; n > 2^31; m > CQS_HIP_KNN_MAX_TARGETS; id_base + m > 2^32;
 *   stride == 0 or stride > CQS_HIP_NEIGHBORS_MAX; a count greater than stride; a neighbour id >= n (the text names the
 *   vertex); the layout's parameter checks, n_epochs > 10000 among them.
 * cqs_hip_umap_transform          the handle-less call, for a daemon that keeps its coordinates in SQLite: uploads 8 n bytes
 *           per call; refusals and failures are in this thread's handle-less text, cqs_hip_layout_last_error(NULL, ..).
 * cqs_hip_layout_transform        the anchors are the handle's current coordinates where they lie on the device: nothing is
 *           uploaded but the lists.  n is the handle's length; the parameters are the handle's, except n_epochs (0: the
 *           default for m).  The handle's coordinates and epoch counter do not change; the new vertices do not join the
 *           layout.  The reason of a refusal is the handle's last_error; a device failure poisons the layout only.
 * cqs_hip_index_umap_transform    `search` of `vectors` [m * dim] at k = clamp(n_neighbors, 1, CQS_HIP_NEIGHBORS_MAX) over
 *           the rows [0, n_anchors) - the plain search where n_anchors == len, else the filtered one with a keep-bitset of
 *           the first n_anchors rows, so it also works after `extend` - in blocks of at most 256 queries, the index held per
 *           block; then the transform on the index's device with id_base = n_anchors and the default parameters but
 *           n_epochs and seed.  anchors_xy [n_anchors * 2], out_xy [m * 2], host.  A vector of the wrong kind (non-finite)
 *           finds no neighbours and lands on (0, 0).  Refuses a row-sharded handle, a row_base other than 0 and
 *           n_anchors > len, as umap_project does, and m > CQS_HIP_KNN_MAX_TARGETS; the reason is in the index's
 *           last_error and the index is not poisoned by a transform's failure. */
#define CQS_HIP_TRANSFORM_ALL 0xFFFFFFFFu
int32_t cqs_hip_umap_transform(int32_t device, uint64_t n, const float* anchors_xy, uint64_t m, uint32_t stride,
                               const uint64_t* nbr_rows, const float* nbr_scores, const uint32_t* nbr_counts,
                               const cqs_hip_layout_params* params, uint64_t id_base, uint32_t epochs,
                               float* out_xy /*[m*2]*/, float* out_sigma /*[m], nullable*/,
                               float* out_weights /*[m*stride], nullable*/);
int32_t cqs_hip_layout_transform(cqs_hip_layout* layout, uint64_t m, uint32_t stride, const uint64_t* nbr_rows,
                                 const float* nbr_scores, const uint32_t* nbr_counts, uint32_t n_epochs, uint64_t id_base,
                                 uint32_t epochs, float* out_xy, float* out_sigma, float* out_weights);
int32_t cqs_hip_index_umap_transform(cqs_hip_index* idx, uint64_t n_anchors, const float* anchors_xy,
                                     const float* vectors, uint64_t m, uint32_t n_neighbors, uint32_t n_epochs, uint64_t seed,
                                     float* out_xy);

/* ---- semantic diff of two resident indexes --------------------------------------
 * The arithmetic of `semantic_diff` (src/diff.rs:99-246; `detect_drift`, src/drift.rs:51-120, sits on it): for every
 * chunk present in both stores the reference fetches both embeddings from SQLite in batches of 1000, computes
 * `full_cosine_similarity` (src/math.rs:35-67) and keeps the pairs below a threshold.  Here both corpora are resident:
 * the rows are read where they lie in HBM and only the answer crosses the bus.  Matching chunks and sorting the result
 * are string work and stay with the caller.
 * Pair i is (stored row rows_a[i] of `a`, stored row rows_b[i] of `b`), both GLOBAL row ids (row_base included, as
 * neighbors / remove / update take them); order is free and a row may appear in any number of pairs.  `a == b` is
 * allowed, and so are borrowing handles (rows are only read).
 * Per pair, exactly src/diff.rs:191-202: sim = full_cosine_similarity(row_a, row_b).unwrap_or(0.0) - dot and both squared
 * norms accumulated in f64 from the f32 rows, denom = sqrt(na) * sqrt(nb); denom == 0 or a non-finite f32 result means
 * "undefined": sim is 0.0f and the pair counts in out_counts[2].  The pair is modified iff sim < threshold (an f32
 * compare), else unchanged; an undefined pair is classified through its 0.0 like any other, as the reference does.
 * out_sims      [m] host, nullable: sim of pair i.  NULL: only the modified list and the counts cross the bus.
 * out_mod_pairs [m] host, nullable: the pair indices of the modified pairs in ascending order, out_counts[0] of them;
 * out_mod_sims  [m] host, nullable: their sims in the same order.  Both or neither.  Slots past the count are untouched.
 * out_counts    [3] host: modified, unchanged, undefined; out_counts[0] + out_counts[1] == m.
 * A pair's sim depends on its two rows and dim only - not on m, the pair's position, the passes or the grid - and
 * sim(x, y) and sim(y, x) are the same bits.  Against the reference's left-to-right f64 loop the three sums differ by at
 * most ~dim * 2^-53 relative, so the f32 result is the reference's or an adjacent f32; where the three sums are exact
 * and the squared norms perfect squares it is the reference's bits.
 * Refused with CQS_HIP_ERR_INVALID, all outputs untouched, neither handle poisoned and the reason in `a`'s last_error,
 * in this order: a NULL a or b; (m == 0 returns CQS_HIP_OK here: out_counts = {0,0,0} if non-NULL, nothing else
 * touched); NULL rows_a, rows_b or out_counts; exactly one of out_mod_pairs / out_mod_sims NULL; a NaN threshold (a
 * stated departure: the reference's `sim < NaN` makes every pair unchanged); either handle row-sharded; the handles on
 * different devices; dim(a) != dim(b) (a stated departure: the reference scores such pairs 0.0); any row outside its
 * index (the text names the first offending pair index and which side).  A poisoned handle on either side ->
 * CQS_HIP_ERR_POISONED.  A device failure poisons `a` only.
 * The call holds BOTH handles' mutexes for its whole length (taken in address order, once when a == b) and orders its
 * launches after the last search of each: searches and maintenance on either handle wait for it.  Work runs in passes of
 * at most 2^20 pairs; a first call makes a staging block of 24 bytes per pair of the largest pass seen, pinned and on the
 * device, which `a` keeps until destroy.  A handle that never calls diff pays nothing. */
int32_t cqs_hip_index_diff(cqs_hip_index* a, const uint64_t* rows_a, cqs_hip_index* b, const uint64_t* rows_b,
                           uint64_t m, float threshold, float* out_sims, uint64_t* out_mod_pairs, float* out_mod_sims,
                           uint64_t* out_counts);

/* ---- best partners between two row lists of two resident indexes -------------------
 * `semantic_diff` matches chunks by key - (file, name, chunk_type) in the reference (src/diff.rs:43-53) - so a function
 * moved to another file, or renamed, leaves one `removed` and one unrelated `added` entry; the comment at :45-47 admits
 * it for line moves and stops there, the host having no cheap way to compare every removed chunk with every added one.
 * With both corpora resident that is the cross similarity of two row lists, reduced on the device to the best partner
 * of every row on either side; the [m_a, m_b] matrix is never stored and only the bests cross the bus.
 * rows_a [m_a], rows_b [m_b]  GLOBAL row ids of `a` and of `b` (row_base included, as diff / neighbors / remove take
 *            them), host.  Any order; a row may be listed more than once.  `a == b` is allowed, and so are borrowing
 *            handles (rows are only read).
 * S[i][j]    the f32 dot of stored row rows_a[i] of `a` and stored row rows_b[j] of `b` - the cosine on COSINE indexes -
 *            accumulated as cqs_hip_index_pairwise accumulates: one fma chain over k in the order 32 it + 8 u + c,
 *            32 it + 8 u + 4 + c (it = 0 .., u = 0..3, c = 0..3).  It is bit for bit the entry cqs_hip_index_pairwise
 *            gives for the same two rows where they live in one index: a function of the two rows and dim only, not of
 *            m_a, m_b, the positions, the tiling or the grid; (a, b) and (b, a) give the same bits.
 * out_best_a [m_a] u64, out_score_a [m_a] f32, host: out_best_a[i] = the POSITION j in rows_b with the greatest S[i][j]
 *            under the f32 total order, the lowest j among equals; out_score_a[i] = that entry.  Only finite entries are
 *            considered (a non-finite entry never wins, as no search of this library emits one); without a finite entry -
 *            which includes m_b == 0 - out_best_a[i] = UINT64_MAX and out_score_a[i] = 0.0f.
 * out_best_b [m_b], out_score_b [m_b]  the same with the roles exchanged: the best i per j, the lowest i among equals.
 *            Ties going to the lowest position on both sides, the pairs with out_best_a[i] == j && out_best_b[j] == i are
 *            a one-to-one matching.
 * m_a == 0 && m_b == 0 returns CQS_HIP_OK and touches nothing.
 * Refused with CQS_HIP_ERR_INVALID, every output untouched, neither handle poisoned and the reason in `a`'s last_error,
 * in this order: a NULL a or b; (both lists empty returns CQS_HIP_OK here, whatever the other arguments); NULL rows_a with
 * m_a > 0 or NULL rows_b with m_b > 0; a NULL output of a side with m > 0; m_a or m_b above CQS_HIP_MATCH_MAX; either
 * handle row-sharded; the handles on different devices; dim(a) != dim(b); any row outside its index (the text names the
 * side and the first offending position, side a first).  A poisoned handle on either side -> CQS_HIP_ERR_POISONED.  A
 * device failure poisons `a` only.
 * The call holds BOTH handles' mutexes for its whole length (taken in address order, once when a == b) and orders its
 * launches after the last search of each.  A first call makes a staging block of 12 bytes per listed row (both lists
 * together) of the largest call seen, pinned and on the device, which `a` keeps until destroy; a handle that never calls
 * match pays nothing.  One copy back and one wait per call.  Longer lists: cut either into blocks of at most
 * CQS_HIP_MATCH_MAX and keep, per row, the greater score under the total order, then the lower position. */
#define CQS_HIP_MATCH_MAX 65536u         /* rows per side of one call */
int32_t cqs_hip_index_match(cqs_hip_index* a, const uint64_t* rows_a, uint32_t m_a, cqs_hip_index* b,
                            const uint64_t* rows_b, uint32_t m_b, uint64_t* out_best_a, float* out_score_a,
                            uint64_t* out_best_b, float* out_score_b);

/* ---- cosine MMR re-rank of a candidate pool ------------------------------------
 * The reference diversifies its top-K pool with `mmr_rerank` (src/search/mmr.rs:59-126) over a surface-feature
 * similarity, because it drops the embeddings after scoring: "embedding-MMR is a follow-up" (mmr.rs:30-37,
 * src/search/query.rs:540-542).  Behind this handle every candidate's row is still in HBM, so both calls run on the
 * device and only the answer crosses the bus.
 * cand_rows  [m] GLOBAL row ids as cqs_hip_index_search emits them (row_base + local), host.  A row outside the index
 *            -> CQS_HIP_ERR_INVALID; m > CQS_HIP_MMR_MAX -> CQS_HIP_ERR_INVALID.  A row may appear more than once: its
 *            entries are then fully similar (equal to the row's own diagonal entry, bit for bit).
 * pairwise:  out [m * m] f32, host: out[i*m + j] = the f32 dot of stored rows cand_rows[i] and cand_rows[j] - the
 *            cosine on a COSINE index.  out[i*m + j] and out[j*m + i] are the same bits; an entry depends on its two
 *            rows only (not on m, the other candidates or the handle's sharding).  m == 0 writes nothing.
 * mmr:       `mmr_rerank` with similarity(i, j) = that dot; cand_scores [m] f32 are the relevance scores, in the
 *            caller's (relevance-descending) order.  Line by line:
 *              lambda is clamped to [0, 1] (mmr.rs:60); limit = min(limit, m) (:62);
 *              limit == 0 or m == 0 -> *out_count = 0, CQS_HIP_OK (:64-66);
 *              lambda >= 1 or m <= limit -> picks 0 .. limit-1, no device work (:67-69);
 *              per step and unselected i: max_sim = the fold of f32 `max` over the selected from 0.0 (:83-90) - negative
 *              similarities count as 0, the first step's max_sim is 0; mmr = lambda * score - (1 - lambda) * max_sim
 *              in f32, the two products and the difference each rounded (:92; no fused multiply-add);
 *              the winner is the greatest mmr under the f32 total order, the lowest index among equals (:107-111).
 *            out_picks [>= min(limit, m)] u32 receives indices INTO THE CANDIDATE LIST in pick order, *out_count their
 *            number (= min(limit, m)).
 *            Stated departure: a non-finite lambda or candidate score -> CQS_HIP_ERR_INVALID (the reference's env parser
 *            refuses the former, mmr.rs:166-178; no search of this library emits the latter).  Arguments are checked
 *            before the early answers above.
 * Neither call poisons the handle on CQS_HIP_ERR_INVALID.  Scratch (the [m, m] Gram matrix: 4 MB at 1024) is made on
 * the first call, sized for the largest m seen, freed at destroy; a handle that never calls these pays nothing.
 * A row-sharded handle gathers the pool's rows on its first shard's device and runs the same kernels: same bytes. */
#define CQS_HIP_MMR_MAX 1024u            /* pool size limit, = CQS_HIP_MAX_K */
int32_t cqs_hip_index_pairwise(cqs_hip_index* idx, const uint64_t* cand_rows, uint32_t m, float* out);
int32_t cqs_hip_index_mmr(cqs_hip_index* idx, const uint64_t* cand_rows, const float* cand_scores, uint32_t m,
                          uint32_t limit, float lambda, uint32_t* out_picks, uint32_t* out_count);

/* Host helpers for packed candidate keys (see above). */
void cqs_hip_unpack_keys(const uint64_t* keys, size_t count, uint64_t* rows, float* scores);
/* Final host-side k-way merge of per-shard candidate lists for one query
 * (north_star: "RCCL all-gather of per-shard (score,id) candidates before the
 * final host-side merge").  lists = n_lists blocks of `stride` keys, of which
 * the first counts[i] are valid and sorted descending.  Writes the top
 * min(k, total) keys, sorted descending; returns that count. */
size_t cqs_hip_merge_keys(const uint64_t* lists, const uint32_t* counts, size_t n_lists, size_t stride,
                          size_t k, uint64_t* out_keys);

/* ---- search: host buffers, one keep-bitset per query ------------------------
 * `search_with_filter` for a block of `b` queries with a filter EACH: query i is filtered by
 * keep_bitsets + i * keep_stride_words (host; keep_stride_words >= ceil(len/32); bit layout
 * as keep_bitset above).  Per query the result is exactly the bytes of
 *   cqs_hip_index_search(idx, queries + i*dim, 1, dim, k, that bitset, mode, threshold, ...)
 * with every rule of that call: an all-pass bitset is the unfiltered search, a bitset that
 * keeps nothing gives count 0, the result length is capped at the kept rows, a non-finite
 * query gives count 0, a dimension mismatch gives counts 0 and CQS_HIP_OK, k > max_k is
 * CQS_HIP_ERR_INVALID.  out_rows / out_scores [b * k], out_counts [b].
 * The queries run in blocks of up to 32 as passes of up to 8 that share the HBM stream: a
 * pass reads a row when any of its queries keeps it.  With the bf16 / int8 shadow on, the
 * blocks go through it like unfiltered ones.  A row-sharded handle answers the queries one
 * by one through its filtered search (correct, not combined). */
int32_t cqs_hip_index_search_filtered(cqs_hip_index* idx, const float* queries, uint32_t b, uint32_t query_dim,
                                      uint32_t k, const uint32_t* keep_bitsets, uint64_t keep_stride_words,
                                      uint32_t mode, float threshold,
                                      uint64_t* out_rows, float* out_scores, uint32_t* out_counts);

/* ---- row tags: filtered search without a host bitset -------------
 * The predicate the reference sends with every filtered and hybrid query - chunk type in an include set, not in an
 * exclude set, language in a set; a chunk without metadata never passes (src/search/query.rs:860-900) - is a function of
 * two small integers per chunk.  Kept beside the rows in device memory, they let the caller send the allowed sets
 * (128 bytes) instead of evaluating a predicate n times and uploading n / 8 bytes: a kernel writes the keep-bitset the
 * scans already read, and the host cost of a filtered search stops depending on n.
 *
 * Tag: one uint32_t per row, read as four 8-bit fields, field f = (tag >> 8 f) & 255.  The library gives the fields no
 * meaning (the cqs shim: field 0 = chunk-type code, field 1 = language code, 255 = "no metadata", fields 2 and 3 spare).
 * Filter: `allow`, 32 host uint32_t words = four 256-bit sets; bit v of field f's set is bit v % 32 of word 8 f + v / 32.
 * A row is kept iff, for every field, the bit named by the row's field value is set.  A field the caller does not
 * constrain has all 256 bits set; a filter of 32 all-ones words keeps every row.
 *
 * set_tags: tags [m] (host) for the rows first_row .. first_row + m - 1 (GLOBAL row ids).  The tagged rows are always a
 * prefix [row_base, row_base + tagged_rows): a call may overwrite inside the prefix and / or extend it.  m == 0 changes
 * nothing.  CQS_HIP_ERR_INVALID, the handle untouched and the reason in last_error: a gap (first_row > row_base +
 * tagged_rows), a range past len, NULL tags with m > 0, a row-sharded handle (not built).  Takes the handle's mutex and
 * waits for the searches in flight, as extend does.  The column (4 B per row) is the library's own also on a borrowing
 * handle; it is made by the first call, sized like the corpus's allocation, and regrown with its contents when extend
 * regrows the corpus (no memory for that: the tags are dropped, tagged_rows is 0 and last_error says so).
 * extend leaves tagged_rows where it was: the new rows have no tag until set_tags covers them.  remove compacts the column
 * with the rows; tagged_rows drops by the number of removed rows that lay below it.  save / load do not persist tags: the
 * blob format is unchanged and a loaded handle has tagged_rows == 0.
 * tagged_rows: the leading rows that have a tag (0 on a row-sharded handle). */
int32_t  cqs_hip_index_set_tags(cqs_hip_index* idx, uint64_t first_row, const uint32_t* tags, uint64_t m);
uint64_t cqs_hip_index_tagged_rows(const cqs_hip_index* idx);
/* search_tagged: first the tag-specific checks, each CQS_HIP_ERR_INVALID without poisoning and with the reason in
 * last_error: NULL allow; a row-sharded handle (not built); tagged_rows < len ("tags cover X of N rows").  After them the
 * call returns, byte for byte, what cqs_hip_index_search returns for the same arguments with keep_bitset = the host
 * bitset of the same predicate, every rule of that call included: a dimension mismatch gives counts 0 and CQS_HIP_OK, a
 * non-finite query count 0, k > max_k is CQS_HIP_ERR_INVALID, an all-pass filter is the unfiltered search, a filter
 * that keeps nothing gives counts 0, k is capped at the kept rows, and the bf16 / int8 shadow is used where that call
 * would use it.  A filter of 32 all-ones words costs no device work and runs cqs_hip_index_search with a NULL bitset;
 * any other runs one small kernel on the handle's stream and waits for its exact kept-row count before the scan.
 * Concurrency: a call with b == 1 whose filter constrains something parks on the handle's combining queue, like a call
 * of cqs_hip_index_search with a keep_bitset: concurrent tagged callers with the same (k, mode, threshold) share passes
 * over the corpus in blocks of up to 32, each under its own filter (the block's bitsets are written by one kernel, see
 * search_tagged_multi), and each gets the bytes of its lone call.  Tagged callers form blocks of their own: they never
 * share one with unfiltered callers or callers with a keep_bitset (all-pass tagged calls ARE unfiltered searches and
 * combine as such).  If extend added rows without tags between parking and the pass, every caller of the block gets the
 * "tags cover X of N rows" refusal.  CQS_HIP_COMBINE=0 or CQS_HIP_COMBINE_TAGGED=0 (read at create) keeps tagged callers
 * off the queue; a call with b > 1 holds the handle's mutex throughout, like a filtered search with b > 1.
 * count_tagged: *out_kept = the rows `allow` keeps - the same kernel and count, no search (same checks). */
int32_t  cqs_hip_index_count_tagged(cqs_hip_index* idx, const uint32_t* allow, uint64_t* out_kept);
int32_t  cqs_hip_index_search_tagged(cqs_hip_index* idx, const float* queries, uint32_t b, uint32_t query_dim,
                                     uint32_t k, const uint32_t* allow, uint32_t mode, float threshold,
                                     uint64_t* out_rows, float* out_scores, uint32_t* out_counts);

/* search_tagged_multi: `b` queries with a tag filter EACH, allows [b * 32] (query i: the 32 words at allows + 32 i).  Per
 * query the result is exactly the bytes of
 *   cqs_hip_index_search_tagged(idx, queries + i*dim, 1, dim, k, allows + 32*i, mode, threshold, ...)
 * with every rule of that call per query: an all-pass filter is the unfiltered answer, a filter that keeps nothing gives
 * count 0, fewer kept rows than k returns them all, a non-finite query gives count 0 without disturbing its neighbours, a
 * dimension mismatch gives counts 0 and CQS_HIP_OK, k > max_k or a bad mode is CQS_HIP_ERR_INVALID.  The tag-specific
 * refusals of search_tagged come first (NULL allows; a row-sharded handle, not built; tagged_rows < len), each
 * CQS_HIP_ERR_INVALID without poisoning and with the reason in last_error.  The queries run in blocks of up to 32: one
 * kernel reads each row's tag once and writes the block's bitsets into the handle's bitset table (one small wait for
 * their exact counts), then the block runs as the blocks of cqs_hip_index_search_filtered run, through the bf16 / int8
 * shadow like those.  Holds the handle's mutex throughout; moves no combine counter.  out_rows / out_scores [b * k],
 * out_counts [b]. */
int32_t  cqs_hip_index_search_tagged_multi(cqs_hip_index* idx, const float* queries, uint32_t b, uint32_t query_dim,
                                           uint32_t k, const uint32_t* allows, uint32_t mode, float threshold,
                                           uint64_t* out_rows, float* out_scores, uint32_t* out_counts);

/* Combining-queue counters of a handle since it was made: passes the queue ran and the
 * queries they carried (queries / passes = mean callers per pass), unfiltered callers only.
 * Either pointer may be NULL.  Diagnostic; not part of the VectorIndex trait. */
void cqs_hip_index_combine_stats(const cqs_hip_index* idx, uint64_t* passes, uint64_t* queries);
/* The same two counters for the blocks of callers with a keep_bitset. */
void cqs_hip_index_combine_filter_stats(const cqs_hip_index* idx, uint64_t* passes, uint64_t* queries);
/* ... and for the blocks of single-query callers of cqs_hip_index_search_tagged. */
void cqs_hip_index_combine_tagged_stats(const cqs_hip_index* idx, uint64_t* passes, uint64_t* queries);

/* ---- bf16 shadow scan --------------------------------------------------------
 * Build (enable != 0) or free (enable == 0) a bf16 copy of the corpus that searches scan first.
 * Answers are unchanged byte for byte: the shadow picks candidates, their f32 rows are rescored with the
 * f32 scan's own arithmetic, and a query whose answer cannot be proven to be the f32 scan's is re-run on
 * it in the same call (device API: in the same stream, by f32 launches that return at once when every
 * query of the block was proven).  Costs n x dim x 2 B of device memory.
 * Built automatically by create / create_device / load of a single-device handle when the f32 corpus is at
 * least 1 GiB, dim % 8 == 0, dim <= 2048, no finite row has a component of magnitude >= 2^64, and the device
 * keeps max(4 GiB, 10 % of its memory) free afterwards; otherwise the handle is created on the f32 path and
 * last_error says why.  Environment, read at create / load: CQS_HIP_SCAN_BF16=0 never builds it
 * automatically, =1 builds it at any size (same dim, outlier and memory rules).
 * CQS_HIP_OK | CQS_HIP_ERR_INVALID (sharded handle, enable on a borrowed handle, dim % 8 != 0, dim > 2048, a
 * finite row with a component of magnitude >= 2^64; reason in last_error) | CQS_HIP_ERR_NOMEM.  The index
 * stays usable on the f32 path after any failure.  enable == 0 works on every single-device handle,
 * borrowed ones included (the per-handle opt-out); enable != 0 on a borrowed handle stays INVALID, whether
 * or not create built the shadow: its rows could have changed since create.  Enable is idempotent.
 * Scope: `cqs_hip_index_search` blocks that run as gemv passes (b <= 8, and the combining queue's exact
 * blocks) and `cqs_hip_index_search_device` blocks of b <= 8 (and of <= 32 queries where dim % 32 != 0);
 * matrix-core blocks, `cqs_hip_index_neighbors` and sharded handles are unchanged.  `extend` converts the
 * new rows (an outlier row there turns the shadow off); save does not persist it (load rebuilds it under
 * the rules above).
 * The int8 copy.  Beside the bf16 copy the handle may keep a second, int8 copy of the corpus (n x dim B plus 4 B per row:
 * with both, 0.75 B per f32 byte), which blocks of <= 4 queries at k <= 87 scan instead of the bf16 one: a quarter of the
 * f32 bytes, the same rescore, proof and f32 fallback, the same answers.  Every other block the shadow takes scans the bf16
 * copy.  It is built wherever a bf16 copy is built (create / create_device / load, and enable != 0 here) when
 * CQS_HIP_SCAN_I8 allows: unset = f32 corpus of at least 1 GiB, =0 never, =1 beside every bf16 copy; dim % 16 == 0, and
 * the free-memory rule holds with both copies.  Where only one copy fits, the bf16 one is kept (it serves every k) and
 * last_error says so.  enable == 0 frees both copies; extend, save and load treat it as they treat the bf16 copy. */
int32_t cqs_hip_index_set_bf16_scan(cqs_hip_index* idx, int32_t enable);
/* bytes of the shadow (0 = off); queries answered by the certified path; queries that fell back to the f32
 * scan (host and device-API searches; waits for the device-API searches in flight).  Any pointer may be NULL. */
void cqs_hip_index_bf16_stats(const cqs_hip_index* idx, uint64_t* bytes, uint64_t* certified, uint64_t* fallbacks);
/* The int8 copy's share: its bytes (codes and row scales; 0 = not built), and of the two counts above the queries whose
 * block scanned the int8 copy (bf16_stats counts every query once, whichever copy served it).  Any pointer may be NULL. */
void cqs_hip_index_i8_stats(const cqs_hip_index* idx, uint64_t* bytes, uint64_t* certified, uint64_t* fallbacks);

/* ---- profiling aid ---------------------------------------------------------
 * With timing enabled every search brackets its dominant scan kernel launch(es)
 * with a HIP event pair on the launch stream (up to 4096 pairs between reads).
 * cqs_hip_index_scan_time synchronises those events, returns how many searches
 * were bracketed and their summed scan time in milliseconds, and resets the
 * pool.  bench.py derives roofline.achieved from it. */
void    cqs_hip_index_set_timing(cqs_hip_index* idx, int32_t enable);
int32_t cqs_hip_index_scan_time(cqs_hip_index* idx, uint32_t* launches, double* total_ms);

/* ==== embed section ==========================================================
 * EmbeddingGemma-300m forward (Gemma3 text encoder, bidirectional, + mean pool + 2 dense):
 * replaces the ONNX Runtime session the reference runs inside `Embedder::embed_batch`
 * (src/embedder/core.rs:1091-1203: inputs `input_ids` / `attention_mask` i64 [B, L]
 * right-padded with pad_id 0 by `pad_2d_i64_from_encodings`, src/embedder/pooling.rs:40-57;
 * output `sentence_embedding` f32 [B, 768], L2-normalised afterwards by the caller,
 * core.rs:1196-1203).  Tokenisation, prefixes, batching by `embed_batch_size()` and the
 * query caches stay on the host exactly as in the reference.
 * Compute: bf16 operands on the matrix cores, f32 accumulation, f32 residual stream. */
typedef struct cqs_hip_embedder cqs_hip_embedder;

typedef struct cqs_hip_embed_config {
    uint32_t vocab_size;       /* 262144 */
    uint32_t hidden;           /* 768  (multiple of 256) */
    uint32_t layers;           /* 24 */
    uint32_t heads;            /* 3 */
    uint32_t kv_heads;         /* 1   (heads / kv_heads <= 4) */
    uint32_t head_dim;         /* 256 (only value supported) */
    uint32_t intermediate;     /* 1152 (multiple of 64) */
    uint32_t dense_hidden;     /* 3072 (multiple of 128) */
    uint32_t sliding_window;   /* 512: config value; the bidirectional mask is |q-k| < window/2 + 1 */
    uint32_t sliding_pattern;  /* 6: layer i is full attention iff (i+1) % pattern == 0 */
    uint32_t max_seq;          /* 2048 (src/embedder/models.rs:455-470) */
    float rms_eps;             /* 1e-6 */
    float rope_theta_global;   /* 1e6 */
    float rope_theta_local;    /* 1e4 */
    float query_pre_attn_scalar; /* 256 */
} cqs_hip_embed_config;

/* Fills *cfg with the EmbeddingGemma-300m geometry (`ModelConfig::embeddinggemma_300m`,
 * src/embedder/models.rs:455-470; dimensions from the public model card). */
void cqs_hip_embed_config_default(cqs_hip_embed_config* cfg);

/* Lifecycle: create (empty) -> set_tensor for every weight -> finalize -> embed* -> destroy.
 * Tensor names are the Hugging Face Gemma3TextModel names (`embed_tokens.weight`,
 * `layers.N.self_attn.q_proj.weight`, ..., `norm.weight`) plus `dense1.weight` [dense_hidden, hidden]
 * and `dense2.weight` [hidden, dense_hidden]; data is f32 row-major and is converted to bf16
 * (matrices) or kept f32 (norm weights) on the device. */
int32_t cqs_hip_embedder_create(const cqs_hip_embed_config* cfg, int32_t device, cqs_hip_embedder** out);
int32_t cqs_hip_embedder_set_tensor(cqs_hip_embedder* e, const char* name, const float* data, uint64_t count);
int32_t cqs_hip_embedder_finalize(cqs_hip_embedder* e);
/* Loader replacing `create_session(model_path, ..)` (src/embedder/provider.rs:349-447).  Reads what the reference's
 * local-model hook holds (CQS_ONNX_DIR, src/embedder/download.rs:12-41): `<dir>/onnx/model.onnx` (structured layout,
 * src/embedder/models.rs:455-457) or `<dir>/model.onnx` (flat layout), with the external-data sidecar
 * `model.onnx_data` beside it (download.rs:82) - the float initialisers are parsed straight from the protobuf wire
 * format (no ONNX Runtime, no protobuf library): named parameters keep their names, `Linear` weights folded into
 * transposed MatMul initialisers are resolved through the consuming node's module path, the two Dense layers by
 * shape.  Without an ONNX file, a Hugging Face checkpoint directory is read instead: `model.safetensors`
 * (+ `2_Dense/model.safetensors`, `3_Dense/model.safetensors`, tensor `linear.weight`).  F32 / BF16 / F16 tensors. */
int32_t cqs_hip_embedder_load_dir(const char* model_dir, const cqs_hip_embed_config* cfg, int32_t device,
                                  cqs_hip_embedder** out);
void cqs_hip_embedder_destroy(cqs_hip_embedder* e);

uint32_t cqs_hip_embedder_dim(const cqs_hip_embedder* e);        /* `embedding_dim()` core.rs:961 */
uint32_t cqs_hip_embedder_max_seq(const cqs_hip_embedder* e);
int32_t  cqs_hip_embedder_poisoned(const cqs_hip_embedder* e);
size_t   cqs_hip_embedder_last_error(const cqs_hip_embedder* e, char* buf, size_t cap);

/* The `session.run` replacement.  input_ids / attention_mask: i64 [batch, seq_len], host; every
 * mask row must be 1...10...0 (right padding).  out: f32 [batch, hidden], host, NOT normalised
 * (the reference normalises per row right after, core.rs:1196-1203).  A row whose mask is all
 * zero yields a zero vector (src/embedder/pooling.rs:113-119).  Errors: bad mask / token id out
 * of range -> CQS_HIP_ERR_INVALID (`EmbedderError::InferenceFailed` in the shim). */
int32_t cqs_hip_embed(cqs_hip_embedder* e, const int64_t* input_ids, const int64_t* attention_mask,
                      uint32_t batch, uint32_t seq_len, float* out);
/* Asynchronous form of the same call, for the index pipeline (the embed stage is its bottleneck when the cache is
 * cold, src/cli/pipeline/embedding.rs:226-421): submit validates and packs the batch into pinned staging, enqueues
 * tables H2D + forward + D2H on one of the engine's two execution contexts (a HIP stream + activation scratch each;
 * consecutive tickets alternate, so two batches' kernel chains interleave on the device) and returns a ticket
 * without waiting; collect waits for that ticket and copies its [batch, hidden] rows out.  Up to 3 tickets may be in
 * flight: while the device runs batches i and i+1 the host packs batch i+2.  A 4th submit without a collect ->
 * CQS_HIP_ERR_INVALID.  Tickets may be collected in any order (and may finish out of order); results do not depend
 * on what else is in flight.  A slot is released only by collecting its ticket: a caller that gives up on a batch
 * (an error in a LATER submit, a cancelled index run) must still collect every ticket it holds - `out` = NULL
 * abandons one (waits for it, releases the slot, drops the rows).
 * submit_ragged takes the batch without padding: `tokens` = the sequences' ids back to back (i32), lens[b] = length
 * of sequence b (0 allowed -> zero vector) - what a length-sorted scheduler holds anyway. */
int32_t cqs_hip_embed_submit(cqs_hip_embedder* e, const int64_t* input_ids, const int64_t* attention_mask,
                             uint32_t batch, uint32_t seq_len, uint64_t* ticket);
int32_t cqs_hip_embed_submit_ragged(cqs_hip_embedder* e, const int32_t* tokens, const uint32_t* lens, uint32_t batch,
                                    uint64_t* ticket);
int32_t cqs_hip_embed_collect(cqs_hip_embedder* e, uint64_t ticket, float* out);
/* `Embedder::warm()` (src/embedder/core.rs:933-957): pay the first-call cost of the search-time forward before the
 * first real query.  One sequence of up to 128 tokens (`embed_query`) runs a kernel chain of its own, replayed from a
 * hipGraph kept per (token count, execution context); a graph is otherwise built the first time its length is seen
 * (eager chain + capture + instantiate on that query's clock).  warm builds and replays the graphs of every length
 * 1..max_tokens (clamped to what the search-time path serves).  Call it with no ticket in flight
 * (CQS_HIP_ERR_INVALID otherwise); it takes about a second for max_tokens = 128. */
int32_t cqs_hip_embedder_warm(cqs_hip_embedder* e, uint32_t max_tokens);
/* Search-time chain counters since the engine was made: graphs captured, captures that FAILED (that length runs its
 * chain eagerly from then on; the cause is in cqs_hip_embedder_last_error), graph replays, eager chain runs.  Any
 * pointer may be NULL.  Diagnostic: lets a caller (and the bench) see which path a query really took. */
void cqs_hip_embedder_query_graph_stats(const cqs_hip_embedder* e, uint64_t* captured, uint64_t* failed,
                                        uint64_t* replays, uint64_t* eager);
/* `normalize_l2` (src/embedder/pooling.rs:60-67) applied to each row of a host [n, dim] matrix, in place: f32
 * left-to-right sum of squares, scale by 1/sqrt when > 0, zero rows stay zero.  Host code (no device work). */
void cqs_hip_normalize_l2_rows(float* rows, uint64_t n, uint32_t dim);
/* Diagnostic twin: final-norm hidden states f32 [batch, seq_len, hidden] (zeros at padded positions). */
int32_t cqs_hip_embed_hidden(cqs_hip_embedder* e, const int64_t* input_ids, const int64_t* attention_mask,
                             uint32_t batch, uint32_t seq_len, float* out_hidden);
/* Milliseconds between the start and the end of the forward of the most recently COLLECTED batch (HIP events on its
 * stream; with other tickets in flight that interval includes the time it shared the device with them). */
float cqs_hip_embedder_last_ms(const cqs_hip_embedder* e);

/* ---- BERT-family auxiliary models ---------------------------------------------------------
 * The two other ONNX models of the reference reuse `create_session` (src/embedder/provider.rs) and are BERT
 * encoders with a small head.  One engine type, two heads:
 *   CQS_HIP_BERT_HEAD_MLM         SPLADE sparse encoder (naver/splade-cocondenser-ensembledistil: BERT-base masked-LM);
 *                                 replaces the `session.run` of `SpladeEncoder::encode` / `encode_batch`
 *                                 (src/splade/mod.rs:595-760, :774-1075)
 *   CQS_HIP_BERT_HEAD_CLASSIFIER  cross-encoder reranker (cross-encoder/ms-marco-MiniLM-L-6-v2); replaces the
 *                                 `session.run` of `Reranker::compute_scores_opt` (src/reranker.rs:343-533)
 *   CQS_HIP_BERT_HEAD_NONE        the BERT-family EMBEDDER presets of the `Embedder` seam (e5-base, v9-200k: BERT-base;
 *                                 bge-large, bge-large-ft: BERT-large; src/embedder/models.rs:346-405): replaces
 *                                 `session.run` + `mean_pool` / `cls_pool` (src/embedder/pooling.rs:87-128)
 * The tokenizer stays on the host as in the reference; token ids come in packed (sequences back to back + lengths).
 * Weights are handed over by HF tensor name (set_tensor, f32, copied) and frozen by finalize.  Calls on one engine
 * are serialised by an internal mutex.  Geometry limits: hidden a multiple of 128 (<= 1024), head dim 32 or 64, and
 * hidden, 3 x hidden and intermediate each a multiple of 192, 256 or 320 (a GEMM tile width). */
typedef struct cqs_hip_bert cqs_hip_bert;
enum { CQS_HIP_BERT_HEAD_MLM = 0, CQS_HIP_BERT_HEAD_CLASSIFIER = 1, CQS_HIP_BERT_HEAD_NONE = 2 /* encoder only: the BERT-family embedders */ };
typedef struct cqs_hip_bert_config {
    uint32_t vocab_size, hidden, layers, heads, intermediate, max_pos, type_vocab;
    uint32_t num_labels;   /* classifier head: outputs per sequence (1..16) */
    uint32_t head;         /* CQS_HIP_BERT_HEAD_* */
    float ln_eps;
} cqs_hip_bert_config;
/* Presets: head = MLM -> BERT-base / vocab 30522 (src/splade/mod.rs:120-150); head = CLASSIFIER -> MiniLM-L6-H384, one
 * label (src/reranker.rs:7,35); head = NONE -> BERT-base (e5-base / v9-200k; for bge-large set hidden 1024, layers 24,
 * heads 16, intermediate 4096: src/embedder/models.rs:346-405). */
int32_t cqs_hip_bert_config_default(uint32_t head, cqs_hip_bert_config* out);
int32_t cqs_hip_bert_create(const cqs_hip_bert_config* cfg, int32_t device, cqs_hip_bert** out);
/* name: the Hugging Face tensor name, with or without the leading `bert.` (e.g.
 * `encoder.layer.3.attention.self.query.weight`, `cls.predictions.transform.dense.bias`, `cls.predictions.bias`,
 * `pooler.dense.weight`, `classifier.weight`); the MLM decoder is tied to `embeddings.word_embeddings.weight`. */
int32_t cqs_hip_bert_set_tensor(cqs_hip_bert* e, const char* name, const float* data, uint64_t count);
int32_t cqs_hip_bert_finalize(cqs_hip_bert* e);
/* create + weights from a model directory + finalize: `{dir}/onnx/model.onnx` or `{dir}/model.onnx` (+ external data;
 * the bundle layout of src/reranker.rs:548-556 and src/splade/mod.rs:433-460), else a Hugging Face checkpoint
 * (`{dir}/model.safetensors`).  cfg gives the geometry (config.json stays the host's business,
 * src/splade/mod.rs:125-150). */
int32_t cqs_hip_bert_load_dir(const char* model_dir, const cqs_hip_bert_config* cfg, int32_t device, cqs_hip_bert** out);
void    cqs_hip_bert_destroy(cqs_hip_bert* e);
/* SPLADE: tokens = the sequences' ids back to back, lens[b] = tokens of sequence b (0 allowed: an all-zero row).
 * out_dense [batch, vocab] f32 = ln(1 + max(0, max over the sequence's tokens of the masked-LM logits)): the
 * pre-pooled `sparse_vector` output form (src/splade/mod.rs:960-978); the caller keeps (id, weight) with
 * weight > threshold, ascending id (src/splade/mod.rs:1049-1062).  The maximum is folded with a strict `>` from -inf
 * (src/splade/mod.rs:1033-1043). */
int32_t cqs_hip_splade_encode(cqs_hip_bert* e, const int32_t* tokens, const uint32_t* lens, uint32_t batch, float* out_dense);
/* The same with that threshold filter done on the device (no [batch, vocab] transfer, no host pass over it): sequence
 * b's (id, weight) pairs with weight > threshold, ascending id, at out_ids / out_weights [b * cap ..]; out_counts[b] =
 * how many passed - above `cap` the row was cut off after its first `cap` entries and the caller takes that sequence
 * through cqs_hip_splade_encode instead (trained models keep 100-300 entries, src/splade/mod.rs:44). */
int32_t cqs_hip_splade_encode_sparse(cqs_hip_bert* e, const int32_t* tokens, const uint32_t* lens, uint32_t batch,
                                     float threshold, uint32_t cap, uint32_t* out_ids, float* out_weights, uint32_t* out_counts);
/* Ticket form of the same (the index pipeline's SPLADE stage, src/splade/mod.rs:774-1075 called per batch): submit packs
 * the batch into pinned staging and enqueues it on one of the engine's two execution contexts (consecutive tickets
 * alternate) without waiting; collect waits for that ticket.  Up to 3 tickets in flight; a ticket is released only by
 * collecting it (out_ids = NULL abandons it).  The blocking call above is submit + collect. */
int32_t cqs_hip_splade_submit_sparse(cqs_hip_bert* e, const int32_t* tokens, const uint32_t* lens, uint32_t batch,
                                     float threshold, uint32_t cap, uint64_t* ticket);
int32_t cqs_hip_splade_collect_sparse(cqs_hip_bert* e, uint64_t ticket, uint32_t* out_ids, float* out_weights,
                                      uint32_t* out_counts);
/* Reranker: (query, passage) pairs as ids + token type ids (NULL = all zero), packed like the above; every sequence
 * non-empty.  out_logits [batch, num_labels] f32; score = sigmoid(out_logits[b * num_labels]) (src/reranker.rs:516-518). */
int32_t cqs_hip_rerank_logits(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens,
                              uint32_t batch, float* out_logits);
/* Embedder presets (head = NONE): pooled sentence vectors f32 [batch, hidden], NOT normalised (the caller applies
 * `normalize_l2`, src/embedder/core.rs:1196-1203).  pooling: 0 = mean over the sequence's tokens (`PoolingStrategy::Mean`,
 * an empty sequence gives zeros), 1 = first token (`PoolingStrategy::Cls`).  type_ids NULL = all zero. */
int32_t cqs_hip_bert_embed(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens,
                           uint32_t batch, uint32_t pooling, float* out);
/* Ticket form (the index pipeline's embed stage with a BERT-family preset, src/cli/pipeline/embedding.rs:226-421):
 * as cqs_hip_embed_submit / _collect; out = NULL abandons the ticket. */
int32_t cqs_hip_bert_embed_submit(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens,
                                  uint32_t batch, uint32_t pooling, uint64_t* ticket);
int32_t cqs_hip_bert_embed_collect(cqs_hip_bert* e, uint64_t ticket, float* out);
/* Diagnostic: final encoder hidden states of the packed tokens, f32 [sum(lens), hidden]. */
int32_t cqs_hip_bert_hidden(cqs_hip_bert* e, const int32_t* tokens, const int32_t* type_ids, const uint32_t* lens,
                            uint32_t batch, float* out_hidden);
uint32_t cqs_hip_bert_vocab(const cqs_hip_bert* e);
int32_t  cqs_hip_bert_poisoned(const cqs_hip_bert* e);
size_t   cqs_hip_bert_last_error(cqs_hip_bert* e, char* buf, size_t cap);

/* ---- sparse index: the SPLADE retrieval leg (`SpladeIndex`, src/splade/index.rs:177-306) ---------------------------
 * The consumer of the sparse vectors cqs_hip_splade_encode_sparse produces: `search_hybrid_inner` asks it for
 * candidate_count_for(limit) >= 500 chunks per query next to the dense leg (src/search/query.rs:898-901) and fuses the
 * two lists itself (:909-1010, stays in Rust).  Replaces the in-memory `postings: HashMap<u32, Vec<(usize, f32)>>` +
 * `HashMap<usize, f32>` accumulation by an HBM-resident posting array and one accumulate launch + the dense index's exact
 * select.  Scores are BIT-IDENTICAL to the reference's: every chunk's sum is built as 0.0 + qw*dw + ... in query-term order,
 * then posting order, f32 multiply and f32 add (index.rs:248-258).
 *
 * create (`SpladeIndex::build`, index.rs:191-212): the n chunks' sparse vectors in chunk-index order as a forward CSR -
 * doc_off [n + 1] (doc_off[0] = 0), tokens / weights [doc_off[n]]; any u32 token id, repeated tokens inside a document
 * kept (each occurrence is its own posting, as in the reference).  id_rank: NULL, or n u32 - a permutation of 0..n-1,
 * id_rank[i] = how many chunk ids sort before chunk i's id (bytes; equal ids in chunk order): equal scores are then
 * ordered by id like `BoundedScoreHeap` (src/search/scoring/candidate.rs:299-334); NULL orders them by chunk index.
 * The one weight bit pattern 0xFFFFFFFF (a NaN) is refused (-> CQS_HIP_ERR_INVALID); every other f32 is accepted.
 * n < 2^32 - 1024. */
typedef struct cqs_hip_sparse_index cqs_hip_sparse_index;
int32_t cqs_hip_sparse_index_create(const uint64_t* doc_off, const uint32_t* tokens, const float* weights, uint64_t n,
                                    const uint32_t* id_rank, int32_t device, cqs_hip_sparse_index** out);
/* The same index from the reference's OWN in-memory form - `postings: HashMap<u32, Vec<(usize, f32)>>` (index.rs:177-187), e.g.
 * right after `SpladeIndex::load` read the persisted file (index.rs:677-1072): token_ids [n_tokens] distinct keys in any order,
 * list_off [n_tokens + 1], post_chunks / post_weights [list_off[n_tokens]] = every key's list in its stored order.  Postings that
 * name a chunk >= n are dropped (the search skips them, index.rs:252); a list need not be ascending (postings of ONE chunk keep
 * their order, all the sums depend on); a key given twice -> CQS_HIP_ERR_INVALID.  Searches give the same bits as an index
 * built by cqs_hip_sparse_index_create from the documents. */
int32_t cqs_hip_sparse_index_create_inverted(const uint32_t* token_ids, const uint64_t* list_off, const uint32_t* post_chunks,
                                             const float* post_weights, uint64_t n_tokens, uint64_t n, const uint32_t* id_rank,
                                             int32_t device, cqs_hip_sparse_index** out);
/* Persistence - the role of `SpladeIndex::save` / `load` / `load_or_build` (index.rs:346-1107): a restart skips the rebuild; the
 * file is tied to the store's `splade_generation` counter (bumped on every write to `sparse_vectors`).  OWN format (the
 * reference's blake3-checksummed `splade.index.bin` is neither read nor written): 64-byte header {magic "CQSHIPS1", version,
 * ranked, chunks, tokens, postings, generation, checksum} + token ids, list offsets, postings and the id order, written to
 * `<path>.tmp`, fsync'ed and renamed over `path`.  load: wrong magic / version / generation / chunk count (expected_chunks
 * 0 = any) / size / checksum / structure -> CQS_HIP_ERR_INVALID, *out stays NULL and the caller builds from the rows
 * (index.rs:1073-1107); a missing file likewise. */
int32_t cqs_hip_sparse_index_save(cqs_hip_sparse_index* idx, const char* path, uint64_t generation, uint64_t* out_checksum);
int32_t cqs_hip_sparse_index_load(const char* path, uint64_t expected_chunks, uint64_t generation, int32_t device,
                                  cqs_hip_sparse_index** out);
void     cqs_hip_sparse_index_destroy(cqs_hip_sparse_index* idx);
uint64_t cqs_hip_sparse_index_len(const cqs_hip_sparse_index* idx);            /* index.rs:294-296 */
uint64_t cqs_hip_sparse_index_unique_tokens(const cqs_hip_sparse_index* idx);  /* index.rs:304-306 */
uint64_t cqs_hip_sparse_index_postings(const cqs_hip_sparse_index* idx);
/* `search_with_filter` (index.rs:223-290; `search` = keep_bitset NULL, :214-216).  The query's (token, weight) terms in
 * the caller's order; keep_bitset: NULL or ceil(n / 32) host words, bit i of word i / 32 = the filter predicate on chunk i
 * (evaluated by the caller on the chunk's id, as `search_hybrid_inner` builds its predicate, src/search/query.rs:861-877).
 * Writes min(k, scored chunks) entries, best first: out_chunks = chunk indices (positions in the build order = id_map
 * indices), out_scores = the raw dot products.  Chunks no posting of the query reaches are not candidates (even at score
 * 0 others may be); non-finite scores are dropped (`would_accept`, candidate.rs:245-247); an empty query, an empty index or
 * k = 0 give *out_count = 0 (index.rs:237-239).  k <= CQS_HIP_MAX_K. */
int32_t cqs_hip_sparse_index_search(cqs_hip_sparse_index* idx, const uint32_t* q_tokens, const float* q_weights, uint32_t n_terms,
                                    uint32_t k, const uint32_t* keep_bitset, uint64_t* out_chunks, float* out_scores,
                                    uint32_t* out_count);
/* The same for a batch of b <= 64 queries in ONE pair of launches (evaluation runs, or a caller that gathers its clients'
 * queries): query q's terms are q_tokens / q_weights [q_off[q], q_off[q + 1]) (q_off [b + 1], ascending); one optional filter for
 * all; out_chunks / out_scores [b][k] (row q holds out_counts[q] entries), out_counts [b].  Every query's answer is the one
 * cqs_hip_sparse_index_search gives for it alone, bit for bit. */
int32_t cqs_hip_sparse_index_search_batch(cqs_hip_sparse_index* idx, const uint64_t* q_off, const uint32_t* q_tokens,
                                          const float* q_weights, uint32_t b, uint32_t k, const uint32_t* keep_bitset,
                                          uint64_t* out_chunks, float* out_scores, uint32_t* out_counts);
/* In-place updates: the sparse leg follows cqs_hip_index_remove / cqs_hip_index_extend of the dense leg
 * without a rebuild from every document's sparse vector.  After either call the handle is indistinguishable from one
 * freshly created from the resulting documents with the resulting id order: same len / unique_tokens / postings, the
 * same bytes from every search, the same file from save.  Both take the handle's mutex: a concurrent search sees the old
 * index or the new one.  INVALID (see last_error) and NOMEM leave the index untouched; a device error poisons the handle.
 *
 * remove: chunks leave the index in place.  `chunks` are chunk indices (what search returns), any order, a duplicate
 * counts once; an index >= len is INVALID.  The survivors keep their relative order, in chunk index and in rank, and are
 * renumbered densely; a token whose every posting belonged to removed chunks leaves the token table. */
int32_t cqs_hip_sparse_index_remove(cqs_hip_sparse_index* idx, const uint64_t* chunks, uint64_t m, uint64_t* out_removed);
/* extend: n_new documents join the index as chunks len .. len + n_new - 1.  doc_off / tokens / weights as in create.
 * new_rank[i] = the FINAL position of new chunk i in ascending id order of the grown index (distinct, < len + n_new);
 * the existing chunks keep their relative order in the remaining positions.  NULL: the new chunks rank after every
 * existing one, in the order given.  On a handle created without id_rank, new_rank must be NULL. */
int32_t cqs_hip_sparse_index_extend(cqs_hip_sparse_index* idx, const uint64_t* doc_off, const uint32_t* tokens,
                                    const float* weights, uint64_t n_new, const uint32_t* new_rank);
/* Chunk tags (tags, filter and rules as cqs_hip_index_set_tags / _search_tagged above): one uint32_t per
 * chunk INDEX (what keep_bitset is indexed by, whatever the id order).  The tagged chunks are a prefix [0, tagged_chunks);
 * set_tags overwrites inside it and / or extends it; a gap, a range past len and NULL tags with m > 0 are INVALID with
 * the handle untouched.  extend leaves the prefix alone; remove renumbers the tags with the chunks and drops the prefix
 * by the number of removed chunks below it; save / load do not persist tags.
 * search_tagged: INVALID for a NULL allow or tagged_chunks < len; otherwise the bytes of cqs_hip_sparse_index_search with
 * the host bitset of the same predicate (an all-ones filter: the keep_bitset == NULL call).  The bitset is written on the
 * device in front of the scoring launch; the call has no extra wait.  The batch call has no tagged twin. */
int32_t  cqs_hip_sparse_index_set_tags(cqs_hip_sparse_index* idx, uint64_t first_chunk, const uint32_t* tags, uint64_t m);
uint64_t cqs_hip_sparse_index_tagged_chunks(const cqs_hip_sparse_index* idx);
int32_t  cqs_hip_sparse_index_search_tagged(cqs_hip_sparse_index* idx, const uint32_t* q_tokens, const float* q_weights,
                                            uint32_t n_terms, uint32_t k, const uint32_t* allow, uint64_t* out_chunks,
                                            float* out_scores, uint32_t* out_count);
/* Concurrent callers: unfiltered single-query cqs_hip_sparse_index_search calls on one handle are combined into shared
 * batches like the dense index's (CQS_HIP_COMBINE=0 / CQS_HIP_COMBINE_WAIT_US, read at create); every caller gets the bits
 * its own call would have produced.  Counters since the handle was made: batches run through the queue and the queries they
 * carried.  Either pointer may be NULL.  Diagnostic. */
void cqs_hip_sparse_index_combine_stats(const cqs_hip_sparse_index* idx, uint64_t* passes, uint64_t* queries);
/* Profiling aid: device time of the last search's accumulate launch (HIP events on its stream) and the postings it read
 * (the sum of its terms' list lengths: 8 bytes each = the launch's algorithmic bytes, with 4 bytes per chunk of score row).
 * Searches are bracketed by the two events only from the first call with a non-NULL accumulate_ms on (round 5: a caller
 * that never asks does not pay for them); that first call reports 0 ms for the search before it. */
int32_t cqs_hip_sparse_index_last_search(const cqs_hip_sparse_index* idx, float* accumulate_ms, uint64_t* touched_postings);
int32_t cqs_hip_sparse_index_poisoned(const cqs_hip_sparse_index* idx);
size_t  cqs_hip_sparse_index_last_error(const cqs_hip_sparse_index* idx, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* CQS_HIP_H */
