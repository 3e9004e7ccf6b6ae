//! MI355X exact GPU index for cqs: `impl VectorIndex` / `impl IndexBackend` over
//! libcqs_hip.so (C ABI: include/cqs_hip.h).
//!
//! Drop-in location: `src/hip.rs`, `#[cfg(feature = "hip-index")] pub mod hip;` in
//! `src/lib.rs`, one row in the backend table (`src/index.rs:338-345`):
//!
//! ```ignore
//! crate::hip::HipBackend, cfg(feature = "hip-index");
//! ```
//!
//! Multi-GPU: `CQS_HIP_DEVICES=0,1,..` makes the ONE daemon process shard the corpus over those devices through
//! `cqs_hip_index_create_sharded` (per-device scan, RCCL all-gather of candidates, host merge inside the library); the
//! trait surface does not change.  Persistence: `index.hipflat` + `index.hipflat.meta`, persisted-first open.
//!
//! Shape follows `CagraIndex` (src/cagra.rs:255-277): the index owns `id_map`
//! (row -> chunk id, rowid order); the device side is addressed by row number.
//! Conventions kept from the reference (src/cagra.rs:445-470, 543-626, 1715-1800):
//! `search` never panics and never returns an error for device trouble - it logs and
//! returns an empty Vec; `try_open` returns `Ok(None)` to fall through to the next
//! backend and `Err` only for store errors.

use std::os::raw::c_char;
use std::sync::atomic::{AtomicBool, Ordering};

use crate::embedder::Embedding;
use crate::hip_tags::TagCodes;
use crate::parser::{ChunkType, Language};
use crate::index::{BackendContext, DistanceMetric, IndexBackend, IndexResult, VectorIndex};
use crate::store::{ClearHnswDirty, Store, StoreError};

// ---- C ABI (include/cqs_hip.h) ------------------------------------------------
#[repr(C)]
struct CqsHipIndex {
    _private: [u8; 0],
}

const CQS_HIP_OK: i32 = 0;
const CQS_HIP_METRIC_COSINE: u32 = 0;
const CQS_HIP_METRIC_DOT: u32 = 1;
const CQS_HIP_MODE_RAW: u32 = 0;

#[link(name = "cqs_hip")]
extern "C" {
    fn cqs_hip_device_count() -> i32;
    fn cqs_hip_device_mem(device: i32, free_bytes: *mut u64, total_bytes: *mut u64) -> i32;
    fn cqs_hip_index_create(
        rows: *const f32,
        n: u64,
        dim: u32,
        metric: u32,
        device: i32,
        row_base: u64,
        out: *mut *mut CqsHipIndex,
    ) -> i32;
    // ONE process, several GPUs (north_star): rows cut over `devices`, RCCL all-gather of per-shard candidates inside
    // the library, host merge; every other entry point takes the returned handle unchanged
    fn cqs_hip_index_create_sharded(
        rows: *const f32,
        n: u64,
        dim: u32,
        metric: u32,
        devices: *const i32,
        n_devices: u32,
        row_base: u64,
        out: *mut *mut CqsHipIndex,
    ) -> i32;
    fn cqs_hip_index_load_sharded(path: *const c_char, expected_dim: u32, expected_rows: u64, devices: *const i32,
                                  n_devices: u32, row_base: u64, out: *mut *mut CqsHipIndex) -> i32;
    fn cqs_hip_index_neighbors(idx: *mut CqsHipIndex, target_row: u64, limit: u32, out_rows: *mut u64,
                               out_scores: *mut f32, out_count: *mut u32) -> i32;
    fn cqs_hip_index_knn_graph(idx: *mut CqsHipIndex, first_row: u64, m: u64, limit: u32, out_rows: *mut u64,
                               out_scores: *mut f32, out_counts: *mut u32) -> i32;
    // `cqs index --umap` on the resident corpus: the kNN graph, then the layout handle (its own opaque type on the C side;
    // this one call is all the shim needs of it), run to its end
    fn cqs_hip_index_umap_project(idx: *mut CqsHipIndex, n_neighbors: u32, n_epochs: u32, seed: u64, out_xy: *mut f32) -> i32;
    fn cqs_hip_index_pca(idx: *mut CqsHipIndex, n_components: u32, n_passes: u32, seed: u64, out_mean: *mut f32,
                         out_axes: *mut f32, out_variance: *mut f32, out_total_variance: *mut f32) -> i32;
    fn cqs_hip_index_pca_project(idx: *mut CqsHipIndex, mean: *const f32, axes: *const f32, n_components: u32, first_row: u64,
                                 m: u64, out: *mut f32) -> i32;
    fn cqs_hip_index_umap_project_init(idx: *mut CqsHipIndex, n_neighbors: u32, n_epochs: u32, seed: u64, init: u32,
                                       out_xy: *mut f32) -> i32;
    // ... and coordinates for rows appended since, among the stored ones, which stay where they are
    fn cqs_hip_index_umap_transform(idx: *mut CqsHipIndex, n_anchors: u64, anchors_xy: *const f32, vectors: *const f32, m: u64,
                                    n_neighbors: u32, n_epochs: u32, seed: u64, out_xy: *mut f32) -> i32;
    // semantic diff of two resident indexes (src/diff.rs:172-215: full_cosine_similarity of matched pairs, the threshold)
    fn cqs_hip_index_diff(a: *mut CqsHipIndex, rows_a: *const u64, b: *mut CqsHipIndex, rows_b: *const u64, m: u64,
                          threshold: f32, out_sims: *mut f32, out_mod_pairs: *mut u64, out_mod_sims: *mut f32,
                          out_counts: *mut u64) -> i32;
    // cosine MMR over the resident rows (src/search/mmr.rs:59-126 with the stored rows' dot as `similarity`)
    fn cqs_hip_index_pairwise(idx: *mut CqsHipIndex, cand_rows: *const u64, m: u32, out: *mut f32) -> i32;
    fn cqs_hip_index_mmr(idx: *mut CqsHipIndex, cand_rows: *const u64, cand_scores: *const f32, m: u32, limit: u32,
                         lambda: f32, out_picks: *mut u32, out_count: *mut u32) -> i32;
    fn cqs_hip_index_metric(idx: *const CqsHipIndex) -> u32;
    fn cqs_hip_index_extend(idx: *mut CqsHipIndex, rows: *const f32, n_new: u64) -> i32;
    fn cqs_hip_index_remove(idx: *mut CqsHipIndex, rows: *const u64, m: u64, out_removed: *mut u64) -> i32;
    fn cqs_hip_index_update(idx: *mut CqsHipIndex, rows: *const u64, vectors: *const f32, m: u64, out_updated: *mut u64) -> i32;
    // persistence (the index.cagra + .meta analogue, src/cagra.rs:973-1157, 1174-1330): the blob is written /
    // validated by the library, the CagraMeta-style sidecar (magic, version, dim, chunk_count, id_map,
    // checksum, metric) by `HipIndex::save` / `HipIndex::load` below via serde_json like src/cagra.rs:1128-1147
    fn cqs_hip_index_save(idx: *mut CqsHipIndex, path: *const c_char, out_checksum: *mut u64) -> i32;
    fn cqs_hip_index_load(path: *const c_char, expected_dim: u32, expected_rows: u64, device: i32, row_base: u64,
                          out: *mut *mut CqsHipIndex) -> i32;
    fn cqs_hip_index_destroy(idx: *mut CqsHipIndex);
    fn cqs_hip_index_len(idx: *const CqsHipIndex) -> u64;
    fn cqs_hip_index_max_k(idx: *const CqsHipIndex) -> u32;
    fn cqs_hip_index_poisoned(idx: *const CqsHipIndex) -> i32;
    fn cqs_hip_index_last_error(idx: *const CqsHipIndex, buf: *mut c_char, cap: usize) -> usize;
    fn cqs_hip_index_set_bf16_scan(idx: *mut CqsHipIndex, enable: i32) -> i32;
    fn cqs_hip_index_bf16_stats(idx: *const CqsHipIndex, bytes: *mut u64, certified: *mut u64, fallbacks: *mut u64);
    fn cqs_hip_index_i8_stats(idx: *const CqsHipIndex, bytes: *mut u64, certified: *mut u64, fallbacks: *mut u64);
    fn cqs_hip_index_search(
        idx: *mut CqsHipIndex,
        queries: *const f32,
        b: u32,
        query_dim: u32,
        k: u32,
        keep_bitset: *const u32,
        mode: u32,
        threshold: f32,
        out_rows: *mut u64,
        out_scores: *mut f32,
        out_counts: *mut u32,
    ) -> i32;
    // a block of queries with a keep-bitset each: per query the bytes of the call above with b = 1
    fn cqs_hip_index_search_filtered(
        idx: *mut CqsHipIndex,
        queries: *const f32,
        b: u32,
        query_dim: u32,
        k: u32,
        keep_bitsets: *const u32,
        keep_stride_words: u64,
        mode: u32,
        threshold: f32,
        out_rows: *mut u64,
        out_scores: *mut f32,
        out_counts: *mut u32,
    ) -> i32;
    fn cqs_hip_index_combine_filter_stats(idx: *const CqsHipIndex, passes: *mut u64, queries: *mut u64);
    fn cqs_hip_index_combine_tagged_stats(idx: *const CqsHipIndex, passes: *mut u64, queries: *mut u64);
    fn cqs_hip_index_search_tagged_multi(
        idx: *mut CqsHipIndex,
        queries: *const f32,
        b: u32,
        query_dim: u32,
        k: u32,
        allows: *const u32,
        mode: u32,
        threshold: f32,
        out_rows: *mut u64,
        out_scores: *mut f32,
        out_counts: *mut u32,
    ) -> i32;
    // row tags (include/cqs_hip.h, "row tags"): one u32 per row beside the corpus, filtered search without a host bitset
    fn cqs_hip_index_set_tags(idx: *mut CqsHipIndex, first_row: u64, tags: *const u32, m: u64) -> i32;
    fn cqs_hip_index_tagged_rows(idx: *const CqsHipIndex) -> u64;
    fn cqs_hip_index_count_tagged(idx: *mut CqsHipIndex, allow: *const u32, out_kept: *mut u64) -> i32;
    fn cqs_hip_index_search_tagged(
        idx: *mut CqsHipIndex,
        queries: *const f32,
        b: u32,
        query_dim: u32,
        k: u32,
        allow: *const u32,
        mode: u32,
        threshold: f32,
        out_rows: *mut u64,
        out_scores: *mut f32,
        out_counts: *mut u32,
    ) -> i32;
}

/// Exact brute-force GPU index (HBM-resident `[n, dim]` f32 + top-k on device).
pub struct HipIndex {
    handle: *mut CqsHipIndex,
    /// row -> chunk id, rowid order (same role as `CagraIndex::id_map`, src/cagra.rs:266).
    id_map: Vec<Box<str>>,
    dim: usize,
    metric: DistanceMetric,
    /// Set when the C side reports a device failure; `is_poisoned()` makes the daemon
    /// rebuild the index (src/index.rs:203-205, src/cagra.rs:472-489).
    poisoned: AtomicBool,
    /// chunk id -> row, built by the first `mmr_rerank` (a pool names up to 1024 ids per query) and dropped by `extend` / `remove`.
    row_of: std::sync::OnceLock<std::collections::HashMap<Box<str>, u64>>,
    /// The codes behind the rows' tags (`set_chunk_meta`); `None`: no tags, `search_with_tags` builds the bitset.
    tag_codes: Option<TagCodes>,
}

// SAFETY: the handle serialises device access behind its own mutex (include/cqs_hip.h,
// "Threading"); `id_map` is immutable after construction.  Same argument as
// `unsafe impl Send/Sync for CagraIndex` (src/cagra.rs:823-830).
unsafe impl Send for HipIndex {}
unsafe impl Sync for HipIndex {}

impl Drop for HipIndex {
    fn drop(&mut self) {
        // destroy() synchronises the index's streams first (src/cagra.rs:289-302)
        unsafe { cqs_hip_index_destroy(self.handle) }
    }
}

/// Sidecar of the persisted blob: the `CagraMeta` of this backend (src/cagra.rs:973-997) - the blob itself holds
/// only rows, so the row -> chunk-id map, the store's chunk count at save time and the blob's checksum live here.
#[derive(serde::Serialize, serde::Deserialize)]
struct HipMeta {
    magic: String,
    version: u32,
    dim: usize,
    chunk_count: usize,
    id_map: Vec<String>,
    checksum: String,
    metric: String,
}

const HIP_META_MAGIC: &str = "cqs-hip-flat-meta";
const HIP_META_VERSION: u32 = 1;

/// `CQS_HIP_DEVICES=0,1,2,3`: shard the corpus over these GPUs inside this process; unset / empty = device 0.
pub fn devices_from_env() -> Vec<i32> {
    let parsed: Vec<i32> = std::env::var("CQS_HIP_DEVICES")
        .ok()
        .map(|v| v.split(',').filter_map(|t| t.trim().parse().ok()).collect())
        .unwrap_or_default();
    if parsed.is_empty() { vec![0] } else { parsed }
}

fn hip_persist_enabled() -> bool {
    // same switch shape as CQS_CAGRA_PERSIST (src/cagra.rs:1013-1021): on unless set to 0 / false / off
    !matches!(std::env::var("CQS_HIP_PERSIST").as_deref(), Ok("0") | Ok("false") | Ok("off"))
}

fn hip_bf16_scan_enabled() -> bool {
    // `1`: a bf16 shadow of the corpus at any size (n x dim x 2 B more device memory), same answers, about half the bytes per
    // search; the library already builds it unasked from a 1 GiB f32 corpus on
    matches!(std::env::var("CQS_HIP_SCAN_BF16").as_deref(), Ok("1"))
}

impl HipIndex {
    /// `CQS_HIP_SCAN_BF16=1`: make sure the bf16 shadow that searches scan first is built (answers unchanged byte for byte).
    /// The library reads the same variable at create / load and has usually built it already (unset: from a 1 GiB f32
    /// corpus on); enable is idempotent, so this call is then a no-op.  A handle that cannot take it (row-sharded,
    /// dim % 8 != 0, an outlier row, no memory) keeps searching on the f32 scan.
    fn enable_bf16_scan_from_env(&self) {
        if !hip_bf16_scan_enabled() {
            return;
        }
        let rc = unsafe { cqs_hip_index_set_bf16_scan(self.handle, 1) };
        if rc != CQS_HIP_OK {
            tracing::warn!(rc, error = %self.last_error(), "HIP bf16 shadow scan not enabled; searching the f32 rows");
        } else {
            let mut bytes = 0u64;
            unsafe { cqs_hip_index_bf16_stats(self.handle, &mut bytes, std::ptr::null_mut(), std::ptr::null_mut()) };
            let mut i8_bytes: u64 = 0;
            unsafe { cqs_hip_index_i8_stats(self.handle, &mut i8_bytes, std::ptr::null_mut(), std::ptr::null_mut()) };
            tracing::info!(bytes, i8_bytes, "HIP bf16 shadow scan enabled");
        }
    }

    /// `CagraIndex::gpu_available_for` analogue (src/cagra.rs:336-376): every listed device must exist and hold its
    /// shard (corpus / devices + score scratch headroom).
    pub fn gpu_available_for(n: usize, dim: usize, devices: &[i32]) -> bool {
        let count = unsafe { cqs_hip_device_count() };
        if count <= 0 || devices.is_empty() {
            return false;
        }
        // corpus + score/scratch headroom must fit HBM (288 GB on MI355X: no 2 GiB host cap,
        // unlike CQS_CAGRA_MAX_BYTES, src/cagra.rs:159-167)
        let per_shard = (n as u64).saturating_mul(dim as u64).saturating_mul(4).saturating_mul(5) / 4 / devices.len() as u64;
        devices.iter().all(|&d| {
            let (mut free, mut total) = (0u64, 0u64);
            d >= 0 && d < count && unsafe { cqs_hip_device_mem(d, &mut free, &mut total) } == CQS_HIP_OK && per_shard <= free
        })
    }

    /// `CagraIndex::build_from_flat` (src/cagra.rs:922-960).
    pub fn build_from_flat(
        id_map: Vec<String>,
        flat_data: Vec<f32>,
        dim: usize,
        metric: DistanceMetric,
        devices: &[i32],
    ) -> Result<Self, String> {
        if id_map.is_empty() || flat_data.len() != id_map.len() * dim || devices.is_empty() {
            return Err("HIP build: empty or misshapen dataset".into());
        }
        let mut handle: *mut CqsHipIndex = std::ptr::null_mut();
        let m = match metric {
            DistanceMetric::Cosine => CQS_HIP_METRIC_COSINE,
            DistanceMetric::DotProduct => CQS_HIP_METRIC_DOT,
        };
        let rc = unsafe {
            if devices.len() == 1 {
                cqs_hip_index_create(flat_data.as_ptr(), id_map.len() as u64, dim as u32, m, devices[0], 0, &mut handle)
            } else {
                cqs_hip_index_create_sharded(flat_data.as_ptr(), id_map.len() as u64, dim as u32, m, devices.as_ptr(),
                                             devices.len() as u32, 0, &mut handle)
            }
        };
        if rc != CQS_HIP_OK || handle.is_null() {
            return Err(format!("cqs_hip_index_create failed: {rc}"));
        }
        Ok(Self {
            handle,
            id_map: id_map.into_iter().map(String::into_boxed_str).collect(),
            dim,
            metric,
            poisoned: AtomicBool::new(false),
            row_of: std::sync::OnceLock::new(),
            tag_codes: None,
        })
    }

    /// Stream the store into a flat buffer (`build_from_store_with_metric`,
    /// src/cagra.rs:842-916).  Zero / non-finite rows are skipped exactly like
    /// `prepare_index_data` (src/hnsw/mod.rs:717-731) so `len()` and row->id agree
    /// with the HNSW backend.
    pub fn build_from_store<Mode>(store: &Store<Mode>, dim: usize, metric: DistanceMetric, devices: &[i32]) -> Result<Self, String> {
        let mut id_map: Vec<String> = Vec::new();
        let mut flat: Vec<f32> = Vec::new();
        let batch = crate::limits::dim_scaled_batch(10_000, dim, 500, 50_000);
        for batch_result in store.embedding_batches(batch) {
            let batch = batch_result.map_err(|e| format!("Failed to fetch batch: {e}"))?;
            for (chunk_id, embedding) in batch {
                let v = embedding.as_slice();
                if v.len() != dim {
                    return Err(format!("dimension mismatch: expected {dim}, got {}", v.len()));
                }
                if !v.iter().any(|x| *x != 0.0) || v.iter().any(|x| !x.is_finite()) {
                    tracing::warn!(chunk_id = %chunk_id, "Skipping zero / non-finite embedding");
                    continue;
                }
                id_map.push(chunk_id);
                flat.extend_from_slice(v);
            }
        }
        Self::build_from_flat(id_map, flat, dim, metric, devices)
    }

    /// Incremental add (the contract `tiered.rs` exposes, src/tiered.rs:1-43).
    pub fn extend(&mut self, ids: Vec<String>, rows: &[f32]) -> Result<(), String> {
        if rows.len() != ids.len() * self.dim {
            return Err("HIP extend: misshapen rows".into());
        }
        let rc = unsafe { cqs_hip_index_extend(self.handle, rows.as_ptr(), ids.len() as u64) };
        if rc != CQS_HIP_OK {
            return Err(self.last_error());
        }
        self.id_map.extend(ids.into_iter().map(String::into_boxed_str));
        self.row_of = std::sync::OnceLock::new();
        Ok(())
    }

    /// Tag every row with its (chunk type, language) codes from `Store::chunk_type_language_map` - call it once after the
    /// index is opened (built, loaded or extended: tags are not persisted, and `extend` leaves the new rows without one).
    /// From then on `search_with_tags` filters on the device.  Returns false, and leaves the index on the host-bitset
    /// path, when a field would need more than 255 codes or the library refuses the tags.
    pub fn set_chunk_meta(&mut self, meta: &std::collections::HashMap<String, (ChunkType, Language)>) -> bool {
        self.tag_codes = None;
        let Some(codes) = TagCodes::assign(meta) else {
            tracing::info!("HIP index: more than 255 chunk types or languages, filtered searches keep the host bitset");
            return false;
        };
        let tags: Vec<u32> = self.id_map.iter().map(|id| codes.tag_of(id, meta)).collect();
        // (handles made here have row_base 0)
        let rc = unsafe { cqs_hip_index_set_tags(self.handle, 0, tags.as_ptr(), tags.len() as u64) };
        if rc != CQS_HIP_OK {
            tracing::warn!(rc, error = %self.last_error(), "HIP index: set_tags refused, filtered searches keep the host bitset");
            return false;
        }
        self.tag_codes = Some(codes);
        true
    }

    /// `search_with_filter` for the predicate `search_hybrid_inner` builds (src/search/query.rs:860-877), without the
    /// loop over every chunk id: the allowed sets go to the library, which writes the bitset on the device
    /// (`cqs_hip_index_search_tagged`; same results as the bitset path, byte for byte).  Falls back to
    /// `search_with_filter` with that predicate when the index has no tags (`set_chunk_meta` not called, or refused) or
    /// they do not cover it (rows added since).  `meta` is only looked at on the fallback.
    pub fn search_with_tags(
        &self,
        query: &Embedding,
        k: usize,
        include: Option<&[ChunkType]>,
        exclude: Option<&[ChunkType]>,
        languages: Option<&[Language]>,
        meta: &std::collections::HashMap<String, (ChunkType, Language)>,
    ) -> Vec<IndexResult> {
        if self.id_map.is_empty() || k == 0 || query.len() != self.dim {
            return Vec::new();
        }
        let covered = unsafe { cqs_hip_index_tagged_rows(self.handle) } as usize == self.id_map.len();
        let Some(codes) = self.tag_codes.as_ref().filter(|_| covered) else {
            let predicate = |id: &str| -> bool {
                if include.is_none() && exclude.is_none() && languages.is_none() {
                    return true;
                }
                meta.get(id).is_some_and(|(ct, lang)| {
                    include.is_none_or(|t| t.contains(ct)) && exclude.is_none_or(|t| !t.contains(ct)) && languages.is_none_or(|l| l.contains(lang))
                })
            };
            return self.search_with_filter(query, k, &predicate);
        };
        let allow = codes.allow(include, exclude, languages);
        let k = k.min(unsafe { cqs_hip_index_max_k(self.handle) } as usize);
        let mut rows = vec![0u64; k];
        let mut scores = vec![0f32; k];
        let mut count = 0u32;
        let rc = unsafe {
            cqs_hip_index_search_tagged(self.handle, query.as_slice().as_ptr(), 1, query.len() as u32, k as u32, allow.as_ptr(),
                                        CQS_HIP_MODE_RAW, 0.0, rows.as_mut_ptr(), scores.as_mut_ptr(), &mut count)
        };
        if rc != CQS_HIP_OK {
            if unsafe { cqs_hip_index_poisoned(self.handle) } != 0 {
                self.poisoned.store(true, Ordering::Release);
            }
            tracing::error!(error = %self.last_error(), rc, "HIP tagged search failed");
            return Vec::new();
        }
        (0..count as usize)
            .filter_map(|i| {
                self.id_map.get(rows[i] as usize).map(|id| IndexResult {
                    id: id.to_string(),
                    score: match self.metric {
                        DistanceMetric::Cosine => scores[i].min(1.0),
                        DistanceMetric::DotProduct => scores[i],
                    },
                })
            })
            .collect()
    }

    /// The rows a tag filter keeps (what the reference logs as `included`, src/cagra.rs:758); `None` without tags.
    pub fn count_with_tags(&self, include: Option<&[ChunkType]>, exclude: Option<&[ChunkType]>, languages: Option<&[Language]>) -> Option<u64> {
        let allow = self.tag_codes.as_ref()?.allow(include, exclude, languages);
        let mut kept = 0u64;
        (unsafe { cqs_hip_index_count_tagged(self.handle, allow.as_ptr(), &mut kept) } == CQS_HIP_OK).then_some(kept)
    }

    /// Delete chunks in place (the tiered backend's other purpose, "to clean orphaned vectors", src/tiered.rs:13-17):
    /// the library compacts the resident rows, `id_map` loses the same positions in the same order.  Ids the index
    /// does not hold are ignored (the watch loop also deletes chunks that were never indexed).  Returns the number
    /// removed; on an error `id_map` stays as it was.
    pub fn remove(&mut self, ids: &[&str]) -> Result<usize, String> {
        let wanted: std::collections::HashSet<&str> = ids.iter().copied().collect();
        let rows: Vec<u64> =
            self.id_map.iter().enumerate().filter(|(_, id)| wanted.contains(&***id)).map(|(i, _)| i as u64).collect();
        if rows.is_empty() {
            return Ok(0);
        }
        let mut removed: u64 = 0;
        // (handles made here have row_base 0: global row ids are `id_map` positions)
        let rc = unsafe { cqs_hip_index_remove(self.handle, rows.as_ptr(), rows.len() as u64, &mut removed) };
        if rc != CQS_HIP_OK {
            return Err(self.last_error());
        }
        let mut gone = rows.into_iter().peekable();
        let mut i: u64 = 0;
        self.id_map.retain(|_| {
            let drop = gone.peek() == Some(&i);
            if drop {
                gone.next();
            }
            i += 1;
            !drop
        });
        self.row_of = std::sync::OnceLock::new();
        Ok(removed as usize)
    }

    /// Write re-embedded chunks back under the ids the index already holds (`Store::update_embeddings_batch`,
    /// src/store/chunks/crud.rs:349-480, after the enrichment pass; the conflict arm of `upsert_chunks_batch` in the watch
    /// loop): the library rewrites the rows where they lie, shadow copies included; `id_map`, the row numbering and the
    /// tags stay.  Ids the index does not hold are skipped, as the reference's UPDATE matches no row for them.  Returns
    /// the number of rows written; an id named twice or a misshapen embedding is an error and writes nothing.
    pub fn update_embeddings(&mut self, updates: &[(String, Embedding)]) -> Result<usize, String> {
        let row_of = self.row_of.get_or_init(|| {
            let mut m = std::collections::HashMap::with_capacity(self.id_map.len());
            for (i, id) in self.id_map.iter().enumerate() {
                m.entry(id.clone()).or_insert(i as u64);
            }
            m
        });
        let mut seen: std::collections::HashSet<&str> = std::collections::HashSet::with_capacity(updates.len());
        let mut rows: Vec<u64> = Vec::new();
        let mut flat: Vec<f32> = Vec::new();
        for (id, embedding) in updates {
            if !seen.insert(id.as_str()) {
                return Err(format!("HIP update: id {id} named twice"));
            }
            let v = embedding.as_slice();
            if v.len() != self.dim {
                return Err(format!("HIP update: dimension mismatch: expected {}, got {}", self.dim, v.len()));
            }
            // (handles made here have row_base 0: global row ids are `id_map` positions)
            if let Some(row) = row_of.get(id.as_str()) {
                rows.push(*row);
                flat.extend_from_slice(v);
            }
        }
        if rows.is_empty() {
            return Ok(0);
        }
        let mut updated: u64 = 0;
        let rc = unsafe { cqs_hip_index_update(self.handle, rows.as_ptr(), flat.as_ptr(), rows.len() as u64, &mut updated) };
        if rc != CQS_HIP_OK {
            if unsafe { cqs_hip_index_poisoned(self.handle) } != 0 {
                self.poisoned.store(true, Ordering::Release);
            }
            return Err(self.last_error());
        }
        Ok(updated as usize)
    }

    /// `CagraIndex::save` (src/cagra.rs:1086-1157): the library streams the rows HBM -> `<path>.tmp` -> fsync -> `.bak`
    /// swap -> rename (save_blob_atomic_with_rollback, src/cagra.rs:1468-1592, restated in C++) and returns the blob's
    /// checksum; the sidecar goes out through write-temp + rename like `write_meta_atomic` (src/cagra.rs:1594-1652).
    /// A blob without its sidecar is useless, so a sidecar failure removes both (src/cagra.rs:1143-1147).
    pub fn save(&self, path: &std::path::Path, chunk_count: usize) -> Result<(), String> {
        let cpath = std::ffi::CString::new(path.to_string_lossy().as_bytes()).map_err(|e| e.to_string())?;
        let mut checksum = 0u64;
        let rc = unsafe { cqs_hip_index_save(self.handle, cpath.as_ptr(), &mut checksum) };
        if rc != CQS_HIP_OK {
            return Err(format!("cqs_hip_index_save failed ({rc}): {}", self.last_error()));
        }
        let meta = HipMeta {
            magic: HIP_META_MAGIC.into(),
            version: HIP_META_VERSION,
            dim: self.dim,
            chunk_count,
            id_map: self.id_map.iter().map(|s| s.to_string()).collect(),
            checksum: format!("{checksum:016x}"),
            metric: self.metric.as_str().to_string(),
        };
        let meta_path = path.with_extension("hipflat.meta");
        let tmp = path.with_extension("hipflat.meta.tmp");
        let write = || -> std::io::Result<()> {
            let f = std::fs::File::create(&tmp)?;
            serde_json::to_writer(std::io::BufWriter::new(&f), &meta).map_err(std::io::Error::other)?;
            f.sync_all()?;
            std::fs::rename(&tmp, &meta_path)
        };
        write().map_err(|e| {
            let _ = std::fs::remove_file(&tmp);
            Self::delete_persisted(path);
            format!("HIP sidecar write failed: {e}")
        })
    }

    /// `CagraIndex::load` (src/cagra.rs:1174-1330): sidecar magic / version / dim / chunk_count must match the store,
    /// then the library validates the blob (header, size, checksum while streaming it to HBM) and the checksum must
    /// be the sidecar's.  Any mismatch is an `Err`: the caller deletes both files and rebuilds.
    pub fn load(path: &std::path::Path, dim: usize, chunk_count: usize, devices: &[i32]) -> Result<Self, String> {
        let meta_path = path.with_extension("hipflat.meta");
        let meta: HipMeta = serde_json::from_reader(std::io::BufReader::new(
            std::fs::File::open(&meta_path).map_err(|e| format!("HIP sidecar unreadable: {e}"))?,
        ))
        .map_err(|e| format!("HIP sidecar unparsable: {e}"))?;
        if meta.magic != HIP_META_MAGIC || meta.version != HIP_META_VERSION {
            return Err("HIP sidecar: bad magic / version".into());
        }
        if meta.dim != dim || meta.chunk_count != chunk_count || meta.id_map.len() > chunk_count {
            return Err("HIP sidecar: stale (dim / chunk_count mismatch)".into());
        }
        let metric: DistanceMetric = meta.metric.parse().map_err(|_| "HIP sidecar: bad metric".to_string())?;
        let cpath = std::ffi::CString::new(path.to_string_lossy().as_bytes()).map_err(|e| e.to_string())?;
        let mut handle: *mut CqsHipIndex = std::ptr::null_mut();
        let rows = meta.id_map.len() as u64;   // zero / non-finite rows were skipped at build: rows <= chunk_count
        let rc = unsafe {
            if devices.len() <= 1 {
                cqs_hip_index_load(cpath.as_ptr(), dim as u32, rows, devices.first().copied().unwrap_or(0), 0, &mut handle)
            } else {
                cqs_hip_index_load_sharded(cpath.as_ptr(), dim as u32, rows, devices.as_ptr(), devices.len() as u32, 0, &mut handle)
            }
        };
        if rc != CQS_HIP_OK || handle.is_null() {
            return Err(format!("HIP blob rejected (rc = {rc})"));
        }
        let idx = Self {
            handle,
            id_map: meta.id_map.into_iter().map(String::into_boxed_str).collect(),
            dim,
            metric,
            poisoned: AtomicBool::new(false),
            row_of: std::sync::OnceLock::new(),
            tag_codes: None,
        };
        // the sidecar must describe THIS blob: its checksum is the one the library just verified against the rows
        let blob_metric = unsafe { cqs_hip_index_metric(idx.handle) };
        let want = match metric { DistanceMetric::Cosine => CQS_HIP_METRIC_COSINE, DistanceMetric::DotProduct => CQS_HIP_METRIC_DOT };
        if blob_metric != want || !blob_checksum_matches(path, &meta.checksum) {
            return Err("HIP sidecar does not match the blob".into());
        }
        Ok(idx)
    }

    /// `CagraIndex::delete_persisted` (src/cagra.rs:1332-1345).
    pub fn delete_persisted(path: &std::path::Path) {
        let _ = std::fs::remove_file(path);
        let _ = std::fs::remove_file(path.with_extension("hipflat.meta"));
    }

    /// `find_neighbors` (src/cli/commands/search/neighbors.rs:86-132) on the resident corpus: exact kNN of an indexed
    /// chunk, itself excluded, (score desc, id asc), limit clamped to [1, SIMILAR_LIMIT_MAX] inside the library.
    /// `None` = the chunk is not in this index (the caller falls back to the store scan).
    pub fn find_neighbors(&self, target_id: &str, limit: usize) -> Option<Vec<IndexResult>> {
        let row = self.id_map.iter().position(|id| &**id == target_id)? as u64;
        let (mut rows, mut scores, mut count) = (vec![0u64; 100], vec![0f32; 100], 0u32);
        let rc = unsafe {
            cqs_hip_index_neighbors(self.handle, row, limit.min(u32::MAX as usize) as u32, rows.as_mut_ptr(),
                                    scores.as_mut_ptr(), &mut count)
        };
        if rc != CQS_HIP_OK {
            tracing::warn!(error = %self.last_error(), rc, "HIP neighbors failed");
            return None;
        }
        Some((0..count as usize)
            .filter_map(|i| self.id_map.get(rows[i] as usize).map(|id| IndexResult { id: id.to_string(), score: scores[i] }))
            .collect())
    }

    /// The exact kNN graph of the resident corpus: entry i is `find_neighbors` of `id_map[i]` - what `cqs index --umap`
    /// hands umap-learn as its precomputed graph instead of streaming every embedding to it.  The rows go to the library
    /// in calls of 4096 targets (whole tiles of 256), so searches on the same handle get their turn between calls.
    /// `None` = the device failed or the handle is row-sharded: the caller keeps its CPU path.
    pub fn knn_graph(&self, limit: usize) -> Option<Vec<Vec<IndexResult>>> {
        let n = self.id_map.len();
        let l = limit.clamp(1, 100);
        let mut graph = Vec::with_capacity(n);
        let (mut rows, mut scores, mut counts) = (vec![0u64; 4096 * l], vec![0f32; 4096 * l], vec![0u32; 4096]);
        let mut first = 0usize;
        while first < n {
            let m = (n - first).min(4096);
            let rc = unsafe {
                cqs_hip_index_knn_graph(self.handle, first as u64, m as u64, l as u32, rows.as_mut_ptr(),
                                        scores.as_mut_ptr(), counts.as_mut_ptr())
            };
            if rc != CQS_HIP_OK {
                tracing::warn!(error = %self.last_error(), rc, "HIP kNN graph failed");
                return None;
            }
            for i in 0..m {
                graph.push((0..counts[i] as usize)
                    .filter_map(|j| {
                        self.id_map.get(rows[i * l + j] as usize).map(|id| IndexResult { id: id.to_string(), score: scores[i * l + j] })
                    })
                    .collect());
            }
            first += m;
        }
        Some(graph)
    }

    /// `cqs index --umap` without the Python child (src/cli/commands/index/umap.rs): 2-D coordinates of every resident chunk,
    /// (id, x, y) in `id_map` order - what the script's stdout is parsed into before `update_umap_coords_batch`.  The exact
    /// kNN graph at `n_neighbors - 1` and umap-learn's layout rules (min_dist 0.1, the stated departures of cqs_hip.h) run
    /// on the device; the index is held per graph call, not during the layout.  `n_epochs == 0` = 500 up to 10 000 chunks,
    /// 200 above.  Fewer than 2 chunks give the origin, as the script does.  `None` = the device failed or the handle is
    /// row-sharded: the caller keeps the script.
    pub fn umap_project(&self, n_neighbors: usize, n_epochs: usize, seed: u64) -> Option<Vec<(String, f32, f32)>> {
        let n = self.id_map.len();
        let mut xy = vec![0f32; 2 * n.max(1)];
        let rc = unsafe {
            cqs_hip_index_umap_project(self.handle, n_neighbors.min(u32::MAX as usize) as u32,
                                       n_epochs.min(u32::MAX as usize) as u32, seed, xy.as_mut_ptr())
        };
        if rc != CQS_HIP_OK {
            tracing::warn!(error = %self.last_error(), rc, "HIP UMAP projection failed");
            return None;
        }
        Some((0..n).map(|i| (self.id_map[i].to_string(), xy[2 * i], xy[2 * i + 1])).collect())
    }

    /// `umap_project` with a choice of initial coordinates: `pca_init` starts the layout from the scaled PCA projection of
    /// the resident rows (umap-learn's init="pca"), so where the clusters end up relative to each other follows the corpus
    /// and not the draw; `false` gives exactly `umap_project`'s bytes.
    pub fn umap_project_init(&self, n_neighbors: usize, n_epochs: usize, seed: u64, pca_init: bool) -> Option<Vec<(String, f32, f32)>> {
        let n = self.id_map.len();
        let mut xy = vec![0f32; 2 * n.max(1)];
        let rc = unsafe {
            cqs_hip_index_umap_project_init(self.handle, n_neighbors.min(u32::MAX as usize) as u32,
                                            n_epochs.min(u32::MAX as usize) as u32, seed, if pca_init { 1 } else { 0 },
                                            xy.as_mut_ptr())
        };
        if rc != CQS_HIP_OK {
            tracing::warn!(error = %self.last_error(), rc, "HIP UMAP projection failed");
            return None;
        }
        Some((0..n).map(|i| (self.id_map[i].to_string(), xy[2 * i], xy[2 * i + 1])).collect())
    }

    /// The top `n_components` (1 to 4) principal axes of the resident rows in `n_passes` streaming passes (0: 16):
    /// (mean [dim], axes [n_components * dim], variance [n_components], total variance).  With `project`, also every
    /// resident row's coordinates along the axes, `n_components` floats each in `id_map` order - a first picture of the
    /// corpus long before a UMAP projection is ready.  `None` = refused (fewer than 2 rows, a row-sharded handle) or failed.
    pub fn pca(&self, n_components: usize, n_passes: usize, seed: u64, project: bool)
               -> Option<(Vec<f32>, Vec<f32>, Vec<f32>, f32, Vec<f32>)> {
        let dim = self.dim;
        let nc = n_components.min(5);   // CQS_HIP_PCA_MAX_COMPONENTS + 1: the buffers stay small, the library refuses it
        let (mut mean, mut axes, mut var, mut total) = (vec![0f32; dim.max(1)], vec![0f32; (nc * dim).max(1)], vec![0f32; nc.max(1)], 0f32);
        let mut rc = unsafe {
            cqs_hip_index_pca(self.handle, nc as u32, n_passes.min(u32::MAX as usize) as u32, seed, mean.as_mut_ptr(),
                              axes.as_mut_ptr(), var.as_mut_ptr(), &mut total)
        };
        let n = self.id_map.len();
        let mut proj = vec![0f32; if project { (n * nc).max(1) } else { 1 }];
        if rc == CQS_HIP_OK && project {
            rc = unsafe { cqs_hip_index_pca_project(self.handle, mean.as_ptr(), axes.as_ptr(), nc as u32, 0, n as u64, proj.as_mut_ptr()) };
        }
        if rc != CQS_HIP_OK {
            tracing::warn!(error = %self.last_error(), rc, "HIP PCA failed");
            return None;
        }
        Some((mean, axes, var, total, proj))
    }

    /// Coordinates for new chunks in a projection that exists, without projecting the corpus again: `anchors_xy` holds the
    /// stored (x, y) of the first `anchors_xy.len()` resident chunks in `id_map` order - what `umap_project` returned and
    /// `update_umap_coords_batch` wrote - and `vectors` the new embeddings, `dim` floats each, before or after they were
    /// appended with `extend`.  Each new row's `n_neighbors` nearest anchors are searched on the device (rows past the
    /// anchors are masked out) and umap-learn's `transform` rules place it among them in one launch; the anchors do not
    /// move.  `n_epochs == 0` = 100 up to 10 000 new rows, 30 above.  Returns one (x, y) per new row, in order.  `None` =
    /// the device failed, the handle is row-sharded, or there are more anchors than resident chunks: the caller projects
    /// again.
    pub fn umap_transform(&self, anchors_xy: &[(f32, f32)], vectors: &[f32], n_neighbors: usize, n_epochs: usize, seed: u64)
                          -> Option<Vec<(f32, f32)>> {
        if self.dim == 0 || vectors.len() % self.dim != 0 {
            return None;
        }
        let m = vectors.len() / self.dim;
        let flat: Vec<f32> = anchors_xy.iter().flat_map(|&(x, y)| [x, y]).collect();
        let mut xy = vec![0f32; 2 * m.max(1)];
        let rc = unsafe {
            cqs_hip_index_umap_transform(self.handle, anchors_xy.len() as u64, flat.as_ptr(), vectors.as_ptr(), m as u64,
                                         n_neighbors.min(u32::MAX as usize) as u32, n_epochs.min(u32::MAX as usize) as u32,
                                         seed, xy.as_mut_ptr())
        };
        if rc != CQS_HIP_OK {
            tracing::warn!(error = %self.last_error(), rc, "HIP UMAP transform failed");
            return None;
        }
        Some((0..m).map(|i| (xy[2 * i], xy[2 * i + 1])).collect())
    }

    /// The embedding loop of `semantic_diff` (src/diff.rs:172-215) for matched pairs of two resident indexes: pair i is
    /// (row `rows_a[i]` of `self`, row `rows_b[i]` of `other`), rows being `id_map` positions.  Returns the modified
    /// pairs as (pair index, similarity) in ascending pair index - `sim < threshold` with
    /// `sim = full_cosine_similarity(..).unwrap_or(0.0)` - and the unchanged count; matching ChunkKeys before and sorting
    /// `modified` after (diff.rs:130-170, :226-236) stay with the caller.  `None` = the device failed, the handles do
    /// not go together (dim, device, sharding) or the threshold is NaN: the caller keeps its SQLite loop.
    pub fn semantic_diff_rows(&self, other: &HipIndex, rows_a: &[u64], rows_b: &[u64], threshold: f32)
                              -> Option<(Vec<(usize, f32)>, usize)> {
        if rows_a.len() != rows_b.len() {
            return None;
        }
        let m = rows_a.len();
        let (mut pairs, mut sims, mut counts) = (vec![0u64; m], vec![0f32; m], [0u64; 3]);
        let rc = unsafe {
            cqs_hip_index_diff(self.handle, rows_a.as_ptr(), other.handle, rows_b.as_ptr(), m as u64, threshold,
                               std::ptr::null_mut(), pairs.as_mut_ptr(), sims.as_mut_ptr(), counts.as_mut_ptr())
        };
        if rc != CQS_HIP_OK {
            if unsafe { cqs_hip_index_poisoned(self.handle) } != 0 {
                self.poisoned.store(true, Ordering::Release);
            }
            tracing::warn!(error = %self.last_error(), rc, "HIP semantic diff failed");
            return None;
        }
        let modified = (0..counts[0] as usize).map(|i| (pairs[i] as usize, sims[i])).collect();
        Some((modified, counts[1] as usize))
    }

    /// `mmr_rerank` (src/search/mmr.rs:59-126) over `(chunk id, relevance)` candidates of this index, in the caller's
    /// relevance-descending order, with the cosine of the stored embeddings as the similarity - the "embedding-MMR"
    /// mmr.rs:30-37 leaves as a follow-up.  Returns the picked indices into `candidates`, in pick order, exactly what
    /// `mmr_rerank` hands `finalize_results` (src/search/query.rs:674-703).  `None` = a candidate is not in this index,
    /// the pool exceeds the library's limit (1024), or the device failed: the caller keeps the surface-feature MMR.
    pub fn mmr_rerank(&self, candidates: &[(String, f32)], limit: usize, lambda: f32) -> Option<Vec<usize>> {
        if candidates.len() > 1024 || !lambda.is_finite() {
            return None;
        }
        // (first occurrence wins, as `position()` in find_neighbors)
        let row_of = self.row_of.get_or_init(|| {
            let mut m = std::collections::HashMap::with_capacity(self.id_map.len());
            for (i, id) in self.id_map.iter().enumerate() {
                m.entry(id.clone()).or_insert(i as u64);
            }
            m
        });
        let rows: Vec<u64> = candidates.iter().map(|(id, _)| row_of.get(id.as_str()).copied()).collect::<Option<_>>()?;
        let scores: Vec<f32> = candidates.iter().map(|(_, s)| *s).collect();
        let mut picks = vec![0u32; candidates.len().max(1)];
        let mut count = 0u32;
        let rc = unsafe {
            cqs_hip_index_mmr(self.handle, rows.as_ptr(), scores.as_ptr(), rows.len() as u32,
                              limit.min(u32::MAX as usize) as u32, lambda, picks.as_mut_ptr(), &mut count)
        };
        if rc != CQS_HIP_OK {
            tracing::warn!(error = %self.last_error(), rc, "HIP MMR re-rank failed");
            return None;
        }
        Some(picks[..count as usize].iter().map(|&i| i as usize).collect())
    }

    fn last_error(&self) -> String {
        let mut buf = vec![0u8; 512];
        let n = unsafe { cqs_hip_index_last_error(self.handle, buf.as_mut_ptr() as *mut c_char, buf.len()) };
        String::from_utf8_lossy(&buf[..n]).into_owned()
    }

    /// (passes, queries) of the combined blocks of filtered callers since the index was opened (diagnostic).
    pub fn combine_filter_stats(&self) -> (u64, u64) {
        let (mut p, mut q) = (0u64, 0u64);
        unsafe { cqs_hip_index_combine_filter_stats(self.handle, &mut p, &mut q) };
        (p, q)
    }

    /// The same for the combined blocks of `search_with_tags` callers (their `b = 1` tagged calls park on the queue).
    pub fn combine_tagged_stats(&self) -> (u64, u64) {
        let (mut p, mut q) = (0u64, 0u64);
        unsafe { cqs_hip_index_combine_tagged_stats(self.handle, &mut p, &mut q) };
        (p, q)
    }

    /// `search_with_filter` for several queries with a predicate each, in ONE call: the queries share passes over the
    /// corpus, every one under its own bitset (`cqs_hip_index_search_filtered`), and each gets what its own
    /// `search_with_filter` call returns.  A query of the wrong dimension gets an empty result.
    pub fn search_many_with_filter(&self, queries: &[&Embedding], k: usize, filters: &[&dyn Fn(&str) -> bool]) -> Vec<Vec<IndexResult>> {
        let b = queries.len();
        if b == 0 || b != filters.len() || self.id_map.is_empty() || k == 0 || queries.iter().any(|q| q.len() != self.dim) {
            return vec![Vec::new(); b];
        }
        let k = k.min(unsafe { cqs_hip_index_max_k(self.handle) } as usize);
        let words = self.id_map.len().div_ceil(32);
        let mut bitsets = vec![0u32; b * words];
        for (j, filter) in filters.iter().enumerate() {
            for (i, id) in self.id_map.iter().enumerate() {
                if filter(id) {
                    bitsets[j * words + i / 32] |= 1u32 << (i % 32);
                }
            }
        }
        let mut flat = Vec::with_capacity(b * self.dim);
        for q in queries {
            flat.extend_from_slice(q.as_slice());
        }
        let (mut rows, mut scores, mut counts) = (vec![0u64; b * k], vec![0f32; b * k], vec![0u32; b]);
        let rc = unsafe {
            cqs_hip_index_search_filtered(self.handle, flat.as_ptr(), b as u32, self.dim as u32, k as u32, bitsets.as_ptr(),
                                          words as u64, CQS_HIP_MODE_RAW, 0.0, rows.as_mut_ptr(), scores.as_mut_ptr(),
                                          counts.as_mut_ptr())
        };
        if rc != CQS_HIP_OK {
            if unsafe { cqs_hip_index_poisoned(self.handle) } != 0 {
                self.poisoned.store(true, Ordering::Release);
            }
            tracing::error!(error = %self.last_error(), rc, "HIP filtered block search failed");
            return vec![Vec::new(); b];
        }
        (0..b)
            .map(|j| {
                (0..counts[j] as usize)
                    .filter_map(|i| {
                        self.id_map.get(rows[j * k + i] as usize).map(|id| IndexResult {
                            id: id.to_string(),
                            score: match self.metric {
                                DistanceMetric::Cosine => scores[j * k + i].min(1.0),
                                DistanceMetric::DotProduct => scores[j * k + i],
                            },
                        })
                    })
                    .collect()
            })
            .collect()
    }

    fn search_impl(&self, query: &Embedding, k: usize, bitset: Option<&[u32]>) -> Vec<IndexResult> {
        let k = k.min(unsafe { cqs_hip_index_max_k(self.handle) } as usize);
        let mut rows = vec![0u64; k];
        let mut scores = vec![0f32; k];
        let mut count = 0u32;
        let rc = unsafe {
            cqs_hip_index_search(
                self.handle,
                query.as_slice().as_ptr(),
                1,
                query.len() as u32,
                k as u32,
                bitset.map_or(std::ptr::null(), |b| b.as_ptr()),
                CQS_HIP_MODE_RAW,
                0.0,
                rows.as_mut_ptr(),
                scores.as_mut_ptr(),
                &mut count,
            )
        };
        if rc != CQS_HIP_OK {
            if unsafe { cqs_hip_index_poisoned(self.handle) } != 0 {
                self.poisoned.store(true, Ordering::Release);
            }
            tracing::error!(error = %self.last_error(), rc, "HIP search failed");
            return Vec::new();
        }
        (0..count as usize)
            .filter_map(|i| {
                self.id_map.get(rows[i] as usize).map(|id| IndexResult {
                    id: id.to_string(),
                    // exact dot of unit vectors; cap the f32 overshoot like src/cagra.rs:656-661
                    score: match self.metric {
                        DistanceMetric::Cosine => scores[i].min(1.0),
                        DistanceMetric::DotProduct => scores[i],
                    },
                })
            })
            .collect()
    }
}

impl VectorIndex for HipIndex {
    /// Called concurrently from the daemon's client threads (src/cli/watch/daemon.rs:273) on one `Arc<dyn VectorIndex>`:
    /// the library combines single-query calls that meet on the handle - single-device or sharded; with a bitset
    /// (`search_with_filter`): single-device, in blocks of their own, every query under its own bitset - into shared
    /// passes over the corpus (include/cqs_hip.h, "Concurrent callers"), each caller still getting the bytes its lone call
    /// would.  `CQS_HIP_COMBINE_BITS=relaxed` in the daemon's environment (read when the index is opened) trades that
    /// bit-reproducibility for throughput past 8 callers (blocks of >= 9 on the matrix cores; scores within 2e-6).
    fn search(&self, query: &Embedding, k: usize) -> Vec<IndexResult> {
        let _span = tracing::debug_span!("hip_search", k).entered();
        if self.id_map.is_empty() || k == 0 {
            return Vec::new();
        }
        if query.len() != self.dim {
            tracing::warn!(expected_dim = self.dim, actual_dim = query.len(), "Query dimension mismatch");
            return Vec::new();
        }
        if self.poisoned.load(Ordering::Acquire) {
            return Vec::new();
        }
        // non-finite queries are rejected inside the C ABI as well (count 0)
        self.search_impl(query, k, None)
    }

    fn len(&self) -> usize {
        unsafe { cqs_hip_index_len(self.handle) as usize }
    }

    fn name(&self) -> &'static str {
        "HIP"
    }

    fn dim(&self) -> usize {
        self.dim
    }

    /// GPU-native filtered search: bitset built on the host from the predicate
    /// (src/cagra.rs:747-757); all-pass / none / k-cap handled by the C ABI
    /// (src/cagra.rs:760-775).
    fn search_with_filter(&self, query: &Embedding, k: usize, filter: &dyn Fn(&str) -> bool) -> Vec<IndexResult> {
        if self.id_map.is_empty() || k == 0 || query.len() != self.dim {
            return Vec::new();
        }
        let n = self.id_map.len();
        let mut bitset = vec![0u32; n.div_ceil(32)];
        for (i, id) in self.id_map.iter().enumerate() {
            if filter(id) {
                bitset[i / 32] |= 1u32 << (i % 32);
            }
        }
        self.search_impl(query, k, Some(&bitset))
    }

    fn is_poisoned(&self) -> bool {
        self.poisoned.load(Ordering::Acquire) || unsafe { cqs_hip_index_poisoned(self.handle) } != 0
    }

    fn max_k(&self) -> Option<usize> {
        Some(unsafe { cqs_hip_index_max_k(self.handle) } as usize)
    }

    /// Scores are the exact dot product of unit vectors = the cosine the brute-force path
    /// recomputes, so the BLOB refetch can be skipped (src/search/query.rs:1152-1172).
    fn index_scores_are_cosine(&self) -> bool {
        matches!(self.metric, DistanceMetric::Cosine)
    }
}

/// Blob header (include/cqs_hip.h, `cqs_hip_index_save`): magic[8] version dim metric pad (u32 x 4) rows checksum (u64 x 2).
fn blob_checksum_matches(path: &std::path::Path, want_hex: &str) -> bool {
    use std::io::Read;
    let mut head = [0u8; 40];
    match std::fs::File::open(path).and_then(|mut f| f.read_exact(&mut head)) {
        Ok(()) => &head[..8] == b"CQSHIPF1" && format!("{:016x}", u64::from_le_bytes(head[32..40].try_into().unwrap())) == want_hex,
        Err(_) => false,
    }
}

/// `IndexBackend` registration; priority above CAGRA (100) and tiered (150).
pub struct HipBackend;

impl<Mode: ClearHnswDirty> IndexBackend<Mode> for HipBackend {
    fn name(&self) -> &'static str {
        "hip"
    }

    fn priority(&self) -> i32 {
        200
    }

    fn try_open(&self, ctx: &BackendContext<'_, Mode>) -> Result<Option<Box<dyn VectorIndex>>, StoreError> {
        const HIP_THRESHOLD_DEFAULT: u64 = 5000; // same gate as CQS_CAGRA_THRESHOLD (src/cagra.rs:1683-1690)
        let threshold: u64 = std::env::var("CQS_HIP_THRESHOLD")
            .ok()
            .and_then(|v| v.parse().ok())
            .or_else(|| ctx.policy.and_then(|p| p.cagra_threshold))
            .unwrap_or(HIP_THRESHOLD_DEFAULT);
        let chunk_count = ctx.store.chunk_count().unwrap_or(0);
        let dim = ctx.store.dim();
        let devices = devices_from_env();
        let gpu_available = HipIndex::gpu_available_for(chunk_count as usize, dim, &devices);
        if chunk_count < threshold || !gpu_available {
            tracing::info!(backend = "hnsw", source = "hip-ineligible", chunk_count, threshold, dim, gpu_available,
                "Vector index backend selected");
            return Ok(None);
        }
        // persisted first (src/cagra.rs:1726-1752): streaming the blob into HBM beats re-reading every BLOB out of
        // SQLite; a stale / corrupt pair is deleted and rebuilt
        let blob = ctx.cqs_dir.join("index.hipflat");
        if hip_persist_enabled() && blob.exists() {
            match HipIndex::load(&blob, dim, chunk_count as usize, &devices) {
                Ok(idx) => {
                    tracing::info!(backend = "hip", source = "persisted", vectors = idx.len(), chunk_count, threshold,
                        "Vector index backend selected");
                    idx.enable_bf16_scan_from_env();   // (the blob does not hold the shadow)
                    return Ok(Some(Box::new(idx) as Box<dyn VectorIndex>));
                }
                Err(e) => {
                    tracing::warn!(error = %e, path = %blob.display(), "HIP persisted load failed, rebuilding from store");
                    HipIndex::delete_persisted(&blob);
                }
            }
        }
        let metric = match DistanceMetric::from_env() {
            Ok(Some(m)) => m,
            Ok(None) => crate::hnsw::HnswIndex::stored_metric(ctx.cqs_dir, "index").unwrap_or(DistanceMetric::Cosine),
            Err(e) => {
                tracing::warn!(error = %e, "Invalid CQS_DISTANCE_METRIC - falling through");
                return Ok(None);
            }
        };
        match HipIndex::build_from_store(ctx.store, dim, metric, &devices) {
            Ok(idx) => {
                tracing::info!(backend = "hip", source = "rebuilt", vectors = idx.len(), chunk_count, devices = ?devices,
                    "Vector index backend selected");
                if hip_persist_enabled() {
                    if let Err(e) = idx.save(&blob, chunk_count as usize) {
                        tracing::warn!(error = %e, path = %blob.display(), "Failed to persist HIP index (will rebuild next restart)");
                    }
                }
                idx.enable_bf16_scan_from_env();
                Ok(Some(Box::new(idx) as Box<dyn VectorIndex>))
            }
            Err(e) => {
                tracing::warn!(error = %e, "Failed to build HIP index, falling through");
                Ok(None)
            }
        }
    }
}
