"""Host-side mirror of the reference's vector-index interface over the C ABI.

Reference surface mirrored here (names, argument meaning, error behaviour):
  DistanceMetric          src/index.rs:45-125
  IndexResult             src/index.rs:129-134
  VectorIndex (trait)     src/index.rs:139-239
  IndexBackend / context  src/index.rs:245-291, selector src/cli/store.rs:470-509
  CagraIndex (exemplar)   src/cagra.rs:255-277, search :443-492, filter :727-820,
                          build_from_flat :922-960, CagraBackend::try_open :1676-1802
  prepare_index_data      src/hnsw/mod.rs:688-746

The reference is Rust; with no Rust toolchain in the build image the host side
above the C ABI is written here (Python for the test/bench harness) and as a
Rust shim *source* in rust_shim/ (see INTEGRATION.md).  Every search goes through
libcqs_hip.so; there is no CPU fallback in this module.
"""
from __future__ import annotations

import ctypes as C
import enum
import logging
from dataclasses import dataclass, field
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

log = logging.getLogger("cqs_amd")


class DistanceMetric(enum.Enum):
    """src/index.rs:45-56."""

    Cosine = 0
    DotProduct = 1

    def as_str(self) -> str:  # src/index.rs:61-66
        return "cosine" if self is DistanceMetric.Cosine else "dot"

    @staticmethod
    def parse(raw: str) -> "DistanceMetric":  # FromStr, src/index.rs:112-125
        s = raw.strip().lower()
        if s == "cosine":
            return DistanceMetric.Cosine
        if s in ("dot", "dotproduct", "dot_product", "dot-product", "innerproduct", "inner_product", "ip"):
            return DistanceMetric.DotProduct
        raise ValueError(f"unknown distance metric {s!r} (supported: cosine, dot)")


@dataclass
class IndexResult:
    """src/index.rs:129-134."""

    id: str
    score: float


@dataclass
class DiffEntry:
    """`DiffEntry` (src/diff.rs) by chunk id; `similarity` is the f32 cosine, None where there is none to give."""

    id: str
    similarity: Optional[float]


@dataclass
class MovedEntry:
    """A chunk the source holds under one key and the target under another (moved to another file, renamed): the two
    ids and the f32 dot of the two stored rows (the cosine on cosine indexes).  The reference has no such entry."""

    source_id: str
    target_id: str
    similarity: float


@dataclass
class DiffResult:
    """`DiffResult` (src/diff.rs:238-245); `moved` is this library's (`semantic_diff(..., moved_threshold=...)`)."""

    added: List[DiffEntry]
    removed: List[DiffEntry]
    modified: List[DiffEntry]
    unchanged_count: int
    moved: List[MovedEntry] = field(default_factory=list)


@dataclass
class DriftEntry:
    """`DriftEntry` (src/drift.rs:12-25)."""

    id: str
    similarity: float
    drift: float


@dataclass
class DriftResult:
    """`DriftResult` (src/drift.rs:27-42)."""

    threshold: float
    min_drift: float
    drifted: List[DriftEntry]
    total_compared: int
    unchanged: int


def _total_order_key(x: float) -> int:
    """f32 -> int in the order of Rust's `f32::total_cmp`."""
    b = int(np.float32(x).view(np.uint32))
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def match_ids(source_ids: Sequence[str], target_ids: Sequence[str], key: Optional[Callable[[str], object]] = None):
    """The matching of `semantic_diff` (src/diff.rs:130-170) over two id lists in row order.  Returns (added: target rows
    whose key the source lacks; removed: source rows whose key the target lacks; matched: [(source row, target row)]).
    Of several rows with one key the last stands for the key, on each side."""
    key = key or (lambda cid: cid)
    src = {key(cid): i for i, cid in enumerate(source_ids)}
    tgt = {key(cid): i for i, cid in enumerate(target_ids)}
    added = [i for k, i in tgt.items() if k not in src]
    removed = [i for k, i in src.items() if k not in tgt]
    matched = [(src[k], i) for k, i in tgt.items() if k in src]
    return added, removed, matched


def sort_modified(entries: Sequence[DiffEntry]) -> List[DiffEntry]:
    """src/diff.rs:226-236: most changed first (similarity ascending under the f32 total order), entries without a
    similarity behind every entry with one, ties by id."""
    return sorted(entries, key=lambda e: (e.similarity is None, 0 if e.similarity is None else _total_order_key(e.similarity), e.id))


def sort_moved(entries: Sequence[MovedEntry]) -> List[MovedEntry]:
    """Like `sort_modified`: least similar first (the f32 total order), ties by the target's id."""
    return sorted(entries, key=lambda e: (_total_order_key(e.similarity), e.target_id))


MATCH_NONE = 0xFFFFFFFFFFFFFFFF   # `best` of a row without a finite entry (its score is 0.0)


def _order_keys(scores: np.ndarray) -> np.ndarray:
    """f32 array -> u32 array in the order of `f32::total_cmp`."""
    b = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def merge_best(best: np.ndarray, score: np.ndarray, other_best: np.ndarray, other_score: np.ndarray) -> None:
    """`cqs_match::merge_best` (match_host.h) over whole arrays, in place: (best, score) are answers over some blocks of the
    other side's list, (other_best, other_score) over another, positions global in that list.  The greater score under
    the f32 total order wins, then the lower position; MATCH_NONE loses to everything."""
    none = np.uint64(MATCH_NONE)
    mine, theirs = _order_keys(score), _order_keys(other_score)
    keep = (best != none) & ((mine > theirs) | ((mine == theirs) & (best <= other_best)))
    take = (other_best != none) & ~keep
    best[take] = other_best[take]
    score[take] = other_score[take]


def mutual_pairs(best_a: np.ndarray, score_a: np.ndarray, best_b: np.ndarray, threshold: float) -> List[Tuple[int, int]]:
    """`cqs_match::mutual_pairs`: the (i, j) with best_a[i] == j, best_b[j] == i and score_a[i] >= threshold (an f32
    compare), in ascending i."""
    thr = np.float32(threshold)
    out = []
    for i in range(len(best_a)):
        j = int(best_a[i])
        if j != MATCH_NONE and j < len(best_b) and int(best_b[j]) == i and np.float32(score_a[i]) >= thr:
            out.append((i, j))
    return out


def drift_entries(modified: Sequence[DiffEntry], min_drift: float) -> List[DriftEntry]:
    """src/drift.rs:73-101: entries without a similarity are skipped; drift = 1.0 - similarity in f32, kept where
    drift >= min_drift; sorted by (drift descending under the f32 total order, id)."""
    out = []
    for e in modified:
        if e.similarity is None:
            continue
        drift = np.float32(1.0) - np.float32(e.similarity)
        if drift >= np.float32(min_drift):
            out.append(DriftEntry(e.id, float(np.float32(e.similarity)), float(drift)))
    return sorted(out, key=lambda d: (-_total_order_key(d.drift), d.id))


class HipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"cqs_hip error {code}: {msg}")
        self.code = code


class VectorIndex:
    """The `VectorIndex` trait (src/index.rs:139-239), defaults included."""

    def search(self, query: np.ndarray, k: int) -> List[IndexResult]:
        raise NotImplementedError

    def __len__(self) -> int:
        raise NotImplementedError

    def is_empty(self) -> bool:
        return len(self) == 0

    def name(self) -> str:
        raise NotImplementedError

    def dim(self) -> int:
        raise NotImplementedError

    def search_with_filter(self, query: np.ndarray, k: int, flt: Callable[[str], bool]) -> List[IndexResult]:
        # default: over-fetch 3x, post-filter, take k (src/index.rs:167-193)
        kk = min(k * 3, 2**63 - 1)
        out = [r for r in self.search(query, kk) if flt(r.id)][:k]
        if len(out) < k and len(self) >= k:
            log.warning("Filter-aware search under-returned: returned=%d requested=%d index_size=%d",
                        len(out), k, len(self))
        return out

    def is_poisoned(self) -> bool:  # src/index.rs:203-205
        return False

    def max_k(self) -> Optional[int]:  # src/index.rs:219-221
        return None

    def index_scores_are_cosine(self) -> bool:  # src/index.rs:236-238
        return False


def prepare_index_data(embeddings: Sequence[Tuple[str, np.ndarray]], expected_dim: int):
    """src/hnsw/mod.rs:688-746: validate dims, skip all-zero and non-finite rows.

    Returns (id_map, flat [kept, dim] f32, kept).  Raises ValueError like
    `HnswError::Build` on empty input, dimension mismatch, or nothing kept.
    """
    if len(embeddings) == 0:
        raise ValueError("No embeddings to index")
    for cid, emb in embeddings:
        if len(emb) != expected_dim:
            raise ValueError(f"Embedding dimension mismatch for {cid}: got {len(emb)}, expected {expected_dim}")
    id_map: List[str] = []
    rows = []
    for cid, emb in embeddings:
        v = np.asarray(emb, dtype=np.float32)
        if not np.any(v != 0.0):
            log.warning("Skipping zero-vector embedding chunk_id=%s", cid)
            continue
        if not np.all(np.isfinite(v)):
            log.warning("Skipping non-finite embedding chunk_id=%s", cid)
            continue
        id_map.append(cid)
        rows.append(v)
    if not id_map:
        raise ValueError("No valid embeddings to index (all were zero-vector or non-finite)")
    return id_map, np.stack(rows).astype(np.float32, copy=False), len(id_map)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def tag_filter(f0: Optional[Iterable[int]] = None, f1: Optional[Iterable[int]] = None,
               f2: Optional[Iterable[int]] = None, f3: Optional[Iterable[int]] = None) -> np.ndarray:
    """The `allow` argument of the tagged searches (include/cqs_hip.h, "row tags"): 32 u32 words = four 256-bit sets,
    one per 8-bit field of a row's tag.  Each argument lists the allowed codes (0 .. 255) of its field; `None` leaves the
    field unconstrained (all 256 bits set).  Bit v of field f's set is bit v % 32 of word 8 f + v // 32."""
    allow = np.zeros(32, dtype=np.uint32)
    for f, codes in enumerate((f0, f1, f2, f3)):
        if codes is None:
            allow[8 * f:8 * f + 8] = 0xFFFFFFFF
            continue
        for v in codes:
            v = int(v)
            if not 0 <= v <= 255:
                raise ValueError(f"tag code {v} of field {f} is not in 0 .. 255")
            allow[8 * f + v // 32] |= np.uint32(1 << (v % 32))
    return allow


def _allow_words(allow) -> np.ndarray:
    a = np.ascontiguousarray(allow, dtype=np.uint32).reshape(-1)
    if a.shape[0] != 32:
        raise ValueError("allow must be 32 uint32 words (tag_filter)")
    return a


class HipIndex(VectorIndex):
    """Exact GPU index: `[n, dim]` f32 rows resident in HBM, brute-force scan + top-k.

    Same shape as `CagraIndex` (src/cagra.rs:255-277): owns `id_map` (row -> chunk id,
    rowid order), serialises device access inside the handle, never raises for device
    trouble in `search` (logs + empty list, src/cagra.rs:445-470,543-626).
    """

    def __init__(self, handle: int, id_map: Optional[List[str]], metric: DistanceMetric):
        self._lib = _lib.load()
        self._h = C.c_void_p(handle)
        self.id_map = id_map
        self.metric = metric
        self._keepalive = None

    # ---- construction ---------------------------------------------------------
    @classmethod
    def build_from_flat(cls, id_map: Optional[List[str]], flat: np.ndarray,
                        metric: DistanceMetric = DistanceMetric.Cosine, device: int = 0,
                        row_base: int = 0) -> "HipIndex":
        """`CagraIndex::build_from_flat` (src/cagra.rs:922-960).  `id_map=None` = integer ids."""
        lib = _lib.load()
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        if flat.ndim != 2:
            raise ValueError("flat must be [n, dim]")
        n, dim = flat.shape
        if id_map is not None and len(id_map) != n:
            raise ValueError("id_map length != rows")
        h = C.c_void_p()
        rc = lib.cqs_hip_index_create(_ptr(flat), n, dim, metric.value, device, row_base, C.byref(h))
        if rc != _lib.OK:
            raise HipError(rc, "cqs_hip_index_create failed")
        return cls(h.value, id_map, metric)

    @classmethod
    def build_sharded(cls, id_map: Optional[List[str]], flat: np.ndarray, devices: Sequence[int],
                      metric: DistanceMetric = DistanceMetric.Cosine, row_base: int = 0) -> "HipIndex":
        """`cqs_hip_index_create_sharded`: ONE process, the rows cut over `devices` (rowid order); the handle
        behaves like any other (`search`, `search_with_filter`, `find_neighbors`, `extend`, `save`)."""
        lib = _lib.load()
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        if flat.ndim != 2:
            raise ValueError("flat must be [n, dim]")
        n, dim = flat.shape
        if id_map is not None and len(id_map) != n:
            raise ValueError("id_map length != rows")
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        h = C.c_void_p()
        rc = lib.cqs_hip_index_create_sharded(_ptr(flat), n, dim, metric.value, _ptr(devs), len(devs), row_base, C.byref(h))
        if rc != _lib.OK:
            raise HipError(rc, "cqs_hip_index_create_sharded failed")
        return cls(h.value, id_map, metric)

    def shards(self):
        """[(device, first_row, rows, gathers_with_rccl)] per shard (one entry for a single-device index)."""
        out = []
        for s in range(int(self._lib.cqs_hip_index_shards(self._h))):
            dev, first, rows, rc = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_int32()
            if self._lib.cqs_hip_index_shard_info(self._h, s, C.byref(dev), C.byref(first), C.byref(rows), C.byref(rc)) == _lib.OK:
                out.append((dev.value, first.value, rows.value, bool(rc.value)))
        return out

    @classmethod
    def build_from_device(cls, id_map: Optional[List[str]], d_ptr: int, n: int, dim: int,
                          metric: DistanceMetric = DistanceMetric.Cosine, device: int = 0,
                          row_base: int = 0, borrow: bool = True, keepalive=None) -> "HipIndex":
        lib = _lib.load()
        h = C.c_void_p()
        rc = lib.cqs_hip_index_create_device(C.c_void_p(d_ptr), n, dim, metric.value, device, row_base,
                                             1 if borrow else 0, C.byref(h))
        if rc != _lib.OK:
            raise HipError(rc, "cqs_hip_index_create_device failed")
        idx = cls(h.value, id_map, metric)
        idx._keepalive = keepalive if borrow else None
        return idx

    @classmethod
    def build_from_embeddings(cls, embeddings: Sequence[Tuple[str, np.ndarray]], dim: int,
                              metric: DistanceMetric = DistanceMetric.Cosine, device: int = 0) -> "HipIndex":
        id_map, flat, _ = prepare_index_data(embeddings, dim)
        return cls.build_from_flat(id_map, flat, metric, device)

    def extend(self, ids: Optional[List[str]], rows: np.ndarray) -> None:
        """Incremental add (tiered.rs extend contract, src/tiered.rs:1-43)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim():
            raise ValueError("rows must be [m, dim]")
        if (self.id_map is None) != (ids is None):
            raise ValueError("ids must match the index's id flavour")
        rc = self._lib.cqs_hip_index_extend(self._h, _ptr(rows), rows.shape[0])
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        if ids is not None:
            self.id_map.extend(ids)

    def remove_rows(self, rows) -> int:
        """`cqs_hip_index_remove`: the stored rows `rows` (global row ids, any order, duplicates count once) leave the
        index in place; the survivors keep their order and are renumbered densely.  Returns the number removed.  Raises
        HipError (INVALID: an id the index does not hold, a borrowed or sharded handle); `id_map` is not touched here."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        removed = C.c_uint64()
        rc = self._lib.cqs_hip_index_remove(self._h, _ptr(r), r.shape[0], C.byref(removed))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return int(removed.value)

    def remove(self, ids: Iterable[str]) -> int:
        """Delete chunks by id (the watch loop's deletions, the tiered backend's "clean orphaned vectors",
        src/tiered.rs:13-17).  Ids the index does not hold are ignored: the watch loop also deletes chunks that were
        never indexed (zero vectors skipped by `prepare_index_data`).  Returns the number removed; on HipError `id_map`
        is left as it was."""
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        local = set()
        if self.id_map is None:
            n = len(self)
            for cid in ids:
                try:
                    row = int(cid)
                except ValueError:
                    continue
                if base <= row < base + n:
                    local.add(row - base)
        else:
            row_of = self._rows_by_id()
            local = {row_of[cid] for cid in ids if cid in row_of}
        if not local:
            return 0
        removed = self.remove_rows([base + i for i in sorted(local)])
        if self.id_map is not None:
            self.id_map[:] = [cid for i, cid in enumerate(self.id_map) if i not in local]
            self.__dict__.pop("_row_of", None)
        return removed

    def update_rows(self, rows, vectors) -> int:
        """`cqs_hip_index_update`: `vectors[i]` replaces the stored row `rows[i]` (global row ids, any order, each at most
        once) where it lies, in the f32 corpus and in the shadow copies; nothing moves and nothing is renumbered.  Returns
        the number of rows written.  Raises HipError (INVALID: an id the index does not hold, an id named twice, a
        borrowed handle)."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[0] != r.shape[0] or (v.shape[0] and v.shape[1] != self.dim()):
            raise ValueError("vectors must be [len(rows), dim]")
        updated = C.c_uint64()
        rc = self._lib.cqs_hip_index_update(self._h, _ptr(r), _ptr(v), r.shape[0], C.byref(updated))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return int(updated.value)

    def update(self, ids: Sequence[str], vectors) -> int:
        """Write new embeddings back under ids the index already holds (`Store::update_embeddings_batch`,
        src/store/chunks/crud.rs:349-480: the enrichment pass; `upsert_chunks_batch`'s conflict arm in the watch loop).
        Ids the index does not hold are skipped, as the reference's UPDATE matches no row for them; an id named twice
        raises ValueError, as its staging table's primary key refuses it.  Returns the number of rows written;
        `id_map` is untouched."""
        ids = list(ids)
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[0] != len(ids) or v.shape[1] != self.dim():
            raise ValueError("vectors must be [len(ids), dim]")
        if len(set(ids)) != len(ids):
            raise ValueError("update: an id is named twice")
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        if self.id_map is None:
            n = len(self)
            held = []
            for i, cid in enumerate(ids):
                try:
                    row = int(cid)
                except ValueError:
                    continue
                if base <= row < base + n:
                    held.append((i, row))
            if len({row for _, row in held}) != len(held):
                raise ValueError("update: an id is named twice")       # ("7" and "07")
        else:
            row_of = self._rows_by_id()
            held = [(i, base + row_of[cid]) for i, cid in enumerate(ids) if cid in row_of]
        if not held:
            return 0
        return self.update_rows([row for _, row in held], v[[i for i, _ in held]])

    # ---- persistence: blob + CagraMeta-style sidecar (src/cagra.rs:973-1157, 1174-1330) -----------
    META_MAGIC = "cqs-hip-flat-meta"
    META_VERSION = 1

    def save(self, path: str) -> None:
        """`CagraIndex::save`: rows blob through the C ABI (atomic tmp -> rename) + `{path}.meta` JSON
        {magic, version, dim, chunk_count, id_map, checksum, metric} (also tmp -> rename)."""
        import json
        import os
        ck = C.c_uint64()
        rc = self._lib.cqs_hip_index_save(self._h, path.encode(), C.byref(ck))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        meta = {"magic": self.META_MAGIC, "version": self.META_VERSION, "dim": self.dim(), "chunk_count": len(self),
                "id_map": self.id_map, "checksum": f"{ck.value:016x}", "metric": self.metric.as_str()}
        tmp = path + ".meta.tmp"
        try:
            with open(tmp, "w") as f:
                json.dump(meta, f)
            os.replace(tmp, path + ".meta")
        except OSError:
            for p in (path, path + ".meta", tmp):   # a blob without its sidecar is useless (cagra.rs:1143-1147)
                try:
                    os.remove(p)
                except OSError:
                    pass
            raise

    @classmethod
    def load(cls, path: str, dim: int, chunk_count: int, device: int = 0,
             devices: Optional[Sequence[int]] = None) -> "HipIndex":
        """`CagraIndex::load`: sidecar magic / version / dim / chunk_count must match the store, the blob's
        checksum must match the sidecar; anything else raises ValueError (caller deletes + rebuilds)."""
        import json
        lib = _lib.load()
        try:
            with open(path + ".meta") as f:
                meta = json.load(f)
        except (OSError, ValueError) as e:
            raise ValueError(f"HIP index sidecar unreadable: {e}")
        if meta.get("magic") != cls.META_MAGIC or meta.get("version") != cls.META_VERSION:
            raise ValueError("HIP index sidecar: bad magic / version")
        if meta.get("dim") != dim or meta.get("chunk_count") != chunk_count:
            raise ValueError("HIP index sidecar: stale (dim / chunk_count mismatch)")
        ids = meta.get("id_map")
        if ids is not None and len(ids) != chunk_count:
            raise ValueError("HIP index sidecar: id_map length mismatch")
        # the sidecar must describe THIS blob: compare its checksum with the blob header's
        import struct
        try:
            with open(path, "rb") as f:
                magic, _ver, _dim, _metric, _pad, _rows, blob_ck = struct.unpack("<8sIIIIQQ", f.read(40))
        except (OSError, struct.error) as e:
            raise ValueError(f"HIP index blob unreadable: {e}")
        if magic != b"CQSHIPF1" or meta.get("checksum") != f"{blob_ck:016x}":
            raise ValueError("HIP index sidecar does not match the blob (checksum)")
        h = C.c_void_p()
        if devices is not None:
            devs = np.ascontiguousarray(list(devices), dtype=np.int32)
            rc = lib.cqs_hip_index_load_sharded(path.encode(), dim, chunk_count, _ptr(devs), len(devs), 0, C.byref(h))
        else:
            rc = lib.cqs_hip_index_load(path.encode(), dim, chunk_count, device, 0, C.byref(h))   # verifies the content
        if rc != _lib.OK:
            raise ValueError(f"HIP index blob rejected (rc={rc})")
        return cls(h.value, ids, DistanceMetric.parse(meta.get("metric", "cosine")))

    @staticmethod
    def delete_persisted(path: str) -> None:
        """`CagraIndex::delete_persisted` (src/cagra.rs:1739-1750)."""
        import os
        for p in (path, path + ".meta"):
            try:
                os.remove(p)
            except OSError:
                pass

    def close(self) -> None:
        if self._h:
            self._lib.cqs_hip_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- trait ------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self._lib.cqs_hip_index_len(self._h))

    def name(self) -> str:
        return "HIP"

    def dim(self) -> int:
        return int(self._lib.cqs_hip_index_dim(self._h))

    def is_poisoned(self) -> bool:
        return bool(self._lib.cqs_hip_index_poisoned(self._h))

    def max_k(self) -> Optional[int]:
        return int(self._lib.cqs_hip_index_max_k(self._h))

    def index_scores_are_cosine(self) -> bool:
        # exact dot of unit vectors == the brute-force cosine (src/search/query.rs:1152-1172)
        return self.metric is DistanceMetric.Cosine

    def last_error(self) -> str:
        buf = C.create_string_buffer(512)
        self._lib.cqs_hip_index_last_error(self._h, buf, 512)
        return buf.value.decode("utf-8", "replace")

    def _id(self, row: int) -> str:
        return str(row) if self.id_map is None else self.id_map[row - int(self._lib.cqs_hip_index_row_base(self._h))]

    def search_batch(self, queries: np.ndarray, k: int, keep_bitset: Optional[np.ndarray] = None,
                     mode: int = _lib.MODE_RAW, threshold: float = 0.0):
        """Block of queries through `cqs_hip_index_search`.  Returns (rows u64 [b,k], scores f32 [b,k], counts u32 [b])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        b, qd = q.shape
        rows = np.zeros((b, max(k, 1)), dtype=np.uint64)
        scores = np.zeros((b, max(k, 1)), dtype=np.float32)
        counts = np.zeros((b,), dtype=np.uint32)
        kb = None
        if keep_bitset is not None:
            kb = np.ascontiguousarray(keep_bitset, dtype=np.uint32)
            if kb.shape[0] < (len(self) + 31) // 32:
                raise ValueError("keep_bitset too short")
        rc = self._lib.cqs_hip_index_search(self._h, _ptr(q), b, qd, k, _ptr(kb), mode, threshold,
                                            _ptr(rows), _ptr(scores), _ptr(counts))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return rows[:, :k], scores[:, :k], counts

    def search_batch_filtered(self, queries: np.ndarray, k: int, keep_bitsets: np.ndarray,
                              mode: int = _lib.MODE_RAW, threshold: float = 0.0):
        """Block of queries with a keep-bitset each (`keep_bitsets` u32 [b, words], words >= ceil(len/32)) through
        `cqs_hip_index_search_filtered`: per query the answer of `search_batch(q, k, keep_bitset=its row)`.
        Returns (rows u64 [b,k], scores f32 [b,k], counts u32 [b])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        b, qd = q.shape
        kb = np.ascontiguousarray(keep_bitsets, dtype=np.uint32)
        if kb.ndim != 2 or kb.shape[0] != b:
            raise ValueError("keep_bitsets must be [b, words]")
        if kb.shape[1] < (len(self) + 31) // 32:
            raise ValueError("keep_bitsets too short")
        rows = np.zeros((b, max(k, 1)), dtype=np.uint64)
        scores = np.zeros((b, max(k, 1)), dtype=np.float32)
        counts = np.zeros((b,), dtype=np.uint32)
        rc = self._lib.cqs_hip_index_search_filtered(self._h, _ptr(q), b, qd, k, _ptr(kb), kb.shape[1], mode, threshold,
                                                     _ptr(rows), _ptr(scores), _ptr(counts))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return rows[:, :k], scores[:, :k], counts

    # ---- row tags (include/cqs_hip.h "row tags") ----------------
    def set_tags(self, tags, first: int = 0) -> None:
        """`cqs_hip_index_set_tags`: one u32 tag per row for the rows `first` .. `first + len(tags) - 1` (global row ids).
        The tagged rows stay a prefix: overwrite inside it and / or extend it.  Raises HipError (INVALID: a gap, a range
        past the end, a sharded handle)."""
        t = np.ascontiguousarray(tags, dtype=np.uint32).reshape(-1)
        rc = self._lib.cqs_hip_index_set_tags(self._h, int(first), _ptr(t), t.shape[0])
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())

    def tagged_rows(self) -> int:
        """The leading rows that have a tag (`cqs_hip_index_tagged_rows`)."""
        return int(self._lib.cqs_hip_index_tagged_rows(self._h))

    def count_tagged(self, allow) -> int:
        """The rows the filter `allow` (`tag_filter`) keeps (`cqs_hip_index_count_tagged`): what cqs logs as `included`."""
        kept = C.c_uint64()
        rc = self._lib.cqs_hip_index_count_tagged(self._h, _ptr(_allow_words(allow)), C.byref(kept))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return int(kept.value)

    def search_tagged_batch(self, queries: np.ndarray, k: int, allow, mode: int = _lib.MODE_RAW, threshold: float = 0.0):
        """Block of queries through `cqs_hip_index_search_tagged`: the answer of `search_batch(queries, k, keep_bitset=the
        host bitset of the same predicate)`, byte for byte, without the bitset.  `allow`: `tag_filter(...)`.
        Returns (rows u64 [b,k], scores f32 [b,k], counts u32 [b])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        b, qd = q.shape
        a = _allow_words(allow)
        rows = np.zeros((b, max(k, 1)), dtype=np.uint64)
        scores = np.zeros((b, max(k, 1)), dtype=np.float32)
        counts = np.zeros((b,), dtype=np.uint32)
        rc = self._lib.cqs_hip_index_search_tagged(self._h, _ptr(q), b, qd, k, _ptr(a), mode, threshold,
                                                   _ptr(rows), _ptr(scores), _ptr(counts))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return rows[:, :k], scores[:, :k], counts

    def search_tagged_multi(self, queries: np.ndarray, k: int, allows, mode: int = _lib.MODE_RAW, threshold: float = 0.0):
        """Block of queries with a tag filter EACH (`allows` u32 [b, 32], rows of `tag_filter(...)`) through
        `cqs_hip_index_search_tagged_multi`: per query the answer of `search_tagged_batch(q, k, its filter)`, the block's
        bitsets written by one kernel.  Returns (rows u64 [b,k], scores f32 [b,k], counts u32 [b])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        b, qd = q.shape
        a = np.ascontiguousarray(allows, dtype=np.uint32).reshape(-1, 32)
        if a.shape[0] != b:
            raise ValueError("allows must be [b, 32] uint32 words (tag_filter per query)")
        rows = np.zeros((b, max(k, 1)), dtype=np.uint64)
        scores = np.zeros((b, max(k, 1)), dtype=np.float32)
        counts = np.zeros((b,), dtype=np.uint32)
        rc = self._lib.cqs_hip_index_search_tagged_multi(self._h, _ptr(q), b, qd, k, _ptr(a), mode, threshold,
                                                         _ptr(rows), _ptr(scores), _ptr(counts))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return rows[:, :k], scores[:, :k], counts

    def search_tagged(self, query: np.ndarray, k: int, allow) -> List[IndexResult]:
        """`search_with_filter` for a predicate over the rows' tags: no loop over the ids, no bitset.  Like `search`, never
        raises for device trouble (logs + []); that includes tags that do not cover the index."""
        if self.is_empty() or k == 0:
            return []
        query = np.asarray(query, dtype=np.float32).reshape(-1)
        if query.shape[0] != self.dim():
            log.warning("Query dimension mismatch expected_dim=%d actual_dim=%d", self.dim(), query.shape[0])
            return []
        if not np.all(np.isfinite(query)):
            return []
        k = min(k, self.max_k())
        try:
            rows, scores, counts = self.search_tagged_batch(query, k, allow)
        except HipError as e:
            log.error("HIP tagged search failed: %s", e)
            return []
        c = int(counts[0])
        return [IndexResult(self._id(int(rows[0, i])), float(scores[0, i])) for i in range(c)]

    def search(self, query: np.ndarray, k: int) -> List[IndexResult]:
        """`VectorIndex::search` (src/index.rs:146): sorted by score desc; never raises for device trouble."""
        if self.is_empty() or k == 0:
            return []
        query = np.asarray(query, dtype=np.float32).reshape(-1)
        if query.shape[0] != self.dim():
            log.warning("Query dimension mismatch expected_dim=%d actual_dim=%d", self.dim(), query.shape[0])
            return []
        if not np.all(np.isfinite(query)):
            log.warning("HIP query embedding contains non-finite values (NaN/Inf), returning empty results")
            return []
        k = min(k, self.max_k())
        try:
            rows, scores, counts = self.search_batch(query, k)
        except HipError as e:
            log.error("HIP search failed: %s", e)
            return []
        c = int(counts[0])
        return [IndexResult(self._id(int(rows[0, i])), float(scores[0, i])) for i in range(c)]

    def search_with_filter(self, query: np.ndarray, k: int, flt: Callable[[str], bool]) -> List[IndexResult]:
        """GPU-native filtered search: host builds the keep-bitset by evaluating the predicate per
        id (src/cagra.rs:747-757); all-pass -> unfiltered, none -> [], k capped at `included`
        (src/cagra.rs:760-775, done inside the C ABI)."""
        if self.is_empty() or k == 0:
            return []
        query = np.asarray(query, dtype=np.float32).reshape(-1)
        if query.shape[0] != self.dim():
            log.warning("Query dimension mismatch expected_dim=%d actual_dim=%d", self.dim(), query.shape[0])
            return []
        if not np.all(np.isfinite(query)):
            return []
        n = len(self)
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        keep = np.fromiter((bool(flt(self._id(base + i))) for i in range(n)), dtype=bool, count=n)
        bits = np.packbits(keep, bitorder="little")
        bits = np.concatenate([bits, np.zeros((-len(bits)) % 4, dtype=np.uint8)]).view(np.uint32)
        k = min(k, self.max_k())
        try:
            rows, scores, counts = self.search_batch(query, k, keep_bitset=bits)
        except HipError as e:
            log.error("HIP filtered search failed: %s", e)
            return []
        c = int(counts[0])
        return [IndexResult(self._id(int(rows[0, i])), float(scores[0, i])) for i in range(c)]

    def search_many_with_filters(self, queries: np.ndarray, k: int,
                                 filters: Sequence[Callable[[str], bool]]) -> List[List[IndexResult]]:
        """`search_with_filter` for a block of queries with a predicate each, in one call (the bitsets are built from
        `id_map` as `search_with_filter` builds its one).  A query of the wrong dimension or with a non-finite component
        gets []."""
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if len(filters) != q.shape[0]:
            raise ValueError("one filter per query")
        if self.is_empty() or k == 0 or q.shape[0] == 0:
            return [[] for _ in filters]
        if q.shape[1] != self.dim():
            log.warning("Query dimension mismatch expected_dim=%d actual_dim=%d", self.dim(), q.shape[1])
            return [[] for _ in filters]
        n = len(self)
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        ids = [self._id(base + i) for i in range(n)]
        bits = np.zeros((q.shape[0], (n + 31) // 32), dtype=np.uint32)
        for j, flt in enumerate(filters):
            keep = np.fromiter((bool(flt(cid)) for cid in ids), dtype=bool, count=n)
            packed = np.packbits(keep, bitorder="little")
            bits[j].view(np.uint8)[:len(packed)] = packed
        k = min(k, self.max_k())
        try:
            rows, scores, counts = self.search_batch_filtered(q, k, bits)
        except HipError as e:
            log.error("HIP filtered search failed: %s", e)
            return [[] for _ in filters]
        return [[IndexResult(self._id(int(rows[j, i])), float(scores[j, i])) for i in range(int(counts[j]))]
                for j in range(q.shape[0])]

    def _rows_by_id(self):
        """chunk id -> local row of an `id_map` index, built on first use and rebuilt after `extend`."""
        if not hasattr(self, "_row_of") or len(self._row_of) != len(self.id_map):
            self._row_of = {cid: i for i, cid in enumerate(self.id_map)}
        return self._row_of

    def neighbors_rows(self, target_row: int, limit: int):
        """`cqs_hip_index_neighbors`: (rows u64, scores f32) of the stored row's nearest neighbours, itself excluded."""
        rows = np.zeros((_lib.NEIGHBORS_MAX,), dtype=np.uint64)
        scores = np.zeros((_lib.NEIGHBORS_MAX,), dtype=np.float32)
        c = C.c_uint32()
        rc = self._lib.cqs_hip_index_neighbors(self._h, target_row, max(0, min(int(limit), 2**32 - 1)), _ptr(rows), _ptr(scores), C.byref(c))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return rows[:c.value], scores[:c.value]

    def find_neighbors(self, target_id: str, limit: int) -> List[IndexResult]:
        """`find_neighbors(store, target, limit)` (src/cli/commands/search/neighbors.rs:86-132) on the resident
        corpus: ids instead of `ChunkSummary`s (hydration stays with the store, :139-146).  Raises `KeyError`
        when the target is not indexed (the reference: "Could not load embedding for ..."), :98-106."""
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        if self.id_map is None:
            row = int(target_id)
            if not (base <= row < base + len(self)):
                raise KeyError(target_id)
        else:
            row_of = self._rows_by_id()
            if target_id not in row_of:
                raise KeyError(target_id)
            row = base + row_of[target_id]
        rows, scores = self.neighbors_rows(row, limit)
        return [IndexResult(self._id(int(r)), float(s)) for r, s in zip(rows, scores)]

    def knn_graph_rows(self, limit: int, first: int = 0, count: Optional[int] = None, rows_per_call: int = 4096):
        """`cqs_hip_index_knn_graph`: the neighbours of the `count` stored rows from the index's `first`-th on (default: to
        the end), each as `neighbors_rows` defines them.  Returns (rows u64 [count, L] global row ids, scores f32
        [count, L], counts u32 [count]) with L = clamp(limit, 1, 100); slots past a count are 0.  The range goes to the
        library in calls of `rows_per_call` targets cut at multiples of 256 rows - whole tiles, so no tile is scanned
        twice - and the answer does not depend on the cut; searches from other threads get the handle between calls."""
        n = len(self)
        first = int(first)
        count = n - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > n:
            raise ValueError("knn_graph_rows: range not in this index")
        lim = max(1, min(int(limit), _lib.NEIGHBORS_MAX))
        per = max(256, min(int(rows_per_call), _lib.KNN_MAX_TARGETS)) // 256 * 256
        rows = np.zeros((count, lim), dtype=np.uint64)
        scores = np.zeros((count, lim), dtype=np.float32)
        counts = np.zeros((count,), dtype=np.uint32)
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        at = first
        while at < first + count:
            stop = min(first + count, (at // per + 1) * per)
            o = at - first
            rc = self._lib.cqs_hip_index_knn_graph(self._h, base + at, stop - at, lim, _ptr(rows[o:]), _ptr(scores[o:]), _ptr(counts[o:]))
            if rc != _lib.OK:
                raise HipError(rc, self.last_error())
            at = stop
        return rows, scores, counts

    def knn_graph(self, limit: int) -> List[List[IndexResult]]:
        """The exact kNN graph of the index by chunk id: entry i is `find_neighbors(id of row i, limit)`."""
        rows, scores, counts = self.knn_graph_rows(limit)
        return [[IndexResult(self._id(int(rows[i, j])), float(scores[i, j])) for j in range(int(counts[i]))]
                for i in range(rows.shape[0])]

    def pca(self, n_components: int = 2, n_passes: Optional[int] = None, seed: int = 42):
        """`cqs_hip_index_pca`: the top principal axes of the stored rows by block subspace iteration on the device
        (include/cqs_hip.h "PCA of the stored rows").  Returns (mean f32 [dim], axes f32 [n_components, dim] orthonormal,
        largest variance first, variance f32 [n_components] as sklearn's explained_variance_, total_variance float: the
        trace of the covariance).  `n_passes` None: the default 16.  Raises HipError (INVALID: n_components not in
        [1, min(4, dim)], more than 64 passes, a row-sharded handle, fewer than 2 rows, non-finite rows)."""
        dim = self.dim()
        nc = max(0, min(int(n_components), _lib.PCA_MAX_COMPONENTS + 1))    # (one past the limit: the library refuses it)
        mean = np.zeros((dim,), dtype=np.float32)
        axes = np.zeros((max(nc, 1), dim), dtype=np.float32)
        var = np.zeros((max(nc, 1),), dtype=np.float32)
        total = C.c_float()
        rc = self._lib.cqs_hip_index_pca(self._h, nc, 0 if n_passes is None else max(0, min(int(n_passes), 2**32 - 1)),
                                         int(seed), _ptr(mean), _ptr(axes), _ptr(var), C.byref(total))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return mean, axes[:nc], var[:nc], float(total.value)

    def pca_project(self, mean, axes, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """`cqs_hip_index_pca_project`: (x - mean) . axes_k for the `count` stored rows from the index's `first`-th on
        (default: to the end), f32 [count, n_components].  `mean` [dim] and `axes` [n_components, dim] are what `pca`
        returns - of this index or of another of the same dimension."""
        mu = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
        ax = np.ascontiguousarray(axes, dtype=np.float32)
        if ax.ndim != 2 or ax.shape[1] != self.dim() or mu.shape[0] != self.dim():
            raise ValueError("pca_project: mean is [dim], axes is [n_components, dim]")
        n = len(self)
        first = int(first)
        count = n - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > n:
            raise ValueError("pca_project: range not in this index")
        out = np.zeros((count if ax.shape[0] <= _lib.PCA_MAX_COMPONENTS else 0, ax.shape[0]), dtype=np.float32)   # (more: the library refuses)
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        rc = self._lib.cqs_hip_index_pca_project(self._h, _ptr(mu), _ptr(ax), ax.shape[0], base + first, count, _ptr(out))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return out

    def umap_project(self, n_neighbors: int = 15, n_epochs: Optional[int] = None, seed: int = 42,
                     rows_per_call: int = 4096, *, init: str = "random") -> np.ndarray:
        """`cqs index --umap` on the resident corpus (src/cli/commands/index/umap.rs): the exact graph of
        `knn_graph_rows(n_neighbors - 1)` - umap-learn counts a point among its own neighbours - in calls of
        `rows_per_call` targets cut at multiples of 256, then a `HipLayout` (cqs_amd/umap.py) on this index's device run to
        its end.  Returns coordinates f32 [n, 2] in row order; fewer than 2 rows give the origin.  Raises what
        `knn_graph_rows` raises on a row-sharded handle.  `init="pca"` starts the layout from the scaled PCA projection of
        the rows (umap-learn's init="pca"; `cqs_hip_index_umap_project_init`, whose bytes this returns) instead of the
        hashed uniform coordinates: where the clusters end up relative to each other then follows the corpus."""
        from .umap import HipLayout, pca_initial_coords
        if init not in ("random", "pca"):
            raise ValueError("umap_project: init is 'random' or 'pca'")
        n = len(self)
        if n < 2:
            return np.zeros((n, 2), dtype=np.float32)
        if int(self._lib.cqs_hip_index_row_base(self._h)) != 0:
            raise ValueError("umap_project: the handle's row_base is not 0")
        start = None
        if init == "pca":
            mean, axes, _, _ = self.pca(min(2, self.dim()), None, seed)
            start = pca_initial_coords(self.pca_project(mean, axes), seed)
        rows, scores, counts = self.knn_graph_rows(int(n_neighbors) - 1, rows_per_call=rows_per_call)
        with HipLayout(rows, scores, counts, device=int(self._lib.cqs_hip_index_device(self._h)),
                       n_epochs=0 if n_epochs is None else int(n_epochs), seed=int(seed)) as lay:
            if start is not None:
                lay.set_coords(start)
            lay.run()
            return lay.coords()

    def umap_transform(self, xy, vectors, n_neighbors: int = 15, n_epochs: Optional[int] = None, seed: int = 42) -> np.ndarray:
        """`cqs_hip_index_umap_transform`: coordinates f32 [m, 2] for the new `vectors` [m, dim] in the layout `xy`
        [n_anchors, 2] of this index's first n_anchors rows, which do not move: each vector's `n_neighbors` nearest of
        those rows (the rows appended since, by `extend`, are masked out), then umap-learn's transform rules in one launch
        (include/cqs_hip.h "UMAP transform of new rows").  Call it after `extend` of new chunks - or before - and store the
        pairs beside the old ones.  Raises HipError on a row-sharded handle, a row_base other than 0 or more anchors than
        rows."""
        a = np.ascontiguousarray(xy, dtype=np.float32)
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("umap_transform: xy is [n_anchors, 2]")
        if v.ndim != 2 or v.shape[1] != self.dim():
            raise ValueError("umap_transform: vectors must be [m, dim]")
        m = v.shape[0]
        out = np.zeros((m, 2), dtype=np.float32)
        rc = self._lib.cqs_hip_index_umap_transform(self._h, a.shape[0], _ptr(a), _ptr(v), m, max(0, min(int(n_neighbors), 2**32 - 1)),
                                                    0 if n_epochs is None else int(n_epochs), int(seed), _ptr(out))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return out

    def umap_project_by_id(self, n_neighbors: int = 15, n_epochs: Optional[int] = None, seed: int = 42,
                           rows_per_call: int = 4096, *, init: str = "random") -> List[Tuple[str, float, float]]:
        """`umap_project` by chunk id, in row order: (id, x, y) - the triples the reference's script answers with."""
        xy = self.umap_project(n_neighbors, n_epochs, seed, rows_per_call, init=init)
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        return [(self._id(base + i), float(xy[i, 0]), float(xy[i, 1])) for i in range(xy.shape[0])]

    # ---- semantic diff of two resident indexes (src/diff.rs:99-246, src/drift.rs:51-120) ------------
    def diff_rows(self, other: "HipIndex", rows_a, rows_b, threshold: float, want_sims: bool = False):
        """`cqs_hip_index_diff`: pair i is (stored row `rows_a[i]` of this index, stored row `rows_b[i]` of `other`), global
        row ids.  Returns (mod_pairs u64: the indices of the pairs with sim < threshold, ascending; mod_sims f32: their
        sims; counts u64 [3]: modified, unchanged, undefined[; sims f32 [m] with `want_sims`]).  Raises HipError (INVALID:
        a row outside its index, different dims or devices, a sharded handle, a NaN threshold)."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint64).reshape(-1)
        rb = np.ascontiguousarray(rows_b, dtype=np.uint64).reshape(-1)
        if ra.shape[0] != rb.shape[0]:
            raise ValueError("one row of each index per pair")
        m = ra.shape[0]
        mod_pairs = np.zeros((m,), dtype=np.uint64)
        mod_sims = np.zeros((m,), dtype=np.float32)
        counts = np.zeros((3,), dtype=np.uint64)
        sims = np.zeros((m,), dtype=np.float32) if want_sims else None
        rc = self._lib.cqs_hip_index_diff(self._h, _ptr(ra), other._h, _ptr(rb), m, float(threshold), _ptr(sims),
                                          _ptr(mod_pairs), _ptr(mod_sims), _ptr(counts))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        c = int(counts[0])
        out = (mod_pairs[:c], mod_sims[:c], counts)
        return out + (sims,) if want_sims else out

    def _all_ids(self) -> List[str]:
        """The id of every stored row, in row order."""
        if self.id_map is not None:
            return self.id_map
        base = self._row_base()
        return [str(base + i) for i in range(len(self))]

    def _row_base(self) -> int:
        return int(self._lib.cqs_hip_index_row_base(self._h))

    def _match_block(self, other: "HipIndex", rows_a: np.ndarray, rows_b: np.ndarray):
        """One `cqs_hip_index_match` call: at most MATCH_MAX rows per side, positions local to the two blocks.  The one
        place `match_rows` touches the device (the CPU tests put a numpy stand-in here)."""
        m_a, m_b = rows_a.shape[0], rows_b.shape[0]
        best_a, score_a = np.full((m_a,), MATCH_NONE, dtype=np.uint64), np.zeros((m_a,), dtype=np.float32)
        best_b, score_b = np.full((m_b,), MATCH_NONE, dtype=np.uint64), np.zeros((m_b,), dtype=np.float32)
        rc = self._lib.cqs_hip_index_match(self._h, _ptr(rows_a) if m_a else None, m_a, other._h, _ptr(rows_b) if m_b else None, m_b,
                                           _ptr(best_a) if m_a else None, _ptr(score_a) if m_a else None,
                                           _ptr(best_b) if m_b else None, _ptr(score_b) if m_b else None)
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return best_a, score_a, best_b, score_b

    def match_rows(self, other: "HipIndex", rows_a, rows_b, block: int = _lib.MATCH_MAX):
        """`cqs_hip_index_match`: for the stored rows `rows_a` of this index and `rows_b` of `other` (global row ids, any
        order, repeats allowed) the best partner of every row on the other side by the f32 dot of the two stored rows.
        Returns (best_a u64 [m_a]: the position in rows_b, ties to the lowest, MATCH_NONE where there is no finite entry;
        score_a f32 [m_a]; best_b u64 [m_b]; score_b f32 [m_b]).  Lists longer than `block` (<= MATCH_MAX) are cut into
        blocks on both sides and the blocks' answers merged by `merge_best`, so any length works; a smaller `block` holds
        the two handles for a shorter time per call."""
        ra = np.ascontiguousarray(rows_a, dtype=np.uint64).reshape(-1)
        rb = np.ascontiguousarray(rows_b, dtype=np.uint64).reshape(-1)
        block = int(block)
        if not 1 <= block <= _lib.MATCH_MAX:
            raise ValueError(f"block must be in 1 .. {_lib.MATCH_MAX}")
        m_a, m_b = ra.shape[0], rb.shape[0]
        best_a, score_a = np.full((m_a,), MATCH_NONE, dtype=np.uint64), np.zeros((m_a,), dtype=np.float32)
        best_b, score_b = np.full((m_b,), MATCH_NONE, dtype=np.uint64), np.zeros((m_b,), dtype=np.float32)
        none = np.uint64(MATCH_NONE)
        for i0 in range(0, max(m_a, 1), block):
            for j0 in range(0, max(m_b, 1), block):
                ba, sa, bb, sb = self._match_block(other, ra[i0:i0 + block], rb[j0:j0 + block])
                ba[ba != none] += np.uint64(j0)
                bb[bb != none] += np.uint64(i0)
                merge_best(best_a[i0:i0 + block], score_a[i0:i0 + block], ba, sa)
                merge_best(best_b[j0:j0 + block], score_b[j0:j0 + block], bb, sb)
        return best_a, score_a, best_b, score_b

    def semantic_diff(self, other: "HipIndex", threshold: float, key: Optional[Callable[[str], object]] = None,
                      moved_threshold: Optional[float] = None) -> "DiffResult":
        """`semantic_diff(source_store, target_store, .., threshold, ..)` (src/diff.rs:99-246) with this index as the source
        and `other` as the target.  Ids are matched by `key(id)` (default: the id itself; the reference's ChunkKey is
        (file, name, chunk_type) without the line); of several ids with one key the last wins (:130-137).  `added`: in
        the target only; `removed`: in the source only; matched pairs go through `diff_rows`: `modified` holds the
        target's id and the similarity of those below the threshold, sorted by (similarity under the f32 total order
        ascending, entries without a similarity last, id) (:226-236); `unchanged_count` the rest.  Matching and sorting
        are string work and stay on the host; the cosines are computed where the rows lie.
        `moved_threshold` (default None: the result above, `moved` empty): the source's removed rows are matched against
        the target's added rows by `match_rows`; a removed and an added chunk that are each other's best partner with a
        similarity (the dot of the stored rows: the cosine on cosine indexes) at or above it become one `moved` entry
        and leave `added` and `removed`.  `moved` is sorted like `modified`: similarity ascending, then target id.  A
        NaN `moved_threshold` raises ValueError."""
        if moved_threshold is not None and moved_threshold != moved_threshold:
            raise ValueError("moved_threshold is NaN")
        src, tgt = self._all_ids(), other._all_ids()
        added, removed, matched = match_ids(src, tgt, key)
        ra = np.asarray([s for s, _ in matched], dtype=np.uint64) + np.uint64(self._row_base())
        rb = np.asarray([t for _, t in matched], dtype=np.uint64) + np.uint64(other._row_base())
        mod_pairs, mod_sims, counts = self.diff_rows(other, ra, rb, threshold)[:3]
        modified = [DiffEntry(tgt[matched[int(p)][1]], float(s)) for p, s in zip(mod_pairs, mod_sims)]
        moved: List[MovedEntry] = []
        if moved_threshold is not None and added and removed:
            best_a, score_a, best_b, _ = self.match_rows(other, np.asarray(removed, dtype=np.uint64) + np.uint64(self._row_base()),
                                                         np.asarray(added, dtype=np.uint64) + np.uint64(other._row_base()))
            pairs = mutual_pairs(best_a, score_a, best_b, moved_threshold)
            moved = sort_moved([MovedEntry(src[removed[i]], tgt[added[j]], float(score_a[i])) for i, j in pairs])
            gone_a, gone_b = {i for i, _ in pairs}, {j for _, j in pairs}
            removed = [s for i, s in enumerate(removed) if i not in gone_a]
            added = [t for j, t in enumerate(added) if j not in gone_b]
        return DiffResult([DiffEntry(tgt[t], None) for t in added], [DiffEntry(src[s], None) for s in removed],
                          sort_modified(modified), int(counts[1]), moved)

    def detect_drift(self, other: "HipIndex", threshold: float, min_drift: float) -> "DriftResult":
        """`detect_drift(ref_store, project_store, .., threshold, min_drift, ..)` (src/drift.rs:51-120) with this index as the
        reference and `other` as the project: the modified entries of `semantic_diff` as drift = 1.0 - similarity in f32,
        kept where drift >= min_drift, sorted by (drift descending, id)."""
        diff = self.semantic_diff(other, threshold)
        return DriftResult(float(threshold), float(min_drift), drift_entries(diff.modified, min_drift),
                           len(diff.modified) + diff.unchanged_count, diff.unchanged_count)

    # ---- cosine MMR over the resident rows (src/search/mmr.rs:59-126) ------------
    def pairwise_rows(self, rows) -> np.ndarray:
        """`cqs_hip_index_pairwise`: the [m, m] f32 dots of the stored rows `rows` (global row ids)."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        m = r.shape[0]
        out = np.zeros((m, m), dtype=np.float32)
        rc = self._lib.cqs_hip_index_pairwise(self._h, _ptr(r), m, _ptr(out))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return out

    def mmr_rows(self, rows, scores, limit: int, lam: float) -> np.ndarray:
        """`cqs_hip_index_mmr`: `mmr_rerank` over the candidates (global row ids `rows`, relevance `scores`) with the
        stored rows' dot as the similarity.  Returns the picked indices into the candidate list, in pick order."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
        if s.shape[0] != r.shape[0]:
            raise ValueError("one score per candidate row")
        m = r.shape[0]
        limit = max(0, min(int(limit), 2**32 - 1))
        picks = np.zeros((max(1, min(limit, m)),), dtype=np.uint32)
        c = C.c_uint32()
        rc = self._lib.cqs_hip_index_mmr(self._h, _ptr(r), _ptr(s), m, limit, float(lam), _ptr(picks), C.byref(c))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return picks[:c.value]

    def mmr_rerank(self, results: List[IndexResult], limit: int, lam: float) -> List[IndexResult]:
        """`mmr_rerank` (src/search/mmr.rs:59-126) over a result list of this index, cosine of the stored rows as the
        similarity: the picked results in pick order and nothing after them - the caller truncates to `limit` exactly as
        `finalize_results` does (src/search/query.rs:685-705).  Raises `KeyError` for an id this index does not hold;
        never raises for device trouble (logs and returns the first `limit` inputs, the reference's order without MMR)."""
        base = int(self._lib.cqs_hip_index_row_base(self._h))
        rows = np.zeros((len(results),), dtype=np.uint64)
        if self.id_map is None:
            for i, r in enumerate(results):
                try:
                    row = int(r.id)
                except ValueError:
                    raise KeyError(r.id)
                if not (base <= row < base + len(self)):
                    raise KeyError(r.id)
                rows[i] = row
        else:
            row_of = self._rows_by_id()
            for i, r in enumerate(results):
                if r.id not in row_of:
                    raise KeyError(r.id)
                rows[i] = base + row_of[r.id]
        limit = max(0, int(limit))
        try:
            picks = self.mmr_rows(rows, [r.score for r in results], limit, lam)
        except HipError as e:
            log.error("HIP MMR re-rank failed, keeping the relevance order: %s", e)
            return list(results[:limit])
        return [results[int(i)] for i in picks]

    def search_mmr(self, query: np.ndarray, pool_k: int, limit: int, lam: float) -> List[IndexResult]:
        """`search` for a pool of `pool_k`, then `mmr_rerank` of it down to `limit`."""
        return self.mmr_rerank(self.search(query, pool_k), limit, lam)

    # ---- device-resident path (bench, sharded search) ---------------------------
    def search_device(self, d_queries: int, b: int, k: int, d_out_keys: int, d_out_counts: int,
                      d_keep: int = 0, mode: int = _lib.MODE_RAW, threshold: float = 0.0, stream: int = 0) -> None:
        """Enqueue `cqs_hip_index_search_device` on `stream` (raw device pointers / hipStream_t as ints)."""
        rc = self._lib.cqs_hip_index_search_device(
            self._h, C.c_void_p(d_queries), b, k, C.c_void_p(d_keep) if d_keep else None, mode, threshold,
            C.c_void_p(d_out_keys), C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None)  # 0 -> NULL = null stream
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())

    def combine_stats(self) -> Tuple[int, int]:
        """(passes, queries) the handle's combining queue has run since it was made (`cqs_hip_index_combine_stats`)."""
        p, q = C.c_uint64(), C.c_uint64()
        self._lib.cqs_hip_index_combine_stats(self._h, C.byref(p), C.byref(q))
        return int(p.value), int(q.value)

    def combine_filter_stats(self) -> Tuple[int, int]:
        """(passes, queries) of the combining queue's blocks of callers with a bitset (`cqs_hip_index_combine_filter_stats`)."""
        p, q = C.c_uint64(), C.c_uint64()
        self._lib.cqs_hip_index_combine_filter_stats(self._h, C.byref(p), C.byref(q))
        return int(p.value), int(q.value)

    def combine_tagged_stats(self) -> Tuple[int, int]:
        """(passes, queries) of the combining queue's blocks of callers with a tag filter (`cqs_hip_index_combine_tagged_stats`)."""
        p, q = C.c_uint64(), C.c_uint64()
        self._lib.cqs_hip_index_combine_tagged_stats(self._h, C.byref(p), C.byref(q))
        return int(p.value), int(q.value)

    def set_bf16_scan(self, enable: bool) -> None:
        """Build / free the bf16 shadow of the corpus (`cqs_hip_index_set_bf16_scan`; create / load already build it from a
        1 GiB f32 corpus on, or at any size with CQS_HIP_SCAN_BF16=1).  Answers stay byte-identical; searches that run as
        gemv passes read half the bytes.  Raises HipError (INVALID: sharded handle, enable on a borrowed handle,
        dim % 8 != 0, dim > 2048, a finite row with a component >= 2^64; NOMEM); the index stays usable either way."""
        rc = self._lib.cqs_hip_index_set_bf16_scan(self._h, 1 if enable else 0)
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())

    def bf16_stats(self) -> Tuple[int, int, int]:
        """(shadow bytes, 0 = off; queries answered by the certified path; queries that fell back to the f32 scan)."""
        b, c, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._lib.cqs_hip_index_bf16_stats(self._h, C.byref(b), C.byref(c), C.byref(f))
        return int(b.value), int(c.value), int(f.value)

    def i8_stats(self) -> Tuple[int, int, int]:
        """(bytes of the shadow's int8 copy, 0 = not built; of bf16_stats' two counts, the queries whose block scanned it)."""
        b, c, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._lib.cqs_hip_index_i8_stats(self._h, C.byref(b), C.byref(c), C.byref(f))
        return int(b.value), int(c.value), int(f.value)

    def set_timing(self, on: bool) -> None:
        self._lib.cqs_hip_index_set_timing(self._h, 1 if on else 0)

    def scan_time(self) -> Tuple[int, float]:
        """(searches bracketed, summed scan-kernel milliseconds) since timing was enabled / last read."""
        n, ms = C.c_uint32(), C.c_double()
        rc = self._lib.cqs_hip_index_scan_time(self._h, C.byref(n), C.byref(ms))
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())
        return int(n.value), float(ms.value)


def unpack_keys(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Decode packed candidate keys -> (rows u64, scores f32) via the C ABI helper."""
    lib = _lib.load()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    rows = np.zeros(keys.shape, dtype=np.uint64)
    scores = np.zeros(keys.shape, dtype=np.float32)
    lib.cqs_hip_unpack_keys(_ptr(keys), keys.size, _ptr(rows), _ptr(scores))
    return rows, scores


def merge_keys(lists: np.ndarray, counts: np.ndarray, k: int) -> np.ndarray:
    """Host k-way merge of per-shard descending key lists ([n_lists, stride] u64) -> top-k keys."""
    lib = _lib.load()
    lists = np.ascontiguousarray(lists, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.zeros((k,), dtype=np.uint64)
    c = lib.cqs_hip_merge_keys(_ptr(lists), _ptr(counts), lists.shape[0], lists.shape[1], k, _ptr(out))
    return out[:c]


# ---- backend registration (src/index.rs:245-345) ------------------------------
@dataclass
class BackendContext:
    """src/index.rs:245-260: what a backend may look at when deciding to open."""

    cqs_dir: str
    store: object            # needs .dim, .chunk_count(), .embedding_batches(batch) -> iter[list[(id, vec)]]
    ef_search: Optional[int] = None
    hip_threshold: int = 5000  # same gate as CQS_CAGRA_THRESHOLD (src/cagra.rs:1683-1690)
    device: int = 0
    persist: bool = True       # CQS_CAGRA_PERSIST analogue (src/cagra.rs:1013)
    devices: Optional[Sequence[int]] = None   # CQS_HIP_DEVICES: shard the corpus over these GPUs (one process)


def dim_scaled_batch(baseline: int, dim: int, lo: int, hi: int) -> int:
    """src/limits.rs:292-300."""
    if dim == 0:
        return max(lo, min(baseline, hi))
    return max(lo, min(baseline * 1024 // dim, hi))


class HipBackend:
    """`IndexBackend` (src/index.rs:271-291) for the exact GPU index; modelled on
    `CagraBackend::try_open` (src/cagra.rs:1676-1802): `None` = not applicable
    (falls through to the next backend, then brute force, src/cli/store.rs:503-508)."""

    def name(self) -> str:
        return "hip"

    def priority(self) -> int:
        return 200  # above cagra (100) and tiered (150), src/index.rs:338-345

    def try_open(self, ctx: BackendContext) -> Optional[VectorIndex]:
        lib = _lib.load()
        n = ctx.store.chunk_count()
        if n < ctx.hip_threshold:
            return None
        if lib.cqs_hip_device_count() <= 0:
            return None
        dim = ctx.store.dim
        free, total = C.c_uint64(), C.c_uint64()
        devs = list(ctx.devices) if ctx.devices else [ctx.device]
        # gpu_available_for (src/cagra.rs:336-376) for EVERY device that will hold a shard: a device counted twice
        # (two shards on one GPU) must have room for both
        for d in sorted(set(devs)):
            if lib.cqs_hip_device_mem(d, C.byref(free), C.byref(total)) != _lib.OK:
                return None
            if n * dim * 4 * 1.25 * devs.count(d) / len(devs) > free.value:
                log.warning("HIP backend: corpus does not fit the memory of device %d, falling through", d)
                return None
        import os
        path = os.path.join(ctx.cqs_dir, "index.hipflat")
        if ctx.persist and os.path.exists(path):           # persisted first (src/cagra.rs:1726-1752)
            try:
                idx = HipIndex.load(path, dim, n, ctx.device, devices=ctx.devices)
                log.info("Vector index backend selected backend=hip source=persisted vectors=%d", len(idx))
                return idx
            except ValueError as e:
                log.warning("HIP persisted load failed, rebuilding from store: %s", e)
                HipIndex.delete_persisted(path)
        embeddings = []
        for batch in ctx.store.embedding_batches(dim_scaled_batch(10_000, dim, 500, 50_000)):
            embeddings.extend(batch)
        try:
            if ctx.devices:
                id_map, flat, _ = prepare_index_data(embeddings, dim)
                idx = HipIndex.build_sharded(id_map, flat, ctx.devices, DistanceMetric.Cosine)
            else:
                idx = HipIndex.build_from_embeddings(embeddings, dim, DistanceMetric.Cosine, ctx.device)
        except (ValueError, HipError) as e:
            log.warning("HIP backend build failed, falling through: %s", e)
            return None
        log.info("Vector index backend selected backend=hip source=rebuilt vectors=%d", len(idx))
        if ctx.persist and len(idx) == n:                  # best-effort save (src/cagra.rs:1786-1795)
            try:
                idx.save(path)
            except (HipError, OSError) as e:
                log.warning("Failed to persist HIP index (will rebuild next restart): %s", e)
        return idx
