"""`HipLayout` - the UMAP layout of a kNN graph on the device (include/cqs_hip.h, "UMAP layout of a kNN graph").

The second half of `cqs index --umap` (src/cli/commands/index/umap.rs): the fuzzy-simplicial-set weights of the graph that
`HipIndex.knn_graph_rows` returns, and the epochs of force-directed layout.  The layout is its own handle: it takes the
graph, not the index, and holds no index while it runs.  `HipIndex.umap_project` is the two halves in one call.

`transform` / `HipLayout.transform` place new rows among coordinates that exist and do not move (include/cqs_hip.h, "UMAP
transform of new rows"): weights, initial position and all epochs in one launch.  `HipIndex.umap_transform` is the
neighbour search and that in one call."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .index import HipError, _ptr


def default_params() -> _lib.LayoutParams:
    """`cqs_hip_layout_params_default`: a, b of min_dist 0.1, learning rate 1, repulsion 1, 5 draws, default epochs, seed 42."""
    p = _lib.LayoutParams()
    _lib.load().cqs_hip_layout_params_default(C.byref(p))
    return p


class HipLayout:
    """One layout of one graph.  `rows` [n, stride] u64 / `scores` [n, stride] f32 / `counts` [n] u32 are what
    `HipIndex.knn_graph_rows` returns for the whole corpus of a handle with row_base 0.  Keyword arguments override the
    fields of `default_params()`.  Raises `HipError` with the refusal's text."""

    def __init__(self, rows, scores, counts, device: int = 0, **params):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        s = np.ascontiguousarray(scores, dtype=np.float32)
        c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if r.ndim != 2 or s.shape != r.shape or c.shape[0] != r.shape[0]:
            raise ValueError("HipLayout: rows and scores are [n, stride], counts is [n]")
        p = default_params()
        for k, v in params.items():
            if not hasattr(p, k):
                raise TypeError(f"HipLayout: no parameter {k!r}")
            setattr(p, k, v)
        h = C.c_void_p()
        rc = self._lib.cqs_hip_layout_create(int(device), r.shape[0], r.shape[1], _ptr(r), _ptr(s), _ptr(c), C.byref(p), C.byref(h))
        if rc != _lib.OK:
            raise HipError(rc, _create_error(self._lib))
        self._h = h

    def close(self) -> None:
        if self._h:
            self._lib.cqs_hip_layout_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self) -> int:
        return int(self._lib.cqs_hip_layout_len(self._h))

    @property
    def edges(self) -> int:
        """Adjacency entries: every undirected edge counts at both ends."""
        return int(self._lib.cqs_hip_layout_edges(self._h))

    @property
    def n_epochs(self) -> int:
        return int(self._lib.cqs_hip_layout_epochs(self._h))

    def last_error(self) -> str:
        buf = C.create_string_buffer(512)
        self._lib.cqs_hip_layout_last_error(self._h, buf, 512)
        return buf.value.decode(errors="replace")

    def _check(self, rc: int) -> None:
        if rc != _lib.OK:
            raise HipError(rc, self.last_error())

    def graph(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, float]:
        """(offsets u64 [n + 1], nbrs u32 [edges], weights f32 [edges], rho f32 [n], sigma f32 [n], w_max)."""
        n, e = len(self), self.edges
        off = np.zeros((n + 1,), dtype=np.uint64)
        nbr = np.zeros((e,), dtype=np.uint32)
        w = np.zeros((e,), dtype=np.float32)
        rho = np.zeros((n,), dtype=np.float32)
        sigma = np.zeros((n,), dtype=np.float32)
        w_max = C.c_float()
        self._check(self._lib.cqs_hip_layout_graph(self._h, _ptr(off), _ptr(nbr), _ptr(w), _ptr(rho), _ptr(sigma), C.byref(w_max)))
        return off, nbr, w, rho, sigma, float(w_max.value)

    def coords(self) -> np.ndarray:
        xy = np.zeros((len(self), 2), dtype=np.float32)
        self._check(self._lib.cqs_hip_layout_coords(self._h, _ptr(xy)))
        return xy

    def set_coords(self, xy) -> None:
        a = np.ascontiguousarray(xy, dtype=np.float32)
        if a.shape != (len(self), 2):
            raise ValueError("set_coords: xy is [n, 2]")
        self._check(self._lib.cqs_hip_layout_set_coords(self._h, _ptr(a)))

    def run(self, epochs: Optional[int] = None) -> int:
        """The next `epochs` epochs (default: all that are left), clamped at `n_epochs`.  Returns the epochs done so far."""
        after = C.c_uint32()
        todo = self.n_epochs if epochs is None else max(0, min(int(epochs), 2**32 - 1))
        self._check(self._lib.cqs_hip_layout_run(self._h, todo, C.byref(after)))
        return int(after.value)


    def transform(self, rows, scores, counts, id_base: Optional[int] = None, epochs: Optional[int] = None,
                  n_epochs: int = 0, want_weights: bool = False):
        """`cqs_hip_layout_transform`: coordinates f32 [m, 2] of m new vertices among this layout's current coordinates,
        which stay where they are (and on the device).  `rows` / `scores` [m, stride] and `counts` [m] are what
        `search_batch` of the new vectors at k = n_neighbors over the anchored rows returns; `id_base` (default: `len`) is
        the first new vertex's future row number; `epochs` runs only that many of the `n_epochs` epochs (0: the default
        for m).  With `want_weights` returns (xy, sigma f32 [m], weights f32 [m, stride])."""
        r, s, c = _lists(rows, scores, counts, "HipLayout.transform")
        first = len(self) if id_base is None else int(id_base)
        call = lambda at, stop, E, xy, sg, w: self._check(self._lib.cqs_hip_layout_transform(
            self._h, stop - at, r.shape[1], _ptr(r[at:stop]), _ptr(s[at:stop]), _ptr(c[at:stop]), E, first + at, _todo(epochs),
            _ptr(xy[at:stop]), None if sg is None else _ptr(sg[at:stop]), None if w is None else _ptr(w[at:stop])))
        return _in_calls(call, r, int(n_epochs), want_weights)


def _lists(rows, scores, counts, who):
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    s = np.ascontiguousarray(scores, dtype=np.float32)
    c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    if r.ndim != 2 or s.shape != r.shape or c.shape[0] != r.shape[0]:
        raise ValueError(f"{who}: rows and scores are [m, stride], counts is [m]")
    return r, s, c


def _todo(epochs: Optional[int]) -> int:
    return _lib.TRANSFORM_ALL if epochs is None else max(0, min(int(epochs), _lib.TRANSFORM_ALL))


def _in_calls(call, r, n_epochs: int, want_weights: bool):
    """m new vertices in calls of at most 65536 with matching ids.  A vertex's answer does not depend on the cut; the
    default epoch count does depend on m, so it is fixed here for the whole of it."""
    m = r.shape[0]
    E = n_epochs if n_epochs or m == 0 else (100 if m <= 10000 else 30)
    xy = np.zeros((m, 2), dtype=np.float32)
    sigma = np.zeros((m,), dtype=np.float32) if want_weights else None
    weights = np.zeros(r.shape, dtype=np.float32) if want_weights else None
    for at in range(0, m, _lib.KNN_MAX_TARGETS):
        call(at, min(m, at + _lib.KNN_MAX_TARGETS), E, xy, sigma, weights)
    return (xy, sigma, weights) if want_weights else xy


def transform(anchors_xy, rows, scores, counts, id_base: Optional[int] = None, epochs: Optional[int] = None,
              device: int = 0, want_weights: bool = False, **params):
    """`cqs_hip_umap_transform`, the handle-less transform: coordinates f32 [m, 2] of m new vertices among the fixed
    `anchors_xy` [n, 2] (uploaded per call).  Lists, `id_base` (default: n) and `epochs` as `HipLayout.transform` takes
    them; keyword arguments override the fields of `default_params()`.  Raises `HipError` with the refusal's text."""
    lib = _lib.load()
    a = np.ascontiguousarray(anchors_xy, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("transform: anchors_xy is [n, 2]")
    r, s, c = _lists(rows, scores, counts, "transform")
    p = default_params()
    for k, v in params.items():
        if not hasattr(p, k):
            raise TypeError(f"transform: no parameter {k!r}")
        setattr(p, k, v)
    first = a.shape[0] if id_base is None else int(id_base)

    def call(at, stop, E, xy, sg, w):
        p.n_epochs = E
        rc = lib.cqs_hip_umap_transform(int(device), a.shape[0], _ptr(a), stop - at, r.shape[1], _ptr(r[at:stop]), _ptr(s[at:stop]),
                                        _ptr(c[at:stop]), C.byref(p), first + at, _todo(epochs), _ptr(xy[at:stop]),
                                        None if sg is None else _ptr(sg[at:stop]), None if w is None else _ptr(w[at:stop]))
        if rc != _lib.OK:
            raise HipError(rc, _create_error(lib))

    return _in_calls(call, r, int(p.n_epochs), want_weights)


def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def _hash5(seed: int, epoch: int, vertex, slot: int, draw: int):
    """The header's hash(seed, epoch, vertex, slot, draw) over a u32 array of vertices."""
    seed = int(seed) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        h = _fmix32(np.asarray([(seed & 0xFFFFFFFF) ^ 0x9E3779B9], dtype=np.uint32))
        h = _fmix32(h ^ np.uint32(seed >> 32))
        h = _fmix32(h ^ np.uint32(epoch))
        h = _fmix32(h ^ np.asarray(vertex, dtype=np.uint32))
        h = _fmix32(h ^ np.uint32(slot))
        return _fmix32(h ^ np.uint32(draw))


def pca_initial_coords(proj, seed: int) -> Optional[np.ndarray]:
    """umap-learn's `noisy_scale_coords` as include/cqs_hip.h states it for `cqs_hip_index_umap_project_init`: `proj`
    [n, 1 or 2] f32 (what `HipIndex.pca_project` returns) -> xy [n, 2] f32 = proj * (10 / max|proj|) + jitter, every
    operation in f32 and rounded once, so the bytes are the C entry point's.  None where max|proj| is 0 or a projection
    is not finite: the layout keeps its hashed uniform coordinates."""
    p = np.ascontiguousarray(proj, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] not in (1, 2):
        raise ValueError("pca_initial_coords: proj is [n, 1] or [n, 2]")
    n = p.shape[0]
    mag = np.abs(p)
    if n == 0 or not np.isfinite(mag).all() or not mag.max() > 0:
        return None
    with np.errstate(over="ignore"):
        scale = np.float32(10.0) / mag.max()
    if not np.isfinite(scale):                                 # a denormal maximum
        return None
    xy = np.zeros((n, 2), dtype=np.float32)
    xy[:, :p.shape[1]] = p * scale
    v = np.arange(n, dtype=np.uint32)
    for c in (0, 1):
        u = (_hash5(seed, 0, v, 1, c) >> np.uint32(8)).astype(np.float32)
        jitter = (u * np.float32(1.0 / 16777216.0) - np.float32(0.5)) * np.float32(2e-4)
        xy[:, c] = xy[:, c] + jitter
    return xy


def _create_error(lib) -> str:
    buf = C.create_string_buffer(512)
    lib.cqs_hip_layout_last_error(None, buf, 512)
    return buf.value.decode(errors="replace")
