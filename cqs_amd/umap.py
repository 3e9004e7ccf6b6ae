"""`HipLayout` - the UMAP layout of a kNN graph on the device (include/cqs_hip.h, "UMAP layout of a kNN graph").

The second half of `cqs index --umap` (src/cli/commands/index/umap.rs): the fuzzy-simplicial-set weights of the graph that
`HipIndex.knn_graph_rows` returns, and the epochs of force-directed layout.  The layout is its own handle: it takes the
graph, not the index, and holds no index while it runs.  `HipIndex.umap_project` is the two halves in one call."""
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


def _create_error(lib) -> str:
    buf = C.create_string_buffer(512)
    lib.cqs_hip_layout_last_error(None, buf, 512)
    return buf.value.decode(errors="replace")
