"""The UMAP layout on the device (include/cqs_hip.h "UMAP layout of a kNN graph") against the numpy
restatement of tests/umap_cases.py: the graph (structure exact, rho bit-equal, weights to 1e-4), single epochs from the
device's own graph and coordinates, determinism, the layout's quality on the four-cluster corpus, the Python surface."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import umap_cases as uc  # noqa: E402
from cqs_amd import HipError, HipIndex, _lib  # noqa: E402
from cqs_amd.umap import HipLayout  # noqa: E402

pytestmark = pytest.mark.gpu


def _pair(stride=1):
    rows = np.zeros((2, stride), dtype=np.uint64)
    rows[0, 0] = 1
    scores = np.full((2, stride), 0.75, dtype=np.float32)
    return rows, scores, np.ones(2, dtype=np.uint32)


def _hub_and_more():
    """The hub (500 spokes list vertex 0, which lists none) widened to stride 14 with ragged extra edges among the spokes."""
    rows, scores, counts = uc.hub_graph(500, 14)
    rng = np.random.default_rng(11)
    for i in range(1, 501, 3):
        extra = rng.choice(np.delete(np.arange(1, 501), i - 1), size=int(rng.integers(1, 14)), replace=False)
        c = len(extra)
        rows[i, 1:1 + c], counts[i] = extra, 1 + c
        scores[i, 1:1 + c] = np.sort(rng.uniform(-0.1, float(scores[i, 0]), c).astype(np.float32))[::-1]
    return rows, scores, counts


@pytest.fixture(scope="module")
def graphs(hip):
    """name -> (rows, scores, counts).  Shared and left unchanged."""
    x, _ = uc.clusters(7, n_clusters=3, per=100, dim=32)
    idx = HipIndex.build_from_flat(None, x)
    g = {"knn_300x32": idx.knn_graph_rows(14)}
    idx.close()
    g["pair_n2"] = _pair()
    g["pair_n2_stride100"] = _pair(100)
    g["repeated_rows_n65_stride14"] = uc.ragged_graph(5, 65, 14, dup_every=3, zero_vertex=5, empty_vertex=7)
    g["n65_stride1"] = uc.ragged_graph(7, 65, 1, empty_vertex=3)
    g["n257_stride100"] = uc.ragged_graph(6, 257, 100, dup_every=4, zero_vertex=256, empty_vertex=0)
    g["hub_n501_stride14"] = _hub_and_more()
    return g


GRAPHS = ["knn_300x32", "pair_n2", "pair_n2_stride100", "repeated_rows_n65_stride14", "n65_stride1", "n257_stride100",
          "hub_n501_stride14"]


@pytest.mark.parametrize("name", GRAPHS)
def test_graph_against_the_restatement(graphs, name):
    rows, scores, counts = graphs[name]
    off, nbr, w, rho, sigma, w_max = uc.graph(rows, scores, counts)
    with HipLayout(rows, scores, counts) as lay:
        d_off, d_nbr, d_w, d_rho, d_sigma, d_w_max = lay.graph()
        assert len(lay) == len(counts) and lay.edges == len(nbr)
    assert np.array_equal(d_off, off) and np.array_equal(d_nbr, nbr)                    # structure: exact
    assert np.array_equal(d_rho.view(np.uint32), rho.view(np.uint32))                   # a minimum of exactly restated f32
    # Both sides stop the bisection within 1e-5 of the target and all weights of a row move the same way with sigma, so a
    # row's weights differ by at most 2e-5 plus f32 rounding; 1e-4 is that with room for expf.
    err = np.abs(d_w.astype(np.float64) - w)
    print(f"{name}: worst weight error {err.max() if len(err) else 0.0:.3g}, worst relative sigma error "
          f"{np.max(np.abs(d_sigma - sigma) / np.maximum(sigma, 1e-300)) if len(sigma) else 0.0:.3g}")
    assert (err <= 1e-4).all()
    # both ends of every edge hold the same weight bits
    n = len(counts)
    vert = np.repeat(np.arange(n), np.diff(d_off.astype(np.int64)))
    at = {(int(i), int(j)): int(b) for i, j, b in zip(vert, d_nbr, d_w.view(np.uint32))}
    assert len(at) == len(d_nbr)
    assert all(at[(j, i)] == b for (i, j), b in at.items())
    want_max = d_w.max() if len(d_w) else np.float32(0.0)
    assert np.float32(d_w_max).view(np.uint32) == np.float32(want_max).view(np.uint32)   # bit for bit
    empty = np.nonzero(counts == 0)[0]
    assert (d_rho[empty] == 0).all() and (d_sigma[empty] == 0).all()


def _step_and_check(lay, graph, e, E, seed, **kw):
    """One device epoch from the device's own coordinates against the f64 restatement of the same step."""
    off, nbr, w, _, _, w_max = graph
    before = lay.coords()
    assert lay.run(1) == e
    after = lay.coords()
    want, mass = uc.epoch_sync(off, nbr, w, w_max, before, e, E, seed, **kw)
    # A term is at most 8 and f32 powf and division contribute a few ulp each: per vertex and coordinate the device may
    # differ from f64 by 1e-5 * (1 + the sum of |terms|), the sum taken from the restatement.
    err = np.abs(after.astype(np.float64) - want)
    bound = 1e-5 * (1.0 + mass)
    print(f"epoch {e}: worst error {err.max():.3g}, worst error / bound {np.max(err / bound):.3g}, moved {np.abs(want - before).max():.3g}")
    assert (err <= bound).all()
    return before, after, mass


@pytest.mark.parametrize("name", ["knn_300x32", "repeated_rows_n65_stride14", "hub_n501_stride14", "n257_stride100"])
def test_single_epochs_against_the_restatement(graphs, name):
    rows, scores, counts = graphs[name]
    seed, E = 1234, 10
    with HipLayout(rows, scores, counts, n_epochs=E, seed=seed) as lay, HipLayout(rows, scores, counts, n_epochs=E, seed=seed) as other:
        g = lay.graph()
        xy = lay.coords()
        assert np.array_equal(xy.view(np.uint32), uc.initial_coords(seed, len(counts)).view(np.uint32))
        # two coincident points that share an edge, and two points 100 apart, where the clip binds
        i = int(np.nonzero(counts)[0][0])
        j = int(rows[i, 0])
        xy[j] = xy[i]
        far = [v for v in range(len(counts)) if v not in (i, j)][:2]
        xy[far[1]] = xy[far[0]] + np.float32(100.0)
        lay.set_coords(xy)
        other.set_coords(xy)
        moved = 0.0
        for e in (1, 2, 3):
            before, after, mass = _step_and_check(lay, g, e, E, seed)
            moved = max(moved, float(mass.max()))
        assert moved > 4.0                                            # (terms were summed, and some were clipped ones)
        assert other.run(3) == 3                                      # the three epochs in one call: the same bytes
        assert np.array_equal(other.coords().view(np.uint32), lay.coords().view(np.uint32))


def test_a_draw_that_hits_its_own_vertex_counts_nothing(graphs):
    rows, scores, counts = graphs["pair_n2"]
    seed, E = 77, 10
    draws = uc.draw_vertex(uc.hash5(seed, 1, 0, 0, np.arange(5, dtype=np.uint32)), 2)
    assert (draws == 0).any() and (draws == 1).any()                  # vertex 0's first entry draws itself and the other
    with HipLayout(rows, scores, counts, n_epochs=E, seed=seed) as lay:
        g = lay.graph()
        assert lay.edges == 2 and g[5] == 1.0
        for e in (1, 2, 3):
            _step_and_check(lay, g, e, E, seed)
    # other parameters than the defaults reach the kernel
    kw = dict(a=np.float32(1.2), b=np.float32(0.7), lr=0.5, repulsion=2.0, negative_samples=3)
    with HipLayout(rows, scores, counts, n_epochs=E, seed=seed, a=1.2, b=0.7, learning_rate=0.5, repulsion=2.0, negative_samples=3) as lay:
        g = lay.graph()
        for e in (1, 2):
            _step_and_check(lay, g, e, E, seed, **kw)


def test_determinism(graphs):
    rows, scores, counts = graphs["knn_300x32"]
    with HipLayout(rows, scores, counts) as a, HipLayout(rows, scores, counts) as b, HipLayout(rows, scores, counts) as c:
        assert a.n_epochs == 500
        start = a.coords()
        c.set_coords(start)                                            # coords -> set_coords on a fresh handle at epoch 0
        assert a.run(1) == 1 and c.run(1) == 1
        assert np.array_equal(a.coords().view(np.uint32), c.coords().view(np.uint32))
        assert a.run(49) == 50
        assert b.run(20) == 20 and b.run(30) == 50
        assert np.array_equal(a.coords().view(np.uint32), b.coords().view(np.uint32))
        assert not np.array_equal(a.coords(), start) and np.isfinite(a.coords()).all()
        assert a.run(10 ** 6) == 500 and a.run(1) == 500               # clamped at n_epochs


def test_layout_quality_on_the_four_cluster_corpus(hip):
    x, labels = uc.clusters(1)
    idx = HipIndex.build_from_flat(None, x)
    got = idx.umap_project(n_neighbors=15, n_epochs=200, seed=42)
    rows, scores, counts = idx.knn_graph_rows(14)
    xy_c = np.zeros((len(x), 2), dtype=np.float32)
    assert hip.cqs_hip_index_umap_project(idx._h, 15, 200, 42, xy_c.ctypes.data) == _lib.OK
    idx.close()
    assert got.shape == (480, 2) and got.dtype == np.float32 and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), xy_c.view(np.uint32))   # the C entry point and the Python one: the same bytes
    off, nbr, w, _, _, w_max = uc.graph(rows, scores, counts)          # the same graph and seed, restated in f64
    y0 = uc.initial_coords(42, len(x))
    want = uc.layout_sync(off, nbr, w, w_max, y0, 200, 42)
    kept, kept_ref, kept_random = uc.preservation(x, got), uc.preservation(x, want), uc.preservation(x, y0)
    pure, pure_ref = uc.purity(labels, got), uc.purity(labels, want)
    print(f"15-NN kept: device {kept:.3f}, restatement {kept_ref:.3f}, random {kept_random:.3f}; purity: device {pure:.3f}, restatement {pure_ref:.3f}")
    assert kept >= kept_ref - 3 * uc.SPREAD                            # three times the restatement's own spread over seeds
    assert kept >= 5 * kept_random
    assert abs(pure - pure_ref) <= 0.01


def test_python_surface(hip):
    for n in (0, 1):
        idx = HipIndex.build_from_flat(None, uc.clusters(3, 1, 2, 32)[0][:n])
        xy = idx.umap_project()
        assert xy.shape == (n, 2) and xy.dtype == np.float32 and not xy.any()
        out = np.full((max(n, 1), 2), 7.0, dtype=np.float32)
        assert hip.cqs_hip_index_umap_project(idx._h, 15, 0, 42, out.ctypes.data) == _lib.OK and not out[:n].any()
        idx.close()
    x, _ = uc.clusters(3, 2, 20, 32)
    two = HipIndex.build_from_flat(None, x[:2])
    xy = two.umap_project(n_epochs=5)
    assert xy.shape == (2, 2) and np.isfinite(xy).all() and xy.any()
    two.close()
    ids = [f"chunk-{i}" for i in range(40)]
    named = HipIndex.build_from_flat(ids, x)
    xy = named.umap_project(n_neighbors=8, n_epochs=20, seed=5)
    by_id = named.umap_project_by_id(n_neighbors=8, n_epochs=20, seed=5)
    assert [t[0] for t in by_id] == ids                               # row order
    assert np.array_equal(np.array([[t[1], t[2]] for t in by_id], dtype=np.float32), xy)
    named.close()
    sharded = HipIndex.build_sharded(None, x, [0])
    with pytest.raises(HipError) as ei:
        sharded.umap_project()
    assert ei.value.code == _lib.ERR_INVALID and "row-sharded" in str(ei.value)
    out = np.full((40, 2), 7.0, dtype=np.float32)
    assert hip.cqs_hip_index_umap_project(sharded._h, 15, 0, 42, out.ctypes.data) == _lib.ERR_INVALID and (out == 7.0).all()
    sharded.close()
    # degenerate layouts and refusals through HipLayout
    none = np.zeros((1, 3), dtype=np.uint64), np.zeros((1, 3), dtype=np.float32), np.zeros(1, dtype=np.uint32)
    with HipLayout(*none) as lay:
        assert len(lay) == 1 and lay.edges == 0 and not lay.coords().any() and lay.run(7) == 7 and not lay.coords().any()
    with pytest.raises(HipError) as ei:
        HipLayout(np.array([[1], [1]], dtype=np.uint64), np.zeros((2, 1), np.float32), np.ones(2, np.uint32))
    assert ei.value.code == _lib.ERR_INVALID and "vertex 1 lists itself" in str(ei.value)
    with pytest.raises(HipError):
        HipLayout(*_pair(), n_epochs=10001)
