"""The UMAP transform on the device (include/cqs_hip.h "UMAP transform of new rows") against the numpy
restatement of tests/umap_transform_cases.py: weights and sigma to 1e-4, the initial position and single epochs from the
device's own weights and positions, bytes (repeat, cut, handle against handle-less, the epoch clamp), refusals through the
built library, the index call as a composition of `search_batch` and the handle-less transform, and the placement's
quality on the hold-out corpus.  Shapes are the smallest at which transform_kernel can still go wrong: m around its
workgroup of four waves, counts around a lane's two slots, n of 1 and 2, no draws, the last vertex ids."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import umap_cases as uc  # noqa: E402
import umap_transform_cases as tc  # noqa: E402
from cqs_amd import HipError, HipIndex, _lib  # noqa: E402
from cqs_amd import umap as hu  # noqa: E402
from cqs_amd.umap import HipLayout  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_COUNTS = (0, 1, 2, 14, 63, 64, 65, 100)


def _special_anchors(seed, n):
    """Anchors with every fourth one 100 away (large d2 in both coefficients, coordinates past 100), and two pairs of
    duplicates."""
    a = tc.random_anchors(seed, n)
    a[::4] += np.float32(100.0)
    a[5], a[9] = a[6], a[10]
    return a


def _special_lists(seed, n, m, stride):
    """Lists in which vertex 0 names both anchors of a duplicate pair, and vertices 1 and 2 name one anchor alone, so they
    start on it (d2 == 0 on the attraction)."""
    rows, scores, counts = tc.random_lists(seed, n, m, stride, counts=(stride, 1, 1, 3, stride - 1), dup_every=4, odd_vertex=3)
    rows[0, :4] = [5, 6, 9, 10]
    return rows, scores, counts


# name -> (anchors, rows, scores, counts, id_base, params).  Shared and left unchanged.
def _cases():
    c = {}
    add = lambda name, anchors, lists, id_base=None, **kw: c.__setitem__(name, (anchors,) + lists + (len(anchors) if id_base is None else id_base, kw))
    add("m1_n1_stride1", tc.random_anchors(1, 1), tc.random_lists(11, 1, 1, 1, counts=(1,)))
    add("m3_n2_stride15", tc.random_anchors(2, 2), tc.random_lists(12, 2, 3, 15, counts=(15, 2, 0)))
    add("m4_n1000_stride15", tc.random_anchors(3, 1000), tc.random_lists(13, 1000, 4, 15, counts=(15, 14, 1, 2), zero_vertex=3))
    add("m5_n1000_stride100", tc.random_anchors(4, 1000), tc.random_lists(14, 1000, 5, 100, counts=(100, 65, 64, 63, 0), dup_every=7))
    add("m9_n1000_stride100_last_ids", tc.random_anchors(5, 1000), tc.random_lists(15, 1000, 9, 100, counts=ALL_COUNTS, odd_vertex=7),
        id_base=2 ** 32 - 9)
    add("m9_n1000_stride15_no_draws", tc.random_anchors(6, 1000), tc.random_lists(16, 1000, 9, 15, counts=(15, 14, 2, 1, 0)),
        negative_samples=0)
    add("m257_n1000_stride100", tc.random_anchors(7, 1000), tc.random_lists(17, 1000, 257, 100, counts=ALL_COUNTS, zero_vertex=5,
                                                                           odd_vertex=15))
    add("m9_n1000_stride15_far_and_duplicate_anchors", _special_anchors(8, 1000), _special_lists(18, 1000, 9, 15))
    add("m5_n2_stride1_other_parameters", tc.random_anchors(9, 2), tc.random_lists(19, 2, 5, 1, counts=(1, 1, 0, 1, 1)),
        a=1.2, b=0.7, learning_rate=0.5, repulsion=2.0, negative_samples=3)
    return c


CASES = _cases()
E, SEED = 10, 1234


def _kw(params):
    """The library's parameter names -> the restatement's."""
    names = {"learning_rate": "lr"}
    return {names.get(k, k): (np.float32(v) if k in ("a", "b") else v) for k, v in params.items()}


def _device(name, epochs, want_weights=False):
    anchors, rows, scores, counts, id_base, params = CASES[name]
    return hu.transform(anchors, rows, scores, counts, id_base=id_base, epochs=epochs, want_weights=want_weights, n_epochs=E, seed=SEED,
                        **params)


@pytest.fixture(scope="module")
def start(hip):
    """name -> (xy at epochs = 0, sigma, weights) from the device, once."""
    return {name: _device(name, 0, want_weights=True) for name in CASES}


@pytest.mark.parametrize("name", list(CASES))
def test_weights_against_the_restatement(start, name):
    _, rows, scores, counts, _, _ = CASES[name]
    _, sigma, w = start[name]
    want_sigma, want_w = tc.weights(scores, counts)
    # Both sides stop the bisection within 1e-5 of the target and all weights of a list move the same way with sigma: the
    # project's bar for the layout's weights.
    err_w, err_s = np.abs(w.astype(np.float64) - want_w), np.abs(sigma.astype(np.float64) - want_sigma)
    print(f"{name}: worst weight error {err_w.max() if err_w.size else 0.0:.3g}, worst sigma error {err_s.max():.3g}")
    assert w.shape == scores.shape and sigma.shape == counts.shape
    assert (err_w <= 1e-4).all() and (err_s <= 1e-4).all()
    past = np.arange(scores.shape[1])[None, :] >= counts[:, None]
    assert (w[past] == 0).all() and (sigma[counts == 0] == 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_initial_position_against_the_restatement(start, name):
    anchors, rows, scores, counts, _, _ = CASES[name]
    xy, _, w = start[name]
    want, mass, placed = tc.initial(anchors, rows, counts, w)              # f64 over the device's own weights
    err, bound = np.abs(xy.astype(np.float64) - want), 1e-5 * (1.0 + mass)
    print(f"{name}: worst error {err.max():.3g}, worst error / bound {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    assert not xy[counts == 0].any()                                        # a count-0 vertex is (0, 0)
    one = counts == 1
    assert np.array_equal(xy[one], anchors[rows[one, 0].astype(np.int64)])  # a single-anchor vertex: equal in value to it
    assert placed[counts > 0].all() and np.isfinite(xy).all()


@pytest.mark.parametrize("name", ["m3_n2_stride15", "m5_n1000_stride100", "m9_n1000_stride100_last_ids", "m9_n1000_stride15_no_draws",
                                  "m257_n1000_stride100", "m9_n1000_stride15_far_and_duplicate_anchors",
                                  "m5_n2_stride1_other_parameters"])
def test_single_epochs_against_the_restatement(start, name):
    anchors, rows, scores, counts, id_base, params = CASES[name]
    before, _, w = start[name]
    _, _, placed = tc.initial(anchors, rows, counts, w)
    moved, clipped = 0.0, 0.0
    for e in (1, 2, 3):
        after = _device(name, e)
        # The device's own previous output and weights, so no active flag can differ; a term is at most 4 and f32 powf and
        # division contribute a few ulp each: 1e-5 * (1 + the sum of |terms|), the sum taken from the restatement.
        want, mass = tc.epoch(anchors, rows, counts, w, before, placed, e, E, SEED, id_base, **_kw(params))
        err, bound = np.abs(after.astype(np.float64) - want), 1e-5 * (1.0 + mass)
        print(f"{name} epoch {e}: worst error {err.max():.3g}, worst error / bound {np.max(err / bound):.3g}, moved {np.abs(want - before).max():.3g}")
        assert (err <= bound).all()
        moved, clipped = max(moved, float(np.abs(want - before).max())), max(clipped, float(mass.max()))
        assert not after[counts == 0].any()
        before = after
    assert moved > 0.0
    if name == "m5_n2_stride1_other_parameters":
        # The attraction decays with distance, so an anchor 100 away pulls weakly; the clip binds on a repulsion from
        # close by: here a vertex that has left its anchor by a little draws that anchor again.
        assert clipped >= 4.0
    if name == "m9_n1000_stride15_no_draws":
        one = counts == 1                                                   # on its anchor and nothing repels: it stays
        assert np.array_equal(before[one], anchors[rows[one, 0].astype(np.int64)])


def test_bytes(hip, start):
    name = "m257_n1000_stride100"
    anchors, rows, scores, counts, id_base, params = CASES[name]
    kw = dict(n_epochs=E, seed=SEED)
    whole = hu.transform(anchors, rows, scores, counts, **kw)
    assert np.array_equal(whole.view(np.uint32), hu.transform(anchors, rows, scores, counts, **kw).view(np.uint32))   # again
    assert not np.array_equal(whole, start[name][0]) and np.isfinite(whole).all()
    for cut in (1, 4, 5, 256):
        two = np.concatenate([hu.transform(anchors, rows[:cut], scores[:cut], counts[:cut], **kw),
                              hu.transform(anchors, rows[cut:], scores[cut:], counts[cut:], id_base=len(anchors) + cut, **kw)])
        assert np.array_equal(two.view(np.uint32), whole.view(np.uint32)), cut
    # `epochs` above E is E, and E is all of them; fewer is not
    assert np.array_equal(hu.transform(anchors, rows, scores, counts, epochs=E + 5, **kw).view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(hu.transform(anchors, rows, scores, counts, epochs=E, **kw).view(np.uint32), whole.view(np.uint32))
    assert not np.array_equal(hu.transform(anchors, rows, scores, counts, epochs=E - 1, **kw), whole)
    # the ids reach the hash
    assert not np.array_equal(hu.transform(anchors, rows, scores, counts, id_base=7, **kw), whole)


def test_layout_handle_against_the_handle_less_call(hip):
    g_rows, g_scores, g_counts = uc.ragged_graph(5, 65, 14, dup_every=3, empty_vertex=7)
    rows, scores, counts = tc.random_lists(31, 65, 9, 15, counts=(15, 14, 2, 1, 0))
    with HipLayout(g_rows, g_scores, g_counts, n_epochs=20, seed=SEED, negative_samples=3, repulsion=1.5) as lay:
        assert lay.run(3) == 3
        anchors = lay.coords()
        xy, sigma, w = lay.transform(rows, scores, counts, n_epochs=E, want_weights=True)
        want = hu.transform(anchors, rows, scores, counts, n_epochs=E, seed=SEED, negative_samples=3, repulsion=1.5, want_weights=True)
        for got_part, want_part in zip((xy, sigma, w), want):
            assert np.array_equal(got_part.view(np.uint32), want_part.view(np.uint32))
        assert np.array_equal(lay.transform(rows, scores, counts, n_epochs=E, id_base=1000, epochs=2).view(np.uint32),
                              hu.transform(anchors, rows, scores, counts, n_epochs=E, id_base=1000, epochs=2, seed=SEED,
                                           negative_samples=3, repulsion=1.5).view(np.uint32))
        assert lay.transform(rows[:0], scores[:0], counts[:0]).shape == (0, 2)
        # the handle is as it was: coordinates, epoch counter, and it still runs
        assert np.array_equal(lay.coords().view(np.uint32), anchors.view(np.uint32)) and len(lay) == 65
        assert lay.run(0) == 3 and lay.run(1) == 4


def _raw(hip, fn, head, rows, scores, counts, tail, m=None, stride=None, out=True):
    """One call through ctypes with 7.0-filled outputs: (rc, whether all three are still 7.0)."""
    m = len(counts) if m is None else m
    stride = rows.shape[1] if stride is None else stride
    xy, sigma, w = (np.full(s, 7.0, dtype=np.float32) for s in ((len(counts), 2), (len(counts),), rows.shape))
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = fn(*head, m, stride, ptr(rows), ptr(scores), ptr(counts), *tail, ptr(xy) if out else None, ptr(sigma), ptr(w))
    return rc, bool((xy == 7.0).all() and (sigma == 7.0).all() and (w == 7.0).all())


def test_refusals_leave_the_outputs_untouched(hip):
    anchors = tc.random_anchors(1, 4)
    rows = np.array([[1, 2], [0, 0], [0, 0], [3, 1]], dtype=np.uint64)
    scores = np.full((4, 2), 0.5, dtype=np.float32)
    counts = np.array([2, 1, 0, 2], dtype=np.uint32)
    p = hu.default_params()
    buf = C.create_string_buffer(256)
    text = lambda: (hip.cqs_hip_layout_last_error(None, buf, 256), buf.value.decode())[1]

    def free(why, n=4, a=anchors, r=rows, s=scores, c=counts, params=p, id_base=4, **kw):
        rc, untouched = _raw(hip, hip.cqs_hip_umap_transform, (0, n, None if a is None else a.ctypes.data), r, s, c,
                             (None if params is None else C.byref(params), id_base, _lib.TRANSFORM_ALL), **kw)
        assert rc == _lib.ERR_INVALID and untouched and text() == "transform: " + why, (why, rc, text())

    free("null params", params=None)
    free("null output buffer", out=False)
    free("null neighbour array", s=None)
    free("null anchors", a=None)
    free("no anchors", n=0)
    free("more than 2^31 anchors", n=2 ** 31 + 1)
    free("more than CQS_HIP_KNN_MAX_TARGETS new vertices", m=65537)
    free("id_base + m is greater than 2^32", id_base=2 ** 32 - 3)
    free("stride not in [1, CQS_HIP_NEIGHBORS_MAX]", stride=0)
    free("stride not in [1, CQS_HIP_NEIGHBORS_MAX]", stride=101)
    free("vertex 2 has a count greater than the stride", c=np.array([2, 1, 3, 2], dtype=np.uint32))
    free("vertex 3 lists a neighbour outside the anchors", r=np.array([[1, 2], [0, 0], [0, 0], [3, 4]], dtype=np.uint64))
    bad = hu.default_params()
    bad.a = float("nan")
    free("non-finite a, b, learning_rate or repulsion", params=bad)
    bad = hu.default_params()
    bad.b = 0.0
    free("a and b must be positive", params=bad)
    bad = hu.default_params()
    bad.n_epochs = 10001
    free("more than 10000 epochs", params=bad)
    free("null params", params=None, n=0, m=65537, stride=0)                  # together: the first in the order answers
    free("no anchors", n=0, m=65537, stride=0, id_base=2 ** 64 - 1)
    rc, untouched = _raw(hip, hip.cqs_hip_umap_transform, (0, 0, None), rows, scores, counts, (C.byref(p), 4, 0), m=0)
    assert rc == _lib.OK and untouched                                       # m == 0: OK, nothing written
    assert _raw(hip, hip.cqs_hip_umap_transform, (99, 4, anchors.ctypes.data), rows, scores, counts, (C.byref(p), 4, 0)) == (_lib.ERR_INVALID, True)
    assert text() == "transform: no such device"
    with pytest.raises(HipError) as ei:
        hu.transform(anchors, rows, scores, counts, n_epochs=10001)
    assert ei.value.code == _lib.ERR_INVALID and "more than 10000 epochs" in str(ei.value)
    with pytest.raises(TypeError):
        hu.transform(anchors, rows, scores, counts, no_such_parameter=1)

    # the same plan behind a layout handle; then a poisoned layout refuses
    hip.cqs_hip_debug_layout_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_layout_fail_next.restype = None
    g_rows, g_scores, g_counts = uc.ragged_graph(7, 4, 2)
    with HipLayout(g_rows, g_scores, g_counts) as lay:
        held = lambda r=rows, c=counts, n_epochs=0, id_base=4, **kw: _raw(hip, hip.cqs_hip_layout_transform, (lay._h,), r, scores, c,
                                                                          (n_epochs, id_base, _lib.TRANSFORM_ALL), **kw)
        assert held(out=False) == (_lib.ERR_INVALID, True) and lay.last_error() == "transform: null output buffer"
        assert held(r=np.array([[1, 2], [0, 0], [0, 0], [3, 4]], dtype=np.uint64)) == (_lib.ERR_INVALID, True)
        assert lay.last_error() == "transform: vertex 3 lists a neighbour outside the anchors"
        assert held(n_epochs=10001) == (_lib.ERR_INVALID, True) and lay.last_error() == "transform: more than 10000 epochs"
        assert held(id_base=2 ** 32 - 3) == (_lib.ERR_INVALID, True)
        with pytest.raises(HipError) as ei:
            lay.transform(rows, scores, np.array([2, 1, 3, 2], dtype=np.uint32))
        assert "vertex 2 has a count greater than the stride" in str(ei.value)
        assert held()[0] == _lib.OK                                           # refusals do not poison
        hip.cqs_hip_debug_layout_fail_next(lay._h)
        assert held() == (_lib.ERR_DEVICE, True)                              # an injected failure, before any device work
        assert held() == (_lib.ERR_POISONED, True)
        with pytest.raises(HipError) as ei:
            lay.coords()
        assert ei.value.code == _lib.ERR_POISONED
    with HipLayout(np.zeros((0, 1), np.uint64), np.zeros((0, 1), np.float32), np.zeros(0, np.uint32)) as none:
        with pytest.raises(HipError) as ei:
            none.transform(rows, scores, counts)
        assert "no anchors" in str(ei.value)


@pytest.fixture(scope="module")
def corpus(hip):
    """The 400 + 80 hold-out split of seed 1 (no restated layout: the anchors' coordinates come from the device)."""
    return tc.split(1)


def test_index_call_is_search_then_transform(hip, corpus):
    xa, _, xn, _ = corpus
    idx = HipIndex.build_from_flat(None, xa)
    xy = idx.umap_project(n_neighbors=15, n_epochs=50, seed=3)
    got = idx.umap_transform(xy, xn, n_neighbors=15, n_epochs=E, seed=SEED)
    rows, scores, counts = idx.search_batch(xn, 15)
    assert (counts == 15).all() and got.shape == (80, 2) and got.dtype == np.float32
    want = hu.transform(xy, rows, scores, counts, id_base=400, n_epochs=E, seed=SEED)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    out = np.zeros((80, 2), dtype=np.float32)                                  # the C entry point, default epochs
    assert hip.cqs_hip_index_umap_transform(idx._h, 400, xy.ctypes.data, xn.ctypes.data, 80, 15, 0, 42, out.ctypes.data) == _lib.OK
    assert np.array_equal(out.view(np.uint32), idx.umap_transform(xy, xn).view(np.uint32))
    assert np.array_equal(out.view(np.uint32), hu.transform(xy, rows, scores, counts, n_epochs=100).view(np.uint32))
    # after `extend` of the new rows the anchors are the first 400: the filtered search's bitset keeps the rest out
    idx.extend(None, xn)
    assert len(idx) == 480
    got = idx.umap_transform(xy, xn, n_neighbors=15, n_epochs=E, seed=SEED)
    bits = np.zeros(15, dtype=np.uint32)
    bits.view(np.uint8)[:60] = np.packbits(np.arange(480) < 400, bitorder="little")
    rows, scores, counts = idx.search_batch(xn, 15, keep_bitset=bits)
    assert (counts == 15).all() and rows.max() < 400
    want = hu.transform(xy, rows, scores, counts, id_base=400, n_epochs=E, seed=SEED)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # refusals: the output stays, the reason is the index's, and the handle still searches
    out = np.full((80, 2), 7.0, dtype=np.float32)
    big = np.zeros((481, 2), dtype=np.float32)
    assert hip.cqs_hip_index_umap_transform(idx._h, 481, big.ctypes.data, xn.ctypes.data, 80, 15, 0, 42, out.ctypes.data) == _lib.ERR_INVALID
    assert (out == 7.0).all() and "more anchors than the index has rows" in idx.last_error()
    assert idx.umap_transform(xy, xn[:0]).shape == (0, 2)
    rows2, _, _ = idx.search_batch(xn, 15, keep_bitset=bits)
    assert np.array_equal(rows2, rows)
    idx.close()
    sharded = HipIndex.build_sharded(None, xa, [0])
    with pytest.raises(HipError) as ei:
        sharded.umap_transform(xy, xn)
    assert ei.value.code == _lib.ERR_INVALID and "row-sharded" in str(ei.value)
    assert hip.cqs_hip_index_umap_transform(sharded._h, 400, xy.ctypes.data, xn.ctypes.data, 80, 15, 0, 42, out.ctypes.data) == _lib.ERR_INVALID
    assert (out == 7.0).all() and (sharded.search_batch(xn[:3], 5)[2] == 5).all()
    sharded.close()
    based = HipIndex.build_from_flat(None, xa, row_base=5)
    with pytest.raises(HipError) as ei:
        based.umap_transform(xy, xn)
    assert ei.value.code == _lib.ERR_INVALID and "row_base" in str(ei.value)
    assert (based.search_batch(xn[:3], 5)[2] == 5).all()
    based.close()


def test_placement_quality_on_the_hold_out_corpus(hip, corpus):
    xa, la, xn, ln = corpus
    idx = HipIndex.build_from_flat(None, xa)
    anchors = idx.umap_project(n_neighbors=15, n_epochs=200, seed=1)
    got = idx.umap_transform(anchors, xn, n_neighbors=15, n_epochs=100, seed=1)
    rows, scores, counts = idx.search_batch(xn, 15)
    idx.close()
    want = tc.transform(anchors, rows, scores, counts, n_epochs=100, seed=1)  # the same anchors and lists, restated in f64
    kept, kept_ref = tc.kept(rows, anchors, got), tc.kept(rows, anchors, want)
    pure, pure_ref = tc.purity(la, ln, anchors, got), tc.purity(la, ln, anchors, want)
    print(f"kept: device {kept:.3f}, restatement {kept_ref:.3f}; purity: device {pure:.3f}, restatement {pure_ref:.3f}")
    assert np.isfinite(got).all()
    assert kept >= kept_ref - 3 * tc.KEPT_SPREAD                               # three times the restatement's spread over seeds
    assert pure >= pure_ref - 3 * tc.PURITY_SPREAD
