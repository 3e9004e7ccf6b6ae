"""The PCA of the stored rows on the device (include/cqs_hip.h "PCA of the stored rows") against numpy's
f64 `eigh` and the numpy restatement of tests/pca_cases.py: accuracy on the recorded corpora and over the sizes at which
the pass kernel takes another path (slab edges, dims that are no multiple of 16 or 64, more than one column tile), few
passes against the restatement, purity (the answer is a function of the stored rows), the degenerate corpora, the
projection, every refusal, and the UMAP layout started from the PCA projection."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_cases as pc  # noqa: E402
import umap_cases as uc  # noqa: E402
from cqs_amd import DistanceMetric, HipError, HipIndex, _lib  # noqa: E402

pytestmark = pytest.mark.gpu
S = pc.SLAB


def _index(x):
    return HipIndex.build_from_flat(None, x, metric=DistanceMetric.DotProduct)


def _planted(n, dim, seed):
    rng = np.random.default_rng(seed)
    s = np.concatenate([[5.0, 3.0, 2.0], 0.5 * 0.9 ** np.arange(max(0, dim - 3))])[:dim]
    return (rng.standard_normal((n, dim)) * s + 0.2).astype(np.float32)


def _pca(x, nc=2, passes=None, seed=42):
    idx = _index(x)
    try:
        return idx.pca(nc, passes, seed)
    finally:
        idx.close()


def _check(x, got, restated, name, want_sin=True):
    """The device's errors against numpy f64 `eigh`, each held to max(100 x the restatement's own, the floor)."""
    k = min(2, x.shape[0] - 1, x.shape[1])
    sin, deficit, var, mean, ortho = pc.errors(x, got, k)
    rs, rd, rv = restated
    print(f"{name}: sin {sin:.2e} (restated {rs:.2e}) deficit {deficit:.2e} ({rd:.2e}) variance {var:.2e} ({rv:.2e}) mean {mean:.2e} ortho {ortho:.2e}")
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert deficit <= max(100.0 * rd, 1e-9), name
    assert var <= max(100.0 * rv, 1e-6), name
    if want_sin:
        assert sin <= max(100.0 * rs, 1e-5), name
    assert mean <= 1e-6, name
    assert ortho <= 1e-6, name
    for axis in got[1]:
        assert axis[int(np.argmax(np.abs(axis)))] > 0, name                     # the sign rule
    _, lam, _ = pc.exact(x)
    assert abs(got[3] - lam.sum()) <= 1e-6 * lam.sum(), name                    # f32 output of the covariance's trace


@pytest.mark.parametrize("name", sorted(pc.RESTATED))
def test_accuracy_on_the_recorded_corpora(hip, name):
    x = pc.corpora()[name]
    _check(x, _pca(x), pc.RESTATED[name], name, want_sin=name != "isotropic")   # no gap there: the deficit only


SIZES = [(2, 40), (3, 40), (S - 1, 40), (S, 40), (S + 1, 40), (2 * S + 3, 40), (2 * S + 3, 24), (2 * S + 3, 96), (2 * S + 3, 100),
         (2 * S + 3, 768), (S + 1, 1028), (S + 1, 4096), (37, 4)]


@pytest.mark.parametrize("n,dim", SIZES)
def test_accuracy_over_slab_edges_and_dims(hip, n, dim):
    """n around the slab constant, dims that are no multiple of 16 (24, 40, 100, 1028) or of 64, one past the column tile
    (1028) and the largest the index takes (4096: four tiles), dim < 8.  The corpus has a planted gap, so the restatement's
    own errors (computed here) are rounding only."""
    x = _planted(n, dim, 100 + n + dim)
    restated = pc.errors(x, pc.pca(x, min(2, dim)), min(2, n - 1, dim))[:3]
    _check(x, _pca(x, min(2, dim)), restated, f"{n}x{dim}")                       # (n == 2: k = 1, the angle of the one direction)


@pytest.mark.parametrize("passes", [1, 2, 4])
@pytest.mark.parametrize("name", ["ring", "planted_777x40"])
def test_few_passes_against_the_restatement(hip, name, passes):
    """Before convergence the answer still shows a wrong Y or S term, which 16 passes hide: both corpora have a mean offset
    (2 and 0.3), so dropping mu (x) S or c moves the captured variance by percents.  Device and restatement differ by their
    f32 summation order only; that noise is what RESTATED's variance column measures, so the captured variance is held to
    100 times it (floor 1e-6), relative to lambda_1 + lambda_2."""
    x = pc.corpora()[name]
    _, lam, _ = pc.exact(x)
    dev, ref = _pca(x, 2, passes), pc.pca(x, 2, passes)
    diff = abs(pc.captured(x, dev[1]) - pc.captured(x, ref[1])) / lam[:2].sum()
    print(f"{name} at {passes} passes: deficit {pc.deficit(x, dev[1], lam):.3e} (restated {pc.deficit(x, ref[1], lam):.3e}), captured differs {diff:.2e}")
    assert diff <= max(100.0 * pc.RESTATED[name][2], 1e-6)
    assert np.abs(dev[2].astype(np.float64) - ref[2].astype(np.float64)).max() <= max(100.0 * pc.RESTATED[name][2], 1e-6) * lam[0]


def _bytes(got):
    return got[0].tobytes() + got[1].tobytes() + got[2].tobytes() + np.float32(got[3]).tobytes()


def test_purity_the_answer_is_a_function_of_the_stored_rows(hip):
    x = _planted(2 * S + 3, 40, 7)
    n = len(x)
    idx = _index(x)
    first = idx.pca(3, 4, 9)
    assert _bytes(idx.pca(3, 4, 9)) == _bytes(first)                             # two calls
    assert _bytes(idx.pca(3, 4, 10)) != _bytes(first)                            # (the seed is an input)
    half = _index(x[:n // 2])
    half.extend(None, x[n // 2:])
    assert _bytes(half.pca(3, 4, 9)) == _bytes(first)                            # create + extend
    half.close()
    patched = x.copy()
    rows = np.array([0, 5, S - 1, S, 2 * S + 2], dtype=np.uint64)                # row 0 is the shift
    patched[rows.astype(np.int64)] = _planted(len(rows), 40, 8)
    assert idx.update_rows(rows, patched[rows.astype(np.int64)]) == len(rows)
    fresh = _index(patched)
    want = fresh.pca(3, 4, 9)
    fresh.close()
    assert _bytes(idx.pca(3, 4, 9)) == _bytes(want) != _bytes(first)             # after update: a fresh index of the rows
    gone = np.array([0, 7, S, 2 * S + 1], dtype=np.uint64)
    assert idx.remove_rows(gone) == len(gone)
    kept = np.delete(patched, gone.astype(np.int64), axis=0)
    fresh = _index(kept)
    want = fresh.pca(3, 4, 9)
    fresh.close()
    assert _bytes(idx.pca(3, 4, 9)) == _bytes(want)                              # after remove likewise
    idx.close()


def test_degenerate_corpora(hip):
    x = pc.identical()
    mean, axes, var, total = _pca(x)
    assert np.array_equal(mean, x[0]) and total == 0.0
    assert (var <= 1e-6 * float(x[0] @ x[0])).all() and np.isfinite(axes).all()
    assert np.abs(axes.astype(np.float64) @ axes.T.astype(np.float64) - np.eye(2)).max() <= 1e-6
    assert np.array_equal(axes, np.eye(24, dtype=np.float32)[:2])                 # the breakdown rule's unit vectors
    x = pc.rank_one()
    mean, axes, var, total = _pca(x)
    _, lam, vec = pc.exact(x)
    assert abs(var[0] - lam[0]) <= 1e-5 * lam[0] and var[1] <= 1e-6 * lam[0] and abs(abs(axes[0] @ vec[:, 0]) - 1) <= 1e-6
    assert np.isfinite(axes).all() and np.abs(axes.astype(np.float64) @ axes.T.astype(np.float64) - np.eye(2)).max() <= 1e-6
    x = _planted(50, 4, 3)                                                        # dim < 8: p = dim, every component
    got = _pca(x, 4, 1)
    _, lam, _ = pc.exact(x)
    assert np.abs(got[2].astype(np.float64) - lam).max() <= 1e-5 * lam[0]
    assert np.abs(got[1].astype(np.float64) @ got[1].T.astype(np.float64) - np.eye(4)).max() <= 1e-6


def test_pca_project(hip):
    x = _planted(2 * S + 3, 100, 5)
    idx = _index(x)
    mean, axes, _, _ = idx.pca(4)
    z = idx.pca_project(mean, axes)
    want, mass = pc.project(x, mean, axes)
    assert z.shape == (len(x), 4) and np.all(np.abs(z - want) <= 1e-5 * (1.0 + mass))
    for first, count in ((S - 3, 7), (0, 1), (2 * S + 2, 1), (S, S), (5, 0)):     # across a slab edge, the ends, nothing
        part = idx.pca_project(mean, axes, first, count)
        assert part.tobytes() == z[first:first + count].tobytes(), (first, count)
    one = idx.pca_project(mean, axes[:1])
    assert np.all(np.abs(one[:, 0] - want[:, 0]) <= 1e-5 * (1.0 + mass[:, 0]))
    out = np.full(8, 7.0, dtype=np.float32)                                       # m == 0: OK, nothing touched, nothing else asked
    assert idx._lib.cqs_hip_index_pca_project(idx._h, mean.ctypes.data, axes.ctypes.data, 4, 0, 0, out.ctypes.data) == _lib.OK
    assert idx._lib.cqs_hip_index_pca_project(idx._h, mean.ctypes.data, axes.ctypes.data, 9, 10 ** 9, 0, out.ctypes.data) == _lib.OK
    assert (out == 7.0).all()
    assert idx._lib.cqs_hip_index_pca_project(idx._h, None, None, 2, 10 ** 9, 0, None) == _lib.OK
    idx.close()
    based = HipIndex.build_from_flat(None, x[:50], metric=DistanceMetric.DotProduct, row_base=1000)    # global row ids
    z2 = np.zeros((3, 4), dtype=np.float32)
    assert based._lib.cqs_hip_index_pca_project(based._h, mean.ctypes.data, axes.ctypes.data, 4, 1010, 3, z2.ctypes.data) == _lib.OK
    assert z2.tobytes() == z[10:13].tobytes()
    z2[:] = 7.0                                                                   # a local row number is outside this index
    assert based._lib.cqs_hip_index_pca_project(based._h, mean.ctypes.data, axes.ctypes.data, 4, 10, 3, z2.ctypes.data) == _lib.ERR_INVALID
    assert (z2 == 7.0).all()
    based.close()


def test_every_refusal_leaves_outputs_and_handle_alone(hip):
    x = _planted(300, 8, 6)
    idx = _index(x)
    lib = idx._lib
    mean, axes, var, total = (np.full(8, 7.0, np.float32), np.full(5 * 8, 7.0, np.float32), np.full(5, 7.0, np.float32), np.full(1, 7.0, np.float32))
    untouched = lambda: all((a == 7.0).all() for a in (mean, axes, var, total))
    call = lambda h, nc, passes, m=mean, a=axes, v=var, t=total: lib.cqs_hip_index_pca(
        h, nc, passes, 42, None if m is None else m.ctypes.data, None if a is None else a.ctypes.data,
        None if v is None else v.ctypes.data, None if t is None else t.ctypes.data)
    assert call(None, 2, 0) == _lib.ERR_INVALID
    for kw, text in ((dict(m=None), "pca: null output buffer"), (dict(a=None), "pca: null output buffer"),
                     (dict(v=None), "pca: null output buffer"), (dict(t=None), "pca: null output buffer")):
        assert call(idx._h, 2, 0, **kw) == _lib.ERR_INVALID and idx.last_error() == text and untouched()
    for nc in (0, 5, 2 ** 32 - 1):
        assert call(idx._h, nc, 0) == _lib.ERR_INVALID and "n_components" in idx.last_error() and untouched()
    assert call(idx._h, 2, 65) == _lib.ERR_INVALID and idx.last_error() == "pca: more than 64 passes" and untouched()
    assert call(idx._h, 0, 65, m=None) == _lib.ERR_INVALID and idx.last_error() == "pca: null output buffer"     # the first in order
    narrow = _index(x[:, :4].copy())
    assert call(narrow._h, 5, 0) == _lib.ERR_INVALID and untouched()
    with pytest.raises(HipError, match="n_components"):
        narrow.pca(5)
    narrow.close()
    one = _index(x[:1])
    assert call(one._h, 1, 0) == _lib.ERR_INVALID and one.last_error() == "pca: fewer than 2 rows" and untouched()
    one.close()
    sharded = HipIndex.build_sharded(None, x, [0], metric=DistanceMetric.DotProduct)
    assert call(sharded._h, 2, 0) == _lib.ERR_INVALID and sharded.last_error() == "pca: not built for a row-sharded handle" and untouched()
    out = np.full((300, 2), 7.0, dtype=np.float32)
    proj = lambda h, m_, a_, nc, first, m, o=out: lib.cqs_hip_index_pca_project(
        h, None if m_ is None else m_.ctypes.data, None if a_ is None else a_.ctypes.data, nc, first, m, None if o is None else o.ctypes.data)
    good_mean, good_axes = np.zeros(8, np.float32), np.eye(8, dtype=np.float32)[:2].copy()
    assert proj(sharded._h, good_mean, good_axes, 2, 0, 10) == _lib.ERR_INVALID and "row-sharded" in sharded.last_error()
    xy = np.full((300, 2), 7.0, dtype=np.float32)
    assert lib.cqs_hip_index_umap_project_init(sharded._h, 15, 10, 42, 1, xy.ctypes.data) == _lib.ERR_INVALID and (xy == 7.0).all()
    assert sharded.search_batch(x[:2], 3)[2].tolist() == [3, 3]
    sharded.close()
    assert proj(None, good_mean, good_axes, 2, 0, 10) == _lib.ERR_INVALID
    for args, text in (((None, good_axes, 2, 0, 10), "null mean or axes"), ((good_mean, None, 2, 0, 10), "null mean or axes"),
                       ((good_mean, good_axes, 0, 0, 10), "n_components"), ((good_mean, good_axes, 5, 0, 10), "n_components"),
                       ((good_mean, good_axes, 2, 300, 1), "range not in this index"), ((good_mean, good_axes, 2, 0, 301), "range not in this index"),
                       ((good_mean, good_axes, 2, 299, 2 ** 64 - 1), "range not in this index")):
        assert proj(idx._h, *args) == _lib.ERR_INVALID and text in idx.last_error() and (out == 7.0).all(), text
    assert proj(idx._h, good_mean, good_axes, 2, 0, 10, None) == _lib.ERR_INVALID and "null output" in idx.last_error()
    assert lib.cqs_hip_index_umap_project_init(idx._h, 15, 10, 42, 2, xy.ctypes.data) == _lib.ERR_INVALID and (xy == 7.0).all()
    assert "unknown init" in idx.last_error()
    assert lib.cqs_hip_index_umap_project_init(idx._h, 15, 10001, 42, 1, xy.ctypes.data) == _lib.ERR_INVALID and (xy == 7.0).all()
    assert idx.last_error() == "layout: more than 10000 epochs"                  # refused before the passes, in the layout's words
    assert lib.cqs_hip_index_umap_project_init(idx._h, 15, 10001, 42, 0, xy.ctypes.data) == _lib.ERR_INVALID and (xy == 7.0).all()
    assert idx.last_error() == "layout: more than 10000 epochs"
    with pytest.raises(ValueError):
        idx.umap_project(15, 10, 42, init="spectral")
    assert idx._lib.cqs_hip_index_poisoned(idx._h) == 0
    rows, scores, counts = idx.search_batch(x[:3], 1)                            # the handle still searches
    assert rows[:, 0].tolist() == [int(np.argmax(x @ x[i])) for i in range(3)]
    assert idx.pca(2)[2][0] > 0
    idx.close()


def _filled(n, dim, nc=2):
    return (np.full(dim, 7.0, np.float32), np.full(nc * dim, 7.0, np.float32), np.full(nc, 7.0, np.float32), np.full(1, 7.0, np.float32),
            np.full((n, nc), 7.0, np.float32), np.full((n, 2), 7.0, np.float32))


@pytest.mark.parametrize("kind", ["nan_row", "inf_row", "nan_first_row", "rows_of_1e25", "rows_of_5e17"])
def test_non_finite_rows_are_refused_after_the_passes(hip, kind):
    """"pca: non-finite rows": the index does not screen its rows.  A NaN or inf anywhere refuses through the mean pass's
    squares, and so do finite rows of 1e25, whose total variance is past f32; finite rows of 5e17 have a total variance
    that fits and overflow only the f32 Y (Gram-Schmidt's breakdown rule puts unit vectors in its place on the way): they
    refuse through the Rayleigh values.  Nothing is written, the handle is not poisoned and still searches."""
    x = _planted(S + 5, 40, 12)
    if kind == "nan_row":
        x[S + 2, 7] = np.nan                                                      # in the short second slab
    elif kind == "inf_row":
        x[3, 0] = np.inf
    elif kind == "nan_first_row":
        x[0, 39] = np.nan                                                         # x_0, the shift of every sum
    elif kind == "rows_of_1e25":
        x *= np.float32(1e25)                                                     # the total variance itself is past f32
    else:
        x *= np.float32(5e17)                                                     # total variance about 1e37, a slab's Y about 6e39
        assert np.isfinite(np.float32(pc.exact(x)[1].sum()))
    idx = _index(x)
    lib = idx._lib
    mean, axes, var, total, proj, xy = _filled(len(x), 40)
    assert lib.cqs_hip_index_pca(idx._h, 2, 0, 42, mean.ctypes.data, axes.ctypes.data, var.ctypes.data, total.ctypes.data) == _lib.ERR_INVALID
    assert idx.last_error() == "pca: non-finite rows"
    assert all((a == 7.0).all() for a in (mean, axes, var, total)) and not idx.is_poisoned()
    assert lib.cqs_hip_index_pca(idx._h, 2, 1, 42, mean.ctypes.data, axes.ctypes.data, var.ctypes.data, total.ctypes.data) == _lib.ERR_INVALID
    assert all((a == 7.0).all() for a in (mean, axes, var, total))
    with pytest.raises(HipError, match="non-finite rows"):
        idx.pca(2)
    assert lib.cqs_hip_index_umap_project_init(idx._h, 15, 10, 42, _lib.UMAP_INIT_PCA, xy.ctypes.data) == _lib.ERR_INVALID   # pca's refusal is the call's
    assert (xy == 7.0).all() and idx.last_error() == "pca: non-finite rows" and not idx.is_poisoned()
    q = _planted(2, 40, 13)
    assert idx.search_batch(q, 3)[2].tolist() == [3, 3]                           # the handle still searches
    good = _planted(S + 5, 40, 12)                                                # ... and answers once the rows are finite again
    bad = np.unique(np.argwhere(~np.isfinite(x) | (np.abs(x) > 1e10))[:, 0]).astype(np.uint64)
    assert idx.update_rows(bad, good[bad.astype(np.int64)]) == len(bad)
    fresh = _index(good)
    assert _bytes(idx.pca(2)) == _bytes(fresh.pca(2))
    fresh.close()
    idx.close()


def test_a_poisoned_handle_answers_poisoned(hip):
    x = _planted(300, 8, 14)
    idx = _index(x)
    lib = idx._lib
    good_mean, good_axes, _, _ = idx.pca(2)
    hip.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_index_fail_next.restype = None
    hip.cqs_hip_debug_index_fail_next(idx._h)
    with pytest.raises(HipError):
        idx.search_batch(x[:9], 5)
    assert idx.is_poisoned()
    mean, axes, var, total, proj, xy = _filled(300, 8)
    assert lib.cqs_hip_index_pca(idx._h, 2, 0, 42, mean.ctypes.data, axes.ctypes.data, var.ctypes.data, total.ctypes.data) == _lib.ERR_POISONED
    assert lib.cqs_hip_index_pca_project(idx._h, good_mean.ctypes.data, good_axes.ctypes.data, 2, 0, 300, proj.ctypes.data) == _lib.ERR_POISONED
    assert lib.cqs_hip_index_pca_project(idx._h, good_mean.ctypes.data, good_axes.ctypes.data, 2, 0, 0, proj.ctypes.data) == _lib.ERR_POISONED
    assert lib.cqs_hip_index_umap_project_init(idx._h, 15, 10, 42, _lib.UMAP_INIT_PCA, xy.ctypes.data) == _lib.ERR_POISONED
    assert all((a == 7.0).all() for a in (mean, axes, var, total, proj, xy))
    with pytest.raises(HipError):
        idx.pca(2)
    with pytest.raises(HipError):
        idx.umap_project(15, 10, 42, init="pca")
    idx.close()


def _project_c(idx, n_neighbors, n_epochs, seed, init):
    out = np.full((len(idx), 2), 7.0, dtype=np.float32)
    assert idx._lib.cqs_hip_index_umap_project_init(idx._h, n_neighbors, n_epochs, seed, init, out.ctypes.data) == _lib.OK, idx.last_error()
    return out


def test_umap_init_random_is_umap_project_and_c_matches_python(hip):
    x, _ = pc.ring(3)
    idx = HipIndex.build_from_flat(None, x)
    old = idx.umap_project(15, 60, 3)
    assert _project_c(idx, 15, 60, 3, _lib.UMAP_INIT_RANDOM).tobytes() == old.tobytes()
    out = np.zeros_like(old)
    assert idx._lib.cqs_hip_index_umap_project(idx._h, 15, 60, 3, out.ctypes.data) == _lib.OK and out.tobytes() == old.tobytes()
    via_c, via_python = _project_c(idx, 15, 60, 3, _lib.UMAP_INIT_PCA), idx.umap_project(15, 60, 3, init="pca")
    assert via_c.tobytes() == via_python.tobytes() != old.tobytes()
    assert [t[1:] for t in idx.umap_project_by_id(15, 60, 3, init="pca")] == [(float(a), float(b)) for a, b in via_python]
    # zero epochs: the initial coordinates themselves, the shared helper's scaling of the device's projection
    mean, axes, _, _ = idx.pca(2, None, 3)
    from cqs_amd.umap import pca_initial_coords
    start = pca_initial_coords(idx.pca_project(mean, axes), 3)
    assert np.abs(start).max() <= 10.0002 and pc.global_rho(x, pc.ring(3)[1], start) >= 0.99
    idx.close()


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_umap_pca_init_keeps_the_global_arrangement(hip, seed):
    x, labels = pc.ring(seed)
    idx = HipIndex.build_from_flat(None, x)
    y = idx.umap_project(15, 200, seed, init="pca")
    idx.close()
    rho, kept, purity = pc.global_rho(x, labels, y), uc.preservation(x, y), uc.purity(labels, y)
    i = seed - 1
    print(f"seed {seed}: rho {rho:.3f} (restated {pc.RECORDED_PCA_RHO[i]}), kept {kept:.3f} ({pc.RECORDED_PCA_KEPT[i]}), purity {purity:.3f} ({pc.RECORDED_PCA_PURITY[i]})")
    assert np.isfinite(y).all()
    assert rho >= pc.RECORDED_PCA_RHO[i] - pc.RHO_MARGIN
    assert kept >= pc.RECORDED_PCA_KEPT[i] - 3 * uc.SPREAD
    assert abs(purity - pc.RECORDED_PCA_PURITY[i]) <= 0.03


def test_umap_pca_init_duplicates_and_the_fallback(hip):
    x, _ = pc.ring(4)
    x[100:110] = x[100]                                                           # ten copies of one row
    idx = HipIndex.build_from_flat(None, x)
    y = idx.umap_project(15, 100, 4, init="pca")
    idx.close()
    assert np.isfinite(y).all() and len({tuple(r) for r in y[100:110].tolist()}) == 10   # they do not stay coincident
    same = np.tile(x[:1], (64, 1))                                                # nothing to scale: the hashed coordinates
    idx = HipIndex.build_from_flat(None, same)
    fallback, hashed = _project_c(idx, 15, 20, 5, _lib.UMAP_INIT_PCA), _project_c(idx, 15, 20, 5, _lib.UMAP_INIT_RANDOM)
    assert np.isfinite(fallback).all() and fallback.tobytes() == hashed.tobytes()
    assert idx.umap_project(15, 20, 5, init="pca").tobytes() == hashed.tobytes()
    idx.close()
