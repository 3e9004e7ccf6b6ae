"""`cqs_hip_index_knn_graph` / `HipIndex.knn_graph_rows` / `HipIndex.knn_graph` (include/cqs_hip.h): the
neighbours of many stored rows in one call.

Four yardsticks, none of them the code under test: the integer Gram matrix of a dyadic corpus (tests/knn_cases.py: every
score an exact f32 whatever the kernel, so the whole graph is compared bit for bit, duplicate runs that hide the target
included); the library's own search of a tile's rows with the target dropped on the host, and `neighbors_rows`, whose
bytes the contract promises; the graph of the same range asked for in other cuts; the oracle's find_neighbors at the
parity tolerance.  The helper itself is held to the oracle in the one test here that needs no GPU.  Run on an MI355X with
`pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import knn_cases as kc
from cqs_amd import DistanceMetric, HipError, HipIndex, _lib, synth
from parity import SCORE_TOL, assert_topk_parity

gpu = pytest.mark.gpu
TILE = 256
BASES = (0, 5000)


def test_expected_graph_is_the_oracles_find_neighbors(oracle):
    """The helper against find_neighbors on the CPU: on exact data the reference's left-to-right f32 sum is the integer
    total too, so ids and score bits are equal, ties and hidden targets included."""
    for n, dim, limits in ((1, 64, (15,)), (2, 64, (1, 15)), (5, 64, (0, 1, 15)), (259, 64, (1, 15, 101)), (259, 768, (100,))):
        for dot in (False, True):
            case = kc.dyadic(n, dim, dot)
            for limit in limits:
                rows, scores, counts = kc.expected_graph(case, limit)
                assert (counts == min(kc.clamp(limit), n - 1)).all()
                first, length = case.run
                targets = set(range(0, n, 37)) | set(range(first, first + length, 13)) | set(kc.hidden_targets(case, limit)[-3:]) | {n - 1}
                for t in sorted(targets):
                    ids, sc = oracle.find_neighbors(case.rows, t, limit)
                    c = int(counts[t])
                    assert len(ids) == c and np.array_equal(ids, rows[t, :c]), (n, dim, dot, limit, t)
                    assert np.array_equal(sc.view(np.uint32), scores[t, :c].view(np.uint32)), (n, dim, dot, limit, t)
    assert kc.hidden_targets(kc.dyadic(700, 64), 100) == list(range(301, 305))      # the run does hide targets at k1 = 101
    assert kc.hidden_targets(kc.dyadic(5, 64), 1) == [3] and kc.hidden_targets(kc.dyadic(5, 64), 15) == []


def graph_call(idx, first, m, limit, fill=0):
    """One call of the C entry point over global rows [first, first + m): (rc, rows [m, L], scores, counts)."""
    L = kc.clamp(limit)
    rows = np.full((m, L), fill, dtype=np.uint64)
    scores = np.full((m, L), fill, dtype=np.float32)
    counts = np.full((m,), fill, dtype=np.uint32)
    rc = idx._lib.cqs_hip_index_knn_graph(idx._h, first, m, max(0, int(limit)), rows.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    return rc, rows, scores, counts


def assert_graph_equal(got, want, ctx=""):
    """Every byte: all L slots of every target (zeros past the count) and the counts."""
    (ra, sa, ca), (rb, sb, cb) = got, want
    assert ra.shape == rb.shape and np.array_equal(ca, cb), (ctx, ca.tolist()[:8], cb.tolist()[:8])
    bad = np.flatnonzero((ra != rb).any(axis=1) | (sa.view(np.uint32) != sb.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (ctx, "targets that differ", bad[:8].tolist(), ra[bad[0]].tolist(), rb[bad[0]].tolist())


def composed(idx, flat, base, limit, lo, hi):
    """The composition the call replaces, for the tile of local rows [lo, hi): one host search of its rows at k1, the
    target dropped on the host."""
    L = kc.clamp(limit)
    k1 = min(L + 1, len(idx))
    r, s, c = idx.search_batch(flat[lo:hi], k1)
    return kc.drop_self(r, s, c, base + np.arange(lo, hi), L)


def assert_composition(idx, flat, base, limit, ctx=""):
    got = idx.knn_graph_rows(limit)
    for lo in range(0, len(idx), TILE):
        hi = min(lo + TILE, len(idx))
        assert_graph_equal(tuple(a[lo:hi] for a in got), composed(idx, flat, base, limit, lo, hi), (ctx, "tile", lo))
    return got


# ---- exact data: the graph bit for bit ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dim", kc.DIMS)
@pytest.mark.parametrize("n", kc.SIZES)
def test_graph_is_exact_on_dyadic_corpora(hip, n, dim):
    for dot in (False, True):
        case = kc.dyadic(n, dim, dot)
        for base in BASES:
            idx = HipIndex.build_from_flat(None, case.rows, DistanceMetric.DotProduct if dot else DistanceMetric.Cosine, row_base=base)
            for limit in kc.LIMITS:
                want = kc.expected_graph(case, limit, base)
                got = idx.knn_graph_rows(limit)
                assert got[0].shape == (n, kc.clamp(limit))
                assert_graph_equal(got, want, (n, dim, dot, base, limit))
                for t in kc.hidden_targets(case, limit)[-2:]:                 # (named, so a failure says which case it is)
                    assert base + t not in got[0][t] and got[2][t] == min(kc.clamp(limit), n - 1)
            idx.close()


# ---- composition on Gaussian unit rows ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dim", kc.DIMS)
def test_graph_is_the_search_of_each_tile_with_the_target_dropped(hip, dim):
    flat = synth.gaussian_unit(700, dim=dim, seed=41)
    for base in BASES:
        idx = HipIndex.build_from_flat(None, flat, row_base=base)
        for limit in (1, 15, 100):
            r, s, c = assert_composition(idx, flat, base, limit, (dim, base, limit))
            assert (c == kc.clamp(limit)).all() and not (r == (base + np.arange(700))[:, None]).any()
        idx.close()


@gpu
@pytest.mark.parametrize("dim", kc.DIMS)
def test_ragged_tile_of_at_most_8_rows_is_neighbors(hip, dim):
    flat = synth.gaussian_unit(259, dim=dim, seed=43)
    idx = HipIndex.build_from_flat(None, flat, row_base=5000)
    for limit in (1, 15, 100):
        r, s, c = idx.knn_graph_rows(limit)
        for t in (256, 257, 258):
            nr, ns = idx.neighbors_rows(5000 + t, limit)
            assert int(c[t]) == len(nr) == kc.clamp(limit)
            assert np.array_equal(r[t], nr) and np.array_equal(s[t].view(np.uint32), ns.view(np.uint32)), (dim, limit, t)
    idx.close()


# ---- cut independence --------------------------------------------------------------------------------------------------
@gpu
def test_answer_does_not_depend_on_how_the_range_is_cut(hip):
    n, base, limit = 700, 5000, 15
    flat = synth.gaussian_unit(n, dim=64, seed=47)
    idx = HipIndex.build_from_flat(None, flat, row_base=base)
    rc, *whole = graph_call(idx, base, n, limit)
    assert rc == _lib.OK
    rng = np.random.default_rng(5)
    cuts = [[1], [255], [256], [257], [1, 255, 256, 257, 511, 512, 513, 699], sorted(rng.choice(np.arange(1, n), 9, replace=False).tolist()),
            list(range(1, n, 97))]
    for cut in cuts:
        edges = [0] + cut + [n]
        parts = []
        for a, z in zip(edges[:-1], edges[1:]):
            rc, *part = graph_call(idx, base + a, z - a, limit)
            assert rc == _lib.OK, idx.last_error()
            parts.append(part)
        assert_graph_equal(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), tuple(whole), cut)
    # the Python mirror's own cuts (calls of 256 and of 512 targets, from an unaligned start)
    for per in (256, 512):
        got = idx.knn_graph_rows(limit, first=100, count=555, rows_per_call=per)
        assert_graph_equal(got, tuple(a[100:655] for a in whole), per)
    assert [len(x) for x in idx.knn_graph_rows(limit, first=700)] == [0, 0, 0]
    idx.close()


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@gpu
def test_every_target_matches_the_oracles_find_neighbors(hip, oracle):
    n, limit = 700, 15
    flat = synth.gaussian_unit(n, dim=768, seed=53)
    idx = HipIndex.build_from_flat(None, flat)
    r, s, c = idx.knn_graph_rows(limit)
    idx.close()
    for t in range(n):                                                        # every target: near-ties compare as sets
        ext_ids, ext_scores = oracle.find_neighbors(flat, t, limit + 40)
        assert_topk_parity(r[t, :c[t]], s[t, :c[t]], ext_ids, ext_scores, limit)
        score_of = dict(zip(ext_ids.tolist(), ext_scores.tolist()))
        assert max(abs(score_of[int(row)] - float(sc)) for row, sc in zip(r[t, :c[t]], s[t, :c[t]])) <= SCORE_TOL
    ids = [f"chunk{i}" for i in range(n)]
    named = HipIndex.build_from_flat(ids, flat)
    graph = named.knn_graph(limit)
    named.close()
    assert len(graph) == n and [x.id for x in graph[5]] == [ids[int(row)] for row in r[5, :c[5]]]
    assert [np.float32(x.score) for x in graph[699]] == s[699, :c[699]].tolist()


# ---- after update, remove and extend ------------------------------------------------------------------------------------
@gpu
def test_graph_follows_the_rows_now_stored(hip):
    dim, base, limit = 64, 5000, 15
    flat = synth.gaussian_unit(600, dim=dim, seed=59)
    idx = HipIndex.build_from_flat(None, flat, row_base=base)
    before = idx.knn_graph_rows(limit)

    def check(now, what):
        got = assert_composition(idx, now, base, limit, what)
        fresh = HipIndex.build_from_flat(None, now, row_base=base)
        assert_graph_equal(got, fresh.knn_graph_rows(limit), (what, "fresh build"))
        fresh.close()
        return got

    upd = np.array([0, 255, 256, 300, 599])
    new = synth.gaussian_unit(len(upd), dim=dim, seed=61)
    assert idx.update_rows(base + upd, new) == len(upd)
    flat = flat.copy()
    flat[upd] = new
    after = check(flat, "update")
    assert not np.array_equal(after[0][upd], before[0][upd])                  # the new rows have other neighbours
    gone = np.concatenate([np.arange(10, 60), [511, 598]])
    assert idx.remove_rows(base + gone) == len(gone)
    flat = np.delete(flat, gone, axis=0)
    assert check(flat, "remove")[0].shape == (548, limit)
    more = synth.gaussian_unit(230, dim=dim, seed=67)
    idx.extend(None, more)
    flat = np.concatenate([flat, more])
    assert check(flat, "extend")[0].shape == (778, limit)                     # a fourth, ragged tile of 10 rows
    idx.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_outputs_and_handle_alone(hip):
    n, base = 300, 5000
    flat = synth.gaussian_unit(n, dim=64, seed=71)
    idx = HipIndex.build_from_flat(None, flat, row_base=base)
    want = idx.search_batch(flat[:3], 5)

    def refused(first, m, why, null=None):
        L = 15
        bufs = [np.full((max(m, 1) if m <= 70000 else 1, L), 7, np.uint64), np.full((max(m, 1) if m <= 70000 else 1, L), 7, np.float32),
                np.full((max(m, 1) if m <= 70000 else 1,), 7, np.uint32)]
        ptrs = [None if null == i else b.ctypes.data for i, b in enumerate(bufs)]
        assert idx._lib.cqs_hip_index_knn_graph(idx._h, first, m, L, *ptrs) == _lib.ERR_INVALID, why
        assert idx.last_error() == "knn_graph: " + why
        assert all((b == 7).all() for b in bufs), why
        assert not idx.is_poisoned()
        got = idx.search_batch(flat[:3], 5)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), why

    for null in (0, 1, 2):
        refused(base, 10, "null output buffer", null=null)
    refused(base, _lib.KNN_MAX_TARGETS + 1, "more than CQS_HIP_KNN_MAX_TARGETS targets in one call")   # (checked before the range: m > len too)
    refused(base - 1, 2, "range not in this index")
    refused(0, 2, "range not in this index")
    refused(base + n, 1, "range not in this index")
    refused(base + n - 5, 6, "range not in this index")
    refused(2 ** 64 - 1, 2, "range not in this index")
    refused(base + 5, 10, "null output buffer", null=1)
    # m == 0: OK, nothing touched, whatever the pointers and the range
    assert idx._lib.cqs_hip_index_knn_graph(idx._h, base + 9999, 0, 15, None, None, None) == _lib.OK
    rc, r, s, c = graph_call(idx, base + 3, 0, 15)
    assert rc == _lib.OK
    with pytest.raises(ValueError):
        idx.knn_graph_rows(15, first=200, count=101)
    # the handle still answers graph calls
    rc, r, s, c = graph_call(idx, base + 299, 1, 15, fill=7)
    assert rc == _lib.OK and c[0] == 15 and base + 299 not in r[0]
    idx.close()


@gpu
def test_sharded_handle_is_refused_and_a_poisoned_one_says_so(hip):
    flat = synth.gaussian_unit(300, dim=64, seed=73)
    sh = HipIndex.build_sharded(None, flat, [0])
    rc, r, s, c = graph_call(sh, 0, 10, 15, fill=7)
    assert rc == _lib.ERR_INVALID and sh.last_error() == "knn_graph: not built for a row-sharded handle"
    assert (r == 7).all() and (s == 7).all() and (c == 7).all() and not sh.is_poisoned()
    rc, *_ = graph_call(sh, 295, 10, 15, fill=7)
    assert rc == _lib.ERR_INVALID and sh.last_error() == "knn_graph: range not in this index"     # the range comes first
    with pytest.raises(HipError):
        sh.knn_graph_rows(15)
    assert sh.search_batch(flat[:2], 5)[2].tolist() == [5, 5]
    sh.close()
    idx = HipIndex.build_from_flat(None, flat)
    hip.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_index_fail_next.restype = None
    hip.cqs_hip_debug_index_fail_next(idx._h)
    with pytest.raises(HipError):
        idx.search_batch(flat[:9], 5)
    assert idx.is_poisoned()
    rc, r, s, c = graph_call(idx, 0, 10, 15, fill=7)
    assert rc == _lib.ERR_POISONED and (r == 7).all() and (c == 7).all()
    idx.close()


@gpu
def test_one_row_index_and_a_first_call_on_a_fresh_handle(hip):
    one = HipIndex.build_from_flat(None, synth.gaussian_unit(1, dim=64, seed=79), row_base=5000)
    rc, r, s, c = graph_call(one, 5000, 1, 15, fill=7)
    assert rc == _lib.OK and c.tolist() == [0] and (r == 0).all() and (s == 0).all()      # count 0, slots written as 0
    one.close()
    two = HipIndex.build_from_flat(None, synth.gaussian_unit(2, dim=64, seed=83))
    rc, r, s, c = graph_call(two, 1, 1, 100, fill=7)                                       # before any search on the handle
    assert rc == _lib.OK and c.tolist() == [1] and r[0, 0] == 0 and (r[0, 1:] == 0).all() and (s[0, 1:] == 0).all()
    two.close()
