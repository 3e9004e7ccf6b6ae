"""Cosine MMR re-rank of a candidate pool on the device (`cqs_hip_index_pairwise` / `cqs_hip_index_mmr`):
the Gram matrix against float64, the greedy loop against the numpy restatement of the reference's `mmr_rerank`
(tests/mmr_cases.py; src/search/mmr.rs:59-126), the edges of mmr.rs:60-69, row-sharded handles and concurrency."""
import ctypes as C
import threading

import numpy as np
import pytest

import mmr_cases as mc
from parity import SCORE_TOL

pytestmark = pytest.mark.gpu

N_ROWS = 2048
_cache = {}


def _index(kind, dim, row_base=0):
    """(rows, HipIndex) over 2 048 rows, built once per (kind, dim, row_base)."""
    from cqs_amd import DistanceMetric, HipIndex
    key = (kind, dim, row_base)
    if key not in _cache:
        if kind == "unit":
            rows, metric = mc.unit_rows(N_ROWS, dim, 100 + dim), DistanceMetric.Cosine
        elif kind == "clustered":
            rows, metric = mc.clustered_unit_rows(N_ROWS, dim, 200 + dim), DistanceMetric.Cosine
        else:
            rows, metric = mc.exact_rows(N_ROWS, dim, 300 + dim), DistanceMetric.DotProduct
        _cache[key] = (rows, HipIndex.build_from_flat(None, rows, metric, row_base=row_base))
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. pairwise vs float64 ---------------------------------------------------------------------------------------------
PAIRWISE = [(dim, m, 0) for dim in (4, 36, 768) for m in (1, 2, 31, 32, 33, 65)] + [(36, 1024, 0), (36, 65, 1_000_003)]


@pytest.mark.parametrize("dim,m,row_base", PAIRWISE)
def test_pairwise_matches_float64(hip, dim, m, row_base):
    rows, idx = _index("unit", dim, row_base)
    rng = np.random.default_rng(dim * 10_000 + m)
    cand = rng.permutation(N_ROWS)[:m].astype(np.uint64)
    if m >= 2:
        cand[m - 1] = cand[0]                                  # one row listed twice
    g = idx.pairwise_rows(cand + np.uint64(row_base))
    assert g.shape == (m, m) and g.dtype == np.float32
    g64 = mc.gram64(rows[cand.astype(np.int64)])
    err = float(np.max(np.abs(g.astype(np.float64) - g64)))
    print("pairwise dim=%d m=%d row_base=%d max|G - G64| = %.3g (bar %.1g)" % (dim, m, row_base, err, SCORE_TOL))
    assert err <= SCORE_TOL
    assert np.array_equal(_bits(g), _bits(g.T)), "G is not bitwise symmetric"
    if m >= 2:
        b = _bits(g)
        assert b[0, m - 1] == b[0, 0] == b[m - 1, m - 1] == b[m - 1, 0], "a row listed twice is not fully similar to itself"
        assert np.array_equal(b[0], b[m - 1]), "the two entries of one row see different similarities"


# ---- 2. exact-arithmetic pools: bit-identical picks, ties included -------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5, 0.75])
@pytest.mark.parametrize("m,limit", [(33, 1), (33, 32), (300, 1), (300, 299)])
def test_exact_pools_give_the_restatements_picks(hip, m, limit, lam):
    rows, idx = _index("exact", 64)
    cand, scores = mc.exact_pool(N_ROWS, m, 7 * m + limit)
    assert len(np.unique(cand)) < m and len(np.unique(scores)) < m            # duplicate rows and duplicate scores
    g64 = mc.gram64(rows[cand.astype(np.int64)])
    # the generator is checked, not trusted: every dot a multiple of 2^-6 of magnitude <= 1, exact in f32
    assert np.array_equal(g64 * 64.0, np.round(g64 * 64.0)) and float(np.max(np.abs(g64))) <= 1.0
    assert np.array_equal(g64.astype(np.float32).astype(np.float64), g64)
    assert np.array_equal(scores.astype(np.float64) * 256.0, np.round(scores.astype(np.float64) * 256.0))
    assert float(scores.min()) >= 0.0 and float(scores.max()) <= 1.0
    want = mc.mmr_rerank(scores, g64, limit, lam)
    got = idx.mmr_rows(cand, scores, limit, lam)
    assert got.dtype == np.uint32 and list(got) == want
    # the device's own Gram matrix is the exact one
    assert np.array_equal(idx.pairwise_rows(cand).astype(np.float64), g64)


# ---- 3. random pools are valid greedy runs --------------------------------------------------------------------------------
def _searched_pool(m):
    key = ("pool", m)
    if key not in _cache:
        rows, idx = _index("clustered", 768)
        q = rows[11].astype(np.float64) + 0.6 * mc.unit_rows(1, 768, 5)[0]
        q = (q / np.linalg.norm(q)).astype(np.float32)
        r, s, c = idx.search_batch(q, m)
        assert int(c[0]) == m
        cand, scores = r[0].copy(), s[0].copy()
        _cache[key] = (cand, scores, mc.gram64(rows[cand.astype(np.int64)]))
    return _cache[key]


def _assert_valid_greedy_run(picks, scores, g64, limit, lam):
    """Replay the device's picks against the float64 Gram matrix: at every step the pick's MMR value is within
    2 x SCORE_TOL of that step's float64 maximum, given the device's own earlier picks.  The bound: one Gram entry's
    tolerance (SCORE_TOL) on each of the two compared values, scaled by (1 - lambda) <= 1; f32 rounding of the two-operation
    formula (~1e-7) is two orders below it."""
    m = len(scores)
    bound = 2.0 * SCORE_TOL
    lam64 = float(np.float32(min(max(lam, 0.0), 1.0)))
    s64 = scores.astype(np.float64)
    max_sim = np.zeros(m)
    taken = np.zeros(m, dtype=bool)
    worst = 0.0
    for t, p in enumerate(picks):
        mmr = lam64 * s64 - (1.0 - lam64) * max_sim
        best = float(np.max(mmr[~taken]))
        worst = max(worst, best - float(mmr[p]))
        assert not taken[p]
        assert float(mmr[p]) >= best - bound, "step %d: pick %d has mmr %.9g, the step's maximum is %.9g" % (t, p, mmr[p], best)
        taken[p] = True
        max_sim = np.maximum(max_sim, g64[:, p])
    print("greedy replay m=%d limit=%d lambda=%g: worst shortfall %.3g (bound %.1g)" % (m, limit, lam, worst, bound))


@pytest.mark.parametrize("lam", [0.3, 0.7, 0.95])
@pytest.mark.parametrize("m,limit", [(97, 20), (97, 100), (500, 20), (500, 100)])
def test_random_pools_are_valid_greedy_runs(hip, m, limit, lam):
    _, idx = _index("clustered", 768)
    cand, scores, g64 = _searched_pool(m)
    picks = [int(x) for x in idx.mmr_rows(cand, scores, limit, lam)]
    assert len(picks) == min(limit, m) and len(set(picks)) == len(picks) and all(0 <= p < m for p in picks)
    if limit >= m:
        assert picks == list(range(m))                         # mmr.rs:67-69: no diversification, input order
        return
    _assert_valid_greedy_run(picks, scores, g64, limit, lam)
    if float(scores[0]) - float(scores[1]) > 2.0 * SCORE_TOL:
        assert picks[0] == 0
    assert picks != list(range(limit)), "the diversity term never changed a pick: the pool does not exercise it"


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------
def _raw_mmr(idx, cand, scores, limit, lam):
    cand = np.ascontiguousarray(cand, dtype=np.uint64)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    picks = np.full((max(1, len(cand)),), 0xFFFFFFFF, dtype=np.uint32)
    c = C.c_uint32(12345)
    rc = idx._lib.cqs_hip_index_mmr(idx._h, cand.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), len(cand), limit,
                                    lam, picks.ctypes.data_as(C.c_void_p), C.byref(c))
    return rc, picks, c.value


def test_edges(hip):
    from cqs_amd import _lib
    rows, idx = _index("exact", 64)
    cand, scores = mc.exact_pool(N_ROWS, 33, 1)
    g64 = mc.gram64(rows[cand.astype(np.int64)])
    assert list(idx.mmr_rows(cand, scores, 0, 0.5)) == []                        # limit = 0
    assert list(idx.mmr_rows(cand[:0], scores[:0], 5, 0.5)) == []                # m = 0
    assert list(idx.mmr_rows(cand, scores, 33, 0.5)) == list(range(33))          # limit >= m
    assert list(idx.mmr_rows(cand, scores, 1000, 0.5)) == list(range(33))
    assert list(idx.mmr_rows(cand, scores, 5, 1.0)) == list(range(5))            # lambda >= 1
    assert list(idx.mmr_rows(cand, scores, 5, 7.0)) == list(range(5))
    assert list(idx.mmr_rows(cand, scores, 5, -3.0)) == list(idx.mmr_rows(cand, scores, 5, 0.0)) == mc.mmr_rerank(scores, g64, 5, 0.0)
    assert idx.pairwise_rows(cand[:0]).shape == (0, 0)
    bad_scores = scores.copy()
    bad_scores[3] = np.inf
    bad_rows = cand.copy()
    bad_rows[32] = N_ROWS
    big = np.arange(1025, dtype=np.uint64)
    for what, args in (("NaN lambda", (cand, scores, 5, float("nan"))),
                       ("infinite score", (cand, bad_scores, 5, 0.5)),
                       ("row outside the index", (bad_rows, scores, 5, 0.5)),
                       ("m = 1025", (big, np.linspace(1, 0, 1025, dtype=np.float32), 5, 0.5))):
        rc, picks, count = _raw_mmr(idx, *args)
        assert rc == _lib.ERR_INVALID, what
        assert count == 0 and int(picks[0]) == 0xFFFFFFFF, what
        assert not idx.is_poisoned(), what
        assert list(idx.mmr_rows(cand, scores, 5, 0.5)) == mc.mmr_rerank(scores, g64, 5, 0.5), what   # still usable
    with pytest.raises(Exception):
        idx.pairwise_rows(bad_rows)
    with pytest.raises(Exception):
        idx.pairwise_rows(big)
    assert not idx.is_poisoned()
    assert np.array_equal(idx.pairwise_rows(cand).astype(np.float64), g64)


def test_result_level_calls_on_an_id_map_index(hip):
    from cqs_amd import DistanceMetric, HipIndex, IndexResult
    rows = mc.clustered_unit_rows(N_ROWS, 36, 9)
    ids = ["chunk-%04d" % i for i in range(N_ROWS)]
    idx = HipIndex.build_from_flat(ids, rows, DistanceMetric.Cosine, row_base=4096)
    q = rows[5]
    pool = idx.search(q, 120)
    assert len(pool) == 120
    picked = idx.mmr_rerank(pool, 15, 0.6)
    assert len(picked) == 15 and len({r.id for r in picked}) == 15 and all(r in pool for r in picked)
    assert picked == idx.search_mmr(q, 120, 15, 0.6)
    # the picks are the restatement's over the device's own Gram matrix (ids -> rows through id_map, row_base added)
    cand = np.array([4096 + ids.index(r.id) for r in pool], dtype=np.uint64)
    want = mc.mmr_rerank([r.score for r in pool], idx.pairwise_rows(cand), 15, 0.6)
    assert [pool[i] for i in want] == picked
    assert idx.mmr_rerank(pool, 500, 0.6) == pool and idx.mmr_rerank(pool, 15, 1.0) == pool[:15]
    assert idx.mmr_rerank([], 5, 0.5) == []
    with pytest.raises(KeyError):
        idx.mmr_rerank(pool[:3] + [IndexResult("no-such-chunk", 0.1)], 2, 0.5)
    idx.close()


# ---- 5. row-sharded handle --------------------------------------------------------------------------------------------------
def test_sharded_handle_gives_the_single_device_bytes(hip):
    from cqs_amd import DistanceMetric, HipIndex
    rows, idx = _index("clustered", 768)
    cand, scores, _ = _searched_pool(97)
    sh = HipIndex.build_sharded(None, rows, [0, 0, 0], DistanceMetric.Cosine)
    assert len(sh.shards()) == 3 and len({int(c) * 3 // N_ROWS for c in cand}) > 1      # the pool spans shards
    assert np.array_equal(_bits(sh.pairwise_rows(cand)), _bits(idx.pairwise_rows(cand)))
    for limit, lam in ((20, 0.3), (20, 0.7), (96, 0.95)):
        assert list(sh.mmr_rows(cand, scores, limit, lam)) == list(idx.mmr_rows(cand, scores, limit, lam))
    # edges go through the same host checks
    from cqs_amd import _lib
    assert _raw_mmr(sh, cand, scores, 5, float("nan"))[0] == _lib.ERR_INVALID and not sh.is_poisoned()
    assert list(sh.mmr_rows(cand, scores, 5, 1.0)) == list(range(5))
    sh.close()
    xrows, xidx = _index("exact", 64)
    xcand, xscores = mc.exact_pool(N_ROWS, 300, 7 * 300 + 299)
    xsh = HipIndex.build_sharded(None, xrows, [0, 0, 0], DistanceMetric.DotProduct)
    want = mc.mmr_rerank(xscores, mc.gram64(xrows[xcand.astype(np.int64)]), 299, 0.5)
    assert list(xsh.mmr_rows(xcand, xscores, 299, 0.5)) == want == list(xidx.mmr_rows(xcand, xscores, 299, 0.5))
    assert np.array_equal(_bits(xsh.pairwise_rows(xcand)), _bits(xidx.pairwise_rows(xcand)))
    xsh.close()


# ---- 6. beside a search -----------------------------------------------------------------------------------------------------
def test_mmr_beside_searches_on_one_handle(hip):
    rows, idx = _index("clustered", 768)
    cand, scores, _ = _searched_pool(500)
    queries = mc.unit_rows(50, 768, 77)
    lone_search = [idx.search_batch(q, 64) for q in queries]
    lone_picks = list(idx.mmr_rows(cand, scores, 40, 0.7))
    errors = []

    def searcher():
        try:
            for q, (r0, s0, c0) in zip(queries, lone_search):
                r, s, c = idx.search_batch(q, 64)
                assert np.array_equal(r, r0) and np.array_equal(_bits(s), _bits(s0)) and np.array_equal(c, c0)
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errors.append(e)

    def reranker():
        try:
            for _ in range(20):
                assert list(idx.mmr_rows(cand, scores, 40, 0.7)) == lone_picks
        except BaseException as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=searcher), threading.Thread(target=reranker)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not idx.is_poisoned()
