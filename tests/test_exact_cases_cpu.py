"""Keeps tests/exact_cases.py honest without a GPU: for every (n, dim) family of tests/test_scan_exact_gpu.py the premise
(f32 arithmetic on this data is exact in any order) and `expected` against the CPU oracle; then a numpy "kernel" with
planted faults, every one of which `assert_exact` must reject."""
import numpy as np
import pytest

import exact_cases as X

FAMILIES = X.families(256)
MAX_QUERIES = 3        # queries per family held to the oracle and to the accumulation orders


def f32_orders(rows, q, rng):
    """The dot of every row with q, accumulated in f32 three ways: forward, a random column order, 64 lane partials
    (columns j % 64) folded by a pairwise tree."""
    n, dim = rows.shape
    prod = rows * q[None, :]
    fwd = np.zeros(n, np.float32)
    for j in range(dim):
        fwd = fwd + prod[:, j]
    rnd = np.zeros(n, np.float32)
    for j in rng.permutation(dim):
        rnd = rnd + prod[:, j]
    pad = np.zeros((n, (dim + 63) // 64 * 64), np.float32)
    pad[:, :dim] = prod
    lanes = np.zeros((n, 64), np.float32)
    for c in range(pad.shape[1] // 64):
        lanes = lanes + pad[:, 64 * c:64 * c + 64]
    while lanes.shape[1] > 1:
        lanes = lanes[:, 0::2] + lanes[:, 1::2]
    return fwd, rnd, lanes[:, 0]


@pytest.mark.parametrize("name,make", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_family_is_exact_and_matches_the_oracle(oracle, name, make):
    c = make()
    scale = 2.0 ** -c.e
    assert c.rows.dtype == np.float32 and c.queries.dtype == np.float32
    assert np.array_equal(c.rows.astype(np.float64), c.C * scale) and np.array_equal(c.queries.astype(np.float64), c.Q * scale)
    D = c.dim - len(c.windows)
    assert (c.C[:, :D] != 0).all() and (c.Q[:, :D] != 0).all()
    assert not (c.S == 0).any(), "a zero total in a case of the GPU matrix"
    rng = np.random.default_rng(7)
    some = np.unique(np.concatenate([rng.integers(0, c.n, 64), [lo for lo, _ in c.windows], [hi - 1 for _, hi in c.windows]]))
    assert np.array_equal(c.S[:, some], c.Q @ c.C[some].T), "S is not the integer matrix product"
    if not c.dot:
        assert np.abs(c.S).max() * scale * scale <= 1.0
    sub = np.arange(c.n) if c.n <= 8192 else np.concatenate([np.arange(4096), np.arange(c.n - 4096, c.n)])
    for qi in range(min(c.Q.shape[0], MAX_QUERIES)):
        want = np.ldexp(c.S[qi, sub].astype(np.float64), -2 * c.e).astype(np.float32)
        for got in f32_orders(c.rows[sub], c.queries[qi], rng):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, qi)
        lo, hi = c.windows[c.target[qi]]
        width = hi - lo
        # the boosted query's top-`width` is its window
        ids, sc = X.expected(c.S[qi], c.e, width)
        assert sorted(ids.tolist()) == list(range(lo, hi)), (name, qi)
        k = min(1024, c.n)
        oid, osc = oracle.index_search(c.rows, c.queries[qi], k)
        X.assert_exact(oid, osc, len(oid), *X.expected(c.S[qi], c.e, k), what="%s q%d plain" % (name, qi))
        scattered = np.random.default_rng(qi).integers(0, 2 ** 32, (c.n + 31) // 32, dtype=np.uint64).astype(np.uint32)
        keep = X.range_bits(c.n, lo + 13, hi + 13) | (scattered & np.uint32(0x80000001))
        oid, osc = oracle.index_search(c.rows, c.queries[qi], k, keep)
        X.assert_exact(oid, osc, len(oid), *X.expected(c.S[qi], c.e, k, keep=keep), what="%s q%d bitset" % (name, qi))
        if not c.dot:
            thr = float(c.score_f32(qi, lo + (hi - lo) // 2))     # a score that occurs: `>=` keeps it, `>` would not
            assert thr > 0.0
            oid, osc = oracle.index_search(c.rows, c.queries[qi], k, None, 1, thr)
            eid, esc = X.expected(c.S[qi], c.e, k, mode=1, thr=thr)
            assert np.float32(thr) in esc
            X.assert_exact(oid, osc, len(oid), eid, esc, what="%s q%d pipeline" % (name, qi))


def test_tier_sizes_reach_each_plan():
    for n_cu in (64, 256, 304):
        plans = {name: X.plan_tiers((X.tier_rows(name, n_cu) + 255) // 256 * 256, n_cu) for name in X.TIERS}
        assert plans["rows16"][0] == 0 and plans["rows16"][2] > 0
        assert plans["rows64"][0] > 0 and plans["rows64"][1] == 0 and plans["rows64"][2] == 0
        assert plans["rows64+32"][1] > 0 and sum(plans["rows64+32"]) <= 96 * n_cu
        assert plans["persistent"][1] > 0 and sum(plans["persistent"]) > 96 * n_cu
        # one step of 256 rows back is the plan before
        assert X.plan_tiers((X.tier_rows("rows64", n_cu) + 255) // 256 * 256 - 256, n_cu)[2] > 0
        assert X.plan_tiers((X.tier_rows("rows64+32", n_cu) + 255) // 256 * 256 - 256, n_cu)[1] == 0
        assert sum(X.plan_tiers((X.tier_rows("persistent", n_cu) + 255) // 256 * 256 - 256, n_cu)) <= 96 * n_cu


def test_window_bits_and_zero_total_guard():
    assert X.bits_of(X.window_bits(100, 1, 32), 100).nonzero()[0].tolist() == list(range(32, 64))
    assert X.bits_of(X.window_bits(100, 2, 32, offset=13), 100).nonzero()[0].tolist() == list(range(77, 100))
    assert X.window_bits(4097, 0, 256).shape[0] == 129
    with pytest.raises(AssertionError, match="zero total"):
        X.expected(np.array([3, 0, -1]), 2, 2)
    ids, sc = X.expected(np.array([3, 0, -1]), 2, 1)
    assert ids.tolist() == [0] and sc.tolist() == [3 / 16]
    # order: score descending, row ascending; a bitset cuts k to the kept rows; none kept = nothing
    ids, _ = X.expected(np.array([5, 7, 5, 7, 1]), 1, 4)
    assert ids.tolist() == [1, 3, 0, 2]
    ids, _ = X.expected(np.array([5, 7, 5, 7, 1]), 1, 4, keep=np.array([0b10101], np.uint32))
    assert ids.tolist() == [0, 2, 4]
    assert X.expected(np.array([5, 7]), 1, 4, keep=np.array([0b100], np.uint32))[0].shape[0] == 0
    # PIPELINE: clamp to [0, 1], `>= thr`
    ids, sc = X.expected(np.array([8, 3, -3, 2]), 1, 4, mode=1, thr=0.75)
    assert ids.tolist() == [0, 1] and sc.tolist() == [1.0, 0.75]


# ---- sensitivity: a numpy "kernel" with planted faults ---------------------------------------------------------------
N, DIM, WIDTH = 4097, 260, 256        # 260 columns: a last partial chunk of four; 17 windows, the last one row 4096 alone


@pytest.fixture(scope="module")
def case():
    return X.dyadic(N, DIM, 6000, nq=17, width=WIDTH)


def tie_position(c, qi):
    """A k at which positions k - 1 and k of query qi's ranking tie (inside its window)."""
    ids, sc = X.expected(c.S[qi], c.e, WIDTH)
    k = int(np.flatnonzero(sc[:-1] == sc[1:])[0]) + 1
    return k


def np_search(c, qis, k, keeps=None, fault=None, fault_arg=None):
    """Scores of every row in float64 from the f32 arrays, masked, sorted by (score descending, row ascending): what a
    correct kernel returns, unless `fault` is planted.  keeps: one bitset per query."""
    rows, qs = c.rows.astype(np.float64), c.queries[qis].astype(np.float64)
    if fault == "column dropped":
        rows = rows.copy(); rows[:, 5] = 0
    if fault == "column of the last partial chunk dropped":
        rows = rows.copy(); rows[:, 257] = 0
    if fault == "query columns swapped":
        qs = qs.copy(); qs[:, [6, 7]] = qs[:, [7, 6]]
    S = (qs @ rows.T).astype(np.float32)
    if fault == "last row not scored":
        S[:, -1] = -np.inf
    if fault == "last tile a copy of the one before":
        t = (c.n - 1) // 64 * 64
        S[:, t:] = S[:, t - 64:t - 64 + (c.n - t)]
    out = []
    for j, qi in enumerate(qis):
        s = S[j].copy()
        kk = k
        if keeps is not None:
            kw = keeps[j].copy()
            word = fault_arg
            if fault == "neighbour slot's bitset word" and j + 1 < len(qis):
                kw[word] = keeps[j + 1][word]
            if fault == "bit 31 ignored":
                kw[word] &= np.uint32(0x7FFFFFFF)
            kept = X.bits_of(kw, c.n)
            kk = min(k, int(X.bits_of(keeps[j], c.n).sum()))
            s[~kept] = -np.inf
        order = np.argsort(-s.astype(np.float64), kind="stable")
        order = order[np.isfinite(s[order])][:kk + 1]
        if fault == "tie broken by the larger row" and j == 0:
            assert s[order[kk - 1]] == s[order[kk]]
            order = np.concatenate([order[:kk - 1], order[kk:kk + 1]])
        order = order[:kk]
        sc = s[order].copy()
        if fault == "one ulp" and j == 0:
            sc[kk // 2] = np.nextafter(sc[kk // 2], np.float32(2))
        out.append((order.astype(np.uint64), sc, len(order)))
    return out


def check(c, qis, k, got, keeps=None):
    for j, qi in enumerate(qis):
        r, s, cnt = got[j]
        X.assert_exact(r, s, cnt, *X.expected(c.S[qi], c.e, k, keep=None if keeps is None else keeps[j]), what="q%d" % qi)


def window_keeps(c, qis):
    return [X.window_bits(c.n, int(c.target[qi]), WIDTH, offset=13) for qi in qis]


def test_numpy_kernel_without_a_fault_passes(case):
    qis = list(range(17))
    check(case, qis, WIDTH, np_search(case, qis, WIDTH))
    check(case, qis, 300, np_search(case, qis, 300, keeps=window_keeps(case, qis)), keeps=window_keeps(case, qis))
    k = tie_position(case, 0)
    check(case, [0], k, np_search(case, [0], k))


@pytest.mark.parametrize("fault", ["column dropped", "column of the last partial chunk dropped", "query columns swapped",
                                   "last row not scored", "last tile a copy of the one before", "one ulp",
                                   "tie broken by the larger row"])
def test_unfiltered_faults_are_rejected(case, fault):
    qis = list(range(17))         # 17 windows of 256 rows: every row of the corpus is in some query's answer
    k = tie_position(case, 0) if fault == "tie broken by the larger row" else WIDTH
    with pytest.raises(AssertionError):
        check(case, qis, k, np_search(case, qis, k, fault=fault))


@pytest.mark.parametrize("fault,word", [("neighbour slot's bitset word", (256 + 13) // 32), ("bit 31 ignored", (13 + 31) // 32)])
def test_bitset_faults_are_rejected(case, fault, word):
    """Windows offset by 13 rows begin and end inside a word: word 8 holds the end of slot 0's window and the beginning of
    slot 1's, and bit 31 of word 1 is a kept row of slot 0."""
    qis = list(range(17))
    keeps = window_keeps(case, qis)
    assert keeps[0][word] != keeps[1][word] or fault == "bit 31 ignored"
    assert keeps[0][word] >> 31 or fault != "bit 31 ignored"
    with pytest.raises(AssertionError):
        check(case, qis, 300, np_search(case, qis, 300, keeps=keeps, fault=fault, fault_arg=word), keeps=keeps)
