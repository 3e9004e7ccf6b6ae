"""Exact-arithmetic scan data: corpora and queries on which every correct kernel returns the same bits (DESIGN.md,
"Exact-data sweeps of the scan").  No GPU and no library here: tests/test_scan_exact_gpu.py takes its inputs and every
expected value from this file, tests/test_exact_cases_cpu.py holds this file to the oracle and to planted faults.

Entries are small integers times 2^-e.  A product is at most 16 units of 2^-2e and a dot product at most 16 dim + boost
units, far below 2^24, so every product and every partial sum, in any order and in any tree, is an exact f32: the
matrix cores' k-ordered chain, the gemv's lane partials and butterfly, the K-split's four-way combine.  The score of a
row is an integer matrix product, scaled; the top-k is the sort by (score descending, row ascending), ties included.

Boost columns.  The last W columns are reserved, one per window of rows (`windows`, by default consecutive ranges of
`width` rows, the last one ragged).  The rows of window w hold 2^-1 in reserved column w (0 in the others) and query i
= a base query + 2^-1 in the column of its target window i % W.  The boost, 2^-2, exceeds twice the largest base
|score| (asserted), so the unfiltered top-`width` of a query is exactly its window, in exact score order: W queries in
one call read the score of every row through the public search, each query slot aiming at another row range.

Zero totals.  A total of 0 could legitimately be +0 or -0, and the two have different ordered keys.  Totals here are
odd by construction: column 0 is odd on both sides, every other base column is even on one side (the query's in odd
columns, the corpus' in even ones), the boost is even.  `dyadic` still checks every total, moves on to the next seed
if one is zero and records the seed it used; `expected` refuses to return a zero total.
"""
import functools
import math

import numpy as np

MAX_K = 1024


def default_windows(n, width):
    return [(lo, min(lo + width, n)) for lo in range(0, n, width)]


class Case:
    """n, dim, e (entries are integers x 2^-e, scores integers x 2^-2e), C int64 [n, dim], Q int64 [nq, dim], S int64
    [nq, n] = Q C^T, rows / queries the f32 arrays, windows [(lo, hi)], target [nq] (window of each query), boost (the
    integer in the reserved columns), seed (the one used), dot (metric of the handle to build)."""

    def score_f32(self, qi, row):
        return np.float32(math.ldexp(int(self.S[qi, row]), -2 * self.e))


def _signed(rng, shape, values):
    return rng.choice(np.asarray(values, dtype=np.int64), size=shape) * rng.choice(np.asarray([-1, 1], dtype=np.int64), size=shape)


def dyadic(n, dim, seed, nq=None, width=MAX_K, windows=None, dot=False):
    """The exact case of n rows x dim columns: see the module docstring.  `windows` overrides the consecutive ranges of
    `width` rows (any ranges, e.g. a few places of a large corpus); nq defaults to one query per window.  dot: e = 0, raw
    integer scores in the thousands (a dot-metric handle's log-spaced bins); else every |score|, boost included, <= 1."""
    windows = default_windows(n, width) if windows is None else [(int(lo), int(hi)) for lo, hi in windows]
    W = len(windows)
    D = dim - W
    assert D >= 1 and all(0 <= lo < hi <= n for lo, hi in windows), (n, dim, windows)
    nq = W if nq is None else nq
    for s in range(seed, seed + 16):
        rng = np.random.default_rng(s)
        C = np.zeros((n, dim), dtype=np.int64)
        Q = np.zeros((nq, dim), dtype=np.int64)
        C[:, :D] = _signed(rng, (n, D), [1, 2, 3, 4])
        Q[:, :D] = _signed(rng, (nq, D), [1, 2, 3, 4])
        C[:, 0] = _signed(rng, (n,), [1, 3])
        Q[:, 0] = _signed(rng, (nq,), [1, 3])
        Q[:, 1:D:2] = _signed(rng, Q[:, 1:D:2].shape, [2, 4])
        C[:, 2:D:2] = _signed(rng, C[:, 2:D:2].shape, [2, 4])
        base = np.rint(C[:, :D].astype(np.float64) @ Q[:, :D].T.astype(np.float64)).astype(np.int64)
        top = int(np.abs(base).max())
        if dot:
            e, boost = 0, 2
            while boost * boost <= 2 * top:
                boost *= 2
        else:
            e = max(2, math.ceil(math.log2(16 * dim) / 2))
            while (1 << (2 * e - 2)) <= 2 * top:
                e += 1
            boost = 1 << (e - 1)
        assert boost * boost > 2 * top, "the boost must exceed twice the largest base |score|"
        assert 16 * D + boost * boost < 2 ** 24, "a partial sum could leave the exact f32 integers"
        target = np.arange(nq) % W
        for w, (lo, hi) in enumerate(windows):
            C[lo:hi, D + w] = boost
        Q[np.arange(nq), D + target] = boost
        S = base.T.copy()
        for i in range(nq):
            lo, hi = windows[target[i]]
            S[i, lo:hi] += boost * boost
        if (S == 0).any():
            continue
        c = Case()
        c.n, c.dim, c.e, c.C, c.Q, c.S, c.windows, c.target, c.boost, c.seed, c.dot = n, dim, e, C, Q, S, windows, target, boost, s, dot
        c.rows = np.ldexp(C.astype(np.float32), -e)
        c.queries = np.ldexp(Q.astype(np.float32), -e)
        assert dot or int(np.abs(S).max()) <= 1 << (2 * e), "a cosine case's |score| must stay <= 1"
        return c
    raise AssertionError("no seed in %d .. %d without a zero total" % (seed, seed + 15))


def bits_of(keep, n):
    return np.unpackbits(np.ascontiguousarray(keep, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


def range_bits(n, lo, hi):
    """Keep-bitset (u32 words, bit r % 32 of word r // 32) of the rows [lo, hi) of n."""
    keep = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
    keep[max(lo, 0):min(hi, n)] = 1
    return np.packbits(keep, bitorder="little").view(np.uint32).copy()


def window_bits(n, w, width, offset=0):
    """Keep-bitset of window w: rows [offset + w width, offset + (w + 1) width) of n."""
    return range_bits(n, offset + w * width, offset + (w + 1) * width)


def expected(S_int, e, k, keep=None, mode=0, thr=0.0, dead=()):
    """(ids u64, scores f32) the search must return for one query: S_int int64 [n] its integer totals (scores are
    S_int x 2^-2e), from integer arithmetic alone.  keep: the bitset (k is cut to the kept rows, none kept = nothing);
    mode 1 = PIPELINE: clamp to [0, 1], then keep `score >= thr`; dead: rows whose score is not finite (never returned).
    Order: score descending, row ascending."""
    S_int = np.asarray(S_int, dtype=np.int64)
    n = S_int.shape[0]
    none = np.zeros(0, np.uint64), np.zeros(0, np.float32)
    if n == 0 or k == 0:
        return none
    alive = np.ones(n, dtype=bool)
    if keep is not None:
        alive = bits_of(keep, n)
        kept = int(alive.sum())
        if kept == 0:
            return none
        k = min(k, kept)
    for r in dead:
        alive[r] = False
    exact = np.ldexp(S_int.astype(np.float64), -2 * e)
    s = exact.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), exact), "a total is no exact f32"
    if mode == 1:
        s = np.clip(s, np.float32(0), np.float32(1))
        alive &= s >= np.float32(thr)
    idx = np.flatnonzero(alive)
    if idx.shape[0] > k:       # (the k-th value first: the sort below then sees the candidates only)
        kth = np.partition(s[idx], idx.shape[0] - k)[idx.shape[0] - k]
        idx = idx[s[idx] >= kth]
    idx = idx[np.lexsort((idx, -s[idx].astype(np.float64)))[:k]]
    assert not (S_int[idx] == 0).any(), "an expected row has a zero total: +0 and -0 are both right"
    return idx.astype(np.uint64), s[idx]


def assert_exact(got_rows, got_scores, count, exp_ids, exp_scores, what=""):
    """An equal count, an identical id list, equal score bits.  Says where the first difference is."""
    c = int(count)
    got_rows = np.asarray(got_rows).reshape(-1)[:c].astype(np.uint64)
    got_bits = np.ascontiguousarray(np.asarray(got_scores, dtype=np.float32).reshape(-1)[:c]).view(np.uint32)
    exp_ids = np.asarray(exp_ids, dtype=np.uint64)
    exp_bits = np.ascontiguousarray(exp_scores, dtype=np.float32).view(np.uint32)
    m = min(c, exp_ids.shape[0])
    bad = np.flatnonzero((got_rows[:m] != exp_ids[:m]) | (got_bits[:m] != exp_bits[:m]))
    if bad.shape[0]:
        p = int(bad[0])
        raise AssertionError("%s: position %d: expected row %d score %r (0x%08x), got row %d score %r (0x%08x); %d of %d positions differ"
                             % (what, p, exp_ids[p], float(exp_bits[p:p + 1].view(np.float32)[0]), exp_bits[p], got_rows[p],
                                float(got_bits[p:p + 1].view(np.float32)[0]), got_bits[p], bad.shape[0], m))
    assert c == exp_ids.shape[0], "%s: count %d, expected %d (the first %d positions agree)" % (what, c, exp_ids.shape[0], m)


# ---- the cases of tests/test_scan_exact_gpu.py (the CPU test walks the same ones) -----------------------------------
GEMV_N = 300
GEMV_FULL_MINUS_4 = (1, 3, 4, 8, 16)
ROW_EDGES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
MFMA_N, MFMA_WIDTH = 4097, 256
QUEUE_N = 80001
QUEUE_WINDOWS = [(0, 256), (30000, 30256), (60101, 60357), (79489, 79745), (79745, 80001)]


def gemv_dims(c):
    """Dims of chunk count c: the full last chunk, the smallest partial one and, for some c, the largest partial one."""
    return sorted({256 * c, 256 * (c - 1) + 4} | ({256 * c - 4} if c in GEMV_FULL_MINUS_4 else set()))


def gemv_blocks(c):
    return (1, 2, 3, 4, 5, 7, 8) if c <= 4 else ((1, 2, 3) if c <= 8 else (1, 2))


@functools.lru_cache(maxsize=4)
def gemv_case(dim, nq=None):
    return dyadic(GEMV_N, dim, 1000 + dim, nq=max(gemv_blocks((dim + 255) // 256)) if nq is None else nq)


def edge_cases(n, dim):
    """The row-count edge corpus of n rows: windows of 1024 rows, eight queries.  Four columns hold three windows at most, so
    there the windows are spread over as many corpora as it takes."""
    wins = default_windows(n, MAX_K)
    per = min(len(wins), dim - 1)
    return [dyadic(n, dim, 2000 + n + dim + g, nq=8, windows=wins[g:g + per]) for g in range(0, len(wins), per)]


@functools.lru_cache(maxsize=2)
def mfma_case(dim, nq=300, dot=False):
    """4097 rows (the last 64-row tile holds one row), 17 windows of 256 rows (the last one holds that row alone)."""
    return dyadic(MFMA_N, dim, 3000 + dim, nq=nq, width=MFMA_WIDTH, dot=dot)


@functools.lru_cache(maxsize=2)
def queue_case(dim, nq=256, n=QUEUE_N):
    """More row tiles than workgroups: the kernels continue from the work queue.  Windows over the first, the last full and
    two interior tiles and over the ragged end (a corpus of another size: the same places, scaled)."""
    wins = QUEUE_WINDOWS if n == QUEUE_N else [(lo * n // QUEUE_N, lo * n // QUEUE_N + 256) for lo, _ in QUEUE_WINDOWS[:3]] + [(n - 512, n - 256), (n - 256, n)]
    return dyadic(n, dim, 4000 + dim + n, nq=nq, windows=wins)


def plan_tiers(n_pad, n_cu):
    """(nA, nB, nC) 64- / 32- / 16-row tasks of the gemv scan over n_pad rows (scan_kernels.hip, plan_tiers)."""
    n64, waves = n_pad // 64, n_cu * 4
    if n64 < 8 * n_cu:
        return 0, 0, n_pad // 16
    nb = (2 * (waves // 2)) & ~1
    if n64 >= 6 * waves and n64 > nb // 2:
        return n64 - nb // 2, nb, 0
    return n64, 0, 0


TIERS = ("rows16", "rows64", "rows64+32", "persistent")
TIER_DIM = 16


def tier_rows(name, n_cu):
    """n just past each plan change of plan_tiers / launch_gemv on a device of n_cu compute units (n_pad = n rounded up to
    256): the last size of 16-row tasks, the first of 64-row tasks, the first with the 32-row tail, the first whose tasks
    exceed 4 n_cu x 24 (the persistent grid)."""
    n64 = {"rows16": 8 * n_cu - 4, "rows64": 8 * n_cu, "rows64+32": 24 * n_cu, "persistent": 94 * n_cu + 4}[name]
    return 64 * n64 - 255 + (0 if name != "rows16" else 100)


@functools.lru_cache(maxsize=2)
def tier_case(name, n_cu):
    """Windows of 1024 rows at the first rows, across the seam of the tiers (64 nA; the middle of the corpus where there is
    one tier), over the last full tasks and, 300 rows, over the ragged end.  Two queries per window."""
    n = tier_rows(name, n_cu)
    nA, nB, nC = plan_tiers((n + 255) // 256 * 256, n_cu)
    seam = 64 * nA if nB else (n // 2 + 13)
    wins = [(0, 1024), (seam - 512, seam + 512), (n - 1324, n - 300), (n - 300, n)]
    c = dyadic(n, TIER_DIM, 5000 + n, nq=8, windows=wins)
    c.tiers = (nA, nB, nC)
    return c


def families(n_cu=256):
    """(name, thunk -> Case) of every (n, dim) family the GPU file uses; the tier sizes for a device of n_cu compute units."""
    out = []
    for c in range(1, 17):
        for dim in gemv_dims(c):
            out.append(("gemv 300x%d" % dim, functools.partial(gemv_case, dim)))
    out.append(("gemv 300x100", functools.partial(gemv_case, 100, 13)))
    for n in ROW_EDGES:
        for dim in (768, 4):
            wins = len(default_windows(n, MAX_K))
            for g in range(-(-wins // min(wins, dim - 1))):
                out.append(("edge %dx%d/%d" % (n, dim, g), (lambda n=n, dim=dim, g=g: edge_cases(n, dim)[g])))
    for dim in (32, 96, 256, 384, 512, 768, 1024, 2048, 4096):
        out.append(("mfma 4097x%d" % dim, functools.partial(mfma_case, dim, 40)))
    out.append(("dot 4097x768", functools.partial(mfma_case, 768, 40, True)))
    for dim in (32, 256):
        out.append(("queue 80001x%d" % dim, functools.partial(queue_case, dim, 256 if dim == 32 else 64)))
    out.append(("queue %dx32" % (512 * n_cu + 257), functools.partial(queue_case, 32, 64, 512 * n_cu + 257)))
    for name in TIERS:
        out.append(("tier %s" % name, functools.partial(tier_case, name, n_cu)))
    return out
