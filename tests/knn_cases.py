"""Exact-arithmetic corpora for the kNN graph (cqs_hip_index_knn_graph) and the graph every correct
implementation returns on them, bit for bit.  No GPU and no library here: tests/test_knn_gpu.py takes its inputs and its
expected values from this file and holds it to the oracle's find_neighbors on the CPU.

Entries are small integers times 2^-e (e = 0 for a dot-metric handle).  A product is at most 16 units of 2^-2e and a dot
of two rows at most 9 + 16 (dim - 1) < 2^14 units, so every product and every partial sum, in any order and in any tree,
is an exact f32: the score of (target, row) is an entry of the integer Gram matrix, scaled, whichever kernel computed it.
Column 0 is odd and every other column is even in every row, so every total is odd: never +0 or -0, which have different
ordered keys.  e is the smallest with |row|^2 <= 1 for every possible row (the cosine handle's linear bins).

Small integers collide: most score lists hold exact ties, resolved by row ascending.  On top of that a RUN of duplicates
of one row is planted, longer than any k1 (101) where the corpus has room: the row has the largest norm a row can have,
so to each member of the run the other members are its top scorers, all tied, and for a member late in the run more than
k1 of them precede it - its own key is not among the k1 the select returns, the case where the finish drops the last
key instead of the target's."""
import functools
import math

import numpy as np

NEIGHBORS_MAX = 100
RUN = 105            # > NEIGHBORS_MAX + 1: hides its late members at every limit
SIZES = (1, 2, 5, 257, 259, 700)
DIMS = (64, 768)
LIMITS = (0, 1, 15, 100, 101)


def clamp(limit):
    return max(1, min(int(limit), NEIGHBORS_MAX))


def run_of(n):
    """(first row, length) of the planted duplicate run in a corpus of n rows; length 0: no room for one."""
    if n >= 2 * RUN:
        first = 200 if n >= 200 + RUN + 100 else n // 3      # (n = 700: rows 200 .. 304, across the tile boundary at 256)
        return first, RUN
    if n >= 5:
        return 1, 3                                          # hides its third member at limit 1 (k1 = 2)
    return 0, 0


class Case:
    """n, dim, e, dot, C int64 [n, dim], G int64 [n, n] = C C^T, rows f32 [n, dim], run (first, length)."""

    def scores_f32(self, g):
        exact = np.ldexp(np.asarray(g, dtype=np.float64), -2 * self.e)
        s = exact.astype(np.float32)
        assert np.array_equal(s.astype(np.float64), exact), "a total is no exact f32"
        return s


@functools.lru_cache(maxsize=None)
def dyadic(n, dim, dot=False, seed=0):
    rng = np.random.default_rng(7000 + 31 * n + dim + seed)
    sign = lambda shape: rng.choice(np.asarray([-1, 1], dtype=np.int64), size=shape)
    C = rng.choice(np.asarray([2, 4], dtype=np.int64), size=(n, dim)) * sign((n, dim))
    C[:, 0] = rng.choice(np.asarray([1, 3], dtype=np.int64), size=n) * sign(n)
    first, length = run_of(n)
    if length:
        top = np.full(dim, 4, dtype=np.int64) * sign(dim)    # the largest norm a row can have
        top[0] = 3 * sign(1)[0]
        C[first:first + length] = top
    top_norm = 9 + 16 * (dim - 1)
    assert top_norm < 2 ** 24, "a partial sum could leave the exact f32 integers"
    c = Case()
    c.n, c.dim, c.dot, c.C, c.run = n, dim, dot, C, (first, length)
    c.e = 0 if dot else math.ceil(math.log2(top_norm) / 2)
    assert dot or top_norm <= 1 << (2 * c.e), "|row|^2 must stay <= 1"
    c.G = C @ C.T
    assert (c.G % 2 != 0).all(), "every total must be odd"
    c.rows = np.ldexp(C.astype(np.float32), -c.e)
    return c


def expected_graph(case, limit, row_base=0):
    """(rows u64 [n, L], scores f32 [n, L], counts u32 [n]) from the integer Gram matrix: per target the other rows by
    (score descending, row ascending), the first L = clamp(limit) of them; zeros past the count."""
    L, n = clamp(limit), case.n
    rows = np.zeros((n, L), dtype=np.uint64)
    scores = np.zeros((n, L), dtype=np.float32)
    counts = np.full(n, min(L, n - 1), dtype=np.uint32)
    c = min(L, n - 1)
    if c == 0:
        return rows, scores, counts
    others = np.arange(n)
    for t in range(n):
        g = case.G[t]
        cand = others[others != t]
        order = cand[np.lexsort((cand, -g[cand]))[:c]]
        rows[t, :c] = order.astype(np.uint64) + np.uint64(row_base)
        scores[t, :c] = case.scores_f32(g[order])
    return rows, scores, counts


def hidden_targets(case, limit):
    """Members of the planted run whose own key is NOT among the k1 = min(L + 1, n) best: at least k1 duplicates precede them."""
    first, length = case.run
    k1 = min(clamp(limit) + 1, case.n)
    return [first + j for j in range(length) if j >= k1]


def drop_self(rows, scores, counts, targets, limit):
    """cqs_search::drop_self over a block of search answers (rows [b, k], scores, counts; targets [b] global rows): the
    first `limit` results that are not the target, in arrays of stride `limit`, zeros past each count."""
    b = len(targets)
    out_rows = np.zeros((b, limit), dtype=np.uint64)
    out_scores = np.zeros((b, limit), dtype=np.float32)
    out_counts = np.zeros(b, dtype=np.uint32)
    for i in range(b):
        c = int(counts[i])
        keep = np.flatnonzero(rows[i, :c] != np.uint64(targets[i]))[:limit]
        out_rows[i, :len(keep)] = rows[i, keep]
        out_scores[i, :len(keep)] = scores[i, keep]
        out_counts[i] = len(keep)
    return out_rows, out_scores, out_counts
