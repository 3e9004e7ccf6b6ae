"""Shared data and expectations of the match tests (`cqs_hip_index_match`).  No GPU and no library here:
tests/test_match_gpu.py takes its inputs and expected values from this file, tests/test_match_host_cpu.py holds the file's
own rules to brute force and to cqs_amd/csrc/match_host.h.

The rule under test: S[i][j] is the f32 dot of two stored rows; a row's best partner is the position on the other side
with the greatest entry under the f32 total order, the lowest position among equals, finite entries only; no finite entry
-> (NONE, 0.0)."""
import numpy as np

NONE = 0xFFFFFFFFFFFFFFFF
MATCH_MAX = 65536
LENGTHS = (1, 31, 32, 33, 64, 65, 97)          # under a tile, a tile, one past; two tiles, one past; three tiles and one row
GENERAL_DIMS = (4, 36, 100, 768)               # under one 8-float step; one 32-float loop trip + a tail; three trips + a tail; the workload's


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def order_keys(s):
    """f32 array -> int64 array in the order of f32::total_cmp; non-finite entries -> -1 (below every finite one)."""
    b = bits(s).astype(np.int64)
    k = np.where(b >> 31, 0xFFFFFFFF - b, b ^ 0x80000000)
    return np.where(np.isfinite(np.asarray(s, np.float32)), k, -1)


def expected_side(s):
    """S [rows, others] f32 -> (best u64 [rows], score f32 [rows]) of each row over the other side."""
    s = np.ascontiguousarray(s, np.float32)
    rows, others = s.shape
    best = np.full(rows, NONE, np.uint64)
    score = np.zeros(rows, np.float32)
    if others == 0:
        return best, score
    k = order_keys(s)
    arg = np.argmax(k, axis=1)                  # (the first of equal maxima: the lowest position)
    has = k[np.arange(rows), arg] >= 0
    best[has] = arg[has].astype(np.uint64)
    score[has] = s[np.arange(rows), arg][has]
    return best, score


def expected_bests(s):
    """S [m_a, m_b] -> (best_a, score_a, best_b, score_b)."""
    s = np.ascontiguousarray(s, np.float32)
    return expected_side(s) + expected_side(np.ascontiguousarray(s.T))


def brute_side(s):
    """expected_side by a plain double loop over python floats and bit keys (the check of the vectorised form)."""
    s = np.ascontiguousarray(s, np.float32)
    best, score = [], []
    for i in range(s.shape[0]):
        top, at = None, NONE
        for j in range(s.shape[1]):
            v = s[i, j]
            if not np.isfinite(v):
                continue
            b = int(v.view(np.uint32))
            k = (0xFFFFFFFF - b) if b >> 31 else (b ^ 0x80000000)
            if top is None or k > top:
                top, at = k, j
        best.append(at)
        score.append(np.float32(0.0) if top is None else s[i, at])
    return np.asarray(best, np.uint64), np.asarray(score, np.float32)


def brute_mutual(best_a, score_a, best_b, threshold):
    thr = np.float32(threshold)
    return [(i, int(best_a[i])) for i in range(len(best_a))
            if int(best_a[i]) != NONE and int(best_b[int(best_a[i])]) == i and np.float32(score_a[i]) >= thr]


def tie_matrix(m_a, m_b, seed, non_finite=True):
    """Scores that are multiples of 1/16 in [-1, 1] from few distinct values: exact ties in most rows and columns; with
    `non_finite`, inf / -inf / NaN entries scattered, one row and one column wholly non-finite, and both zeros."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(-3, 4, (m_a, m_b)).astype(np.float32) / np.float32(16.0)).astype(np.float32)
    s[s == 0] = rng.choice(np.array([0.0, -0.0], np.float32), size=int((s == 0).sum()))
    if non_finite and m_a and m_b:
        bad = rng.random((m_a, m_b)) < 0.1
        s[bad] = rng.choice(np.array([np.inf, -np.inf, np.nan], np.float32), size=int(bad.sum()))
        s[m_a // 2, :] = np.nan
        s[:, m_b // 3] = np.inf
    return s


# ---- exact data: entries are multiples of 1/8, every dot exact in any order -------------------------------------------
EXACT_DIM, EXACT_NA, EXACT_NB = 64, 200, 300


def exact_rows(n, dim, seed):
    """Entries from {-1, 0, 1} / 8 (tests/mmr_cases.py's exact_rows): a dot is a multiple of 2^-6 of magnitude <= dim / 64."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-1, 2, (n, dim)).astype(np.float32) / np.float32(8.0)).astype(np.float32)


def exact_corpora():
    a, b = exact_rows(EXACT_NA, EXACT_DIM, 11), exact_rows(EXACT_NB, EXACT_DIM, 12)
    b[17] = a[5]                                # one row of b is a row of a: its dot with it is the squared norm
    b[250] = a[5]
    return a, b


def exact_scores(a, b):
    """[n_a, n_b] f32 by integer arithmetic: (8 a) (8 b)^T / 64.  A zero total is +0.0: the device's chain starts from
    +0.0 and round-to-nearest sums never give -0.0 from it."""
    ia, ib = np.rint(a.astype(np.float64) * 8).astype(np.int64), np.rint(b.astype(np.float64) * 8).astype(np.int64)
    return ((ia @ ib.T).astype(np.float64) / 64.0).astype(np.float32)


def row_list(n, m, seed):
    """m local rows of an index of n rows, in no order, drawn from few distinct rows: duplicated rows at several
    positions (so exact ties between positions) at every length above 2; both ends of the index among them."""
    rng = np.random.default_rng(seed)
    distinct = rng.choice(n, size=max(1, min(n, (2 * m + 2) // 3)), replace=False)
    distinct[0] = n - 1
    if len(distinct) > 1:
        distinct[1] = 0
    rows = rng.choice(distinct, size=m, replace=True)
    rows[:min(m, len(distinct))] = distinct[:min(m, len(distinct))]
    return rng.permutation(rows).astype(np.uint64)


# ---- general data ------------------------------------------------------------------------------------------------------
def gaussian_rows(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- the mid-size case against numpy f64 -----------------------------------------------------------------------------
MID_N, MID_DIM, MID_MA, MID_MB, MID_SEED = 5000, 768, 1000, 3000, 2024
MID_SCORE_TOL = 1e-5          # the library's parity tolerance
MID_TIE_BAND = 2e-6           # best and runner-up closer than this: either may win on the device
MID_TIE_SHARE = 0.01          # at most this share of rows inside the band (asserted on the CPU and in the GPU test)


def mid_case():
    """(a, b, rows_a, rows_b): two 5 000 x 768 indexes of unit Gaussian rows and lists of 1 000 and 3 000 distinct rows."""
    a, b = gaussian_rows(MID_N, MID_DIM, MID_SEED), gaussian_rows(MID_N, MID_DIM, MID_SEED + 1)
    rng = np.random.default_rng(MID_SEED + 2)
    return a, b, rng.choice(MID_N, MID_MA, replace=False).astype(np.uint64), rng.choice(MID_N, MID_MB, replace=False).astype(np.uint64)


def mid_reference(a, b, rows_a, rows_b):
    """numpy f64: per side (best, best score, clear: the runner-up is more than MID_TIE_BAND below the best)."""
    s = a[rows_a.astype(np.int64)].astype(np.float64) @ b[rows_b.astype(np.int64)].astype(np.float64).T

    def side(m):
        order = np.argsort(-m, axis=1, kind="stable")[:, :2]
        top, second = m[np.arange(m.shape[0]), order[:, 0]], m[np.arange(m.shape[0]), order[:, 1]]
        return order[:, 0].astype(np.uint64), top, (top - second) > MID_TIE_BAND

    return side(s), side(np.ascontiguousarray(s.T))


# ---- a numpy stand-in for HipIndex._match_block (the Python logic's tests) -----------------------------------------------
class FakeMatcher:
    """What HipIndex.match_rows / semantic_diff need of a HipIndex, with the device call done by numpy over a given
    [n_self, n_other] f32 score matrix of local rows."""

    def __init__(self, scores, base=0, ids=None):
        self.scores, self.base, self.id_map, self.calls = np.ascontiguousarray(scores, np.float32), base, ids, []

    def _match_block(self, other, rows_a, rows_b):
        assert len(rows_a) <= MATCH_MAX and len(rows_b) <= MATCH_MAX
        self.calls.append((len(rows_a), len(rows_b)))
        la, lb = np.asarray(rows_a, np.int64) - self.base, np.asarray(rows_b, np.int64) - other.base
        return expected_bests(self.scores[np.ix_(la, lb)].reshape(len(la), len(lb)))

    def _all_ids(self):
        return self.id_map

    def _row_base(self):
        return self.base
