"""Exact-arithmetic corpora and pair lists for the semantic diff (cqs_hip_index_diff), and the answer every
correct implementation gives on them.

A row has 0, 1, 4 or 16 non-zero entries, all of one magnitude 2^t with signs of their own.  Every product of two entries is
then +-2^(ta + tb), every sum of at most 16 of them is exact in f64 in any order, a squared norm is k * 4^t with k in
{1, 4, 16} - a perfect square - and the cosine of two rows is (signed overlap) / sqrt(ka * kb), a multiple of 1/16: exact in
f32.  So the reference's left-to-right loop, a wave butterfly and numpy all give the same bits, and `expected_sims` below is
that value; tests/test_diff_host_cpu.py holds it to oracle.full_cosine_similarity pair by pair without a GPU.

Corpus B's first rows are made from corpus A's: row 0 all zero in both (undefined: sim 0.0, counted), B[1] = A[1], B[2] = -A[2],
B[3] orthogonal to A[3] (disjoint support), B[4] = A[4] scaled by 2^5.  `pairs(m)` starts with those five pairs and goes on
with random ones; the list for m is a prefix of the list for any larger m."""
import numpy as np

DIMS = (4, 8, 252, 768, 4096)
MS = (1, 63, 64, 65, 257, 1000)
ROWS = 300


def _positions(dim):
    """Where non-zeros may fall: both ends of the row, so that a lost tail or a lost first piece shows."""
    head = list(range(min(dim, 12)))
    tail = [p for p in range(max(0, dim - 12), dim) if p not in head]
    return np.array(head + tail)


def _row(rng, dim, k, t):
    v = np.zeros(dim, np.float32)
    pos = rng.choice(_positions(dim), size=k, replace=False)
    v[pos] = np.float32(2.0 ** t) * rng.choice(np.array([-1.0, 1.0], np.float32), size=k)
    return v


def corpus(dim, seed, rows=ROWS):
    rng = np.random.default_rng(seed)
    ks = [k for k in (1, 4, 16) if k <= min(dim, len(_positions(dim)))]
    out = np.zeros((rows, dim), np.float32)
    for i in range(1, rows):
        out[i] = _row(rng, dim, int(rng.choice(ks)), int(rng.integers(-20, 21)))
    return out


def corpora(dim):
    """(A, B) with the special first rows described above."""
    a, b = corpus(dim, 1000 + dim), corpus(dim, 2000 + dim)
    b[1] = a[1]
    b[2] = -a[2]
    pos = _positions(dim)
    a[3] = 0
    b[3] = 0
    a[3, pos[0]] = 4.0
    b[3, pos[-1] if pos[-1] != pos[0] else pos[1]] = -0.5
    b[4] = a[4] * np.float32(32.0)
    return a, b


def pairs(m, rows=ROWS, seed=77):
    """(rows of A, rows of B) of m pairs, local row numbers: the five special pairs, then random ones (rows repeat)."""
    rng = np.random.default_rng(seed)
    ra = np.concatenate([np.arange(5), rng.integers(0, rows, 1000)]).astype(np.uint64)
    rb = np.concatenate([np.arange(5), rng.integers(0, rows, 1000)]).astype(np.uint64)
    return ra[:m].copy(), rb[:m].copy()


def expected_sims(a, b, ra, rb):
    """(sims f32 [m], undefined bool [m]): `full_cosine_similarity(a[ra[i]], b[rb[i]]).unwrap_or(0.0)` and whether it was None."""
    x, y = a[ra.astype(np.int64)].astype(np.float64), b[rb.astype(np.int64)].astype(np.float64)
    dot, na, nb = (x * y).sum(axis=1), (x * x).sum(axis=1), (y * y).sum(axis=1)
    denom = np.sqrt(na) * np.sqrt(nb)
    undefined = denom == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        sims = np.where(undefined, 0.0, dot / np.where(undefined, 1.0, denom)).astype(np.float32)
    return sims, undefined


def thresholds(sims, undefined):
    """-1.0, 0.0, a value equal to one defined pair's sim (that pair is unchanged), 1.0, +inf, -inf."""
    defined = np.sort(np.unique(sims[~undefined])) if (~undefined).any() else np.array([0.25], np.float32)
    return [np.float32(-1.0), np.float32(0.0), np.float32(defined[len(defined) // 2]), np.float32(1.0), np.float32(np.inf), np.float32(-np.inf)]


def expected_answer(sims, undefined, threshold):
    """(mod_pairs u64, mod_sims f32, counts [modified, unchanged, undefined]) of diff.rs:191-202 on these sims."""
    mod = np.flatnonzero(sims < np.float32(threshold)).astype(np.uint64)
    return mod, sims[mod.astype(np.int64)], [len(mod), len(sims) - len(mod), int(undefined.sum())]
