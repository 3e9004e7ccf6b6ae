"""Helpers of the MMR tests (no tests here): a numpy restatement of the reference's `mmr_rerank`
(src/search/mmr.rs:59-126) over an explicit similarity matrix, the float64 Gram matrix, and the case generators
tests/test_mmr_cpu.py and tests/test_mmr_gpu.py share."""
import numpy as np


def total_order_keys(x):
    """f32 array -> u32 keys whose unsigned order is `f32::total_cmp`'s (mmr.rs:107)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


_NEG_INF_KEY = int(total_order_keys(np.array([-np.inf], np.float32))[0])


def mmr_rerank(scores, sim, limit, lam, running_max=False):
    """`mmr_rerank` with similarity(i, j) = sim[i][j]: f32 arithmetic, the two products and the difference each rounded
    (numpy never fuses), winner by total order, lowest index among equals.  running_max=False re-folds `max` over the
    selected from 0.0 at every step as mmr.rs:83-90 does; True keeps a running maximum (what the device kernel does)."""
    lam = np.float32(lam)
    lam = np.float32(min(max(lam, np.float32(0.0)), np.float32(1.0)))           # :60
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    n = scores.shape[0]
    limit = min(int(limit), n)                                                  # :62
    if limit == 0:                                                              # :64-66
        return []
    if lam >= np.float32(1.0) or n <= limit:                                    # :67-69
        return list(range(limit))
    sim = np.asarray(sim, dtype=np.float32).reshape(n, n)
    one_minus = np.float32(1.0) - lam
    selected, mask = [], np.zeros(n, dtype=bool)
    run = np.zeros(n, dtype=np.float32)
    while len(selected) < limit:                                                # :74
        if running_max:
            max_sim = run
        else:
            max_sim = np.zeros(n, dtype=np.float32)                             # fold(0.0f32, f32::max), :83-90
            for j in selected:
                max_sim = np.fmax(max_sim, sim[:, j])                           # (f32::max drops a NaN operand: fmax)
        rel = lam * scores                                                      # :92, each operation rounded to f32
        div = one_minus * max_sim
        mmr = rel - div
        assert rel.dtype == div.dtype == mmr.dtype == np.float32
        keys = total_order_keys(mmr).astype(np.int64)
        keys[mask] = -1
        best = int(np.argmax(keys))                                             # first maximum = lowest index, :107-111
        if keys[best] < _NEG_INF_KEY:                                           # nothing beats NEG_INFINITY, :118-120
            break
        mask[best] = True
        selected.append(best)
        run = np.fmax(run, sim[:, best])
    return selected


def gram64(rows):
    r = np.asarray(rows, dtype=np.float64)
    return r @ r.T


def unit_rows(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def clustered_unit_rows(n, dim, seed, clusters=24, noise=0.35):
    """Unit rows around a few centres: similarities spread over (0, 1), so the diversity term decides picks."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[rng.integers(0, clusters, n)] + noise * rng.standard_normal((n, dim)) / np.sqrt(dim)   # |noise term| ~ noise
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def exact_rows(n, dim, seed):
    """Entries from {-1, 0, 1} / 8: every dot of two rows is a multiple of 2^-6 of magnitude <= dim / 64, exact in f32 in
    any summation order (dim = 64: magnitude <= 1)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-1, 2, (n, dim)).astype(np.float32) / np.float32(8.0)).astype(np.float32)


def exact_pool(n_rows, m, seed):
    """(candidate local rows, scores) for exact_rows: duplicate rows and duplicate scores (multiples of 2^-8 in [0, 1],
    few distinct values), so exact ties occur at most steps."""
    rng = np.random.default_rng(seed)
    distinct = rng.choice(n_rows, size=max(2, m // 3), replace=False)
    cand = rng.choice(distinct, size=m, replace=True)
    scores = np.sort(rng.integers(0, 17, m).astype(np.float32) * np.float32(16.0 / 256.0))[::-1]
    return cand.astype(np.uint64), np.ascontiguousarray(scores, dtype=np.float32)


def random_pool(rng, m):
    """A random symmetric similarity matrix with negative entries and ties, and descending scores (CPU tests)."""
    a = np.round(rng.uniform(-0.5, 1.0, (m, m)) * 16) / 16
    sim = np.triu(a) + np.triu(a, 1).T
    scores = np.sort(np.round(rng.uniform(0, 1, m) * 32) / 32)[::-1]
    return scores.astype(np.float32), sim.astype(np.float32)
