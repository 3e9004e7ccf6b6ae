"""The UMAP transform's rules (include/cqs_hip.h, "UMAP transform of new rows") restated in numpy on top of
tests/umap_cases.py: f64 where the header says f32 arithmetic may differ, exact f32 / u32 where it fixes the bits
(distances, the active rule, the hash, the draws, alpha).  Also the in-place variant the header departs from, the case
generators of the transform's tests, the hold-out corpus and its two quality measures.

Run as a script it repeats the prototype of DESIGN.md §3.18a - synchronous rule, in-place rule, initial position only and a
uniform-random placement on the hold-out corpus over SEEDS - and prints the table recorded there."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import umap_cases as uc  # noqa: E402

SEEDS = uc.SEEDS
HELD_OUT_PER_CLUSTER = 20
# The prototype as recorded in DESIGN.md §3.18a (this file run as a script): the synchronous restatement over SEEDS,
# E = 100, the 15 nearest anchors.  SPREAD = max - min; the device's quality test allows three times it.
RECORDED_SYNC_KEPT = (0.259, 0.262, 0.258, 0.283, 0.254)
RECORDED_SYNC_PURITY = (0.995, 0.965, 0.970, 0.979, 0.993)
KEPT_SPREAD = 0.029
PURITY_SPREAD = 0.030


# ---- exact-bit rules ----------------------------------------------------------------------------------------------------
def default_epochs(m):
    return 100 if m <= 10000 else 30


def alpha_of(lr, e, E):
    """f32: (lr / 4) * (1 - (e - 1) / E), each operation rounded once."""
    done = np.float32(e - 1) / np.float32(E)
    return (np.float32(lr) * np.float32(0.25)) * (np.float32(1.0) - done)


# ---- weights and initial position, f64 ------------------------------------------------------------------------------------
def weights_of(scores):
    """(sigma f64, w f64 [c]) of one new vertex's f32 scores: rho = 0, target = log2(c), the bisection in f64."""
    d = uc.distances(np.asarray(scores, dtype=np.float32)).astype(np.float64)
    c = len(d)
    if c == 0:
        return 0.0, np.zeros(0)
    target = np.log2(float(c))
    lo, hi, mid = 0.0, np.inf, 1.0
    for _ in range(64):
        with np.errstate(over="ignore", under="ignore"):
            psum = float(np.where(d > 0, np.exp(-d / mid), 1.0).sum())
        if abs(psum - target) < 1e-5:
            break
        if psum > target:
            hi = mid
            mid = (lo + hi) / 2.0
        else:
            lo = mid
            mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
    sigma = max(mid, 1e-3 * float(d.mean()))
    with np.errstate(under="ignore"):
        return sigma, np.where(d <= 0, 1.0, np.exp(-d / sigma))


def weights(scores, counts):
    """(sigma f64 [m], w f64 [m, stride], 0 past the counts)."""
    scores, counts = np.asarray(scores, dtype=np.float32), np.asarray(counts)
    sigma, w = np.zeros(len(counts)), np.zeros(scores.shape)
    for i, c in enumerate(counts):
        sigma[i], w[i, :int(c)] = weights_of(scores[i, :int(c)])
    return sigma, w


def initial(anchors, rows, counts, w):
    """(y f64 [m, 2], per-coordinate sum of |q_t Y_t| f64 [m, 2], placed bool [m]) from weights `w` [m, stride] (the
    device's f32 or the restatement's).  A vertex with no entries or W == 0 is the origin and `placed` is False."""
    Y = np.asarray(anchors, dtype=np.float64)
    rows, counts, w = np.asarray(rows).astype(np.int64), np.asarray(counts), np.asarray(w, dtype=np.float64)
    valid = np.arange(rows.shape[1])[None, :] < counts[:, None]
    w = np.where(valid, w, 0.0)
    W = w.sum(axis=1)
    placed = W > 0
    q = w / np.where(placed, W, 1.0)[:, None]
    terms = q[:, :, None] * Y[np.where(valid, rows, 0)]
    terms = np.where((valid & placed[:, None])[:, :, None], terms, 0.0)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1), placed


# ---- the epochs -----------------------------------------------------------------------------------------------------------
def _term(coef_kind, a, b, repulsion, y, other):
    dy = y - other
    d2 = (dy * dy).sum(axis=1)
    ca, cr = uc._coeffs(a, b, repulsion, d2)
    coef = np.where(d2 > 0, ca if coef_kind == "a" else cr, 0.0)
    return np.where((d2 > 0)[:, None], np.clip(coef[:, None] * dy, -4.0, 4.0), 0.0)


def epoch(anchors, rows, counts, w32, y, placed, e, E, seed, id_base, a=uc.A_DEFAULT, b=uc.B_DEFAULT, lr=1.0, repulsion=1.0,
          negative_samples=5, in_place=False):
    """One epoch in f64 from positions `y` [m, 2].  `w32` [m, stride] is taken as f32 (the device's, or the restatement's
    rounded), so the active flags are the device's.  Returns (y_new f64, the per-vertex, per-coordinate sum of |terms|).
    `in_place` is umap-learn's rule, which the header departs from: y moves after every term."""
    Y = np.asarray(anchors, dtype=np.float64)
    n = len(Y)
    rows, counts = np.asarray(rows).astype(np.int64), np.asarray(counts)
    y = np.asarray(y, dtype=np.float64).copy()
    m, stride = rows.shape
    a, b, repulsion = float(np.float32(a)), float(np.float32(b)), float(np.float32(repulsion))
    alpha = float(alpha_of(lr, e, E))
    w32 = np.where(np.arange(stride)[None, :] < counts[:, None], np.asarray(w32, dtype=np.float32), np.float32(0.0))
    top = w32.max(axis=1) if stride else np.zeros(m, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(top[:, None] > 0, w32 / top[:, None], np.float32(0.0)).astype(np.float32)
    ids = (np.uint64(id_base) + np.arange(m, dtype=np.uint64)).astype(np.uint32)
    total, mass = np.zeros((m, 2)), np.zeros((m, 2))
    for t in range(int(counts.max()) if m else 0):
        act = (t < counts) & placed & uc.active(e, p[:, t])
        if not act.any():
            continue
        v = np.nonzero(act)[0]
        others = [Y[rows[v, t]]] + [Y[uc.draw_vertex(uc.hash5(seed, e, ids[v], t, k), n).astype(np.int64)]
                                    for k in range(int(negative_samples))]
        for i, other in enumerate(others):
            term = _term("a" if i == 0 else "r", a, b, repulsion, y[v], other)
            total[v] += term
            mass[v] += np.abs(term)
            if in_place:
                y[v] += alpha * term
    return (y if in_place else y + alpha * total), mass


def transform(anchors, rows, scores, counts, id_base=None, n_epochs=0, epochs=None, seed=42, in_place=False, **kw):
    """The full run in f64: weights, initial position, then `epochs` (default: all) of the E epochs."""
    rows, counts = np.asarray(rows), np.asarray(counts)
    E = n_epochs or default_epochs(len(counts))
    _, w = weights(scores, counts)
    y, _, placed = initial(anchors, rows, counts, w)
    w32 = w.astype(np.float32)
    base = len(anchors) if id_base is None else id_base
    for e in range(1, (E if epochs is None else min(epochs, E)) + 1):
        y, _ = epoch(anchors, rows, counts, w32, y, placed, e, E, seed, base, in_place=in_place, **kw)
    return y


# ---- case generators ------------------------------------------------------------------------------------------------------
def random_lists(seed, n, m, stride, counts=None, dup_every=0, zero_vertex=None, odd_vertex=None):
    """(rows u64 [m, stride], scores f32 [m, stride] descending, counts u32 [m]) over n anchors; ids may repeat in a list
    where n is small.  `counts`: cycled over the vertices (clamped at stride), else random in [0, stride].  `dup_every`:
    every such slot has score 1.0 (d = 0); `zero_vertex`: all of its entries at d = 0; `odd_vertex`: scores above 1 and
    below 0 among its entries."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((m, stride), dtype=np.uint64)
    scores = np.zeros((m, stride), dtype=np.float32)
    cnt = np.zeros(m, dtype=np.uint32)
    for i in range(m):
        c = min(stride, int(counts[i % len(counts)])) if counts is not None else int(rng.integers(0, stride + 1))
        pick = rng.choice(n, size=c, replace=c > n)
        sc = rng.uniform(-0.2, 0.999, size=c).astype(np.float32)
        if dup_every:
            sc[::dup_every] = 1.0
        if i == zero_vertex:
            sc[:] = 1.0
        if i == odd_vertex and c:
            sc[0] = 1.5
            sc[-1] = -0.75
        rows[i, :c], scores[i, :c], cnt[i] = pick, np.sort(sc)[::-1], c
    return rows, scores, cnt


def random_anchors(seed, n, scale=10.0):
    return np.random.default_rng(seed).uniform(-scale, scale, size=(n, 2)).astype(np.float32)


# ---- the hold-out corpus ----------------------------------------------------------------------------------------------------
def nearest_anchors(x_anchor, x_new, k=15):
    """(rows u64 [m, k], scores f32 [m, k], counts u32 [m]) as `search` lays them out: score desc, row asc."""
    s = (x_new.astype(np.float64) @ x_anchor.astype(np.float64).T).astype(np.float32)
    n = x_anchor.shape[0]
    kk = min(k, n)
    rows = np.zeros((len(x_new), k), dtype=np.uint64)
    scores = np.zeros((len(x_new), k), dtype=np.float32)
    for i in range(len(x_new)):
        order = np.lexsort((np.arange(n), -s[i]))[:kk]
        rows[i, :kk], scores[i, :kk] = order, s[i, order]
    return rows, scores, np.full(len(x_new), kk, dtype=np.uint32)


def split(seed):
    """uc.clusters(seed), 480 x 32, cut into 400 anchors and 80 held-out rows (20 per cluster, drawn with
    default_rng(1000 + seed)), both in row order: (x_anchor, labels_anchor, x_new, labels_new)."""
    x, labels = uc.clusters(seed)
    rng = np.random.default_rng(1000 + seed)
    held = np.zeros(len(x), dtype=bool)
    for c in np.unique(labels):
        held[rng.choice(np.nonzero(labels == c)[0], size=HELD_OUT_PER_CLUSTER, replace=False)] = True
    return x[~held], labels[~held], x[held], labels[held]


@functools.lru_cache(maxsize=None)
def holdout(seed):
    """The split with its anchors laid out by the f64 restatement of the layout (200 epochs): (x_anchor, labels_anchor,
    x_new, labels_new, anchors f32 [400, 2], rows, scores, counts of the 15 nearest anchors).  Cached: shared, not to be
    changed."""
    xa, la, xn, ln = split(seed)
    anchors = uc.restated_layout(xa, seed).astype(np.float32)
    return (xa, la, xn, ln, anchors) + nearest_anchors(xa, xn, 15)


def _nearest_layout(anchors, y, k):
    d = ((np.asarray(y, dtype=np.float64)[:, None, :] - np.asarray(anchors, dtype=np.float64)[None, :, :]) ** 2).sum(axis=2)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def kept(rows, anchors, y, k=15):
    """Mean share of each new point's k nearest anchor rows (`rows`, from the search) among its k nearest anchor layout
    points."""
    lo = _nearest_layout(anchors, y, k)
    return float(np.mean([len(set(int(r) for r in rows[i, :k]) & set(lo[i])) / k for i in range(len(y))]))


def purity(labels_anchor, labels_new, anchors, y, k=15):
    """Mean share of each new point's k nearest anchor layout points that carry its label."""
    return float(np.mean(labels_anchor[_nearest_layout(anchors, y, k)] == np.asarray(labels_new)[:, None]))


def random_placement(seed, anchors, m):
    lo, hi = np.asarray(anchors).min(axis=0), np.asarray(anchors).max(axis=0)
    return np.random.default_rng(2000 + seed).uniform(lo, hi, size=(m, 2))


def main():
    print("| seed | synchronous: kept / purity | in place: kept / purity | initial position only | uniform-random placement |")
    print("|---|---|---|---|---|")
    ks, ps = [], []
    for seed in SEEDS:
        xa, la, xn, ln, anchors, rows, scores, counts = holdout(seed)
        q = lambda y: f"{kept(rows, anchors, y):.3f} / {purity(la, ln, anchors, y):.3f}"
        ys = transform(anchors, rows, scores, counts, n_epochs=100, seed=seed)
        yp = transform(anchors, rows, scores, counts, n_epochs=100, seed=seed, in_place=True)
        y0 = transform(anchors, rows, scores, counts, n_epochs=100, epochs=0, seed=seed)
        ks.append(kept(rows, anchors, ys))
        ps.append(purity(la, ln, anchors, ys))
        print(f"| {seed} | {q(ys)} | {q(yp)} | {q(y0)} | {q(random_placement(seed, anchors, len(xn)))} |", flush=True)
        cut = np.concatenate([transform(anchors, rows[:33], scores[:33], counts[:33], n_epochs=100, seed=seed),
                              transform(anchors, rows[33:], scores[33:], counts[33:], id_base=len(anchors) + 33, n_epochs=100, seed=seed)])
        assert cut.tobytes() == ys.tobytes(), "a call split at vertex 33 with a matching id_base must give the same bytes"
    print(f"synchronous kept: min {min(ks):.3f} max {max(ks):.3f} spread {max(ks) - min(ks):.3f}; "
          f"purity: min {min(ps):.3f} max {max(ps):.3f} spread {max(ps) - min(ps):.3f}")


if __name__ == "__main__":
    main()
