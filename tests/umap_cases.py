"""The UMAP layout's rules (include/cqs_hip.h, "UMAP layout of a kNN graph") restated in numpy, f64 where the header says
f32 arithmetic may differ and exact f32 / u32 where it fixes the bits (distances, rho, the active rule, the hash, the draws,
the initial coordinates, alpha).  Also the in-place sequential variant the header departs from, the case generators of the
layout's tests, and the two quality measures (15-NN preservation, same-cluster purity).

Run as a script it repeats the prototype of DESIGN.md §3.18 - synchronous rule, in-place rule and a random layout on the
four-cluster corpus over SEEDS - and prints the table recorded there."""
import numpy as np

A_DEFAULT = np.float32(1.5769434603)
B_DEFAULT = np.float32(0.8950608779)
NEIGHBORS_MAX = 100

# The prototype as recorded in DESIGN.md §3.18 (this file run as a script): the synchronous restatement's 15-NN
# preservation over SEEDS, 200 epochs.  SPREAD = max - min; the device's quality test allows three times it.
SEEDS = (1, 2, 3, 4, 5)
RECORDED_SYNC_PRESERVATION = (0.290, 0.293, 0.299, 0.290, 0.284)
SPREAD = 0.015


# ---- exact-bit rules ----------------------------------------------------------------------------------------------------
def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def hash5(seed, epoch, vertex, slot, draw):
    """hash(seed, epoch, vertex, slot, draw) of the header; the last four broadcast as u32 arrays."""
    seed = int(seed) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        h = fmix32(np.uint32((seed & 0xFFFFFFFF) ^ 0x9E3779B9))
        h = fmix32(h ^ np.uint32(seed >> 32))
        h = fmix32(h ^ np.asarray(epoch, dtype=np.uint32))
        h = fmix32(h ^ np.asarray(vertex, dtype=np.uint32))
        h = fmix32(h ^ np.asarray(slot, dtype=np.uint32))
        h = fmix32(h ^ np.asarray(draw, dtype=np.uint32))
    return h


def draw_vertex(h, n):
    return ((np.asarray(h, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.uint32)


def initial_coords(seed, n):
    """[n, 2] f32: uniform in [-10, 10) from the hash at epoch 0, slot 0, draw = the coordinate; the origin for n < 2."""
    if n < 2:
        return np.zeros((n, 2), dtype=np.float32)
    v = np.arange(n, dtype=np.uint32)
    out = np.empty((n, 2), dtype=np.float32)
    for c in (0, 1):
        u = (hash5(seed, 0, v, 0, c) >> np.uint32(8)).astype(np.float32)
        out[:, c] = u * np.float32(20.0 / 16777216.0) - np.float32(10.0)
    return out


def active(e, p):
    """f32: floorf(e * p) != floorf((e - 1) * p), each product rounded once."""
    p = np.asarray(p, dtype=np.float32)
    return np.floor(np.float32(e) * p) != np.floor(np.float32(e - 1) * p)


def alpha_of(lr, e, E):
    done = np.float32(e - 1) / np.float32(E)
    return np.float32(lr) * (np.float32(1.0) - done)


def distances(scores):
    """d = max(0, 1 - score) in f32."""
    d = np.float32(1.0) - np.asarray(scores, dtype=np.float32)
    return np.where(d > 0, d, np.float32(0.0)).astype(np.float32)


# ---- the adjacency and the fuzzy simplicial set ---------------------------------------------------------------------------
def adjacency(rows, counts):
    """(offsets u64 [n + 1], nbrs u32 [edges]): i's forward list in list order, then the vertices that list i and are not in
    i's list, ascending.  Written from sets and sorted lists, not as the library's counting sort."""
    n = len(counts)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n < 2:
        return off, np.zeros(0, dtype=np.uint32)
    fwd = [[int(x) for x in rows[i, :int(counts[i])]] for i in range(n)]
    listed_by = [[] for _ in range(n)]
    for j in range(n):
        for t in fwd[j]:
            listed_by[t].append(j)
    out = []
    for i in range(n):
        mine = set(fwd[i])
        entries = fwd[i] + sorted(j for j in listed_by[i] if j not in mine)
        off[i + 1] = off[i] + np.uint64(len(entries))
        out.extend(entries)
    return off, np.asarray(out, dtype=np.uint32)


def smooth_knn(d):
    """(rho f32, sigma f64) of one vertex's f32 distances `d` (its forward list), the bisection in f64."""
    c = len(d)
    if c == 0:
        return np.float32(0.0), 0.0
    pos = d[d > 0]
    rho = pos.min() if len(pos) else np.float32(0.0)
    x = d.astype(np.float64) - float(rho)
    target = np.log2(c + 1.0)
    lo, hi, mid = 0.0, np.inf, 1.0
    for _ in range(64):
        with np.errstate(over="ignore", under="ignore"):
            psum = float(np.where(x > 0, np.exp(-np.where(x > 0, x, 0.0) / mid), 1.0).sum())
        if abs(psum - target) < 1e-5:
            break
        if psum > target:
            hi = mid
            mid = (lo + hi) / 2.0
        else:
            lo = mid
            mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
    return np.float32(rho), max(mid, 1e-3 * float(d.astype(np.float64).mean()))


def forward_weights(d, rho, sigma):
    x = d.astype(np.float64) - float(rho)
    if sigma == 0.0:
        return np.ones(len(d))
    with np.errstate(under="ignore"):
        return np.where(x <= 0, 1.0, np.exp(-np.where(x > 0, x, 0.0) / sigma))


def graph(rows, scores, counts):
    """The header's graph in f64: (offsets, nbrs, weights f64, rho f32, sigma f64, w_max f64)."""
    rows, counts = np.asarray(rows), np.asarray(counts)
    n = len(counts)
    off, nbr = adjacency(rows, counts)
    d = distances(scores)
    rho = np.zeros(n, dtype=np.float32)
    sigma = np.zeros(n, dtype=np.float64)
    fw = []
    for i in range(n):
        di = d[i, :int(counts[i])] if n else d[:0]
        rho[i], sigma[i] = smooth_knn(di)
        fw.append({int(rows[i, s]): w for s, w in enumerate(forward_weights(di, rho[i], sigma[i]))})
    w = np.zeros(len(nbr), dtype=np.float64)
    for i in range(n if n >= 2 else 0):
        for t in range(int(off[i]), int(off[i + 1])):
            j = int(nbr[t])
            a, b = fw[i].get(j, 0.0), fw[j].get(i, 0.0)
            w[t] = a + b - a * b
    return off, nbr, w, rho, sigma, (w.max() if len(w) else 0.0)


# ---- the epochs -----------------------------------------------------------------------------------------------------------
def _coeffs(a, b, repulsion, d2):
    with np.errstate(divide="ignore", invalid="ignore"):
        pw = np.power(d2, b)
        ca = -2.0 * a * b * np.power(d2, b - 1.0) / (a * pw + 1.0)
        cr = 2.0 * repulsion * b / ((0.001 + d2) * (a * pw + 1.0))
    return ca, cr


def epoch_sync(off, nbr, w, w_max, y, e, E, seed, a=A_DEFAULT, b=B_DEFAULT, lr=1.0, repulsion=1.0, negative_samples=5):
    """One synchronous epoch in f64 from coordinates `y` [n, 2].  `w` / `w_max` are taken as f32 (the device's, or the
    restatement's rounded) so the active flags are the device's.  Returns (y_new f64, the per-vertex, per-coordinate sum of
    |terms| f64 [n, 2])."""
    n = len(off) - 1
    y = np.asarray(y, dtype=np.float64)
    a, b, repulsion = float(np.float32(a)), float(np.float32(b)), float(np.float32(repulsion))
    total, mass = np.zeros((n, 2)), np.zeros((n, 2))
    if len(nbr):
        deg = np.diff(off.astype(np.int64))
        vert = np.repeat(np.arange(n, dtype=np.int64), deg)
        slot = np.arange(len(nbr), dtype=np.int64) - off[:-1].astype(np.int64)[vert]
        p = np.asarray(w, dtype=np.float32) / np.float32(w_max)
        act = active(e, p)
        vi, sl, vj = vert[act], slot[act], nbr[act].astype(np.int64)
        dy = y[vi] - y[vj]
        d2 = (dy * dy).sum(axis=1)
        ca, _ = _coeffs(a, b, repulsion, d2)
        term = np.where((d2 > 0)[:, None], 2.0 * np.clip(np.where(d2 > 0, ca, 0.0)[:, None] * dy, -4.0, 4.0), 0.0)
        np.add.at(total, vi, term)
        np.add.at(mass, vi, np.abs(term))
        for k in range(int(negative_samples)):
            q = draw_vertex(hash5(seed, e, vi.astype(np.uint32), sl.astype(np.uint32), k), n).astype(np.int64)
            dy = y[vi] - y[q]
            d2 = (dy * dy).sum(axis=1)
            _, cr = _coeffs(a, b, repulsion, d2)
            ok = (d2 > 0) & (q != vi)
            term = np.where(ok[:, None], np.clip(np.where(ok, cr, 0.0)[:, None] * dy, -4.0, 4.0), 0.0)
            np.add.at(total, vi, term)
            np.add.at(mass, vi, np.abs(term))
    return y + float(alpha_of(lr, e, E)) * total, mass


def layout_sync(off, nbr, w, w_max, y0, E, seed, epochs=None, **kw):
    y = np.asarray(y0, dtype=np.float64)
    w32, wm32 = np.asarray(w, dtype=np.float32), np.float32(w_max)
    for e in range(1, (E if epochs is None else epochs) + 1):
        y, _ = epoch_sync(off, nbr, w32, wm32, y, e, E, seed, **kw)
    return y


def layout_in_place(off, nbr, w, w_max, y0, E, seed, a=A_DEFAULT, b=B_DEFAULT, lr=1.0, repulsion=1.0, negative_samples=5):
    """umap-learn's rule, which the header departs from: entry by entry in adjacency order, each active entry moves both of
    its ends at once and its draws move the vertex; same active flags, same draws."""
    n = len(off) - 1
    y = np.asarray(y0, dtype=np.float64).copy()
    a, b, repulsion = float(np.float32(a)), float(np.float32(b)), float(np.float32(repulsion))
    p = np.asarray(w, dtype=np.float32) / np.float32(w_max)
    deg = np.diff(off.astype(np.int64))
    vert = np.repeat(np.arange(n, dtype=np.int64), deg)
    slot = np.arange(len(nbr), dtype=np.int64) - off[:-1].astype(np.int64)[vert]
    for e in range(1, E + 1):
        alpha = float(alpha_of(lr, e, E))
        idx = np.nonzero(active(e, p))[0]
        draws = np.stack([draw_vertex(hash5(seed, e, vert[idx].astype(np.uint32), slot[idx].astype(np.uint32), k), n)
                          for k in range(int(negative_samples))], axis=1) if len(idx) else np.zeros((0, 0), np.uint32)
        for r, t in enumerate(idx):
            i, j = int(vert[t]), int(nbr[t])
            dy = y[i] - y[j]
            d2 = float(dy @ dy)
            if d2 > 0:
                ca = -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0)
                g = np.clip(ca * dy, -4.0, 4.0)
                y[i] += alpha * g
                y[j] -= alpha * g
            for q in draws[r]:
                q = int(q)
                if q == i:
                    continue
                dy = y[i] - y[q]
                d2 = float(dy @ dy)
                if d2 > 0:
                    cr = 2.0 * repulsion * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                    y[i] += alpha * np.clip(cr * dy, -4.0, 4.0)
    return y


# ---- case generators ------------------------------------------------------------------------------------------------------
def clusters(seed, n_clusters=4, per=120, dim=32, noise=1.0, centre_norm=4.0):
    """(unit rows f32 [n_clusters * per, dim], labels): Gaussian clusters around centres of norm `centre_norm`."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, dim))
    centres *= centre_norm / np.linalg.norm(centres, axis=1, keepdims=True)
    labels = np.repeat(np.arange(n_clusters), per)
    x = centres[labels] + noise * rng.standard_normal((n_clusters * per, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), labels


def exact_knn(x, limit):
    """(rows u64 [n, limit], scores f32 [n, limit], counts u32 [n]) as cqs_hip_index_knn_graph lays them out: score desc,
    row asc, the target excluded."""
    n = x.shape[0]
    s = (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    np.fill_diagonal(s, -np.inf)
    k = min(limit, n - 1)
    rows = np.zeros((n, limit), dtype=np.uint64)
    scores = np.zeros((n, limit), dtype=np.float32)
    for i in range(n):
        order = np.lexsort((np.arange(n), -s[i]))[:k]
        rows[i, :k], scores[i, :k] = order, s[i, order]
    return rows, scores, np.full(n, k, dtype=np.uint32)


def hub_graph(n_spokes=500, stride=1):
    """Vertex 0 is listed by every other vertex and lists none of them (count 0); spoke i also lists nothing else."""
    n = n_spokes + 1
    rows = np.zeros((n, stride), dtype=np.uint64)
    scores = np.zeros((n, stride), dtype=np.float32)
    counts = np.ones(n, dtype=np.uint32)
    counts[0] = 0
    scores[1:, 0] = np.linspace(0.2, 0.9, n_spokes, dtype=np.float32)
    return rows, scores, counts


def ragged_graph(seed, n, stride, dup_every=0, zero_vertex=None, empty_vertex=None):
    """A random graph of ragged counts.  `dup_every`: every such slot has score 1.0 (d = 0: a repeated row);
    `zero_vertex`: all of its neighbours at d = 0; `empty_vertex`: count 0."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, stride), dtype=np.uint64)
    scores = np.zeros((n, stride), dtype=np.float32)
    counts = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        c = int(rng.integers(0 if n > 2 else 1, min(stride, n - 1) + 1))
        if i == empty_vertex:
            c = 0
        others = np.delete(np.arange(n), i)
        pick = rng.choice(others, size=c, replace=False)
        sc = np.sort(rng.uniform(-0.2, 0.999, size=c).astype(np.float32))[::-1]
        if dup_every:
            sc[::dup_every] = 1.0
            sc = np.sort(sc)[::-1]
        if i == zero_vertex:
            sc[:] = 1.0
        rows[i, :c], scores[i, :c], counts[i] = pick, sc, c
    return rows, scores, counts


# ---- quality --------------------------------------------------------------------------------------------------------------
def _knn_sets(dist, k):
    d = dist.copy()
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def preservation(x, y, k=15):
    """Mean share of each point's k nearest rows (cosine) that are among its k nearest layout points."""
    hi = _knn_sets(1.0 - x.astype(np.float64) @ x.astype(np.float64).T, k)
    y = np.asarray(y, dtype=np.float64)
    lo = _knn_sets(((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2), k)
    return float(np.mean([len(set(hi[i]) & set(lo[i])) / k for i in range(len(x))]))


def purity(labels, y, k=15):
    """Mean share of each point's k nearest layout points that carry its label."""
    y = np.asarray(y, dtype=np.float64)
    lo = _knn_sets(((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2), k)
    return float(np.mean(labels[lo] == labels[:, None]))


def restated_layout(x, seed, n_epochs=200, n_neighbors=15):
    rows, scores, counts = exact_knn(x, n_neighbors - 1)
    off, nbr, w, _, _, w_max = graph(rows, scores, counts)
    return layout_sync(off, nbr, w, w_max, initial_coords(seed, len(x)), n_epochs, seed)


def main():
    print("| seed | synchronous: 15-NN kept / purity | in place: kept / purity | random: kept / purity |")
    print("|---|---|---|---|")
    kept = []
    for seed in SEEDS:
        x, labels = clusters(seed)
        rows, scores, counts = exact_knn(x, 14)
        off, nbr, w, _, _, w_max = graph(rows, scores, counts)
        y0 = initial_coords(seed, len(x))
        ys = layout_sync(off, nbr, w, w_max, y0, 200, seed)
        yp = layout_in_place(off, nbr, w, w_max, y0, 200, seed)
        kept.append(preservation(x, ys))
        print(f"| {seed} | {kept[-1]:.3f} / {purity(labels, ys):.3f} | {preservation(x, yp):.3f} / {purity(labels, yp):.3f} "
              f"| {preservation(x, y0):.3f} / {purity(labels, y0):.3f} |", flush=True)
    print(f"synchronous 15-NN kept: min {min(kept):.3f} max {max(kept):.3f} spread {max(kept) - min(kept):.3f}")


if __name__ == "__main__":
    main()
