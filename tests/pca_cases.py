"""The PCA of the stored rows (include/cqs_hip.h, "PCA of the stored rows") restated in numpy: the host steps in f64 as
the header states them (Gram-Schmidt with its breakdown rule, the small eigen-solve, the sign rule), the device's sums in
f32 per slab of 1024 rows and f64 across slabs (the mean pass in f64 throughout) - numpy's own summation order inside a
slab, which is not the device's, so the device is held to 100 times this restatement's own error, not to its bits.  Exact f32 / u32 where the header fixes the
bits: the start matrix, the jitter, the scaling of the initial coordinates.  Also the corpora of the PCA tests and
`global_rho`, the figure of merit of DESIGN.md §3.18b.

Run as a script it prints the tables recorded in §3.18b and the values recorded below."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import umap_cases as uc  # noqa: E402

BLOCK = 8
SLAB = 1024
DEFAULT_PASSES = 16
SEEDS = (1, 2, 3, 4, 5)


# ---- exact-bit rules ----------------------------------------------------------------------------------------------------
def start_matrix(seed, dim):
    """V0 [dim, 8] f32: float(hash(seed, 0, d, 2, j) >> 8) * 2^-23 - 1."""
    d = np.arange(dim, dtype=np.uint32)
    out = np.empty((dim, BLOCK), dtype=np.float32)
    for j in range(BLOCK):
        u = (uc.hash5(seed, 0, d, 2, j) >> np.uint32(8)).astype(np.float32)
        out[:, j] = u * np.float32(1.0 / 8388608.0) - np.float32(1.0)
    return out


def jitter(seed, n):
    """[n, 2] f32: (float(hash(seed, 0, i, 1, c) >> 8) * 2^-24 - 0.5) * 2e-4, each step rounded once."""
    v = np.arange(n, dtype=np.uint32)
    out = np.empty((n, 2), dtype=np.float32)
    for c in (0, 1):
        u = (uc.hash5(seed, 0, v, 1, c) >> np.uint32(8)).astype(np.float32)
        out[:, c] = (u * np.float32(1.0 / 16777216.0) - np.float32(0.5)) * np.float32(2e-4)
    return out


def noisy_scale_coords(proj, seed):
    """proj f32 [n, 1 or 2] -> xy f32 [n, 2], or None where max|proj| is 0 or a projection is not finite."""
    p = np.asarray(proj, dtype=np.float32)
    mag = np.abs(p)
    if p.size == 0 or not np.isfinite(mag).all() or not mag.max() > 0:
        return None
    with np.errstate(over="ignore"):
        scale = np.float32(10.0) / mag.max()
    if not np.isfinite(scale):                                 # a denormal maximum
        return None
    xy = np.zeros((p.shape[0], 2), dtype=np.float32)
    xy[:, :p.shape[1]] = p * scale
    return xy + jitter(seed, p.shape[0])


# ---- the host steps, f64 ----------------------------------------------------------------------------------------------------
def gram_schmidt(a, p):
    """Columns 0 .. p-1 of a [dim, 8] f64 orthonormalised as the header states, the rest zeroed.  -> (q, columns replaced)."""
    a = np.array(a, dtype=np.float64)
    dim = a.shape[0]
    replaced = []

    def project_out(j):
        for _ in range(2):
            for i in range(j):
                a[:, j] -= (a[:, i] @ a[:, j]) * a[:, i]

    for j in range(p):
        before = np.sqrt(a[:, j] @ a[:, j])
        ok = np.isfinite(before) and before > 0
        after = 0.0
        if ok:
            project_out(j)
            after = np.sqrt(a[:, j] @ a[:, j])
            ok = np.isfinite(after) and after > 1e-10 * before
        if not ok:
            replaced.append(j)
            for e in range(dim):
                a[:, j] = 0.0
                a[e, j] = 1.0
                project_out(j)
                after = np.sqrt(a[:, j] @ a[:, j])
                if after * after >= 1.0 / (2.0 * dim):
                    break
        a[:, j] /= after
    a[:, p:] = 0.0
    return a, replaced


def fix_sign(axis):
    axis = np.array(axis, dtype=np.float32)
    at = int(np.argmax(np.abs(axis)))          # the first of equal magnitudes
    return -axis if axis[at] < 0 else axis


def small_eigen(h):
    """Symmetric [p, p] f64 -> (eigenvalues descending, eigenvectors in columns)."""
    lam, w = np.linalg.eigh(h)
    order = np.argsort(-lam, kind="stable")        # equal eigenvalues keep their order (a zero matrix gives the identity)
    return lam[order], w[:, order]


# ---- the method ---------------------------------------------------------------------------------------------------------------
def _slabs(n):
    return [(s, min(n, s + SLAB)) for s in range(0, n, SLAB)]


def moments(x):
    """(x_0, mu - x_0 f64 [dim], total variance f64): the sums of x - x_0 and of its squares in f64."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    xs = x.astype(np.float64) - x[0].astype(np.float64)
    shift_mean = xs.sum(axis=0) / n
    return x[0], shift_mean, (float((xs * xs).sum()) - n * float(shift_mean @ shift_mean)) / (n - 1)


def one_pass(xs, shift_mean, v):
    """Z^T Z V in f64 from the f32 block of v: per slab t = xs V - c, Y = xs^T t, S = sum t in f32; f64 across slabs."""
    v32 = v.astype(np.float32)
    c = (shift_mean @ v32.astype(np.float64)).astype(np.float32)
    y = np.zeros(v.shape)
    s = np.zeros(BLOCK)
    for a, b in _slabs(xs.shape[0]):
        t = xs[a:b] @ v32 - c
        y += (xs[a:b].T @ t).astype(np.float64)
        s += t.sum(axis=0, dtype=np.float32).astype(np.float64)
    return y - np.outer(shift_mean, s), v32


def pca(x, n_components=2, n_passes=0, seed=42):
    """-> (mean f32 [dim], axes f32 [nc, dim], variance f32 [nc], total variance f64, columns replaced in any Gram-Schmidt)."""
    x = np.asarray(x, dtype=np.float32)
    n, dim = x.shape
    p = min(BLOCK, dim)
    passes = n_passes or DEFAULT_PASSES
    x0, shift_mean, total = moments(x)
    xs = x - x0
    v0 = start_matrix(seed, dim).astype(np.float64)
    v0[:, p:] = 0.0
    v, replaced = gram_schmidt(v0, p)
    for _ in range(passes):
        y, _ = one_pass(xs, shift_mean, v)
        v, r = gram_schmidt(y, p)
        replaced += r
    y, v32 = one_pass(xs, shift_mean, v)
    v = v32.astype(np.float64)
    h = v[:, :p].T @ y[:, :p]
    lam, w = small_eigen(0.5 * (h + h.T))
    axes = np.stack([fix_sign((v[:, :p] @ w[:, k]).astype(np.float32)) for k in range(n_components)])
    mean = (x0.astype(np.float64) + shift_mean).astype(np.float32)
    return mean, axes, (lam[:n_components] / (n - 1)).astype(np.float32), total, replaced


def project(x, mean, axes):
    """(x - mean) . axes_k in f64 from the f32 difference, and the bound's mass |x - mean| |a| per row and axis."""
    z = (np.asarray(x, dtype=np.float32) - np.asarray(mean, dtype=np.float32)).astype(np.float64)
    a = np.asarray(axes, dtype=np.float64)
    return z @ a.T, np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1)[:, None] * np.linalg.norm(a, axis=1)[None, :]


# ---- the reference and the error measures -------------------------------------------------------------------------------------
def exact(x):
    """numpy f64: (mean, eigenvalues of the covariance descending, eigenvectors in columns) - `eigh` of the covariance, or
    where there are fewer rows than columns the SVD of the centred rows (the other eigenvalues are 0)."""
    x = np.asarray(x, dtype=np.float64)
    n, dim = x.shape
    mu = x.mean(axis=0)
    z = x - mu
    if n < dim:
        _, s, vt = np.linalg.svd(z, full_matrices=False)
        lam = np.zeros(dim)
        lam[:len(s)] = s * s / (n - 1)
        return mu, lam, vt.T
    lam, vec = np.linalg.eigh(z.T @ z / (n - 1))
    return mu, lam[::-1], vec[:, ::-1]


def gap(lam, k=2):
    """lambda_9 / lambda_k: what 16 passes of an 8-column block converge by (0 where there is no ninth)."""
    return float(lam[BLOCK] / lam[k - 1]) if len(lam) > BLOCK and lam[k - 1] > 0 else 0.0


def subspace_sin(axes, vec, k=2):
    """sin of the largest principal angle between span(axes[:k]) and span(vec[:, :k])."""
    q, _ = np.linalg.qr(np.asarray(axes[:k], dtype=np.float64).T)
    sv = np.linalg.svd(vec[:, :k].T @ q, compute_uv=False)
    return float(np.sqrt(max(0.0, 1.0 - min(1.0, sv.min()) ** 2)))


def captured(x, axes, k=2):
    """The variance captured by span(axes[:k]) (the axes orthonormalised in f64 first: their own f32 rounding is
    orthonormality's to answer for), f64."""
    x = np.asarray(x, dtype=np.float64)
    z = x - x.mean(axis=0)
    q, _ = np.linalg.qr(np.asarray(axes[:k], dtype=np.float64).T)
    return float(((z @ q) ** 2).sum() / (x.shape[0] - 1))


def deficit(x, axes, lam, k=2):
    """Relative captured-variance deficit of the first k axes against the k largest eigenvalues."""
    return float(1.0 - captured(x, axes, k) / lam[:k].sum())


def errors(x, got, k=2):
    """(sin, deficit, largest |variance - lambda| / lambda_1, |mean - mu| max, orthonormality defect) of a pca() answer."""
    mean, axes, var = got[0], got[1], got[2]
    mu, lam, vec = exact(x)
    a = np.asarray(axes, dtype=np.float64)
    return (subspace_sin(axes, vec, k), deficit(x, axes, lam, k), float(np.abs(var[:k].astype(np.float64) - lam[:k]).max() / lam[0]),
            float(np.abs(mean.astype(np.float64) - mu).max()), float(np.abs(a @ a.T - np.eye(len(a))).max()))


# ---- the corpora --------------------------------------------------------------------------------------------------------------
def ring(seed, n_clusters=12, per=40, dim=32, noise=0.25, radii=(3.0, 1.8), offset=2.0):
    """(unit rows f32 [480, 32], labels): clusters whose centres lie on an ellipse around a common mean."""
    rng = np.random.default_rng(1000 + seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, 3)))
    theta = 2.0 * np.pi * np.arange(n_clusters) / n_clusters
    centres = offset * q[:, 0][None, :] + radii[0] * np.cos(theta)[:, None] * q[:, 1][None, :] + radii[1] * np.sin(theta)[:, None] * q[:, 2][None, :]
    labels = np.repeat(np.arange(n_clusters), per)
    x = centres[labels] + noise * rng.standard_normal((n_clusters * per, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), labels


def planted(seed, n, dim, sigmas, tail=0.7, decay=0.95, offset=0.3):
    """Gaussian rows with singular directions of scale sigmas, then tail * decay^i, rotated, plus a constant offset."""
    rng = np.random.default_rng(seed)
    s = np.concatenate([np.asarray(sigmas, dtype=np.float64), tail * decay ** np.arange(dim - len(sigmas))])
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    return ((rng.standard_normal((n, dim)) * s) @ q.T + offset).astype(np.float32)


def isotropic(seed=5, n=600, dim=24):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def identical(n=300, dim=24, seed=6):
    return np.tile(np.random.default_rng(seed).standard_normal((1, dim)).astype(np.float32), (n, 1))


def rank_one(n=300, dim=24, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 1)) * rng.standard_normal((1, dim)) + 0.5).astype(np.float32)


def corpora():
    """name -> rows: the gapped corpora and the isotropic one."""
    return {"ring": ring(1)[0], "clusters": uc.clusters(1)[0], "planted_1000x96": planted(2, 1000, 96, (4.0, 2.0, 1.0)),
            "planted_777x40": planted(3, 777, 40, (3.0, 2.9, 1.0)), "isotropic": isotropic()}


# The restatement's own errors at p = 8, 16 passes, seed 42 (this file run as a script): sin of the top-2 subspace angle,
# relative captured-variance deficit, largest |variance - lambda| / lambda_1.  The device adds in another order, so its bars
# are 100 times these, with floors of 1e-5 (sin, gapped corpora), 1e-9 (deficit) and 1e-6 (variances: an f32 output alone
# rounds by 6e-8).  The isotropic corpus has no gap to converge to: only its deficit is asked for.
RESTATED = {
    "ring": (4.5e-7, 1.3e-13, 1.4e-7),
    "clusters": (6.8e-7, 2.3e-13, 2.2e-7),
    "planted_1000x96": (4.7e-7, 1.9e-13, 3.2e-8),
    "planted_777x40": (4.2e-7, 1.5e-13, 1.8e-7),
    "isotropic": (6.8e-3, 6.6e-6, 8.6e-6),
}
GAP_BAR = 0.25


def bars(name):
    s, d, v = RESTATED[name]
    return max(100.0 * s, 1e-5), max(100.0 * d, 1e-9), max(100.0 * v, 1e-6)


# ---- the figure of merit of the layout ----------------------------------------------------------------------------------------
def _ranks(v):
    r = np.empty(len(v))
    r[np.argsort(v, kind="stable")] = np.arange(len(v))
    return r


def global_rho(x, labels, y):
    """Spearman correlation between the pairwise distances of the cluster centroids in row space and in the layout."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ks = np.unique(labels)
    cx = np.stack([x[labels == k].mean(axis=0) for k in ks])
    cy = np.stack([y[labels == k].mean(axis=0) for k in ks])
    iu = np.triu_indices(len(ks), 1)
    dx = np.linalg.norm(cx[:, None, :] - cx[None, :, :], axis=2)[iu]
    dy = np.linalg.norm(cy[:, None, :] - cy[None, :, :], axis=2)[iu]
    return float(np.corrcoef(_ranks(dx), _ranks(dy))[0, 1])


def pca_start(x, seed):
    """The PCA initial coordinates of the restatement (None: the hashed ones stay)."""
    mean, axes, _, _, _ = pca(x, min(2, x.shape[1]), 0, seed)
    z, _ = project(x, mean, axes)
    return noisy_scale_coords(z.astype(np.float32), seed)


def restated_layout(x, seed, init, n_epochs=200, n_neighbors=15):
    rows, scores, counts = uc.exact_knn(x, n_neighbors - 1)
    off, nbr, w, _, _, w_max = uc.graph(rows, scores, counts)
    y0 = uc.initial_coords(seed, len(x))
    if init == "pca":
        start = pca_start(x, seed)
        y0 = y0 if start is None else start
    return uc.layout_sync(off, nbr, w, w_max, y0, n_epochs, seed)


# The restatement on `ring(seed)`, 200 epochs, PCA init (this file run as a script): global_rho, 15-NN kept, purity.  The
# device's rho may fall short of its seed's by RHO_MARGIN = 0.045.  That number is the bound the feature was specified
# with (the spread of its author's prototype over five seeds, on a ring of their own); it is NOT this table's spread, which
# is 0.958 - 0.885 = 0.073.  What it has to cover here is the layout's sensitivity to rounding: a change of the mean in the
# eighth digit moved single rhos of this table by up to 0.035.
RECORDED_PCA_RHO = (0.885, 0.937, 0.891, 0.958, 0.952)
RECORDED_PCA_KEPT = (0.421, 0.415, 0.420, 0.411, 0.418)
RECORDED_PCA_PURITY = (0.911, 0.889, 0.941, 0.936, 0.904)
RHO_MARGIN = 0.045


def main():
    print("| corpus | lambda_9 / lambda_2 | sin | deficit | variance | mean | orthonormality |")
    print("|---|---|---|---|---|---|---|")
    for name, x in corpora().items():
        e = errors(x, pca(x))
        print(f"| {name} {x.shape[0]} x {x.shape[1]} | {gap(exact(x)[1]):.3f} | {e[0]:.1e} | {e[1]:.1e} | {e[2]:.1e} | {e[3]:.1e} | {e[4]:.1e} |", flush=True)
    for passes in (1, 2, 4):
        x = corpora()["planted_1000x96"]
        print(f"planted_1000x96 at {passes} passes: deficit {deficit(x, pca(x, 2, passes)[1], exact(x)[1]):.3e}")
    print("| seed | random init: rho / kept / purity | PCA init: rho / kept / purity | PCA projection alone: rho |")
    print("|---|---|---|---|")
    for seed in SEEDS:
        x, labels = ring(seed)
        yr, yp = restated_layout(x, seed, "random"), restated_layout(x, seed, "pca")
        print(f"| {seed} | {global_rho(x, labels, yr):.3f} / {uc.preservation(x, yr):.3f} / {uc.purity(labels, yr):.3f} "
              f"| {global_rho(x, labels, yp):.3f} / {uc.preservation(x, yp):.3f} / {uc.purity(labels, yp):.3f} "
              f"| {global_rho(x, labels, pca_start(x, seed)):.3f} |", flush=True)


if __name__ == "__main__":
    main()
