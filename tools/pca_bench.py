"""PCA of the stored rows, measured: ms per pass and its fraction of 8 TB/s, the whole of `pca` +
`pca_project`, numpy's `eigh` of the covariance on the CPU as the comparison line, and `umap_project` with both inits.

    python tools/pca_bench.py [--rows 17523 1000000] [--dim 768] [--umap-rows 17523] [--repeat 3]

Prints one JSON line per corpus size.  Nothing here gates: the numbers go into §3.18b."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cqs_amd import HipIndex  # noqa: E402

HBM_PEAK = 8.0e12


def corpus(n, dim, seed=1, clusters=64):
    """Unit rows around `clusters` centres, generated in blocks."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, dim)).astype(np.float32) * 2.0
    x = np.empty((n, dim), dtype=np.float32)
    for at in range(0, n, 65536):
        m = min(65536, n - at)
        b = centres[rng.integers(0, clusters, m)] + rng.standard_normal((m, dim), dtype=np.float32)
        x[at:at + m] = b / np.linalg.norm(b, axis=1, keepdims=True)
    return x


def best(fn, repeat):
    times = []
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[17523, 1000000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--umap-rows", type=int, default=17523, help="largest corpus umap_project is timed on")
    ap.add_argument("--cpu-rows", type=int, default=1000000, help="largest corpus numpy's eigh line is computed on")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    for n in a.rows:
        x = corpus(n, a.dim)
        idx = HipIndex.build_from_flat(None, x)
        idx.pca(2, 1)                                                         # warm: code objects, allocator
        t1, _ = best(lambda: idx.pca(2, 1), a.repeat)                         # mean pass + 2 passes
        t16, got = best(lambda: idx.pca(2, 16), a.repeat)                     # mean pass + 17 passes
        per_pass = (t16 - t1) / 15.0
        tp, z = best(lambda: idx.pca_project(got[0], got[1]), a.repeat)
        line = {"rows": n, "dim": a.dim, "pca_ms": round(t16 * 1e3, 3), "pass_ms": round(per_pass * 1e3, 4),
                "pass_fraction_of_8TBps": round(n * a.dim * 4 / per_pass / HBM_PEAK, 4), "project_ms": round(tp * 1e3, 3),
                "pca_plus_project_ms": round((t16 + tp) * 1e3, 3),
                "explained_variance_ratio": [round(float(v) / got[3], 5) for v in got[2]]}
        if n <= a.cpu_rows:
            t = time.perf_counter()
            mu = x.mean(axis=0, dtype=np.float64)
            cov = np.zeros((a.dim, a.dim))
            for at in range(0, n, 65536):
                zb = x[at:at + 65536].astype(np.float64) - mu
                cov += zb.T @ zb
            lam, vec = np.linalg.eigh(cov / (n - 1))
            line["numpy_eigh_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            q, _ = np.linalg.qr(got[1].astype(np.float64).T)
            sv = np.linalg.svd(vec[:, ::-1][:, :2].T @ q, compute_uv=False)
            line["sin_top2_vs_numpy"] = float(np.sqrt(max(0.0, 1.0 - min(1.0, sv.min()) ** 2)))
            line["variance_rel_err_vs_numpy"] = float(np.abs(got[2].astype(np.float64) - lam[::-1][:2]).max() / lam[-1])
        if n <= a.umap_rows:
            idx.umap_project(15, 10, 42)                                      # warm: the graph's and the layout's code objects
            for init in ("random", "pca"):
                t, _ = best(lambda: idx.umap_project(15, None, 42, init=init), a.repeat)
                line[f"umap_project_{init}_ms"] = round(t * 1e3, 1)
        idx.close()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
