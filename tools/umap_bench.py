#!/usr/bin/env python3
"""`HipIndex.umap_project`'s two halves, timed apart, at the reference's corpus size and at 1M rows.

  python tools/umap_bench.py [--sizes 17523,1000000] [--dim 768] [--n-neighbors 15] [--cpu-epochs 10] [--out FILE.json]

Per size, one index of Gaussian unit rows, host-timed around the blocking calls:
  graph_s    `knn_graph_rows(n_neighbors - 1)` over all rows
  create_s   `HipLayout(...)`: the argument plan and the adjacency transpose on the host, the upload, the weights on the device
  epoch_ms   `run()` to the end over the default epochs (500 up to 10 000 rows, 200 above), per epoch;  total_s = all three
At the first size the numpy restatement of the same rule (tests/umap_cases.py, f64, one thread) is timed on the CPU: its
graph in full, `--cpu-epochs` epochs extrapolated to the same count.  If `import umap` works, umap-learn's `fit_transform`
(n_neighbors, min_dist 0.1, cosine, random_state 42) on the same rows is a second line; nothing is installed for it.
One JSON line.  No threshold: the reading belongs in DESIGN §3.18."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="17523,1000000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--cpu-epochs", type=int, default=10)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import umap_cases as uc
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex
    from cqs_amd.umap import HipLayout
    if not torch.cuda.is_available():
        raise SystemExit("umap_bench needs a GPU: nothing here is measured without one")
    sizes = [int(s) for s in a.sizes.split(",") if s]
    say = lambda *what: print(*what, file=sys.stderr, flush=True)                       # progress; the result is the JSON line
    res = {"tool": "umap_bench", "dim": a.dim, "n_neighbors": a.n_neighbors, "device": torch.cuda.get_device_name(0), "sizes": []}
    for at, n in enumerate(sizes):
        flat = make_unit_rows(torch, n, a.dim, 0xC950021, torch.device("cuda")).cpu().numpy()
        torch.cuda.empty_cache()
        idx = HipIndex.build_from_flat(None, flat)
        idx.knn_graph_rows(a.n_neighbors - 1, first=0, count=min(n, 4096))              # scratch and staging at full size
        t0 = time.perf_counter()
        rows, scores, counts = idx.knn_graph_rows(a.n_neighbors - 1)
        t_graph = time.perf_counter() - t0
        idx.close()
        say(f"n={n}: graph {t_graph:.2f} s")
        t0 = time.perf_counter()
        lay = HipLayout(rows, scores, counts)
        t_create = time.perf_counter() - t0
        epochs, edges = lay.n_epochs, lay.edges
        graph = lay.graph()
        start = lay.coords()
        t0 = time.perf_counter()
        lay.run()
        t_run = time.perf_counter() - t0
        xy = lay.coords()
        lay.close()
        say(f"n={n}: create {t_create:.2f} s, {epochs} epochs {t_run:.2f} s")
        row = {"n": n, "edges": edges, "epochs": epochs, "graph_s": round(t_graph, 3), "create_s": round(t_create, 3),
               "epoch_ms": round(t_run / epochs * 1e3, 4), "run_s": round(t_run, 3), "total_s": round(t_graph + t_create + t_run, 3),
               "finite": bool(np.isfinite(xy).all()), "max_abs_coord": round(float(np.abs(xy).max()), 2)}
        if at == 0:
            t0 = time.perf_counter()
            uc.graph(rows, scores, counts)
            row["cpu_numpy_graph_s"] = round(time.perf_counter() - t0, 3)
            say(f"n={n}: numpy graph {row['cpu_numpy_graph_s']} s")
            off, nbr, w, _, _, w_max = graph
            y = start.astype(np.float64)
            t0 = time.perf_counter()
            for e in range(1, a.cpu_epochs + 1):
                y, _ = uc.epoch_sync(off, nbr, w, w_max, y, e, epochs, 42)
            t_cpu = (time.perf_counter() - t0) / max(1, a.cpu_epochs)
            row["cpu_numpy_epoch_ms"] = round(t_cpu * 1e3, 2)
            row["cpu_numpy_total_s_extrapolated"] = round(row["cpu_numpy_graph_s"] + t_cpu * epochs, 1)
            try:
                import umap                                                              # noqa: F401  (only if it is there)
                t0 = time.perf_counter()
                umap.UMAP(n_neighbors=a.n_neighbors, min_dist=0.1, metric="cosine", random_state=42).fit_transform(flat)
                row["umap_learn_s"] = round(time.perf_counter() - t0, 2)
            except ImportError:
                row["umap_learn_s"] = None
        res["sizes"].append(row)
        del flat
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
