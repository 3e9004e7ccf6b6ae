#!/usr/bin/env python3
"""`HipIndex.umap_transform` against the only route there was before it, a full `umap_project`.

  python tools/umap_transform_bench.py [--n 1000000] [--dim 768] [--new 256,4096] [--n-neighbors 15] [--repeats 3] [--out FILE.json]

One index of n Gaussian unit rows, host-timed around the blocking calls:
  project_s     `umap_project` once: the anchors' coordinates, and the time a re-projection of the corpus costs
then per count m of new rows (Gaussian unit rows of another seed), the best of `--repeats`:
  search_ms     `search_batch` of the m rows at k = n_neighbors in blocks of 256: the new rows' nearest anchors
  transform_ms  `cqs_amd.umap.transform` over those lists: the upload of the anchors (8 n bytes), the lists, ONE launch of
                transform_kernel over the default epochs (100), the answer back; transform_epochs_0_ms is the same call
                with `epochs=0`, so the difference is what the epochs cost
  call_ms       `umap_transform`, the two in one call
One JSON line.  No threshold: the reading belongs in DESIGN §3.18a."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--new", type=str, default="256,4096")
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex
    from cqs_amd import umap as hu
    if not torch.cuda.is_available():
        raise SystemExit("umap_transform_bench needs a GPU: nothing here is measured without one")
    say = lambda *what: print(*what, file=sys.stderr, flush=True)                       # progress; the result is the JSON line
    counts_new = [int(s) for s in a.new.split(",") if s]
    flat = make_unit_rows(torch, a.n, a.dim, 0xC950021, torch.device("cuda")).cpu().numpy()
    fresh = make_unit_rows(torch, max(counts_new), a.dim, 0xC950022, torch.device("cuda")).cpu().numpy()
    torch.cuda.empty_cache()
    idx = HipIndex.build_from_flat(None, flat)
    del flat
    t0 = time.perf_counter()
    xy = idx.umap_project(n_neighbors=a.n_neighbors)
    t_project = time.perf_counter() - t0
    say(f"n={a.n}: umap_project {t_project:.2f} s")
    res = {"tool": "umap_transform_bench", "n": a.n, "dim": a.dim, "n_neighbors": a.n_neighbors,
           "device": torch.cuda.get_device_name(0), "project_s": round(t_project, 3), "new": []}

    def best(fn):
        out, t = None, float("inf")
        for _ in range(max(1, a.repeats)):
            t0 = time.perf_counter()
            out = fn()
            t = min(t, time.perf_counter() - t0)
        return out, t * 1e3

    def search(v):
        parts = [idx.search_batch(v[at:at + 256], a.n_neighbors) for at in range(0, len(v), 256)]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))

    for m in counts_new:
        v = fresh[:m]
        (rows, scores, counts), t_search = best(lambda: search(v))
        placed, t_transform = best(lambda: hu.transform(xy, rows, scores, counts))
        _, t_initial = best(lambda: hu.transform(xy, rows, scores, counts, epochs=0))
        whole, t_call = best(lambda: idx.umap_transform(xy, v, n_neighbors=a.n_neighbors))
        say(f"m={m}: search {t_search:.2f} ms, transform {t_transform:.2f} ms ({t_initial:.2f} ms without its epochs), "
            f"umap_transform {t_call:.2f} ms")
        res["new"].append({"m": m, "epochs": 100 if m <= 10000 else 30, "search_ms": round(t_search, 3),
                           "transform_ms": round(t_transform, 3), "transform_epochs_0_ms": round(t_initial, 3),
                           "call_ms": round(t_call, 3),
                           "same_bytes": bool(np.array_equal(placed.view(np.uint32), whole.view(np.uint32))),
                           "finite": bool(np.isfinite(whole).all()), "reprojection_over_call": round(t_project * 1e3 / t_call, 1)})
    idx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
