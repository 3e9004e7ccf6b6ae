#!/usr/bin/env python3
"""`cqs_hip_index_knn_graph` over a whole corpus against the two routes it replaces.

  python tools/knn_bench.py [--n 1000000] [--dim 768] [--limit 15] [--rows-per-call 4096] [--sample 200] [--out FILE.json]

One index of `--n` x `--dim` Gaussian unit rows, host-timed around the blocking calls, all three in the same run:
  graph        `HipIndex.knn_graph_rows(limit)` over all rows, in calls of `--rows-per-call` targets
  composition  the same tiles as host searches: `search_batch(rows of the tile, k1)` (the tile's vectors uploaded again, the
               packed keys downloaded and unpacked) and the target dropped on the host, into the same three arrays
  neighbors    `neighbors_rows` for `--sample` evenly spaced targets, extrapolated to n rows
Before anything is timed the first four tiles and the last one are compared byte for byte between graph and composition
(which also warms the scratch and the staging block); afterwards the two full results are compared the same way.  One JSON
line.  No threshold: the reading belongs in DESIGN §3.16."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--limit", type=int, default=15)
    ap.add_argument("--rows-per-call", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a GPU: nothing here is measured without one")
    n, dim = a.n, a.dim
    L = max(1, min(a.limit, 100))
    k1 = min(L + 1, n)
    flat = make_unit_rows(torch, n, dim, 0xC950021, torch.device("cuda")).cpu().numpy()
    torch.cuda.empty_cache()
    idx = HipIndex.build_from_flat(None, flat)

    def compose(lo, hi, rows, scores, counts):
        """Tile [lo, hi) through the host search, the target dropped on the host (vectorised: one stable shift per row)."""
        r, s, c = idx.search_batch(flat[lo:hi], k1)
        valid = np.arange(k1)[None, :] < c[:, None]
        keep = valid & (r != np.arange(lo, hi, dtype=np.uint64)[:, None])
        order = np.argsort(~keep, axis=1, kind="stable")[:, :L]              # the kept slots first, in their order
        kept = np.take_along_axis(keep, order, axis=1)
        rows[lo:hi] = np.where(kept, np.take_along_axis(r, order, axis=1), np.uint64(0))
        scores[lo:hi] = np.where(kept, np.take_along_axis(s, order, axis=1), np.float32(0))
        counts[lo:hi] = kept.sum(axis=1)

    def same(x, y, lo, hi):
        return all(np.array_equal(p[lo:hi].view(np.uint8), q[lo:hi].view(np.uint8)) for p, q in zip(x, y))

    comp = (np.zeros((n, L), np.uint64), np.zeros((n, L), np.float32), np.zeros((n,), np.uint32))
    tiles = [(lo, min(lo + TILE, n)) for lo in range(0, n, TILE)]
    checked = 0
    for lo, hi in tiles[:4] + tiles[-1:]:
        got = idx.knn_graph_rows(L, first=lo, count=hi - lo)
        compose(lo, hi, *comp)
        if not all(np.array_equal(g.view(np.uint8), c[lo:hi].view(np.uint8)) for g, c in zip(got, comp)):
            raise SystemExit(f"graph and composition differ in tile [{lo}, {hi})")
        checked += 1
    idx.knn_graph_rows(L, first=0, count=min(n, a.rows_per_call), rows_per_call=a.rows_per_call)   # the staging block at its full size
    t0 = time.perf_counter()
    graph = idx.knn_graph_rows(L, rows_per_call=a.rows_per_call)
    t_graph = time.perf_counter() - t0
    t0 = time.perf_counter()
    for lo, hi in tiles:
        compose(lo, hi, *comp)
    t_comp = time.perf_counter() - t0
    if not same(graph, comp, 0, n):
        raise SystemExit("graph and composition differ over the whole corpus")
    targets = np.linspace(0, n - 1, num=min(a.sample, n), dtype=np.int64)
    idx.neighbors_rows(int(targets[0]), L)
    t0 = time.perf_counter()
    for t in targets:
        idx.neighbors_rows(int(t), L)
    t_nb = (time.perf_counter() - t0) / len(targets)
    idx.close()
    res = {"tool": "knn_bench", "n": n, "dim": dim, "limit": L, "k1": k1, "rows_per_call": a.rows_per_call, "tiles": len(tiles),
           "tiles_checked_before_timing": checked, "whole_graph_equal": True,
           "graph_s": round(t_graph, 3), "graph_rows_per_s": round(n / t_graph),
           "composition_s": round(t_comp, 3), "composition_rows_per_s": round(n / t_comp),
           "neighbors_ms_per_row": round(t_nb * 1e3, 4), "neighbors_sample": int(len(targets)), "neighbors_extrapolated_s": round(t_nb * n, 1),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
