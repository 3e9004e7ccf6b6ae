#!/usr/bin/env python3
"""Blocking-call latency of the device MMR re-rank beside the search that feeds it.

  python tools/mmr_latency.py [--rows 100000] [--dim 768] [--calls 100] [--warmup 10] [--out FILE.json]

On a seeded index of unit rows: for each pool shape (m = 500, limit = 20) and (m = 1024, limit = 100) the pool is the
real answer of a k = m search; the tool then times, from the same process and the same handle, `calls` blocking
`mmr_rows` calls of that pool and `calls` blocking k = 500 searches (the search that would precede the re-rank, for
scale), alternating the two so that both see the same clocks.  Every call ends in the library's own stream
synchronise, so the host clock around it is the caller's latency.  Prints one JSON line: per shape the median, the
quartiles and the extremes in microseconds.  No threshold: nothing comparable existed before."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(500, 20), (1024, 100)]
LAMBDA = 0.7


def spread(us):
    a = np.sort(np.asarray(us, dtype=np.float64))
    q = lambda f: float(a[min(len(a) - 1, int(f * len(a)))])   # noqa: E731
    return {"median_us": round(float(np.median(a)), 1), "p25_us": round(q(0.25), 1), "p75_us": round(q(0.75), 1),
            "min_us": round(float(a[0]), 1), "max_us": round(float(a[-1]), 1), "calls": len(a)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if a.calls < 50:
        ap.error("--calls must be at least 50 (the figures are medians)")
    from cqs_amd import HipIndex, _lib
    if _lib.load().cqs_hip_device_count() <= 0:
        sys.exit("mmr_latency: no HIP device (a latency is measured on the GPU or not at all)")
    rng = np.random.default_rng(0xC950)
    rows = rng.standard_normal((a.rows, a.dim)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    queries = rng.standard_normal((a.calls + a.warmup, a.dim)).astype(np.float32)
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    idx = HipIndex.build_from_flat(None, rows)
    res = {"tool": "mmr_latency", "rows": a.rows, "dim": a.dim, "lambda": LAMBDA, "shapes": []}
    for m, limit in SHAPES:
        r, s, c = idx.search_batch(queries[0], m)
        assert int(c[0]) == m
        cand, scores = r[0].copy(), s[0].copy()
        t_mmr, t_search = [], []
        picks0 = None
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            idx.search_batch(queries[i], 500)
            t1 = time.perf_counter()
            picks = idx.mmr_rows(cand, scores, limit, LAMBDA)
            t2 = time.perf_counter()
            if picks0 is None:
                picks0 = picks.copy()
            assert np.array_equal(picks, picks0) and len(picks) == limit
            if i >= a.warmup:
                t_search.append((t1 - t0) * 1e6)
                t_mmr.append((t2 - t1) * 1e6)
        res["shapes"].append({"m": m, "limit": limit, "mmr_rows": spread(t_mmr), "search_k500": spread(t_search)})
    idx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
