#!/usr/bin/env python3
"""`cqs_hip_index_remove` against the only alternative, a rebuild from host memory.

  python tools/remove_bench.py [--rows 1000000] [--dim 768] [--remove 1000] [--reps 10] [--rebuild-reps 5] [--out FILE.json]

Per configuration (the f32 corpus alone; the bf16 and int8 shadow copies beside it), host-timed around the blocking calls:
  scattered  remove of `--remove` seeded random rows of the whole corpus
  block      remove of one contiguous block of `--remove` rows starting at row 1000
  rebuild    `HipIndex.build_from_flat` of the surviving rows from host memory (no store read: this flatters the rebuild)
After every timed removal the index is extended by as many rows again (untimed), so every repeat runs at `--rows` rows.
One untimed warm-up per shape; the median, the minimum and the maximum of the repeats are reported.  `payload_bytes` is
what an ideal in-place move would read once and write once (rows above the first removed row, every copy the handle
holds); `payload_tbps` = 2 x payload_bytes / median time, `share_of_hbm` that over the 8 TB/s peak.  The compaction itself
moves every byte twice (through the bounce buffer), so its own traffic is 2 x the payload's."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBPS = 8.0


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--remove", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rebuild-reps", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex
    if not torch.cuda.is_available():
        raise SystemExit("remove_bench needs a GPU: nothing here is measured without one")
    n, dim, m = a.rows, a.dim, a.remove
    flat = make_unit_rows(torch, n, dim, 0xC950001, torch.device("cuda")).cpu().numpy()
    refill = flat[:m].copy()
    rng = np.random.default_rng(0xC950003)
    shapes = {"scattered": np.sort(rng.choice(n, size=m, replace=False)).astype(np.uint64),
              "block": np.arange(1000, 1000 + m, dtype=np.uint64)}
    res = {"tool": "remove_bench", "rows": n, "dim": dim, "removed": m, "configs": {}}
    for cfg, env in (("f32", "0"), ("f32_bf16_i8", "1")):
        os.environ["CQS_HIP_SCAN_BF16"] = env
        os.environ["CQS_HIP_SCAN_I8"] = env
        idx = HipIndex.build_from_flat(None, flat)
        copies = {"bf16_bytes": idx.bf16_stats()[0], "i8_bytes": idx.i8_stats()[0]}
        row_bytes = dim * 4 + (dim * 2 if copies["bf16_bytes"] else 0) + (dim + 4 if copies["i8_bytes"] else 0)
        out = dict(copies)
        for name, rows in shapes.items():
            ms = []
            for rep in range(a.reps + 1):                     # the first one warms the kernels and the allocator
                t0 = time.perf_counter()
                removed = idx.remove_rows(rows)
                t1 = time.perf_counter()
                assert removed == m and len(idx) == n - m
                idx.extend(None, refill)
                if rep:
                    ms.append((t1 - t0) * 1e3)
            payload = (n - m - int(rows[0])) * row_bytes
            s = spread(ms)
            s["payload_bytes"] = payload
            s["payload_tbps"] = round(2 * payload / (s["median_ms"] * 1e-3) / 1e12, 3)
            s["share_of_hbm"] = round(s["payload_tbps"] / HBM_PEAK_TBPS, 3)
            out[name] = s
            print(cfg, name, json.dumps(s), flush=True)
        idx.close()
        kept = np.delete(flat, shapes["scattered"].astype(np.int64), axis=0)
        ms = []
        for rep in range(a.rebuild_reps + 1):
            t0 = time.perf_counter()
            f = HipIndex.build_from_flat(None, kept)
            t1 = time.perf_counter()
            f.close()
            if rep:
                ms.append((t1 - t0) * 1e3)
        out["rebuild"] = spread(ms)
        print(cfg, "rebuild", json.dumps(out["rebuild"]), flush=True)
        del kept
        res["configs"][cfg] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
