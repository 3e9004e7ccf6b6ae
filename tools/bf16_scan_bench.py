"""bf16 shadow scan vs the f32 scan, host API, one process.

For each corpus (unit rows, 768-d; BASELINE configs[1] = 1M and configs[4] = 10M shapes) two owned handles over the same
rows: `f32` (as today) and `bf16` (cqs_hip_index_set_bf16_scan on).  Every shape is warmed up, then the two handles are
timed in alternating rounds (host clock around `cqs_hip_index_search`, which ends in a stream synchronise) and the median
per round is kept.  Shapes: b = 1 at k = 20 and k = 500 (the combining-queue path), b = 2 / 4 / 8 at k = 20.  Every answer
of the bf16 handle is compared byte for byte with the f32 handle's.  Prints one JSON line.

usage: python tools/bf16_scan_bench.py [--sizes 1m,10m] [--rounds 7] [--queries 32]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cqs_amd import HipIndex  # noqa: E402

SIZES = {"1m": 1_000_000, "10m": 10_000_000}
SHAPES = [(1, 20), (1, 500), (2, 20), (4, 20), (8, 20)]   # (queries per call, k)
HBM_PEAK_TBS = 8.0


def unit_rows_on_device(n, dim, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    d = torch.empty((n, dim), device="cuda", dtype=torch.float32)
    for lo in range(0, n, 1 << 18):
        hi = min(n, lo + (1 << 18))
        x = torch.randn((hi - lo, dim), generator=g, device="cuda"); x /= x.norm(dim=1, keepdim=True); d[lo:hi] = x
    return d


def run_calls(idx, qs, b, k):
    """One pass over the query set in calls of b queries; returns (seconds per query, answers)."""
    out = []
    t0 = time.perf_counter()
    for i in range(0, len(qs) - b + 1, b):
        out.append(idx.search_batch(qs[i:i + b], k))
    dt = time.perf_counter() - t0
    return dt / (len(out) * b), out


def same(x, y):
    for (ra, sa, ca), (rb, sb, cb) in zip(x, y):
        if not np.array_equal(ca, cb):
            return False
        for i in range(len(ca)):
            c = int(ca[i])
            if not (np.array_equal(ra[i, :c], rb[i, :c]) and np.array_equal(sa[i, :c].view(np.uint32), sb[i, :c].view(np.uint32))):
                return False
    return True


def bench_size(name, n, dim, rounds, nq):
    d_rows = unit_rows_on_device(n, dim, 20260 + n % 997)
    g = torch.Generator(device="cuda"); g.manual_seed(7 + n % 991)
    qs = torch.randn((nq, dim), generator=g, device="cuda"); qs /= qs.norm(dim=1, keepdim=True)
    qs = qs.cpu().numpy()
    f32 = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=False)
    bf = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=False)
    del d_rows
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    bf.set_bf16_scan(True)
    enable_s = time.perf_counter() - t0
    shadow_bytes = bf.bf16_stats()[0]
    res = {"rows": n, "dim": dim, "shadow_bytes": shadow_bytes, "enable_s": round(enable_s, 3), "shapes": {}}
    for b, k in SHAPES:
        for idx in (f32, bf):                              # warm-up of this shape on both handles
            run_calls(idx, qs, b, k)
        _, c0, f0 = bf.bf16_stats()
        tf, tb, equal = [], [], True
        for _ in range(rounds):                            # alternate the two handles, same process
            sf, af = run_calls(f32, qs, b, k)
            sb, ab = run_calls(bf, qs, b, k)
            tf.append(sf); tb.append(sb)
            equal = equal and same(af, ab)
        _, c1, f1 = bf.bf16_stats()
        mf, mb = statistics.median(tf), statistics.median(tb)
        res["shapes"][f"b{b}_k{k}"] = {
            "f32_ms_per_query": round(mf * 1e3, 4), "bf16_ms_per_query": round(mb * 1e3, 4),
            "ratio": round(mb / mf, 3), "certified_fraction": round((c1 - c0) / max(1, (c1 - c0) + (f1 - f0)), 4),
            "fallbacks": f1 - f0, "byte_equal": bool(equal),
            "f32_spread_ms": [round(min(tf) * 1e3, 4), round(max(tf) * 1e3, 4)],
            "bf16_spread_ms": [round(min(tb) * 1e3, 4), round(max(tb) * 1e3, 4)]}
    f32.close(); bf.close()
    torch.cuda.empty_cache()
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1m,10m")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--queries", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bf16_scan_bench needs the GPU"
    out = {"tool": "bf16_scan_bench", "hbm_peak_tbs": HBM_PEAK_TBS, "rounds": a.rounds, "queries": a.queries, "sizes": {}}
    for s in a.sizes.split(","):
        name, res = bench_size(s, SIZES[s], 768, a.rounds, a.queries)
        out["sizes"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
