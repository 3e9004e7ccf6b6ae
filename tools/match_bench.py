#!/usr/bin/env python3
"""`cqs_hip_index_match` between two resident corpora, and the route that existed before it.

  python tools/match_bench.py [--n 1000000] [--dim 768] [--lists 1024,8192,65536] [--reps 5] [--out FILE.json]

Two indexes of `--n` x `--dim` unit rows borrowed from torch tensors; for each list length m, m distinct random rows per
side.  Host-timed around the blocking call (it ends in a stream wait), the first two calls left out: time per call and the
implied TFLOP/s on the algorithmic 2 m^2 dim flops.  For m = 1024 only, beside it the route available before this call:
`search_batch_filtered` on `b` with a's m vectors taken from HOST memory (no API reads stored rows back) and one
keep-bitset of rows_b for every query, k = 1 - the A side's answer only; the B side would need the same again the other
way round.  Before anything is timed the 1024 case is held to numpy f64 over the host copies of its rows (scores within
1e-5, the best position wherever numpy's best and runner-up are more than 2e-6 apart).  One JSON line.  No threshold on the
times: the reading belongs in DESIGN §3.17a / §8."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--lists", type=str, default="1024,8192,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex
    if not torch.cuda.is_available():
        raise SystemExit("match_bench needs a GPU: nothing here is measured without one")
    n, dim = a.n, a.dim
    os.environ.setdefault("CQS_HIP_SCAN_BF16", "0")   # (the match reads the f32 rows; the old route is timed on the f32 scan)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0x3A7C4)
    da = make_unit_rows(torch, n, dim, 0xC950041, dev)
    db = make_unit_rows(torch, n, dim, 0xC950042, dev)
    ia = HipIndex.build_from_device(None, da.data_ptr(), n, dim, borrow=True, keepalive=da)
    ib = HipIndex.build_from_device(None, db.data_ptr(), n, dim, borrow=True, keepalive=db)

    def median(fn):
        times = []
        for _ in range(a.reps + 2):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        times = sorted(times[2:])
        return times[len(times) // 2], times[0], times[-1]

    res = {"tool": "match_bench", "n": n, "dim": dim, "reps": a.reps, "device": torch.cuda.get_device_name(0), "lists": {}}
    for m in [int(x) for x in a.lists.split(",") if x]:
        m = min(m, n)
        rows_a = torch.randperm(n, generator=g, device=dev)[:m].cpu().numpy().astype(np.uint64)
        rows_b = torch.randperm(n, generator=g, device=dev)[:m].cpu().numpy().astype(np.uint64)
        entry = {}
        if m <= 1024:
            ha = da[torch.from_numpy(rows_a.astype(np.int64)).to(dev)].cpu().numpy()
            hb = db[torch.from_numpy(rows_b.astype(np.int64)).to(dev)].cpu().numpy()
            s = ha.astype(np.float64) @ hb.astype(np.float64).T
            best_a, score_a, best_b, score_b = ia.match_rows(ib, rows_a, rows_b)
            for best, score, ref in ((best_a, score_a, s), (best_b, score_b, s.T)):
                top2 = np.sort(ref, axis=1)[:, -2:]
                clear = top2[:, 1] - top2[:, 0] > 2e-6
                if np.abs(score - top2[:, 1]).max() > 1e-5 or not np.array_equal(best[clear], np.argmax(ref, axis=1)[clear].astype(np.uint64)):
                    raise SystemExit("the device's bests differ from numpy f64's")
            # the route before: a's vectors from host memory, rows_b as a keep-bitset, k = 1 (the A side only)
            words = np.zeros(((n + 31) // 32,), np.uint32)
            np.bitwise_or.at(words, (rows_b >> np.uint64(5)).astype(np.int64), (np.uint32(1) << (rows_b & np.uint64(31)).astype(np.uint32)))
            keeps = np.ascontiguousarray(np.broadcast_to(words, (m, words.shape[0])))
            got_rows, got_scores, counts = ib.search_batch_filtered(ha, 1, keeps)
            pos_of = {int(r): j for j, r in enumerate(rows_b)}
            old_best = np.array([pos_of[int(r)] for r in np.asarray(got_rows).reshape(m, -1)[:, 0]], np.uint64)
            top2 = np.sort(s, axis=1)[:, -2:]
            clear = top2[:, 1] - top2[:, 0] > 2e-6
            if not np.array_equal(old_best[clear], best_a[clear]):
                raise SystemExit("the filtered-search route and the match disagree on a clear best")
            t = median(lambda: ib.search_batch_filtered(ha, 1, keeps))
            entry["filtered_search_a_side_ms_median_min_max"] = [round(x * 1e3, 3) for x in t]
            entry["checked_against_numpy_f64"] = True
        t = median(lambda: ia.match_rows(ib, rows_a, rows_b))
        flops = 2.0 * m * m * dim
        entry["match_ms_median_min_max"] = [round(x * 1e3, 3) for x in t]
        entry["match_TFLOPs"] = round(flops / t[0] / 1e12, 2)
        res["lists"][str(m)] = entry
    ia.close(); ib.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
