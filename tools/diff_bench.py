#!/usr/bin/env python3
"""`cqs_hip_index_diff` between two resident corpora against the two CPU routes it replaces.

  python tools/diff_bench.py [--n 1000000] [--dim 768] [--pairs 1000000] [--reps 10] [--cpu-sample 20000] [--out FILE.json]

Two indexes of `--n` x `--dim` unit rows (the second holds the first's rows in another order, each perturbed: about 1 % of them
far enough to fall below the threshold 0.9), borrowed from torch tensors, and `--pairs` matched pairs in random order, so both
gathers are random.  Host-timed around the blocking call (it ends in a stream wait), the first two calls left out:
  diff            `cqs_hip_index_diff` with the modified list and the counts only
  diff_with_sims  the same with out_sims (4 bytes a pair more across the bus)
and the achieved bytes/s of each on the algorithmic 2 * pairs * dim * 4 bytes.  Beside them, over `--cpu-sample` of the pairs
with their rows in host memory, per pair and extrapolated to all pairs:
  oracle_loop     oracle.full_cosine_similarity pair by pair on one core (the reference's loop)
  numpy_f64       dot and norms as f64 row sums over blocks of 1000 pairs (the reference's batch size)
Before anything is timed the sampled pairs are checked against the oracle: every sim equal or adjacent, the same pairs below
the threshold.  One JSON line.  No threshold on the times: the reading belongs in DESIGN §3.17."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESHOLD = 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-sample", type=int, default=20_000)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex
    from oracle import oracle
    if not torch.cuda.is_available():
        raise SystemExit("diff_bench needs a GPU: nothing here is measured without one")
    n, dim, m = a.n, a.dim, a.pairs
    os.environ.setdefault("CQS_HIP_SCAN_BF16", "0")   # (the diff reads the f32 rows: no shadow copies of 3 GB corpora for it)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0xD1FF)
    da = make_unit_rows(torch, n, dim, 0xC950031, dev)
    sigma = torch.randperm(n, generator=g, device=dev)
    scale = torch.where(torch.rand(n, 1, generator=g, device=dev) < 0.01, 3.0, 0.05) / dim ** 0.5
    db = da[sigma]
    db += torch.randn(n, dim, generator=g, device=dev) * scale
    db /= db.norm(dim=1, keepdim=True)
    ia = HipIndex.build_from_device(None, da.data_ptr(), n, dim, borrow=True, keepalive=da)
    ib = HipIndex.build_from_device(None, db.data_ptr(), n, dim, borrow=True, keepalive=db)
    pick = torch.randint(0, n, (m,), generator=g, device=dev) if m != n else torch.randperm(n, generator=g, device=dev)
    rows_b = pick.cpu().numpy().astype(np.uint64)
    rows_a = sigma[pick].cpu().numpy().astype(np.uint64)

    # the sampled pairs on the host, and the check against the oracle before anything is timed
    s = min(a.cpu_sample, m)
    sample = np.linspace(0, m - 1, num=s, dtype=np.int64)
    ha = da[torch.from_numpy(rows_a[sample].astype(np.int64)).to(dev)].cpu().numpy()
    hb = db[torch.from_numpy(rows_b[sample].astype(np.int64)).to(dev)].cpu().numpy()
    mod, mod_sims, counts, sims = ia.diff_rows(ib, rows_a, rows_b, THRESHOLD, want_sims=True)
    t0 = time.perf_counter()
    want = np.array([oracle.full_cosine_similarity(ha[i], hb[i]) for i in range(s)], np.float32)
    t_oracle = (time.perf_counter() - t0) / s
    got = sims[sample]
    near = (got == want) | (got == np.nextafter(want, np.float32(2))) | (got == np.nextafter(want, np.float32(-2)))
    if not near.all() or not np.array_equal(got < np.float32(THRESHOLD), want < np.float32(THRESHOLD)):
        raise SystemExit("the device's sims differ from the oracle's on the sampled pairs")
    if int(counts[0]) != int((sims < np.float32(THRESHOLD)).sum()) or not np.array_equal(mod, np.flatnonzero(sims < np.float32(THRESHOLD))):
        raise SystemExit("the modified list is not the filter of out_sims")
    t0 = time.perf_counter()
    for lo in range(0, s, 1000):
        x, y = ha[lo:lo + 1000].astype(np.float64), hb[lo:lo + 1000].astype(np.float64)
        (np.einsum("ij,ij->i", x, y) / (np.sqrt(np.einsum("ij,ij->i", x, x)) * np.sqrt(np.einsum("ij,ij->i", y, y)))).astype(np.float32)
    t_numpy = (time.perf_counter() - t0) / s

    def timed(want_sims):
        times = []
        for rep in range(a.reps + 2):
            t0 = time.perf_counter()
            ia.diff_rows(ib, rows_a, rows_b, THRESHOLD, want_sims=want_sims)
            times.append(time.perf_counter() - t0)
        times = sorted(times[2:])
        return times[len(times) // 2], times[0], times[-1]

    # alternate the two forms so that drift of the machine falls on both
    lists_only, with_sims = timed(False), timed(True)
    lists_again = timed(False)
    ia.close(); ib.close()
    algo = 2.0 * m * dim * 4
    res = {"tool": "diff_bench", "n": n, "dim": dim, "pairs": m, "threshold": THRESHOLD, "modified": int(counts[0]),
           "modified_share": round(int(counts[0]) / m, 4), "undefined": int(counts[2]), "sampled_pairs_checked": s,
           "sims_one_ulp_from_oracle": int((got != want).sum()), "reps": a.reps,
           "diff_ms_median_min_max": [round(t * 1e3, 3) for t in lists_only], "diff_again_ms_median_min_max": [round(t * 1e3, 3) for t in lists_again],
           "diff_with_sims_ms_median_min_max": [round(t * 1e3, 3) for t in with_sims],
           "algorithmic_bytes": int(algo), "diff_GBps": round(algo / lists_only[0] / 1e9, 1), "diff_with_sims_GBps": round(algo / with_sims[0] / 1e9, 1),
           "oracle_loop_us_per_pair": round(t_oracle * 1e6, 3), "oracle_loop_extrapolated_s": round(t_oracle * m, 2),
           "numpy_f64_us_per_pair": round(t_numpy * 1e6, 3), "numpy_f64_extrapolated_s": round(t_numpy * m, 2),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
