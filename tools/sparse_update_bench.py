#!/usr/bin/env python3
"""`cqs_hip_sparse_index_remove` / `cqs_hip_sparse_index_extend` against the only alternative before them, a rebuild of the
sparse index from host memory.

  python tools/sparse_update_bench.py [--chunks 1000000] [--update 1000] [--reps 10] [--rebuild-reps 3] [--out FILE.json]

The corpus is the one `bench_legs/sparse.py` measures (`synth.sparse_corpus`: ~96 postings per chunk, 30 522 tokens, skewed).
Host-timed around the blocking calls, integer-addressed (unranked) handle:
  remove   `--update` seeded scattered chunks leave the index
  extend   the same documents join it again (as its last chunks)
  rebuild  `HipSpladeIndex.build_from_csr` of the documents that remain after the remove, from host memory (no store
           scan: this flatters the rebuild)
One untimed warm-up pair, then `--reps` pairs, every pair at `--chunks` chunks; median, minimum and maximum are reported.
`payload_bytes` is what the call must move at least: every posting read once and written once (16 B x postings) plus
the range directories written (4 B x entries); `payload_tbps` = payload_bytes / median time.  The remove reads the postings
a second time (its counting pass) and both calls read the new array once more to fill the directories."""
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


def csr_take(np, csr, docs):
    off, tok, w = csr
    lens = (off[1:] - off[:-1]).astype(np.int64)[docs]
    new_off = np.zeros(docs.size + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum(lens)
    idx = np.repeat(off[:-1].astype(np.int64)[docs] - new_off[:-1].astype(np.int64), lens) + np.arange(int(new_off[-1]), dtype=np.int64)
    return new_off, tok[idx], w[idx]


def directory_entries(np, tok, chunks, n_cu=256):
    """The range directories' entries for these postings (cqs_amd/csrc/sparse_geometry.h)."""
    n_pad = max((chunks + 1023) // 1024 * 1024, 1024)
    rw = 1024
    while rw > 64 and n_pad // rw < n_cu * 16:
        rw //= 2
    lens = np.bincount(tok)
    lists = int(np.count_nonzero(lens >= 32))
    per_list = n_pad // rw + 1
    budget = max(16 << 20, 2 * int(tok.size))
    return min(lists, budget // per_list) * per_list


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--update", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    from cqs_amd import _lib, synth
    from cqs_amd.splade_index import HipSpladeIndex
    if _lib.load().cqs_hip_device_count() <= 0:
        raise SystemExit("sparse_update_bench needs a GPU: nothing here is measured without one")
    n, m, vocab = a.chunks, a.update, 30522
    corpus = synth.sparse_corpus(n, vocab)
    ix = HipSpladeIndex.build_from_csr(None, *corpus)
    P = ix.postings()
    res = {"tool": "sparse_update_bench", "chunks": n, "postings": P, "unique_tokens": ix.unique_tokens(), "updated": m}
    rng = np.random.default_rng(0x5BA2F1)
    cur = np.arange(n, dtype=np.int64)                        # the document every chunk of the handle holds
    after_remove = None
    t_rm, t_ex, moved = [], [], 0
    for rep in range(a.reps + 1):                             # the first pair warms the kernels and the allocator
        rows = np.sort(rng.choice(n, size=m, replace=False))
        docs = csr_take(np, corpus, cur[rows])
        t0 = time.perf_counter()
        removed = ix.remove_chunks(rows)
        t1 = time.perf_counter()
        assert removed == m and len(ix) == n - m
        if after_remove is None:
            after_remove = np.delete(cur, rows)
        t2 = time.perf_counter()
        ix.extend_csr(None, *docs)
        t3 = time.perf_counter()
        assert len(ix) == n and ix.postings() == P
        moved = int(docs[0][-1])
        cur = np.concatenate([np.delete(cur, rows), cur[rows]])
        if rep:
            t_rm.append((t1 - t0) * 1e3)
            t_ex.append((t3 - t2) * 1e3)
    payload = 16 * P + 4 * directory_entries(np, corpus[1], n)
    for name, ms in (("remove", t_rm), ("extend", t_ex)):
        s = spread(ms)
        s["payload_bytes"] = payload
        s["payload_tbps"] = round(payload / (s["median_ms"] * 1e-3) / 1e12, 3)
        s["share_of_hbm"] = round(s["payload_tbps"] / HBM_PEAK_TBPS, 3)
        res[name] = s
        print(name, json.dumps(s), flush=True)
    res["postings_per_update"] = moved
    # the handle after all that against a rebuild of the same documents: one query, the same bytes
    qt, qw = synth.sparse_queries(1, 64, vocab, seed=0x5BA2F3)[0]
    got = ix.search_raw(qt, qw, 500)
    ix.close()
    fresh = HipSpladeIndex.build_from_csr(None, *csr_take(np, corpus, cur))
    want = fresh.search_raw(qt, qw, 500)
    fresh.close()
    assert got[2] == 0 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    kept = csr_take(np, corpus, after_remove)
    ms = []
    for rep in range(a.rebuild_reps + 1):
        t0 = time.perf_counter()
        f = HipSpladeIndex.build_from_csr(None, *kept)
        t1 = time.perf_counter()
        f.close()
        if rep:
            ms.append((t1 - t0) * 1e3)
    res["rebuild"] = spread(ms)
    print("rebuild", json.dumps(res["rebuild"]), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
