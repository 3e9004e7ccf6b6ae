#!/usr/bin/env python3
"""What a filtered search costs in front of the bitset: the tagged calls against the host-bitset ones.

  python tools/tagged_filter_bench.py [--rows 1000000] [--dim 768] [--chunks 1000000] [--k 20] [--reps 200]
                                      [--predicate-reps 3] [--skip-sparse] [--out FILE.json]

The predicate is the reference's: chunk type in an include set, language in a set (src/search/query.rs:860-900), over 30
chunk types and 50 languages drawn uniformly; it keeps about one row in thirty.  Per index (dense 1M x 768; the 1M-chunk
sparse corpus of tools/sparse_bench.py), the median, minimum and maximum over repeated BLOCKING single-query calls of
  a  search_tagged: the 128-byte filter, the bitset written on the device
  b  the host-bitset call with the bitset built beforehand (the library's cost behind the bitset alone)
  c  b plus building the bitset from a numpy tag array with vectorised numpy (two table lookups, an AND, packbits)
  d  search_with_filter with a per-id Python predicate that looks the id up in a dict, as the mirror does today
b to d run code the tags do not touch.  Dense only: `count_tagged` at `--rows` rows and at 256 rows (one workgroup) - the
launch, the kernel and the wait for the count, and the same with next to no kernel.  The kernel's own time comes from
a profiler run of its own, not from here; `kernel_bytes` = 4 n + n / 8 is what it reads and writes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TYPES, LANGS = 30, 50
INCLUDE_TYPES, INCLUDE_LANGS = (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--predicate-reps", type=int, default=3)
    ap.add_argument("--skip-sparse", action="store_true")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex, _lib, synth, tag_filter
    from cqs_amd.splade_index import HipSpladeIndex
    if not torch.cuda.is_available():
        raise SystemExit("tagged_filter_bench needs a GPU: nothing here is measured without one")
    allow = tag_filter(INCLUDE_TYPES, INCLUDE_LANGS)
    type_ok = np.zeros(256, dtype=bool)
    type_ok[list(INCLUDE_TYPES)] = True
    lang_ok = np.zeros(256, dtype=bool)
    lang_ok[list(INCLUDE_LANGS)] = True

    def make_tags(n, seed):
        rng = np.random.default_rng(seed)
        return (rng.integers(0, TYPES, size=n, dtype=np.uint32) | (rng.integers(0, LANGS, size=n, dtype=np.uint32) << np.uint32(8)))

    def numpy_bits(tags):
        keep = type_ok[tags & np.uint32(255)] & lang_ok[(tags >> np.uint32(8)) & np.uint32(255)]
        packed = np.packbits(keep, bitorder="little")
        out = np.zeros((len(tags) + 31) // 32 * 4, dtype=np.uint8)
        out[:packed.size] = packed
        return out.view(np.uint32)

    def predicate_for(tags):
        meta = {str(i): (int(t) & 255, (int(t) >> 8) & 255) for i, t in enumerate(tags)}     # id -> (chunk type, language)
        types, langs = set(INCLUDE_TYPES), set(INCLUDE_LANGS)

        def flt(cid):
            m = meta.get(cid)
            return m is not None and m[0] in types and m[1] in langs
        return flt

    res = {"tool": "tagged_filter_bench", "k": a.k, "filter": {"types": len(INCLUDE_TYPES), "of": TYPES, "languages": len(INCLUDE_LANGS), "of_": LANGS}}

    # ---- dense ---------------------------------------------------------------------------------------------------------
    n, dim = a.rows, a.dim
    flat = make_unit_rows(torch, n, dim, 0xC950011, torch.device("cuda")).cpu().numpy()
    q = make_unit_rows(torch, 1, dim, 0xC950012, torch.device("cuda")).cpu().numpy()[0]
    idx = HipIndex.build_from_flat(None, flat)
    del flat
    tags = make_tags(n, 0xC950013)
    idx.set_tags(tags)
    bits = numpy_bits(tags)
    kept = idx.count_tagged(allow)
    assert kept == int(np.unpackbits(bits.view(np.uint8), bitorder="little")[:n].sum())
    got, want = idx.search_tagged_batch(q, a.k, allow), idx.search_batch(q, a.k, keep_bitset=bits)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)), "tagged and host-bitset answers differ"
    flt = predicate_for(tags)
    dense = {"rows": n, "dim": dim, "kept_rows": kept, "bf16_shadow_bytes": idx.bf16_stats()[0], "kernel_bytes": 4 * n + n // 8,
             "a_search_tagged": timed(lambda: idx.search_tagged_batch(q, a.k, allow), a.reps),
             "b_host_bitset_prebuilt": timed(lambda: idx.search_batch(q, a.k, keep_bitset=bits), a.reps),
             "c_numpy_bitset_and_search": timed(lambda: idx.search_batch(q, a.k, keep_bitset=numpy_bits(tags)), a.reps),
             "unfiltered": timed(lambda: idx.search_batch(q, a.k), a.reps),
             "count_tagged": timed(lambda: idx.count_tagged(allow), a.reps),
             "d_python_predicate": timed(lambda: idx.search_with_filter(q, a.k, flt), a.predicate_reps, warm=1)}
    idx.close()
    small = HipIndex.build_from_flat(None, np.ascontiguousarray(make_unit_rows(torch, 256, dim, 0xC950014, torch.device("cuda")).cpu().numpy()))
    small.set_tags(tags[:256])
    dense["count_tagged_256_rows"] = timed(lambda: small.count_tagged(allow), a.reps)
    small.close()
    res["dense"] = dense
    print("dense", json.dumps(dense), flush=True)

    # ---- sparse --------------------------------------------------------------------------------------------------------
    if not a.skip_sparse:
        lib = _lib.load()
        off, tok, w = synth.sparse_corpus(a.chunks)
        sp = HipSpladeIndex.build_from_csr(None, off, tok, w)
        del off, tok, w
        stags = make_tags(a.chunks, 0xC950015)
        sp.set_tags(stags)
        sbits = numpy_bits(stags)
        qt, qw = synth.sparse_queries(1, 64)[0]
        out, sc, cnt = np.zeros(a.k, dtype=np.uint64), np.zeros(a.k, dtype=np.float32), C.c_uint32()

        def host_bitset(b):
            rc = lib.cqs_hip_sparse_index_search(sp._h, qt.ctypes.data, qw.ctypes.data, qt.size, a.k, b.ctypes.data, out.ctypes.data,
                                                 sc.ctypes.data, C.byref(cnt))
            assert rc == _lib.OK
            return out[:cnt.value].copy(), sc[:cnt.value].copy()
        tch, tsc, trc = sp.search_tagged_raw(qt, qw, a.k, allow)
        hch, hsc = host_bitset(sbits)
        assert trc == _lib.OK and np.array_equal(tch, hch) and np.array_equal(tsc.view(np.uint32), hsc.view(np.uint32))
        sflt = predicate_for(stags)
        query = [(int(t), float(x)) for t, x in zip(qt, qw)]
        sparse = {"chunks": a.chunks, "postings": sp.postings(), "terms": int(qt.size), "kernel_bytes": 4 * a.chunks + a.chunks // 8,
                  "a_search_tagged": timed(lambda: sp.search_tagged_raw(qt, qw, a.k, allow), a.reps),
                  "b_host_bitset_prebuilt": timed(lambda: host_bitset(sbits), a.reps),
                  "c_numpy_bitset_and_search": timed(lambda: host_bitset(numpy_bits(stags)), a.reps),
                  "unfiltered": timed(lambda: sp.search_raw(qt, qw, a.k), a.reps),
                  "d_python_predicate": timed(lambda: sp.search_with_filter(query, a.k, sflt), a.predicate_reps, warm=1)}
        sp.close()
        res["sparse"] = sparse
        print("sparse", json.dumps(sparse), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
