#!/usr/bin/env python3
"""Filtered concurrent callers: what N daemon client threads see when every `search` carries a keep-bitset (hybrid search,
--lang / type filters).  N native threads, each one blocking cqs_hip_index_search(b = 1, keep_bitset) call at a time
(cqs_hip_debug_client_storm_filtered), on handles over the same rows made with CQS_HIP_COMBINE_FILTERED=0 (the serial path)
and with the default (filtered callers share passes), with and without the shadow copies.  The runs of the handles are
interleaved, repeated, and reported as median and min..max queries/s; every answer is compared with the lone call's.
Also: the host cost of staging the bitsets of an 8-query block, from block timings.  Prints one JSON document.

  python tools/filtered_clients.py [--rows 1000000] [--dim 768] [--reps 5] [--calls 960]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cqs_amd import HipIndex, synth  # noqa: E402


def make(rows, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return HipIndex.build_from_flat(None, rows)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=960, help="calls per run, over all threads")
    ap.add_argument("--queries", type=int, default=48)
    a = ap.parse_args()
    n, dim, nq = a.rows, a.dim, a.queries
    rows = synth.gaussian_unit(n, dim=dim, seed=synth.SEED_CORPUS)
    qs = np.ascontiguousarray(synth.gaussian_unit(nq, dim=dim, seed=synth.SEED_QUERY))
    words = (n + 31) // 32
    rng = np.random.default_rng(5)
    bits = {}
    for name, dens in (("1/2", 0.5), ("1/16", 1 / 16)):
        keep = rng.random((nq, words * 32)) < dens
        bits[name] = np.ascontiguousarray(np.packbits(keep, axis=1, bitorder="little")).view(np.uint32)
    handles = {}
    for shadow in (False, True):
        sh = {"CQS_HIP_SCAN_BF16": "1" if shadow else "0", "CQS_HIP_SCAN_I8": "1" if shadow else "0"}
        handles[("serial", shadow)] = make(rows, CQS_HIP_COMBINE_FILTERED="0", **sh)
        handles[("combined", shadow)] = make(rows, CQS_HIP_COMBINE_FILTERED="1", **sh)
    lib = next(iter(handles.values()))._lib
    storm = lib.cqs_hip_debug_client_storm_filtered
    storm.restype = C.c_double
    storm.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                      C.c_void_p, C.c_void_p, C.c_void_p]
    out = {"rows": n, "dim": dim, "reps": a.reps, "calls_per_run": a.calls, "bitset_bytes": words * 4, "cells": []}
    f32 = handles[("serial", False)]
    for k in (20, 500):
        for dens, kb in bits.items():
            want = [f32.search_batch(qs[i], k, keep_bitset=kb[i]) for i in range(nq)]
            want_r = np.stack([w[0][0] for w in want]); want_s = np.stack([w[1][0] for w in want]); want_c = np.array([w[2][0] for w in want])
            for T in (1, 8, 16):
                per = max(20, a.calls // T)
                qps = {key: [] for key in handles}
                cpp = {key: 0.0 for key in handles}
                for rep in range(a.reps + 1):                       # (rep 0 warms every handle)
                    for key, idx in handles.items():
                        r = np.zeros((nq, k), np.uint64); s = np.zeros((nq, k), np.float32); c = np.zeros((nq,), np.uint32)
                        p0, q0 = idx.combine_filter_stats()
                        el = storm(idx._h, qs.ctypes.data, nq, dim, k, kb.ctypes.data, kb.shape[1], T, per, r.ctypes.data, s.ctypes.data, c.ctypes.data)
                        p1, q1 = idx.combine_filter_stats()
                        assert el > 0, "a client call failed"
                        asked = sorted({(t + i * T) % nq for t in range(T) for i in range(per)})
                        assert np.array_equal(c[asked], want_c[asked]) and np.array_equal(r[asked], want_r[asked]) and \
                            np.array_equal(s[asked].view(np.uint32), want_s[asked].view(np.uint32)), ("answers differ from the lone call's", key, k, dens, T)
                        if rep:
                            qps[key].append(T * per / el)
                            cpp[key] = (q1 - q0) / max(p1 - p0, 1)
                for key in handles:
                    v = qps[key]
                    out["cells"].append({"k": k, "density": dens, "threads": T, "path": key[0], "shadow": key[1],
                                         "qps_median": round(statistics.median(v), 1), "qps_min": round(min(v), 1), "qps_max": round(max(v), 1),
                                         "mean_callers_per_pass": round(cpp[key], 2)})
    # host cost of staging 8 bitsets: wall time minus scan-kernel time of an 8-query block, filtered against unfiltered
    idx = handles[("combined", False)]
    kb = bits["1/2"]
    stage = {}
    for name, call in (("filtered", lambda: idx.search_batch_filtered(qs[:8], 20, kb[:8])), ("unfiltered", lambda: idx.search_batch(qs[:8], 20))):
        call()
        idx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(50):
            call()
        wall = (time.perf_counter() - t0) / 50 * 1e3
        _, ms = idx.scan_time()
        idx.set_timing(False)
        stage[name] = {"wall_ms": round(wall, 4), "scan_ms": round(ms / 50, 4), "outside_scan_ms": round(wall - ms / 50, 4)}
    stage["staging_8_bitsets_ms"] = round(stage["filtered"]["outside_scan_ms"] - stage["unfiltered"]["outside_scan_ms"], 4)
    out["block_of_8"] = stage
    for idx in handles.values():
        idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
