#!/usr/bin/env python3
"""Tagged concurrent callers: what N daemon client threads see when every `search` carries a tag filter of its own
(`search_with_tags`; the shim's `search_with_filter`).  N native threads, each one blocking cqs_hip_index_search_tagged
(b = 1) call at a time (cqs_hip_debug_client_storm_tagged), on handles over the same rows and tags:
  serial tagged         a handle made under CQS_HIP_COMBINE_TAGGED=0 (one kernel + one pass per caller, under the mutex)
  combined tagged       the default: tagged callers park on the combining queue, a block's bitsets come from one kernel
  combined host bitset  the same default handle, the callers passing the HOST bitset of the same predicate instead
                        (cqs_hip_debug_client_storm_filtered)
with and without the shadow copies.  The runs are interleaved, repeated, and reported as median and min..max queries/s;
every answer is compared with the lone tagged call's.  `gate` (1 thread): the combined-tagged median is not below the
serial-tagged median by more than the serial handle's own min..max spread.  Prints one JSON document.

  python tools/tagged_clients.py [--rows 1000000] [--dim 768] [--reps 3] [--calls 960] [--threads 1,8,16] [--combined-first] [--control]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cqs_amd import HipIndex, synth, tag_filter  # noqa: E402


def make(rows, tags, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        idx = HipIndex.build_from_flat(None, rows)
        idx.set_tags(tags)
        return idx
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=960, help="calls per run, over all threads")
    ap.add_argument("--queries", type=int, default=48)
    ap.add_argument("--threads", default="1,8,16", help="thread counts, comma-separated")
    ap.add_argument("--control", action="store_true",
                    help="a second serial handle as a column of its own: what two handles on the SAME path differ by")
    ap.add_argument("--combined-first", action="store_true",
                    help="make the combined handles before the serial ones (tells a handle's placement from its path)")
    a = ap.parse_args()
    n, dim, nq = a.rows, a.dim, a.queries
    rows = synth.gaussian_unit(n, dim=dim, seed=synth.SEED_CORPUS)
    qs = np.ascontiguousarray(synth.gaussian_unit(nq, dim=dim, seed=synth.SEED_QUERY))
    rng = np.random.default_rng(5)
    tags = (rng.integers(0, 16, size=n).astype(np.uint32) | (rng.integers(0, 50, size=n).astype(np.uint32) << np.uint32(8)))
    # one filter per query: 8 (density 1/2) or 1 (1/16) of field 0's 16 codes, drawn per query
    allows, bits = {}, {}
    for name, m in (("1/2", 8), ("1/16", 1)):
        al = np.stack([tag_filter(sorted(int(v) for v in rng.choice(16, size=m, replace=False))) for _ in range(nq)])
        keep = np.stack([((al[i][0] >> (tags & np.uint32(15))) & np.uint32(1)).astype(bool) for i in range(nq)])
        allows[name] = np.ascontiguousarray(al, dtype=np.uint32)
        bits[name] = np.ascontiguousarray(np.packbits(np.pad(keep, ((0, 0), (0, (-n) % 32))), axis=1, bitorder="little")).view(np.uint32)
    handles = {}
    for shadow in (False, True):
        sh = {"CQS_HIP_SCAN_BF16": "1" if shadow else "0", "CQS_HIP_SCAN_I8": "1" if shadow else "0"}
        for path in (("combined", "serial") if a.combined_first else ("serial", "combined")):
            handles[(path, shadow)] = make(rows, tags, CQS_HIP_COMBINE_TAGGED="0" if path == "serial" else "1", **sh)
        if a.control:
            handles[("serial_b", shadow)] = make(rows, tags, CQS_HIP_COMBINE_TAGGED="0", **sh)
    lib = next(iter(handles.values()))._lib
    storm_t = lib.cqs_hip_debug_client_storm_tagged
    storm_f = lib.cqs_hip_debug_client_storm_filtered
    storm_f.restype = C.c_double
    storm_f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                        C.c_void_p, C.c_void_p, C.c_void_p]
    columns = [("serial tagged", "serial", True), ("combined tagged", "combined", True), ("combined host bitset", "combined", False)]
    if a.control:
        columns.append(("serial tagged B", "serial_b", True))
    out = {"rows": n, "dim": dim, "reps": a.reps, "calls_per_run": a.calls, "combined_first": a.combined_first, "cells": [], "gate_1_thread": []}
    f32 = handles[("serial", False)]
    for k in (20, 500):
        for dens in allows:
            al, kb = allows[dens], bits[dens]
            want = [f32.search_tagged_batch(qs[i], k, al[i]) for i in range(nq)]
            want_r = np.stack([w[0][0] for w in want]); want_s = np.stack([w[1][0] for w in want]); want_c = np.array([w[2][0] for w in want])
            for T in [int(t) for t in a.threads.split(",")]:
                per = max(20, a.calls // T)
                runs = [(name, path, tagged, shadow) for shadow in (False, True) for name, path, tagged in columns]
                qps = {r: [] for r in runs}
                cpp = {r: 0.0 for r in runs}
                for rep in range(a.reps + 1):                       # (rep 0 warms every handle)
                    for run in runs:
                        name, path, tagged, shadow = run
                        idx = handles[(path, shadow)]
                        r = np.zeros((nq, k), np.uint64); s = np.zeros((nq, k), np.float32); c = np.zeros((nq,), np.uint32)
                        stats = idx.combine_tagged_stats if tagged else idx.combine_filter_stats
                        p0, q0 = stats()
                        if tagged:
                            el = storm_t(idx._h, qs.ctypes.data, nq, dim, k, al.ctypes.data, T, per, r.ctypes.data, s.ctypes.data, c.ctypes.data)
                        else:
                            el = storm_f(idx._h, qs.ctypes.data, nq, dim, k, kb.ctypes.data, kb.shape[1], T, per, r.ctypes.data, s.ctypes.data, c.ctypes.data)
                        p1, q1 = stats()
                        assert el > 0, ("a client call failed", run, idx.last_error())
                        asked = sorted({(t + i * T) % nq for t in range(T) for i in range(per)})
                        assert np.array_equal(c[asked], want_c[asked]) and np.array_equal(r[asked], want_r[asked]) and \
                            np.array_equal(s[asked].view(np.uint32), want_s[asked].view(np.uint32)), ("answers differ from the lone call's", run, k, dens, T)
                        if rep:
                            qps[run].append(T * per / el)
                            cpp[run] = (q1 - q0) / max(p1 - p0, 1)
                for run in runs:
                    v = qps[run]
                    out["cells"].append({"k": k, "density": dens, "threads": T, "column": run[0], "shadow": run[3],
                                         "qps_median": round(statistics.median(v), 1), "qps_min": round(min(v), 1), "qps_max": round(max(v), 1),
                                         "mean_callers_per_pass": round(cpp[run], 2)})
                if T == 1:
                    for shadow in (False, True):
                        ser, com = qps[("serial tagged", "serial", True, shadow)], qps[("combined tagged", "combined", True, shadow)]
                        spread = max(ser) - min(ser)
                        out["gate_1_thread"].append({"k": k, "density": dens, "shadow": shadow, "serial_median": round(statistics.median(ser), 1),
                                                     "serial_spread": round(spread, 1), "combined_median": round(statistics.median(com), 1),
                                                     "holds": bool(statistics.median(com) >= statistics.median(ser) - spread)})
                        if a.control:       # the same rule between two handles on the same (serial) path
                            ctl = qps[("serial tagged B", "serial_b", True, shadow)]
                            out["gate_1_thread"][-1].update({"control_median": round(statistics.median(ctl), 1),
                                                             "control_holds": bool(statistics.median(ctl) >= statistics.median(ser) - spread)})
    for idx in handles.values():
        idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
