#!/usr/bin/env python3
"""`search_device` cells around the shadow search's tail at 1M x 768 (the bench's corpus and its 330 seeded queries): ms per
search for b in {1, 2, 4, 8} x k in {1, 20, 87, 100, 500}, and, where the library has the hook, how many of the 330 queries
certified on the finisher's prefix and how many went on to the second sort, per k (b = 1).  One JSON line.  Run it once per
arm and process (CQS_HIP_LIB picks another build, CQS_HIP_TAIL_PREFIX=0 the full-sort arm, CQS_HIP_TAIL_PREFIX_FIRST=0 the
tail without tiers).
usage: tail_cells.py [--steps 200] [--rows 1000000] [--bs 1,2,4,8] [--ks 1,20,87,100,500] [--census-ks 1,5,20,50,87] [--no-census]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--bs", type=str, default="1,2,4,8")
ap.add_argument("--ks", type=str, default="1,20,87,100,500")
ap.add_argument("--census-ks", type=str, default="1,5,20,50,87")
ap.add_argument("--no-census", action="store_true")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bench_legs.common import make_unit_rows
from cqs_amd import HipIndex, _lib

dev, dim = "cuda:0", 768
rows = make_unit_rows(torch, a.rows, dim, 0xC950001, dev)
queries = make_unit_rows(torch, 330, dim, 0xC950002, dev)
idx = HipIndex.build_from_device(None, rows.data_ptr(), a.rows, dim, borrow=True, keepalive=rows)
st = torch.cuda.current_stream().cuda_stream
out = {"lib": os.environ.get("CQS_HIP_LIB", "tree"), "tail_prefix": os.environ.get("CQS_HIP_TAIL_PREFIX", "1"),
       "tail_prefix_first": os.environ.get("CQS_HIP_TAIL_PREFIX_FIRST", "unset"), "rows": a.rows, "cells_ms": {}}
for b in [int(v) for v in a.bs.split(",")]:
    for k in [int(v) for v in a.ks.split(",")]:
        keys = torch.zeros((b, k), dtype=torch.int64, device=dev)
        counts = torch.zeros((b,), dtype=torch.int32, device=dev)

        def run(n):
            for i in range(n):
                q0 = (i * b) % (330 - b)
                idx.search_device(queries[q0].data_ptr(), b, k, keys.data_ptr(), counts.data_ptr(), stream=st)
            torch.cuda.synchronize()

        run(20)
        t = time.perf_counter()
        run(a.steps)
        out["cells_ms"][f"b{b}_k{k}"] = round((time.perf_counter() - t) / a.steps * 1e3, 5)
lib = _lib.load()
if not a.no_census and hasattr(lib, "cqs_hip_debug_tail_verdicts"):
    f = lib.cqs_hip_debug_tail_verdicts
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]

    def pre():
        cert, p = np.zeros(1, np.uint32), np.zeros(2, np.uint64)
        assert f(idx._h, 1, cert.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)) == _lib.OK
        return int(p[0]), int(p[1])

    out["census_330_queries_b1"] = {}
    for k in [int(v) for v in a.census_ks.split(",")]:
        keys = torch.zeros((1, k), dtype=torch.int64, device=dev)
        counts = torch.zeros((1,), dtype=torch.int32, device=dev)
        p0, c0 = pre(), idx.bf16_stats()
        for i in range(330):
            idx.search_device(queries[i].data_ptr(), 1, k, keys.data_ptr(), counts.data_ptr(), stream=st)
        p1, c1 = pre(), idx.bf16_stats()
        out["census_330_queries_b1"][f"k{k}"] = {"prefix_certified": p1[0] - p0[0], "second_sort": p1[1] - p0[1],
                                                 "certified": c1[1] - c0[1], "fallbacks": c1[2] - c0[2]}
print(json.dumps(out), flush=True)
idx.close()
