#!/usr/bin/env python3
"""Where the tail of a certified shadow search spends its time: the phase stamps (s_memrealtime, CQS_HIP_DEBUG_STAMPS=1)
of select_body and of rescore_certify_kernel for the headline shape, one query against 1M x 768 rows at k = 20 through
`search_device`, medians over the searches.  Stamps 0-5 are workgroup (0, 0)'s select, 6 / 7 the first candidate's row
loads issued / reduced (lane 0 of that workgroup's wave 1), 10 its ticket returned; 14 / 11 / 12 / 13 belong to whichever
workgroup finishes the query: its ticket returned, the exact keys listed in LDS, sorted, outputs stored.  A finisher whose
prefix does not certify under CQS_HIP_TAIL_PREFIX_FIRST leaves three more (words 16-18): prefix refused, second select done,
remaining rows' keys in LDS.  --crowd N plants, for every query, 20 rows at cosine 0.894 and N just below them (closer than the
int8 copy's B_q): 150 makes every prefix at k = 20 fail and every k' certify, which is how the slow path is timed.
usage: tail_stamps.py [--searches 50] [--rows 1000000] [--dim 768] [--k 20] [--crowd 0]"""
import argparse
import ctypes as C
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--searches", type=int, default=50)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--crowd", type=int, default=0)
a = ap.parse_args()
os.environ["CQS_HIP_DEBUG_STAMPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bench_legs.common import make_unit_rows
from cqs_amd import HipIndex, _lib

dev = "cuda:0"
rows = make_unit_rows(torch, a.rows, a.dim, 0xC950001, dev)
queries = make_unit_rows(torch, a.searches + 5, a.dim, 0xC950002, dev)
if a.crowd:
    per = 20 + a.crowd
    for i in range(a.searches + 5):
        blk = rows[i * per:(i + 1) * per]
        w = torch.full((per, 1), 2.0, device=dev)
        w[20:, 0] = 1.97 + 0.0001 * (torch.arange(a.crowd, device=dev) % 50)
        v = queries[i][None] * w + (blk - (blk @ queries[i])[:, None] * queries[i][None])
        rows[i * per:(i + 1) * per] = v / v.norm(dim=1, keepdim=True)
idx = HipIndex.build_from_device(None, rows.data_ptr(), a.rows, a.dim, borrow=True, keepalive=rows)
lib = _lib.load()
hook = lib.cqs_hip_debug_tail_stamps
hook.restype = C.c_int32
hook.argtypes = [C.c_void_p, C.c_void_p]
keys = torch.zeros((1, a.k), dtype=torch.int64, device=dev)
counts = torch.zeros((1,), dtype=torch.int32, device=dev)
st = torch.cuda.current_stream().cuda_stream
got = []
for i in range(a.searches + 5):
    idx.search_device(queries[i].data_ptr(), 1, a.k, keys.data_ptr(), counts.data_ptr(), stream=st)
    torch.cuda.synchronize()
    buf = np.zeros(20, np.uint64)                          # (16 words from a library without the slow path's stamps)
    assert hook(idx._h, buf.ctypes.data_as(C.c_void_p)) == _lib.OK, idx.last_error()
    if i >= 5:                                             # (the first searches warm the caches and the clocks)
        got.append(buf.astype(np.int64))
d = np.stack(got)
us = lambda x, y: (d[:, x] - d[:, y]) * 0.01               # 100 MHz counter
_, cert, fb = idx.bf16_stats()
print(f"# tail stamps: {a.rows} x {a.dim}, k = {a.k}, b = 1, {a.searches} searches")
print(f"# certified {cert}, fallbacks {fb} (warm-up included); groups listed by the select: median {int(np.median(d[:, 8]))},"
      f" candidates: median {int(np.median(d[:, 9]))} (CQS_HIP_I8_GROUPS={os.environ.get('CQS_HIP_I8_GROUPS', '1')})")
vh = lib.cqs_hip_debug_tail_verdicts
vh.restype = C.c_int32
vh.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
cw, pw = np.zeros(1, np.uint32), np.zeros(2, np.uint64)
assert vh(idx._h, 1, cw.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p)) == _lib.OK
print(f"# finisher: {int(pw[0])} searches certified on the prefix of 6k + 40 candidates, {int(pw[1])} went on to sort all (warm-up included;"
      f" CQS_HIP_TAIL_PREFIX={os.environ.get('CQS_HIP_TAIL_PREFIX', '1')},"
      f" CQS_HIP_TAIL_PREFIX_FIRST={os.environ.get('CQS_HIP_TAIL_PREFIX_FIRST', 'unset')}, CQS_HIP_LIB={os.environ.get('CQS_HIP_LIB', 'unset')})")


def line(name, v):
    print(f"{name:46s} median {np.median(v):6.2f}  p10 {np.percentile(v, 10):6.2f}  p90 {np.percentile(v, 90):6.2f} us")


s = us
line("  histogram of the maxima (link 1) 0 -> 1", s(1, 0))
line("  decide the threshold bin (2)    1 -> 2", s(2, 1))
line("  group list (link 3)             2 -> 3", s(3, 2))
line("  candidates (link 4)             3 -> 4", s(4, 3))
line("  sort (link 5)                   4 -> 5", s(5, 4))
line("select (links 1-5)                0 -> 5", s(5, 0))
line("first row loads issued            5 -> 6", s(6, 5))
line("first row reduced (link 6)        6 -> 7", s(7, 6))
line("wg 0: store, drain, barrier, ticket 7 -> 10", s(10, 7))
line("finisher's ticket after wg 0's   10 -> 14", s(14, 10))
line("finisher's keys loaded (link 9)  14 -> 11", s(11, 14))
line("sort (link 10)                   11 -> 12", s(12, 11))
line("outputs stored (link 11)         12 -> 13", s(13, 12))
line("links 6-10                        6 -> 12", s(12, 6))
line("whole tail                        0 -> 13", s(13, 0))
slow = d[:, 16] != 0
if slow.any():
    d = d[slow]
    print(f"# slow path (prefix refused, the finisher goes on alone): {int(slow.sum())} of {len(slow)} searches")
    line("  ticket -> prefix refused       14 -> 16", s(16, 14))
    line("  second select                  16 -> 17", s(17, 16))
    line("  remaining rows rescored        17 -> 18", s(18, 17))
    line("  sort of all kept keys          18 -> 12", s(12, 18))
    line("  slow path                      16 -> 12", s(12, 16))
    line("  whole tail of these            0 -> 13", s(13, 0))
idx.close()
