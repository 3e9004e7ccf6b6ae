#!/usr/bin/env python3
"""A loop of the two tag kernels for a kernel trace (`rocprofv3 --kernel-trace -- python tools/tags_multi_loop.py`, no
counters in the same run): `tags_keep_multi_kernel` through its debug hook at f = 8 and f = 32, and `tags_keep_kernel`
through `count_tagged`, over the same tag column.  Half-full filters in field 0; the kernels do not look at the rows, so
the index is narrow (dim 64).  In such a loop the column is probably re-read from cache.

  python tools/tags_multi_loop.py [--rows 1000000] [--loops 300]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cqs_amd import HipIndex, _lib, tag_filter  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--loops", type=int, default=300)
    a = ap.parse_args()
    n = a.rows
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((n, 64), dtype=np.float32)
    tags = (rng.integers(0, 16, size=n).astype(np.uint32) | (rng.integers(0, 50, size=n).astype(np.uint32) << np.uint32(8)))
    idx = HipIndex.build_from_flat(None, rows)
    idx.set_tags(tags)
    allows = np.ascontiguousarray(np.stack([tag_filter(sorted(int(v) for v in rng.choice(16, size=8, replace=False))) for _ in range(32)]))
    words = (n + 31) // 32
    out = np.zeros(32 * words, dtype=np.uint32)
    kept = np.zeros(32, dtype=np.uint64)
    want = [int(((allows[j][0] >> (tags & np.uint32(15))) & np.uint32(1)).sum()) for j in range(32)]
    for f in (8, 32):
        for _ in range(a.loops):
            rc = idx._lib.cqs_hip_debug_index_tag_keep_multi(idx._h, allows.ctypes.data_as(C.c_void_p), f, 0,
                                                             out.ctypes.data_as(C.c_void_p), kept.ctypes.data_as(C.c_void_p))
            assert rc == _lib.OK, idx.last_error()
        assert [int(x) for x in kept[:f]] == want[:f]
    for i in range(a.loops):
        assert idx.count_tagged(allows[i % 32]) == want[i % 32]
    idx.close()
    print("tags_multi_loop ok", n, a.loops)


if __name__ == "__main__":
    main()
