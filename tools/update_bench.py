#!/usr/bin/env python3
"""`cqs_hip_index_update` against what followed such a write before it existed.

  python tools/update_bench.py [--rows 1000000] [--dim 768] [--update 1000,10000] [--reps 10] [--rebuild-reps 3] [--out FILE.json]
  CQS_HIP_LIB=/path/to/parent/libcqs_hip.so python tools/update_bench.py      # the comparison legs on the parent commit's library

One index of `--rows` x `--dim` with the bf16 and int8 shadow copies on (CQS_HIP_SCAN_BF16=1, CQS_HIP_SCAN_I8=1), and per
size of `--update` a seeded random set of rows with new vectors, host-timed around the blocking calls:
  update         `cqs_hip_index_update` of those rows (skipped, and said so, when the library has no such symbol)
  remove_extend  `cqs_hip_index_remove` of the rows + `cqs_hip_index_extend` by their new vectors: what a caller had to do
                 before (it also renumbers every survivor; the caller's id_map / tags / bitsets rebuild is NOT timed)
  rebuild        `cqs_hip_index_create` of the patched array from host memory (no store read: this flatters the rebuild)
The library is driven through ctypes directly, so the same file runs against this tree's build and, with CQS_HIP_LIB,
against the parent commit's.  One untimed warm-up per shape; median, minimum and maximum of the repeats.  `payload_bytes`
is what the update must write: the rows' f32, bf16 and int8 bytes and scales; it also crosses PCIe once as f32."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def load_library():
    path = os.environ.get("CQS_HIP_LIB") or os.path.join(ROOT, "cqs_amd", "libcqs_hip.so")
    lib = C.CDLL(path)
    p, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32
    lib.cqs_hip_index_create.restype = i32
    lib.cqs_hip_index_create.argtypes = [p, u64, u32, u32, i32, u64, C.POINTER(p)]
    lib.cqs_hip_index_remove.restype = i32
    lib.cqs_hip_index_remove.argtypes = [p, p, u64, C.POINTER(u64)]
    lib.cqs_hip_index_extend.restype = i32
    lib.cqs_hip_index_extend.argtypes = [p, p, u64]
    lib.cqs_hip_index_destroy.restype = None
    lib.cqs_hip_index_destroy.argtypes = [p]
    lib.cqs_hip_index_len.restype = u64
    lib.cqs_hip_index_len.argtypes = [p]
    for name in ("cqs_hip_index_bf16_stats", "cqs_hip_index_i8_stats"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [p, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    has_update = hasattr(lib, "cqs_hip_index_update")
    if has_update:
        lib.cqs_hip_index_update.restype = i32
        lib.cqs_hip_index_update.argtypes = [p, p, p, u64, C.POINTER(u64)]
    return lib, path, has_update


def create(lib, flat):
    h = C.c_void_p()
    rc = lib.cqs_hip_index_create(flat.ctypes.data, flat.shape[0], flat.shape[1], 0, 0, 0, C.byref(h))   # (metric 0: cosine)
    if rc != 0:
        raise SystemExit(f"cqs_hip_index_create failed: {rc}")
    return h


def copy_bytes(lib, h):
    out = []
    for name in ("cqs_hip_index_bf16_stats", "cqs_hip_index_i8_stats"):
        b, c, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
        getattr(lib, name)(h, C.byref(b), C.byref(c), C.byref(f))
        out.append(int(b.value))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--update", type=str, default="1000,10000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_legs.common import make_unit_rows
    if not torch.cuda.is_available():
        raise SystemExit("update_bench needs a GPU: nothing here is measured without one")
    os.environ["CQS_HIP_SCAN_BF16"] = "1"
    os.environ["CQS_HIP_SCAN_I8"] = "1"
    lib, path, has_update = load_library()
    n, dim = a.rows, a.dim
    sizes = [int(s) for s in a.update.split(",") if s]
    flat = make_unit_rows(torch, n, dim, 0xC950011, torch.device("cuda")).cpu().numpy()
    fresh = make_unit_rows(torch, max(sizes), dim, 0xC950012, torch.device("cuda")).cpu().numpy()
    rng = np.random.default_rng(0xC950013)
    res = {"tool": "update_bench", "library": path, "rows": n, "dim": dim, "sizes": {}}
    if not has_update:
        print("this library has no cqs_hip_index_update: the comparison legs alone", flush=True)
    for m in sizes:
        rows = rng.choice(n, size=m, replace=False).astype(np.uint64)      # unsorted, as a caller's batch is
        vec = np.ascontiguousarray(fresh[:m])
        out = {}
        h = create(lib, flat)
        bf16_bytes, i8_bytes = copy_bytes(lib, h)
        row_bytes = dim * 4 + (dim * 2 if bf16_bytes else 0) + (dim + 4 if i8_bytes else 0)
        out.update(bf16_bytes=bf16_bytes, i8_bytes=i8_bytes, payload_bytes=m * row_bytes)
        if has_update:
            ms, done = [], C.c_uint64()
            for rep in range(a.reps + 1):                                   # the first one warms the kernel and the staging pair
                t0 = time.perf_counter()
                rc = lib.cqs_hip_index_update(h, rows.ctypes.data, vec.ctypes.data, m, C.byref(done))
                t1 = time.perf_counter()
                assert rc == 0 and done.value == m, rc
                if rep:
                    ms.append((t1 - t0) * 1e3)
            out["update"] = spread(ms)
            out["update"]["rows_per_s"] = round(m / (out["update"]["median_ms"] * 1e-3))
            print(m, "update", json.dumps(out["update"]), flush=True)
        ms, gone = [], C.c_uint64()
        for rep in range(a.reps + 1):
            # the same m row NUMBERS every repeat (after the first, some are rows an earlier repeat appended: the cost is
            # the compaction behind the first removed row and the append, which do not depend on which chunk a row holds)
            t0 = time.perf_counter()
            rc = lib.cqs_hip_index_remove(h, rows.ctypes.data, m, C.byref(gone))
            rc2 = lib.cqs_hip_index_extend(h, vec.ctypes.data, m) if rc == 0 else -1
            t1 = time.perf_counter()
            assert rc == 0 and rc2 == 0 and gone.value == m and lib.cqs_hip_index_len(h) == n, (rc, rc2)
            if rep:
                ms.append((t1 - t0) * 1e3)
        out["remove_extend"] = spread(ms)
        print(m, "remove_extend", json.dumps(out["remove_extend"]), flush=True)
        lib.cqs_hip_index_destroy(h)
        patched = flat.copy()
        patched[rows.astype(np.int64)] = vec
        ms = []
        for rep in range(a.rebuild_reps + 1):
            t0 = time.perf_counter()
            f = create(lib, patched)
            t1 = time.perf_counter()
            lib.cqs_hip_index_destroy(f)
            if rep:
                ms.append((t1 - t0) * 1e3)
        del patched
        out["rebuild"] = spread(ms)
        print(m, "rebuild", json.dumps(out["rebuild"]), flush=True)
        res["sizes"][str(m)] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
