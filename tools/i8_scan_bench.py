#!/usr/bin/env python3
"""The int8 copy of the shadow against the bf16 copy and the f32 scan, through `search_device` on borrowed handles
(DESIGN.md §3.11).  Writes the JSON that profiles/i8_scan_bench.json keeps (its `needed_kprime` block comes from
tools/i8_kprime_measure.py).

  python tools/i8_scan_bench.py [--rows 1000000 10000000] [--iters 200] [--out FILE.json]

Per corpus size (bench.py's seeded Gaussian unit rows and queries): host-timed create without and with the int8 copy, and
for (b, k) shapes the milliseconds per search of three handles over the same rows - default policy (int8 where it serves),
CQS_HIP_SCAN_I8=0 (bf16 copy), both variables 0 (f32 scan) - timed with events around `iters` back-to-back searches, plus
whether the three returned identical bytes and what the int8 counters say."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1, 1), (1, 5), (1, 20), (1, 50), (1, 87), (1, 100), (2, 20), (3, 20), (4, 20), (8, 20)]


def make(HipIndex, d_rows, bf16, i8):
    for name, v in (("CQS_HIP_SCAN_BF16", bf16), ("CQS_HIP_SCAN_I8", i8)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = v
    n, dim = d_rows.shape
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=True, keepalive=d_rows)
    return h, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    from bench_legs.common import make_unit_rows
    from cqs_amd import HipIndex
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    res = {"tool": "i8_scan_bench", "iters": a.iters, "sizes": {}}
    warm = make_unit_rows(torch, 1024, a.dim, 1, dev)
    make(HipIndex, warm, "0", "0")[0].close()                      # runtime start-up stays out of the first timed create
    for n in a.rows:
        rows = make_unit_rows(torch, n, a.dim, 0xC950001, dev)
        qs = make_unit_rows(torch, 8 * 32, a.dim, 0xC950002, dev).view(32, 8, a.dim)
        h_f32, t_f32 = make(HipIndex, rows, "0", "0")
        h_bf, t_bf = make(HipIndex, rows, None, "0")
        h_i8, t_i8 = make(HipIndex, rows, None, None)
        size = {"rows": n, "bf16_bytes": h_bf.bf16_stats()[0], "i8_bytes": h_i8.i8_stats()[0],
                "create_s": {"f32_only": round(t_f32, 4), "bf16": round(t_bf, 4), "bf16_and_i8": round(t_i8, 4)}, "shapes": {}}
        for b, k in SHAPES:
            out = {}
            keys = {}
            for name, h in (("i8", h_i8), ("bf16", h_bf), ("f32", h_f32)):
                ok = torch.zeros((32, b, k), dtype=torch.int64, device=dev)
                oc = torch.zeros((32, b), dtype=torch.int32, device=dev)
                def run(i):
                    h.search_device(qs[i % 32, :b].data_ptr(), b, k, ok[i % 32].data_ptr(), oc[i % 32].data_ptr(), stream=st.cuda_stream)
                for i in range(32):
                    run(i)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                iters = a.iters if n <= 2_000_000 else max(20, a.iters // 5)
                e0.record(st)
                for i in range(iters):
                    run(i)
                e1.record(st)
                torch.cuda.synchronize()
                out[name + "_ms"] = round(e0.elapsed_time(e1) / iters, 5)
                keys[name] = (ok.cpu(), oc.cpu())
            out["byte_equal"] = all(bool((keys[x][0] == keys["f32"][0]).all() and (keys[x][1] == keys["f32"][1]).all()) for x in ("i8", "bf16"))
            size["shapes"]["b%d_k%d" % (b, k)] = out
            print(n, b, k, json.dumps(out), flush=True)
        size["i8_stats"] = list(h_i8.i8_stats())
        size["bf16_stats_of_default_handle"] = list(h_i8.bf16_stats())
        res["sizes"][str(n)] = size
        for h in (h_f32, h_bf, h_i8):
            h.close()
        del rows
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
