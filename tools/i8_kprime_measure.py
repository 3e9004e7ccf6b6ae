#!/usr/bin/env python3
"""Smallest k' at which the int8 copy's certificate closes, per query (cqs_amd/csrc/scan_i8.h, i8_kprime).

  python tools/i8_kprime_measure.py [--rows 1000000 10000000] [--out FILE.json]

The bench's seeded corpus distribution (bench_legs.common.make_unit_rows: Gaussian unit rows; seed 0xC950001 at 1M rows is
bench.py's own corpus) and its 330 seeded queries (0xC950002).  The corpus is quantised as i8_build_kernel does (scale =
max|x_i| / 127 in f32, round to nearest even, clamp), R_8 = max ||x - x~|| + gamma' (||x|| + ||x~||) in f64, B_q = ||q|| R_8,
and for each k the needed k' of a query is the smallest k' with  s~_(k'+1) + B_q < s_(k)  (the certificate's rule (b), rescore_certify_kernel).
Scores come from torch's f32 matmul, not the scan kernels: they differ from the kernels' by ~1e-7, against B_q ~ 1.3e-2.
Prints one JSON object: per (rows, k) the median / p99 / max needed k' over the queries."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 5, 20, 50, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=330)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    import torch
    from bench_legs.common import make_unit_rows
    dev = torch.device("cuda")
    q = make_unit_rows(torch, a.queries, a.dim, 0xC950002, dev)
    gamma = (a.dim + 2) * 2.0 ** -24 / (1 - (a.dim + 2) * 2.0 ** -24)
    res = {}
    for n in a.rows:
        rows = make_unit_rows(torch, n, a.dim, 0xC950001, dev)
        S = torch.empty((n, a.queries), dtype=torch.float32, device=dev)
        St = torch.empty((n, a.queries), dtype=torch.float32, device=dev)
        r8 = 0.0
        for lo in range(0, n, 1 << 18):
            x = rows[lo:lo + (1 << 18)]
            sc = x.abs().amax(dim=1, keepdim=True) / 127.0
            xt = torch.round(x / sc).clamp(-127, 127) * sc
            xd, td = x.double(), xt.double()
            r8 = max(r8, float(((xd - td).norm(dim=1) + gamma * (xd.norm(dim=1) + td.norm(dim=1))).max()))
            S[lo:lo + (1 << 18)] = x @ q.T
            St[lo:lo + (1 << 18)] = xt @ q.T
        del rows
        bq = r8 * q.double().norm(dim=1).float()                      # [queries]
        top_t = torch.cat([torch.topk(St[:, i:i + 33].T.contiguous(), 1024, dim=1).values.T for i in range(0, a.queries, 33)], dim=1)
        top_e = torch.cat([torch.topk(S[:, i:i + 33].T.contiguous(), max(KS), dim=1).values.T for i in range(0, a.queries, 33)], dim=1)
        del S, St
        res[str(n)] = {"r8": r8}
        for k in KS:
            ok = (top_t + bq[None, :]) < top_e[k - 1][None, :]       # [1024, queries]: index = k'
            need = torch.where(ok.any(0), ok.float().argmax(0), torch.tensor(9999, device=dev)).clamp(min=k)
            s = need.sort().values.cpu().tolist()
            res[str(n)][str(k)] = {"median": s[len(s) // 2], "p99": s[int(0.99 * len(s))], "max": s[-1]}
        print(n, json.dumps(res[str(n)]), flush=True)
    line = json.dumps({"what": "needed k' of the int8 certificate, %d seeded unit queries, dim %d" % (a.queries, a.dim), "rows": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
