"""The planted corpus of the prefix-first tests (test_tail_prefix_first_cpu.py proves on the CPU which branch of the tail
kernel each query takes; test_tail_prefix_first_gpu.py runs them), and the branch a query takes from its scores.

20 000 Gaussian unit rows x 768 and four Gaussian unit queries, nearly orthogonal to each other, so what is planted for one
leaves the others' scores where they were:
  query 0  20 rows at cosine ~0.894, then a crowd of 150 at ~0.892: closer than the int8 copy's B_q (~0.01 here).  At k = 20 the
           prefix of 160 ends inside the crowd and fails; all 170 fit k' = 350, which certifies.              -> "slow"
  query 1  the same with a crowd of 400: the prefix fails, and so do all k': the f32 fallback answers.          -> "fallback"
  query 2  nothing planted: certifies on the prefix.                                                          -> "fast"
  query 3  a crowd of 60: the prefix passes the crowd and certifies.                                          -> "fast"
"""
import numpy as np

from cqs_amd import synth

N, DIM, K = 20_000, 768, 20
CROWDS = (150, 400, 0, 60)
WANT = ("slow", "fallback", "fast", "fast")


def planted():
    rows = synth.gaussian_unit(N, dim=DIM, seed=9801)
    q = synth.gaussian_unit(4, dim=DIM, seed=9802)
    rng = np.random.default_rng(9803)
    pick = rng.choice(N, sum(20 + c for c in CROWDS if c), replace=False)
    at = 0
    for qi, crowd in enumerate(CROWDS):
        if not crowd:
            continue
        for j in range(20 + crowd):
            r = pick[at + j]
            w = 2.0 if j < 20 else 1.97 + 0.0001 * (j % 50)
            perp = rows[r] - np.dot(rows[r], q[qi]) * q[qi]
            v = q[qi] * w + perp
            rows[r] = (v / np.linalg.norm(v)).astype(np.float32)
        at += 20 + crowd
    return rows, q


def branch(approx, exact, bq, k, valid=None):
    """The tail's branch for one RAW query from its approximate scores (the scan's, one per row), its exact scores and B_q:
    "few" (no more than 6k + 40 valid rows: all rescored in tier 1), "fast" (the prefix certifies), "slow" (it does not, all
    k' = 10k + 150 do) or "fallback" (they do not either) - and the margin by which the deciding inequality holds or fails."""
    j1, kp = 6 * k + 40, 10 * k + 150
    idx = np.arange(len(approx)) if valid is None else np.flatnonzero(valid)
    order = idx[np.lexsort((idx, -approx[idx].astype(np.float64)))]      # approximate score descending, then row ascending
    if len(order) <= j1:
        return "few", np.inf
    s_k = np.sort(exact[order[:j1]])[::-1][k - 1]
    gap = float(s_k) - (float(approx[order[j1]]) + float(bq))
    if gap > 0:
        return "fast", gap
    if len(order) <= kp:
        return "slow", -gap
    s_k = np.sort(exact[order[:kp]])[::-1][k - 1]
    gap2 = float(s_k) - (float(approx[order[kp]]) + float(bq))
    return ("slow" if gap2 > 0 else "fallback"), min(-gap, abs(gap2))
