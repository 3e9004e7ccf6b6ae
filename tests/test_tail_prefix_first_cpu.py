"""Which branch of the prefix-first tail each query of the planted corpus takes (tests/tail_first_cases.py), proved without
a device: the int8 copy's scores from the numpy emulation of its build and scan (tests/shadow_emul.py, bit for bit the
kernels': test_shadow_premises_gpu.py), the exact scores in f64, B_q = ||q|| R.  test_tail_prefix_first_gpu.py runs the same
corpus and reads the same branches off the device counters; this test keeps a change of the corpus, of k' or of the prefix
length from turning its slow-path cases into three runs of the fast path."""
import numpy as np

from shadow_emul import build_i8, r_and_norm, scan_i8
from tail_first_cases import DIM, K, WANT, branch, planted


def test_planted_queries_land_in_their_branches():
    rows, q = planted()
    codes, scale = build_i8(rows)
    r, _ = r_and_norm(None, rows, codes, scale, DIM)
    near = (codes.astype(np.float64) * scale.astype(np.float64)[:, None]) @ q.astype(np.float64).T     # [n, 4], rounding aside
    exact = rows.astype(np.float64) @ q.astype(np.float64).T
    for qi, want in enumerate(WANT):
        # the kernel's own bits for the 1000 rows nearest the top (k' + 1 = 351 of them matter; the rest are 0.05 further down)
        top = np.sort(np.argsort(-near[:, qi])[:1000])
        assert near[top, qi].min() < np.sort(near[:, qi])[::-1][400] - 0.01
        approx = scan_i8(codes[top], scale[top], q[qi])
        assert np.abs(approx - near[top, qi]).max() < 1e-5
        bq = float(np.linalg.norm(q[qi].astype(np.float64))) * r
        got = [branch(approx, exact[top, qi], b, K) for b in (bq, bq * (1 + 1e-6))]     # (the device's B_q: rounded up, 2^-40 slacks)
        assert got[0][0] == got[1][0] == want, (qi, want, got, bq)
        assert got[1][1] > 2e-4, (qi, got)                 # the deciding inequality is not near its edge: f32 rounding cannot move it
    # fewer valid rows than tier 1 asks for
    assert branch(near[:100, 0].astype(np.float32), exact[:100, 0], 0.01, K)[0] == "few"
    assert branch(near[:161, 0].astype(np.float32), exact[:161, 0], 0.01, K)[0] != "few"
