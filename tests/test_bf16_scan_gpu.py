"""The dense index's bf16 shadow scan (include/cqs_hip.h, cqs_hip_index_set_bf16_scan).

Every test compares a handle with the shadow on against the same rows in a handle without it (or the same handle before
enabling): identical rows, identical score BITS, identical counts.  The shadow only changes which bytes are read; the
certificate (or the f32 fallback) makes the answer the f32 scan's.  Run on an MI355X with `pytest -m gpu`."""
import threading

import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth
from cqs_amd.index import HipError
from parity import assert_topk_parity

pytestmark = pytest.mark.gpu
MARGIN = 64


def pair(rows, metric=DistanceMetric.Cosine):
    """(handle with the shadow on, handle without) over the same rows."""
    a = HipIndex.build_from_flat(None, rows, metric)
    a.set_bf16_scan(True)
    b = HipIndex.build_from_flat(None, rows, metric)
    return a, b


def assert_same(got, want, ctx=""):
    (ra, sa, ca), (rb, sb, cb) = got, want
    assert np.array_equal(ca, cb), (ctx, ca, cb)
    for i in range(len(ca)):
        c = int(ca[i])
        assert np.array_equal(ra[i, :c], rb[i, :c]), (ctx, i)
        assert np.array_equal(sa[i, :c].view(np.uint32), sb[i, :c].view(np.uint32)), (ctx, i)


def both(a, b, q, k, **kw):
    got, want = a.search_batch(q, k, **kw), b.search_batch(q, k, **kw)
    assert_same(got, want, (k, kw.get("mode", 0), kw.get("threshold", 0.0)))
    return got


def bf16_round(x):
    """f32 -> bf16 -> f32, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


CORPORA = [(n, d) for d in (128, 264, 768) for n in (1, 255, 257, 4097)] + \
          [(n, d) for d in (1024, 2048) for n in (1, 257, 4097)] + [(100_000, 768)]


@pytest.mark.parametrize("n,dim", CORPORA)
def test_unit_corpora_identical(hip, n, dim):
    rows = synth.gaussian_unit(n, dim=dim, seed=1000 + n + dim)
    qs = synth.gaussian_unit(8, dim=dim, seed=2000 + n + dim)
    a, b = pair(rows)
    by, _, _ = a.bf16_stats()
    assert by == n * dim * 2
    for k in (1, 20, 100, 500, 1000):
        if k == 1000 and n == 100_000:
            _, cert, fb = a.bf16_stats()
            assert cert > 0 and fb == 0, (cert, fb)
        for nb in (1, 2, 3, 5, 8):
            both(a, b, qs[:nb], k)
    _, cert, fb = a.bf16_stats()
    assert cert + fb == 5 * 19                       # every query of every block took the shadow path
    a.close(); b.close()


def test_against_the_oracle(hip, oracle):
    rows = synth.gaussian_unit(20_000, seed=31)
    qs = synth.gaussian_unit(3, seed=32)
    a, _ = pair(rows)
    for k in (20, 500):
        r, s, c = a.search_batch(qs, k)
        for i in range(len(qs)):
            ext_ids, ext_scores = oracle.index_search(rows, qs[i], k + MARGIN)
            assert_topk_parity(r[i, :c[i]], s[i, :c[i]], ext_ids, ext_scores, k)
    assert a.bf16_stats()[1] > 0
    a.close()


def test_dot_metric_unnormalised(hip):
    rng = np.random.default_rng(7)
    rows = (rng.standard_normal((4000, 768)) * rng.uniform(0.1, 30, (4000, 1))).astype(np.float32)
    qs = rng.standard_normal((5, 768)).astype(np.float32)
    a, b = pair(rows, DistanceMetric.DotProduct)
    for k in (1, 20, 100, 500):
        for nb in (1, 5):
            both(a, b, qs[:nb], k)
    a.close(); b.close()


def test_pipeline_mode_thresholds(hip):
    rows = synth.gaussian_unit(30_000, seed=41)
    qs = synth.gaussian_unit(4, seed=42)
    a, b = pair(rows)
    top = b.search_batch(qs[:1], 1)[1][0, 0]
    for thr in (0.0, 0.05, 0.1, float(top) * 0.9, float(top), 0.999, -0.5):
        for k in (1, 20, 500):
            for nb in (1, 4):
                both(a, b, qs[:nb], k, mode=_lib.MODE_PIPELINE, threshold=thr)
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["sparse", "dense", "all", "none"])
def test_keep_bitsets(hip, kind):
    n = 50_000
    rows = synth.gaussian_unit(n, seed=51)
    qs = synth.gaussian_unit(3, seed=52)
    rng = np.random.default_rng(53)
    keep = {"sparse": rng.random(n) < 0.01, "dense": rng.random(n) < 0.9,
            "all": np.ones(n, bool), "none": np.zeros(n, bool)}[kind]
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    for i in np.nonzero(keep)[0]:
        words[i // 32] |= np.uint32(1) << np.uint32(i % 32)
    a, b = pair(rows)
    for k in (1, 20, 500):
        for nb in (1, 3):
            got = both(a, b, qs[:nb], k, keep_bitset=words)
            if kind == "none":
                assert not got[2].any()
            else:
                assert all(keep[r] for i in range(nb) for r in got[0][i, :got[2][i]])
    a.close(); b.close()


def adversarial_corpus(rng, sign, npairs, lo, hi):
    """Rows whose components sit on bf16 half-ulp points (signs aligned to `sign`), in pairs: A rounds every component
    DOWN by half an ulp; its partner B moves one component just past the halfway point (rounds UP: +1 bf16 ulp) and
    another of the same magnitude 16 f32 ulps down (same bf16 value) - B is below A in f32 and above it in bf16."""
    dim = sign.shape[0]
    mag = rng.uniform(lo, hi, (npairs, dim)).astype(np.float32)
    m = (mag.view(np.uint32) >> 16) & ~np.uint32(1)                       # bf16 value with an even last bit
    kc, lc = 3, 500
    m[:, lc] = m[:, kc]
    a_rows = ((m << 16) | 0x8000).view(np.float32)                         # halfway: rounds down to m
    b_bits = (m << 16) | 0x8000
    b_bits[:, kc] = (m[:, kc] << 16) | 0x8001
    b_bits[:, lc] = (m[:, lc] << 16) | 0x7FF0
    b_rows = b_bits.view(np.float32)
    qd = (sign / 32).astype(np.float64)
    sa_, sb_ = (a_rows * sign).astype(np.float64) @ qd, (b_rows * sign).astype(np.float64) @ qd
    ta_, tb_ = bf16_round(a_rows * sign).astype(np.float64) @ qd, bf16_round(b_rows * sign).astype(np.float64) @ qd
    assert (sb_ < sa_).all() and (tb_ > ta_).all()                         # bf16 reverses every pair's order
    rows = np.concatenate([a_rows, b_rows]) * sign
    return np.ascontiguousarray(rows[rng.permutation(len(rows))], dtype=np.float32)


def test_adversarial_rounding(hip):
    """bf16 rounding reverses the order of near-equal f32 scores (pairs closer than B_q).  The answers must still be the
    f32 scan's, and the certificate must be exercised both ways: a small corpus where every row is rescored (certified)
    and a crowded one where the k-th and (k'+1)-th scores are closer than B_q (fallback)."""
    rng = np.random.default_rng(61)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    qs = [q_adv, -q_adv] + list(synth.gaussian_unit(6, seed=62))
    stats = []
    for npairs, lo, hi, ks in ((300, 2.0 ** -6, 2.0 ** -4, (1, 10, 50, 500)),        # 600 rows: k = 500 rescoring all
                               (1500, 2.0 ** -6, 2.0 ** -4, (1, 10, 50, 300)),
                               (1500, 2.0 ** -5, 1.05 * 2.0 ** -5, (1, 20, 100))):    # crowded scores
        rows = adversarial_corpus(rng, sign, npairs, lo, hi)
        sa, fb = pair(rows)
        for q in qs:
            for k in ks:
                both(sa, fb, q, k)
        both(sa, fb, np.stack(qs[:8]), 20)
        stats.append(sa.bf16_stats())
        sa.close(); fb.close()
    assert stats[0][1] > 0, stats                                          # certified
    assert stats[2][2] > 0, stats                                          # fell back
    assert sum(s[1] for s in stats) > 0 and sum(s[2] for s in stats) > 0


def test_heavy_ties_fall_back(hip):
    row = synth.gaussian_unit(1, seed=71)
    rows = np.repeat(row, 5000, axis=0)
    a, b = pair(rows)
    for k in (1, 20, 500):
        both(a, b, synth.gaussian_unit(1, seed=72)[0], k)
    assert a.bf16_stats()[2] > 0
    a.close(); b.close()


def test_crowded_threshold_bin_falls_back(hip):
    q = synth.gaussian_unit(1, seed=81)[0]
    rows = np.concatenate([np.repeat(2.0 * q[None, :], 3000, axis=0), synth.gaussian_unit(3000, seed=82)]).astype(np.float32)
    a, b = pair(rows, DistanceMetric.DotProduct)
    for k in (1, 20, 500):
        both(a, b, q, k, mode=_lib.MODE_PIPELINE, threshold=0.5)         # 3000 scores clamped to 1.0
    assert a.bf16_stats()[2] > 0
    a.close(); b.close()


def test_non_finite_rows_never_emitted(hip):
    rows = synth.gaussian_unit(3000, seed=91)
    q = synth.gaussian_unit(1, seed=92)[0]
    bad = [5, 77, 1000, 2999]
    for j, v in zip(bad, (np.nan, np.inf, -np.inf, np.nan)):
        rows[j] = q                                                        # would be the best rows if finite
        rows[j, 10] = v
    a, b = pair(rows)
    for k in (1, 20, 500):
        got = both(a, b, q, k)
        assert not set(bad) & set(got[0][0, :got[2][0]].tolist())
    a.close(); b.close()


def test_outlier_row_refuses_enable(hip):
    rows = synth.gaussian_unit(2000, seed=93)
    rows[17, 3] = np.float32(2.0 ** 64)
    q = synth.gaussian_unit(1, seed=94)[0]
    a = HipIndex.build_from_flat(None, rows)
    want = a.search_batch(q, 20)
    with pytest.raises(HipError) as e:
        a.set_bf16_scan(True)
    assert e.value.code == _lib.ERR_INVALID
    assert a.bf16_stats()[0] == 0
    assert_same(a.search_batch(q, 20), want)
    a.close()


def test_invalid_handles(hip):
    rows = synth.gaussian_unit(1000, seed=95)
    sh = HipIndex.build_sharded(None, rows, [0, 0])
    with pytest.raises(HipError) as e:
        sh.set_bf16_scan(True)
    assert e.value.code == _lib.ERR_INVALID
    sh.close()
    odd = np.ascontiguousarray(synth.gaussian_unit(1000, dim=100, seed=96))
    h = HipIndex.build_from_flat(None, odd)
    with pytest.raises(HipError) as e:
        h.set_bf16_scan(True)
    assert e.value.code == _lib.ERR_INVALID
    q = synth.gaussian_unit(1, dim=100, seed=97)[0]
    assert h.search_batch(q, 5)[2][0] == 5
    h.close()
    import torch
    d = torch.from_numpy(rows).cuda()
    bor = HipIndex.build_from_device(None, d.data_ptr(), 1000, 768, borrow=True, keepalive=d)
    with pytest.raises(HipError) as e:
        bor.set_bf16_scan(True)
    assert e.value.code == _lib.ERR_INVALID
    bor.close()


def test_extend_after_enable(hip):
    rows = synth.gaussian_unit(6000, seed=101)
    qs = synth.gaussian_unit(4, seed=102)
    a = HipIndex.build_from_flat(None, rows[:1000])
    a.set_bf16_scan(True)
    a.extend(None, rows[1000:3000])
    a.extend(None, rows[3000:])
    b = HipIndex.build_from_flat(None, rows)
    for k in (1, 20, 500):
        got = both(a, b, qs, k)
    assert (got[0] >= 3000).any()                                         # rows of the extensions are found
    assert a.bf16_stats()[0] >= 6000 * 768 * 2
    a.close(); b.close()


def test_save_load_enable(hip, tmp_path):
    rows = synth.gaussian_unit(5000, seed=111)
    qs = synth.gaussian_unit(3, seed=112)
    a, b = pair(rows)
    path = str(tmp_path / "idx.hipflat")
    a.save(path)
    c = HipIndex.load(path, 768, 5000)
    assert c.bf16_stats()[0] == 0                                         # not persisted
    c.set_bf16_scan(True)
    for k in (1, 20, 500):
        assert_same(c.search_batch(qs, k), b.search_batch(qs, k))
    assert c.bf16_stats()[1] > 0
    for h in (a, b, c):
        h.close()


def test_disable_reenable(hip):
    rows = synth.gaussian_unit(3000, seed=121)
    q = synth.gaussian_unit(1, seed=122)[0]
    a, b = pair(rows)
    assert a.bf16_stats()[0] == 3000 * 768 * 2
    a.set_bf16_scan(False)
    assert a.bf16_stats()[0] == 0
    both(a, b, q, 20)
    a.set_bf16_scan(True)
    assert a.bf16_stats()[0] == 3000 * 768 * 2
    both(a, b, q, 20)
    a.close(); b.close()


def test_concurrent_callers(hip):
    rows = synth.gaussian_unit(300_000, seed=131)
    qs = synth.gaussian_unit(64, seed=132)
    a, b = pair(rows)
    want = [b.search_batch(qs[i], 20) for i in range(len(qs))]
    p0, q0 = a.combine_stats()
    for n_threads in (8, 16):
        errs = []

        def work(t):
            try:
                for rep in range(6):
                    for i in range(t, len(qs), n_threads):
                        assert_same(a.search_batch(qs[i], 20), want[i], (t, rep, i))
            except BaseException as e:  # noqa: BLE001 - surfaced below
                errs.append((t, repr(e)))

        th = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
        [x.start() for x in th]
        [x.join() for x in th]
        assert not errs, errs
    p1, q1 = a.combine_stats()
    assert q1 - q0 == 2 * 6 * len(qs)
    assert (q1 - q0) > 1.5 * (p1 - p0), f"the queue did not combine: {q1 - q0} queries in {p1 - p0} passes"
    _, cert, fb = a.bf16_stats()
    assert cert > 0 and cert + fb == q1 - q0
    a.close(); b.close()


def test_full_size_1m(hip):
    """BASELINE configs[1] shape: 1M x 768 unit rows, 64 unit queries, k = 20 and k = 500, one query per call."""
    import torch
    n, dim = 1_000_000, 768
    g = torch.Generator(device="cuda"); g.manual_seed(20261)
    d_rows = torch.empty((n, dim), device="cuda", dtype=torch.float32)
    for lo in range(0, n, 1 << 18):
        hi = min(n, lo + (1 << 18))
        x = torch.randn((hi - lo, dim), generator=g, device="cuda"); x /= x.norm(dim=1, keepdim=True); d_rows[lo:hi] = x
    d_qs = torch.randn((64, dim), generator=g, device="cuda"); d_qs /= d_qs.norm(dim=1, keepdim=True)
    qs = d_qs.cpu().numpy()
    a = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=False)
    a.set_bf16_scan(True)
    b = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=False)
    del d_rows
    for k in (20, 500):
        for i in range(len(qs)):
            both(a, b, qs[i], k)
    _, cert, fb = a.bf16_stats()
    assert cert + fb == 128 and fb / 128 <= 0.01, (cert, fb)
    a.close(); b.close()
