"""The int8 copy of the dense index's shadow (include/cqs_hip.h, cqs_hip_index_i8_stats).

Every test compares a handle that has the int8 copy (CQS_HIP_SCAN_I8=1 CQS_HIP_SCAN_BF16=1 at create) against a handle over
the same rows made with both variables 0: identical keys (rows and score BITS) and identical counts, through
`search_device` and through the host searches.  The int8 copy only changes which bytes are read; the certificate (or the
f32 fallback) makes the answer the f32 scan's.  Run on an MI355X with `pytest -m gpu`."""
import threading

import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth

pytestmark = pytest.mark.gpu
ENV_BF16, ENV_I8 = "CQS_HIP_SCAN_BF16", "CQS_HIP_SCAN_I8"
I8_MAX_Q = 4                      # scan_i8.h: kI8MaxQ
K_SWITCH = 87                     # largest k with i8_kprime(k) = 10k + 150 <= 1023


@pytest.fixture
def torch():
    import torch as t
    return t


def setenv(monkeypatch, bf16, i8):
    for name, v in ((ENV_BF16, bf16), (ENV_I8, i8)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def i8_bytes(n, dim):
    return n * dim + n * 4


def owned_pair(monkeypatch, rows, metric=DistanceMetric.Cosine):
    """(owned handle with both copies, owned handle on f32 alone) over the same rows."""
    setenv(monkeypatch, "1", "1")
    a = HipIndex.build_from_flat(None, rows, metric)
    setenv(monkeypatch, "0", "0")
    b = HipIndex.build_from_flat(None, rows, metric)
    setenv(monkeypatch, None, None)
    n, dim = rows.shape
    assert a.bf16_stats()[0] == n * dim * 2 and a.i8_stats()[0] == i8_bytes(n, dim), a.last_error()
    assert b.bf16_stats()[0] == 0 and b.i8_stats()[0] == 0
    return a, b


def dev_pair(monkeypatch, torch, rows, metric=DistanceMetric.Cosine):
    """The same as borrowed handles over one device buffer."""
    d = rows if hasattr(rows, "data_ptr") else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    n, dim = d.shape
    setenv(monkeypatch, "1", "1")
    a = HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d)
    setenv(monkeypatch, "0", "0")
    b = HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d)
    setenv(monkeypatch, None, None)
    assert a.bf16_stats()[0] == n * dim * 2 and a.i8_stats()[0] == i8_bytes(n, dim), a.last_error()
    assert b.bf16_stats()[0] == 0 and b.i8_stats()[0] == 0
    return a, b


def dev_search(torch, h, d_q, k, d_keep=None, mode=_lib.MODE_RAW, threshold=0.0, stream=None):
    b = d_q.shape[0]
    keys = torch.full((b, k), -1, dtype=torch.int64, device="cuda")   # every slot must be written
    counts = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    st = stream if stream is not None else torch.cuda.current_stream()
    h.search_device(d_q.data_ptr(), b, k, keys.data_ptr(), counts.data_ptr(), d_keep=d_keep.data_ptr() if d_keep is not None else 0,
                    mode=mode, threshold=threshold, stream=st.cuda_stream)
    return keys, counts


def assert_same_dev(torch, a, b, d_q, k, ctx="", **kw):
    ka, ca = dev_search(torch, a, d_q, k, **kw)
    kb, cb = dev_search(torch, b, d_q, k, **kw)
    torch.cuda.synchronize()
    ka, ca, kb, cb = ka.cpu().numpy(), ca.cpu().numpy(), kb.cpu().numpy(), cb.cpu().numpy()
    assert np.array_equal(ca, cb), (ctx, k, ca, cb)
    assert np.array_equal(ka, kb), (ctx, k)
    return ka, ca


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


def served(h):
    """Queries the int8 copy served so far (certified + fallbacks)."""
    return sum(h.i8_stats()[1:])


# dims with a partial last chunk (128, 272, 768, 1040), a full one (1024, 2048); n around the task and tier edges
CORPORA = [(n, d) for d in (128, 272, 768) for n in (1, 255, 257, 4097)] + \
          [(n, d) for d in (16, 1024, 1040, 2048) for n in (1, 257, 4097)] + [(100_000, 768)]
KS = (1, 20, K_SWITCH, K_SWITCH + 1, 100, 500, 1000)   # both sides of the int8 / bf16 switch


@pytest.mark.parametrize("n,dim", CORPORA)
def test_device_path_identical(hip, monkeypatch, torch, n, dim):
    rows = synth.gaussian_unit(n, dim=dim, seed=5000 + n + dim)
    d_q = torch.from_numpy(synth.gaussian_unit(8, dim=dim, seed=6000 + n + dim)).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    want_i8 = 0
    for k in KS:
        for nb in range(1, 9):
            assert_same_dev(torch, a, b, d_q[:nb], k, (n, dim, nb))
            want_i8 += nb if (nb <= I8_MAX_Q and k <= K_SWITCH) else 0
    _, cert, fb = a.bf16_stats()
    assert cert + fb == len(KS) * 36                  # every query of every block took the shadow, counted once
    assert served(a) == want_i8                       # and the int8 copy served the blocks of <= 4 queries at k <= 87
    if n == 100_000:
        assert a.i8_stats()[1] > 0
    assert b.bf16_stats()[1:] == (0, 0) and b.i8_stats()[1:] == (0, 0)
    a.close(); b.close()


@pytest.mark.parametrize("n,dim", [(1, 128), (257, 768), (4097, 272), (4097, 2048), (100_000, 768)])
def test_host_path_identical(hip, monkeypatch, n, dim):
    rows = synth.gaussian_unit(n, dim=dim, seed=5100 + n + dim)
    qs = synth.gaussian_unit(8, dim=dim, seed=6100 + n + dim)
    a, b = owned_pair(monkeypatch, rows)
    want_i8 = 0
    for k in KS:
        for nb in range(1, 9):
            both(a, b, qs[:nb], k)
            want_i8 += nb if (nb <= I8_MAX_Q and k <= K_SWITCH) else 0
    assert served(a) == want_i8
    assert sum(a.bf16_stats()[1:]) == len(KS) * 36
    a.close(); b.close()


def test_dot_metric_and_pipeline(hip, monkeypatch, torch):
    rng = np.random.default_rng(27)
    rows = (rng.standard_normal((6000, 768)) * rng.uniform(0.1, 30, (6000, 1))).astype(np.float32)
    qs = rng.standard_normal((4, 768)).astype(np.float32)
    d_q = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows, DistanceMetric.DotProduct)
    for k in (1, 20, 80):
        for nb in (1, 2, 3, 4):
            assert_same_dev(torch, a, b, d_q[:nb], k)
    a.close(); b.close()
    a, b = owned_pair(monkeypatch, rows, DistanceMetric.DotProduct)
    for k in (1, 20, 80):
        both(a, b, qs, k)
    a.close(); b.close()
    rows = synth.gaussian_unit(30_000, seed=28)
    qs = synth.gaussian_unit(4, seed=29)
    d_q = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    top = float(b.search_batch(qs[:1], 1)[1][0, 0])
    for thr in (0.0, 0.05, 0.1, top * 0.9, top, 0.999, -0.5):
        for k in (1, 20, 80):
            for nb in (1, 4):
                assert_same_dev(torch, a, b, d_q[:nb], k, thr, mode=_lib.MODE_PIPELINE, threshold=thr)
                both(a, b, qs[:nb], k, mode=_lib.MODE_PIPELINE, threshold=thr)
    assert served(a) > 0
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["sparse", "dense", "all", "none"])
def test_keep_bitsets(hip, monkeypatch, torch, kind):
    n = 50_000
    rows = synth.gaussian_unit(n, seed=31)
    qs = synth.gaussian_unit(3, seed=32)
    d_q = torch.from_numpy(qs).cuda()
    rng = np.random.default_rng(33)
    keep = {"sparse": rng.random(n) < 0.01, "dense": rng.random(n) < 0.9,
            "all": np.ones(n, bool), "none": np.zeros(n, bool)}[kind]
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    idx = np.nonzero(keep)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    d_keep = torch.from_numpy(words.view(np.int32)).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 20, 80, 500):
        for nb in (1, 3):
            ka, ca = assert_same_dev(torch, a, b, d_q[:nb], k, kind, d_keep=d_keep)
            rows_out = (0xFFFFFFFF - (ka.astype(np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)
            for i in range(nb):
                assert keep[rows_out[i, :ca[i]]].all()
            both(a, b, qs[:nb], k, keep_bitset=words)
    a.close(); b.close()


def test_ties_fall_back_or_certify_exactly(hip, monkeypatch, torch):
    """Many identical rows: more candidates tie at the cut than any k' holds, so the certificate cannot close and the f32
    scan answers; the stats say so."""
    base = synth.gaussian_unit(300, seed=41)
    rows = np.ascontiguousarray(np.repeat(base, 20, axis=0))      # 6000 rows, every row 20 times
    qs = synth.gaussian_unit(2, seed=42)
    a, b = dev_pair(monkeypatch, torch, rows)
    d_q = torch.from_numpy(qs).cuda()
    for k in (1, 20, 80):
        assert_same_dev(torch, a, b, d_q[:1], k)
        assert_same_dev(torch, a, b, d_q, k)
    assert served(a) == 9
    a.close(); b.close()
    a, b = owned_pair(monkeypatch, rows)
    for k in (1, 20, 80):
        both(a, b, qs, k)
    a.close(); b.close()


def test_int8_order_reversed_still_f32_answer(hip, monkeypatch, torch):
    """Pairs of rows (A, B) that differ by a hundredth of a quantisation step in two components, built so that the f32 scan
    scores A above B and the int8 scan B above A (B crosses a rounding midpoint in a component the query weighs half as much
    as the one where it loses).  Pair 0 is the clear top two, so k = 1 cuts between its rows: the answer must be the f32
    one, by certificate or by fallback, and the int8 counters account for every query."""
    dim, npairs = 768, 2000
    q = synth.gaussian_unit(1, seed=44)[0]
    base = synth.gaussian_unit(npairs, seed=45)
    base[0] = q + np.float32(0.5) * base[0]
    base[0] /= np.linalg.norm(base[0])
    rows = np.empty((2 * npairs, dim), np.float32)
    aq = np.abs(q)
    for p in range(npairs):
        x = base[p].copy()
        top = int(np.argmax(np.abs(x)))
        s = np.float32(np.abs(x[top]) / np.float32(127))
        w = aq.copy(); w[top] = 0
        j = int(np.argmax(w))
        w[j] = 0; w[top] = np.inf
        i = int(np.argmin(np.abs(w - aq[j] / 2)))
        cj = np.clip(np.rint(x[j] / s), -100, 100)
        ci = np.clip(np.rint(x[i] / s), -100, 100)
        sj, si = np.sign(q[j]), np.sign(q[i])
        a_row, b_row = x.copy(), x.copy()
        a_row[j] = np.float32(cj * s)
        a_row[i] = np.float32((ci + si * 0.495) * s)          # code ci
        b_row[j] = np.float32((cj - sj * 0.01) * s)           # f32 score: - 0.01 s |q_j|; code still cj
        b_row[i] = np.float32((ci + si * 0.505) * s)          # f32 score: + 0.01 s |q_i| = half of that; code ci + si
        rows[2 * p], rows[2 * p + 1] = a_row, b_row
    exact = rows.astype(np.float64) @ q.astype(np.float64)
    assert (exact[0::2] > exact[1::2]).all()                   # f32 order: A above B in every pair
    assert exact[:2].min() > exact[2:].max() + 0.1             # pair 0 is the top two
    a, b = dev_pair(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q[None]).cuda()
    for k in (1, 2, 3, 20, 80):
        ka, _ = assert_same_dev(torch, a, b, d_q, k)
        assert 0xFFFFFFFF - (int(ka[0, 0]) & 0xFFFFFFFF) == 0  # row A of pair 0
    c8, f8 = a.i8_stats()[1:]
    assert c8 + f8 == 5, (c8, f8)
    a.close(); b.close()
    a, b = owned_pair(monkeypatch, rows)
    for k in (1, 2, 3, 20, 80):
        assert both(a, b, q, k)[0][0, 0] == 0
    assert served(a) == 5
    a.close(); b.close()


def test_adversarial_rows(hip, monkeypatch, torch):
    """Rows at rounding midpoints, one dominant component, tiny and huge scales, a zero row, denormal rows."""
    rng = np.random.default_rng(47)
    dim = 768
    rows = synth.gaussian_unit(4000, seed=48)
    rows[10] = 0.0
    rows[11] = np.float32(1e-41)                                       # denormal row: scale underflows to 0
    rows[12] = 0.0; rows[12, 5] = 1.0                                  # one dominant component
    rows[13] = (rng.integers(-126, 127, dim) + 0.5).astype(np.float32) / np.float32(127 * 30)   # every component at a midpoint
    rows[13, 0] = np.float32(1.0 / 30)
    rows[14] = rows[14] * np.float32(1e-30)
    rows[15] = rows[15] * np.float32(1e15)
    rows[16] = rows[16] * np.float32(-1e15)
    qs = synth.gaussian_unit(3, seed=49)
    a, b = dev_pair(monkeypatch, torch, rows, DistanceMetric.DotProduct)
    d_q = torch.from_numpy(qs).cuda()
    for k in (1, 20, 80):
        for nb in (1, 3):
            assert_same_dev(torch, a, b, d_q[:nb], k)
    a.close(); b.close()
    a, b = owned_pair(monkeypatch, rows, DistanceMetric.DotProduct)
    for k in (1, 20, 80):
        both(a, b, qs, k)
    a.close(); b.close()


def test_non_finite_rows_and_queries(hip, monkeypatch, torch):
    rows = synth.gaussian_unit(3000, seed=51)
    q = synth.gaussian_unit(1, seed=52)[0]
    bad = [5, 77, 1000, 2999]
    for j, v in zip(bad, (np.nan, np.inf, -np.inf, np.nan)):
        rows[j] = q                                                        # would be the best rows if finite
        rows[j, 10] = v
    a, b = owned_pair(monkeypatch, rows)
    for k in (1, 20, 80):
        got = both(a, b, q, k)
        assert not set(bad) & set(got[0][0, :got[2][0]].tolist())
    qn = np.stack([q, q, q]); qn[1, 3] = np.nan                            # host: a non-finite query answers empty
    got = both(a, b, qn, 20)
    assert got[2].tolist() == [20, 0, 20]
    a.close(); b.close()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 20, 80):
        ka, ca = assert_same_dev(torch, a, b, torch.from_numpy(q[None]).cuda(), k)
        out = (0xFFFFFFFF - (ka.astype(np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)
        assert not set(bad) & set(out[0, :ca[0]].tolist())
    s0 = a.i8_stats()
    assert_same_dev(torch, a, b, torch.from_numpy(qn).cuda(), 20)          # device: the NaN query is never certified
    s1 = a.i8_stats()
    assert s1[1] + s1[2] - s0[1] - s0[2] == 3 and s1[2] - s0[2] >= 1
    a.close(); b.close()


def test_extend_save_load_and_free(hip, monkeypatch, tmp_path):
    rows = synth.gaussian_unit(6000, seed=61)
    qs = synth.gaussian_unit(4, seed=62)
    setenv(monkeypatch, "1", "1")
    a = HipIndex.build_from_flat(None, rows[:1000])
    assert a.i8_stats()[0] == i8_bytes(1000, 768)
    a.extend(None, rows[1000:3000])
    a.extend(None, rows[3000:])
    setenv(monkeypatch, "0", "0")
    b = HipIndex.build_from_flat(None, rows)
    for k in (1, 20, 80):
        got = both(a, b, qs, k)
    assert (got[0] >= 3000).any()                                         # rows of the extensions are found
    assert a.i8_stats()[0] >= i8_bytes(6000, 768) and served(a) == 12
    path = str(tmp_path / "idx.hipflat")
    a.save(path)
    c = HipIndex.load(path, 768, 6000)                                    # both variables 0: nothing is rebuilt
    assert c.bf16_stats()[0] == 0 and c.i8_stats()[0] == 0
    setenv(monkeypatch, "1", "1")
    d = HipIndex.load(path, 768, 6000)                                    # not persisted: rebuilt by the policy at load
    assert d.bf16_stats()[0] == 6000 * 768 * 2 and d.i8_stats()[0] == i8_bytes(6000, 768)
    c.set_bf16_scan(True)                                                 # set_bf16_scan(1) follows CQS_HIP_SCAN_I8 too
    assert c.i8_stats()[0] == i8_bytes(6000, 768)
    setenv(monkeypatch, "1", "0")
    e = HipIndex.load(path, 768, 6000)                                    # CQS_HIP_SCAN_I8=0: the bf16 copy alone
    assert e.bf16_stats()[0] == 6000 * 768 * 2 and e.i8_stats()[0] == 0
    setenv(monkeypatch, "1", None)
    f = HipIndex.load(path, 768, 6000)                                    # unset: below 1 GiB the bf16 copy alone
    assert f.bf16_stats()[0] == 6000 * 768 * 2 and f.i8_stats()[0] == 0
    setenv(monkeypatch, None, None)
    for h in (c, d, e, f):
        for k in (1, 20, 80):
            assert_same(h.search_batch(qs, k), b.search_batch(qs, k))
    assert served(c) == 12 and served(d) == 12 and served(e) == 0 and served(f) == 0
    before = d.i8_stats()
    d.set_bf16_scan(False)                                                # frees both copies; the counts stay
    assert d.bf16_stats()[0] == 0 and d.i8_stats() == (0,) + before[1:]
    assert_same(d.search_batch(qs, 20), b.search_batch(qs, 20))
    assert d.i8_stats() == (0,) + before[1:]
    for h in (a, b, c, d, e, f):
        h.close()


def test_dim_rule(hip, monkeypatch):
    """dim % 8 == 0 but % 16 != 0: the bf16 copy alone, and last_error says why."""
    rows = synth.gaussian_unit(2000, dim=264, seed=71)
    q = synth.gaussian_unit(1, dim=264, seed=72)[0]
    setenv(monkeypatch, "1", "1")
    a = HipIndex.build_from_flat(None, rows)
    setenv(monkeypatch, "0", "0")
    b = HipIndex.build_from_flat(None, rows)
    setenv(monkeypatch, None, None)
    assert a.bf16_stats()[0] == 2000 * 264 * 2 and a.i8_stats()[0] == 0
    assert "multiple of 16" in a.last_error()
    both(a, b, q, 20)
    assert served(a) == 0 and sum(a.bf16_stats()[1:]) == 1
    a.close(); b.close()


def test_concurrent_callers(hip, monkeypatch):
    rows = synth.gaussian_unit(300_000, seed=81)
    qs = synth.gaussian_unit(64, seed=82)
    a, b = owned_pair(monkeypatch, rows)
    want = [b.search_batch(qs[i], 20) for i in range(len(qs))]
    q0 = a.combine_stats()[1]
    for n_threads in (3, 16):
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
    q1 = a.combine_stats()[1]
    assert q1 - q0 == 2 * 6 * len(qs)
    _, cert, fb = a.bf16_stats()
    assert cert > 0 and cert + fb == q1 - q0          # every query counted once, whichever copy its block scanned
    assert 0 < served(a) <= cert + fb                 # blocks of <= 4 callers scanned the int8 copy
    a.close(); b.close()


def test_side_stream_interleaved_with_host(hip, monkeypatch, torch):
    rows = synth.gaussian_unit(40_000, seed=91)
    qs = synth.gaussian_unit(6, seed=92)
    d_q = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for i in range(6):
        with torch.cuda.stream(side):
            ka, ca = dev_search(torch, a, d_q[i:i + 1], 20, stream=side)
        got = a.search_batch(qs[(i + 1) % 6], 20)
        side.synchronize()
        kb, cb = dev_search(torch, b, d_q[i:i + 1], 20)
        torch.cuda.synchronize()
        assert np.array_equal(ka.cpu().numpy(), kb.cpu().numpy()) and np.array_equal(ca.cpu().numpy(), cb.cpu().numpy())
        assert_same(got, b.search_batch(qs[(i + 1) % 6], 20))
    assert served(a) == 12
    a.close(); b.close()


def _gaussian_unit_device(torch, n, dim, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    d_rows = torch.empty((n, dim), device="cuda", dtype=torch.float32)
    for lo in range(0, n, 1 << 18):
        hi = min(n, lo + (1 << 18))
        x = torch.randn((hi - lo, dim), generator=g, device="cuda"); x /= x.norm(dim=1, keepdim=True); d_rows[lo:hi] = x
    d_qs = torch.randn((32, dim), generator=g, device="cuda"); d_qs /= d_qs.norm(dim=1, keepdim=True)
    return d_rows, d_qs


def test_bench_shape_1m_default_policy(hip, monkeypatch, torch):
    """1M x 768 f32, default environment: a borrowed handle has both copies, and 32 seeded unit queries at k = 20 are all
    served by the int8 copy with no fallback, bit for bit the f32 handle's answers."""
    n, dim = 1_000_000, 768
    d_rows, d_qs = _gaussian_unit_device(torch, n, dim, 20263)
    setenv(monkeypatch, None, None)
    a = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=True, keepalive=d_rows)
    setenv(monkeypatch, "0", "0")
    b = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=True, keepalive=d_rows)
    setenv(monkeypatch, None, None)
    assert a.bf16_stats()[0] == n * dim * 2 and a.i8_stats()[0] == i8_bytes(n, dim), a.last_error()
    for i in range(32):
        assert_same_dev(torch, a, b, d_qs[i:i + 1], 20, i)
    assert a.i8_stats()[1:] == (32, 0) and a.bf16_stats()[1:] == (32, 0)
    for k in (1, 5, 50, 80):
        assert_same_dev(torch, a, b, d_qs[:4], k)
    assert_same_dev(torch, a, b, d_qs[:8], 500)                            # past the switch: the bf16 copy
    assert served(a) == 32 + 16 and sum(a.bf16_stats()[1:]) == 32 + 16 + 8
    a.close(); b.close()


def test_10m_rows(hip, monkeypatch, torch):
    """10M x 768 (30.7 GB of f32 rows, 54 GB with both copies and the scratch): k = 20, one query per call."""
    n, dim = 10_000_000, 768
    free, _ = torch.cuda.mem_get_info()
    if free < 70 << 30:
        pytest.skip("device memory is short for the 10M-row case: %.0f GiB free, 70 GiB needed" % (free / 2 ** 30))
    d_rows, d_qs = _gaussian_unit_device(torch, n, dim, 20264)
    setenv(monkeypatch, None, None)
    a = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=True, keepalive=d_rows)
    setenv(monkeypatch, "0", "0")
    b = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, borrow=True, keepalive=d_rows)
    setenv(monkeypatch, None, None)
    assert a.i8_stats()[0] == i8_bytes(n, dim), a.last_error()
    for i in range(16):
        assert_same_dev(torch, a, b, d_qs[i:i + 1], 20, i)
    c8, f8 = a.i8_stats()[1:]
    assert c8 + f8 == 16 and f8 <= 1, (c8, f8)
    a.close(); b.close()
