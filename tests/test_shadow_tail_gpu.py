"""The fused tail of a shadow search: B_q, rescore and certify in one launch, the last workgroup of each query to arrive
certifying (scan_bf16.hip, rescore_certify_kernel).

Every comparison is between a handle with the shadow (both copies: CQS_HIP_SCAN_BF16=1 CQS_HIP_SCAN_I8=1, or the default
policy at 1M rows) and a CQS_HIP_SCAN_BF16=0 handle over the same rows: identical counts and identical keys in every one of
the k slots through `search_device`, identical rows and score bits through the host searches.  The cases aim at what the
fusion adds: the per-query ticket re-armed by every search, candidate counts from 0 to 1023, workgroup counts that do and
do not divide evenly, words handed from workgroup to workgroup while the previous search's copies are still in the L1s
(the 20 000-row corpus), and B_q computed inside the launch.  Run on an MI355X with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth

pytestmark = pytest.mark.gpu
ENV_BF16, ENV_I8 = "CQS_HIP_SCAN_BF16", "CQS_HIP_SCAN_I8"
I8_MAX_Q, K_SWITCH = 4, 87        # scan_i8.h: kI8MaxQ; the largest k the int8 copy serves
BS = (1, 2, 3, 4, 5, 8)
KS = (1, 20, 87, 88, 500, 1000)
COMBOS = [(b, k) for b in BS for k in KS]


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


def dev_pair(monkeypatch, torch, rows, metric=DistanceMetric.Cosine, policy=("1", "1")):
    """(borrowed handle with both copies, borrowed handle on f32 alone) over one device buffer."""
    d = rows if hasattr(rows, "data_ptr") else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    n, dim = d.shape
    setenv(monkeypatch, *policy)
    a = HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d)
    setenv(monkeypatch, "0", "0")
    b = HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d)
    setenv(monkeypatch, None, None)
    assert a.bf16_stats()[0] == n * dim * 2 and a.i8_stats()[0] == n * dim + n * 4, a.last_error()
    assert b.bf16_stats()[0] == 0 and b.i8_stats()[0] == 0
    return a, b


def dev_search(torch, h, d_q, k, d_keep=None, mode=_lib.MODE_RAW, threshold=0.0, stream=None):
    b = d_q.shape[0]
    keys = torch.full((b, k), -1, dtype=torch.int64, device="cuda")   # every slot must be written
    counts = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())               # (the two fills above ran on the current stream)
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


def assert_same_host(a, b, q, k, ctx="", **kw):
    (ra, sa, ca), (rb, sb, cb) = a.search_batch(q, k, **kw), b.search_batch(q, k, **kw)
    assert np.array_equal(ca, cb), (ctx, k, ca, cb)
    for i in range(len(ca)):
        c = int(ca[i])
        assert np.array_equal(ra[i, :c], rb[i, :c]), (ctx, k, i)
        assert np.array_equal(sa[i, :c].view(np.uint32), sb[i, :c].view(np.uint32)), (ctx, k, i)
    return ca


def served(b, k):
    """(queries the shadow serves, queries of them the int8 copy serves) of one search."""
    return b, (b if b <= I8_MAX_Q and k <= K_SWITCH else 0)


def plan(n_searches, pool):
    """Search i: (first query, b, k).  Consecutive searches differ in b, in k and in every query (the step of 11 is past the
    largest b), so a word left over from the search before gives a wrong answer."""
    out = []
    for i in range(n_searches):
        b, k = COMBOS[(i * 7) % len(COMBOS)]         # 7 and 36 are coprime: every (b, k), five or six times each
        out.append(((i * 11) % (pool - 8), b, k))
    return out


def unit_rows_on_device(torch, n, dim, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    d = torch.empty((n, dim), device="cuda", dtype=torch.float32)
    for lo in range(0, n, 1 << 18):
        hi = min(n, lo + (1 << 18))
        x = torch.randn((hi - lo, dim), generator=g, device="cuda"); x /= x.norm(dim=1, keepdim=True); d[lo:hi] = x
    return d


@pytest.mark.parametrize("n", [1_000_000, 20_000])
def test_200_searches_back_to_back(hip, monkeypatch, torch, n):
    """200 searches on one handle with no host sync between them.  At 1M rows the default policy builds both copies; at
    20 000 rows consecutive searches reuse the same CUs within microseconds, with the previous search's ekeys and B_q still
    in their L1s."""
    dim, pool = 768, 64
    d_rows = unit_rows_on_device(torch, n, dim, 7000 + n)
    d_qs = torch.from_numpy(synth.gaussian_unit(pool, dim=dim, seed=7100 + (n % 1000))).cuda()
    a, b = dev_pair(monkeypatch, torch, d_rows, policy=(None, None) if n >= 1_000_000 else ("1", "1"))
    searches = plan(200, pool)
    want = [dev_search(torch, b, d_qs[q0:q0 + nb], k) for q0, nb, k in searches]
    torch.cuda.synchronize()
    got = [dev_search(torch, a, d_qs[q0:q0 + nb], k) for q0, nb, k in searches]     # back to back: no sync
    torch.cuda.synchronize()
    for i, ((kg, cg), (kw, cw)) in enumerate(zip(got, want)):
        assert torch.equal(cg, cw), (n, i, searches[i], cg.tolist(), cw.tolist())
        assert torch.equal(kg, kw), (n, i, searches[i])
    want_all = sum(served(nb, k)[0] for _, nb, k in searches)
    want_i8 = sum(served(nb, k)[1] for _, nb, k in searches)
    _, cert, fb = a.bf16_stats()
    _, cert8, fb8 = a.i8_stats()
    assert cert + fb == want_all and cert8 + fb8 == want_i8, (cert, fb, cert8, fb8, want_all, want_i8)
    assert cert > 0 and cert8 > 0
    # the host searches take the same tail: every (b, k) once, other queries each time
    qs = d_qs.cpu().numpy()
    for j, (nb, k) in enumerate(COMBOS):
        q0 = (j * 13) % (pool - 8)
        assert_same_host(a, b, qs[q0:q0 + nb], k, (n, nb))
    _, cert2, fb2 = a.bf16_stats()
    assert cert2 + fb2 == want_all + sum(nb for nb, _ in COMBOS)
    a.close(); b.close()


def test_two_streams_interleaved_with_host(hip, monkeypatch, torch):
    rows = synth.gaussian_unit(300_000, seed=7201)
    qs = synth.gaussian_unit(56, seed=7202)
    d_qs = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    shapes = [(2, 20), (5, 20), (1, 500), (4, 87), (3, 88), (8, 1)]      # int8 and bf16 blocks by turns
    steps = [(4 * j, *shapes[j % len(shapes)]) for j in range(12)]
    want_dev = [dev_search(torch, b, d_qs[i:i + nb], k) for i, nb, k in steps]
    want_host = [b.search_batch(qs[i], 20) for i in range(24)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got_dev, got_host = [], []
    for j, (i, nb, k) in enumerate(steps):
        got_dev.append(dev_search(torch, a, d_qs[i:i + nb], k, stream=s1 if j % 2 == 0 else s2))   # no sync: the handle orders the scratch
        got_host.append(a.search_batch(qs[2 * j], 20))
        got_host.append(a.search_batch(qs[2 * j + 1], 20))
    torch.cuda.synchronize()
    for (kg, cg), (kw, cw) in zip(got_dev, want_dev):
        assert torch.equal(kg, kw) and torch.equal(cg, cw)
    for (rg, sg, cg), (rw, sw, cw) in zip(got_host, want_host):
        assert np.array_equal(cg, cw) and np.array_equal(rg, rw) and np.array_equal(sg.view(np.uint32), sw.view(np.uint32))
    _, cert, fb = a.bf16_stats()
    assert cert + fb == sum(nb for _, nb, _ in steps) + 24 and cert > 0, (cert, fb)
    a.close(); b.close()


def test_pipeline_thresholds_and_dot_metric(hip, monkeypatch, torch):
    """PIPELINE searches keep the stand-alone bound launch (the scan's drop rule reads B_q); the dot metric has no unit rows."""
    rows = synth.gaussian_unit(30_000, seed=7301)
    qs = synth.gaussian_unit(8, seed=7302)
    d_q = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    top = float(b.search_batch(qs[:1], 1)[1][0, 0])
    for thr in (0.0, 0.05, 0.1, top * 0.9, top, 0.999, -0.5):
        for k in (1, 20, 500):
            for nb in (1, 4, 8):
                assert_same_dev(torch, a, b, d_q[:nb], k, thr, mode=_lib.MODE_PIPELINE, threshold=thr)
                assert_same_dev(torch, a, b, d_q[nb - 1:nb], k, thr)          # RAW in between: B_q from the fused launch again
        assert_same_host(a, b, qs[:3], 20, thr, mode=_lib.MODE_PIPELINE, threshold=thr)
    a.close(); b.close()
    rng = np.random.default_rng(7303)
    rows = (rng.standard_normal((6000, 768)) * rng.uniform(0.1, 30, (6000, 1))).astype(np.float32)
    qs = rng.standard_normal((5, 768)).astype(np.float32)
    d_q = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows, DistanceMetric.DotProduct)
    for k in (1, 20, 87, 500):
        for nb in (1, 3, 5):
            assert_same_dev(torch, a, b, d_q[:nb], k, "dot")
            assert_same_host(a, b, qs[:nb], k, "dot")
    a.close(); b.close()


def test_uncertified_queries_fall_back(hip, monkeypatch, torch):
    """Queries the finisher does not certify: the half-ulp adversarial rows, a NaN query, a query whose norm makes
    B_q = +inf.  The verdict must reach the gated f32 launches: answers equal, fallbacks counted on the device."""
    from test_bf16_scan_gpu import adversarial_corpus
    rng = np.random.default_rng(7401)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    qs = np.stack([q_adv, -q_adv] + list(synth.gaussian_unit(4, seed=7402)))
    d_qs = torch.from_numpy(qs).cuda()
    rows = adversarial_corpus(rng, sign, 1500, 2.0 ** -5, 1.05 * 2.0 ** -5)      # crowded scores
    a, b = dev_pair(monkeypatch, torch, rows)
    issued = 0
    for i in range(len(qs)):
        for k in (1, 20, 100):
            assert_same_dev(torch, a, b, d_qs[i:i + 1], k, ("adv", i))
            issued += 1
    assert_same_dev(torch, a, b, d_qs, 20, "adv block")
    assert_same_dev(torch, a, b, d_qs[:4], 20, "adv block of 4")
    issued += len(qs) + 4
    _, cert, fb = a.bf16_stats()
    assert cert + fb == issued and fb > 0, (cert, fb)
    a.close(); b.close()

    rows = synth.gaussian_unit(20_000, seed=7403)
    q = synth.gaussian_unit(4, seed=7404)
    q[1, 7] = np.nan
    q[2] *= np.float32(2e30)            # ||q|| max||x|| past 2^100: B_q = +inf, every score still finite in f32
    d_q = torch.from_numpy(q).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 20, 500):
        before = a.bf16_stats()[2]
        assert_same_dev(torch, a, b, d_q, k, "nan + inf")
        assert_same_dev(torch, a, b, d_q[1:2], k, "nan")
        assert_same_dev(torch, a, b, d_q[2:3], k, "inf")
        assert_same_dev(torch, a, b, d_q[3:4], k, "plain")
        assert a.bf16_stats()[2] - before >= 4, k          # the NaN and the +inf query, twice each
        assert_same_host(a, b, q[2:4], k, "inf host")
    assert a.bf16_stats()[1] > 0
    a.close(); b.close()


def test_few_and_no_candidates(hip, monkeypatch, torch):
    """Fewer candidates than one workgroup holds, and none at all: the workgroups still count their arrivals, the last one
    writes zero counts and every key slot."""
    rows = synth.gaussian_unit(3, seed=7501)
    qs = synth.gaussian_unit(4, seed=7502)
    d_q = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 2, 20, 500):
        for nb in (1, 4):
            _, counts = assert_same_dev(torch, a, b, d_q[:nb], k, "3 rows")
            assert (counts == min(k, 3)).all()
            assert_same_host(a, b, qs[:nb], k, "3 rows")
    a.close(); b.close()
    n = 50_000
    rows = synth.gaussian_unit(n, seed=7503)
    a, b = dev_pair(monkeypatch, torch, rows)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    d_none = torch.from_numpy(words.view(np.int32)).cuda()
    two = words.copy(); two[10] = 1; two[900] = 1 << 17
    d_two = torch.from_numpy(two.view(np.int32)).cuda()
    d_q8 = torch.from_numpy(synth.gaussian_unit(8, seed=7504)).cuda()
    for k in (1, 20, 88, 1000):
        for nb in (1, 3, 8):
            _, counts = assert_same_dev(torch, a, b, d_q8[:nb], k, "none", d_keep=d_none)
            assert not counts.any()
            _, counts = assert_same_dev(torch, a, b, d_q8[:nb], k, "two", d_keep=d_two)
            assert (counts == min(k, 2)).all()
            assert_same_dev(torch, a, b, d_q8[:nb], k, "all rows again")
    a.close(); b.close()


def test_bq_of_the_fused_launch_has_the_bound_kernels_bits(hip, monkeypatch, torch):
    lib = _lib.load()
    read_bq = lib.cqs_hip_debug_shadow_bq
    read_bq.restype = C.c_int32
    read_bq.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    hooks = {}
    for name in ("cqs_hip_debug_shadow_bound", "cqs_hip_debug_shadow_bound_i8"):
        fn = getattr(lib, name)
        fn.restype = C.c_int32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        hooks[name] = fn
    for dim in (128, 768, 2048):
        rows = synth.gaussian_unit(3000, dim=dim, seed=7600 + dim)
        a, b = dev_pair(monkeypatch, torch, rows)
        rng = np.random.default_rng(7601 + dim)
        qs = [rng.standard_normal(dim).astype(np.float32) * np.float32(s) for s in (1.0, 1e-3, 37.0, 2e30)]
        nan = rng.standard_normal(dim).astype(np.float32); nan[3] = np.nan
        qs += [nan, np.zeros(dim, np.float32), rng.standard_normal(dim).astype(np.float32), rng.standard_normal(dim).astype(np.float32)]
        q = np.ascontiguousarray(np.stack(qs))
        d_q = torch.from_numpy(q).cuda()
        for q0, nb, k, hook in ((0, 4, 20, "cqs_hip_debug_shadow_bound_i8"), (4, 3, 87, "cqs_hip_debug_shadow_bound_i8"),
                                (0, 8, 20, "cqs_hip_debug_shadow_bound"), (2, 4, 500, "cqs_hip_debug_shadow_bound")):
            assert_same_dev(torch, a, b, d_q[q0:q0 + nb], k, (dim, q0, nb))        # RAW: B_q comes from the fused launch
            fused = np.zeros(nb, np.float32)
            assert read_bq(a._h, nb, fused.ctypes.data) == _lib.OK
            dev, host = np.zeros(nb, np.float32), np.zeros(nb, np.float32)
            part = np.ascontiguousarray(q[q0:q0 + nb])
            assert hooks[hook](a._h, part.ctypes.data, nb, dev.ctypes.data, host.ctypes.data) == _lib.OK
            assert np.array_equal(fused.view(np.uint32), dev.view(np.uint32)), (dim, q0, nb, k, fused, dev)
        a.close(); b.close()
