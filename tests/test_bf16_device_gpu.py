"""The bf16 shadow on the device-API search (`cqs_hip_index_search_device`) and the shadow policy at create
(include/cqs_hip.h).

Every comparison is between a borrowed handle made with CQS_HIP_SCAN_BF16=1 (shadow built at create) and one made with
CQS_HIP_SCAN_BF16=0 over the same device rows, both searched through `search_device`: identical keys (rows and score
bits, every one of the k slots) and identical counts.  Run on an MI355X with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth
from cqs_amd.index import HipError

pytestmark = pytest.mark.gpu
ENV = "CQS_HIP_SCAN_BF16"


@pytest.fixture
def torch():
    import torch as t
    return t


def borrowed(monkeypatch, d_rows, metric=DistanceMetric.Cosine, env=None):
    if env is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, env)
    n, dim = d_rows.shape
    h = HipIndex.build_from_device(None, d_rows.data_ptr(), n, dim, metric, borrow=True, keepalive=d_rows)
    monkeypatch.delenv(ENV, raising=False)
    return h


def dev_pair(monkeypatch, torch, rows, metric=DistanceMetric.Cosine):
    """(borrowed handle with the shadow, borrowed handle without) over the same device rows."""
    d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    a = borrowed(monkeypatch, d, metric, "1")
    b = borrowed(monkeypatch, d, metric, "0")
    n, dim = rows.shape
    assert a.bf16_stats()[0] == n * dim * 2, a.last_error()
    assert b.bf16_stats()[0] == 0
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


CORPORA = [(n, d) for d in (128, 264, 768) for n in (1, 255, 257, 4097)] + \
          [(n, d) for d in (1024, 2048) for n in (1, 257, 4097)] + [(100_000, 768)]
KS = (1, 20, 100, 500, 1000)


@pytest.mark.parametrize("n,dim", CORPORA)
def test_device_path_identical(hip, monkeypatch, torch, n, dim):
    rows = synth.gaussian_unit(n, dim=dim, seed=3000 + n + dim)
    d_q = torch.from_numpy(synth.gaussian_unit(8, dim=dim, seed=4000 + n + dim)).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in KS:
        for nb in range(1, 9):
            assert_same_dev(torch, a, b, d_q[:nb], k, (n, dim, nb))
    _, cert, fb = a.bf16_stats()
    assert cert + fb == len(KS) * 36                  # every query of every block took the shadow path
    if n == 100_000:
        assert cert > 0
    assert b.bf16_stats()[1:] == (0, 0)
    a.close(); b.close()


def test_device_dot_metric_and_pipeline(hip, monkeypatch, torch):
    rng = np.random.default_rng(17)
    rows = (rng.standard_normal((6000, 768)) * rng.uniform(0.1, 30, (6000, 1))).astype(np.float32)
    d_q = torch.from_numpy(rng.standard_normal((5, 768)).astype(np.float32)).cuda()
    a, b = dev_pair(monkeypatch, torch, rows, DistanceMetric.DotProduct)
    for k in (1, 20, 500):
        for nb in (1, 5):
            assert_same_dev(torch, a, b, d_q[:nb], k)
    a.close(); b.close()
    rows = synth.gaussian_unit(30_000, seed=18)
    d_q = torch.from_numpy(synth.gaussian_unit(4, seed=19)).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    top = float(b.search_batch(synth.gaussian_unit(4, seed=19)[:1], 1)[1][0, 0])
    for thr in (0.0, 0.05, 0.1, top * 0.9, top, 0.999, -0.5):
        for k in (1, 20, 500):
            for nb in (1, 4):
                assert_same_dev(torch, a, b, d_q[:nb], k, thr, mode=_lib.MODE_PIPELINE, threshold=thr)
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["sparse", "dense", "all", "none"])
def test_device_bitsets(hip, monkeypatch, torch, kind):
    n = 50_000
    rows = synth.gaussian_unit(n, seed=21)
    d_q = torch.from_numpy(synth.gaussian_unit(3, seed=22)).cuda()
    rng = np.random.default_rng(23)
    keep = {"sparse": rng.random(n) < 0.01, "dense": rng.random(n) < 0.9,
            "all": np.ones(n, bool), "none": np.zeros(n, bool)}[kind]
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    idx = np.nonzero(keep)[0]
    np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
    d_keep = torch.from_numpy(words.view(np.int32)).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 20, 500):
        for nb in (1, 3):
            keys, counts = assert_same_dev(torch, a, b, d_q[:nb], k, kind, d_keep=d_keep)
            if kind == "none":
                assert not counts.any()
    a.close(); b.close()


def test_device_nan_query_runs_f32(hip, monkeypatch, torch):
    rows = synth.gaussian_unit(20_000, seed=31)
    q = synth.gaussian_unit(3, seed=32)
    q[1, 7] = np.nan
    d_q = torch.from_numpy(q).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 20, 500):
        assert_same_dev(torch, a, b, d_q, k)
        assert_same_dev(torch, a, b, d_q[1:2], k)
    _, cert, fb = a.bf16_stats()
    assert fb >= 6 and cert > 0, (cert, fb)              # the NaN query is never certified: the gated f32 pass ran
    a.close(); b.close()


def test_device_adversarial_rounding_falls_back(hip, monkeypatch, torch):
    from test_bf16_scan_gpu import adversarial_corpus
    rng = np.random.default_rng(61)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    qs = np.stack([q_adv, -q_adv] + list(synth.gaussian_unit(6, seed=62)))
    d_qs = torch.from_numpy(qs).cuda()
    stats = []
    for npairs, lo, hi, ks in ((300, 2.0 ** -6, 2.0 ** -4, (1, 10, 50, 500)),
                               (1500, 2.0 ** -5, 1.05 * 2.0 ** -5, (1, 20, 100))):    # crowded scores
        rows = adversarial_corpus(rng, sign, npairs, lo, hi)
        a, b = dev_pair(monkeypatch, torch, rows)
        for i in range(len(qs)):
            for k in ks:
                assert_same_dev(torch, a, b, d_qs[i:i + 1], k, (npairs, i))
        assert_same_dev(torch, a, b, d_qs, 20, npairs)
        stats.append(a.bf16_stats())
        a.close(); b.close()
    assert stats[0][1] > 0, stats                        # certified
    assert stats[1][2] > 0, stats                        # fell back, counted by the device path
    assert sum(s[1] + s[2] for s in stats) == 8 * 4 + 8 + 8 * 3 + 8


def test_device_side_stream_interleaved_with_host(hip, monkeypatch, torch):
    rows = synth.gaussian_unit(300_000, seed=41)
    qs = synth.gaussian_unit(24, seed=42)
    d_qs = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    want_dev = [dev_search(torch, b, d_qs[i:i + 2], 20) for i in range(0, 24, 2)]
    want_host = [b.search_batch(qs[i], 20) for i in range(24)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got_dev, got_host = [], []
    for j, i in enumerate(range(0, 24, 2)):
        got_dev.append(dev_search(torch, a, d_qs[i:i + 2], 20, stream=side))   # no sync: the handle orders the scratch
        got_host.append(a.search_batch(qs[i], 20))
        got_host.append(a.search_batch(qs[i + 1], 20))
    torch.cuda.synchronize()
    for (kg, cg), (kw, cw) in zip(got_dev, want_dev):
        assert torch.equal(kg, kw) and torch.equal(cg, cw)
    for (rg, sg, cg), (rw, sw, cw) in zip(got_host, want_host):
        assert np.array_equal(cg, cw) and np.array_equal(rg, rw) and np.array_equal(sg.view(np.uint32), sw.view(np.uint32))
    _, cert, fb = a.bf16_stats()
    assert cert + fb == 48 and cert > 0, (cert, fb)
    a.close(); b.close()


def test_auto_policy_small_and_borrowed_rules(hip, monkeypatch, torch):
    rows = synth.gaussian_unit(1000, seed=51)
    d = torch.from_numpy(rows).cuda()
    h = borrowed(monkeypatch, d)                        # default policy: 3 MB is far below the 1 GiB line
    assert h.bf16_stats()[0] == 0
    assert "1 GiB" in h.last_error()
    h.close()
    h = borrowed(monkeypatch, d, env="1")
    assert h.bf16_stats()[0] == 1000 * 768 * 2
    with pytest.raises(HipError) as e:                  # enabling on a borrowed handle stays refused, shadow or not
        h.set_bf16_scan(True)
    assert e.value.code == _lib.ERR_INVALID
    ref = borrowed(monkeypatch, d, env="0")
    d_q = torch.from_numpy(synth.gaussian_unit(2, seed=52)).cuda()
    assert_same_dev(torch, h, ref, d_q, 20)
    h.set_bf16_scan(False)                              # the per-handle opt-out frees it
    counted = h.bf16_stats()[1:]
    assert h.bf16_stats()[0] == 0 and sum(counted) == 2   # (the device counts survive the shadow)
    assert_same_dev(torch, h, ref, d_q, 20)
    assert h.bf16_stats()[1:] == counted
    h.close(); ref.close()
    odd = torch.from_numpy(np.ascontiguousarray(synth.gaussian_unit(300, dim=100, seed=53))).cuda()
    h = borrowed(monkeypatch, odd, env="1")             # dim % 8 != 0: created on f32, last_error says why
    assert h.bf16_stats()[0] == 0 and "multiple of 8" in h.last_error()
    h.close()
    out = synth.gaussian_unit(300, seed=54)
    out[7, 3] = np.float32(2.0 ** 64)
    h = borrowed(monkeypatch, torch.from_numpy(out).cuda(), env="1")
    assert h.bf16_stats()[0] == 0 and "2^64" in h.last_error()
    h.close()
    owned = HipIndex.build_from_flat(None, rows)        # owned small handle: no shadow unless asked
    assert owned.bf16_stats()[0] == 0
    owned.close()


def test_auto_policy_bench_shape_1m(hip, monkeypatch, torch):
    """1M x 768 f32 (3 GB, over the 1 GiB line): a default borrowed handle has the shadow and answers the bench shape
    (one query, k = 20) exactly as a CQS_HIP_SCAN_BF16=0 handle, with no fallback."""
    n, dim = 1_000_000, 768
    g = torch.Generator(device="cuda"); g.manual_seed(20262)
    d_rows = torch.empty((n, dim), device="cuda", dtype=torch.float32)
    for lo in range(0, n, 1 << 18):
        hi = min(n, lo + (1 << 18))
        x = torch.randn((hi - lo, dim), generator=g, device="cuda"); x /= x.norm(dim=1, keepdim=True); d_rows[lo:hi] = x
    d_qs = torch.randn((32, dim), generator=g, device="cuda"); d_qs /= d_qs.norm(dim=1, keepdim=True)
    a = borrowed(monkeypatch, d_rows)
    b = borrowed(monkeypatch, d_rows, env="0")
    assert a.bf16_stats()[0] == n * dim * 2, a.last_error()
    assert b.bf16_stats()[0] == 0
    for i in range(32):
        assert_same_dev(torch, a, b, d_qs[i:i + 1], 20, i)
    assert a.bf16_stats()[1:] == (32, 0)
    assert_same_dev(torch, a, b, d_qs[:8], 500)
    _, cert, fb = a.bf16_stats()
    assert cert + fb == 40 and fb <= 1, (cert, fb)
    a.close(); b.close()


def test_device_bound_matches_host(hip, monkeypatch, torch):
    lib = _lib.load()
    fn = lib.cqs_hip_debug_shadow_bound
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    for dim in (128, 768, 2048):
        rows = synth.gaussian_unit(3000, dim=dim, seed=60 + dim)
        h = borrowed(monkeypatch, torch.from_numpy(rows).cuda(), env="1")
        rng = np.random.default_rng(dim)
        qs = [rng.standard_normal(dim).astype(np.float32) * s for s in (1.0, 1e-3, 37.0)]
        qs += [np.zeros(dim, np.float32), np.full(dim, 1e30, np.float32), rng.standard_normal(dim).astype(np.float32) * 1e18]
        nan = rng.standard_normal(dim).astype(np.float32); nan[3] = np.nan
        inf = rng.standard_normal(dim).astype(np.float32); inf[5] = np.inf
        qs += [nan, inf]
        q = np.ascontiguousarray(np.stack(qs))
        dev, host = np.zeros(len(qs), np.float32), np.zeros(len(qs), np.float32)
        assert fn(h._h, q.ctypes.data, len(qs), dev.ctypes.data, host.ctypes.data) == _lib.OK
        for i in range(len(qs)):
            if np.isinf(host[i]):
                assert np.isinf(dev[i]) and dev[i] > 0, (dim, i, dev[i], host[i])
            else:
                assert np.isfinite(dev[i]) and host[i] >= 0, (dim, i)
                assert dev[i] >= host[i] and dev[i] <= np.nextafter(host[i], np.float32(np.inf)), (dim, i, dev[i], host[i])
        assert np.isinf(host[6]) and np.isinf(host[7])   # non-finite queries: no certificate
        assert np.isinf(host[4])                          # ||q|| R past the f32 range
        h.close()
