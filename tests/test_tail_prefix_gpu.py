"""The finisher of the shadow search's tail sorts a prefix of the rescored candidates first and certifies on it where it can
(scan_bf16.hip, tail_prefix.h: tail_prefix_first, tail_prefix_certifies; rank_sort.h: rank_sort_keys_wide; DESIGN.md §3.11,
"Prefix certificate").  Only the int8 copy's k' = 10k + 150 leaves room for a proper prefix (blocks of <= 4 queries at k <= 87
over rows whose dim is a multiple of 16); the bf16 copy's blocks (b = 8, k >= 88, dim = 8) run the finisher unchanged.

Three handles over the same rows: `on` (default), `off` (CQS_HIP_TAIL_PREFIX=0: every candidate sorted at once, the parent's
verdicts) and `f32` (both copies off).  After every `search_device`: counts and keys in every one of the k slots equal in all
three; the per-query verdicts `cert` (read from the device through cqs_hip_debug_tail_verdicts) and both counter pairs
(bf16_stats, i8_stats) exactly equal between `on` and `off`.  Which branch ran is observed, not supposed: the hook also returns
how many queries certified on the prefix and how many went on to the second sort; `off` must leave both at 0.
Shapes are small: each case takes seconds.  Run on an MI355X with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth
from test_shadow_tail_gpu import dev_search, setenv

pytestmark = pytest.mark.gpu
ENV_SWITCH = "CQS_HIP_TAIL_PREFIX"
BS = (1, 3, 4, 8)
KS = (1, 20, 87, 88, 500)


@pytest.fixture
def torch():
    import torch as t
    return t


def trio(monkeypatch, torch, rows, metric=DistanceMetric.Cosine):
    """(on, off, f32) over one device buffer."""
    d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    n, dim = d.shape
    made = []
    for shadow, switch in (("1", None), ("1", "0"), ("0", None)):
        setenv(monkeypatch, shadow, shadow)
        if switch is None:
            monkeypatch.delenv(ENV_SWITCH, raising=False)
        else:
            monkeypatch.setenv(ENV_SWITCH, switch)
        made.append(HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d))
    setenv(monkeypatch, None, None)
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    on, off, f32 = made
    for h in (on, off):
        assert h.bf16_stats()[0] == n * dim * 2, h.last_error()
        assert (h.i8_stats()[0] != 0) == (dim % 16 == 0)
    assert f32.bf16_stats()[0] == 0
    return on, off, f32


def verdicts(h, b):
    """(cert[0, b) of the last device search, (queries certified on the prefix, queries that went on) since the build)."""
    f = _lib.load().cqs_hip_debug_tail_verdicts
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    cert = np.full(b, 7, np.uint32)
    pre = np.full(2, 7, np.uint64)
    assert f(h._h, b, cert.ctypes.data_as(C.c_void_p), pre.ctypes.data_as(C.c_void_p)) == _lib.OK
    return cert, (int(pre[0]), int(pre[1]))


def tickets(h, b=32):
    f = _lib.load().cqs_hip_debug_shadow_tickets
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.full(b, 7, np.uint32)
    assert f(h._h, b, out.ctypes.data_as(C.c_void_p)) == _lib.OK
    return out


def same(torch, hs, d_q, k, ctx, **kw):
    """One search on each handle.  Returns `on`'s cert array."""
    on, off, f32 = hs
    res = [dev_search(torch, h, d_q, k, **kw) for h in hs]
    torch.cuda.synchronize()
    (k1, c1), (k0, c0), (kf, cf) = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in res]
    assert np.array_equal(c1, c0) and np.array_equal(c1, cf), (ctx, c1, c0, cf)
    assert np.array_equal(k1, k0), (ctx, "on / off")
    assert np.array_equal(k1, kf), (ctx, "on / f32")
    b = d_q.shape[0]
    cert1, _ = verdicts(on, b)
    cert0, pre0 = verdicts(off, b)
    assert np.array_equal(cert1, cert0), (ctx, cert1, cert0)
    assert pre0 == (0, 0), (ctx, pre0)
    assert on.bf16_stats()[1:] == off.bf16_stats()[1:], (ctx, on.bf16_stats(), off.bf16_stats())
    assert on.i8_stats()[1:] == off.i8_stats()[1:], (ctx, on.i8_stats(), off.i8_stats())
    return cert1


def close(hs):
    for h in hs:
        assert not tickets(h).any() if h.bf16_stats()[0] else True
        h.close()


@pytest.mark.parametrize("dim", [8, 768, 2048])
@pytest.mark.parametrize("n", [300, 4097, 20_000])
def test_shapes_raw_and_pipeline(hip, monkeypatch, torch, n, dim):
    rows = synth.gaussian_unit(n, dim=dim, seed=9000 + n + dim)
    qs = synth.gaussian_unit(16, dim=dim, seed=9100 + dim)
    d_q = torch.from_numpy(qs).cuda()
    hs = trio(monkeypatch, torch, rows)
    top = float(hs[2].search_batch(qs[:1], 1)[1][0, 0])
    issued = 0
    for j, nb in enumerate(BS):
        for k in KS:
            q0 = (3 * j + k) % 8
            same(torch, hs, d_q[q0:q0 + nb], k, (n, dim, nb, k))
            # thresholds at and just under the best score: the prefix's best rows are dropped once exact, or all but a few
            for thr in (min(max(top, 0.0), 1.0), max(top * 0.8, 0.0), 0.0):
                same(torch, hs, d_q[q0:q0 + nb], k, (n, dim, nb, k, thr), mode=_lib.MODE_PIPELINE, threshold=thr)
            issued += 4 * nb
    _, cert, fb = hs[0].bf16_stats()
    assert cert + fb == issued and cert > 0, (cert, fb, issued)
    _, (pc, pf) = verdicts(hs[0], 1)
    if dim % 16 == 0 and n > 46:     # (k = 1 through the int8 copy: a proper prefix of 46 among min(n, 160) candidates)
        assert pc > 0, (pc, pf)
    if dim % 16 != 0:                # the bf16 copy alone: k' = 2k + 32 < 6k + 40, never a proper prefix
        assert (pc, pf) == (0, 0)
    close(hs)


def test_gaussian_rows_certify_on_the_prefix(hip, monkeypatch, torch):
    """20 000 Gaussian unit rows, RAW: every query of an int8 block at k <= 20 certifies on its prefix and none goes on;
    at k = 88 and in blocks of 8 the bf16 copy serves and no prefix is tried."""
    dim, n = 768, 20_000
    rows = synth.gaussian_unit(n, dim=dim, seed=9501)
    d_q = torch.from_numpy(synth.gaussian_unit(16, dim=dim, seed=9502)).cuda()
    hs = trio(monkeypatch, torch, rows)
    want = 0
    for k in (1, 5, 20):
        for q0, nb in ((0, 1), (1, 3), (4, 4)):
            cert = same(torch, hs, d_q[q0:q0 + nb], k, ("gauss", k, nb))
            assert cert.all()
            want += nb
            assert verdicts(hs[0], 1)[1] == (want, 0), (k, nb, verdicts(hs[0], 1)[1], want)
    for k, nb in ((88, 1), (20, 8), (500, 3)):
        assert same(torch, hs, d_q[:nb], k, ("gauss bf16", k, nb)).all()
        assert verdicts(hs[0], 1)[1] == (want, 0)
    close(hs)


@pytest.mark.parametrize("crowd", [60, 150, 400])
def test_crowd_below_the_kth(hip, monkeypatch, torch, crowd):
    """20 rows close to the query, then `crowd` rows within B_q below them, then the rest far away, k = 20 (prefix 160, k' =
    350).  60: the prefix passes the crowd and certifies.  150: the prefix ends inside the crowd and fails, the second sort
    runs and all k' certify.  400: the prefix fails and so do all k': the f32 scan answers."""
    dim, n = 768, 20_000
    rng = np.random.default_rng(9200 + crowd)
    rows = synth.gaussian_unit(n, dim=dim, seed=9201)
    q = synth.gaussian_unit(4, dim=dim, seed=9202)

    def unit(v):
        return (v / np.linalg.norm(v)).astype(np.float32)

    pick = rng.choice(n, 20 + crowd, replace=False)
    for j, r in enumerate(pick):
        w = 2.0 if j < 20 else 1.97 + 0.0001 * (j % 50)     # cosines about 0.894 and 0.892: closer than the int8 copy's B_q
        perp = rows[r] - np.dot(rows[r], q[0]) * q[0]       # (orthogonal to the query: the cosine is set by w alone)
        rows[r] = unit(q[0] * w + perp)
    hs = trio(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    cert = same(torch, hs, d_q[:1], 20, ("crowd", crowd))
    _, pre = verdicts(hs[0], 1)
    assert (int(cert[0]), pre) == {60: (1, (1, 0)), 150: (1, (0, 1)), 400: (0, (0, 1))}[crowd], (crowd, cert, pre)
    for k in (1, 21, 87):
        for nb in (1, 2, 4):
            same(torch, hs, d_q[:nb], k, ("crowd", crowd, k, nb))
    close(hs)


def test_half_ulp_adversarial_rows(hip, monkeypatch, torch):
    """The half-ulp adversarial corpus of test_bf16_scan_gpu.py, its two queries beside plain ones, block after block."""
    from test_bf16_scan_gpu import adversarial_corpus
    rng = np.random.default_rng(9601)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    plain = list(synth.gaussian_unit(6, seed=9602))
    qs = np.stack([plain[0], q_adv, plain[1], -q_adv] + plain[2:])
    d_qs = torch.from_numpy(qs).cuda()
    rows = adversarial_corpus(rng, sign, 1500, 2.0 ** -5, 1.05 * 2.0 ** -5)
    hs = trio(monkeypatch, torch, rows)
    for k in (1, 20, 87, 100):
        for q0, nb in ((0, 4), (4, 4), (0, 8), (1, 1), (3, 1), (0, 3), (2, 2)):
            same(torch, hs, d_qs[q0:q0 + nb], k, ("adv", k, q0, nb))
    assert hs[0].bf16_stats()[2] > 0
    close(hs)


def test_equal_scores_and_every_segment_count(hip, monkeypatch, torch):
    """Duplicated rows give candidates with equal score bits (the exact-rank branch of either sort), and k from 1 to 87
    over 4097 rows gives the wide sort prefixes of 46 to 562 keys: 8, 4, 2 and 1 threads per key; from k = 88 on the bf16
    copy serves and the finisher sorts once."""
    dim, n = 768, 4097
    rows = synth.gaussian_unit(n, dim=dim, seed=9301)
    rows[1::2] = rows[0::2][: n // 2]                          # every row twice
    d_q = torch.from_numpy(synth.gaussian_unit(8, dim=dim, seed=9302)).cuda()
    hs = trio(monkeypatch, torch, rows)
    for k in (1, 2, 5, 14, 15, 20, 36, 37, 48, 87, 88, 112, 113, 240, 241, 495, 496, 500):
        for nb in (1, 3):
            same(torch, hs, d_q[:nb], k, ("dups", k, nb))
    close(hs)


def test_uncertifiable_beside_certified_and_tickets(hip, monkeypatch, torch):
    """A NaN query and a B_q = +inf query beside certified ones: their cert is 0 in both arms, the others' 1.  Then 200 searches
    with no sync, k alternating between prefixes that certify and blocks that sort everything; ticket words 0 afterwards."""
    dim, n = 768, 20_000
    rows = synth.gaussian_unit(n, dim=dim, seed=9401)
    q = synth.gaussian_unit(16, dim=dim, seed=9402)
    q[1, 7] = np.nan
    q[2] *= np.float32(2e30)
    hs = trio(monkeypatch, torch, rows)
    on, off, f32 = hs
    d_q = torch.from_numpy(q).cuda()
    fb_want = 0
    for k in (1, 20, 88):
        for q0, nb in ((0, 4), (1, 1), (2, 2), (0, 8), (3, 3)):
            cert = same(torch, hs, d_q[q0:q0 + nb], k, ("bad", k, q0, nb))
            want = np.array([0 if i in (1, 2) else 1 for i in range(q0, q0 + nb)], np.uint32)
            assert np.array_equal(cert, want), (k, q0, nb, cert)
            fb_want += int((want == 0).sum())
    assert on.bf16_stats()[1:] == (3 * 18 - fb_want, fb_want)
    plan = [((i * 5) % 8 + 3, BS[i % 4], KS[(i * 3) % 5]) for i in range(200)]
    want = [dev_search(torch, f32, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    torch.cuda.synchronize()
    got = [dev_search(torch, on, d_q[q0:q0 + nb], k) for q0, nb, k in plan]          # back to back: no sync
    got0 = [dev_search(torch, off, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    torch.cuda.synchronize()
    for i, ((kg, cg), (k0, c0), (kw, cw)) in enumerate(zip(got, got0, want)):
        assert torch.equal(cg, cw) and torch.equal(kg, kw) and torch.equal(c0, cw) and torch.equal(k0, kw), (i, plan[i])
    assert on.bf16_stats()[1:] == off.bf16_stats()[1:] and on.i8_stats()[1:] == off.i8_stats()[1:]
    assert on.bf16_stats()[2] == fb_want, "every query of the 200 searches is certifiable"
    close(hs)
