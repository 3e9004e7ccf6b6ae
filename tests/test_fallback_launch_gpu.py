"""The f32 fallback behind a certified shadow search as ONE gated launch: an exact brute-force top-k of the block
(scan_fallback.hip, f32_topk_fallback_kernel; DESIGN.md §3.11 "One gated launch").

Every comparison is between a handle with the shadow (CQS_HIP_SCAN_BF16=1 CQS_HIP_SCAN_I8=1, so that the shadow exists at
these sizes) and a handle with both copies off (the plain f32 scan + select) over the same rows: identical counts and
identical keys in every one of the k slots through `search_device`, identical rows and score bits through the host API.
The gate is forced open with the means of the other shadow tests: a NaN query or a query whose B_q is +inf in the block (the
whole block is then recomputed, so the ordinary queries beside it are answered by the fallback too), and the half-ulp
adversarial rows.  `bf16_stats` proves in every case that the gate was really open.  Every input is an ordinary in-bounds
search.  Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth
from test_shadow_tail_gpu import assert_same_dev, assert_same_host, dev_search, setenv, unit_rows_on_device

pytestmark = pytest.mark.gpu
CAP = 128                    # scan_fallback.h: kFallbackMaxK
ENV_SWITCH = "CQS_HIP_FALLBACK_ONE_LAUNCH"
BIG = np.float32(2e30)       # ||q|| max||x|| past 2^100: B_q = +inf, every score of unit rows still finite in f32


@pytest.fixture
def torch():
    import torch as t
    return t


def pair(monkeypatch, torch, rows, metric=DistanceMetric.Cosine, switch=None):
    """(borrowed handle with the shadow, borrowed handle on f32 alone) over one device buffer.  The int8 copy is built where
    its dim rule allows (dim % 16 == 0)."""
    d = rows if hasattr(rows, "data_ptr") else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    n, dim = d.shape
    setenv(monkeypatch, "1", "1")
    if switch is not None:
        monkeypatch.setenv(ENV_SWITCH, switch)
    a = HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d)
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    setenv(monkeypatch, "0", "0")
    ref = HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d)
    setenv(monkeypatch, None, None)
    assert a.bf16_stats()[0] == n * dim * 2, a.last_error()
    assert a.i8_stats()[0] == (n * dim + n * 4 if dim % 16 == 0 else 0), a.last_error()
    assert ref.bf16_stats()[0] == 0
    return a, ref


def queries(dim, count, seed):
    """Unit queries; 1 has a NaN component, 2 a B_q of +inf."""
    q = synth.gaussian_unit(count, dim=dim, seed=seed)
    q[1, dim // 2] = np.nan
    q[2] *= BIG
    return q


def fallbacks(h):
    return h.bf16_stats()[2]


@pytest.mark.parametrize("dim", [8, 264, 768, 1024, 2048])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 1023, 4097, 20_000, 300_000])
def test_shapes(hip, monkeypatch, torch, n, dim):
    """Fewer rows than workgroups, than waves, one more than a tile; dims that end in a partial 256-float chunk (264, 768)."""
    d_rows = unit_rows_on_device(torch, n, dim, 9000 + n + dim)
    q = queries(dim, 8, 9001 + dim)
    d_q = torch.from_numpy(q).cuda()
    a, ref = pair(monkeypatch, torch, d_rows)
    ks = [1, 20, CAP, CAP + 1] + ([n + 2] if n + 2 <= CAP else [])      # k > n at the small sizes (and 20 > n at n <= 3)
    for k in ks:
        for q0, nb in ((2, 1), (1, 2), (0, 3), (0, 8)):                  # each block holds query 1 or 2: its gate is open
            before = fallbacks(a)
            ka, ca = assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], k, (n, dim, q0, nb))
            assert fallbacks(a) > before, (n, dim, k, q0, nb)
            assert (ca <= min(k, n)).all()
            if q0 <= 1 < q0 + nb:
                assert ca[1 - q0] == 0 and not ka[1 - q0].any()          # the NaN query: every score non-finite
        assert_same_host(a, ref, q[2:5], k, (n, dim))
    a.close(); ref.close()


@pytest.mark.parametrize("k", [1, 20, CAP, CAP + 1])
def test_block_widths_mixed_and_consecutive(hip, monkeypatch, torch, k):
    """b in {1, 2, 3, 5, 8}, certified and uncertified queries in one block and in consecutive blocks, no sync between them.
    k = CAP + 1 takes the two gated launches and agrees all the same."""
    n, dim = 20_000, 768
    d_rows = unit_rows_on_device(torch, n, dim, 9100)
    q = queries(dim, 24, 9101)
    q[13, 5] = np.nan
    d_q = torch.from_numpy(q).cuda()
    a, ref = pair(monkeypatch, torch, d_rows)
    bad = {1, 2, 13}
    blocks = [(3, 1), (2, 1), (4, 2), (1, 2), (0, 3), (5, 3), (9, 5), (14, 5), (0, 8), (16, 8), (6, 8), (1, 1), (20, 2), (12, 3)]
    want = [dev_search(torch, ref, d_q[q0:q0 + nb], k) for q0, nb in blocks]
    torch.cuda.synchronize()
    got = [dev_search(torch, a, d_q[q0:q0 + nb], k) for q0, nb in blocks]          # back to back: no sync
    torch.cuda.synchronize()
    for i, ((kg, cg), (kw, cw)) in enumerate(zip(got, want)):
        assert torch.equal(cg, cw), (k, blocks[i], cg.tolist(), cw.tolist())
        assert torch.equal(kg, kw), (k, blocks[i])
    _, cert, fb = a.bf16_stats()
    assert cert + fb == sum(nb for _, nb in blocks) and cert > 0
    assert fb >= sum(len(bad & set(range(q0, q0 + nb))) for q0, nb in blocks)
    a.close(); ref.close()


def test_ties_and_non_finite_rows(hip, monkeypatch, torch):
    """(a) 5 000 copies of one row, every fourth row, so that every workgroup holds some: the order is by row alone.
    (b) fewer than k finite rows.  (c) no finite row at all: count 0 and zero keys."""
    n, dim = 20_000, 768
    base = synth.gaussian_unit(n, dim=dim, seed=9200)
    q = queries(dim, 4, 9201)
    q[2] = q[0] * BIG                                              # (the tied rows are this query's best)
    d_q = torch.from_numpy(q).cuda()
    rows = base.copy()
    v = q[0] + 0.5 * base[0]
    rows[::4] = (v / np.linalg.norm(v)).astype(np.float32)
    a, ref = pair(monkeypatch, torch, rows)
    for k in (1, 20, CAP):
        for q0, nb in ((2, 1), (0, 3), (0, 4)):
            before = fallbacks(a)
            ka, ca = assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], k, ("ties", k, nb))
            assert fallbacks(a) > before
            top = ka[2 - q0].view(np.uint64)                      # query 2: k tied rows, ascending
            assert ca[2 - q0] == k and len(set((top >> np.uint64(32)).tolist())) == 1
            assert ((np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))) == np.arange(k, dtype=np.uint64) * np.uint64(4)).all()
    a.close(); ref.close()

    rows = base[:5000].copy()
    rows[:, 3] = np.nan
    finite = [7, 255, 256, 1000, 4095, 4096, 4999]
    rows[finite] = base[finite]
    a, ref = pair(monkeypatch, torch, rows)
    for q0, nb in ((2, 1), (0, 4)):
        before = fallbacks(a)
        ka, ca = assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], 20, ("few", nb))
        assert fallbacks(a) > before and ca[2 - q0] == len(finite)
    a.close(); ref.close()

    rows = base[:5000].copy()
    rows[:, 700] = np.inf
    a, ref = pair(monkeypatch, torch, rows)
    for q0, nb in ((2, 1), (0, 4)):
        before = fallbacks(a)
        ka, ca = assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], 20, ("none", nb))
        assert fallbacks(a) > before and not ca.any() and not ka.any()
    a.close(); ref.close()


@pytest.mark.parametrize("metric", [DistanceMetric.Cosine, DistanceMetric.DotProduct])
def test_modes_filters_and_adversarial_rows(hip, monkeypatch, torch, metric):
    """The half-ulp adversarial corpus (scores around 0.75: inside PIPELINE's clamp), both metrics: RAW, PIPELINE at three
    thresholds (one drops everything), a shared bitset that empties whole workgroups' ranges, a two-row and an empty one."""
    from test_bf16_scan_gpu import adversarial_corpus
    rng = np.random.default_rng(9300)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    plain = queries(dim, 6, 9301)
    q = np.stack([q_adv, plain[0], -q_adv, plain[1], plain[3], plain[4]])       # plain[1]: the NaN query
    d_q = torch.from_numpy(q).cuda()
    rows = adversarial_corpus(rng, sign, 1500, 2.0 ** -5, 1.05 * 2.0 ** -5)
    n = len(rows)
    a, ref = pair(monkeypatch, torch, rows, metric)
    top = float(ref.search_batch(q[:1], 1)[1][0, 0])
    assert 0.5 < top < 1.0
    words = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    words[: len(words) // 3] = 0                                   # tiles 0..3 of 12: workgroups with nothing to score
    two = np.zeros_like(words); two[40] = 1 << 17; two[-1] = 1     # rows 1297 and 2976
    keeps = [torch.from_numpy(w.view(np.int32)).cuda() for w in (words, two, np.zeros_like(words))]
    adv_fb = 0
    for k in (1, 20, CAP):
        before = fallbacks(a)
        for j in (0, 2):                                                      # (the gate opens on the certificate itself, or not)
            assert_same_dev(torch, a, ref, d_q[j:j + 1], k, ("adv alone", k, j))
        adv_fb += fallbacks(a) - before
        for q0, nb in ((0, 4), (2, 2), (3, 1), (0, 6)):                       # each block holds the NaN query
            ctx = (str(metric), k, q0, nb)
            before = fallbacks(a)
            assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], k, ctx)
            for thr in (0.0, top - 2e-3, 1.5):
                ka, ca = assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], k, ctx + (thr,), mode=_lib.MODE_PIPELINE, threshold=thr)
                assert thr < 1.0 or not ca.any()
            for i, d_keep in enumerate(keeps):
                ka, ca = assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], k, ctx + ("keep", i), d_keep=d_keep)
                assert (ca <= (n, 2, 0)[i]).all()
            assert_same_dev(torch, a, ref, d_q[q0:q0 + nb], k, ctx, d_keep=keeps[0], mode=_lib.MODE_PIPELINE, threshold=top - 2e-3)
            assert fallbacks(a) - before >= 8, ctx
    assert adv_fb > 0                                              # the crowded pairs defeat the certificate at some k
    # one bitset per query: the host API's table form, which keeps the scan + select
    tabs = np.stack([words, two, words ^ np.uint32(0xFFFFFFFF)])
    for k in (20, CAP):
        ra, sa, ca = a.search_batch_filtered(q[[0, 2, 4]], k, tabs)
        rb, sb, cb = ref.search_batch_filtered(q[[0, 2, 4]], k, tabs)
        assert np.array_equal(ca, cb) and np.array_equal(ra, rb) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    assert_same_host(a, ref, q[[0, 2, 4]], 20, "host")
    a.close(); ref.close()


def test_200_searches_back_to_back(hip, monkeypatch, torch):
    """No host sync between 200 searches at 20 000 rows, certified and forced-fallback blocks alternating: the tickets are
    re-armed by every open launch, and the hand-off scratch is reused while the previous search's words are still in the
    caches of the CUs that read them."""
    n, dim, pool = 20_000, 768, 64
    d_rows = unit_rows_on_device(torch, n, dim, 9400)
    good = synth.gaussian_unit(pool, dim=dim, seed=9401)
    d_good = torch.from_numpy(good).cuda()
    d_bad = torch.from_numpy(np.ascontiguousarray(good * BIG)).cuda()      # every query: B_q = +inf
    a, ref = pair(monkeypatch, torch, d_rows)
    shapes = [(1, 20), (3, 1), (8, CAP), (2, 20), (5, 7), (4, CAP), (1, 1), (8, 20)]
    searches = []
    for i in range(200):
        nb, k = shapes[(i // 2) % len(shapes)]
        searches.append((d_bad if i % 2 else d_good, (i * 11) % (pool - 8), nb, k))
    want = [dev_search(torch, ref, src[q0:q0 + nb], k) for src, q0, nb, k in searches]
    torch.cuda.synchronize()
    got = [dev_search(torch, a, src[q0:q0 + nb], k) for src, q0, nb, k in searches]
    torch.cuda.synchronize()
    for i, ((kg, cg), (kw, cw)) in enumerate(zip(got, want)):
        assert torch.equal(cg, cw), (i, searches[i][1:], cg.tolist(), cw.tolist())
        assert torch.equal(kg, kw), (i, searches[i][1:])
    _, cert, fb = a.bf16_stats()
    assert cert + fb == sum(nb for _, _, nb, _ in searches)
    assert fb >= sum(nb for i, (_, _, nb, _) in enumerate(searches) if i % 2) and cert > 0
    a.close(); ref.close()


def test_two_streams_and_host_searches(hip, monkeypatch, torch):
    """Two caller streams by turns with host searches between them: the handle orders the searches, each after every user of
    the hand-off scratch and its tickets."""
    n, dim = 20_000, 768
    d_rows = unit_rows_on_device(torch, n, dim, 9500)
    q = queries(dim, 16, 9501)
    d_q = torch.from_numpy(q).cuda()
    a, ref = pair(monkeypatch, torch, d_rows)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    blocks = [(0, 3, 20), (3, 2, 20), (2, 1, CAP), (4, 8, 1), (1, 2, 20), (8, 4, CAP), (0, 8, 20), (2, 1, 1)]
    want = [dev_search(torch, ref, d_q[q0:q0 + nb], k) for q0, nb, k in blocks]
    torch.cuda.synchronize()
    got = []
    for i, (q0, nb, k) in enumerate(blocks):
        got.append(dev_search(torch, a, d_q[q0:q0 + nb], k, stream=(s1, s2)[i % 2]))
        if i % 3 == 2:
            assert_same_host(a, ref, q[4:7], k, ("host between", i))
    torch.cuda.synchronize()
    for i, ((kg, cg), (kw, cw)) in enumerate(zip(got, want)):
        assert torch.equal(cg, cw), (blocks[i], cg.tolist(), cw.tolist())
        assert torch.equal(kg, kw), blocks[i]
    assert fallbacks(a) >= 6
    a.close(); ref.close()


def test_switch_off_against_on(hip, monkeypatch, torch):
    """CQS_HIP_FALLBACK_ONE_LAUNCH=0 (the gated scan + select) against the default: identical bytes, open and closed gates."""
    n, dim = 20_000, 768
    d_rows = unit_rows_on_device(torch, n, dim, 9600)
    q = queries(dim, 8, 9601)
    d_q = torch.from_numpy(q).cuda()
    on, ref = pair(monkeypatch, torch, d_rows)
    off, ref2 = pair(monkeypatch, torch, d_rows, switch="0")
    ref2.close()
    for k in (1, 20, CAP, CAP + 1):
        for q0, nb in ((3, 1), (2, 1), (0, 3), (0, 8), (3, 5)):
            assert_same_dev(torch, on, off, d_q[q0:q0 + nb], k, ("switch", k, q0, nb))
            assert_same_dev(torch, on, ref, d_q[q0:q0 + nb], k, ("ref", k, q0, nb))
    c_off, f_off = off.bf16_stats()[1:]
    assert on.bf16_stats()[1:] == (2 * c_off, 2 * f_off) and f_off > 0      # (`on` ran every search twice: same verdicts)
    on.close(); off.close(); ref.close()
