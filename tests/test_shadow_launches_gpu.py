"""A certified shadow search in three launches: the select of the k' + 1 approximate keys runs inside the tail kernel (every
workgroup of a query selects for itself: scan_bf16.hip, rescore_certify_kernel calling select_device.h), and the gated f32
scan behind it is launched on the persistent grid (scan_kernels.hip, launch_gemv).

As in test_shadow_tail_gpu.py every comparison is between a handle with the shadow (both copies) and a CQS_HIP_SCAN_BF16=0
handle over the same rows: identical counts and identical keys in every one of the k slots through `search_device`,
identical rows and score bits through the host searches.  The cases aim at what this change adds: the select's front end
and its radix fallback run by up to 64 workgroups per query at once, waves that rescore several candidates each (blocks whose
workgroups would not fit the device in one round), the work-queue heads zeroed by the tail kernel and then advanced by an
open-gated f32 scan that dequeues from them, and open and closed gates by turns.  Every input is an ordinary in-bounds
search.  Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest

from cqs_amd import DistanceMetric, _lib, synth
from test_shadow_tail_gpu import (COMBOS, assert_same_dev, assert_same_host, dev_pair, dev_search, plan, served,
                                  unit_rows_on_device)

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch():
    import torch as t
    return t


@pytest.mark.parametrize("metric", [DistanceMetric.Cosine, DistanceMetric.DotProduct])
@pytest.mark.parametrize("n", [1_000_000, 20_000])
def test_every_shape_both_apis(hip, monkeypatch, torch, n, metric):
    """b x k through both APIs, RAW and PIPELINE with thresholds around the top score, with and without a bitset."""
    dim, pool = 768, 40
    d_rows = unit_rows_on_device(torch, n, dim, 8000 + n)
    if metric == DistanceMetric.DotProduct:                      # rows of many lengths: raw dot products, log-spaced bins
        g = torch.Generator(device="cuda"); g.manual_seed(8001)
        d_rows *= torch.empty((n, 1), device="cuda").uniform_(0.1, 30.0, generator=g)
    qs = synth.gaussian_unit(pool, dim=dim, seed=8100 + (n % 1000))
    d_qs = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, d_rows, metric, policy=(None, None) if n >= 1_000_000 else ("1", "1"))
    rng = np.random.default_rng(8002)
    words = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)     # about half the rows
    words[: len(words) // 3] = 0                                  # and whole tasks with no row to score
    d_keep = torch.from_numpy(words.view(np.int32)).cuda()
    top = float(b.search_batch(qs[:1], 1)[1][0, 0])
    thr_top = min(max(top, 0.0), 1.0)
    for j, (nb, k) in enumerate(COMBOS):
        q0 = (j * 5) % (pool - 8)
        ctx = (n, str(metric), nb, k)
        assert_same_dev(torch, a, b, d_qs[q0:q0 + nb], k, ctx)
        assert_same_dev(torch, a, b, d_qs[q0:q0 + nb], k, ctx, d_keep=d_keep)
        for thr in (0.0, thr_top * 0.5, thr_top):
            assert_same_dev(torch, a, b, d_qs[q0:q0 + nb], k, ctx + (thr,), mode=_lib.MODE_PIPELINE, threshold=thr)
        assert_same_dev(torch, a, b, d_qs[q0:q0 + nb], k, ctx, d_keep=d_keep, mode=_lib.MODE_PIPELINE, threshold=thr_top * 0.25)
        assert_same_host(a, b, qs[q0:q0 + nb], k, ctx)
        assert_same_host(a, b, qs[q0:q0 + nb], k, ctx, keep_bitset=words)
        assert_same_host(a, b, qs[q0:q0 + nb], k, ctx, mode=_lib.MODE_PIPELINE, threshold=thr_top * 0.5)
    issued = sum(nb for nb, _ in COMBOS) * 9
    _, cert, fb = a.bf16_stats()
    assert cert + fb == issued and cert > 0, (cert, fb, issued)
    a.close(); b.close()


@pytest.mark.parametrize("n", [1_000_000, 20_000])
def test_200_searches_back_to_back(hip, monkeypatch, torch, n):
    """No host sync between 200 searches of changing (b, k): tickets re-armed, work-queue heads re-zeroed by each tail
    launch, every workgroup's select reading what the scan of THIS search wrote while the last search's lines are hot."""
    dim, pool = 768, 64
    d_rows = unit_rows_on_device(torch, n, dim, 8200 + n)
    d_qs = torch.from_numpy(synth.gaussian_unit(pool, dim=dim, seed=8300 + (n % 1000))).cuda()
    a, b = dev_pair(monkeypatch, torch, d_rows, policy=(None, None) if n >= 1_000_000 else ("1", "1"))
    searches = plan(200, pool)
    want = [dev_search(torch, b, d_qs[q0:q0 + nb], k) for q0, nb, k in searches]
    torch.cuda.synchronize()
    got = [dev_search(torch, a, d_qs[q0:q0 + nb], k) for q0, nb, k in searches]
    torch.cuda.synchronize()
    for i, ((kg, cg), (kw, cw)) in enumerate(zip(got, want)):
        assert torch.equal(cg, cw), (n, i, searches[i], cg.tolist(), cw.tolist())
        assert torch.equal(kg, kw), (n, i, searches[i])
    _, cert, fb = a.bf16_stats()
    _, cert8, fb8 = a.i8_stats()
    assert cert + fb == sum(served(nb, k)[0] for _, nb, k in searches), (cert, fb)
    assert cert8 + fb8 == sum(served(nb, k)[1] for _, nb, k in searches), (cert8, fb8)
    assert cert > 0 and cert8 > 0
    a.close(); b.close()


@pytest.mark.parametrize("n", [1_000_000, 300_000, 20_000])
def test_open_and_closed_gates_by_turns(hip, monkeypatch, torch, n):
    """Queries that cannot be certified (a NaN query, a B_q = +inf query) beside certified ones in one block, and blocks of
    either kind one after the other with no sync.  At 300 000 and 1M rows the open-gated f32 scan runs on the persistent grid
    and dequeues from the heads the tail kernel has just zeroed; the closed-gated one must leave them alone."""
    dim = 768
    d_rows = unit_rows_on_device(torch, n, dim, 8400 + n)
    q = synth.gaussian_unit(16, dim=dim, seed=8401)
    q[1, 7] = np.nan
    q[2] *= np.float32(2e30)             # ||q|| max||x|| past 2^100: B_q = +inf, every score still finite in f32
    q[9] *= np.float32(2e30)
    d_q = torch.from_numpy(q).cuda()
    a, b = dev_pair(monkeypatch, torch, d_rows, policy=("1", "1"))
    # (first query, b): blocks with 0, 1 or 2 uncertifiable queries; b = 3 is two f32 passes, b = 5 and 8 the 8-query pass
    blocks = [(3, 1), (0, 4), (4, 4), (2, 1), (3, 2), (1, 3), (4, 5), (8, 8), (0, 8), (10, 3), (9, 1), (12, 4), (2, 2), (5, 3)]
    bad = {1, 2, 9}
    issued = want_fb = 0
    for k in (1, 20, 88, 500):
        steps = [(q0, nb, k) for q0, nb in blocks]
        want = [dev_search(torch, b, d_q[q0:q0 + nb], k) for q0, nb, _ in steps]
        torch.cuda.synchronize()
        got = [dev_search(torch, a, d_q[q0:q0 + nb], k) for q0, nb, _ in steps]       # back to back: no sync
        torch.cuda.synchronize()
        for i, ((kg, cg), (kw, cw)) in enumerate(zip(got, want)):
            assert torch.equal(cg, cw), (n, k, steps[i], cg.tolist(), cw.tolist())
            assert torch.equal(kg, kw), (n, k, steps[i])
        issued += sum(nb for _, nb in blocks)
        want_fb += sum(len(bad & set(range(q0, q0 + nb))) for q0, nb in blocks)
    _, cert, fb = a.bf16_stats()
    assert cert + fb == issued and fb >= want_fb and cert > 0, (cert, fb, issued, want_fb)
    a.close(); b.close()


def test_adversarial_rows_beside_certified_queries(hip, monkeypatch, torch):
    """The half-ulp adversarial corpus of test_bf16_scan_gpu.py: two queries it is built against share blocks with plain
    ones, block after block."""
    from test_bf16_scan_gpu import adversarial_corpus
    rng = np.random.default_rng(8501)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    plain = list(synth.gaussian_unit(6, seed=8502))
    qs = np.stack([plain[0], q_adv, plain[1], -q_adv] + plain[2:])
    d_qs = torch.from_numpy(qs).cuda()
    rows = adversarial_corpus(rng, sign, 1500, 2.0 ** -5, 1.05 * 2.0 ** -5)
    a, b = dev_pair(monkeypatch, torch, rows)
    issued = 0
    for k in (1, 20, 100, 500):
        for q0, nb in ((0, 4), (4, 4), (0, 8), (1, 1), (4, 1), (0, 3), (2, 2), (4, 3)):
            assert_same_dev(torch, a, b, d_qs[q0:q0 + nb], k, ("adv", k, q0, nb))
            issued += nb
    _, cert, fb = a.bf16_stats()
    assert cert + fb == issued and fb > 0, (cert, fb, issued)
    a.close(); b.close()


def test_heavy_ties_and_a_crowded_threshold_bin(hip, monkeypatch, torch):
    """The select's radix fallback from inside the tail kernel.  (a) 12 000 copies of one row hold the top score: more
    entries in the threshold bin than the sort block takes, all tied, so the order is by row alone.  (b) 150 rows close to
    the query above a crowd of 12 000 copies of a farther row: the (k' + 1)-th approximate key sits in the crowd, the top k
    does not, and the answer can still be certified."""
    dim, n = 768, 40_000
    rng = np.random.default_rng(8601)
    base = synth.gaussian_unit(n, dim=dim, seed=8602)
    qs = synth.gaussian_unit(4, dim=dim, seed=8603)

    def unit(v):
        return (v / np.linalg.norm(v)).astype(np.float32)

    # (a) the tied rows are the best ones for qs[0]
    rows = base.copy()
    rows[1::3][:12_000] = unit(qs[0] + 0.5 * base[0])
    d_q = torch.from_numpy(qs).cuda()
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 20, 87, 200, 500, 1000):
        for nb in (1, 3, 4, 8):
            assert_same_dev(torch, a, b, d_q[:nb], k, ("ties", k, nb))
        assert_same_host(a, b, qs[:2], k, ("ties host", k))
    a.close(); b.close()

    # (b) the crowd is below the near rows
    rows = base.copy()
    rows[2::3][:12_000] = unit(0.35 * qs[0] + base[1])
    near = rng.choice(np.arange(0, n, 3), 150, replace=False)
    for j, r in enumerate(near):
        rows[r] = unit(qs[0] * (1.5 + 0.01 * j) + base[r])
    a, b = dev_pair(monkeypatch, torch, rows)
    for k in (1, 20, 40, 87, 200):          # k' + 1 = 2k + 33 or the int8 copy's own k': past the 150 near rows from k = 87 at the latest
        for nb in (1, 2, 4):
            assert_same_dev(torch, a, b, d_q[:nb], k, ("crowd", k, nb))
        assert_same_host(a, b, qs[:1], k, ("crowd host", k))
    _, cert, fb = a.bf16_stats()
    assert cert + fb == 5 * (1 + 2 + 4 + 1) and cert > 0, (cert, fb)
    a.close(); b.close()
