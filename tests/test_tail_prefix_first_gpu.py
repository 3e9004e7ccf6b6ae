"""Prefix first: where the int8 copy's k' leaves room for a proper prefix, the tail kernel's workgroups select and rescore
the certificate's prefix alone (6k + 40 candidates), and the finisher does the rest by itself only where the prefix does not
certify (scan_bf16.hip, rescore_certify_kernel; tail_plan.h; DESIGN.md §3.11, "Prefix first").

Three handles over the same rows, built with CQS_HIP_SCAN_BF16=1 CQS_HIP_SCAN_I8=1 so that small corpora take the int8 chain:
`on` (CQS_HIP_TAIL_PREFIX_FIRST=1), `off` (=0: every workgroup selects k' + 1 and the query's waves rescore all k', the
parent's tail) and `f32` (both copies off, the exact reference).  After every `search_device`: counts and keys in every one of
the k slots equal in all three; the verdicts, both prefix counters (cqs_hip_debug_tail_verdicts) and the certified / fallback
counts of both copies equal between `on` and `off`.  Which branch a planted query takes is read off `off`'s counters here and
proved on the CPU in test_tail_prefix_first_cpu.py.  Shapes are small: each case takes seconds.  Run on an MI355X with
`pytest -m gpu`."""
import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth
from tail_first_cases import CROWDS, K, WANT, planted
from test_shadow_tail_gpu import dev_search, setenv
from test_tail_prefix_gpu import tickets, verdicts

pytestmark = pytest.mark.gpu
ENV_SWITCH = "CQS_HIP_TAIL_PREFIX_FIRST"
BS = (1, 3, 4)
KS = (1, 20, 50, 87)


@pytest.fixture
def torch():
    import torch as t
    return t


def trio(monkeypatch, torch, rows, metric=DistanceMetric.Cosine):
    """(on, off, f32) over one device buffer."""
    d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    n, dim = d.shape
    made = []
    for shadow, switch in (("1", "1"), ("1", "0"), ("0", None)):
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


def same(torch, hs, d_q, k, ctx, **kw):
    """One search on each handle, everything the two arms must agree on.  Returns (cert, the prefix counters) of `off`."""
    on, off, f32 = hs
    res = [dev_search(torch, h, d_q, k, **kw) for h in hs]
    torch.cuda.synchronize()
    (k1, c1), (k0, c0), (kf, cf) = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in res]
    assert np.array_equal(c1, c0) and np.array_equal(c1, cf), (ctx, c1, c0, cf)
    assert k1.tobytes() == k0.tobytes(), (ctx, "on / off")
    assert k1.tobytes() == kf.tobytes(), (ctx, "on / f32")
    b = d_q.shape[0]
    cert1, pre1 = verdicts(on, b)
    cert0, pre0 = verdicts(off, b)
    assert np.array_equal(cert1, cert0), (ctx, cert1, cert0)
    assert pre1 == pre0, (ctx, pre1, pre0)
    assert on.bf16_stats()[1:] == off.bf16_stats()[1:], (ctx, on.bf16_stats(), off.bf16_stats())
    assert on.i8_stats()[1:] == off.i8_stats()[1:], (ctx, on.i8_stats(), off.i8_stats())
    return cert0, pre0


def close(hs):
    for h in hs:
        assert not tickets(h).any() if h.bf16_stats()[0] else True
        h.close()


@pytest.fixture(scope="module")
def planted_rows():
    return planted()


@pytest.mark.parametrize("dim", [8, 768])
@pytest.mark.parametrize("n", [100, 300, 4097, 20_000])
def test_fast_path_shapes_raw_and_pipeline(hip, monkeypatch, torch, n, dim):
    """Gaussian unit rows: the prefix certifies (dim 768, the int8 copy) or no proper prefix exists (dim 8: the bf16 copy alone;
    n = 100 at k >= 20: fewer rows than tier 1 asks for).  PIPELINE at two thresholds drops the best rows once exact."""
    rows = synth.gaussian_unit(n, dim=dim, seed=9700 + n + dim)
    qs = synth.gaussian_unit(8, dim=dim, seed=9750 + dim)
    d_q = torch.from_numpy(qs).cuda()
    hs = trio(monkeypatch, torch, rows)
    top = float(hs[2].search_batch(qs[:1], 1)[1][0, 0])
    for j, nb in enumerate(BS):
        for k in KS:
            q0 = (j + k) % 4
            before = verdicts(hs[1], 1)[1]
            cert, pre = same(torch, hs, d_q[q0:q0 + nb], k, (n, dim, nb, k))
            proper = dim % 16 == 0 and n > 6 * k + 40
            assert sum(pre) - sum(before) == (nb if proper else 0), (n, dim, nb, k, before, pre)
            if proper and k <= 20:                         # (as in test_tail_prefix_gpu.py: these certify on the prefix, every one)
                assert cert.all() and pre == (before[0] + nb, before[1]), (n, dim, nb, k, before, pre)
            for thr in (min(max(top, 0.0), 1.0), max(top * 0.8, 0.0)):
                same(torch, hs, d_q[q0:q0 + nb], k, (n, dim, nb, k, thr), mode=_lib.MODE_PIPELINE, threshold=thr)
    close(hs)


def test_planted_branches_one_by_one_and_side_by_side(hip, monkeypatch, torch, planted_rows):
    """The planted corpus: a query whose prefix fails and whose k' certify, one whose k' fail too (the gated fallback answers:
    its counter rises by exactly one), and two that certify on the prefix - alone, then in one block, then at other k."""
    rows, q = planted_rows
    hs = trio(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    for qi, want in enumerate(WANT):
        before, fb_before = verdicts(hs[1], 1)[1], [h.bf16_stats()[2] for h in hs[:2]]
        cert, pre = same(torch, hs, d_q[qi:qi + 1], K, ("planted", qi, CROWDS[qi]))
        for h, fb0 in zip(hs[:2], fb_before):              # (same() held cert and the prefix counters equal on both arms)
            got = (int(cert[0]), pre[0] - before[0], pre[1] - before[1], h.bf16_stats()[2] - fb0)
            assert got == {"fast": (1, 1, 0, 0), "slow": (1, 0, 1, 0), "fallback": (0, 0, 1, 1)}[want], (qi, want, got)
    before, fb_before = verdicts(hs[1], 1)[1], [h.bf16_stats()[2] for h in hs[:2]]
    cert, pre = same(torch, hs, d_q, K, "all four in one block")
    assert cert.tolist() == [1, 0, 1, 1] and (pre[0] - before[0], pre[1] - before[1]) == (2, 2)
    assert [h.bf16_stats()[2] - fb0 for h, fb0 in zip(hs[:2], fb_before)] == [1, 1]
    for k in (1, 19, 21, 50, 87):
        for q0, nb in ((0, 1), (1, 1), (0, 3), (1, 3), (0, 4)):
            same(torch, hs, d_q[q0:q0 + nb], k, ("planted", k, q0, nb))
    thr = 0.893                                            # PIPELINE between the planted rows and their crowds, and under both
    for t in (thr, 0.5):
        for q0, nb in ((0, 1), (1, 1), (0, 4)):
            same(torch, hs, d_q[q0:q0 + nb], K, ("planted pipeline", t, q0, nb), mode=_lib.MODE_PIPELINE, threshold=t)
    close(hs)


def test_fewer_candidates_than_tier_one_asks_for(hip, monkeypatch, torch, planted_rows):
    """A keep-bitset leaving 50 rows of 20 000: every valid row is a candidate and is rescored in tier 1; rule (a), one sort, no
    prefix tried.  Then 161 and 162 rows kept at k = 20: the smallest counts with a proper prefix."""
    rows, q = planted_rows
    n = rows.shape[0]
    hs = trio(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    rng = np.random.default_rng(9901)
    for kept in (50, 160, 161, 162):
        words = np.zeros((n + 31) // 32, dtype=np.uint32)
        for r in rng.choice(n, kept, replace=False):
            words[r // 32] |= np.uint32(1 << (r % 32))
        d_keep = torch.from_numpy(words.view(np.int32)).cuda()
        for k in KS:
            for nb in BS:
                before = verdicts(hs[1], 1)[1]
                cert, pre = same(torch, hs, d_q[:nb], k, ("kept", kept, k, nb), d_keep=d_keep)
                if kept <= 10 * k + 150:                   # rule (a): every kept row was rescored
                    assert cert.all()
                assert sum(pre) - sum(before) == (nb if kept > 6 * k + 40 else 0), (kept, k, nb, before, pre)
    close(hs)


def test_nan_rows_infinite_bound_and_tied_rows(hip, monkeypatch, torch):
    """Rows with NaN, a query whose B_q is +inf beside others, and 5 000 identical rows at the top of a query: the threshold
    bin holds all of them in both tiers' selects, no prefix and no k' can certify a tie, the fallback answers."""
    dim, n = 768, 20_000
    rows = synth.gaussian_unit(n, dim=dim, seed=9911)
    q = synth.gaussian_unit(6, dim=dim, seed=9912)
    rows[5, 7] = np.nan
    rows[4096, 0] = np.nan
    rows[n - 1, dim - 1] = np.nan
    v = q[3] * 2.0 + rows[7000]
    rows[7000:12_000] = (v / np.linalg.norm(v)).astype(np.float32)
    q[2] *= np.float32(2e30)
    hs = trio(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    for k in KS:
        for q0, nb in ((0, 1), (2, 1), (3, 1), (0, 4), (2, 3), (3, 3)):
            cert, _ = same(torch, hs, d_q[q0:q0 + nb], k, ("odd", k, q0, nb))
            for c, i in zip(cert.tolist(), range(q0, q0 + nb)):
                assert c == 0 or i not in (2, 3), (k, q0, nb, cert)     # (the others may have the tied rows among their candidates)
    close(hs)


def agree_after_unsynchronised(torch, hs, d_q, last):
    """After a run with no sync on both arms: what the device accumulated must agree (both prefix counters, the certified /
    fallback counts of both copies: a verdict that differed in any search shows in them), and the verdicts of the last
    search (the cert words are the handle's: only the last search's can be read)."""
    on, off, _ = hs
    (c1, p1), (c0, p0) = verdicts(on, last), verdicts(off, last)
    assert np.array_equal(c1, c0) and p1 == p0, (c1, c0, p1, p0)
    assert on.bf16_stats()[1:] == off.bf16_stats()[1:] and on.i8_stats()[1:] == off.i8_stats()[1:]
    assert not tickets(on).any() and not tickets(off).any()
    return p1


def test_200_unsynchronised_searches_leave_the_tickets_at_zero(hip, monkeypatch, torch, planted_rows):
    """Fast-path and slow-path queries by turns, back to back with no sync; then the ticket words read back as 0.  The cert
    words of a search are overwritten by the next, so each distinct search of the plan is then repeated with a sync and its
    verdicts compared one by one."""
    rows, q = planted_rows
    hs = trio(monkeypatch, torch, rows)
    on, off, f32 = hs
    d_q = torch.from_numpy(q).cuda()
    plan = [((0, 1), (2, 1), (1, 1), (3, 1), (0, 4), (2, 2), (1, 3))[i % 7] + ((20, 1, 50, 20, 87)[i % 5],) for i in range(200)]
    want = [dev_search(torch, f32, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    torch.cuda.synchronize()
    got = [dev_search(torch, on, d_q[q0:q0 + nb], k) for q0, nb, k in plan]          # back to back: no sync
    got0 = [dev_search(torch, off, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    torch.cuda.synchronize()
    for i, ((kg, cg), (k0, c0), (kw, cw)) in enumerate(zip(got, got0, want)):
        assert torch.equal(cg, cw) and torch.equal(kg, kw) and torch.equal(c0, cw) and torch.equal(k0, kw), (i, plan[i])
    pre = agree_after_unsynchronised(torch, hs, d_q, plan[-1][1])
    assert pre[1] > 20, pre                                 # (the slow path did run)
    for q0, nb, k in sorted(set(plan)):
        same(torch, hs, d_q[q0:q0 + nb], k, ("replayed", q0, nb, k))
    close(hs)


def test_two_streams_with_a_host_search_between(hip, monkeypatch, torch, planted_rows):
    """Device searches on two streams by turns with a host search after each, no sync, on both arms; then as above."""
    rows, q = planted_rows
    hs = trio(monkeypatch, torch, rows)
    on, off, f32 = hs
    d_q = torch.from_numpy(q).cuda()
    steps = [((0, 1, 20), (2, 2, 20), (1, 1, 50), (0, 4, 20), (3, 1, 1), (1, 3, 87))[j % 6] for j in range(12)]
    want_dev = [dev_search(torch, f32, d_q[i:i + nb], k) for i, nb, k in steps]
    want_host = [f32.search_batch(q[j % 4], 20) for j in range(12)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for h in (on, off):
        got_dev, got_host = [], []
        for j, (i, nb, k) in enumerate(steps):
            got_dev.append(dev_search(torch, h, d_q[i:i + nb], k, stream=s1 if j % 2 == 0 else s2))   # no sync: the handle orders the scratch
            got_host.append(h.search_batch(q[j % 4], 20))
        torch.cuda.synchronize()
        for (kg, cg), (kw, cw) in zip(got_dev, want_dev):
            assert torch.equal(kg, kw) and torch.equal(cg, cw)
        for (rg, sg, cg), (rw, sw, cw) in zip(got_host, want_host):
            assert np.array_equal(cg, cw) and np.array_equal(rg, rw) and np.array_equal(sg.view(np.uint32), sw.view(np.uint32))
    # (both arms ran the same launches in the same order: whichever search wrote the first cert word last, it is the same one)
    pre = agree_after_unsynchronised(torch, hs, d_q, 1)
    assert pre[1] > 0, pre
    for i, nb, k in sorted(set(steps)):
        same(torch, hs, d_q[i:i + nb], k, ("replayed", i, nb, k))
    close(hs)
