"""The int8 shadow scan publishes one (maximum, argmax, runner-up) triple per workgroup of four consecutive tasks, and the
tail kernel's select walks those groups (scan_i8.hip, group_map.h, select_device.h; DESIGN.md §3.11, "Workgroup maxima").

Four handles over the same rows, both copies built at any size (CQS_HIP_SCAN_I8=1 CQS_HIP_SCAN_BF16=1): `on`
(CQS_HIP_I8_GROUPS=1: workgroup maxima in every int8 block), `off` (CQS_HIP_I8_GROUPS=0: one maximum per task, the parent's
scan and select), `f32` (both copies off) and `dflt` (the switch unset: workgroup maxima where 4 (k' + 1)^2 <= n_pad, so at
these sizes mostly the `off` path and from 131 072 rows on the `on` path at k = 1).  After every search: counts and keys in
every one of the k slots equal in all four; the per-query verdicts `cert`, the certified / fallback counters of both copies
and the prefix counters exactly equal between `on`, `off` and `dflt`.

Sizes are the smallest at which each piece of geometry exists on a 256-CU device: 16-row tasks (n < 131 072: a group is 64
rows), 64-row tasks (a group is 256 rows), and from 393 216 rows the 32-row tier behind them.  The index pads n to 256 rows,
so on this device n_tasks is a multiple of 4 at every n; a partial last group and a group across the tier boundary are
covered device-free (test_group_map_cpu.py), and here by the rows past n that the last group's waves mask off.
Each case takes seconds.  Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth
from test_shadow_tail_gpu import dev_search, setenv
from test_tail_prefix_gpu import tickets, verdicts

pytestmark = pytest.mark.gpu
ENV_SWITCH = "CQS_HIP_I8_GROUPS"
BS = (1, 2, 3, 4)
KS = (1, 20, 87)


@pytest.fixture
def torch():
    import torch as t
    return t


def trio(monkeypatch, torch, rows, metric=DistanceMetric.Cosine):
    """(on, off, f32, dflt) over one device buffer."""
    d = rows if hasattr(rows, "data_ptr") else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    n, dim = d.shape
    made = []
    for shadow, switch in (("1", "1"), ("1", "0"), ("0", None), ("1", None)):
        setenv(monkeypatch, shadow, shadow)
        if switch is None:
            monkeypatch.delenv(ENV_SWITCH, raising=False)
        else:
            monkeypatch.setenv(ENV_SWITCH, switch)
        made.append(HipIndex.build_from_device(None, d.data_ptr(), n, dim, metric, borrow=True, keepalive=d))
    setenv(monkeypatch, None, None)
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    on, off, f32, dflt = made
    for h in (on, off, dflt):
        assert h.bf16_stats()[0] == n * dim * 2 and h.i8_stats()[0] == n * dim + n * 4, h.last_error()
    assert f32.bf16_stats()[0] == 0 and f32.i8_stats()[0] == 0
    return on, off, f32, dflt


def same(torch, hs, d_q, k, ctx, **kw):
    """One device search on each handle.  Returns (`on`'s keys, `on`'s cert array)."""
    on, off, f32, dflt = hs
    res = [dev_search(torch, h, d_q, k, **kw) for h in hs]
    torch.cuda.synchronize()
    (k1, c1), (k0, c0), (kf, cf), (kd, cd) = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in res]
    assert np.array_equal(c1, c0) and np.array_equal(c1, cf) and np.array_equal(c1, cd), (ctx, c1, c0, cf, cd)
    assert np.array_equal(k1, k0), (ctx, "on / off")
    assert np.array_equal(k1, kf), (ctx, "on / f32")
    assert np.array_equal(k1, kd), (ctx, "on / dflt")
    b = d_q.shape[0]
    cert1, pre1 = verdicts(on, b)
    for name, h in (("off", off), ("dflt", dflt)):
        cert0, pre0 = verdicts(h, b)
        assert np.array_equal(cert1, cert0), (ctx, name, cert1, cert0)
        assert pre1 == pre0, (ctx, name, pre1, pre0)
        assert on.bf16_stats()[1:] == h.bf16_stats()[1:], (ctx, name, on.bf16_stats(), h.bf16_stats())
        assert on.i8_stats()[1:] == h.i8_stats()[1:], (ctx, name, on.i8_stats(), h.i8_stats())
    return k1, cert1


def same_host(hs, call, ctx):
    """One host search on each handle (`call(h)` -> rows, scores, counts): equal rows, score bits and counts in all four."""
    (r1, s1, c1), others = call(hs[0]), [call(h) for h in hs[1:]]
    for r0, s0, c0 in others:
        assert np.array_equal(c1, c0), (ctx, c1, c0)
        for i, c in enumerate(c1):
            assert np.array_equal(r1[i, :c], r0[i, :c]), (ctx, i)
            assert np.array_equal(s1[i, :c].view(np.uint32), s0[i, :c].view(np.uint32)), (ctx, i)
    on, off, _, dflt = hs
    assert on.bf16_stats()[1:] == off.bf16_stats()[1:] == dflt.bf16_stats()[1:], ctx
    assert on.i8_stats()[1:] == off.i8_stats()[1:] == dflt.i8_stats()[1:], ctx
    return r1, c1


def key_rows(keys):
    return (0xFFFFFFFF - (keys.astype(np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)


def close(hs):
    for h in hs:
        assert not tickets(h).any() if h.bf16_stats()[0] else True
        h.close()


def sweep(torch, hs, d_q, top, ctx):
    """Every block size and k, RAW and PIPELINE at three thresholds around the best score."""
    issued = 0
    for j, nb in enumerate(BS):
        for k in KS:
            q0 = (3 * j + k) % 8
            same(torch, hs, d_q[q0:q0 + nb], k, ctx + (nb, k))
            for thr in (min(max(top, 0.0), 1.0), max(top * 0.8, 0.0), 0.0):
                same(torch, hs, d_q[q0:q0 + nb], k, ctx + (nb, k, thr), mode=_lib.MODE_PIPELINE, threshold=thr)
            issued += 4 * nb
    _, cert, fb = hs[0].bf16_stats()
    assert cert + fb == issued, (cert, fb, issued)
    assert hs[0].i8_stats()[1] + hs[0].i8_stats()[2] == issued, "every block of <= 4 queries at k <= 87 goes through the int8 copy"


def device_rows(torch, n, dim, seed):
    """Gaussian unit rows made on the device (the large corpora: seconds of host time otherwise)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    r = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
    return r / r.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("metric", [DistanceMetric.Cosine, DistanceMetric.DotProduct])
@pytest.mark.parametrize("dim", [16, 768, 2048])
@pytest.mark.parametrize("n", [3, 255, 257, 4097])
def test_small_corpora_16_row_tasks(hip, monkeypatch, torch, n, dim, metric):
    rows = synth.gaussian_unit(n, dim=dim, seed=9700 + n + dim)
    if metric is DistanceMetric.DotProduct:
        rows = rows * np.linspace(0.5, 3.0, n, dtype=np.float32)[:, None]      # raw dot products: the log-spaced bins
    qs = synth.gaussian_unit(12, dim=dim, seed=9750 + dim)
    hs = trio(monkeypatch, torch, rows, metric)
    top = float(hs[2].search_batch(qs[:1], 1)[1][0, 0])
    sweep(torch, hs, torch.from_numpy(qs).cuda(), top, (n, dim, metric.name))
    close(hs)


@pytest.mark.parametrize("n,dim", [(131_072 + 64, 768), (131_072 + 128, 16), (131_072 + 192, 16), (393_216 + 64, 16)])
def test_64_row_tasks_and_the_32_row_tier(hip, monkeypatch, torch, n, dim):
    d = device_rows(torch, n, dim, 9800 + n % 1000 + dim)
    qs = synth.gaussian_unit(12, dim=dim, seed=9850 + dim)
    hs = trio(monkeypatch, torch, d)
    top = float(hs[2].search_batch(qs[:1], 1)[1][0, 0])
    sweep(torch, hs, torch.from_numpy(qs).cuda(), top, (n, dim))
    close(hs)


def plant(rows, q, r, w):
    """Row r becomes a unit row whose cosine with q is set by w alone."""
    perp = rows[r] - np.dot(rows[r], q) * q
    perp /= np.linalg.norm(perp)
    v = q * w + perp
    rows[r] = (v / np.linalg.norm(v)).astype(np.float32)


def test_planted_rows_in_one_group(hip, monkeypatch, torch):
    """64-row tasks, groups of 256 rows.  Two of the best rows in one group but in different waves; two in one wave; a row and
    its copy that tie at a group's maximum across waves (answered in row order); the best row of all in the last group,
    whose waves mask off the rows past n."""
    n, dim = 131_072 + 64, 768
    rows = device_rows(torch, n, dim, 9901).cpu().numpy()
    q = synth.gaussian_unit(4, dim=dim, seed=9902)
    g = 256
    spots = {5 * g + 3: 3.0, 5 * g + 64 + 7: 2.9,            # one group, waves 0 and 1
             9 * g + 130: 2.8, 9 * g + 140: 2.7,             # one group, both in wave 2
             20 * g + 10: 2.6, 20 * g + 200: 2.6,            # copies: waves 0 and 3
             n - 1: 3.5}                                      # the last row of the last (partly masked) group
    for r, w in spots.items():
        plant(rows, q[0], r, w)
    rows[20 * g + 200] = rows[20 * g + 10]
    hs = trio(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    want = [n - 1, 5 * g + 3, 5 * g + 64 + 7, 9 * g + 130, 9 * g + 140, 20 * g + 10, 20 * g + 200]
    for k in KS + (7,):
        for nb in BS:
            keys, _ = same(torch, hs, d_q[:nb], k, ("planted", k, nb))
            assert key_rows(keys[0, :min(k, 7)]).tolist() == want[:min(k, 7)], (k, nb, key_rows(keys[0, :7]))
    close(hs)


def test_bitsets_that_empty_groups_and_tasks(hip, monkeypatch, torch):
    """A shared bitset (device API and host API) that empties a whole group, one task of another, and all but one row of a
    third; then per-query bitsets through the host API (the scan's PQ form), one of them empty."""
    n, dim = 131_072 + 64, 16
    d = device_rows(torch, n, dim, 9911)
    q = synth.gaussian_unit(8, dim=dim, seed=9912)
    hs = trio(monkeypatch, torch, d)
    bits = np.ones(n, bool)
    top = key_rows(same(torch, hs, torch.from_numpy(q).cuda()[:1], 20, ("bitset, before"))[0][0])
    g0 = int(top[0]) // 256
    bits[g0 * 256:(g0 + 1) * 256] = False                     # the group that held the best row: gone
    r1 = next(int(r) for r in top if int(r) // 256 != g0)
    bits[r1 // 64 * 64: r1 // 64 * 64 + 64] = False           # the one task of another group that held its best row
    bits[3 * 256: 4 * 256] = False
    bits[3 * 256 + 77] = True                                 # one row left in a group
    bits[(n // 256) * 256:] = False                           # the rows of the last group
    words = np.packbits(np.pad(bits, (0, (-n) % 32)), bitorder="little").view(np.uint32)
    d_keep = torch.from_numpy(words.view(np.int32)).cuda()
    d_q = torch.from_numpy(q).cuda()
    for k in KS:
        for nb in BS:
            keys, _ = same(torch, hs, d_q[:nb], k, ("bitset", k, nb), d_keep=d_keep)
            assert bits[key_rows(keys[keys != 0])].all()
            same_host(hs, lambda h: h.search_batch(q[:nb], k, keep_bitset=words), ("host bitset", k, nb))
    tab = np.tile(words, (4, 1))
    tab[1] = 0                                                # query 1 keeps nothing
    tab[2] = 0xFFFFFFFF                                       # query 2 keeps everything
    tab[3, : (100 * 256) // 32] = 0                           # query 3 loses the first 100 groups
    for k in KS:
        for nb in BS:
            _, counts = same_host(hs, lambda h: h.search_batch_filtered(q[:nb], k, tab[:nb]), ("per-query bitsets", k, nb))
            assert nb < 2 or counts[1] == 0
    close(hs)


def test_half_ulp_adversarial_rows(hip, monkeypatch, torch):
    """The half-ulp adversarial corpus of test_bf16_scan_gpu.py, its two queries beside plain ones."""
    from test_bf16_scan_gpu import adversarial_corpus
    rng = np.random.default_rng(9921)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    plain = list(synth.gaussian_unit(4, seed=9922))
    qs = np.stack([plain[0], q_adv, plain[1], -q_adv] + plain[2:])
    d_qs = torch.from_numpy(qs).cuda()
    hs = trio(monkeypatch, torch, adversarial_corpus(rng, sign, 1500, 2.0 ** -5, 1.05 * 2.0 ** -5))
    for k in KS:
        for q0, nb in ((0, 4), (2, 4), (1, 1), (3, 1), (0, 3), (2, 2)):
            same(torch, hs, d_qs[q0:q0 + nb], k, ("adv", k, q0, nb))
    close(hs)


def test_twelve_thousand_tied_rows(hip, monkeypatch, torch):
    """12 000 copies of one row tie above everything else: more candidates than the select's LDS list holds, so the radix
    select over the whole score row answers, in row order."""
    n, dim = 20_000, 768
    rows = synth.gaussian_unit(n, dim=dim, seed=9931)
    q = synth.gaussian_unit(4, dim=dim, seed=9932)
    rng = np.random.default_rng(9933)
    tied = np.sort(rng.choice(n, 12_000, replace=False))
    plant(rows, q[0], tied[0], 2.0)
    rows[tied] = rows[tied[0]]
    hs = trio(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    for k in KS:
        for nb in BS:
            keys, _ = same(torch, hs, d_q[:nb], k, ("tied", k, nb))
            assert key_rows(keys[0]).tolist() == tied[:k].tolist()
    close(hs)


def test_second_list_overflows_in_tasks(hip, monkeypatch, torch):
    """1 150 groups each hold two copies of one row that lies above everything else (equal codes, so equal approximate scores:
    one histogram bin): every listed group has a runner-up at the threshold bin, and their 4 600 tasks do not fit the second
    list's 4 096 slots, so the select gathers every listed group; the 2 300 candidates go through the bitonic sort and are
    answered in row order.  With one maximum per task (switch off) the same rows are 2 300 tasks at most and the list holds
    them."""
    n, dim = 80_000, 768                                       # 16-row tasks: a group is 64 rows, 1 250 groups
    rows = synth.gaussian_unit(n, dim=dim, seed=9941)
    q = synth.gaussian_unit(4, dim=dim, seed=9942)
    rng = np.random.default_rng(9943)
    hot = []
    for g in range(1150):
        a, b = rng.choice(64, 2, replace=False)
        hot += [g * 64 + int(a), g * 64 + int(b)]
    hot.sort()
    plant(rows, q[0], hot[0], 2.0)
    rows[hot] = rows[hot[0]]
    hs = trio(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    for k in (87, 20, 1):
        for nb in BS:
            keys, _ = same(torch, hs, d_q[:nb], k, ("overflow", k, nb))
            assert key_rows(keys[0]).tolist() == hot[:k]
    close(hs)


def test_uncertifiable_beside_certified_and_tickets(hip, monkeypatch, torch):
    """A NaN query and a B_q = +inf query beside certified ones: their cert is 0 in both arms, the others' 1.  Then 200
    searches with no sync, b alternating (the scan's 1-, 2- and 4-query passes back to back on the same LDS slots and the same
    gmax rows); ticket words 0 afterwards."""
    n, dim = 20_000, 768
    rows = synth.gaussian_unit(n, dim=dim, seed=9951)
    q = synth.gaussian_unit(16, dim=dim, seed=9952)
    q[1, 7] = np.nan
    q[2] *= np.float32(2e30)
    hs = trio(monkeypatch, torch, rows)
    on, off, f32, dflt = hs
    d_q = torch.from_numpy(q).cuda()
    fb_want = 0
    for k in KS:
        for q0, nb in ((0, 4), (1, 1), (2, 2), (0, 3), (3, 3)):
            _, cert = same(torch, hs, d_q[q0:q0 + nb], k, ("bad", k, q0, nb))
            want = np.array([0 if i in (1, 2) else 1 for i in range(q0, q0 + nb)], np.uint32)
            assert np.array_equal(cert, want), (k, q0, nb, cert)
            fb_want += int((want == 0).sum())
    assert on.i8_stats()[1:] == (3 * 13 - fb_want, fb_want)
    plan = [((i * 5) % 8 + 3, BS[i % 4], KS[(i * 2) % 3]) for i in range(200)]
    want = [dev_search(torch, f32, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    torch.cuda.synchronize()
    got = [dev_search(torch, on, d_q[q0:q0 + nb], k) for q0, nb, k in plan]          # back to back: no sync
    got0 = [dev_search(torch, off, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    gotd = [dev_search(torch, dflt, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    torch.cuda.synchronize()
    for i, ((kg, cg), (k0, c0), (kd, cd), (kw, cw)) in enumerate(zip(got, got0, gotd, want)):
        assert torch.equal(cg, cw) and torch.equal(kg, kw) and torch.equal(c0, cw) and torch.equal(k0, kw), (i, plan[i])
        assert torch.equal(cd, cw) and torch.equal(kd, kw), (i, plan[i])
    assert on.bf16_stats()[1:] == off.bf16_stats()[1:] and on.i8_stats()[1:] == off.i8_stats()[1:]
    assert on.i8_stats()[2] == fb_want, "every query of the 200 searches is certifiable"
    close(hs)
