"""Consecutive int8 shadow scans sweep the copy in alternating directions, and the workgroups at the two ends of a
streamed copy load plainly (scan_i8.hip, i8_sweep.h, index_shadow.hip; DESIGN.md §3.11, "Serpentine sweep").  Only the order
in time and the load instruction change, so every output is the parent's bit for bit.

Four handles over the same rows, both copies built at any size (CQS_HIP_SCAN_I8=1 CQS_HIP_SCAN_BF16=1): `win`
(CQS_HIP_I8_SERPENTINE=w:<bytes>: the sweep alternates and the scan takes its nontemporal instantiation with a plain-load
window of a quarter of the copy plus one byte at each end, so the window's edge falls inside these small corpora, in the
middle of a workgroup's rows), `off` (=0: the parent's scan), `f32` (both copies off) and `on` (the switch unset: the sweep
alternates; the load policy is untouched below 200 MiB, and at 131 136 x 2048 the copy is streamed and wholly inside the
two windows).  After every search: counts and keys in every one of the k slots equal in all four; the per-query verdicts
`cert`, the certified / fallback counters of both copies and the prefix counters exactly equal between `win`, `off` and `on`.
Every list of searches runs twice with one search in between, so each (b, k, mode) meets both parities.

Sizes: 16-row tasks (n < 131 072: a workgroup is 64 rows; 3 and 255 rows are one partly masked workgroup, 257 two) and
64-row tasks (a workgroup is 256 rows).  The index pads n to 256 rows, so n_tasks is a multiple of 4 here; every n_tasks mod 4,
a partial last group and a group across the 64 / 32-row boundary are covered device-free (test_i8_serpentine_cpu.py).
Each case takes seconds.  Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipIndex, _lib, synth
from test_i8_groups_gpu import close, device_rows, key_rows, plant, same, same_host
from test_shadow_premises_gpu import I8, hooks, score_rows  # noqa: F401  (hooks: the fixture behind score_rows)
from test_shadow_tail_gpu import dev_search, setenv

pytestmark = pytest.mark.gpu
ENV_SWITCH = "CQS_HIP_I8_SERPENTINE"
BS = (1, 2, 4)
KS = (1, 20, 87)


@pytest.fixture
def torch():
    import torch as t
    return t


def window_bytes(n, dim):
    return n * dim // 4 + 1


def quad(monkeypatch, torch, rows, owned=False):
    """(win, off, f32, on): the order test_i8_groups_gpu.same compares in (first against the rest)."""
    if owned:
        host = np.ascontiguousarray(rows, dtype=np.float32)
        n, dim = host.shape
    else:
        d = rows if hasattr(rows, "data_ptr") else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
        n, dim = d.shape
    made = []
    for shadow, switch in (("1", "w:%d" % window_bytes(n, dim)), ("1", "0"), ("0", None), ("1", None)):
        setenv(monkeypatch, shadow, shadow)
        if switch is None:
            monkeypatch.delenv(ENV_SWITCH, raising=False)
        else:
            monkeypatch.setenv(ENV_SWITCH, switch)
        if owned:
            made.append(HipIndex.build_from_flat(None, host))
        else:
            made.append(HipIndex.build_from_device(None, d.data_ptr(), n, dim, DistanceMetric.Cosine, borrow=True, keepalive=d))
    setenv(monkeypatch, None, None)
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    win, off, f32, on = made
    for h in (win, off, on):
        assert h.bf16_stats()[0] == n * dim * 2 and h.i8_stats()[0] == n * dim + n * 4, h.last_error()
    assert f32.bf16_stats()[0] == 0 and f32.i8_stats()[0] == 0
    return win, off, f32, on


def both_parities(torch, hs, d_q, searches, ctx):
    """`searches` = [(q0, nb, k, kwargs)]: the list, one more search, the list again - each entry on either parity."""
    for lap in (0, 1):
        for q0, nb, k, kw in searches:
            same(torch, hs, d_q[q0:q0 + nb], k, ctx + (lap, q0, nb, k, tuple(kw.items())), **kw)
        if lap == 0 and len(searches) % 2 == 0:
            same(torch, hs, d_q[:1], 1, ctx + ("between",))


def sweep(torch, hs, d_q, top, ctx):
    searches = []
    for j, nb in enumerate(BS):
        for k in KS:
            q0 = (3 * j + k) % 8
            searches.append((q0, nb, k, {}))
            searches.append((q0, nb, k, {"mode": _lib.MODE_PIPELINE, "threshold": max(top * 0.8, 0.0)}))
    both_parities(torch, hs, d_q, searches, ctx)
    assert hs[0].i8_stats()[1] + hs[0].i8_stats()[2] == hs[0].bf16_stats()[1] + hs[0].bf16_stats()[2], \
        "every block of <= 4 queries at k <= 87 goes through the int8 copy"


def score_rows_equal(hooks, hs, qs, ctx):
    """The int8 scan's score rows, before any select, twice per handle (both parities): the same bits in `win`, `off`, `on`."""
    win, off, _, on = hs
    for nb in BS:
        for lap in (0, 1):
            ref, bq_ref = score_rows(hooks, off, I8, qs[:nb])
            for name, h in (("win", win), ("on", on)):
                got, bq = score_rows(hooks, h, I8, qs[:nb])
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (ctx, name, nb, lap)
                assert np.array_equal(bq.view(np.uint32), bq_ref.view(np.uint32)), (ctx, name, nb, lap)


@pytest.mark.parametrize("dim", [16, 768, 2048])
@pytest.mark.parametrize("n", [3, 255, 257, 4097, 131_072 + 64])
def test_every_shape_on_both_parities(hip, hooks, monkeypatch, torch, n, dim):
    if n > 100_000:
        d = device_rows(torch, n, dim, 9600 + dim)
    else:
        d = torch.from_numpy(synth.gaussian_unit(n, dim=dim, seed=9600 + n + dim)).cuda()
    qs = synth.gaussian_unit(12, dim=dim, seed=9650 + dim)
    hs = quad(monkeypatch, torch, d)
    top = float(hs[2].search_batch(qs[:1], 1)[1][0, 0])
    sweep(torch, hs, torch.from_numpy(qs).cuda(), top, (n, dim))
    score_rows_equal(hooks, hs, qs, (n, dim))
    close(hs)


def test_planted_rows_in_the_first_and_the_last_workgroup(hip, monkeypatch, torch):
    """64-row tasks, workgroups of 256 rows.  The best rows lie in workgroup 0 (launched last on a reversed sweep) and in the
    last, partly masked workgroup (launched first on it); two more in the workgroups the plain-load window's edges cut."""
    n, dim = 131_072 + 64, 768
    rows = device_rows(torch, n, dim, 9661).cpu().numpy()
    q = synth.gaussian_unit(4, dim=dim, seed=9662)
    edge = window_bytes(n, dim) // dim                       # the row the first window ends in
    spots = {n - 1: 3.5, 3: 3.0, 255: 2.9, n - 64: 2.8, edge: 2.7, n - 1 - edge: 2.6}
    for r, w in spots.items():
        plant(rows, q[0], r, w)
    hs = quad(monkeypatch, torch, rows)
    d_q = torch.from_numpy(q).cuda()
    want = [n - 1, 3, 255, n - 64, edge, n - 1 - edge]
    for lap in (0, 1, 2):                                      # (12 searches per lap, then one more: the parities swap)
        for k in KS + (6,):
            for nb in BS:
                keys, _ = same(torch, hs, d_q[:nb], k, ("planted", lap, k, nb))
                assert key_rows(keys[0, :min(k, 6)]).tolist() == want[:min(k, 6)], (lap, k, nb, key_rows(keys[0, :6]))
        same(torch, hs, d_q[:1], 1, ("planted, between", lap))
    close(hs)


def test_bitset_that_empties_the_first_and_the_last_group(hip, monkeypatch, torch):
    """A shared keep-bitset (device API and host API) without the rows of the first group and of the last group: the waves
    at both ends of either sweep skip their reads and publish -inf."""
    n, dim = 131_072 + 64, 16
    d = device_rows(torch, n, dim, 9671)
    q = synth.gaussian_unit(8, dim=dim, seed=9672)
    hs = quad(monkeypatch, torch, d)
    bits = np.ones(n, bool)
    bits[:256] = False
    bits[(n // 256) * 256:] = False
    words = np.packbits(np.pad(bits, (0, (-n) % 32)), bitorder="little").view(np.uint32)
    d_keep = torch.from_numpy(words.view(np.int32)).cuda()
    d_q = torch.from_numpy(q).cuda()
    for lap in (0, 1):
        for k in KS:
            for nb in BS:
                keys, _ = same(torch, hs, d_q[:nb], k, ("bitset", lap, k, nb), d_keep=d_keep)
                assert bits[key_rows(keys[keys != 0])].all()
                same_host(hs, lambda h: h.search_batch(q[:nb], k, keep_bitset=words), ("host bitset", lap, k, nb))
        same(torch, hs, d_q[:1], 1, ("bitset, between", lap))
    close(hs)


def test_back_to_back_and_after_extend_remove_update(hip, hooks, monkeypatch, torch):
    """Owned handles.  Twelve searches with no sync in between, b and k changing (both parities back to back on the same
    score rows and the same gmax rows); then extend, remove and update, each followed by three searches: the first sweeps
    forwards again, the other two on either parity."""
    n, dim = 131_072 + 64, 16
    rows = device_rows(torch, n, dim, 9681).cpu().numpy()
    q = synth.gaussian_unit(12, dim=dim, seed=9682)
    hs = quad(monkeypatch, torch, rows, owned=True)
    win, off, f32, on = hs
    d_q = torch.from_numpy(q).cuda()
    plan = [((i * 5) % 8, BS[i % 3], KS[(i * 2) % 3]) for i in range(12)]
    want = [dev_search(torch, f32, d_q[q0:q0 + nb], k) for q0, nb, k in plan]
    torch.cuda.synchronize()
    got = [[dev_search(torch, h, d_q[q0:q0 + nb], k) for q0, nb, k in plan] for h in (win, off, on)]   # back to back: no sync
    torch.cuda.synchronize()
    for name, res in zip(("win", "off", "on"), got):
        for i, ((kg, cg), (kw, cw)) in enumerate(zip(res, want)):
            assert torch.equal(cg, cw) and torch.equal(kg, kw), (name, i, plan[i])
    assert win.bf16_stats()[1:] == off.bf16_stats()[1:] == on.bf16_stats()[1:]
    assert win.i8_stats()[1:] == off.i8_stats()[1:] == on.i8_stats()[1:]

    def three(ctx):
        for i, (nb, k) in enumerate(((1, 20), (4, 87), (2, 1))):
            same(torch, hs, d_q[i:i + nb], k, ctx + (i, nb, k))
        score_rows_equal(hooks, hs, q, ctx)

    same(torch, hs, d_q[:1], 20, ("odd",))                     # leave the parity set before the rows change
    more = synth.gaussian_unit(300, dim=dim, seed=9683)
    plant(more, q[0], 299, 3.0)                                # the new best row, in the new last workgroup
    for h in hs:
        h.extend(None, more)
    three(("after extend",))
    gone = np.concatenate([np.arange(0, 256, 2), np.arange(70_000, 70_100), [n + 299]]).astype(np.uint64)
    for h in hs:
        assert h.remove_rows(gone) == len(gone)
    three(("after remove",))
    new = synth.gaussian_unit(3, dim=dim, seed=9684)
    plant(new, q[1], 0, 3.0)
    plant(new, q[2], 2, 3.0)
    where = np.array([1, 65_000, len(win) - 1], np.uint64)    # the first and the last workgroup, and one in the middle
    for h in hs:
        assert h.update_rows(where, new) == 3
    three(("after update",))
    close(hs)
