"""Exact-data sweeps of every form of the dense scan ("Exact-data sweeps of the scan").

The data of tests/exact_cases.py has no rounding: every correct kernel returns the same bits, so each check here is an
equal count, an identical id list and equal score bits, with every expected value from `exact_cases.expected` (integer
arithmetic), never from the library.  A query's unfiltered top-`width` is exactly its window of rows, so one call with a
query per window reads the score of every row of the corpus out of the form under test, each query slot aiming at
another row range.  tests/test_exact_cases_cpu.py holds the generator and the checker to the oracle and to planted
faults."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_cases as X
from cqs_amd import DistanceMetric, HipIndex, _lib, unpack_keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def build(c, **kw):
    return HipIndex.build_from_flat(None, c.rows, DistanceMetric.DotProduct if c.dot else DistanceMetric.Cosine, **kw)


def block(idx, c, qis, k, what, keep=None, keeps=None, mode=_lib.MODE_RAW, thr=0.0, dead=(), row_base=0):
    """One call with the queries `qis` of the case as its block; every query's answer held to `expected`."""
    qis = list(qis)
    q = c.queries[qis]
    if keeps is not None:
        r, s, cnt = idx.search_batch_filtered(q, k, np.stack(keeps), mode=mode, threshold=thr)
    else:
        r, s, cnt = idx.search_batch(q, k, keep_bitset=keep, mode=mode, threshold=thr)
    for j, qi in enumerate(qis):
        eid, esc = X.expected(c.S[qi], c.e, k, keep=keeps[j] if keeps is not None else keep, mode=mode, thr=thr, dead=dead)
        X.assert_exact(r[j], s[j], cnt[j], eid + np.uint64(row_base), esc,
                       what="%s: %d x %d, block of %d, slot %d (query %d, window %s), k %d" % (what, c.n, c.dim, len(qis), j, qi, c.windows[c.target[qi]], k))


def scattered_bits(c, seed):
    """A keep-bitset with about half the rows, the last one among them."""
    keep = np.random.default_rng(seed).integers(0, 2 ** 32, (c.n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    keep |= X.range_bits(c.n, c.n - 1, c.n)
    return keep & X.range_bits(c.n, 0, c.n)


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- a. gemv: every chunk count x both last-chunk forms x every pass width ------------------------------------------
@pytest.mark.parametrize("chunks", range(1, 17))
def test_gemv_every_chunk_count_and_pass_width(hip, chunks):
    """scan_gemv_kernel<NCH = chunks, BQ, RI, ., FULL, ...>: dims 256 c (FULL) and 256 (c - 1) + 4 (the smallest partial last
    chunk; for some c also 256 c - 4), 300 rows = 16-row tasks with a ragged last one, k = 300 = every row of every query.
    Blocks of 1, 2, 4 and 5..8 queries are the BQ = 1, 2, 4, 8 passes; 3 = 2 + 1, 7 = a padded 8-query pass."""
    for dim in X.gemv_dims(chunks):
        c = X.gemv_case(dim)
        idx = build(c)
        for b in X.gemv_blocks(chunks):
            block(idx, c, range(b), X.GEMV_N, "gemv")
            if b > 1:
                block(idx, c, range(c.Q.shape[0] - b, c.Q.shape[0]), X.GEMV_N, "gemv")
        idx.close()


def test_gemv_block_of_13_where_the_matrix_cores_do_not_apply(hip):
    """dim % 32 != 0: blocks of >= 9 queries stay on gemv passes, 13 = 8 + 5."""
    c = X.gemv_case(100, 13)
    idx = build(c)
    block(idx, c, range(13), X.GEMV_N, "gemv 8 + 5")
    idx.close()


# ---- b. row-count edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [768, 4])
@pytest.mark.parametrize("n", X.ROW_EDGES)
def test_row_count_edges(hip, n, dim):
    """Windows of 1024 rows at k = 1024: the single queries and the block of eight read every row's score, unfiltered, then
    once more with each window as the shared keep-bitset (where every query of the block is checked on the window's rows)."""
    for c in X.edge_cases(n, dim):
        idx = build(c)
        for w in range(len(c.windows)):
            block(idx, c, [w], X.MAX_K, "edge, single")
        block(idx, c, range(8), X.MAX_K, "edge, eight")
        for lo, hi in c.windows:
            keep = X.range_bits(n, lo, hi)
            block(idx, c, [0], X.MAX_K, "edge, single, shared bitset", keep=keep)
            block(idx, c, range(8), X.MAX_K, "edge, eight, shared bitset", keep=keep)
        idx.close()


# ---- c. per-query bitsets ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def idx768(hip):
    c = X.mfma_case(768)
    idx = build(c)
    yield c, idx
    idx.close()


@pytest.mark.parametrize("b", [2, 5, 8, 9, 20])
def test_per_query_bitsets(idx768, b):
    """search_batch_filtered: query i keeps window i (256 rows of 4097); every other slot's window is offset by 13 rows, so it
    begins and ends inside a 32-bit word that its neighbours' windows share.  k = 300 > the kept rows.  Then the same block
    with an all-zero bitset in its first slot and an all-ones bitset in its last."""
    c, idx = idx768
    n = c.n
    for start in (0, 17 - b if b < 17 else 3):
        qis = list(range(start, start + b))
        keeps = [X.window_bits(n, int(c.target[qi]), X.MFMA_WIDTH, offset=13 if j % 2 else 0) for j, qi in enumerate(qis)]
        block(idx, c, qis, 300, "per-query bitsets", keeps=keeps)
        keeps[0] = np.zeros_like(keeps[0])
        keeps[-1] = X.range_bits(n, 0, n)
        block(idx, c, qis, 300, "per-query bitsets, none / all", keeps=keeps)


# ---- d. matrix-core forms, default switches -----------------------------------------------------------------------------
MFMA_BLOCKS = [9, 16, 32, 33, 64, 65, 128, 129, 256, 300]
MFMA_OTHER_DIM = {9: 256, 16: 512, 32: 1024, 33: 32, 64: 96, 65: 384, 128: 2048, 129: 4096, 256: 384, 300: 96}


def mfma_sweep(idx, c, b, what):
    """Blocks of b queries over the 17 windows of 256 rows (two blocks where b < 17): every row of the corpus is read."""
    for start in ((0, b) if b < 17 else (0,)):
        block(idx, c, range(start, start + b), X.MFMA_WIDTH, what)


@pytest.mark.parametrize("b,dim", [(b, 768) for b in MFMA_BLOCKS] + sorted(MFMA_OTHER_DIM.items()))
def test_matrix_core_forms(hip, b, dim):
    """9-32 queries at 256 / 512 / 768 / 1024 dimensions: scan_mfma_ks_kernel; else scan_mfma16_kernel with the 32-, 64- and
    128-query tiles (129-256: two query blocks; 300 = 256 + 44).  4097 rows: the last row tile holds one row."""
    c = X.mfma_case(dim) if dim == 768 else X.mfma_case(dim, 2 * b if b < 17 else b + 1)
    idx = build(c)
    mfma_sweep(idx, c, b, "matrix cores")
    block(idx, c, [(1 + i) % c.Q.shape[0] for i in range(b)], X.MFMA_WIDTH, "matrix cores, shared bitset", keep=scattered_bits(c, b))
    thr = float(c.score_f32(2, c.windows[2][0] + 100))      # a score that occurs (the kernels gate with !(s >= thr))
    block(idx, c, range(b), X.MFMA_WIDTH, "matrix cores, PIPELINE", mode=_lib.MODE_PIPELINE, thr=thr)
    idx.close()


def queue_sweep(idx, c, b, what, k=256):
    block(idx, c, range(b), k, what)      # five windows: the first, two interior, the last full tile, the ragged end


@pytest.mark.parametrize("b,dim", [(9, 32), (33, 32), (65, 32), (129, 32), (256, 32), (32, 256)])
def test_matrix_core_work_queue(hip, b, dim):
    """80 001 rows: more row tiles than workgroups (1251 tiles of 64 rows for the K-split kernel, 626 of 128 for blocks of
    > 64 queries), so the workgroups continue from the work queue."""
    c = X.queue_case(dim, 256 if dim == 32 else 64)
    idx = build(c)
    queue_sweep(idx, c, b, "matrix cores, work queue")
    idx.close()


@pytest.mark.parametrize("b", [9, 33])
def test_matrix_core_work_queue_of_256_row_tiles(hip, b):
    """The 32- and 64-query tiles take 256 rows at two workgroups per CU: past 512 CUs' worth of rows they queue too."""
    c = X.queue_case(32, 64, 512 * n_cu() + 257)
    idx = build(c)
    queue_sweep(idx, c, b, "matrix cores, work queue, 256-row tiles")
    idx.close()


# ---- e. forms behind switches: one child process per setting ------------------------------------------------------------
SWITCHES = [("CQS_HIP_SCAN_MFMA_WAVES", "8"), ("CQS_HIP_SCAN_MFMA_WAVES", "4"), ("CQS_HIP_SCAN_MFMA_KSPLIT", "0"),
            ("CQS_HIP_SCAN_MFMA_KSPLIT", "2"), ("CQS_HIP_SELECT_AUX", "0")]
_child_failed = []                      # once a child process has failed, no further one is started in this session


def switch_runs(var, cu):
    """[(case thunk, [(first query, b, k)])] of one switch."""
    if var == "CQS_HIP_SCAN_MFMA_WAVES":
        blocks = [(0, b, 256) for b in (9, 33, 65, 129, 256)] + [(9, 9, 256)]
        return [(lambda: X.mfma_case(768), blocks), (lambda: X.queue_case(32, 256), [(0, b, 256) for b in (9, 33, 65, 129, 256)])]
    if var == "CQS_HIP_SCAN_MFMA_KSPLIT":
        blocks = [(0, b, 256) for b in (9, 32, 33, 64)] + [(9, 9, 256)]
        return [(lambda d=d: X.mfma_case(d), blocks) for d in (256, 512, 768, 1024)] + [(lambda: X.queue_case(256, 64), [(0, b, 256) for b in (9, 32, 33, 64)])]
    singles = [(w, 1, k) for w in range(4) for k in (100, 500, 1024)]
    return [(lambda: X.mfma_case(768), [(w, 1, k) for w in (0, 7, 16) for k in (100, 500, 1024)]),
            (lambda: X.tier_case("persistent", cu), singles)]


def child_dump(path, var):
    """In the child: the switch's searches, what came back to an .npz."""
    cu = n_cu() if var == "CQS_HIP_SELECT_AUX" else 0      # (the other switches' corpora do not depend on it)
    out = {"n_cu": np.int64(cu)}
    for ci, (make, blocks) in enumerate(switch_runs(var, cu)):
        c = make()
        idx = build(c)
        for bi, (q0, b, k) in enumerate(blocks):
            r, s, cnt = idx.search_batch(c.queries[q0:q0 + b], k)
            out["r_%d_%d" % (ci, bi)], out["s_%d_%d" % (ci, bi)], out["c_%d_%d" % (ci, bi)] = r, s, cnt
        idx.close()
    np.savez(path, **out)


@pytest.mark.parametrize("var,value", SWITCHES, ids=["%s=%s" % s for s in SWITCHES])
def test_forms_behind_switches(hip, tmp_path, var, value):
    """WAVES=8 / =4: scan_mfma_kernel in its seven tile configurations; KSPLIT=0: the LDS-tiled kernels for 9-32 queries at
    the K-split dimensions; KSPLIT=2: the two-workgroup K-split form for 33-64; SELECT_AUX=0: the select that gathers every
    group, at the k from which the index is otherwise used.  Each on the 4097-row corpus and on a work-queue corpus."""
    assert not _child_failed, "not started: the child for %s failed before this one" % _child_failed[0]
    path = str(tmp_path / "dump.npz")
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_scan_exact_gpu as t\nt.child_dump(%r, %r)\n" % (ROOT, os.path.join(ROOT, "tests"), path, var)
    env = dict(os.environ)
    env[var] = value
    _child_failed.append("%s=%s" % (var, value))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    _child_failed.pop()
    d = np.load(path)
    for ci, (make, blocks) in enumerate(switch_runs(var, int(d["n_cu"]))):
        c = make()
        for bi, (q0, b, k) in enumerate(blocks):
            r, s, cnt = d["r_%d_%d" % (ci, bi)], d["s_%d_%d" % (ci, bi)], d["c_%d_%d" % (ci, bi)]
            for j in range(b):
                X.assert_exact(r[j], s[j], cnt[j], *X.expected(c.S[q0 + j], c.e, k),
                               what="%s=%s: %d x %d, block of %d, slot %d, k %d" % (var, value, c.n, c.dim, b, j, k))


# ---- f. task tiers and the select's index ---------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("tier", X.TIERS)
def test_task_tiers(hip, tier, b):
    """n just past each plan change of plan_tiers / launch_gemv for this device's CU count: 16-row tasks, 64-row tasks, 64-row
    + 32-row tail, the persistent grid.  Windows at the first rows, across the seam of the tiers, over the last full tasks
    and over the ragged end; k = 20 (the select without the (argmax, runner-up) index), 100 and 1024 (with it)."""
    c = X.tier_case(tier, n_cu())
    idx = build(c)
    for k in (20, 100, X.MAX_K):
        for start in range(0, 4, b):
            block(idx, c, range(start, start + b), k, "tiers %s %s" % (tier, c.tiers))
    idx.close()


# ---- g. other routes that must give the same bytes ----------------------------------------------------------------------
def routes_sweep(idx, c, what, **kw):
    """gemv blocks of eight and one, and the matrix-core block of 17, over the 17 windows: every row."""
    for qis in (range(0, 8), range(8, 16), [16], range(17)):
        block(idx, c, qis, X.MFMA_WIDTH, what, **kw)


def test_route_sharded(hip):
    """Three shards on one device: another task plan per shard and a host merge, the same bytes."""
    c = X.mfma_case(768)
    idx = HipIndex.build_sharded(None, c.rows, [0, 0, 0])
    routes_sweep(idx, c, "sharded [0, 0, 0]")
    block(idx, c, range(8), X.MFMA_WIDTH, "sharded, shared bitset", keep=scattered_bits(c, 5))
    idx.close()


def test_route_extend_in_two_pieces(hip):
    c = X.mfma_case(768)
    idx = HipIndex.build_from_flat(None, c.rows[:1500])
    idx.extend(None, c.rows[1500:4000])
    idx.extend(None, c.rows[4000:])
    routes_sweep(idx, c, "extend")
    idx.close()


def test_route_row_base(hip):
    c = X.mfma_case(768)
    idx = build(c, row_base=100000)
    routes_sweep(idx, c, "row_base", row_base=100000)
    idx.close()


def test_route_search_device_through_torch_pointers(hip):
    import torch
    c = X.mfma_case(768)
    d_rows = torch.from_numpy(c.rows).cuda()
    idx = HipIndex.build_from_device(None, d_rows.data_ptr(), c.n, c.dim, borrow=True, keepalive=d_rows)
    k = X.MFMA_WIDTH
    for qis in (range(0, 8), range(8, 16), [16], range(17), range(40)):
        qis = list(qis)
        d_q = torch.from_numpy(c.queries[qis]).cuda()
        keys = torch.full((len(qis), k), -1, dtype=torch.int64, device="cuda")
        counts = torch.full((len(qis),), -1, dtype=torch.int32, device="cuda")
        idx.search_device(d_q.data_ptr(), len(qis), k, keys.data_ptr(), counts.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hk, hc = keys.cpu().numpy().view(np.uint64), counts.cpu().numpy()
        for j, qi in enumerate(qis):
            r, s = unpack_keys(hk[j, :hc[j]])
            X.assert_exact(r, s, hc[j], *X.expected(c.S[qi], c.e, k), what="search_device, block of %d, slot %d" % (len(qis), j))
    idx.close()


@pytest.mark.parametrize("i8", ["0", "1"], ids=["bf16", "bf16+int8"])
def test_route_shadow_forced(hip, monkeypatch, i8):
    """The handle scans its bf16 (and int8) copy first and certifies or falls back to the f32 scan: the same bytes either
    way, and every query is counted as one or the other."""
    c = X.mfma_case(768)
    monkeypatch.setenv("CQS_HIP_SCAN_BF16", "1")
    monkeypatch.setenv("CQS_HIP_SCAN_I8", i8)
    idx = build(c)
    assert idx.bf16_stats()[0] == c.n * c.dim * 2 and (idx.i8_stats()[0] > 0) == (i8 == "1"), idx.last_error()
    asked = 0
    for qis in (range(0, 8), range(8, 16), [16], range(3, 7), range(12, 15)):
        block(idx, c, qis, X.MFMA_WIDTH, "shadow forced (int8 %s)" % i8)
        asked += len(qis)
    _, certified, fallbacks = idx.bf16_stats()
    assert certified + fallbacks == asked, (certified, fallbacks, asked)
    idx.close()


def test_route_dot_metric_integers(hip):
    """e = 0: integer entries, raw scores in the thousands, the dot handle's log-spaced bins."""
    c = X.mfma_case(768, dot=True)
    assert c.e == 0 and np.abs(c.S).max() > 2000
    idx = build(c)
    routes_sweep(idx, c, "dot metric")
    block(idx, c, range(8), X.MAX_K, "dot metric, k = 1024")
    idx.close()


# ---- h. non-finite rows in exact data -------------------------------------------------------------------------------------
def test_non_finite_rows_inside_a_window(hip):
    """A NaN row and a +inf row in window 5: its answer is the expected list without them (through a bitset: width - 2
    rows), every other window is unchanged."""
    c = X.mfma_case(768)
    rows = c.rows.copy()
    lo, hi = c.windows[5]
    dead = (lo + 7, hi - 64)
    rows[dead[0], 3] = NAN
    rows[dead[1], 700] = INF
    idx = HipIndex.build_from_flat(None, rows)
    routes_sweep(idx, c, "non-finite rows", dead=dead)
    keep = X.range_bits(c.n, lo, hi)
    r, s, cnt = idx.search_batch(c.queries[5], X.MFMA_WIDTH, keep_bitset=keep)
    assert cnt[0] == X.MFMA_WIDTH - 2
    block(idx, c, [5], X.MFMA_WIDTH, "non-finite rows, shared bitset", keep=keep, dead=dead)
    block(idx, c, range(17), X.MFMA_WIDTH, "non-finite rows, shared bitset, matrix cores", keep=keep, dead=dead)
    block(idx, c, range(3, 8), 300, "non-finite rows, per-query bitsets", dead=dead,
          keeps=[X.window_bits(c.n, w, X.MFMA_WIDTH) for w in range(3, 8)])
    idx.close()
