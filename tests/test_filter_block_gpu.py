"""One keep-bitset per query: cqs_hip_index_search_filtered and the combining queue's blocks of filtered callers
(include/cqs_hip.h).  The yardstick everywhere is the lone filtered call on the same handle,
`search_batch(q_i, k, keep_bitset=bits_i)`, which runs the shared-bitset kernels: rows, score bits and counts must be equal.
The cases live in filter_block_cases.py (the handles whose environment is read at create run them in a child process).
Run on an MI355X with `pytest -m gpu`."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import filter_block_cases as cases
from cqs_amd import DistanceMetric, _lib
from cqs_amd.index import HipError
from parity import assert_topk_parity

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def child(fn, **env):
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, "-c", f"import filter_block_cases as c; c.{fn}()"], capture_output=True, text=True,
                       env=e, timeout=600)
    assert p.returncode == 0 and f"{fn} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# 5 003: 16-row tasks, ragged last word and task; 140 005: 64-row tasks; 400 037: 64- + 32-row tiers; 1 600 000: persistent
# grid + work queue.  dim 64: partial chunk; 768: full chunks; 1280: five chunks, passes of <= 2 queries.
@pytest.mark.parametrize("n,dim", [(5003, 64), (5003, 768), (5003, 1280), (140_005, 64), (140_005, 768), (400_037, 64),
                                   (1_600_000, 64)])
def test_blocks_equal_the_lone_filtered_calls(hip, n, dim):
    c = cases.Corpus(n, dim)
    c.sweep()
    if n == 5003 and dim == 64:
        # independent of the library's own lone call: masked f32 dot + stable sort in numpy, the project's parity rule
        for k in (20, 500):
            r, s, cnt = c.idx.search_batch_filtered(c.qs, k, c.bits)
            for i in range(cases.FAMILY):
                sc = np.where(c.keep[i], c.rows @ c.qs[i], -np.inf).astype(np.float32)
                order = np.argsort(-sc, kind="stable")[:min(k + 64, int(c.keep[i].sum()))]
                assert_topk_parity(r[i, :cnt[i]], s[i, :cnt[i]], order, sc[order], min(k, int(c.keep[i].sum())))
    c.close()


@pytest.mark.parametrize("n,dim", [(5003, 768), (140_005, 64)])
def test_dot_metric_blocks(hip, n, dim):
    c = cases.Corpus(n, dim, DistanceMetric.DotProduct, seed=1)
    c.sweep(ks=(1, 100))
    c.close()


def test_every_rule_of_the_lone_call(hip):
    c = cases.Corpus(5003, 64)
    idx, qs, bits = c.idx, c.qs, c.bits
    r, s, cnt = idx.search_batch_filtered(qs, 20, bits)
    assert cnt[8] == 0 and cnt[5] == 1 and cnt[6] == 7                     # empty; one row; capped at the kept rows
    ur, us, uc = idx.search_batch(qs[7], 20)                               # all-pass == unfiltered
    cases.same((r[7], s[7], cnt[7]), (ur[0], us[0], uc[0]), "all-pass")
    bad = qs.copy()
    bad[3, 5] = np.nan
    r, s, cnt = idx.search_batch_filtered(bad, 20, bits)
    assert cnt[3] == 0
    for i in (2, 4, 9):
        cases.same((r[i], s[i], cnt[i]), c.lone(i, 20, _lib.MODE_RAW, 0.0), ("beside a non-finite query", i))
    assert not idx.search_batch_filtered(qs[:, :32], 20, bits)[2].any()    # dimension mismatch: counts 0
    with pytest.raises(HipError) as e:
        idx.search_batch_filtered(qs, 1025, bits)
    assert e.value.code == _lib.ERR_INVALID
    wide = np.concatenate([bits, np.full((len(bits), 3), 0xFFFFFFFF, np.uint32)], axis=1)   # a stride beyond ceil(n / 32)
    for i in range(cases.FAMILY):
        c.lone(i, 20, _lib.MODE_RAW, 0.0)
    before = idx.combine_filter_stats()                                    # (lone filtered calls are blocks of one)
    r, s, cnt = idx.search_batch_filtered(qs, 20, wide)
    assert idx.combine_filter_stats() == before                            # the block entry point is not the queue
    for i in range(cases.FAMILY):
        cases.same((r[i], s[i], cnt[i]), c.lone(i, 20, _lib.MODE_RAW, 0.0), ("wide stride", i))
    res = idx.search_many_with_filters(qs[:3], 5, [lambda cid: int(cid) % 2 == 0, lambda cid: False, lambda cid: True])
    assert [len(x) for x in res] == [5, 0, 5] and all(int(x.id) % 2 == 0 for x in res[0])
    assert [x.id for x in res[2]] == [x.id for x in idx.search(qs[2], 5)]
    c.close()


def test_extend_regrows_the_table(hip):
    c = cases.Corpus(5003, 64)
    c.check_block(5, 20, _lib.MODE_RAW, 0.0)
    more = cases.synth.gaussian_unit(9000, dim=64, seed=77)
    c.idx.extend(None, more)
    c.rows = np.concatenate([c.rows, more])
    c.keep = cases.family(c.rows, c.qs, 123)
    c.bits = np.stack([cases.pack(k) for k in c.keep])
    c._lone.clear()
    c.sweep(blocks=(3, 13), ks=(20,))
    c.close()


def test_shadow_copies_certify_filtered_blocks(hip):
    child("child_shadow", CQS_HIP_SCAN_BF16="1", CQS_HIP_SCAN_I8="1")


def test_uncertified_queries_are_redone_with_their_own_bitsets(hip):
    child("child_adversarial", CQS_HIP_SCAN_BF16="1", CQS_HIP_SCAN_I8="0")


def test_filtered_callers_share_passes(hip):
    """8 and 16 native threads, one query and its bitset per call: lone answers, and the queue really combined."""
    c = cases.Corpus(140_005, 768)
    p, q, total = cases.storm_case(c)
    assert q == total, (q, total)
    assert q > 1.5 * p, f"the filtered queue did not combine: {q} queries in {p} passes"
    c.close()


def test_opt_out_keeps_the_serial_path(hip):
    child("child_opt_out", CQS_HIP_COMBINE_FILTERED="0")


def test_mixed_python_callers(hip):
    """Filtered, unfiltered and PIPELINE callers at once: each gets its lone answer."""
    c = cases.Corpus(140_005, 64)
    idx = c.idx
    thr = 0.05
    want_u = [idx.search_batch(c.qs[i], 20) for i in range(cases.FAMILY)]
    want_p = [idx.search_batch(c.qs[i], 20, mode=_lib.MODE_PIPELINE, threshold=thr) for i in range(cases.FAMILY)]
    for i in range(cases.FAMILY):
        c.lone(i, 20, _lib.MODE_RAW, 0.0), c.lone(i, 20, _lib.MODE_PIPELINE, thr)
    errs = []

    def work(t):
        try:
            for rep in range(5):
                for i in range(t % 4, cases.FAMILY, 4):
                    kind = t % 4
                    if kind == 0:
                        got, want = idx.search_batch(c.qs[i], 20), want_u[i]
                    elif kind == 1:
                        got, want = idx.search_batch(c.qs[i], 20, mode=_lib.MODE_PIPELINE, threshold=thr), want_p[i]
                    else:
                        mode, th = (_lib.MODE_RAW, 0.0) if kind == 2 else (_lib.MODE_PIPELINE, thr)
                        got = idx.search_batch(c.qs[i], 20, keep_bitset=c.bits[i], mode=mode, threshold=th)
                        w = c.lone(i, 20, mode, th)
                        want = (w[0][None], w[1][None], np.array([w[2]]))
                    cases.same((got[0][0], got[1][0], got[2][0]), (want[0][0], want[1][0], want[2][0]), (t, rep, i))
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errs.append((t, repr(e)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(12)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs
    c.close()


def test_poisoned_handle_wakes_every_parked_filtered_caller(hip):
    import ctypes as C
    c = cases.Corpus(140_005, 768)
    idx = c.idx
    lib = _lib.load()
    lib.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    lib.cqs_hip_debug_index_fail_next.restype = None
    codes, lock, start = [], threading.Lock(), threading.Barrier(9)

    def work(t):
        start.wait()
        for rep in range(40):
            i = (t + rep) % cases.FAMILY
            try:
                idx.search_batch(c.qs[i], 20, keep_bitset=c.bits[i])
            except HipError as e:
                with lock:
                    codes.append(e.code)

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [x.start() for x in th]
    start.wait()
    lib.cqs_hip_debug_index_fail_next(idx._h)
    [x.join(timeout=60) for x in th]
    assert not any(x.is_alive() for x in th), "a filtered caller is still parked on a poisoned handle"
    assert idx.is_poisoned()
    assert codes.count(_lib.ERR_DEVICE) == 1, codes
    assert codes.count(_lib.ERR_POISONED) == len(codes) - 1 and len(codes) >= 8, codes
    c.close()
