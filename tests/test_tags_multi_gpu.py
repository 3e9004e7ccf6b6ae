"""Tag filters per query (include/cqs_hip.h "row tags"): `tags_keep_multi_kernel` word for word against
numpy, `cqs_hip_index_search_tagged_multi` against the lone `cqs_hip_index_search_tagged` call and against
`cqs_hip_index_search_filtered` with the host bitsets of the same predicates, and the combining queue's blocks of single
tagged callers.  Rows, score bits, counts, status and message must be equal: no tolerance anywhere.  The cases live in
tags_multi_cases.py (handles whose environment is read at create run them in a child process)."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import tags_cases as tc
import tags_multi_cases as mc
from cqs_amd import DistanceMetric, HipError, HipIndex, _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROW_COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 5000, mc.N_BIG)
FS = (1, 2, 8, 9, 31, 32)
SENTINEL = 0xDEADBEEF


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def child(fn, **env):
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, "-c", f"import tags_multi_cases as c; c.{fn}()"], capture_output=True, text=True,
                       env=e, timeout=600)
    assert p.returncode == 0 and f"{fn} ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.fixture(scope="module")
def data(hip):
    rows, q, tags = mc.data()
    q, allows = mc.block_case(q, tags, 9400)
    for a in (rows, q, tags, allows):
        a.setflags(write=False)
    return rows, q, tags, allows


@pytest.fixture(scope="module")
def storm_data(hip):
    made = mc.storm_corpus()
    for a in made:
        a.setflags(write=False)
    return made


# ---- 1. the kernel, word for word ----------------------------------------------------------------------------------------
def hook(hip, idx, allows, max_blocks=0):
    """-> (words [f, ceil(n / 32)], kept [f]).  The hook runs the kernel into a table of 32 rows with two guard words
    behind each, all pre-filled, and fails if a guard word or a word of a row >= f changed; the output arrays here have
    guards of their own."""
    n, f = len(idx), len(allows)
    words = (n + 31) // 32
    out = np.full(f * words + 2, 0xA5A5A5A5, dtype=np.uint32)
    kept = np.full(f + 1, 0xDEAD, dtype=np.uint64)
    a = np.ascontiguousarray(allows, dtype=np.uint32)
    rc = hip.cqs_hip_debug_index_tag_keep_multi(idx._h, _ptr(a), f, max_blocks, _ptr(out), _ptr(kept))
    assert rc == _lib.OK, idx.last_error()
    assert out[-1] == out[-2] == 0xA5A5A5A5 and kept[-1] == 0xDEAD
    return out[:-2].reshape(f, words), kept[:-1]


def check_kernel(hip, idx, tags, f, seed, max_blocks=0):
    allows = mc.kernel_filters(tags, f, seed)
    words, kept = hook(hip, idx, allows, max_blocks)
    for j in range(f):
        mask = tc.keep_mask(tags, allows[j])
        assert np.array_equal(words[j], tc.bits_of(mask)), (len(tags), f, j, max_blocks)      # the bits past n are zero
        assert int(kept[j]) == int(mask.sum()), (len(tags), f, j, max_blocks)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_kernel_word_for_word(hip, data, n):
    rows = data[0]
    tags = tc.unique_end_tags(n, 9200 + n)
    idx = mc.tagged_index(rows[:n], tags)
    for f in FS:
        check_kernel(hip, idx, tags, f, 9300 + n)
    assert not idx.is_poisoned()
    idx.close()


@pytest.mark.parametrize("max_blocks", (1, 3))
def test_kernel_grid_stride_loop(hip, data, max_blocks):
    rows = data[0]
    n = 5000                                             # five steps of 1024 rows: 5 and 2 / 2 / 1 per workgroup
    tags = tc.unique_end_tags(n, 9200 + n)
    idx = mc.tagged_index(rows[:n], tags)
    for f in FS:
        check_kernel(hip, idx, tags, f, 9300 + n, max_blocks)
    idx.close()


# ---- 2. block bytes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", (DistanceMetric.Cosine, DistanceMetric.DotProduct))
@pytest.mark.parametrize("n", (5000, mc.N_BIG))
def test_block_bytes(data, n, metric):
    rows, q, tags, allows = data
    tags = tags[:n]
    if n != len(data[2]):                                # (first_row / last_row of the smaller corpus are its own)
        q, allows = mc.block_case(q, tags, 9400)
    idx = mc.tagged_index(rows[:n], tags, metric)
    bits = mc.host_bits(tags, allows)
    lone = mc.Lone(idx, q, allows)
    kept = [int(tc.keep_mask(tags, a).sum()) for a in allows]
    assert kept[1] == n and kept[2] == 0 and kept[4] == 7 and kept[5] == 1 and 0 < kept[0] < n
    assert not np.isfinite(q[3]).all()
    for b in (1, 2, 9, 32, 33, 40):
        for k in (1, 20, 500):
            for mode, thr in ((_lib.MODE_RAW, 0.0), (_lib.MODE_PIPELINE, 0.0), (_lib.MODE_PIPELINE, 0.3)):
                c = mc.check_block(idx, lone, q, allows, bits, b, k, mode, thr)
                if mode == _lib.MODE_RAW:
                    want = [0 if not np.isfinite(q[i]).all() else min(k, kept[i]) for i in range(b)]
                    assert list(c) == want, (n, b, k)
    # the all-pass query of the block is the unfiltered answer
    r, s, c = idx.search_tagged_multi(q[:9], 20, allows[:9])
    ur, us, uc = idx.search_batch(q[1], 20)
    mc.same_query((r[1], s[1], c[1]), (ur[0], us[0], uc[0]), "all-pass")
    assert sorted(int(x) for x in r[4, :7]) == sorted(np.flatnonzero(tc.keep_mask(tags, allows[4])))
    assert not idx.is_poisoned()
    idx.close()


# ---- 3. rules ------------------------------------------------------------------------------------------------------------
def _raw(lib, idx, q, b, qd, k, allows, mode=_lib.MODE_RAW, multi=True):
    q = np.ascontiguousarray(q, dtype=np.float32)
    rows = np.zeros((max(b, 1), max(k, 1)), dtype=np.uint64)
    scores = np.zeros((max(b, 1), max(k, 1)), dtype=np.float32)
    counts = np.full((max(b, 1),), SENTINEL, dtype=np.uint32)
    a = None if allows is None else np.ascontiguousarray(allows, dtype=np.uint32)
    fn = lib.cqs_hip_index_search_tagged_multi if multi else lib.cqs_hip_index_search_tagged
    rc = fn(idx._h, _ptr(q), b, qd, k, _ptr(a), mode, 0.0, _ptr(rows), _ptr(scores), _ptr(counts))
    return rc, counts, idx.last_error()


def test_rules(hip, data):
    rows, q, tags, _allows = data
    n = 3000
    tags = tags[:n]
    q, allows = mc.block_case(q, tags, 9500)
    good = np.flatnonzero(np.isfinite(q).all(axis=1))[:3]
    q3, a3 = np.ascontiguousarray(q[good]), np.ascontiguousarray(np.stack([allows[0], allows[7], allows[8]]))
    idx = mc.tagged_index(rows[:n], tags)
    assert _raw(hip, idx, q3, 0, mc.DIM, 20, a3)[1][0] == SENTINEL                         # b = 0 touches nothing
    for b in (1, 3):
        # status, counts and last_error equal those of search_tagged with the block's first filter
        for args in ((q3, b, mc.DIM, 0), (q3[:, :48], b, 48, 20), (q3, b, mc.DIM, 1025)):
            m, s = _raw(hip, idx, *args, a3), _raw(hip, idx, *args, a3[0], multi=False)
            assert m[0] == s[0] and m[2] == s[2] and list(m[1][:b]) == list(s[1][:b]) == [0] * b, (args[1:], m, s)
        m = _raw(hip, idx, q3, b, mc.DIM, 20, a3, mode=_lib.MODE_PIPELINE + 1)
        s = _raw(hip, idx, q3, b, mc.DIM, 20, a3[0], mode=_lib.MODE_PIPELINE + 1, multi=False)
        assert m[0] == s[0] == _lib.ERR_INVALID and m[2] == s[2] == "search: bad mode"
    assert _raw(hip, idx, q3, 3, mc.DIM, 1025, a3)[2] == "search: k > max_k"
    assert _raw(hip, idx, q3[:, :48], 3, 48, 20, a3)[::2] == (_lib.OK, "search: query dimension mismatch (empty result)")
    # the tag-specific refusals: INVALID, nothing touched, nothing poisoned
    rc, counts, msg = _raw(hip, idx, q3, 3, mc.DIM, 20, None)
    assert rc == _lib.ERR_INVALID and msg == "search_tagged_multi: null allow" and list(counts) == [SENTINEL] * 3
    s = HipIndex.build_sharded(None, rows[:n], [0, 0])
    with pytest.raises(HipError) as e:
        s.search_tagged_multi(q3, 20, a3)
    assert e.value.code == _lib.ERR_INVALID and "search_tagged_multi: not built for a row-sharded handle" in str(e.value)
    assert not s.is_poisoned() and list(s.search_batch(q3, 20)[2]) == [20, 20, 20]
    s.close()
    before = idx.combine_tagged_stats()
    idx.search_tagged_multi(q[:9], 20, allows[:9])
    assert idx.combine_tagged_stats() == before                                             # the block entry point is not the queue
    # extend: the new rows have no tag; after set_tags the answers are the host-bitset ones again, the table regrown
    more = mc.synth.gaussian_unit(4000, mc.DIM, seed=77)
    more_tags = tc.random_tags(4000, 78)
    idx.extend(None, more)
    assert len(idx) == 7000 and idx.tagged_rows() == n
    with pytest.raises(HipError) as e:
        idx.search_tagged_multi(q[:9], 20, allows[:9])
    assert e.value.code == _lib.ERR_INVALID and "search_tagged_multi: tags cover 3000 of 7000 rows" in str(e.value)
    with pytest.raises(HipError) as e:                   # (the single call, which parks when it may, is refused before it parks)
        idx.search_tagged_batch(q[0], 20, allows[0])
    assert "search_tagged: tags cover 3000 of 7000 rows" in str(e.value)
    assert not idx.is_poisoned() and list(idx.search_batch(q3, 20)[2]) == [20, 20, 20]
    idx.set_tags(more_tags, first=n)
    tags2 = np.concatenate([tags, more_tags])
    bits = mc.host_bits(tags2, allows)
    for b, k in ((9, 20), (40, 500)):
        mc.check_block(idx, mc.Lone(idx, q, allows), q, allows, bits, b, k)
    # remove: the column is compacted with the rows
    gone = np.sort(np.random.default_rng(79).choice(7000, size=2500, replace=False))
    assert idx.remove_rows(gone) == len(gone) and idx.tagged_rows() == len(idx) == 4500
    tags3 = np.delete(tags2, gone)
    bits = mc.host_bits(tags3, allows)
    for b, k in ((9, 20), (40, 500)):
        mc.check_block(idx, mc.Lone(idx, q, allows), q, allows, bits, b, k)
    assert not idx.is_poisoned()
    idx.close()


# ---- 4. through the shadow copies ----------------------------------------------------------------------------------------
def test_shadow_copies_serve_tagged_blocks(hip):
    child("child_shadow", CQS_HIP_SCAN_BF16="1", CQS_HIP_SCAN_I8="1")


# ---- 5. - 8. the queue -----------------------------------------------------------------------------------------------------
def test_tagged_callers_share_passes(hip, storm_data):
    """8 and 16 native threads, one query and its tag filter per call: lone answers, and the queue really combined."""
    rows, qs, tags, allows = storm_data
    idx = mc.tagged_index(rows, tags)
    lone = mc.Lone(idx, qs, allows)
    want = [lone(i, 20) for i in range(len(qs))]
    for i in range(len(qs)):                             # the lone tagged call is the host-bitset call, byte for byte
        r, s, c = idx.search_batch(qs[i], 20, keep_bitset=tc.bits_of(tc.keep_mask(tags, allows[i])))
        mc.same_query((r[0], s[0], c[0]), want[i], ("host bitset", i))
    p, q, total = mc.storm_case(idx, qs, allows, want)
    print("tagged storm:", q, "queries in", p, "passes")
    assert q == total, (q, total)
    assert q > 1.5 * p, f"the tagged queue did not combine: {q} queries in {p} passes"
    assert not idx.is_poisoned()
    idx.close()


def test_opt_out_keeps_the_serial_path(hip):
    child("child_opt_out", CQS_HIP_COMBINE_TAGGED="0")


def test_mixed_python_callers(hip, data):
    """Unfiltered, host-bitset, tagged and PIPELINE-tagged callers at once on one handle: each gets its lone answer."""
    rows, q, tags, allows = data
    idx = mc.tagged_index(rows, tags)
    thr = 0.05
    ok = [i for i in range(13) if np.isfinite(q[i]).all()]
    bits = mc.host_bits(tags, allows[:13])
    lone = mc.Lone(idx, q, allows)
    want_u = {i: idx.search_batch(q[i], 20) for i in ok}
    want_h = {i: idx.search_batch(q[i], 20, keep_bitset=bits[i]) for i in ok}
    for i in ok:
        lone(i, 20), lone(i, 20, _lib.MODE_PIPELINE, thr)
    errs = []

    def work(t):
        try:
            for rep in range(5):
                for i in ok[t % 4::4]:
                    kind = t % 4
                    if kind == 0:
                        got, want = idx.search_batch(q[i], 20), want_u[i]
                        want = (want[0][0], want[1][0], want[2][0])
                    elif kind == 1:
                        got, want = idx.search_batch(q[i], 20, keep_bitset=bits[i]), want_h[i]
                        want = (want[0][0], want[1][0], want[2][0])
                    else:
                        mode, th = (_lib.MODE_RAW, 0.0) if kind == 2 else (_lib.MODE_PIPELINE, thr)
                        got, want = idx.search_tagged_batch(q[i], 20, allows[i], mode=mode, threshold=th), lone(i, 20, mode, th)
                    mc.same_query((got[0][0], got[1][0], got[2][0]), want, (t, rep, i))
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errs.append((t, repr(e)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(12)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs
    assert not idx.is_poisoned()
    idx.close()


def test_poisoned_handle_wakes_every_parked_tagged_caller(hip, storm_data):
    """The host-side fail-next hook (no device fault involved) fails one pass: its leader reports the device error, everybody
    else POISONED, nobody stays parked."""
    rows, qs, tags, allows = storm_data
    idx = mc.tagged_index(rows, tags)
    hip.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_index_fail_next.restype = None
    codes, lock, start = [], threading.Lock(), threading.Barrier(9)

    def work(t):
        start.wait()
        for rep in range(40):
            i = (t + rep) % len(qs)
            try:
                idx.search_tagged_batch(qs[i], 20, allows[i])
            except HipError as e:
                with lock:
                    codes.append(e.code)

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [x.start() for x in th]
    start.wait()
    hip.cqs_hip_debug_index_fail_next(idx._h)
    [x.join(timeout=60) for x in th]
    assert not any(x.is_alive() for x in th), "a tagged caller is still parked on a poisoned handle"
    assert idx.is_poisoned()
    assert codes.count(_lib.ERR_DEVICE) == 1, codes
    assert codes.count(_lib.ERR_POISONED) == len(codes) - 1 and len(codes) >= 8, codes
    idx.close()
