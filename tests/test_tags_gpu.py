"""Row tags on the device (include/cqs_hip.h "row tags"): `cqs_hip_index_set_tags` / `_count_tagged` /
`_search_tagged`.  ONE rule is the test: a tagged call returns the bytes of `cqs_hip_index_search` on the same handle with
keep_bitset = the host bitset of the same predicate - rows, score bits, counts, status and message.  No tolerance anywhere.
The bitset the kernel writes is read back through the test hook and compared word for word with numpy's.  dim 64 throughout."""
import ctypes as C
import threading

import numpy as np
import pytest

import tags_cases as tc
from cqs_amd import DistanceMetric, HipError, HipIndex, _lib, synth, tag_filter

pytestmark = pytest.mark.gpu

DIM = 64
N_BIG = 70001
ROW_COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 5000, N_BIG)
SENTINEL = 0xDEADBEEF


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def data(hip):
    rows = synth.gaussian_unit(N_BIG, DIM, seed=9100)
    q = synth.gaussian_unit(9, DIM, seed=9101)
    tags = tc.unique_end_tags(N_BIG, 9102)
    tags[[3, 64, 65, 2047, 2048, 4095, 4999]] = 0x0B0B0B0B          # seven rows with a tag of their own, all below 5 000
    for a in (rows, q, tags):
        a.setflags(write=False)
    return rows, q, tags


def tagged_index(rows, tags, metric=DistanceMetric.Cosine, row_base=0):
    idx = HipIndex.build_from_flat(None, rows, metric, row_base=row_base)
    idx.set_tags(tags, first=row_base)
    assert idx.tagged_rows() == len(tags) == len(idx)
    return idx


@pytest.fixture(scope="module")
def indexes(data):
    rows, _q, tags = data
    made = {}

    def get(n, metric=DistanceMetric.Cosine):
        if (n, metric) not in made:
            made[(n, metric)] = tagged_index(rows[:n], tags[:n], metric)
        return made[(n, metric)]
    yield get
    for idx in made.values():
        idx.close()


def assert_same(got, want, what=""):
    (gr, gs, gc), (wr, ws, wc) = got, want
    assert np.array_equal(gc, wc), (what, gc, wc)
    assert np.array_equal(gr, wr), what
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), what


def hook_words(hip, idx, allow):
    n = len(idx)
    words = np.full((n + 31) // 32 + 2, 0xA5A5A5A5, dtype=np.uint32)   # (two guard words behind the bitset)
    a = np.ascontiguousarray(allow, dtype=np.uint32)
    assert hip.cqs_hip_debug_index_tag_keep(idx._h, _ptr(a), _ptr(words)) == _lib.OK, idx.last_error()
    assert words[-1] == words[-2] == 0xA5A5A5A5
    return words[:-2]


# ---- the kernel's bitset and count -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_bitset_and_count(hip, data, n):
    rows, _q, _tags = data
    tags = tc.unique_end_tags(n, 9200 + n)
    idx = tagged_index(rows[:n], tags)
    filters = tc.filters_for(tags, 9300 + n)
    assert set(filters) >= {"all_pass", "empty_field_2", "half_full", "only_255", "first_row", "last_row"} and len(filters) == 10
    for name, allow in filters.items():
        mask = tc.keep_mask(tags, allow)
        want = tc.bits_of(mask)                                         # ceil(n / 32) words, the bits past n zero
        assert np.array_equal(hook_words(hip, idx, allow), want), (n, name)
        assert idx.count_tagged(allow) == int(mask.sum()), (n, name)
    assert idx.count_tagged(filters["all_pass"]) == n and idx.count_tagged(filters["empty_field_2"]) == 0
    assert idx.count_tagged(filters["first_row"]) == 1 and idx.count_tagged(filters["last_row"]) == 1
    assert int(tc.keep_mask(tags, filters["first_row"]).argmax()) == 0
    assert int(tc.keep_mask(tags, filters["last_row"]).argmax()) == n - 1
    assert not idx.is_poisoned()
    idx.close()


# ---- search bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", (DistanceMetric.Cosine, DistanceMetric.DotProduct))
@pytest.mark.parametrize("n", (5000, N_BIG))
def test_search_bytes(data, indexes, n, metric):
    _rows, q, tags = data
    idx = indexes(n, metric)
    filters = tc.filters_for(tags[:n], 9400 + n)
    for name in ("half_full", "one_value_field_0", "one_value_field_3", "only_255"):
        allow = filters[name]
        mask = tc.keep_mask(tags[:n], allow)
        assert 0 < mask.sum() < n, name
        bits = tc.bits_of(mask)
        for b in (1, 3, 9):
            for k in (1, 20, 500):
                got = idx.search_tagged_batch(q[:b], k, allow)
                want = idx.search_batch(q[:b], k, keep_bitset=bits)
                assert_same(got, want, (n, metric, name, b, k))
                assert list(got[2]) == [min(k, int(mask.sum()))] * b


@pytest.mark.parametrize("n", (5000, N_BIG))
def test_pipeline_mode_with_a_threshold(data, indexes, n):
    _rows, q, tags = data
    idx = indexes(n)
    allow = tc.filters_for(tags[:n], 9400 + n)["half_full"]
    bits = tc.bits_of(tc.keep_mask(tags[:n], allow))
    for b in (1, 3, 9):
        for thr in (0.0, 0.3, 0.45):
            got = idx.search_tagged_batch(q[:b], 20, allow, mode=_lib.MODE_PIPELINE, threshold=thr)
            print("pipeline", n, b, thr, list(got[2]))
            assert_same(got, idx.search_batch(q[:b], 20, keep_bitset=bits, mode=_lib.MODE_PIPELINE, threshold=thr), (n, b, thr))


def test_seven_rows_and_nothing(data, indexes):
    _rows, q, tags = data
    for n in (5000, N_BIG):
        idx = indexes(n)
        seven = tag_filter([11])
        mask = tc.keep_mask(tags[:n], seven)
        assert int(mask.sum()) == 7 and idx.count_tagged(seven) == 7
        for b in (1, 3, 9):
            got = idx.search_tagged_batch(q[:b], 20, seven)
            assert list(got[2]) == [7] * b
            assert all(sorted(int(r) for r in got[0][i, :7]) == sorted(np.flatnonzero(mask)) for i in range(b))
            assert_same(got, idx.search_batch(q[:b], 20, keep_bitset=tc.bits_of(mask)), (n, b))
            nothing = tag_filter(None, None, [])
            got = idx.search_tagged_batch(q[:b], 20, nothing)
            assert list(got[2]) == [0] * b
            assert_same(got, idx.search_batch(q[:b], 20, keep_bitset=tc.bits_of(np.zeros(n, bool))), (n, b, "nothing"))


# ---- every rule of cqs_hip_index_search, against the host-bitset call ------------------------------------------------------
def _raw(lib, idx, q, b, qd, k, *, allow=None, keep=None, mode=_lib.MODE_RAW, tagged):
    q = np.ascontiguousarray(q, dtype=np.float32)
    rows = np.zeros((max(b, 1), max(k, 1)), dtype=np.uint64)
    scores = np.zeros((max(b, 1), max(k, 1)), dtype=np.float32)
    counts = np.full((max(b, 1),), SENTINEL, dtype=np.uint32)
    if tagged:
        a = np.ascontiguousarray(allow, dtype=np.uint32)
        rc = lib.cqs_hip_index_search_tagged(idx._h, _ptr(q), b, qd, k, _ptr(a), mode, 0.0, _ptr(rows), _ptr(scores), _ptr(counts))
    else:
        kb = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint32)
        rc = lib.cqs_hip_index_search(idx._h, _ptr(q), b, qd, k, _ptr(kb), mode, 0.0, _ptr(rows), _ptr(scores), _ptr(counts))
    return rc, counts, rows, scores.view(np.uint32), idx.last_error()


def _both(lib, idx, tags, allow, q, b, qd, k, mode=_lib.MODE_RAW):
    bits = tc.bits_of(tc.keep_mask(tags, allow))
    t = _raw(lib, idx, q, b, qd, k, allow=allow, mode=mode, tagged=True)
    h = _raw(lib, idx, q, b, qd, k, keep=bits, mode=mode, tagged=False)
    assert t[0] == h[0] and t[4] == h[4], (t[0], h[0], t[4], h[4])
    for x, y in zip(t[1:4], h[1:4]):
        assert np.array_equal(x, y)
    return t


def test_rules_carry_over(hip, data, indexes):
    _rows, q, tags = data
    n = 5000
    idx = indexes(n)
    tags = tags[:n]
    half = tc.filters_for(tags, 9400 + n)["half_full"]
    kept = int(tc.keep_mask(tags, half).sum())
    for allow in (half, tc.ALL):
        assert _both(hip, idx, tags, allow, q, 0, DIM, 20)[1][0] == SENTINEL                       # b = 0: nothing is touched
        for b in (1, 3):
            assert list(_both(hip, idx, tags, allow, q, b, DIM, 0)[1][:b]) == [0] * b              # k = 0
            t = _both(hip, idx, tags, allow, q[:, :48], b, 48, 20)                                 # dimension mismatch
            assert t[0] == _lib.OK and list(t[1][:b]) == [0] * b and t[4] == "search: query dimension mismatch (empty result)"
            t = _both(hip, idx, tags, allow, q, b, DIM, 1025)
            assert t[0] == _lib.ERR_INVALID and t[4] == "search: k > max_k" and list(t[1][:b]) == [0] * b
            t = _both(hip, idx, tags, allow, q, b, DIM, 20, mode=_lib.MODE_PIPELINE + 1)
            assert t[0] == _lib.ERR_INVALID and t[4] == "search: bad mode"
        bad = q.copy()
        bad[1, DIM - 1] = np.nan
        assert list(_both(hip, idx, tags, allow, bad, 3, DIM, 20)[1]) == [20, 0, 20]               # a non-finite query
        assert list(_both(hip, idx, tags, allow, bad[1], 1, DIM, 20)[1]) == [0]
        assert list(_both(hip, idx, tags, allow, bad[1:], 1, DIM, 20)[1]) == [0]
    # all-pass is the unfiltered search, bit for bit (and counts as one: the queue combines it)
    for b in (1, 3, 9):
        assert_same(idx.search_tagged_batch(q[:b], 20, tc.ALL), idx.search_batch(q[:b], 20), b)
    # a filter that is not all-ones but keeps every row: still the unfiltered answer, as an all-kept bitset gives it
    present = [sorted(set(int(v) for v in (tags >> np.uint32(8 * f)) & np.uint32(255))) for f in range(4)]
    every = tag_filter(*present)
    assert not np.array_equal(every, tc.ALL) and idx.count_tagged(every) == n
    for b in (1, 3):
        assert_same(idx.search_tagged_batch(q[:b], 20, every), idx.search_batch(q[:b], 20), b)
        _both(hip, idx, tags, every, q, b, DIM, 20)
    # k is capped at the kept rows
    few = tag_filter([11])
    t = _both(hip, idx, tags, few, q, 3, DIM, 500)
    assert list(t[1]) == [7, 7, 7]
    assert 20 <= kept < 1024 and list(_both(hip, idx, tags, half, q, 3, DIM, 1024)[1]) == [kept] * 3
    assert not idx.is_poisoned()


# ---- lifecycle -------------------------------------------------------------------------------------------------------
def _check_against_host_bitsets(idx, tags, q, seed, what):
    filters = tc.filters_for(tags, seed)
    for name in ("half_full", "one_value_field_1", "only_255", "last_row"):
        mask = tc.keep_mask(tags, filters[name])
        for b, k in ((1, 20), (3, 1), (9, 500)):
            assert_same(idx.search_tagged_batch(q[:b], k, filters[name]), idx.search_batch(q[:b], k, keep_bitset=tc.bits_of(mask)),
                        (what, name, b, k))


def test_extend_needs_tags_for_the_new_rows(data):
    rows, q, tags = data
    idx = tagged_index(rows[:3000], tags[:3000], row_base=100)
    half = tc.filters_for(tags[:3500], 9500)["half_full"]
    idx.extend(None, rows[3000:3500])                                   # (regrows the corpus, and the column with it)
    assert len(idx) == 3500 and idx.tagged_rows() == 3000
    with pytest.raises(HipError) as e:
        idx.search_tagged_batch(q[:3], 20, half)
    assert e.value.code == _lib.ERR_INVALID and "search_tagged: tags cover 3000 of 3500 rows" in str(e.value)
    with pytest.raises(HipError):
        idx.count_tagged(half)
    assert idx.search_tagged(q[0], 20, half) == [] and not idx.is_poisoned()
    assert list(idx.search_batch(q[:3], 20)[2]) == [20, 20, 20]         # still searchable
    idx.set_tags(tags[3000:3400], first=100 + 3000)                     # in two calls; the second overlaps the first
    assert idx.tagged_rows() == 3400
    idx.set_tags(tags[3300:3500], first=100 + 3300)
    assert idx.tagged_rows() == 3500
    _check_against_host_bitsets(idx, tags[:3500], q, 9501, "extended")
    assert len(idx.search_tagged(q[0], 20, half)) == 20
    idx.close()


@pytest.mark.parametrize("budget", (0, 97))
def test_remove_compacts_the_column(hip, data, budget):
    rows, q, tags = data
    n = 5000
    rng = np.random.default_rng(9600)
    gone = np.sort(rng.choice(n, size=1500, replace=False))
    kept_tags = np.delete(tags[:n], gone)
    a = tagged_index(rows[:n], tags[:n])
    hip.cqs_hip_debug_index_remove_budget(a._h, budget)                 # 97 rows per pass: the column moves in dozens of passes
    assert a.remove_rows(gone) == len(gone)
    assert a.tagged_rows() == len(a) == n - len(gone)
    f = tagged_index(np.delete(rows[:n], gone, axis=0), kept_tags)
    filters = tc.filters_for(kept_tags, 9601)
    for name, allow in filters.items():
        assert np.array_equal(hook_words(hip, a, allow), tc.bits_of(tc.keep_mask(kept_tags, allow))), name
        assert a.count_tagged(allow) == f.count_tagged(allow)
        for b, k in ((1, 20), (3, 500), (9, 1)):
            assert_same(a.search_tagged_batch(q[:b], k, allow), f.search_tagged_batch(q[:b], k, allow), (name, b, k))
    _check_against_host_bitsets(a, kept_tags, q, 9602, "removed")
    a.close(); f.close()
    # only part of the index tagged: the prefix follows the host rule, and the tags below it still sit on their rows
    p = HipIndex.build_from_flat(None, rows[:n], row_base=7)
    p.set_tags(tags[:2000], first=7)
    hip.cqs_hip_debug_index_remove_budget(p._h, budget)
    assert p.remove_rows(gone + 7) == len(gone)
    below = int((gone < 2000).sum())
    assert p.tagged_rows() == 2000 - below
    p.set_tags(kept_tags[2000 - below:], first=7 + 2000 - below)
    assert p.tagged_rows() == len(p)
    for name, allow in filters.items():
        assert np.array_equal(hook_words(hip, p, allow), tc.bits_of(tc.keep_mask(kept_tags, allow))), name
    p.close()


def test_remove_everything_refill_and_retag(data):
    rows, q, tags = data
    idx = tagged_index(rows[:600], tags[:600])
    assert idx.remove_rows(np.arange(600)) == 600
    assert len(idx) == 0 and idx.tagged_rows() == 0
    assert idx.count_tagged(tag_filter([0])) == 0
    assert list(idx.search_tagged_batch(q[:3], 20, tag_filter([0]))[2]) == [0, 0, 0]
    idx.extend(None, rows[1000:1800])
    assert idx.tagged_rows() == 0
    with pytest.raises(HipError):
        idx.search_tagged_batch(q[:1], 20, tag_filter([0]))
    idx.set_tags(tags[1000:1800])
    _check_against_host_bitsets(idx, tags[1000:1800], q, 9700, "refilled")
    idx.close()


def test_save_and_load_do_not_persist_tags(data, tmp_path):
    rows, q, tags = data
    idx = tagged_index(rows[:600], tags[:600])
    path = str(tmp_path / "t.hipflat")
    idx.save(path)
    loaded = HipIndex.load(path, DIM, 600)
    assert loaded.tagged_rows() == 0 and idx.tagged_rows() == 600
    with pytest.raises(HipError) as e:
        loaded.search_tagged_batch(q[:1], 20, tag_filter([0]))
    assert "tags cover 0 of 600 rows" in str(e.value)
    loaded.set_tags(tags[:600])
    allow = tc.filters_for(tags[:600], 9800)["half_full"]
    assert_same(loaded.search_tagged_batch(q[:3], 20, allow), idx.search_tagged_batch(q[:3], 20, allow))
    idx.close(); loaded.close()


def test_shadow_serves_tagged_searches(data):
    rows, q, tags = data
    n = 5000
    idx = tagged_index(rows[:n], tags[:n])
    allow = tc.filters_for(tags[:n], 9900)["half_full"]
    bits = tc.bits_of(tc.keep_mask(tags[:n], allow))
    plain = {(b, k): idx.search_batch(q[:b], k, keep_bitset=bits) for b in (1, 3, 8) for k in (20, 500)}
    idx.set_bf16_scan(True)
    assert idx.bf16_stats()[0] > 0, idx.last_error()
    for (b, k), want in plain.items():
        _by, c0, f0 = idx.bf16_stats()
        got = idx.search_tagged_batch(q[:b], k, allow)
        _by, c1, f1 = idx.bf16_stats()
        host = idx.search_batch(q[:b], k, keep_bitset=bits)
        _by, c2, f2 = idx.bf16_stats()
        # the tagged call went through the shadow exactly where the host-bitset call does (at k = 20: every query)
        assert (c1 - c0) + (f1 - f0) == (c2 - c1) + (f2 - f1), (b, k)
        if k == 20:
            assert (c1 - c0) + (f1 - f0) == b, (b, k, c0, c1, f0, f1)
        assert_same(got, host, (b, k))
        assert_same(got, want, (b, k, "f32"))                           # and the shadow changes no byte
    assert idx.bf16_stats()[1] > 0
    idx.close()


# ---- invalid calls ---------------------------------------------------------------------------------------------------
def test_invalid_calls_leave_the_handle_untouched(hip, data):
    rows, q, tags = data
    n = 3000
    idx = HipIndex.build_from_flat(None, rows[:n], row_base=50)
    idx.set_tags(tags[:2000], first=50)
    t = np.ascontiguousarray(tags[:100])

    def set_tags(first, ptr, m):
        return hip.cqs_hip_index_set_tags(idx._h, first, ptr, m), idx.last_error()
    assert set_tags(50 + 2001, _ptr(t), 10) == (_lib.ERR_INVALID, "set_tags: gap: first row past the tagged rows")
    assert set_tags(49, _ptr(t), 10) == (_lib.ERR_INVALID, "set_tags: first row below this index")
    big = np.ascontiguousarray(tags[:2000])
    assert set_tags(50 + 1500, _ptr(big), 1501) == (_lib.ERR_INVALID, "set_tags: range past the end of the index")
    assert set_tags(50, None, 10) == (_lib.ERR_INVALID, "set_tags: null tags")
    assert set_tags(50 + 9999, None, 0)[0] == _lib.OK                    # m == 0: nothing, whatever the arguments
    assert idx.tagged_rows() == 2000 and len(idx) == n and not idx.is_poisoned()
    idx.set_tags(tags[2000:n], first=50 + 2000)
    half = tc.filters_for(tags[:n], 9950)["half_full"]
    before = idx.search_tagged_batch(q[:3], 20, half)
    assert before[0].min() >= 50                                        # global row ids
    out = (np.zeros((3, 20), np.uint64), np.zeros((3, 20), np.float32), np.full(3, SENTINEL, np.uint32))
    rc = hip.cqs_hip_index_search_tagged(idx._h, _ptr(q), 3, DIM, 20, None, 0, 0.0, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]))
    assert rc == _lib.ERR_INVALID and idx.last_error() == "search_tagged: null allow" and list(out[2]) == [SENTINEL] * 3
    kept = C.c_uint64(5)
    assert hip.cqs_hip_index_count_tagged(idx._h, None, C.byref(kept)) == _lib.ERR_INVALID and kept.value == 0
    assert not idx.is_poisoned() and idx.tagged_rows() == n
    assert_same(idx.search_tagged_batch(q[:3], 20, half), before, "after invalid calls")
    # a row-sharded handle: stated as not built, and it still searches
    s = HipIndex.build_sharded(None, rows[:n], [0, 0])
    want = s.search_batch(q[:3], 20)
    with pytest.raises(HipError) as e:
        s.set_tags(tags[:n])
    assert e.value.code == _lib.ERR_INVALID and "set_tags: not built for a row-sharded handle" in str(e.value)
    with pytest.raises(HipError) as e:
        s.search_tagged_batch(q[:3], 20, half)
    assert e.value.code == _lib.ERR_INVALID and "search_tagged: not built for a row-sharded handle" in str(e.value)
    with pytest.raises(HipError):
        s.count_tagged(half)
    assert s.tagged_rows() == 0 and not s.is_poisoned()
    assert_same(s.search_batch(q[:3], 20), want, "sharded after the refused calls")
    s.close()
    # a poisoned handle (the hook cqs_hip_index_search's tests use): the failing call reports the device error, later ones POISONED
    hip.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_index_fail_next.restype = None
    hip.cqs_hip_debug_index_fail_next(idx._h)
    with pytest.raises(HipError) as e:
        idx.search_tagged_batch(q[:3], 20, half)
    assert e.value.code == _lib.ERR_DEVICE and idx.is_poisoned()
    for call in (lambda: idx.search_tagged_batch(q[:3], 20, half), lambda: idx.search_tagged_batch(q[:3], 20, tc.ALL),
                 lambda: idx.count_tagged(half), lambda: idx.set_tags(tags[:10], first=50)):
        with pytest.raises(HipError) as e:
            call()
        assert e.value.code == _lib.ERR_POISONED
    idx.close()


def test_a_borrowed_handle_may_have_tags(data):
    import torch
    rows, q, tags = data
    n = 3000
    d = torch.from_numpy(np.ascontiguousarray(rows[:n])).cuda()
    b = HipIndex.build_from_device(None, d.data_ptr(), n, DIM, borrow=True, keepalive=d)
    b.set_tags(tags[:n])
    assert b.tagged_rows() == n
    _check_against_host_bitsets(b, tags[:n], q, 9960, "borrowed")
    b.close()


# ---- threads ---------------------------------------------------------------------------------------------------------
def test_tagged_and_plain_callers_share_a_handle(data, indexes):
    _rows, q, tags = data
    n = 5000
    idx = indexes(n)
    filters = tc.filters_for(tags[:n], 9400 + n)
    allows = [filters["half_full"], filters["one_value_field_0"], filters["only_255"], tag_filter([11])]
    lone_tagged = [idx.search_tagged_batch(q[i], 20, allows[i]) for i in range(4)]
    lone_plain = [idx.search_batch(q[4 + i], 20) for i in range(4)]
    errors = []

    def tagged(i):
        try:
            for _ in range(30):
                assert_same(idx.search_tagged_batch(q[i], 20, allows[i]), lone_tagged[i], ("tagged", i))
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errors.append(e)

    def plain(i):
        try:
            for _ in range(30):
                assert_same(idx.search_batch(q[4 + i], 20), lone_plain[i], ("plain", i))
        except BaseException as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=tagged, args=(i,)) for i in range(4)] + [threading.Thread(target=plain, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:1]
    assert not idx.is_poisoned()
