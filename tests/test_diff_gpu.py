"""`cqs_hip_index_diff` / `HipIndex.diff_rows` / `semantic_diff` / `detect_drift` (include/cqs_hip.h): the
cosines of matched pairs of two resident indexes, the pairs below a threshold compacted in pair order.

The yardstick is oracle.full_cosine_similarity (src/math.rs:35-67, pinned by the reference's KATs), pair by pair: bit for
bit on tests/diff_cases.py's exact data, equal or adjacent f32 on random data - the f64 sums carry ~dim * 2^-53 relative
error in any order, far below half an f32 ulp, so only a value on a rounding boundary can move, and then by one.  Run on an
MI355X with `pytest -m gpu`."""
import threading

import numpy as np
import pytest

import diff_cases as dc
from cqs_amd import DistanceMetric, HipError, HipIndex, _lib

pytestmark = pytest.mark.gpu
FILL = 7


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def raw_diff(a, b, ra, rb, thr, sims=True, lists=True, counts=True, m=None):
    """The C ABI with pattern-filled outputs of len(ra) + 3 slots: (rc, sims, mod_pairs, mod_sims, counts), whole arrays."""
    ra, rb = np.ascontiguousarray(ra, np.uint64), np.ascontiguousarray(rb, np.uint64)
    n = len(ra) + 3
    o_sims, o_pairs, o_msims = np.full(n, FILL, np.float32), np.full(n, FILL, np.uint64), np.full(n, FILL, np.float32)
    o_counts = np.full(3, FILL, np.uint64)
    p = lambda arr, on: arr.ctypes.data if on else None
    rc = a._lib.cqs_hip_index_diff(a._h, ra.ctypes.data, b._h, rb.ctypes.data, len(ra) if m is None else m, float(thr), p(o_sims, sims),
                                   p(o_pairs, lists), p(o_msims, lists), p(o_counts, counts))
    return rc, o_sims, o_pairs, o_msims, o_counts


def untouched(*arrays):
    return all((np.asarray(x) == FILL).all() for x in arrays)


def oracle_sims(oracle, a, b, ra, rb):
    """(sims f32 [m], undefined bool [m]) by the oracle, one pair at a time."""
    sims, undefined = np.zeros(len(ra), np.float32), np.zeros(len(ra), bool)
    for i in range(len(ra)):
        s = oracle.full_cosine_similarity(a[int(ra[i])], b[int(rb[i])])
        undefined[i] = s is None
        sims[i] = 0.0 if s is None else s
    return sims, undefined


def adjacent_or_equal(got, want):
    return (bits(got) == bits(want)) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


def assert_answer(got, sims, undefined, thr, ctx, want_sims=None):
    """A raw_diff answer against per-pair sims (the call's own, or the oracle's where they must be its bits): out_sims, both
    lists in full, all three counts, and nothing written past them."""
    rc, o_sims, o_pairs, o_msims, o_counts = got
    m = len(sims)
    assert rc == _lib.OK, ctx
    if want_sims is not False:
        assert np.array_equal(bits(o_sims[:m]), bits(sims)), ctx
    mod, mod_sims, counts = dc.expected_answer(sims, undefined, thr)
    assert list(o_counts) == counts, (ctx, list(o_counts), counts)
    assert np.array_equal(o_pairs[:len(mod)], mod) and np.array_equal(bits(o_msims[:len(mod)]), bits(mod_sims)), ctx
    assert untouched(o_pairs[len(mod):], o_msims[len(mod):]) and (want_sims is False or untouched(o_sims[m:])), ctx


@pytest.mark.parametrize("dim", dc.DIMS)
def test_exact_data_bit_for_bit_against_the_oracle(hip, oracle, dim):
    a, b = dc.corpora(dim)
    ia, ib = HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b)
    ra, rb = dc.pairs(max(dc.MS))
    want, undefined = oracle_sims(oracle, a, b, ra, rb)
    assert undefined[0] and want[1] == 1.0 and want[2] == -1.0 and want[3] == 0.0 and want[4] == 1.0   # zero, identical, negated, orthogonal, scaled
    for m in dc.MS:
        for thr in dc.thresholds(want[:m], undefined[:m]):
            assert_answer(raw_diff(ia, ib, ra[:m], rb[:m], thr), want[:m], undefined[:m], thr, (dim, m, float(thr)))
    # without out_sims: only the lists and the counts
    got = raw_diff(ia, ib, ra[:257], rb[:257], 0.5, sims=False)
    assert untouched(got[1])
    assert_answer(got, want[:257], undefined[:257], 0.5, (dim, "no out_sims"), want_sims=False)
    # without the lists: sims and counts
    got = raw_diff(ia, ib, ra[:257], rb[:257], 0.5, lists=False)
    assert got[0] == _lib.OK and untouched(got[2], got[3]) and np.array_equal(bits(got[1][:257]), bits(want[:257]))
    assert list(got[4]) == dc.expected_answer(want[:257], undefined[:257], 0.5)[2]
    ia.close(); ib.close()


@pytest.fixture(scope="module")
def random_pair(hip):
    """dim -> (A, B, index of A, index of B, rows_a, rows_b): unit rows at 768, non-unit at 252; B's rows are A's, some
    perturbed a little, some a lot, so the cosines spread from ~0 to 1."""
    made = {}

    def get(dim):
        if dim not in made:
            rng = np.random.default_rng(500 + dim)
            n = 1500
            a = rng.standard_normal((n, dim)).astype(np.float32)
            noise = rng.standard_normal((n, dim)).astype(np.float32) * rng.choice(np.array([0.02, 0.3, 1.0, 3.0], np.float32), size=(n, 1))
            b = (a + noise).astype(np.float32)
            if dim == 768:
                a /= np.linalg.norm(a, axis=1, keepdims=True)
                b /= np.linalg.norm(b, axis=1, keepdims=True)
            else:
                a *= np.float32(41.0)
            ra = np.concatenate([np.arange(n), rng.integers(0, n, 500)]).astype(np.uint64)
            rb = np.concatenate([np.arange(n), rng.integers(0, n, 500)]).astype(np.uint64)
            made[dim] = (a, b, HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b), ra, rb)
        return made[dim]

    yield get
    for v in made.values():
        v[2].close(); v[3].close()


@pytest.fixture(scope="module")
def random_ref(random_pair, oracle):
    """dim -> the oracle's (sims, undefined) of random_pair(dim)'s pairs, computed once."""
    made = {}

    def get(dim):
        if dim not in made:
            a, b, _, _, ra, rb = random_pair(dim)
            made[dim] = oracle_sims(oracle, a, b, ra, rb)
        return made[dim]
    return get


@pytest.mark.parametrize("dim", (768, 252))
def test_random_data_equal_or_adjacent_and_classified_as_the_oracle(random_pair, random_ref, oracle, dim):
    a, b, ia, ib, ra, rb = random_pair(dim)
    want, undefined = random_ref(dim)
    assert not undefined.any()
    # the threshold: the midpoint of two adjacent distinct oracle values, with no oracle value within one ulp of it - so a
    # device value one ulp off its oracle value still falls on the oracle's side
    vals = np.unique(want)
    lo = len(vals) // 3
    thr = np.float32((np.float64(vals[lo]) + np.float64(vals[lo + 1])) / 2.0)
    below, above = np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf))
    assert ((want < below) | (want > above)).all() and 0 < (want < thr).sum() < len(want)
    rc, sims, pairs, msims, counts = raw_diff(ia, ib, ra, rb, thr)
    m = len(ra)
    assert rc == _lib.OK
    ok = adjacent_or_equal(sims[:m], want)
    print(f"dim {dim}: {int((bits(sims[:m]) != bits(want)).sum())} of {m} sims one ulp from the oracle's, {int((~ok).sum())} further")
    assert ok.all()
    mod = np.flatnonzero(want < thr)
    assert list(counts) == [len(mod), m - len(mod), 0]
    assert np.array_equal(pairs[:len(mod)], mod.astype(np.uint64)) and np.array_equal(bits(msims[:len(mod)]), bits(sims[mod]))
    assert untouched(pairs[len(mod):], msims[len(mod):], sims[m:])
    # a stored row holding a NaN (extend takes rows unchecked) is undefined: 0.0, counted, classified through its 0.0
    bad = a[:1].copy()
    bad[0, dim - 1] = np.nan
    ix = HipIndex.build_from_flat(None, a[:10])
    ix.extend(None, bad)
    for t, n_mod in ((0.5, 1), (0.0, 0)):
        rc, sims, pairs, msims, counts = raw_diff(ix, ia, [3, 10], [3, 3], t)                # (row 3 against itself, the NaN row against row 3)
        assert rc == _lib.OK and bits(sims[1]) == 0 and list(counts) == [n_mod, 2 - n_mod, 1] and list(pairs[:n_mod]) == [1][:n_mod]
        assert oracle.full_cosine_similarity(bad[0], a[3]) is None
    ix.close()


def set_budget(idx, pairs):
    idx._lib.cqs_hip_debug_index_diff_budget(idx._h, pairs)


def test_a_pairs_sim_depends_on_its_rows_alone(random_pair, random_ref):
    a, b, ia, ib, ra, rb = random_pair(768)
    m = 700
    ra, rb = ra[900:900 + m], rb[900:900 + m]                                 # (the identity pairing's tail and the random pairs' head)
    rc, sims, pairs, msims, counts = raw_diff(ia, ib, ra, rb, 0.6)
    n_mod = int(counts[0])
    assert rc == _lib.OK and 0 < n_mod < m
    whole = (bits(sims[:m]).copy(), pairs[:n_mod].copy(), bits(msims[:n_mod]).copy(), list(counts))
    # passes: the budget cuts the call, the answer stays
    for budget in (1, 64, 100):
        set_budget(ia, budget)
        rc, s2, p2, ms2, c2 = raw_diff(ia, ib, ra, rb, 0.6)
        assert rc == _lib.OK and np.array_equal(bits(s2[:m]), whole[0]) and np.array_equal(p2[:n_mod], whole[1]), budget
        assert np.array_equal(bits(ms2[:n_mod]), whole[2]) and list(c2) == whole[3] and untouched(p2[n_mod:], ms2[n_mod:], s2[m:]), budget
    set_budget(ia, 0)
    # shuffled: every pair keeps its bits; the list is the shuffled call's own filter
    perm = np.random.default_rng(3).permutation(m)
    rc, s2, p2, ms2, c2 = raw_diff(ia, ib, ra[perm], rb[perm], 0.6)
    assert rc == _lib.OK and np.array_equal(bits(s2[:m]), whole[0][perm]) and list(c2) == whole[3]
    assert np.array_equal(p2[:n_mod], np.flatnonzero(s2[:m] < np.float32(0.6)).astype(np.uint64))
    # repeated: the list twice over, and a single pair alone (another grid)
    rc, s2, p2, ms2, c2 = raw_diff(ia, ib, np.concatenate([ra, ra]), np.concatenate([rb, rb]), 0.6)
    assert rc == _lib.OK and np.array_equal(bits(s2[:m]), whole[0]) and np.array_equal(bits(s2[m:2 * m]), whole[0]) and int(c2[0]) == 2 * n_mod
    assert np.array_equal(p2[:2 * n_mod], np.concatenate([whole[1], whole[1] + np.uint64(m)]))
    for i in (0, 333, m - 1):
        rc, s2, _, _, _ = raw_diff(ia, ib, ra[i:i + 1], rb[i:i + 1], 0.6)
        assert rc == _lib.OK and bits(s2[:1])[0] == whole[0][i]
    # (a, b) against (b, a): the same bits
    rc, s2, p2, ms2, c2 = raw_diff(ib, ia, rb, ra, 0.6)
    assert rc == _lib.OK and np.array_equal(bits(s2[:m]), whole[0]) and np.array_equal(p2[:n_mod], whole[1]) and list(c2) == whole[3]


def test_one_handle_on_both_sides(random_pair, oracle):
    a, _, ia, _, ra, rb = random_pair(252)
    ra, rb = ra[1400:1700], rb[1400:1700]                                     # rows 1400 .. 1499 against themselves, then random pairs
    want, undefined = oracle_sims(oracle, a, a, ra, rb)
    rc, sims, pairs, msims, counts = raw_diff(ia, ia, ra, rb, 0.5)
    m = len(ra)
    assert rc == _lib.OK and adjacent_or_equal(sims[:m], want).all() and int(counts[0]) + int(counts[1]) == m and int(counts[2]) == 0
    assert (sims[:100] > np.float32(0.999999)).all() and int(counts[1]) >= 100                       # rows 1400 .. 1499 against themselves
    assert np.array_equal(pairs[:int(counts[0])], np.flatnonzero(sims[:m] < np.float32(0.5)).astype(np.uint64))


def test_row_base_on_each_side_and_a_borrowing_handle(random_pair):
    import torch
    a, b, ia, ib, ra, rb = random_pair(768)
    ra, rb = ra[1300:1700], rb[1300:1700]
    rc, sims, pairs, msims, counts = raw_diff(ia, ib, ra, rb, 0.7)
    assert rc == _lib.OK
    ja = HipIndex.build_from_flat(None, a, row_base=5000)
    d = torch.from_numpy(b).cuda()
    jb = HipIndex.build_from_device(None, d.data_ptr(), b.shape[0], b.shape[1], row_base=123, borrow=True, keepalive=d)
    for x, y, rx, ry in ((ja, jb, ra + np.uint64(5000), rb + np.uint64(123)), (jb, ja, rb + np.uint64(123), ra + np.uint64(5000)),
                         (ja, ib, ra + np.uint64(5000), rb), (ia, jb, ra, rb + np.uint64(123))):
        got = raw_diff(x, y, rx, ry, 0.7)
        assert got[0] == _lib.OK and all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got[1:], (sims, pairs, msims, counts)))
    # a local row number where a global one belongs is outside the index
    got = raw_diff(ja, jb, ra, rb + np.uint64(123), 0.7)
    assert got[0] == _lib.ERR_INVALID and untouched(*got[1:]) and ja.last_error() == "diff: pair 0: row of a not in its index"
    ja.close(); jb.close()


def test_after_update_and_remove_the_diff_sees_the_new_rows(hip, oracle):
    rng = np.random.default_rng(71)
    a = rng.standard_normal((600, 252)).astype(np.float32)
    b = (a + rng.standard_normal((600, 252)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    ia, ib = HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b)
    ra = rb = np.arange(600, dtype=np.uint64)
    assert raw_diff(ia, ib, ra, rb, 0.8)[0] == _lib.OK
    rows = rng.choice(600, 200, replace=False)
    b[rows] = a[rows] * np.float32(-2.0)
    assert ib.update_rows(rows, b[rows]) == 200
    want, undefined = oracle_sims(oracle, a, b, ra, rb)
    rc, sims, pairs, msims, counts = raw_diff(ia, ib, ra, rb, 0.8)
    assert rc == _lib.OK and adjacent_or_equal(sims[:600], want).all() and (sims[rows] < np.float32(-0.999999)).all()
    assert np.array_equal(pairs[:int(counts[0])], np.flatnonzero(sims[:600] < np.float32(0.8)).astype(np.uint64)) and int(counts[0]) >= 200
    gone = np.sort(rng.choice(600, 150, replace=False))
    assert ib.remove_rows(gone) == 150
    b = np.delete(b, gone, axis=0)
    ra = rb = np.arange(450, dtype=np.uint64)
    want, undefined = oracle_sims(oracle, a, b, ra, rb)
    rc, sims, pairs, msims, counts = raw_diff(ia, ib, ra, rb, 0.8)
    assert rc == _lib.OK and adjacent_or_equal(sims[:450], want).all() and int(counts[0]) + int(counts[1]) == 450
    assert np.array_equal(pairs[:int(counts[0])], np.flatnonzero(sims[:450] < np.float32(0.8)).astype(np.uint64))
    got = raw_diff(ia, ib, [0], [450], 0.8)                                                          # the removed rows are gone
    assert got[0] == _lib.ERR_INVALID and ia.last_error() == "diff: pair 0: row of b not in its index"
    ia.close(); ib.close()


def test_refusals_leave_everything_as_it_was(random_pair):
    a, b, ia, ib, ra, rb = random_pair(768)
    _, _, ic, _, _, _ = random_pair(252)
    q = a[:3].copy()
    before = (ia.search_batch(q, 20), ib.search_batch(q, 20))
    ra, rb = ra[:50].copy(), rb[:50].copy()
    far_a, far_b = ra.copy(), rb.copy()
    far_a[7] = len(ia)
    far_b[3] = 2 ** 40
    sh = HipIndex.build_sharded(None, a[:600], [0, 0], DistanceMetric.Cosine)
    lib = ia._lib

    def refused(x, y, why, owner=None, **kw):
        args = dict(ra=ra, rb=rb, thr=0.5)
        args.update(kw)
        got = raw_diff(x, y, args.pop("ra"), args.pop("rb"), args.pop("thr"), **args)
        assert got[0] == _lib.ERR_INVALID and untouched(*got[1:]), why
        assert (owner or x).last_error() == "diff: " + why
        assert not x.is_poisoned() and not y.is_poisoned()

    refused(ia, ib, "pair 7: row of a not in its index", ra=far_a)
    refused(ia, ib, "pair 3: row of b not in its index", rb=far_b)
    refused(ia, ib, "pair 3: row of b not in its index", ra=far_a, rb=far_b)                         # the first offending pair
    refused(ia, ic, "the two handles differ in dim")
    refused(ic, ia, "the two handles differ in dim")
    refused(ia, ib, "threshold is NaN", thr=np.nan)
    refused(ia, ib, "null out_counts", counts=False)
    refused(sh, ib, "not built for a row-sharded handle")
    refused(ia, sh, "not built for a row-sharded handle")
    refused(sh, sh, "not built for a row-sharded handle", ra=far_a, rb=far_b)                        # (before the rows are looked at)
    refused(ia, ic, "threshold is NaN", thr=np.nan, ra=far_a)                                        # the documented order: NaN, dim, rows
    refused(ia, ic, "the two handles differ in dim", ra=far_a)
    # exactly one of the two list outputs; null row lists
    n = len(ra) + 3
    o = [np.full(n, FILL, np.float32), np.full(n, FILL, np.uint64), np.full(n, FILL, np.float32), np.full(3, FILL, np.uint64)]
    call = lambda pa, pb, p1, p2: lib.cqs_hip_index_diff(ia._h, pa, ib._h, pb, 50, 0.5, o[0].ctypes.data, p1, p2, o[3].ctypes.data)
    assert call(ra.ctypes.data, rb.ctypes.data, o[1].ctypes.data, None) == _lib.ERR_INVALID and ia.last_error() == "diff: out_mod_pairs and out_mod_sims go together"
    assert call(ra.ctypes.data, rb.ctypes.data, None, o[2].ctypes.data) == _lib.ERR_INVALID and untouched(*o)
    assert call(None, rb.ctypes.data, o[1].ctypes.data, o[2].ctypes.data) == _lib.ERR_INVALID and ia.last_error() == "diff: null rows_a"
    assert call(ra.ctypes.data, None, o[1].ctypes.data, o[2].ctypes.data) == _lib.ERR_INVALID and ia.last_error() == "diff: null rows_b" and untouched(*o)
    # a null handle on either side; m == 0 asks for nothing and zeroes the counts
    assert lib.cqs_hip_index_diff(ia._h, ra.ctypes.data, None, rb.ctypes.data, 50, 0.5, *(x.ctypes.data for x in o)) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_diff(None, ra.ctypes.data, ib._h, rb.ctypes.data, 50, 0.5, *(x.ctypes.data for x in o)) == _lib.ERR_INVALID and untouched(*o)
    got = raw_diff(ia, ic, far_a, far_b, np.nan, m=0)
    assert got[0] == _lib.OK and list(got[4]) == [0, 0, 0] and untouched(*got[1:4])
    assert lib.cqs_hip_index_diff(ia._h, None, ib._h, None, 0, 0.5, None, None, None, None) == _lib.OK
    with pytest.raises(HipError) as e:
        ia.diff_rows(ib, far_a, rb, 0.5)
    assert e.value.code == _lib.ERR_INVALID and "pair 7: row of a" in str(e.value)
    # a diff that runs leaves both handles' searches as they were
    assert raw_diff(ia, ib, ra, rb, 0.5)[0] == _lib.OK and raw_diff(ia, sh, ra, rb, 0.5)[0] == _lib.ERR_INVALID
    after = (ia.search_batch(q, 20), ib.search_batch(q, 20))
    for x, y in zip(before, after):
        assert all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(x, y))
    assert not ia.is_poisoned() and not ib.is_poisoned() and not sh.is_poisoned()
    sh.close()


def test_a_poisoned_handle_on_either_side(hip):
    """The library's injection hook fails one host search as a device error would (no device fault): that handle is poisoned,
    a diff that names it on either side answers POISONED with the outputs untouched, and the other handle stays usable."""
    import ctypes as C
    hip.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_index_fail_next.restype = None
    rows = np.random.default_rng(8).standard_normal((64, 8)).astype(np.float32)
    good, bad = HipIndex.build_from_flat(None, rows), HipIndex.build_from_flat(None, rows)
    hip.cqs_hip_debug_index_fail_next(bad._h)
    with pytest.raises(HipError):
        bad.search_batch(rows[:1], 3)
    assert bad.is_poisoned() and not good.is_poisoned()
    r = np.arange(10, dtype=np.uint64)
    for x, y in ((good, bad), (bad, good), (bad, bad)):
        got = raw_diff(x, y, r, r, 0.5)
        assert got[0] == _lib.ERR_POISONED and untouched(*got[1:])
    got = raw_diff(good, good, r, r, 0.5)
    assert got[0] == _lib.OK and list(got[4]) == [0, 10, 0] and not good.is_poisoned()
    good.close(); bad.close()


def test_python_mirror_end_to_end(hip, oracle):
    """semantic_diff / detect_drift over two small named indexes: the device's similarities under the host's matching."""
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((6, 64)).astype(np.float32)
    src = HipIndex.build_from_flat(["f:keep", "f:gone", "f:turned", "f:near", "f:dup#1", "f:dup#2"], rows)
    tgt_rows = np.stack([rows[2] * np.float32(-1.0), rows[0] * np.float32(3.0), rows[3] + np.float32(0.05) * rows[1], rows[5], rows[1] + rows[4]]).astype(np.float32)
    tgt = HipIndex.build_from_flat(["f:turned", "f:keep", "f:near", "f:dup#9", "f:new"], tgt_rows, row_base=40)
    d = src.semantic_diff(tgt, 0.9999, key=lambda cid: cid.split("#")[0])
    assert [x.id for x in d.added] == ["f:new"] and [x.id for x in d.removed] == ["f:gone"] and d.unchanged_count == 2
    assert [x.id for x in d.modified] == ["f:turned", "f:near"]
    near = oracle.full_cosine_similarity(rows[3], tgt_rows[2])
    assert adjacent_or_equal(np.float32([d.modified[0].similarity, d.modified[1].similarity]), np.float32([-1.0, near])).all()
    r = src.detect_drift(tgt, 0.9999, 0.5)
    assert [x.id for x in r.drifted] == ["f:turned"] and r.total_compared == 3 and r.unchanged == 1      # (no key: dup matches nothing)
    assert r.drifted[0].drift == float(np.float32(1.0) - np.float32(r.drifted[0].similarity))
    mod, msims, counts, sims = src.diff_rows(tgt, [0, 2], [41, 40], 0.0, want_sims=True)
    assert list(mod) == [1] and list(counts) == [1, 1, 0] and sims[0] > 0.999999 and msims[0] == sims[1]
    src.close(); tgt.close()


def test_threads_diff_both_ways_beside_searches(random_pair):
    a, b, ia, ib, ra, rb = random_pair(768)
    ra, rb = ra[:1200], rb[:1200]
    q = b[5:6].copy()
    lone_ab, lone_ba = raw_diff(ia, ib, ra, rb, 0.6), raw_diff(ib, ia, rb, ra, 0.6)
    lone_sa, lone_sb = ia.search_batch(q, 10), ib.search_batch(q, 10)
    assert lone_ab[0] == _lib.OK and lone_ba[0] == _lib.OK
    same = lambda x, y: all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(x, y))
    wrong = []

    def work(fn, lone):
        for _ in range(25):
            if not same(fn(), lone):
                wrong.append(fn)

    threads = [threading.Thread(target=work, args=(lambda: raw_diff(ia, ib, ra, rb, 0.6)[1:], lone_ab[1:])),
               threading.Thread(target=work, args=(lambda: raw_diff(ib, ia, rb, ra, 0.6)[1:], lone_ba[1:])),
               threading.Thread(target=work, args=(lambda: raw_diff(ia, ia, ra, ra, 0.6)[4:], raw_diff(ia, ia, ra, ra, 0.6)[4:])),
               threading.Thread(target=work, args=(lambda: ia.search_batch(q, 10), lone_sa)),
               threading.Thread(target=work, args=(lambda: ib.search_batch(q, 10), lone_sb))]
    for t in threads:
        t.daemon = True
        t.start()
    for t in threads:
        t.join(timeout=60)                                                       # a lock-order mistake fails here instead of stalling
    assert not any(t.is_alive() for t in threads), "a thread is stuck: the two handles' mutexes were taken in different orders"
    assert not wrong and not ia.is_poisoned() and not ib.is_poisoned()
