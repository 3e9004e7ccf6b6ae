"""`cqs_hip_index_match` / `HipIndex.match_rows` / `semantic_diff(..., moved_threshold=...)` (include/cqs_hip.h, DESIGN.md
§3.17a): for two lists of stored rows of two resident indexes, the best partner of every row on the other side.

The yardsticks: integer arithmetic on tests/match_cases.py's exact data; `cqs_hip_index_pairwise` over one index that
holds both corpora, bit for bit, on general data (an entry is the Gram kernel's fma chain of its two rows); numpy f64 at
the library's parity tolerance for the mid-size case.  Every case goes through the C ABI.  Run on an MI355X with
`pytest -m gpu`."""
import numpy as np
import pytest

import match_cases as mc
from cqs_amd import DistanceMetric, HipError, HipIndex, _lib

pytestmark = pytest.mark.gpu
FILL = 7
bits = mc.bits


def raw_match(a, b, ra, rb, m_a=None, m_b=None, null=()):
    """The C ABI with pattern-filled outputs of len + 3 slots: (rc, best_a, score_a, best_b, score_b), whole arrays.
    `null`: names among rows_a, rows_b, best_a, score_a, best_b, score_b to pass as NULL."""
    ra, rb = np.ascontiguousarray(ra, np.uint64), np.ascontiguousarray(rb, np.uint64)
    o = [np.full(len(ra) + 3, FILL, np.uint64), np.full(len(ra) + 3, FILL, np.float32),
         np.full(len(rb) + 3, FILL, np.uint64), np.full(len(rb) + 3, FILL, np.float32)]
    p = lambda arr, name: None if name in null else arr.ctypes.data
    rc = a._lib.cqs_hip_index_match(a._h, p(ra, "rows_a"), len(ra) if m_a is None else m_a, b._h, p(rb, "rows_b"),
                                    len(rb) if m_b is None else m_b, p(o[0], "best_a"), p(o[1], "score_a"), p(o[2], "best_b"), p(o[3], "score_b"))
    return (rc,) + tuple(o)


def untouched(*arrays):
    return all((np.asarray(x) == FILL).all() for x in arrays)


def assert_bests(got, want, ctx):
    """A raw_match answer against (best_a, score_a, best_b, score_b): positions, score bits, nothing written past them."""
    rc, *out = got
    assert rc == _lib.OK, ctx
    for side, (g, w) in enumerate(zip(out, want)):
        m = len(w)
        same = np.array_equal(g[:m], w) if side % 2 == 0 else np.array_equal(bits(g[:m]), bits(w))
        assert same, (ctx, "best_a score_a best_b score_b".split()[side], g[:m][:8], w[:8])
        assert untouched(g[m:]), ctx


# ---- 1. exact data, two indexes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact(hip):
    a, b = mc.exact_corpora()
    ia, ib = HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b)
    yield a, b, ia, ib, mc.exact_scores(a, b)
    ia.close(); ib.close()


@pytest.mark.parametrize("m_a", mc.LENGTHS)
def test_exact_data_positions_and_score_bits(exact, m_a):
    a, b, ia, ib, s = exact
    ties = 0
    for m_b in mc.LENGTHS:
        ra, rb = mc.row_list(mc.EXACT_NA, m_a, 100 + m_a), mc.row_list(mc.EXACT_NB, m_b, 200 + m_b)
        sub = s[np.ix_(ra.astype(np.int64), rb.astype(np.int64))]
        want = mc.expected_bests(sub)
        assert_bests(raw_match(ia, ib, ra, rb), want, (m_a, m_b))
        ties += int((sub == want[1][:, None]).sum() - m_a)                      # entries that tie with their row's best
        assert m_a < 3 or len(set(ra.tolist())) < m_a                           # a stored row at more than one position
    assert m_a == 1 or ties > 0


# ---- 2. general data, bit for bit against pairwise over one index of both corpora ---------------------------------------
@pytest.fixture(scope="module")
def general(hip):
    """dim -> (a, b, index of a, index of b, index of a's rows followed by b's)."""
    made = {}

    def get(dim):
        if dim not in made:
            a, b = mc.gaussian_rows(700, dim, 30 + dim), mc.gaussian_rows(900, dim, 31 + dim)
            made[dim] = (a, b, HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b),
                         HipIndex.build_from_flat(None, np.concatenate([a, b])))
        return made[dim]

    yield get
    for v in made.values():
        for ix in v[2:]:
            ix.close()


def pairwise_block(iab, n_a, ra, rb):
    """S[rows_a, rows_b] by cqs_hip_index_pairwise over the joint index (len(ra) + len(rb) <= 1024)."""
    assert len(ra) + len(rb) <= _lib.MMR_MAX
    g = iab.pairwise_rows(np.concatenate([ra, rb + np.uint64(n_a)]))
    return np.ascontiguousarray(g[:len(ra), len(ra):])


@pytest.mark.parametrize("dim", mc.GENERAL_DIMS)
def test_general_data_bit_for_bit_against_pairwise(general, dim):
    a, b, ia, ib, iab = general(dim)
    rng = np.random.default_rng(dim)
    for m_a, m_b in ((300, 700), (97, 33), (1, 500)):
        ra = rng.choice(len(a), m_a, replace=False).astype(np.uint64)
        rb = rng.choice(len(b), m_b, replace=False).astype(np.uint64)
        s = pairwise_block(iab, len(a), ra, rb)
        want = mc.expected_bests(s)
        assert_bests(raw_match(ia, ib, ra, rb), want, (dim, m_a, m_b))
        # (b, a): the same entries, the roles exchanged
        assert_bests(raw_match(ib, ia, rb, ra), want[2:] + want[:2], (dim, m_a, m_b, "swapped"))


# ---- 3. one handle on both sides ------------------------------------------------------------------------------------------
def test_one_handle_overlapping_lists(general):
    a, _, ia, _, _ = general(768)
    ra = np.array(list(range(100, 160)) + [120, 130], np.uint64)                 # rows 100 .. 159, then 120 and 130 again
    rb = np.array([130, 120] + list(range(110, 170)) + [115], np.uint64)         # 130, 120, rows 110 .. 169, then 115 again
    rc, best_a, score_a, best_b, score_b = raw_match(ia, ia, ra, rb)
    assert rc == _lib.OK
    diag = np.diagonal(ia.pairwise_rows(np.arange(100, 170, dtype=np.uint64)))   # the rows' dots with themselves
    for i, row in enumerate(ra):
        where = np.flatnonzero(rb == row)
        if len(where):                                                           # unit rows: nothing beats a row's own copy
            assert best_a[i] == where[0] and bits(score_a[i]) == bits(diag[int(row) - 100]), (i, row)
    assert best_a[20] == 1 and best_a[60] == 1 and best_a[30] == 0 and best_a[15] == 7    # rows 120 (twice), 130, 115: the lowest position
    for j, row in enumerate(rb):
        where = np.flatnonzero(ra == row)
        if len(where):
            assert best_b[j] == where[0] and bits(score_b[j]) == bits(diag[int(row) - 100]), (j, row)
    want = mc.expected_bests(ia.pairwise_rows(np.concatenate([ra, rb]))[:len(ra), len(ra):])
    assert_bests((rc, best_a, score_a, best_b, score_b), want, "a is b")


# ---- 4. ties across tiles -------------------------------------------------------------------------------------------------
def test_ties_across_tiles_go_to_the_lowest_position(general):
    a, b, ia, ib, iab = general(100)
    rng = np.random.default_rng(4)
    ra, rb = rng.choice(len(a), 90, replace=False).astype(np.uint64), rng.choice(len(b), 90, replace=False).astype(np.uint64)
    # the stored row of b that A row ra[0] likes best of all, at positions 3, 40 and 70 (tiles 0, 1 and 2); likewise on the A side
    rb[[3, 40, 70]] = int(np.argmax(b.astype(np.float64) @ a[int(ra[0])].astype(np.float64)))
    ra[[3, 40, 70]] = int(np.argmax(a.astype(np.float64) @ b[int(rb[0])].astype(np.float64)))
    s = pairwise_block(iab, len(a), ra, rb)
    want = mc.expected_bests(s)
    got = raw_match(ia, ib, ra, rb)
    assert_bests(got, want, "ties")
    assert (bits(s[:, 3]) == bits(s[:, 40])).all() and (bits(s[:, 3]) == bits(s[:, 70])).all()
    assert (bits(s[3]) == bits(s[40])).all() and (bits(s[3]) == bits(s[70])).all()
    first_b, first_a = int(np.flatnonzero(rb == rb[3])[0]), int(np.flatnonzero(ra == ra[3])[0])      # (3, unless the draw had the row earlier)
    assert got[1][0] == first_b and not np.isin(got[1][:90], (40, 70)).any()     # the lowest position, never a later copy
    assert got[3][0] == first_a and not np.isin(got[3][:90], (40, 70)).any()


# ---- 5. non-finite entries ------------------------------------------------------------------------------------------------
def test_non_finite_entries_never_win(hip):
    big = np.float32(3e38)
    a = np.array([[big, 0, 0, 0], [-big, 0, 0, 0], [1, 2, 0, 0], [0, 0, 1, 0], [0.5, 0, 0, 1]], np.float32)
    b = np.array([[big, 0, 0, 0], [2, 1, 0, 0], [-big, 0, 0, 0], [0, 0, 0, 3], [big, 0, 0, 0]], np.float32)
    ia = HipIndex.build_from_flat(None, a, metric=DistanceMetric.DotProduct)
    ib = HipIndex.build_from_flat(None, b, metric=DistanceMetric.DotProduct)
    s = np.zeros((5, 5), np.float32)                                             # the fma chain over k = 0 .. 3: every step exact or an overflow
    with np.errstate(over="ignore"):
        for k in range(4):
            s = (a[:, k].astype(np.float64)[:, None] * b[:, k].astype(np.float64)[None, :] + s.astype(np.float64)).astype(np.float32)
    assert np.isinf(s[0, [0, 1, 2, 4]]).all() and s[0, 2] < 0 and s[1, 2] > 0 and np.isfinite(s[2]).all() and not np.isnan(s).any()
    r5 = np.arange(5, dtype=np.uint64)
    want = mc.expected_bests(s)
    assert_bests(raw_match(ia, ib, r5, r5), want, "overflow")
    assert want[0][0] == 3 and want[0][1] == 3 and bits(want[1][:2]).tolist() == [0, 0]   # rows 0 and 1: their one finite entry, not +inf
    assert want[0][2] == 0 and want[1][2] == np.float32(3e38)                     # a huge finite entry wins as any other, the lower of two equal ones
    # a row whose every entry overflows: (NONE, 0.0), on both sides
    rb = np.array([0, 2, 4, 0], np.uint64)
    ra = np.array([0, 1, 0], np.uint64)
    rc, best_a, score_a, best_b, score_b = raw_match(ia, ib, ra, rb)
    assert rc == _lib.OK and (best_a[:3] == mc.NONE).all() and (bits(score_a[:3]) == 0).all()
    assert (best_b[:4] == mc.NONE).all() and (bits(score_b[:4]) == 0).all() and untouched(best_a[3:], score_a[3:], best_b[4:], score_b[4:])
    # an empty other side: the same for every row, and the empty side's outputs may be NULL
    for null in ((), ("rows_b", "best_b", "score_b")):
        rc, best_a, score_a, best_b, score_b = raw_match(ia, ib, r5, np.zeros(0, np.uint64), null=null)
        assert rc == _lib.OK and (best_a[:5] == mc.NONE).all() and (bits(score_a[:5]) == 0).all() and untouched(best_a[5:], score_a[5:], best_b, score_b)
    rc, best_a, score_a, best_b, score_b = raw_match(ia, ib, np.zeros(0, np.uint64), r5, null=("rows_a", "best_a", "score_a"))
    assert rc == _lib.OK and (best_b[:5] == mc.NONE).all() and (bits(score_b[:5]) == 0).all() and untouched(best_a, score_a, best_b[5:], score_b[5:])
    # both empty: nothing touched, whatever else is passed
    got = raw_match(ia, ib, r5, r5, m_a=0, m_b=0)
    assert got[0] == _lib.OK and untouched(*got[1:])
    assert ia._lib.cqs_hip_index_match(ia._h, None, 0, ib._h, None, 0, None, None, None, None) == _lib.OK
    ia.close(); ib.close()


# ---- 6. row_base on both handles, a borrowing handle ------------------------------------------------------------------------
def test_row_base_on_each_side_and_a_borrowing_handle(general):
    import torch
    a, b, ia, ib, _ = general(768)
    rng = np.random.default_rng(6)
    ra, rb = rng.choice(len(a), 150, replace=False).astype(np.uint64), rng.choice(len(b), 210, replace=False).astype(np.uint64)
    ra[:2], rb[:2] = [0, len(a) - 1], [len(b) - 1, 0]                            # both ends of each index
    want = raw_match(ia, ib, ra, rb)
    assert want[0] == _lib.OK
    ja = HipIndex.build_from_flat(None, a, row_base=5000)
    d = torch.from_numpy(b).cuda()
    jb = HipIndex.build_from_device(None, d.data_ptr(), b.shape[0], b.shape[1], row_base=123, borrow=True, keepalive=d)
    for x, y, rx, ry in ((ja, jb, ra + np.uint64(5000), rb + np.uint64(123)), (ja, ib, ra + np.uint64(5000), rb), (ia, jb, ra, rb + np.uint64(123))):
        got = raw_match(x, y, rx, ry)
        assert got[0] == _lib.OK and all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got[1:], want[1:]))
    got = raw_match(jb, ja, rb + np.uint64(123), ra + np.uint64(5000))
    assert got[0] == _lib.OK and all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got[1:], want[3:] + want[1:3]))
    # a local row number where a global one belongs is outside the index
    got = raw_match(ja, jb, ra, rb + np.uint64(123))
    assert got[0] == _lib.ERR_INVALID and untouched(*got[1:]) and ja.last_error() == "match: rows_a[0] not in its index"
    ja.close(); jb.close()


# ---- 7. after extend, remove and update ---------------------------------------------------------------------------------------
def test_after_extend_remove_and_update_the_match_sees_the_rows_now_stored(hip):
    rng = np.random.default_rng(7)
    a, b = mc.gaussian_rows(400, 100, 70), mc.gaussian_rows(500, 100, 71)
    ia, ib = HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b)
    assert raw_match(ia, ib, np.arange(50, dtype=np.uint64), np.arange(60, dtype=np.uint64))[0] == _lib.OK     # (staging made before the changes)
    more = mc.gaussian_rows(64, 100, 72)
    ia.extend(None, more)
    a = np.concatenate([a, more])
    gone = np.sort(rng.choice(500, 120, replace=False))
    assert ib.remove_rows(gone) == 120
    b = np.delete(b, gone, axis=0)
    rows = rng.choice(len(b), 90, replace=False)
    b[rows] = a[rng.choice(len(a), 90, replace=False)] * np.float32(0.5)
    assert ib.update_rows(rows, b[rows]) == 90
    changed = rng.choice(len(a), 30, replace=False)
    a[changed] = mc.gaussian_rows(30, 100, 73)
    assert ia.update_rows(changed, a[changed]) == 30
    fa, fb = HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b)
    ra, rb = np.arange(len(a), dtype=np.uint64), np.arange(len(b), dtype=np.uint64)
    got, want = raw_match(ia, ib, ra, rb), raw_match(fa, fb, ra, rb)
    assert got[0] == _lib.OK and want[0] == _lib.OK
    assert all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got[1:], want[1:]))
    s64 = a.astype(np.float64) @ b.astype(np.float64).T
    assert np.abs(got[2][:len(a)] - s64.max(axis=1)).max() < 1e-5 and np.abs(got[4][:len(b)] - s64.max(axis=0)).max() < 1e-5
    assert (got[1][:len(a)][464 - 64:464] < len(b)).all()                        # the extended rows have partners
    got = raw_match(ia, ib, ra, np.array([len(b)], np.uint64))                   # the removed rows are gone
    assert got[0] == _lib.ERR_INVALID and ia.last_error() == "match: rows_b[0] not in its index"
    for ix in (ia, ib, fa, fb):
        ix.close()


# ---- 8. every refusal -------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(general):
    a, b, ia, ib, _ = general(768)
    _, _, ic, _, _ = general(100)
    q = a[:3].copy()
    before = (ia.search_batch(q, 20), ib.search_batch(q, 20))
    ra, rb = np.arange(40, dtype=np.uint64), np.arange(50, dtype=np.uint64)
    far_a, far_b = ra.copy(), rb.copy()
    far_a[7] = len(ia)
    far_b[3] = 2 ** 40
    sh = HipIndex.build_sharded(None, a[:600], [0, 0], DistanceMetric.Cosine)
    lib = ia._lib

    def refused(x, y, why, **kw):
        args = dict(ra=ra, rb=rb)
        args.update(kw)
        got = raw_match(x, y, args.pop("ra"), args.pop("rb"), **args)
        assert got[0] == _lib.ERR_INVALID and untouched(*got[1:]), why
        assert x.last_error() == "match: " + why
        assert not x.is_poisoned() and not y.is_poisoned()

    refused(ia, ib, "null rows_a", null=("rows_a",))
    refused(ia, ib, "null rows_b", null=("rows_b",))
    for name, side in (("best_a", "a"), ("score_a", "a"), ("best_b", "b"), ("score_b", "b")):
        refused(ia, ib, f"null output of side {side}", null=(name,))
    refused(ia, ib, "m_a above CQS_HIP_MATCH_MAX", m_a=_lib.MATCH_MAX + 1)         # (refused before a row is read)
    refused(ia, ib, "m_b above CQS_HIP_MATCH_MAX", m_b=_lib.MATCH_MAX + 1)
    refused(sh, ib, "not built for a row-sharded handle")
    refused(ia, sh, "not built for a row-sharded handle")
    refused(ia, ic, "the two handles differ in dim")
    refused(ic, ia, "the two handles differ in dim")
    refused(ia, ib, "rows_a[7] not in its index", ra=far_a)
    refused(ia, ib, "rows_b[3] not in its index", rb=far_b)
    refused(ia, ib, "rows_a[7] not in its index", ra=far_a, rb=far_b)               # side a first
    # the documented order: each call has everything wrong that comes later
    refused(ia, sh, "null rows_a", null=("rows_a", "best_b"), m_b=_lib.MATCH_MAX + 1, ra=far_a)
    refused(ia, sh, "null output of side b", null=("best_b",), m_b=_lib.MATCH_MAX + 1, ra=far_a)
    refused(ia, sh, "m_b above CQS_HIP_MATCH_MAX", m_b=_lib.MATCH_MAX + 1, ra=far_a)
    refused(ic, sh, "not built for a row-sharded handle", ra=far_a)
    refused(ic, ib, "the two handles differ in dim", ra=far_a, rb=far_b)
    # a null handle on either side comes before everything, both lists empty included
    o = [np.full(43, FILL, np.uint64), np.full(43, FILL, np.float32), np.full(53, FILL, np.uint64), np.full(53, FILL, np.float32)]
    ptrs = [x.ctypes.data for x in o]
    assert lib.cqs_hip_index_match(ia._h, ra.ctypes.data, 40, None, rb.ctypes.data, 50, *ptrs) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_match(None, ra.ctypes.data, 40, ib._h, rb.ctypes.data, 50, *ptrs) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_match(None, None, 0, ib._h, None, 0, *ptrs) == _lib.ERR_INVALID and untouched(*o)
    # both lists empty is accepted before the later checks: a sharded handle, other dims, NULL everything
    assert lib.cqs_hip_index_match(ic._h, None, 0, sh._h, None, 0, None, None, None, None) == _lib.OK
    with pytest.raises(HipError) as e:
        ia.match_rows(ib, far_a, rb)
    assert e.value.code == _lib.ERR_INVALID and "rows_a[7]" in str(e.value)
    # a match that runs, and the refusals before it, leave both handles' searches as they were
    assert raw_match(ia, ib, ra, rb)[0] == _lib.OK
    after = (ia.search_batch(q, 20), ib.search_batch(q, 20))
    for x, y in zip(before, after):
        assert all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(x, y))
    assert not ia.is_poisoned() and not ib.is_poisoned() and not ic.is_poisoned() and not sh.is_poisoned()
    sh.close()


def test_a_poisoned_handle_on_either_side(hip):
    """The library's injection hook fails one host search as a device error would (no device fault): a match that names
    that handle on either side answers POISONED with the outputs untouched, and the other handle stays usable."""
    import ctypes as C
    hip.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_index_fail_next.restype = None
    rows = mc.gaussian_rows(64, 8, 8)                                            # unit rows: a row's best partner is itself
    good, bad = HipIndex.build_from_flat(None, rows), HipIndex.build_from_flat(None, rows)
    hip.cqs_hip_debug_index_fail_next(bad._h)
    with pytest.raises(HipError):
        bad.search_batch(rows[:1], 3)
    assert bad.is_poisoned() and not good.is_poisoned()
    r = np.arange(10, dtype=np.uint64)
    for x, y in ((good, bad), (bad, good), (bad, bad)):
        got = raw_match(x, y, r, r)
        assert got[0] == _lib.ERR_POISONED and untouched(*got[1:])
    got = raw_match(good, good, r, r)
    assert got[0] == _lib.OK and list(got[1][:10]) == list(range(10)) and not good.is_poisoned()
    good.close(); bad.close()


# ---- 9. determinism -----------------------------------------------------------------------------------------------------------
def test_same_call_same_bytes_and_a_permuted_list_permutes_the_answer(general):
    a, b, ia, ib, iab = general(768)
    rng = np.random.default_rng(9)
    n_a, n_b = 301, 707
    ra, rb = rng.choice(len(a), n_a, replace=False).astype(np.uint64), rng.choice(len(b), n_b, replace=False).astype(np.uint64)
    one, two = raw_match(ia, ib, ra, rb), raw_match(ia, ib, ra, rb)
    assert one[0] == _lib.OK and all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(one[1:], two[1:]))
    perm = rng.permutation(n_b)
    got = raw_match(ia, ib, ra, rb[perm])
    assert got[0] == _lib.OK
    inv = np.argsort(perm)                                                       # the new position of old position j
    s = pairwise_block(iab, len(a), ra, rb)                                      # where a row's best score occurs once in its row of S, the
    lone_a = (bits(s) == bits(one[2][:n_a])[:, None]).sum(axis=1) == 1           # partner is the same stored row wherever it is listed
    assert lone_a.mean() > 0.99
    assert np.array_equal(got[1][:n_a][lone_a], inv[one[1][:n_a].astype(np.int64)].astype(np.uint64)[lone_a]) and np.array_equal(bits(got[2][:n_a]), bits(one[2][:n_a]))
    assert np.array_equal(got[3][:n_b], one[3][:n_b][perm]) and np.array_equal(bits(got[4][:n_b]), bits(one[4][:n_b][perm]))   # (rows_a keeps its order)
    # an entry does not depend on the lists around it: one row against the whole of rows_b (another grid)
    for i in (0, 100, n_a - 1):
        lone = raw_match(ia, ib, ra[i:i + 1], rb)
        assert lone[0] == _lib.OK and lone[1][0] == one[1][i] and bits(lone[2][:1])[0] == bits(one[2][i:i + 1])[0]


# ---- 10. the mid-size case against numpy f64 -----------------------------------------------------------------------------------
def test_mid_size_against_numpy_f64(hip):
    a, b, ra, rb = mc.mid_case()
    (na_best, na_top, na_clear), (nb_best, nb_top, nb_clear) = mc.mid_reference(a, b, ra, rb)
    assert (~na_clear).mean() <= mc.MID_TIE_SHARE and (~nb_clear).mean() <= mc.MID_TIE_SHARE
    ia, ib = HipIndex.build_from_flat(None, a), HipIndex.build_from_flat(None, b)
    rc, best_a, score_a, best_b, score_b = raw_match(ia, ib, ra, rb)
    assert rc == _lib.OK
    ea, eb = np.abs(score_a[:mc.MID_MA] - na_top).max(), np.abs(score_b[:mc.MID_MB] - nb_top).max()
    print(f"mid-size: max |score - f64| {ea:.3e} (a) {eb:.3e} (b); near ties {int((~na_clear).sum())} of {mc.MID_MA}, {int((~nb_clear).sum())} of {mc.MID_MB}")
    assert ea <= mc.MID_SCORE_TOL and eb <= mc.MID_SCORE_TOL
    assert np.array_equal(best_a[:mc.MID_MA][na_clear], na_best[na_clear]) and np.array_equal(best_b[:mc.MID_MB][nb_clear], nb_best[nb_clear])
    assert untouched(best_a[mc.MID_MA:], score_a[mc.MID_MA:], best_b[mc.MID_MB:], score_b[mc.MID_MB:])
    # HipIndex.match_rows in blocks that do not divide the lists: the one call's bytes
    got = ia.match_rows(ib, ra, rb, block=700)
    for g, w, m in zip(got, (best_a, score_a, best_b, score_b), (mc.MID_MA, mc.MID_MA, mc.MID_MB, mc.MID_MB)):
        assert np.array_equal(g.view(np.uint8), w[:m].view(np.uint8))
    ia.close(); ib.close()


# ---- 11. semantic_diff end to end ------------------------------------------------------------------------------------------------
def test_semantic_diff_reports_moved_chunks(hip):
    rows = mc.gaussian_rows(8, 64, 110)
    noise = mc.gaussian_rows(1, 64, 111)[0]
    renamed = rows[2] + np.float32(0.1) * noise
    renamed = (renamed / np.linalg.norm(renamed)).astype(np.float32)
    src = HipIndex.build_from_flat(["a.rs:keep", "a.rs:moves", "a.rs:old_name", "a.rs:deleted", "a.rs:edited"], rows[:5])
    tgt_rows = np.stack([rows[0], rows[1], renamed, rows[5], rows[4] + np.float32(0.8) * rows[6]]).astype(np.float32)
    tgt = HipIndex.build_from_flat(["a.rs:keep", "b.rs:moves", "a.rs:new_name", "a.rs:brand_new", "a.rs:edited"], tgt_rows, row_base=40)
    plain = src.semantic_diff(tgt, 0.95)
    assert [x.id for x in plain.added] == ["b.rs:moves", "a.rs:new_name", "a.rs:brand_new"] and plain.moved == []
    assert [x.id for x in plain.removed] == ["a.rs:moves", "a.rs:old_name", "a.rs:deleted"]
    assert [x.id for x in plain.modified] == ["a.rs:edited"] and plain.unchanged_count == 1
    assert plain == src.semantic_diff(tgt, 0.95, moved_threshold=None)
    d = src.semantic_diff(tgt, 0.95, moved_threshold=0.9)
    assert [(m.source_id, m.target_id) for m in d.moved] == [("a.rs:old_name", "a.rs:new_name"), ("a.rs:moves", "b.rs:moves")]   # least similar first
    assert 0.9 <= d.moved[0].similarity < 0.9999 and abs(d.moved[1].similarity - 1.0) < 1e-5
    assert [x.id for x in d.added] == ["a.rs:brand_new"] and [x.id for x in d.removed] == ["a.rs:deleted"]
    assert d.modified == plain.modified and d.unchanged_count == plain.unchanged_count
    # a threshold nothing reaches moves nothing; NaN is refused
    assert src.semantic_diff(tgt, 0.95, moved_threshold=1.5) == plain
    with pytest.raises(ValueError):
        src.semantic_diff(tgt, 0.95, moved_threshold=float("nan"))
    src.close(); tgt.close()
