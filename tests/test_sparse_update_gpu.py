"""cqs_hip_sparse_index_remove / cqs_hip_sparse_index_extend on the device.  ONE rule is the test: after
either call the handle is indistinguishable from a handle freshly built (`build_from_csr`) from the resulting documents
with the resulting id order - equal len / unique_tokens / postings, the same bytes from every search (with and without a
keep mask, single and batched, and from one query that names every token, so every directory entry of every list is
read), and the same file out of `save`.  No tolerance anywhere; `oracle.SpladeIndex` is the yardstick of the searches
themselves."""
import threading

import numpy as np
import pytest

import sparse_cases as sc

pytestmark = pytest.mark.gpu

N, VOCAB = 3000, 200


@pytest.fixture(scope="module")
def S(hip):
    from cqs_amd import splade_index
    return splade_index


@pytest.fixture(scope="module")
def base():
    """The default shape, never modified: 3 000 chunks, vocabulary 200, 4-12 postings per chunk (about 24 k postings, lists
    from 1 to about 2 000 postings), plus a pool of further documents to extend with."""
    rng = np.random.default_rng(20240611)
    off, tok, w = sc.corpus(rng, N, VOCAB, 4, 12, dup_frac=0.3, special=True)
    xoff, xtok, xw = sc.corpus(rng, N, VOCAB, 4, 12, dup_frac=0.3, special=True)
    tok, xtok = tok + np.uint32(1), xtok + np.uint32(1)             # token ids 1 .. 200: id 0 stays free for a token no chunk uses
    ids = ["c%05d" % i for i in rng.permutation(2 * N)]            # string ids in shuffled order
    for a in (off, tok, w, xoff, xtok, xw):
        a.setflags(write=False)
    return dict(doc=(off, tok, w), extra=(xoff, xtok, xw), ids=tuple(ids[:N]), extra_ids=tuple(ids[N:]))


# ---- documents as CSR arrays ------------------------------------------------------------------------------------------
def csr_take(csr, docs):
    off, tok, w = csr
    docs = np.asarray(docs, dtype=np.int64)
    lens = (off[1:] - off[:-1]).astype(np.int64)[docs]
    new_off = np.zeros(docs.size + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum(lens)
    starts = off[:-1].astype(np.int64)[docs]
    idx = np.repeat(starts - new_off[:-1].astype(np.int64), lens) + np.arange(int(new_off[-1]), dtype=np.int64)
    return new_off, tok[idx], w[idx]


def csr_delete(csr, gone):
    n = csr[0].size - 1
    return csr_take(csr, np.delete(np.arange(n), np.unique(np.asarray(gone, dtype=np.int64))))


def csr_concat(a, b):
    return (np.concatenate([a[0], b[0][1:] + a[0][-1]]).astype(np.uint64), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]))


class Model:
    """The documents and ids a handle should hold, kept beside it."""

    def __init__(self, S, csr, ids=None, id_rank=None):
        self.S, self.csr, self.ids = S, tuple(np.array(a) for a in csr), None if ids is None else list(ids)
        self.rank = None if id_rank is None else np.asarray(id_rank, dtype=np.uint32)     # explicit ranks (ids None)
        self.ix = S.HipSpladeIndex.build_from_csr(self.ids, *self.csr, id_rank=self.rank)

    @property
    def n(self):
        return self.csr[0].size - 1

    def fresh(self):
        return self.S.HipSpladeIndex.build_from_csr(self.ids, *self.csr, id_rank=self.rank)

    def remove(self, chunks):
        gone = np.unique(np.asarray(chunks, dtype=np.int64))
        if self.ids is not None:
            got = self.ix.remove([self.ids[int(c)] for c in chunks])
            gone_set = set(gone.tolist())
            self.ids = [cid for i, cid in enumerate(self.ids) if i not in gone_set]
        else:
            got = self.ix.remove_chunks(chunks)
        assert got == gone.size
        if self.rank is not None:
            self.rank = np.argsort(np.argsort(np.delete(self.rank, gone))).astype(np.uint32)
        self.csr = csr_delete(self.csr, gone)
        assert self.ix.id_map == self.ids

    def extend(self, csr, ids=None, new_rank=None):
        self.ix.extend_csr(ids, *csr, new_rank=new_rank)
        if self.rank is not None:
            total = self.n + csr[0].size - 1
            if new_rank is None:
                self.rank = np.concatenate([self.rank, np.arange(self.n, total, dtype=np.uint32)])
            else:
                free = np.setdiff1d(np.arange(total, dtype=np.uint32), np.asarray(new_rank, dtype=np.uint32))
                self.rank = np.concatenate([free[self.rank], np.asarray(new_rank, dtype=np.uint32)])
        self.csr = csr_concat(self.csr, csr)
        if ids is not None:
            self.ids = self.ids + list(ids)
        assert self.ix.id_map == self.ids

    def close(self):
        self.ix.close()


def _bytes(res):
    return tuple(np.ascontiguousarray(a).tobytes() for a in res[:-1]) + (res[-1],)


def assert_rule(m, oracle, tmp_path=None, queries=3, seed=1):
    """The full rule for model `m`: its handle against a fresh build of its documents."""
    ix, fresh = m.ix, m.fresh()
    try:
        n = m.n
        assert len(ix) == len(fresh) == n
        assert ix.unique_tokens() == fresh.unique_tokens()
        assert ix.postings() == fresh.postings() == int(m.csr[0][-1])
        rng = np.random.default_rng(seed)
        vocab = np.unique(m.csr[1])
        qs = []
        for _ in range(queries):
            t = rng.choice(vocab, size=min(24, vocab.size), replace=False).astype(np.uint32) if vocab.size else np.array([5], np.uint32)
            t = np.concatenate([t, np.array([VOCAB + 9], dtype=np.uint32)])         # and a token nobody has
            qs.append((t, (rng.random(t.size, dtype=np.float32) * 2 + 0.05).astype(np.float32)))
        masks = [None] + ([rng.random(n) < 0.5, rng.random(n) < 0.05] if n else [])
        for qt, qw in qs:
            for k in (1, 500, 1024):
                for keep in masks:
                    assert _bytes(ix.search_raw(qt, qw, k, keep)) == _bytes(fresh.search_raw(qt, qw, k, keep)), (k, keep is None)
        for keep in masks:
            assert _bytes(ix.search_batch_raw(qs, 500, keep)) == _bytes(fresh.search_batch_raw(qs, 500, keep))
        # every token of the vocabulary in one query: every directory entry of every list is read
        if vocab.size:
            every = (vocab.astype(np.uint32), np.ones(vocab.size, dtype=np.float32))
            a, b = ix.search_raw(*every, 1024), fresh.search_raw(*every, 1024)
            assert a[2] == 0 and _bytes(a) == _bytes(b)
        if n and oracle is not None:
            o = oracle.SpladeIndex(*m.csr, ids=m.ids, id_rank=m.rank)
            oc, os_ = o.search_raw(qs[0][0], qs[0][1], 500, masks[1])
            hc, hs, rc = ix.search_raw(qs[0][0], qs[0][1], 500, masks[1])
            assert rc == 0 and np.array_equal(hc, oc) and np.array_equal(hs.view(np.uint32), os_.view(np.uint32))
        if tmp_path is not None:
            pa, pb = str(tmp_path / "updated.bin"), str(tmp_path / "fresh.bin")
            assert ix.save(pa, 41) == fresh.save(pb, 41)
            assert open(pa, "rb").read() == open(pb, "rb").read()
            back = m.S.HipSpladeIndex.load(pa, 41, m.ids)
            assert back is not None and len(back) == n
            if vocab.size:
                assert _bytes(back.search_raw(qs[0][0], qs[0][1], 500)) == _bytes(ix.search_raw(qs[0][0], qs[0][1], 500))
            back.close()
    finally:
        fresh.close()


def _model(S, base, ranked):
    return Model(S, base["doc"], base["ids"] if ranked else None)


def _extra(base, lo, hi, ranked):
    return csr_take(base["extra"], np.arange(lo, hi)), (base["extra_ids"][lo:hi] if ranked else None)


RANKED = pytest.mark.parametrize("ranked", [True, False], ids=["ranked", "unranked"])


# ---- remove -----------------------------------------------------------------------------------------------------------
@RANKED
@pytest.mark.parametrize("pattern", ["scattered", "block", "first", "last", "unsorted_dups", "all_but_one"])
def test_remove(S, oracle, base, tmp_path, ranked, pattern):
    rng = np.random.default_rng(3)
    chunks = {"scattered": rng.choice(N, size=N // 10, replace=False), "block": np.arange(1200, 1700), "first": [0], "last": [N - 1],
              "unsorted_dups": [2500, 3, 3, 777, 2500, 4, 2999, 3], "all_but_one": np.delete(np.arange(N), 1234)}[pattern]
    m = _model(S, base, ranked)
    m.remove(chunks)
    assert_rule(m, oracle, tmp_path)
    m.close()


@RANKED
def test_remove_everything_then_refill(S, oracle, base, tmp_path, ranked):
    m = _model(S, base, ranked)
    m.remove(np.arange(N))
    assert len(m.ix) == 0 and m.ix.unique_tokens() == 0 and m.ix.postings() == 0
    assert m.ix.search_raw([1, 2], [1.0, 1.0], 10)[0].size == 0
    assert m.ix.remove_chunks([]) == 0                                # m == 0 changes nothing
    assert_rule(m, oracle, tmp_path)
    csr, ids = _extra(base, 0, 700, ranked)
    m.extend(csr, ids)
    assert_rule(m, oracle, tmp_path)
    m.close()


@RANKED
def test_a_dying_token(S, oracle, base, ranked):
    off, tok, w = (np.array(a) for a in base["doc"])
    tok[tok == 150] = 149
    for c in (17, 1500, 2999):                                       # three chunks alone hold token 150
        tok[int(off[c])] = 150
    m = Model(S, (off, tok, w), base["ids"] if ranked else None)
    before = m.ix.unique_tokens()
    assert m.ix.search_raw([150], [1.0], 10)[0].size == 3
    m.remove([2999, 17, 1500])
    assert m.ix.unique_tokens() == before - 1
    ch, sc_, rc = m.ix.search_raw([150], [1.0], 10)
    assert rc == 0 and ch.size == 0
    assert_rule(m, oracle)
    m.close()


# ---- extend -----------------------------------------------------------------------------------------------------------
@RANKED
@pytest.mark.parametrize("count", [1, 300, 3000])
def test_extend(S, oracle, base, tmp_path, ranked, count):
    m = _model(S, base, ranked)
    csr, ids = _extra(base, 0, count, ranked)
    m.extend(csr, ids)
    assert_rule(m, oracle, tmp_path)
    m.close()


@pytest.mark.parametrize("where", ["before_all", "after_all", "between"])
def test_extend_ids_that_sort_anywhere(S, oracle, base, where):
    m = _model(S, base, True)
    csr, _ = _extra(base, 0, 40, True)
    ids = {"before_all": ["a%04d" % i for i in range(40)], "after_all": ["z%04d" % i for i in range(40)],
           "between": [sorted(base["ids"])[37 * i + 5] + ("x" if i % 2 else "") for i in range(40)]}[where]   # every other one equal to an old id
    m.extend(csr, ids)
    assert_rule(m, oracle)
    m.close()


@RANKED
def test_extend_unseen_tokens_and_an_empty_document(S, oracle, base, ranked):
    m = _model(S, base, ranked)
    off = np.array([0, 2, 2, 5], dtype=np.uint64)                     # the middle document has no postings: it never scores
    tok = np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 7], dtype=np.uint32)
    w = np.array([1.5, 0.25, 2.0, -1.0, 0.5], dtype=np.float32)
    before = m.ix.unique_tokens()
    m.extend((off, tok, w), ["c99990", "a-first", "m-middle"] if ranked else None)
    assert m.ix.unique_tokens() == before + 2
    ch, _s, rc = m.ix.search_raw([0, 0xFFFFFFFF], [1.0, 1.0], 10)
    assert rc == 0 and sorted(ch.tolist()) == [N, N + 2]
    assert_rule(m, oracle)
    m.close()


def test_extend_csr_without_new_rank(S, oracle, base):
    csr, ids = _extra(base, 100, 150, True)
    m = _model(S, base, True)
    m.ix.extend_csr(ids, *csr, new_rank=None)                         # the mirror ranks the ids itself
    m.csr, m.ids = csr_concat(m.csr, csr), m.ids + list(ids)
    assert_rule(m, oracle)
    m.close()
    m = _model(S, base, False)
    m.ix.extend_csr(None, *csr, new_rank=None)                        # NULL: nothing to rank on an unranked handle
    m.csr = csr_concat(m.csr, csr)
    assert_rule(m, oracle)
    m.close()
    # a handle created with id_rank, extended with NULL: the new chunks rank after every existing one, in the order given
    rng = np.random.default_rng(8)
    m = Model(S, base["doc"], None, id_rank=rng.permutation(N))
    m.extend(csr, None, None)
    assert_rule(m, oracle)
    m.extend(csr, None, rng.choice(N + 100, size=50, replace=False).astype(np.uint32))
    assert_rule(m, oracle)
    m.close()


# ---- the watch loop ---------------------------------------------------------------------------------------------------
@RANKED
def test_watch_loop_sequence(S, oracle, base, tmp_path, ranked):
    rng = np.random.default_rng(12)
    m = _model(S, base, ranked)
    for rnd in range(6):
        m.remove(rng.choice(m.n, size=40, replace=False))
        assert_rule(m, oracle, queries=1, seed=rnd)
        csr, ids = _extra(base, 40 * rnd, 40 * rnd + 40, ranked)
        m.extend(csr, ids)
        assert_rule(m, oracle, tmp_path if rnd == 5 else None, queries=1, seed=100 + rnd)
    m.close()


def test_hybrid_legs_agree_after_remove(S, hip, base):
    """`dense.remove(ids)` beside `sparse.remove(ids)`: the fused result is the one two fresh handles over the survivors give."""
    from cqs_amd import HipIndex, synth
    rows = synth.gaussian_unit(N, seed=91)
    ids = tuple(base["ids"])                                          # (the dense mirror keeps and edits the list it is given)
    dense, sparse = HipIndex.build_from_flat(list(ids), rows), S.HipSpladeIndex.build_from_csr(list(ids), *base["doc"])
    rng = np.random.default_rng(4)
    gone = np.sort(rng.choice(N, size=250, replace=False))
    gone_ids = [ids[i] for i in gone] + ["never-indexed"]
    assert dense.remove(gone_ids) == 250 and sparse.remove(gone_ids) == 250
    keep_ids = [cid for i, cid in enumerate(ids) if i not in set(gone.tolist())]
    assert dense.id_map == keep_ids and sparse.id_map == keep_ids
    dense2 = HipIndex.build_from_flat(keep_ids, np.delete(rows, gone, axis=0))
    sparse2 = S.HipSpladeIndex.build_from_csr(keep_ids, *csr_delete(base["doc"], gone))
    qt, qw = sc.query(rng, VOCAB, 30)
    sq = list(zip(qt.tolist(), qw.tolist()))
    q = rows[5] + 0.3 * synth.gaussian_unit(1, seed=101)[0]
    q = (q / np.linalg.norm(q)).astype(np.float32)
    for pred in (None, lambda cid: int(cid[-1]) % 3 != 0):            # both passes of the pipeline: unfiltered and filtered
        fused = []
        for d_ix, s_ix in ((dense, sparse), (dense2, sparse2)):
            d = d_ix.search(q, 500) if pred is None else d_ix.search_with_filter(q, 500, pred)
            s = s_ix.search_with_filter(sq, 500, pred)
            assert not set(r.id for r in s) & set(gone_ids)
            fused.append([(r.id, r.score) for r in S.fuse_hybrid(d, s, 0.7, 500)])
        assert fused[0] == fused[1] and len(fused[0]) > 0
    for x in (dense, sparse, dense2, sparse2):
        x.close()


# ---- sizes at which the geometry changes ------------------------------------------------------------------------------------
def _small(rng, n, nnz=(1, 5), vocab=60):
    return sc.corpus(rng, n, vocab, nnz[0], nnz[1], dup_frac=0.3)


@RANKED
@pytest.mark.parametrize("steps", [(31, 32, 33, 32, 31), (1024, 1025, 1024, 1023)])
def test_small_size_edges(S, oracle, ranked, steps):
    """Across a keep-bitset word boundary (32) and an n_pad granule (1024), by extend and by remove."""
    rng = np.random.default_rng(steps[0])
    pool = _small(rng, 1100)
    ids = ["k%04d" % i for i in rng.permutation(1100)] if ranked else None
    used = steps[0]
    m = Model(S, csr_take(pool, np.arange(used)), ids[:used] if ranked else None)
    assert_rule(m, oracle, queries=1)
    for nxt in steps[1:]:
        if nxt > m.n:
            add = nxt - m.n
            m.extend(csr_take(pool, np.arange(used, used + add)), ids[used:used + add] if ranked else None)
            used += add
        else:
            m.remove(rng.choice(m.n, size=m.n - nxt, replace=False))
        assert m.n == nxt
        assert_rule(m, oracle, queries=1)
    m.close()


@RANKED
def test_chunks_without_postings_and_a_single_posting(S, oracle, ranked):
    empty = (np.zeros(6, dtype=np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))     # 5 chunks, no postings at all
    m = Model(S, empty, ["e%d" % i for i in (3, 1, 4, 0, 2)] if ranked else None)
    m.remove([1, 3])
    assert_rule(m, oracle)
    one = (np.array([0, 0, 1], dtype=np.uint64), np.array([9], np.uint32), np.array([2.5], np.float32))
    m.extend(one, ["e9", "a0"] if ranked else None)
    assert m.ix.postings() == 1 and m.ix.search_raw([9], [1.0], 5)[0].tolist() == [4]
    assert_rule(m, oracle)
    m.remove([4])
    assert m.ix.postings() == 0 and m.ix.unique_tokens() == 0
    assert_rule(m, oracle)
    m.close()


def _big(rng, n, vocab=3000):
    """2-4 postings per chunk with a skewed vocabulary, vectorised."""
    lens = rng.integers(2, 5, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    P = int(off[-1])
    tok = (vocab * rng.random(P) ** 3).astype(np.uint32)
    w = (rng.random(P, dtype=np.float32) * 2.5 + 0.01).astype(np.float32)
    return off, tok, w


@pytest.mark.parametrize("ranked", [True, False], ids=["ranked", "unranked"])
@pytest.mark.parametrize("hi,lo", [(263000, 261500), (526000, 523000)], ids=["group16", "rw64_128"])
def test_geometry_edges(S, ranked, hi, lo):
    """The smallest sizes at which the constructors change their mind (256 CUs): 16- against 64-chunk groups at n_pad =
    262 144, 64- against 128-chunk wave ranges at n_pad = 524 288 - crossed by remove, and back by extend."""
    rng = np.random.default_rng(hi)
    m = Model(S, _big(rng, hi), None, id_rank=rng.permutation(hi) if ranked else None)
    gone = rng.choice(hi, size=hi - lo, replace=False)
    back = csr_take(m.csr, np.sort(gone))
    m.remove(gone)
    _rule_without_save(m)
    m.extend(back, None, rng.choice(hi, size=hi - lo, replace=False).astype(np.uint32) if ranked else None)
    assert m.n == hi
    _rule_without_save(m)
    m.close()


def _rule_without_save(m, n_queries=8):
    ix, fresh = m.ix, m.fresh()
    try:
        assert (len(ix), ix.unique_tokens(), ix.postings()) == (len(fresh), fresh.unique_tokens(), fresh.postings())
        rng = np.random.default_rng(5)
        vocab = np.unique(m.csr[1])
        qs = []
        for _ in range(n_queries):
            t = rng.choice(vocab, size=30, replace=False).astype(np.uint32)
            qs.append((t, (rng.random(30, dtype=np.float32) * 2 + 0.05).astype(np.float32)))
        keep = rng.random(m.n) < 0.3
        for i, (qt, qw) in enumerate(qs):
            k = (1, 500, 1024)[i % 3]
            assert _bytes(ix.search_raw(qt, qw, k)) == _bytes(fresh.search_raw(qt, qw, k))
            assert _bytes(ix.search_raw(qt, qw, k, keep)) == _bytes(fresh.search_raw(qt, qw, k, keep))
        assert _bytes(ix.search_batch_raw(qs, 500)) == _bytes(fresh.search_batch_raw(qs, 500))
        every = (vocab.astype(np.uint32), np.ones(vocab.size, dtype=np.float32))
        assert _bytes(ix.search_raw(*every, 1024)) == _bytes(fresh.search_raw(*every, 1024))
    finally:
        fresh.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
@RANKED
def test_refusals_leave_the_index_untouched(S, base, ranked):
    import ctypes as C
    m = _model(S, base, ranked)
    ix, lib = m.ix, m.ix._lib
    qt, qw = sc.query(np.random.default_rng(2), VOCAB, 20)
    want = _bytes(ix.search_raw(qt, qw, 500))
    ids_before = None if ix.id_map is None else list(ix.id_map)

    def untouched(fragment):
        assert fragment in ix.last_error, ix.last_error
        assert len(ix) == N and _bytes(ix.search_raw(qt, qw, 500)) == want and ix.id_map == ids_before

    def raw_refused(fragment):                                       # after a refusal through the bare C ABI
        buf = C.create_string_buffer(512)
        lib.cqs_hip_sparse_index_last_error(ix._h, buf, 512)
        ix.last_error = buf.value.decode()
        untouched(fragment)

    with pytest.raises(S.HipError):
        ix.remove_chunks([5, N])
    untouched("chunk index not in this index")
    removed = C.c_uint64(9)
    assert lib.cqs_hip_sparse_index_remove(ix._h, None, 3, C.byref(removed)) == -1 and removed.value == 0
    raw_refused("null chunks")
    off1 = np.array([0, 1], dtype=np.uint64)
    t1, w1 = np.array([5], dtype=np.uint32), np.array([1.0], dtype=np.float32)
    id1 = ["new-1"] if ranked else None
    for bad_off, n_new, frag in ((np.array([0, 2, 1], dtype=np.uint64), 2, "doc_off not ascending"),
                                 (np.array([1, 2], dtype=np.uint64), 1, "doc_off does not start at 0")):
        tt, ww = np.array([5, 6], dtype=np.uint32), np.array([1.0, 2.0], dtype=np.float32)
        assert lib.cqs_hip_sparse_index_extend(ix._h, bad_off.ctypes.data, tt.ctypes.data, ww.ctypes.data, n_new, None) == -1
        raw_refused(frag)
    assert lib.cqs_hip_sparse_index_extend(ix._h, off1.ctypes.data, None, w1.ctypes.data, 1, None) == -1
    raw_refused("null tokens / weights")
    assert lib.cqs_hip_sparse_index_extend(ix._h, off1.ctypes.data, t1.ctypes.data, None, 1, None) == -1
    raw_refused("null tokens / weights")
    assert lib.cqs_hip_sparse_index_extend(ix._h, off1.ctypes.data, t1.ctypes.data, w1.ctypes.data, 0xFFFFFFFF - N, None) == -1
    raw_refused("too many chunks")                                   # len + n_new past the chunk limit create enforces
    bad_w = w1.copy()
    bad_w.view(np.uint32)[0] = 0xFFFFFFFF
    with pytest.raises(S.HipError):
        ix.extend_csr(id1, off1, t1, bad_w)
    untouched("reserved NaN payload")
    off2 = np.array([0, 1, 2], dtype=np.uint64)
    t2, w2 = np.array([5, 6], dtype=np.uint32), np.array([1.0, 2.0], dtype=np.float32)
    id2 = ["new-1", "new-2"] if ranked else None
    if ranked:
        with pytest.raises(S.HipError):
            ix.extend_csr(id2, off2, t2, w2, new_rank=[7, 7])
        untouched("new_rank given twice")
        with pytest.raises(S.HipError):
            ix.extend_csr(id2, off2, t2, w2, new_rank=[7, N + 2])
        untouched("new_rank out of range")
        with pytest.raises(ValueError):
            ix.extend_csr(None, off2, t2, w2)                        # the ids' flavour must match the handle's
    else:
        with pytest.raises(S.HipError):
            ix.extend_csr(None, off2, t2, w2, new_rank=[7, 8])
        untouched("new_rank on an index created without id_rank")
        with pytest.raises(ValueError):
            ix.extend_csr(["a", "b"], off2, t2, w2)
    assert len(ix) == N and _bytes(ix.search_raw(qt, qw, 500)) == want and ix.id_map == ids_before
    assert lib.cqs_hip_sparse_index_poisoned(ix._h) == 0
    m.close()


# ---- searches during updates ------------------------------------------------------------------------------------------------
def test_searches_during_updates_see_the_old_index_or_the_new_one(S, base):
    """4 threads search one query while the main thread removes the last 50 chunks and extends them back, 10 times: every
    answer is, byte for byte, the answer with those chunks or the answer without them."""
    m = _model(S, base, True)
    ix = m.ix
    tail = np.arange(N - 50, N)
    tail_csr, tail_ids = csr_take(m.csr, tail), m.ids[N - 50:]
    qt, qw = sc.query(np.random.default_rng(6), VOCAB, 30)
    with_them = _bytes(ix.search_raw(qt, qw, 500))
    ix.remove_chunks(tail)
    without = _bytes(ix.search_raw(qt, qw, 500))
    del ix.id_map[N - 50:]
    ix.extend_csr(tail_ids, *tail_csr)
    assert _bytes(ix.search_raw(qt, qw, 500)) == with_them and with_them != without
    failed = []

    def client():
        for _ in range(200):
            r = _bytes(ix.search_raw(qt, qw, 500))
            if r[-1] != 0 or r not in (with_them, without):
                failed.append(r[-1])
                return

    threads = [threading.Thread(target=client) for _ in range(4)]
    for t in threads:
        t.start()
    for _ in range(10):
        assert ix.remove(tail_ids) == 50
        ix.extend_csr(tail_ids, *tail_csr)
    for t in threads:
        t.join()
    assert not failed, failed
    assert _bytes(ix.search_raw(qt, qw, 500)) == with_them
    m.close()
