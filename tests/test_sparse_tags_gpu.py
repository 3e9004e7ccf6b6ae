"""Chunk tags on the sparse index (include/cqs_hip.h "Chunk tags"): `cqs_hip_sparse_index_search_tagged`
returns the bytes of `cqs_hip_sparse_index_search` with the host bitset of the same predicate - chunk order and score bits -
on an integer-addressed index and on one with string ids (where the bitset is looked up through the id order), and the
tags follow `remove` / `extend`.  The small corpora of tests/sparse_cases.py.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import sparse_cases as sc
import tags_cases as tc
from cqs_amd import HipError, _lib, tag_filter

pytestmark = pytest.mark.gpu

N, VOCAB = 3000, 200


@pytest.fixture(scope="module")
def S(hip):
    from cqs_amd import splade_index
    return splade_index


@pytest.fixture(scope="module")
def base():
    rng = np.random.default_rng(20250101)
    doc = sc.corpus(rng, N, VOCAB, 4, 12, dup_frac=0.3, special=True)
    extra = sc.corpus(rng, 500, VOCAB, 4, 12, dup_frac=0.3, special=True)
    ids = ["c%05d" % i for i in rng.permutation(N + 500)]          # string ids in shuffled order: rank != chunk index
    queries = [sc.query(rng, VOCAB, t, dups=d, absent=a) for t, d, a in ((3, 0, 0), (24, 2, 1), (64, 0, 3), (150, 5, 0))]
    tags = tc.unique_end_tags(N + 500, 8800)
    for a in doc + extra + (tags,):
        a.setflags(write=False)
    return dict(doc=doc, extra=extra, ids=ids, queries=queries, tags=tags)


def build(S, base, ranked, n=N):
    off, tok, w = base["doc"]
    e = int(off[n])
    return S.HipSpladeIndex.build_from_csr(base["ids"][:n] if ranked else None, off[:n + 1], tok[:e], w[:e])


def assert_tagged_is_host_bitset(ix, tags, queries, seed, what):
    n = len(ix)
    assert ix.tagged_chunks() == n == len(tags)
    filters = tc.filters_for(tags, seed)
    nonempty = 0
    for name, allow in filters.items():
        mask = tc.keep_mask(tags, allow)
        for qt, qw in queries:
            for k in (1, 20, 500):
                tch, tsc, trc = ix.search_tagged_raw(qt, qw, k, allow)
                hch, hsc, hrc = ix.search_raw(qt, qw, k, keep=mask)
                assert trc == hrc == _lib.OK, (what, name, ix.last_error)
                assert np.array_equal(tch, hch), (what, name, k)
                assert np.array_equal(tsc.view(np.uint32), hsc.view(np.uint32)), (what, name, k)
                assert all(mask[int(c)] for c in tch)
                nonempty += len(tch) > 0
                if name == "all_pass":                                  # the keep_bitset == NULL call
                    uch, usc, urc = ix.search_raw(qt, qw, k)
                    assert urc == _lib.OK and np.array_equal(tch, uch) and np.array_equal(tsc.view(np.uint32), usc.view(np.uint32))
                if name == "empty_field_2":
                    assert len(tch) == 0
    assert nonempty > 20, what


@pytest.mark.parametrize("ranked", (False, True))
def test_tagged_search_is_the_host_bitset_search(S, base, ranked):
    ix = build(S, base, ranked)
    assert ix.tagged_chunks() == 0
    ix.set_tags(base["tags"][:1000])
    ix.set_tags(base["tags"][900:N], first=900)                         # overwrite inside the prefix and extend it
    assert_tagged_is_host_bitset(ix, base["tags"][:N], base["queries"], 8801, ("plain", ranked))
    ix.close()


@pytest.mark.parametrize("n", (1, 33, 64, 65))
def test_small_indexes(S, base, n):
    ix = build(S, base, True, n)
    tags = tc.unique_end_tags(n, 8810 + n)
    ix.set_tags(tags)
    off, tok, w = base["doc"]
    every_token = np.unique(tok[:int(off[n])]).astype(np.uint32)          # a query that reaches every chunk
    present = (every_token, np.ones(len(every_token), dtype=np.float32))
    filters = tc.filters_for(tags, 8820 + n)
    for name, allow in filters.items():
        mask = tc.keep_mask(tags, allow)
        tch, tsc, trc = ix.search_tagged_raw(*present, 100, allow)
        hch, hsc, hrc = ix.search_raw(*present, 100, keep=mask)
        assert trc == hrc == _lib.OK and np.array_equal(tch, hch) and np.array_equal(tsc.view(np.uint32), hsc.view(np.uint32)), (n, name)
        assert len(tch) == int(mask.sum()), (n, name)                   # every chunk holds one of the query's tokens
    ix.close()


@pytest.mark.parametrize("ranked", (False, True))
def test_tags_follow_remove_and_extend(S, base, ranked):
    ix = build(S, base, ranked)
    tags = np.array(base["tags"])
    ix.set_tags(tags[:N])
    rng = np.random.default_rng(8830)
    gone = np.sort(rng.choice(N, size=700, replace=False))
    assert ix.remove_chunks(np.concatenate([gone, gone[:5]])) == 700    # (duplicates count once)
    kept_tags = np.delete(tags[:N], gone)
    kept_ids = [cid for i, cid in enumerate(base["ids"][:N]) if i not in set(gone.tolist())]
    if ranked:
        ix.id_map[:] = kept_ids                                          # (remove_chunks leaves the id bookkeeping to its caller)
    assert_tagged_is_host_bitset(ix, kept_tags, base["queries"][:3], 8831, ("removed", ranked))
    # extend: the new chunks have no tag until set_tags covers them
    xoff, xtok, xw = base["extra"]
    new_ids = None if not ranked else base["ids"][N:N + 500]
    ix.extend_csr(new_ids, xoff, xtok, xw)
    assert len(ix) == N - 700 + 500 and ix.tagged_chunks() == N - 700
    half = tc.filters_for(kept_tags, 8832)["half_full"]
    qt, qw = base["queries"][1]
    ch, _sc, rc = ix.search_tagged_raw(qt, qw, 20, half)
    assert rc == _lib.ERR_INVALID and len(ch) == 0 and "tags cover 2300 of 2800 chunks" in ix.last_error
    assert ix.search_raw(qt, qw, 20)[2] == _lib.OK                       # still searchable
    ix.set_tags(tags[N:N + 500], first=N - 700)
    all_tags = np.concatenate([kept_tags, tags[N:N + 500]])
    assert_tagged_is_host_bitset(ix, all_tags, base["queries"][:3], 8833, ("extended", ranked))
    # only part of the index tagged: the prefix drops by the removed chunks below it
    ix.close()
    p = build(S, base, ranked)
    p.set_tags(tags[:1200])
    assert p.remove_chunks(gone) == 700
    if ranked:
        p.id_map[:] = kept_ids
    below = int((gone < 1200).sum())
    assert p.tagged_chunks() == 1200 - below
    p.set_tags(kept_tags[1200 - below:], first=1200 - below)
    assert_tagged_is_host_bitset(p, kept_tags, base["queries"][:2], 8834, ("partial", ranked))
    # everything goes, the index is refilled and tagged again
    assert p.remove_chunks(np.arange(len(p))) == N - 700 and p.tagged_chunks() == 0
    if ranked:
        p.id_map[:] = []
    p.extend_csr(new_ids, xoff, xtok, xw)
    assert p.tagged_chunks() == 0
    p.set_tags(tags[:500])
    assert_tagged_is_host_bitset(p, tags[:500], base["queries"][:2], 8835, ("refilled", ranked))
    p.close()


def test_save_and_load_do_not_persist_tags(S, base, tmp_path):
    ix = build(S, base, False)
    ix.set_tags(base["tags"][:N])
    path = str(tmp_path / "sparse.bin")
    ix.save(path, 3)
    loaded = S.HipSpladeIndex.load(path, 3)
    assert loaded is not None and len(loaded) == N and loaded.tagged_chunks() == 0 and ix.tagged_chunks() == N
    ix.close(); loaded.close()


def test_invalid_calls_leave_the_handle_untouched(hip, S, base):
    ix = build(S, base, True)
    tags = np.ascontiguousarray(base["tags"][:N])
    ix.set_tags(tags[:2000])
    h = ix._h

    def set_tags(first, ptr, m):
        rc = hip.cqs_hip_sparse_index_set_tags(h, first, ptr, m)
        buf = C.create_string_buffer(512)
        hip.cqs_hip_sparse_index_last_error(h, buf, 512)
        return rc, buf.value.decode()
    p = tags.ctypes.data_as(C.c_void_p)
    assert set_tags(2001, p, 10) == (_lib.ERR_INVALID, "sparse set_tags: gap: first row past the tagged rows")
    assert set_tags(2000, p, 1001) == (_lib.ERR_INVALID, "sparse set_tags: range past the end of the index")
    assert set_tags(0, None, 10) == (_lib.ERR_INVALID, "sparse set_tags: null tags")
    assert set_tags(99999, None, 0)[0] == _lib.OK
    with pytest.raises(HipError):
        ix.set_tags(tags[:10], first=2500)
    assert ix.tagged_chunks() == 2000 and len(ix) == N
    ix.set_tags(tags[2000:], first=2000)
    qt, qw = base["queries"][1]
    half = tc.filters_for(tags, 8840)["half_full"]
    before = ix.search_tagged_raw(qt, qw, 20, half)
    assert before[2] == _lib.OK and len(before[0]) > 0
    ch, _sc, rc = ix.search_tagged_raw(qt, qw, 20, None)                 # null allow
    assert rc == _lib.ERR_INVALID and len(ch) == 0 and ix.last_error == "sparse search_tagged: null allow"
    ch, _sc, rc = ix.search_tagged_raw(qt, qw, 2000, half)               # the rules of the search itself carry over
    assert rc == _lib.ERR_INVALID and "k > CQS_HIP_MAX_K" in ix.last_error
    assert hip.cqs_hip_sparse_index_poisoned(h) == 0
    after = ix.search_tagged_raw(qt, qw, 20, half)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1].view(np.uint32), before[1].view(np.uint32))
    assert len(ix.search_tagged([(int(t), float(x)) for t, x in zip(qt, qw)], 20, tag_filter())) == 20
    ix.close()
