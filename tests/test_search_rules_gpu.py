"""The host rules of the search path (cqs_amd/csrc/search_host.h: argument plan, kept-row count and k_eff, query staging,
neighbours' clamp and self-exclusion) behave the same behind a single-device handle and behind a row-sharded one.  One small
corpus with a ragged last bitset word and two score-row granules (300 rows: shards of 256 and 44), opened both ways over
the same device.  Per case both handles give the same status, message, counts and rows; scores go through the parity rule
(a shard's scan and the whole corpus's plan their tasks differently, so score bits are not compared)."""
import ctypes as C

import numpy as np
import pytest

from cqs_amd import HipIndex, _lib, synth
from parity import assert_topk_parity

pytestmark = pytest.mark.gpu

N, DIM = 300, 64
SENTINEL = 0xDEADBEEF


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def pair(hip):
    rows = synth.gaussian_unit(N, DIM, seed=7300)
    qs = synth.gaussian_unit(3, DIM, seed=7301)
    single = HipIndex.build_from_flat(None, rows)
    sharded = HipIndex.build_sharded(None, rows, [0, 0])
    assert [s[2] for s in sharded.shards()] == [256, 44]
    yield hip, qs, single, sharded
    single.close()
    sharded.close()


def _search(lib, idx, q, b, qd, k, keep=None, mode=_lib.MODE_RAW):
    q = np.ascontiguousarray(q, dtype=np.float32)
    width = max(k, 1)
    rows = np.zeros((max(b, 1), width), dtype=np.uint64)
    scores = np.zeros((max(b, 1), width), dtype=np.float32)
    counts = np.full((max(b, 1),), SENTINEL, dtype=np.uint32)
    kb = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint32)
    rc = lib.cqs_hip_index_search(idx._h, _ptr(q), b, qd, k, _ptr(kb), mode, 0.0, _ptr(rows), _ptr(scores), _ptr(counts))
    return rc, counts, rows, scores, idx.last_error()


def _neighbors(lib, idx, target, limit):
    rows = np.zeros((_lib.NEIGHBORS_MAX,), dtype=np.uint64)
    scores = np.zeros((_lib.NEIGHBORS_MAX,), dtype=np.float32)
    c = C.c_uint32(SENTINEL)
    rc = lib.cqs_hip_index_neighbors(idx._h, target, limit, _ptr(rows), _ptr(scores), C.byref(c))
    return rc, np.array([c.value], dtype=np.uint32), rows[None, :], scores[None, :], idx.last_error()


def _same(a, b, rc, counts=None, message=None):
    """The two handles' answers: the expected status on both, equal counts and rows, scores within the parity rule."""
    assert a[0] == b[0] == rc, (a[0], b[0])
    assert np.array_equal(a[1], b[1]), (a[1], b[1])
    if counts is not None:
        assert list(a[1]) == list(counts), a[1]
    if message is not None:
        assert a[4] == b[4] == message, (a[4], b[4])
    if rc != _lib.OK:
        return
    for i, c in enumerate(a[1]):
        if c == SENTINEL:
            continue
        assert np.array_equal(a[2][i, :c], b[2][i, :c]), (i, a[2][i, :c], b[2][i, :c])
        assert_topk_parity(b[2][i, :c], b[3][i, :c], a[2][i, :c], a[3][i, :c], int(c))


def _bits(keep, garbage=False):
    words = np.packbits(np.asarray(keep, dtype=bool), bitorder="little")
    words = np.concatenate([words, np.zeros((-len(words)) % 4, dtype=np.uint8)]).view(np.uint32).copy()
    if garbage and len(keep) % 32:
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(len(keep) % 32)   # bits past the last row are not rows
    return words


def test_argument_plan(pair):
    lib, qs, single, sharded = pair
    both = lambda *a, **kw: (_search(lib, single, *a, **kw), _search(lib, sharded, *a, **kw))
    _same(*both(qs, 0, DIM, 20), _lib.OK, [SENTINEL])                                    # b = 0: nothing is touched
    for b in (1, 3):
        _same(*both(qs, b, DIM, 0), _lib.OK, [0] * b)                                    # k = 0
        _same(*both(qs[:, :48], b, 48, 20), _lib.OK, [0] * b, "search: query dimension mismatch (empty result)")
        _same(*both(qs, b, DIM, 1025), _lib.ERR_INVALID, [0] * b, "search: k > max_k")
        _same(*both(qs, b, DIM, 20, mode=_lib.MODE_PIPELINE + 1), _lib.ERR_INVALID, [0] * b, "search: bad mode")
    _same(*both(qs[:, :48], 3, 48, 1025), _lib.OK, [0, 0, 0],                            # the mismatch answers before k is looked at
          "search: query dimension mismatch (empty result)")
    assert not single.is_poisoned() and not sharded.is_poisoned()


def test_nan_query_in_the_middle_of_a_block(pair):
    lib, qs, single, sharded = pair
    bad = qs.copy()
    bad[1, DIM - 1] = np.nan
    _same(_search(lib, single, bad, 3, DIM, 20), _search(lib, sharded, bad, 3, DIM, 20), _lib.OK, [20, 0, 20])
    _same(_search(lib, single, bad[1], 1, DIM, 20), _search(lib, sharded, bad[1], 1, DIM, 20), _lib.OK, [0])


@pytest.mark.parametrize("b", [1, 3])
def test_bitset_rules(pair, b):
    lib, qs, single, sharded = pair
    none = _bits(np.zeros(N, bool), garbage=True)
    _same(_search(lib, single, qs, b, DIM, 20, keep=none), _search(lib, sharded, qs, b, DIM, 20, keep=none), _lib.OK, [0] * b)
    every = _bits(np.ones(N, bool), garbage=True)
    for idx in (single, sharded):                                  # all kept = the unfiltered call, bit for bit
        f, u = _search(lib, idx, qs, b, DIM, 20, keep=every), _search(lib, idx, qs, b, DIM, 20)
        assert f[0] == u[0] == _lib.OK and list(f[1]) == [20] * b
        assert np.array_equal(f[2], u[2]) and np.array_equal(f[3].view(np.uint32), u[3].view(np.uint32))
    _same(_search(lib, single, qs, b, DIM, 20, keep=every), _search(lib, sharded, qs, b, DIM, 20, keep=every), _lib.OK, [20] * b)
    few = np.zeros(N, bool)
    few[[5, 255, 299]] = True                                      # both shards, the last bit of the ragged word
    a = _search(lib, single, qs, b, DIM, 20, keep=_bits(few, garbage=True))
    _same(a, _search(lib, sharded, qs, b, DIM, 20, keep=_bits(few, garbage=True)), _lib.OK, [3] * b)
    assert all(sorted(int(r) for r in a[2][i, :3]) == [5, 255, 299] for i in range(b))


def test_neighbors_rules(pair):
    lib, qs, single, sharded = pair
    for target in (0, 256, N - 1):
        a = _neighbors(lib, single, target, 0)                     # limit 0 is 1
        _same(a, _neighbors(lib, sharded, target, 0), _lib.OK, [1])
        assert int(a[2][0, 0]) != target
        a = _neighbors(lib, single, target, 1000)                  # clamped to NEIGHBORS_MAX
        _same(a, _neighbors(lib, sharded, target, 1000), _lib.OK, [_lib.NEIGHBORS_MAX])
        assert target not in set(int(r) for r in a[2][0])
    _same(_neighbors(lib, single, N, 5), _neighbors(lib, sharded, N, 5), _lib.ERR_INVALID, [0],
          "neighbors: target row not in this index")
