"""`cqs_hip_index_remove` / `HipIndex.remove` (include/cqs_hip.h): rows leave the resident corpus in place.

The yardstick everywhere is a fresh `HipIndex.build_from_flat` of `np.delete(flat, removed, axis=0)`: after a removal the
index must be indistinguishable from it - the same bytes from every search (rows, score BITS, counts), the same shadow
bytes, the same saved blob.  No tolerance anywhere except for the blocks of 32 queries on the matrix cores, which go through
tests/parity.py as every matrix-core comparison here does.  Run on an MI355X with `pytest -m gpu`."""
import ctypes as C
import json

import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipError, HipIndex, _lib, synth
from parity import assert_topk_parity

pytestmark = pytest.mark.gpu
ENV_BF16, ENV_I8 = "CQS_HIP_SCAN_BF16", "CQS_HIP_SCAN_I8"
BF16, I8 = 1, 2
N_OF_DIM = {4: 5000, 768: 4097, 4096: 3001}
SMALL_BUDGET = 1000               # rows per pass: the runs behind row 0 or the block take 3-5 passes and straddle their boundaries;
                                  # 0 = the bounce buffer's own budget, which every corpus here fits in one pass


def pattern(name, n):
    if name == "one":
        return np.array([n // 3])
    if name == "row0":
        return np.array([0])
    if name == "last":
        return np.array([n - 1])
    if name == "block":
        return np.arange(200, 600)                      # crosses rows 224, 256 and 512
    if name == "every_second":
        return np.arange(0, n, 2)
    if name == "random30":
        return np.random.default_rng(n).choice(n, size=int(0.3 * n), replace=False)
    raise KeyError(name)


PATTERNS = ("one", "row0", "last", "block", "every_second", "random30")


def set_budget(hip, idx, rows):
    hip.cqs_hip_debug_index_remove_budget(idx._h, rows)


def assert_same(got, want, ctx=""):
    (ra, sa, ca), (rb, sb, cb) = got, want
    assert np.array_equal(ca, cb), (ctx, ca, cb)
    for i in range(len(ca)):
        c = int(ca[i])
        assert np.array_equal(ra[i, :c], rb[i, :c]), (ctx, i)
        assert np.array_equal(sa[i, :c].view(np.uint32), sb[i, :c].view(np.uint32)), (ctx, i)


def assert_searches_match(a, f, q, ctx=""):
    """Every search of the issue's list on the index after removal `a` and the fresh one `f`."""
    assert len(a) == len(f), ctx
    n = len(f)
    for b in (1, 8):
        for k in (1, 20, 500):
            kk = min(k, n)
            assert_same(a.search_batch(q[:b], kk), f.search_batch(q[:b], kk), (ctx, b, k))
    # 32 queries: the matrix cores where dim % 32 == 0.  Bit-identical as well (the same kernel over the same rows, row
    # count and launch shape), which is what is asserted; the parity helper first, at its own tolerance.
    k = min(20, n)
    ra, sa, ca = a.search_batch(q, k)
    rf, sf, cf = f.search_batch(q, min(k + 64, n))
    for i in range(q.shape[0]):
        assert_topk_parity(ra[i, :ca[i]], sa[i, :ca[i]], rf[i, :cf[i]], sf[i, :cf[i]], k)
    assert_same((ra, sa, ca), f.search_batch(q, k), (ctx, 32))


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dim", sorted(N_OF_DIM))
def test_remove_matches_rebuild(hip, dim, name):
    n = N_OF_DIM[dim]
    flat = synth.gaussian_unit(n, dim=dim, seed=7000 + dim)
    q = synth.gaussian_unit(32, dim=dim, seed=7100 + dim)
    gone = pattern(name, n)
    kept = np.delete(flat, gone, axis=0)
    for metric, base, budget in ((DistanceMetric.Cosine, 0, 0), (DistanceMetric.DotProduct, 1000, SMALL_BUDGET),
                                 (DistanceMetric.Cosine, 1000, SMALL_BUDGET), (DistanceMetric.DotProduct, 0, 0)):
        a = HipIndex.build_from_flat(None, flat, metric, row_base=base)
        f = HipIndex.build_from_flat(None, kept, metric, row_base=base)
        a.search_batch(q[:8], 20)                                 # scratch sized for the old n: the removal must not rely on it
        set_budget(hip, a, budget)
        ids = (gone + base)[::-1]                                 # unsorted ...
        ids = np.concatenate([ids, ids[:3]])                      # ... with duplicates
        assert a.remove_rows(ids) == len(gone)
        assert_searches_match(a, f, q, (dim, name, metric, base, budget))
        a.close(); f.close()


@pytest.mark.parametrize("dim", (4, 768))
def test_remove_every_row_then_refill(hip, dim):
    n = 3000
    flat = synth.gaussian_unit(n, dim=dim, seed=7200 + dim)
    q = synth.gaussian_unit(32, dim=dim, seed=7300 + dim)
    a = HipIndex.build_from_flat(None, flat, row_base=64)
    assert a.remove_rows(np.arange(64, 64 + n)) == n
    assert len(a) == 0 and a.is_empty() and not a.is_poisoned()
    rows, scores, counts = a.search_batch(q[:8], 20)
    assert not counts.any()
    assert a.search(q[0], 20) == []
    more = synth.gaussian_unit(1500, dim=dim, seed=7400 + dim)
    a.extend(None, more)
    f = HipIndex.build_from_flat(None, more, row_base=64)
    assert_searches_match(a, f, q, (dim, "refilled"))
    a.close(); f.close()


def id_pair(flat, gone, base=1000, metric=DistanceMetric.Cosine):
    """(index over `flat` with ids c0.., fresh index over the surviving rows with the surviving ids, those ids)."""
    ids = [f"c{i}" for i in range(flat.shape[0])]
    gone_set = set(int(g) for g in gone)
    kept_ids = [cid for i, cid in enumerate(ids) if i not in gone_set]
    a = HipIndex.build_from_flat(list(ids), flat, metric, row_base=base)
    f = HipIndex.build_from_flat(list(kept_ids), np.delete(flat, gone, axis=0), metric, row_base=base)
    return a, f, kept_ids


def test_filtered_searches_after_removal(hip):
    n, dim = 4097, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=7500)
    q = synth.gaussian_unit(8, dim=dim, seed=7501)
    gone = pattern("random30", n)
    a, f, kept_ids = id_pair(flat, gone)
    preds = [lambda cid, m=m: int(cid[1:]) % m == 0 for m in (2, 3, 5, 7, 11, 13, 17, 19)]
    a.search_many_with_filters(q, 20, preds)                      # the keep-bitset table is made for the old row count
    set_budget(hip, a, SMALL_BUDGET)
    assert a.remove([f"c{int(g)}" for g in gone]) == len(gone)
    assert a.id_map == kept_ids
    for i in range(3):
        assert a.search_with_filter(q[i], 20, preds[i]) == f.search_with_filter(q[i], 20, preds[i])
    got, want = a.search_many_with_filters(q, 20, preds), f.search_many_with_filters(q, 20, preds)
    assert got == want and all(len(r) == 20 for r in got)
    a.close(); f.close()


def test_remove_extend_remove(hip):
    n, dim = 4097, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=7600)
    more = synth.gaussian_unit(1500, dim=dim, seed=7601)
    q = synth.gaussian_unit(32, dim=dim, seed=7602)
    a = HipIndex.build_from_flat(None, flat)
    set_budget(hip, a, SMALL_BUDGET)
    gone1 = pattern("random30", n)
    assert a.remove_rows(gone1) == len(gone1)
    a.extend(None, more[:100])                                      # inside cap_rows: lands on the rows the removal left behind
    a.extend(None, more[100:])                                      # past cap_rows: reallocates
    final = np.concatenate([np.delete(flat, gone1, axis=0), more])
    gone2 = np.concatenate([pattern("block", len(final)), np.arange(len(final) - 650, len(final) - 640)])
    assert a.remove_rows(gone2) == len(gone2)
    final = np.delete(final, gone2, axis=0)
    f = HipIndex.build_from_flat(None, final)
    assert_searches_match(a, f, q, "remove-extend-remove")
    a.close(); f.close()


def test_neighbors_and_mmr_after_removal(hip):
    n, dim = 4097, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=7700)
    q = synth.gaussian_unit(2, dim=dim, seed=7701)
    gone = pattern("every_second", n)
    a, f, kept_ids = id_pair(flat, gone)
    set_budget(hip, a, SMALL_BUDGET)
    assert a.remove([f"c{int(g)}" for g in gone]) == len(gone)
    for cid in (kept_ids[0], kept_ids[777], kept_ids[-1]):
        assert a.find_neighbors(cid, 10) == f.find_neighbors(cid, 10)
    with pytest.raises(KeyError):
        a.find_neighbors("c0", 10)                                  # removed
    pool = f.search(q[0], 100)
    assert a.search(q[0], 100) == pool
    assert a.mmr_rerank(pool, 10, 0.5) == f.mmr_rerank(pool, 10, 0.5)
    rows = np.arange(1000, 1040, dtype=np.uint64)
    assert np.array_equal(a.pairwise_rows(rows).view(np.uint32), f.pairwise_rows(rows).view(np.uint32))
    a.close(); f.close()


@pytest.fixture
def shadow_hooks(hip):
    hip.cqs_hip_debug_shadow_rows.restype = C.c_int32
    hip.cqs_hip_debug_shadow_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return hip


def read_bf16(hooks, h):
    out = np.zeros((len(h), h.dim()), np.uint16)
    assert hooks.cqs_hip_debug_shadow_rows(h._h, BF16, 0, len(h), out.ctypes.data, None) == _lib.OK
    return out


def read_i8(hooks, h):
    codes, scales = np.zeros((len(h), h.dim()), np.int8), np.zeros(len(h), np.float32)
    assert hooks.cqs_hip_debug_shadow_rows(h._h, I8, 0, len(h), codes.ctypes.data, scales.ctypes.data) == _lib.OK
    return codes, scales


def setenv(monkeypatch, bf16, i8):
    for name, v in ((ENV_BF16, bf16), (ENV_I8, i8)):
        monkeypatch.setenv(name, v)


@pytest.mark.parametrize("with_i8", (False, True))
@pytest.mark.parametrize("name", ("block", "random30"))
def test_shadow_copies_are_compacted(shadow_hooks, monkeypatch, with_i8, name):
    hooks = shadow_hooks
    n, dim = 4097, 768                                              # dim % 16 == 0: both copies
    flat = synth.gaussian_unit(n, dim=dim, seed=7800)
    q = synth.gaussian_unit(8, dim=dim, seed=7801)
    gone = pattern(name, n)
    kept = np.delete(flat, gone, axis=0)
    setenv(monkeypatch, "0", "0")
    plain = HipIndex.build_from_flat(None, kept)                    # the fresh f32 index: the answers' yardstick
    if with_i8:
        setenv(monkeypatch, "1", "1")                               # both copies at create, as tests/test_i8_scan_gpu.py builds them
        a = HipIndex.build_from_flat(None, flat)
        fs = HipIndex.build_from_flat(None, kept)                   # the fresh shadow: the copies' yardstick
    else:
        a = HipIndex.build_from_flat(None, flat)
        fs = HipIndex.build_from_flat(None, kept)
        a.set_bf16_scan(True); fs.set_bf16_scan(True)               # (CQS_HIP_SCAN_I8=0: the bf16 copy alone)
    bytes_bf16, bytes_i8 = a.bf16_stats()[0], a.i8_stats()[0]
    assert bytes_bf16 == n * dim * 2 and bytes_i8 == (n * dim + n * 4 if with_i8 else 0), a.last_error()
    a.search_batch(q[:4], 20)
    cert0, i8_cert0 = a.bf16_stats()[1], a.i8_stats()[1]
    set_budget(hooks, a, SMALL_BUDGET)
    assert a.remove_rows(gone) == len(gone)
    for b in (1, 4, 8):
        for k in (1, 20, 500):
            assert_same(a.search_batch(q[:b], k), plain.search_batch(q[:b], k), (name, with_i8, b, k))
    by, cert, fb = a.bf16_stats()
    i8_by, i8_cert, i8_fb = a.i8_stats()
    print("shadow after remove:", name, with_i8, "bf16", (by, cert - cert0, fb), "i8", (i8_by, i8_cert - i8_cert0, i8_fb),
          "fresh", fs.bf16_stats(), fs.i8_stats())
    assert by == bytes_bf16 and i8_by == bytes_i8                   # nothing was reallocated
    assert cert > cert0                                             # the certified path still serves
    if with_i8:
        assert i8_cert > i8_cert0
    assert np.array_equal(read_bf16(hooks, a), read_bf16(hooks, fs))
    if with_i8:
        (ca, sa), (cf, sf) = read_i8(hooks, a), read_i8(hooks, fs)
        assert np.array_equal(ca, cf) and np.array_equal(sa.view(np.uint32), sf.view(np.uint32))
    a.close(); fs.close(); plain.close()


def test_save_after_remove_equals_fresh_save(hip, tmp_path):
    n, dim = 4097, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=7900)
    q = synth.gaussian_unit(32, dim=dim, seed=7901)
    gone = pattern("random30", n)
    a, f, kept_ids = id_pair(flat, gone, base=0)
    set_budget(hip, a, SMALL_BUDGET)
    a.remove([f"c{int(g)}" for g in gone])
    pa, pf = str(tmp_path / "a.hipflat"), str(tmp_path / "f.hipflat")
    a.save(pa); f.save(pf)
    assert open(pa, "rb").read() == open(pf, "rb").read()
    ma, mf = json.load(open(pa + ".meta")), json.load(open(pf + ".meta"))
    assert ma == mf and ma["checksum"] == mf["checksum"] and ma["chunk_count"] == len(kept_ids)
    l = HipIndex.load(pa, dim, len(kept_ids))
    assert l.id_map == kept_ids
    assert_searches_match(l, f, q, "loaded")
    a.close(); f.close(); l.close()


def test_invalid_calls_leave_the_index_untouched(hip):
    import torch
    n, dim = 3000, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=8000)
    q = synth.gaussian_unit(8, dim=dim, seed=8001)
    a = HipIndex.build_from_flat(None, flat, row_base=100)
    before = a.search_batch(q, 20)
    for bad in ([150, 99], [150, 100 + n], [2 ** 40]):
        with pytest.raises(HipError) as e:
            a.remove_rows(bad)
        assert e.value.code == _lib.ERR_INVALID and "remove: row id not in this index" in str(e.value)
    assert hip.cqs_hip_index_remove(a._h, None, 3, None) == _lib.ERR_INVALID and "remove: null rows" in a.last_error()
    assert hip.cqs_hip_index_remove(a._h, None, 0, None) == _lib.OK                       # m == 0: nothing, whatever the pointer
    assert a.remove_rows([]) == 0
    assert len(a) == n and not a.is_poisoned()
    assert_same(a.search_batch(q, 20), before, "after invalid calls")
    a.close()
    # a borrowed handle: the rows are the caller's
    d = torch.from_numpy(flat).cuda()
    b = HipIndex.build_from_device(None, d.data_ptr(), n, dim, borrow=True, keepalive=d)
    with pytest.raises(HipError) as e:
        b.remove_rows([5])
    assert e.value.code == _lib.ERR_INVALID and "borrows" in str(e.value) and len(b) == n
    b.close()
    # a row-sharded parent: stated as not built, and it still searches
    s = HipIndex.build_sharded(None, flat, [0, 0])
    want = s.search_batch(q, 20)
    with pytest.raises(HipError) as e:
        s.remove_rows([5])
    assert e.value.code == _lib.ERR_INVALID and "remove: not supported on a row-sharded handle" in str(e.value)
    assert len(s) == n and not s.is_poisoned()
    assert_same(s.search_batch(q, 20), want, "sharded after the refused call")
    s.close()


def test_python_bookkeeping(hip):
    n, dim = 3000, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=8100)
    gone = [5, 6, 7, 2000, n - 1]
    a, f, kept_ids = id_pair(flat, gone)
    assert a.find_neighbors("c5", 3)                               # (builds the id -> row cache the removal must drop)
    asked = ["c2000", "never-indexed", "c5", "c6", f"c{n - 1}", "c7", "c5", "c999999"]
    assert a.remove(asked) == len(gone)
    assert a.id_map == kept_ids and len(a) == n - len(gone)
    assert a.remove(["never-indexed", "c5"]) == 0 and a.id_map == kept_ids
    assert a.find_neighbors("c8", 5) == f.find_neighbors("c8", 5)
    assert a.find_neighbors(f"c{n - 2}", 5) == f.find_neighbors(f"c{n - 2}", 5)
    # integer ids
    b = HipIndex.build_from_flat(None, flat, row_base=10)
    assert b.remove(["15", "x", "9", str(10 + n), "15", "11"]) == 2 and len(b) == n - 2
    b.close()
    # an injected device failure (the hook cqs_hip_index_search's tests use): HipError, id_map as it was, handle poisoned
    hip.cqs_hip_debug_index_fail_next.argtypes = [C.c_void_p]
    hip.cqs_hip_debug_index_fail_next.restype = None
    hip.cqs_hip_debug_index_fail_next(a._h)
    with pytest.raises(HipError) as e:
        a.remove(["c8", "c9"])
    assert e.value.code == _lib.ERR_DEVICE and a.id_map == kept_ids and a.is_poisoned()
    with pytest.raises(HipError) as e:
        a.remove(["c8"])
    assert e.value.code == _lib.ERR_POISONED and a.id_map == kept_ids
    a.close(); f.close()
