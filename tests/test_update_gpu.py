"""`cqs_hip_index_update` / `HipIndex.update_rows` / `HipIndex.update` (include/cqs_hip.h): stored rows are
rewritten where they lie, the shadow's copies of them included.

The yardstick everywhere is a fresh `HipIndex.build_from_flat` of the patched array: after an update the index must be
indistinguishable from it - the same bytes from every search (rows, score BITS, counts), the same bf16 words, int8 codes
and scales over ALL rows, the same saved blob.  No tolerance anywhere except for the blocks of 32 queries on the matrix
cores, which go through tests/parity.py first as in tests/test_remove_gpu.py.  Run on an MI355X with `pytest -m gpu`."""
import ctypes as C
import json
import threading

import numpy as np
import pytest

from cqs_amd import DistanceMetric, HipError, HipIndex, _lib, synth
from cqs_amd.index import tag_filter
from test_remove_gpu import assert_same, assert_searches_match

pytestmark = pytest.mark.gpu
ENV_BF16, ENV_I8 = "CQS_HIP_SCAN_BF16", "CQS_HIP_SCAN_I8"
BF16, I8 = 1, 2
# no shadow; bf16 without int8; the smallest int8 dim; % 8 but not % 16 or % 128; the workload's; the shadow's largest; past it
N_OF_DIM = {4: 5000, 8: 3000, 16: 3000, 72: 3000, 768: 4097, 2048: 1500, 4096: 1001}
SMALL_BUDGET = 1000               # rows per pass: the block and the larger patterns take 3-5 passes that straddle them;
                                  # 0 = the staging buffer's own byte budget, which every update here fits in one pass
PATTERNS = ("one", "row0", "last", "block", "every_second", "random30", "all")


def pattern(name, n):
    if name == "one":
        return np.array([n // 3])
    if name == "row0":
        return np.array([0])
    if name == "last":
        return np.array([n - 1])
    if name == "block":
        return np.arange(200, 600)
    if name == "every_second":
        return np.arange(0, n, 2)
    if name == "random30":
        return np.random.default_rng(n).choice(n, size=int(0.3 * n), replace=False)
    if name == "all":
        return np.arange(n)
    raise KeyError(name)


def shadow_env(monkeypatch, on):
    monkeypatch.setenv(ENV_BF16, "1" if on else "0")
    if on:
        monkeypatch.setenv(ENV_I8, "1")


def expect_copies(dim, on):
    """(bf16 copy, int8 copy) a handle of this dim holds under shadow_env(on)."""
    bf16 = on and dim % 8 == 0 and dim <= 2048
    return bf16, bf16 and dim % 16 == 0


@pytest.fixture
def hooks(hip):
    hip.cqs_hip_debug_shadow_rows.restype = C.c_int32
    hip.cqs_hip_debug_shadow_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return hip


def set_budget(hip, idx, rows):
    hip.cqs_hip_debug_index_update_budget(idx._h, rows)


def read_bf16(hooks, h):
    out = np.zeros((len(h), h.dim()), np.uint16)
    assert hooks.cqs_hip_debug_shadow_rows(h._h, BF16, 0, len(h), out.ctypes.data, None) == _lib.OK
    return out


def read_i8(hooks, h):
    codes, scales = np.zeros((len(h), h.dim()), np.int8), np.zeros(len(h), np.float32)
    assert hooks.cqs_hip_debug_shadow_rows(h._h, I8, 0, len(h), codes.ctypes.data, scales.ctypes.data) == _lib.OK
    return codes, scales


def assert_shadow_bytes_match(hooks, a, f, ctx=""):
    """Both copies over ALL rows, the updated ones and the untouched ones; the same copies exist on both handles."""
    assert a.bf16_stats()[0] == f.bf16_stats()[0] and a.i8_stats()[0] == f.i8_stats()[0], (ctx, a.last_error(), f.last_error())
    if a.bf16_stats()[0]:
        assert np.array_equal(read_bf16(hooks, a), read_bf16(hooks, f)), ctx
    if a.i8_stats()[0]:
        (ca, sa), (cf, sf) = read_i8(hooks, a), read_i8(hooks, f)
        assert np.array_equal(ca, cf) and np.array_equal(sa.view(np.uint32), sf.view(np.uint32)), ctx


def assert_saves_match(a, f, tmp_path, ctx=""):
    pa, pf = str(tmp_path / "a.hipflat"), str(tmp_path / "f.hipflat")
    a.save(pa); f.save(pf)
    assert open(pa, "rb").read() == open(pf, "rb").read(), ctx
    assert json.load(open(pa + ".meta"))["checksum"] == json.load(open(pf + ".meta"))["checksum"], ctx


def assert_search_bits_match(a, f, q, ctx=""):
    """assert_searches_match's list of searches, bits alone: with a NaN row stored, a score may be NaN, which no
    tolerance compares; the bytes still have to be the fresh index's."""
    assert len(a) == len(f), ctx
    for b in (1, 8, 32):
        for k in (1, 20, 500):
            assert_same(a.search_batch(q[:b], k), f.search_batch(q[:b], k), (ctx, b, k))


def patched_with(flat, rows, seed):
    """(the new vectors of `rows`, `flat` with them written in)."""
    new = synth.gaussian_unit(len(rows), dim=flat.shape[1], seed=seed)
    out = flat.copy()
    out[rows] = new
    return new, out


@pytest.mark.parametrize("shadow", (True, False), ids=("shadow", "f32"))
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("dim", sorted(N_OF_DIM))
def test_update_matches_rebuild(hooks, monkeypatch, tmp_path, dim, name, shadow):
    shadow_env(monkeypatch, shadow)
    n = N_OF_DIM[dim]
    flat = synth.gaussian_unit(n, dim=dim, seed=9000 + dim)
    q = synth.gaussian_unit(32, dim=dim, seed=9100 + dim)
    rows = pattern(name, n)
    rows = rows[np.random.default_rng(17).permutation(len(rows))]      # unsorted
    new, patched = patched_with(flat, rows, 9200 + dim)
    has_bf16, has_i8 = expect_copies(dim, shadow)
    combos = ((DistanceMetric.Cosine, 0, 0), (DistanceMetric.DotProduct, 1000, SMALL_BUDGET),
              (DistanceMetric.Cosine, 1000, SMALL_BUDGET), (DistanceMetric.DotProduct, 0, 0))
    for metric, base, budget in combos:
        ctx = (dim, name, shadow, metric, base, budget)
        a = HipIndex.build_from_flat(None, flat, metric, row_base=base)
        f = HipIndex.build_from_flat(None, patched, metric, row_base=base)
        sizes = a.bf16_stats()[0], a.i8_stats()[0]
        assert sizes == (n * dim * 2 if has_bf16 else 0, n * dim + n * 4 if has_i8 else 0), (ctx, a.last_error())
        a.search_batch(q[:8], 20)                                       # warm: scratch exists before the update
        set_budget(hooks, a, budget)
        assert a.update_rows(rows + base, new) == len(rows)
        assert len(a) == n and int(hooks.cqs_hip_index_row_base(a._h)) == base and not a.is_poisoned()
        assert (a.bf16_stats()[0], a.i8_stats()[0]) == sizes, ctx
        assert_searches_match(a, f, q, ctx)
        assert_shadow_bytes_match(hooks, a, f, ctx)
        if budget:
            assert_saves_match(a, f, tmp_path, ctx)
        a.close(); f.close()


@pytest.mark.parametrize("dim", (16, 768))
def test_rule_by_rule_rows(hooks, monkeypatch, dim):
    shadow_env(monkeypatch, True)
    n = 3000
    flat = synth.gaussian_unit(n, dim=dim, seed=9300 + dim)
    q = synth.gaussian_unit(32, dim=dim, seed=9301 + dim)
    rows = np.array([2500, 7, 1024])
    new = synth.gaussian_unit(3, dim=dim, seed=9302 + dim)
    new[0] = 0.0                                                        # a zero row
    new[1, dim // 2] = np.nan                                           # a row with one NaN
    new[2] *= 0.25
    new[2, dim - 1] = 3.0                                               # a row whose maximum sits in the last component
    patched = flat.copy()
    patched[rows] = new
    a = HipIndex.build_from_flat(None, flat)
    f = HipIndex.build_from_flat(None, patched)
    assert a.bf16_stats()[0] and a.i8_stats()[0], a.last_error()
    a.search_batch(q[:8], 20)
    assert a.update_rows(rows, new) == 3
    assert_search_bits_match(a, f, q, (dim, "zero, NaN, last-component maximum"))
    assert_shadow_bytes_match(hooks, a, f, dim)
    codes, scales = read_i8(hooks, a)
    assert not codes[2500].any() and scales[2500] == 0.0                # as a fresh build stores them
    assert np.isnan(scales[7]) and not codes[7].any()
    assert codes[1024, dim - 1] == 127
    # a finite component of 2^64: the shadow cannot certify against it and goes, as in extend; the call succeeds
    big = synth.gaussian_unit(1, dim=dim, seed=9303 + dim)
    big[0, 3] = 2.0 ** 64
    patched[11] = big[0]
    assert a.update_rows([11], big) == 1
    assert ">= 2^64" in a.last_error() and "shadow turned off" in a.last_error() and a.last_error().startswith("update:")
    assert a.bf16_stats()[0] == 0 and a.i8_stats()[0] == 0 and not a.is_poisoned()
    g = HipIndex.build_from_flat(None, patched)                         # (builds no shadow either, for the same row)
    assert g.bf16_stats()[0] == 0
    assert_search_bits_match(a, g, q, (dim, "2^64"))
    a.close(); f.close(); g.close()


def test_refused_calls_leave_the_index_untouched(hip, monkeypatch):
    import torch
    shadow_env(monkeypatch, True)
    n, dim, base = 3000, 768, 100
    flat = synth.gaussian_unit(n, dim=dim, seed=9400)
    q = synth.gaussian_unit(8, dim=dim, seed=9401)
    new = synth.gaussian_unit(3, dim=dim, seed=9402)
    a = HipIndex.build_from_flat(None, flat, row_base=base)
    before = a.search_batch(q, 20)
    for bad, why in (([150, base + n, 151], "row id not in this index"), ([150, base - 1, 151], "row id not in this index"),
                     ([150, 151, 150], "row id named twice"), ([150, 150, 151], "row id named twice")):
        with pytest.raises(HipError) as e:
            a.update_rows(bad, new)
        assert e.value.code == _lib.ERR_INVALID and "update: " + why in str(e.value), bad
    r = np.array([150, 151, 152], dtype=np.uint64)
    assert hip.cqs_hip_index_update(a._h, r.ctypes.data, None, 3, None) == _lib.ERR_INVALID and "update: null vectors" in a.last_error()
    assert hip.cqs_hip_index_update(a._h, None, new.ctypes.data, 3, None) == _lib.ERR_INVALID and "update: null rows" in a.last_error()
    assert hip.cqs_hip_index_update(a._h, None, None, 0, None) == _lib.OK            # m == 0: nothing, whatever the pointers
    assert a.update_rows([], np.zeros((0, dim), np.float32)) == 0
    assert len(a) == n and not a.is_poisoned()
    assert_same(a.search_batch(q, 20), before, "after the refused calls")
    a.close()
    # a borrowed handle: the rows are the caller's
    d = torch.from_numpy(flat).cuda()
    b = HipIndex.build_from_device(None, d.data_ptr(), n, dim, borrow=True, keepalive=d)
    before = b.search_batch(q, 20)
    with pytest.raises(HipError) as e:
        b.update_rows([5, 6, 7], new)
    assert e.value.code == _lib.ERR_INVALID and "borrows" in str(e.value) and not b.is_poisoned()
    assert_same(b.search_batch(q, 20), before, "borrowed, after the refused call")
    assert np.array_equal(d.cpu().numpy(), flat)
    b.close()


def test_tagged_searches_after_update(hip, monkeypatch):
    shadow_env(monkeypatch, True)
    n, dim, base = 4097, 768, 1000
    flat = synth.gaussian_unit(n, dim=dim, seed=9500)
    q = synth.gaussian_unit(8, dim=dim, seed=9501)
    rows = pattern("random30", n)[::-1]
    new, patched = patched_with(flat, rows, 9502)
    tags = (np.arange(n, dtype=np.uint32) % 7) | ((np.arange(n, dtype=np.uint32) % 3) << 8)
    a = HipIndex.build_from_flat(None, flat, row_base=base)
    f = HipIndex.build_from_flat(None, patched, row_base=base)
    a.set_tags(tags, first=base); f.set_tags(tags, first=base)
    a.search_tagged_batch(q, 20, tag_filter([1, 2]))
    set_budget(hip, a, SMALL_BUDGET)
    assert a.update_rows(rows + base, new) == len(rows)
    assert a.tagged_rows() == n                                         # a chunk that keeps its id keeps its type and language
    for allow in (tag_filter([1, 2]), tag_filter(None, [0]), tag_filter([3], [1, 2]), tag_filter()):
        assert a.count_tagged(allow) == f.count_tagged(allow)
        for b, k in ((1, 20), (8, 20), (8, 500)):
            assert_same(a.search_tagged_batch(q[:b], k, allow), f.search_tagged_batch(q[:b], k, allow), (b, k))
    a.close(); f.close()


def test_update_remove_extend_update(hip, monkeypatch):
    shadow_env(monkeypatch, True)
    n, dim = 4097, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=9600)
    more = synth.gaussian_unit(700, dim=dim, seed=9601)
    q = synth.gaussian_unit(32, dim=dim, seed=9602)
    a = HipIndex.build_from_flat(None, flat)
    set_budget(hip, a, SMALL_BUDGET)
    up1 = pattern("random30", n)
    new1, cur = patched_with(flat, up1, 9603)
    assert a.update_rows(up1, new1) == len(up1)
    gone = pattern("block", n)
    assert a.remove_rows(gone) == len(gone)
    cur = np.delete(cur, gone, axis=0)
    a.extend(None, more[:100])                                          # inside cap_rows: lands where the removal made room
    a.extend(None, more[100:])                                          # past cap_rows: the corpus and its copies are reallocated
    cur = np.concatenate([cur, more])
    up2 = np.concatenate([np.arange(len(cur) - 650, len(cur) - 550), [0, 199, 200, 3500]])[::-1]   # extended rows, moved rows
    new2, cur = patched_with(cur, up2, 9604)
    assert a.update_rows(up2, new2) == len(up2)
    f = HipIndex.build_from_flat(None, cur)
    assert_searches_match(a, f, q, "update-remove-extend-update")
    # pairwise over a pool holding updated rows, neighbors of an updated row: the fresh index's bits
    pool = np.concatenate([up2[:20], np.arange(1000, 1020)]).astype(np.uint64)
    assert np.array_equal(a.pairwise_rows(pool).view(np.uint32), f.pairwise_rows(pool).view(np.uint32))
    for row in (int(up2[0]), 0, 1234):
        (ra, sa), (rf, sf) = a.neighbors_rows(row, 10), f.neighbors_rows(row, 10)
        assert np.array_equal(ra, rf) and np.array_equal(np.asarray(sa).view(np.uint32), np.asarray(sf).view(np.uint32)), row
    a.close(); f.close()


def test_update_by_id_skips_unknown_ids_and_keeps_id_map(hip):
    n, dim = 3000, 768
    flat = synth.gaussian_unit(n, dim=dim, seed=9700)
    q = synth.gaussian_unit(8, dim=dim, seed=9701)
    ids = [f"c{i}" for i in range(n)]
    asked = ["c2000", "never-indexed", "c5", f"c{n - 1}", "c999999", "c0"]
    held = [2000, 5, n - 1, 0]
    vec = synth.gaussian_unit(len(asked), dim=dim, seed=9702)
    patched = flat.copy()
    patched[held] = vec[[0, 2, 3, 5]]
    a = HipIndex.build_from_flat(list(ids), flat, row_base=1000)
    f = HipIndex.build_from_flat(list(ids), patched, row_base=1000)
    assert a.find_neighbors("c5", 3)                                    # (builds the id -> row cache: an update keeps it)
    assert a.update(asked, vec) == len(held)
    assert a.id_map == ids and len(a) == n
    assert a.update(["never-indexed"], vec[:1]) == 0
    with pytest.raises(ValueError):
        a.update(["c7", "c8", "c7"], vec[:3])                           # the reference's staging table: id TEXT PRIMARY KEY
    for i in range(3):
        assert a.search(q[i], 20) == f.search(q[i], 20)
    assert a.find_neighbors("c5", 5) == f.find_neighbors("c5", 5)
    a.close(); f.close()
    b = HipIndex.build_from_flat(None, flat, row_base=10)               # integer ids
    assert b.update(["15", "x", "9", str(10 + n), "11"], vec[:5]) == 2
    with pytest.raises(ValueError):
        b.update(["15", "015"], vec[:2])
    b.close()


def test_row_sharded_handle(hip):
    n, dim, base = 3000, 768, 1000
    flat = synth.gaussian_unit(n, dim=dim, seed=9800)
    q = synth.gaussian_unit(32, dim=dim, seed=9801)
    s = HipIndex.build_sharded(None, flat, [0, 0, 0], row_base=base)
    starts = [first for _, first, _, _ in s.shards()]
    assert starts == [base, base + 1024, base + 2048], s.shards()
    rows = np.concatenate([np.arange(900, 2200), [0, n - 1]])[::-1]     # spans both shard boundaries, both ends
    new, patched = patched_with(flat, rows, 9802)
    before = s.search_batch(q[:8], 20)
    # every id is checked against the whole handle first: a bad id in the LAST shard's range leaves the FIRST shard's rows
    for bad in ([5, 10, n - 2, n - 2], [5, 10, n]):
        with pytest.raises(HipError) as e:
            s.update_rows(np.array(bad) + base, new[:len(bad)])
        assert e.value.code == _lib.ERR_INVALID and "update: row id" in str(e.value) and not s.is_poisoned()
        assert_same(s.search_batch(q[:8], 20), before, bad)
    hip.cqs_hip_debug_index_update_budget(s._h, 300)
    assert s.update_rows(rows + base, new) == len(rows)
    f = HipIndex.build_sharded(None, patched, [0, 0, 0], row_base=base)
    assert [first for _, first, _, _ in s.shards()] == starts and len(s) == n
    assert_searches_match(s, f, q, "sharded")
    s.close(); f.close()


def test_searches_during_updates_see_one_version(hip, monkeypatch):
    """Four threads search one handle while a fifth flips 500 rows between two versions 40 times: every answer is, byte for
    byte, the lone answer under version A or under version B."""
    shadow_env(monkeypatch, True)
    n, dim, k = 4097, 768, 20
    flat = synth.gaussian_unit(n, dim=dim, seed=9900)
    q = synth.gaussian_unit(4, dim=dim, seed=9901)
    rows = np.random.default_rng(5).choice(n, size=500, replace=False)
    va = synth.gaussian_unit(500, dim=dim, seed=9902)
    vb = synth.gaussian_unit(500, dim=dim, seed=9903)
    # the rows under test are the queries' best matches in one version and far from them in the other
    va[:4] = q
    arr_a, arr_b = flat.copy(), flat.copy()
    arr_a[rows], arr_b[rows] = va, vb
    fa, fb = HipIndex.build_from_flat(None, arr_a), HipIndex.build_from_flat(None, arr_b)
    lone = [[tuple(x.tobytes() for x in h.search_batch(q[i:i + 1], k)) for h in (fa, fb)] for i in range(4)]
    assert all(lone[i][0] != lone[i][1] for i in range(4))
    fa.close(); fb.close()
    a = HipIndex.build_from_flat(None, arr_a)
    done = threading.Event()
    bad, seen, errors = [], [set() for _ in range(4)], []

    def searcher(i):
        try:
            for _ in range(100000):
                got = tuple(x.tobytes() for x in a.search_batch(q[i:i + 1], k))
                if got == lone[i][0]:
                    seen[i].add("A")
                elif got == lone[i][1]:
                    seen[i].add("B")
                else:
                    bad.append(i)
                if done.is_set():
                    break
        except Exception as e:                                          # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)

    def updater():
        try:
            for it in range(40):
                assert a.update_rows(rows, vb if it % 2 == 0 else va) == 500
        except Exception as e:                                          # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    threads = [threading.Thread(target=searcher, args=(i,)) for i in range(4)] + [threading.Thread(target=updater)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not bad, f"{len(bad)} answers were neither version's"
    assert not a.is_poisoned()
    print("versions seen per searcher:", [sorted(s) for s in seen])
    for i in range(4):                                                  # 40 updates, the last one back to A
        assert tuple(x.tobytes() for x in a.search_batch(q[i:i + 1], k)) == lone[i][0]
    a.close()
