"""The device-free part of cqs_hip_index_match (cqs_amd/csrc/match_host.h) in a stand-alone program under ASAN + UBSan: the
argument plan (every refusal alone, and together for their order; row_base 0 and 5000; rows at both ends of each index; an
empty side; one row too many), the global -> local rows, the packed key's round trip with its "none" sentinel, merge_best
and mutual_pairs against brute force over score matrices full of exact ties.  Then the C ABI's new symbol without a
device, and the Python logic of HipIndex.match_rows (blocking, merging) and semantic_diff(..., moved_threshold=...) over a
numpy stand-in for the device call.  No GPU."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_cases as mc  # noqa: E402

INVALID, NOTHING, RUN = "-1", "0", "1"
DRIVER = os.path.join(ROOT, "tests", "match_host_driver.cpp")
MAX = mc.MATCH_MAX


def fbits(x):
    return int(np.float32(x).view(np.uint32))


def side(present=1, sharded=0, device=0, dim=768, base=0, length=1000):
    return (present, sharded, device, dim, base, length)


def _plan_cases():
    """name -> (side a, side b, m_a, m_b, (rows_a, rows_b, best_a, score_a, best_b, score_b present), rows_a, rows_b, plan, why)."""
    c = {}
    full = (1, 1, 1, 1, 1, 1)
    for base in (0, 5000):
        t = f"_base{base}"
        a, b = side(base=base, length=1000), side(base=base + 7, length=300)
        lo_a, hi_a, lo_b, hi_b = base, base + 999, base + 7, base + 306
        c["ends_of_both" + t] = (a, b, 4, 3, full, [lo_a, hi_a, hi_a, lo_a], [hi_b, lo_b, hi_b], RUN, "")
        c["a_row_repeats" + t] = (a, b, 3, 1, full, [lo_a + 5] * 3, [lo_b], RUN, "")
        c["same_handle" + t] = (a, a, 2, 2, full, [lo_a, hi_a], [hi_a, hi_a], RUN, "")
        c["empty_b" + t] = (a, b, 2, 0, (1, 0, 1, 1, 0, 0), [lo_a, hi_a], [], RUN, "")
        c["empty_a" + t] = (a, b, 0, 2, (0, 1, 0, 0, 1, 1), [], [lo_b, hi_b], RUN, "")
        c["a_full_list" + t] = (a, b, MAX, 1, full, [lo_a + i % 1000 for i in range(MAX)], [lo_b], RUN, "")
        # every refusal alone
        c["null_a" + t] = (side(present=0), b, 1, 1, full, [lo_a], [lo_b], INVALID, "null handle")
        c["null_b" + t] = (a, side(present=0), 1, 1, full, [lo_a], [lo_b], INVALID, "null handle")
        c["null_rows_a" + t] = (a, b, 1, 1, (0, 1, 1, 1, 1, 1), [lo_a], [lo_b], INVALID, "null rows_a")
        c["null_rows_b" + t] = (a, b, 1, 1, (1, 0, 1, 1, 1, 1), [lo_a], [lo_b], INVALID, "null rows_b")
        c["null_best_a" + t] = (a, b, 1, 1, (1, 1, 0, 1, 1, 1), [lo_a], [lo_b], INVALID, "null output of side a")
        c["null_score_a" + t] = (a, b, 1, 1, (1, 1, 1, 0, 1, 1), [lo_a], [lo_b], INVALID, "null output of side a")
        c["null_best_b" + t] = (a, b, 1, 1, (1, 1, 1, 1, 0, 1), [lo_a], [lo_b], INVALID, "null output of side b")
        c["null_score_b" + t] = (a, b, 1, 1, (1, 1, 1, 1, 1, 0), [lo_a], [lo_b], INVALID, "null output of side b")
        c["null_out_b_with_empty_a" + t] = (a, b, 0, 1, (0, 1, 0, 0, 1, 0), [], [lo_b], INVALID, "null output of side b")
        c["a_one_too_many" + t] = (a, b, MAX + 1, 1, full, [lo_a] * (MAX + 1), [lo_b], INVALID, "m_a above CQS_HIP_MATCH_MAX")
        c["b_one_too_many" + t] = (a, b, 1, MAX + 1, full, [lo_a], [lo_b] * (MAX + 1), INVALID, "m_b above CQS_HIP_MATCH_MAX")
        c["sharded_a" + t] = (side(sharded=1, base=base, length=0), b, 1, 1, full, [lo_a], [lo_b], INVALID, "not built for a row-sharded handle")
        c["sharded_b" + t] = (a, side(sharded=1, base=base, length=0), 1, 1, full, [lo_a], [lo_b], INVALID, "not built for a row-sharded handle")
        c["other_device" + t] = (a, side(device=1, base=base + 7, length=300), 1, 1, full, [lo_a], [lo_b], INVALID, "the two handles are on different devices")
        c["other_dim" + t] = (a, side(dim=252, base=base + 7, length=300), 1, 1, full, [lo_a], [lo_b], INVALID, "the two handles differ in dim")
        c["a_past_end" + t] = (a, b, 3, 1, full, [lo_a, hi_a + 1, lo_a], [lo_b], INVALID, "rows_a[1] not in its index")
        c["b_past_end" + t] = (a, b, 1, 3, full, [lo_a], [lo_b, lo_b, hi_b + 1], INVALID, "rows_b[2] not in its index")
        c["b_below_base" + t] = (a, b, 1, 2, full, [lo_a], [lo_b - 1, lo_b], INVALID, "rows_b[0] not in its index")
        c["a_wraps" + t] = (a, b, 1, 1, full, [2 ** 64 - 1], [lo_b], INVALID, "rows_a[0] not in its index")
        c["a_before_b" + t] = (a, b, 3, 2, full, [lo_a, lo_a, hi_a + 6], [hi_b + 9, lo_b], INVALID, "rows_a[2] not in its index")
        c["empty_index" + t] = (side(base=base, length=0), b, 1, 1, full, [lo_a], [lo_b], INVALID, "rows_a[0] not in its index")
        c["a_bad_with_empty_b" + t] = (a, b, 1, 0, (1, 0, 1, 1, 0, 0), [hi_a + 1], [], INVALID, "rows_a[0] not in its index")
        # ... and together: the first in the documented order answers.  Each case has everything wrong that comes after.
        wrong_b = side(sharded=1, device=1, dim=252, base=base + 7, length=0)
        over = [9999999] * (MAX + 1)
        c["order_1_null_handle" + t] = (side(present=0), wrong_b, MAX + 1, MAX + 1, (0, 0, 0, 0, 0, 0), [], [], INVALID, "null handle")
        c["order_2_nothing" + t] = (a, wrong_b, 0, 0, (0, 0, 0, 0, 0, 0), [], [], NOTHING, "")
        c["order_3_null_rows_a" + t] = (a, wrong_b, MAX + 1, MAX + 1, (0, 0, 0, 0, 0, 0), [], [], INVALID, "null rows_a")
        c["order_3_null_rows_b" + t] = (a, wrong_b, MAX + 1, MAX + 1, (1, 0, 0, 0, 0, 0), over, [], INVALID, "null rows_b")
        c["order_4_null_out_a" + t] = (a, wrong_b, MAX + 1, MAX + 1, (1, 1, 1, 0, 0, 0), over, over, INVALID, "null output of side a")
        c["order_4_null_out_b" + t] = (a, wrong_b, MAX + 1, MAX + 1, (1, 1, 1, 1, 0, 1), over, over, INVALID, "null output of side b")
        c["order_5_m_a" + t] = (a, wrong_b, MAX + 1, MAX + 1, full, over, over, INVALID, "m_a above CQS_HIP_MATCH_MAX")
        c["order_5_m_b" + t] = (a, wrong_b, 2, MAX + 1, full, [9999999, 0], over, INVALID, "m_b above CQS_HIP_MATCH_MAX")
        c["order_6_sharded" + t] = (a, wrong_b, 2, 2, full, [9999999, 0], [0, 0], INVALID, "not built for a row-sharded handle")
        c["order_7_device" + t] = (a, side(device=1, dim=252, base=base + 7, length=0), 2, 2, full, [9999999, 0], [0, 0], INVALID,
                                   "the two handles are on different devices")
        c["order_8_dim" + t] = (a, side(dim=252, base=base + 7, length=0), 2, 2, full, [9999999, 0], [0, 0], INVALID, "the two handles differ in dim")
        c["nothing" + t] = (a, b, 0, 0, full, [], [], NOTHING, "")
    return c


PLANS = _plan_cases()
MATRICES = {"ties_7x9": (7, 9, True), "ties_40x33": (40, 33, True), "ties_65x130": (65, 130, True), "finite_50x50": (50, 50, False),
            "one_row": (1, 20, True), "one_column": (20, 1, False)}
BLOCKS = (1, 7, 32, 1000)
KEYS = {"one": (1.0, 0), "minus_one_far": (-1.0, 0xFFFFFFFE), "zero": (0.0, 5), "minus_zero": (-0.0, 5), "tiny": (1e-45, 65535), "huge": (3e38, 7),
        "most_negative": (-3.4028235e38, 0), "inf": (np.inf, 3), "minus_inf": (-np.inf, 3), "nan": (np.nan, 3), "minus_nan": (-np.nan, 0)}


def _write_matrix(path, s):
    with open(path, "wb") as f:
        f.write(struct.pack("<2Q", s.shape[0], s.shape[1]))
        f.write(np.ascontiguousarray(s, np.float32).tobytes())


@pytest.fixture(scope="module")
def matrices(tmp_path_factory):
    d = tmp_path_factory.mktemp("match_matrices")
    out = {}
    for i, (name, (m_a, m_b, non_finite)) in enumerate(MATRICES.items()):
        s = mc.tie_matrix(m_a, m_b, 40 + i, non_finite)
        path = str(d / (name + ".bin"))
        _write_matrix(path, s)
        out[name] = (s, path)
    return out


@pytest.fixture(scope="module")
def got(tmp_path_factory, matrices):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("match_host") / "match_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", str(exe)], check=True, capture_output=True)
    lines = []
    for name, (a, b, m_a, m_b, flags, ra, rb, _, _) in PLANS.items():
        lines.append(" ".join(str(v) for v in ("plan", name) + a + b + (m_a, m_b) + flags + (len(ra),) + tuple(ra) + (len(rb),) + tuple(rb)))
    for name, (score, pos) in KEYS.items():
        lines.append(f"key {name} {fbits(score)} {pos}")
    for name, (_, path) in matrices.items():
        for block in BLOCKS:
            for rev in (0, 1):
                lines.append(f"merge {name}@{block}@{rev} {path} {block} {rev}")
        for ti, thr in enumerate((-np.inf, -0.0625, 0.0, 0.125, 0.1875, np.inf, np.nan)):
            lines.append(f"mutual {name}#{ti} {path} {fbits(thr)}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    ints = lambda s: [int(x) for x in s.split(",") if x]
    plans, keys, merges, mutuals = {}, {}, {}, {}
    for ln in p.stdout.splitlines():
        f = ln.split("|")
        if f[0] in PLANS:
            plans[f[0]] = (f[1], f[2], ints(f[3]), ints(f[4]))
        elif f[0] in KEYS:
            keys[f[0]] = tuple(int(x) for x in f[1:4])
        elif "@" in f[0]:
            assert len(f) == 5, ln[:200]
            merges[f[0]] = tuple(ints(x) for x in f[1:5])
        else:
            mutuals[f[0]] = [tuple(int(x) for x in t.split(":")) for t in f[1].split(",") if t]
    assert set(plans) == set(PLANS) and set(keys) == set(KEYS)
    assert len(merges) == len(MATRICES) * len(BLOCKS) * 2 and len(mutuals) == len(MATRICES) * 7
    return plans, keys, merges, mutuals


def test_every_refusal_alone_and_their_order(got):
    plans = got[0]
    for name, case in PLANS.items():
        assert plans[name][:2] == (case[7], case[8]), name
        if case[7] == RUN:                                                       # the rows the kernel would take: row_base taken off
            assert plans[name][2] == [r - case[0][4] for r in case[5]] and plans[name][3] == [r - case[1][4] for r in case[6]], name
    assert sum(1 for c in PLANS.values() if c[7] == INVALID) >= 2 * 30 and sum(1 for c in PLANS.values() if c[7] == RUN) == 2 * 6
    assert plans["ends_of_both_base5000"][2] == [0, 999, 999, 0] and plans["ends_of_both_base5000"][3] == [299, 0, 299]


def test_key_round_trip_and_the_sentinel(got):
    keys = got[1]
    for name, (score, pos) in KEYS.items():
        key, best, score_bits = keys[name]
        if np.isfinite(score):
            assert key != 0 and best == pos and score_bits == fbits(score), name
            assert key == (int(mc.order_keys(np.float32([score]))[0]) << 32) | (0xFFFFFFFF - pos), name
        else:
            assert (key, best, score_bits) == (0, mc.NONE, 0), name              # "none": (UINT64_MAX, +0.0f)
    order = ["most_negative", "minus_one_far", "minus_zero", "zero", "tiny", "one", "huge"]
    assert [keys[n][0] for n in order] == sorted(keys[n][0] for n in order)      # the f32 total order, -0.0 below +0.0
    assert keys["most_negative"][0] > 0                                          # every real candidate is above "none"


def test_merge_best_over_blocks_is_the_one_block_answer(got, matrices):
    merges = got[2]
    some_none = some_tie = False
    for name, (s, _) in matrices.items():
        want = mc.expected_bests(s)
        # the vectorised expectation (what the GPU tests compare against) is itself held to a plain double loop
        for (b, sc), (bb, bsc) in ((want[:2], mc.brute_side(s)), (want[2:], mc.brute_side(np.ascontiguousarray(s.T)))):
            assert np.array_equal(b, bb) and np.array_equal(mc.bits(sc), mc.bits(bsc)), name
        want = (want[0].tolist(), mc.bits(want[1]).tolist(), want[2].tolist(), mc.bits(want[3]).tolist())
        for block in BLOCKS:
            for rev in (0, 1):
                assert merges[f"{name}@{block}@{rev}"] == want, (name, block, rev)
        some_none |= mc.NONE in want[0] and mc.NONE in want[2]
        k = mc.order_keys(s)
        some_tie |= bool(((k == k.max(axis=1, keepdims=True)) & (k >= 0)).sum(axis=1).max() > 1)
    assert some_none and some_tie


def test_mutual_pairs_against_brute_force(got, matrices):
    mutuals = got[3]
    kept = set()
    for name, (s, _) in matrices.items():
        best_a, score_a, best_b, _ = mc.expected_bests(s)
        for ti, thr in enumerate((-np.inf, -0.0625, 0.0, 0.125, 0.1875, np.inf, np.nan)):
            want = mc.brute_mutual(best_a, score_a, best_b, thr)
            assert mutuals[f"{name}#{ti}"] == want, (name, thr)
            assert len({i for i, _ in want}) == len(want) == len({j for _, j in want})          # one-to-one
            kept.add((ti, bool(want)))
        assert mutuals[f"{name}#6"] == [] and mutuals[f"{name}#5"] == []        # NaN keeps nothing; nothing reaches +inf
    assert (0, True) in kept and (3, True) in kept and (2, True) in kept


def test_match_symbol_without_a_device():
    """The library exports the entry point; a null handle is refused before anything else, the outputs untouched."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    rows = np.arange(4, dtype=np.uint64)
    o = [np.full(4, 7, np.uint64), np.full(4, 7.0, np.float32), np.full(4, 7, np.uint64), np.full(4, 7.0, np.float32)]
    ptrs = [x.ctypes.data for x in o]
    assert lib.cqs_hip_index_match(None, rows.ctypes.data, 4, None, rows.ctypes.data, 4, *ptrs) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_match(None, None, 0, None, None, 0, *ptrs) == _lib.ERR_INVALID          # (before "both lists empty")
    assert all((x == 7).all() for x in o)
    assert _lib.MATCH_MAX == mc.MATCH_MAX
    text = open(os.path.join(ROOT, "include", "cqs_hip.h")).read()
    assert f"#define CQS_HIP_MATCH_MAX {mc.MATCH_MAX}u" in text


# ---- HipIndex.match_rows / semantic_diff(moved_threshold): the Python logic over a numpy stand-in ------------------------
def _fake(scores, base_a=0, base_b=0, ids_a=None, ids_b=None):
    from cqs_amd.index import HipIndex
    for name in ("match_rows", "semantic_diff"):
        setattr(mc.FakeMatcher, name, getattr(HipIndex, name))
    return mc.FakeMatcher(scores, base_a, ids_a), mc.FakeMatcher(np.zeros((0, 0), np.float32), base_b, ids_b)


def test_match_rows_blocks_merge_to_the_one_call_answer():
    s = mc.tie_matrix(130, 97, 77)
    a, b = _fake(s, base_a=5000, base_b=40)
    rng = np.random.default_rng(1)
    la, lb = rng.integers(0, 130, 210), rng.integers(0, 97, 150)                  # repeats: equal rows at several positions
    la[[3, 200]], lb[[5, 140]] = 130 // 2, 97 // 3                                # the row and the column without a finite entry
    ra, rb = la.astype(np.uint64) + np.uint64(5000), lb.astype(np.uint64) + np.uint64(40)
    want = mc.expected_bests(s[np.ix_(la, lb)])
    assert mc.NONE in want[0] and mc.NONE in want[2]
    for block in (mc.MATCH_MAX, 210, 105, 64, 50, 7, 1):                          # blocks that do and do not divide the lists
        a.calls.clear()
        got = a.match_rows(b, ra, rb, block=block)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), block
        assert len(a.calls) == -(-210 // block) * -(-150 // block) and max(max(c) for c in a.calls) <= block
    # an empty side, and both
    got = a.match_rows(b, ra[:5], np.zeros(0, np.uint64), block=2)
    assert (got[0] == mc.NONE).all() and (mc.bits(got[1]) == 0).all() and len(got[2]) == 0 and len(got[3]) == 0
    got = a.match_rows(b, [], [])
    assert all(len(x) == 0 for x in got)
    for bad in (0, mc.MATCH_MAX + 1):
        with pytest.raises(ValueError):
            a.match_rows(b, ra, rb, block=bad)


def test_merge_and_mutual_mirrors_are_the_headers(got, matrices):
    """cqs_amd.index.merge_best / mutual_pairs against the driver's answers (match_host.h) on the same matrices."""
    from cqs_amd.index import MATCH_NONE, merge_best, mutual_pairs
    assert MATCH_NONE == mc.NONE
    merges, mutuals = got[2], got[3]
    for name, (s, _) in matrices.items():
        best, score = np.full(s.shape[0], mc.NONE, np.uint64), np.zeros(s.shape[0], np.float32)
        for j0 in reversed(range(0, s.shape[1], 7)):
            b, sc = mc.expected_side(s[:, j0:j0 + 7])
            b[b != np.uint64(mc.NONE)] += np.uint64(j0)
            merge_best(best, score, b, sc)
        assert best.tolist() == merges[f"{name}@7@1"][0] and mc.bits(score).tolist() == merges[f"{name}@7@1"][1], name
        best_a, score_a, best_b, _ = mc.expected_bests(s)
        for ti, thr in enumerate((-np.inf, -0.0625, 0.0, 0.125, 0.1875, np.inf, np.nan)):
            assert mutual_pairs(best_a, score_a, best_b, thr) == mutuals[f"{name}#{ti}"], (name, thr)


def _diff_fakes():
    """Source and target whose diff has three removed and three added chunks: one moved with an identical vector (1.0),
    one renamed (0.96875), one pair of strangers (0.25); `diff_rows` is a stub that reports every matched pair unchanged."""
    ids_a = ["a.rs:keep", "a.rs:moves", "a.rs:old_name", "a.rs:deleted"]
    ids_b = ["b.rs:moves", "a.rs:keep", "a.rs:brand_new", "a.rs:new_name"]
    s = np.float32([[0.0, 0.5, 0.0, 0.0], [1.0, 0.0, 0.125, 0.5], [0.5, 0.0, 0.125, 0.96875], [0.125, 0.0, 0.25, 0.125]])
    a, b = _fake(s, base_a=100, base_b=7, ids_a=ids_a, ids_b=ids_b)
    stub = lambda self, other, ra, rb, thr, want_sims=False: (np.zeros(0, np.uint64), np.zeros(0, np.float32), np.asarray([0, len(ra), 0], np.uint64))
    mc.FakeMatcher.diff_rows = stub
    return a, b


def test_semantic_diff_moved_threshold_host_logic():
    from cqs_amd.index import DiffEntry, DiffResult, MovedEntry
    a, b = _diff_fakes()
    plain = a.semantic_diff(b, 0.95)
    assert plain == DiffResult([DiffEntry("b.rs:moves", None), DiffEntry("a.rs:brand_new", None), DiffEntry("a.rs:new_name", None)],
                               [DiffEntry("a.rs:moves", None), DiffEntry("a.rs:old_name", None), DiffEntry("a.rs:deleted", None)], [], 1)
    assert plain.moved == [] and a.calls == []                                    # the default: today's result, no match call
    assert a.semantic_diff(b, 0.95, moved_threshold=None) == plain and a.calls == []
    d = a.semantic_diff(b, 0.95, moved_threshold=0.9)
    assert a.calls == [(3, 3)]                                                    # removed against added, global rows on each side
    assert d.moved == [MovedEntry("a.rs:old_name", "a.rs:new_name", 0.96875), MovedEntry("a.rs:moves", "b.rs:moves", 1.0)]   # similarity ascending
    assert [x.id for x in d.added] == ["a.rs:brand_new"] and [x.id for x in d.removed] == ["a.rs:deleted"]
    assert d.modified == [] and d.unchanged_count == 1
    # the threshold is inclusive and an f32 compare; the strangers are mutual at 0.25 and move only under it
    assert len(a.semantic_diff(b, 0.95, moved_threshold=0.96875).moved) == 2 and len(a.semantic_diff(b, 0.95, moved_threshold=0.97).moved) == 1
    d = a.semantic_diff(b, 0.95, moved_threshold=0.25)
    assert [m.source_id for m in d.moved] == ["a.rs:deleted", "a.rs:old_name", "a.rs:moves"] and d.added == [] and d.removed == []
    assert a.semantic_diff(b, 0.95, moved_threshold=float("inf")) == plain
    with pytest.raises(ValueError):
        a.semantic_diff(b, 0.95, moved_threshold=float("nan"))
    # equal similarities: ties by target id
    from cqs_amd.index import sort_moved
    got = sort_moved([MovedEntry("x", "t2", 0.5), MovedEntry("y", "t1", 0.5), MovedEntry("z", "t0", 0.75), MovedEntry("w", "t9", -0.0), MovedEntry("v", "t8", 0.0)])
    assert [m.target_id for m in got] == ["t9", "t8", "t1", "t2", "t0"]
    # existing constructions and comparisons keep working
    assert DiffResult([], [], [], 0) == DiffResult([], [], [], 0, []) and DiffResult([], [], [], 0).moved == []


def test_mid_case_seed_leaves_few_near_ties():
    """tests/test_match_gpu.py's mid-size case: numpy f64 alone leaves at most 1 % of the rows of either side with a
    runner-up within the near-tie band of the best (the GPU test asserts the same before it compares positions).  A check
    of the test data alone, on the CPU, so it does not depend on the library."""
    a, b, ra, rb = mc.mid_case()
    assert a.shape == b.shape == (5000, 768) and len(ra) == 1000 and len(rb) == 3000
    (_, _, clear_a), (_, _, clear_b) = mc.mid_reference(a, b, ra, rb)
    assert (~clear_a).mean() <= mc.MID_TIE_SHARE and (~clear_b).mean() <= mc.MID_TIE_SHARE
    assert mc.MID_TIE_BAND == 2e-6 and mc.MID_SCORE_TOL == 1e-5 and mc.MID_TIE_SHARE == 0.01
