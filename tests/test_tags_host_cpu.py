"""The device-free part of the row tags (cqs_amd/csrc/tags_host.h) in a stand-alone program under ASAN +
UBSan: the per-row rule tags_keep_kernel computes against a numpy restatement, the all-pass test, set_tags' range rules,
the count-taking keep rule against plan_keep on the equivalent bitset, and the tagged prefix after a removal.  Then
`tag_filter`'s bit layout and the C ABI's new symbols without a device.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tags_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOTHING, WRITE = "-1", "0", "1"
UNFILTERED, EMPTY, FILTERED = 0, 1, 2


def _keep_cases():
    """name -> (tags, allow, k)."""
    c = {}
    for n in (1, 31, 32, 33, 64, 65, 257, 1000):
        tags = tc.unique_end_tags(n, 10 + n)
        for fname, allow in tc.filters_for(tags, 20 + n).items():
            for k in (1, 20):
                c[f"n{n}_{fname}_k{k}"] = (tags, allow, k)
    rng = np.random.default_rng(5)
    for i in range(8):     # fully random tags and filters: every field value 0 .. 255 occurs
        n = int(rng.integers(1, 700))
        tags = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        allow = rng.integers(0, 2**32, size=32, dtype=np.uint64).astype(np.uint32)
        if i % 2:
            allow |= rng.integers(0, 2**32, size=32, dtype=np.uint64).astype(np.uint32)   # denser sets: some rows do pass
        c[f"random_{i}"] = (tags, allow, 7)
    edge = np.array([0x00000000, 0xFFFFFFFF, 0x000000FF, 0xFF000000, 0x00FF00FF], dtype=np.uint32)
    c["edge_0_and_255_allowed"] = (edge, tc.allow_of([0, 255], [0, 255], [0, 255], [0, 255]), 3)
    c["edge_only_0"] = (edge, tc.allow_of([0], [0], [0], [0]), 3)
    c["edge_only_255"] = (edge, tc.allow_of([255], [255], [255], [255]), 3)
    one_short = tc.ALL.copy()
    one_short[31] = 0x7FFFFFFF      # everything but value 255 of field 3: not all-pass, and row 1 of `edge` fails
    c["all_but_one_bit"] = (edge, one_short, 3)
    return c


SET_CASES = {   # name -> (first_row, m or ("null", m), row_base, len, tagged)
    "first_call_whole": (0, 100, 0, 100, 0),
    "first_call_part": (0, 40, 0, 100, 0),
    "overwrite_inside": (10, 20, 0, 100, 40),
    "overwrite_and_extend": (30, 50, 0, 100, 40),
    "extend_at_the_prefix_end": (40, 60, 0, 100, 40),
    "extend_to_exactly_len": (1040, 60, 1000, 100, 40),
    "gap": (41, 5, 0, 100, 40),
    "gap_with_base": (1041, 5, 1000, 100, 40),
    "gap_on_an_untagged_index": (1, 5, 0, 100, 0),
    "past_the_end": (40, 61, 0, 100, 40),
    "past_the_end_inside_prefix": (10, 91, 0, 100, 100),
    "past_the_end_huge_m": (0, 2**64 - 1, 0, 100, 100),
    "below_the_base": (999, 5, 1000, 100, 40),
    "nothing": (0, 0, 0, 100, 40),
    "nothing_anywhere": (5000, 0, 0, 100, 40),
    "nothing_null": (0, ("null", 0), 0, 100, 40),
    "null_tags": (0, ("null", 5), 0, 100, 40),
    "empty_index": (0, 1, 0, 0, 0),
}

RM_CASES = {    # name -> (n, row_base, tagged, ids)
    "below_the_prefix": (300, 0, 200, [5, 17, 199]),
    "above_the_prefix": (300, 0, 200, [200, 250, 299]),
    "straddling": (300, 0, 200, [198, 199, 200, 201]),
    "duplicates": (300, 0, 200, [5, 5, 250, 5, 199, 199]),
    "with_base": (300, 1000, 200, [1005, 1199, 1200]),
    "untagged_index": (300, 0, 0, [0, 1, 2]),
    "fully_tagged": (300, 0, 300, [0, 150, 299]),
    "everything": (50, 0, 20, list(range(50))),
    "whole_prefix": (300, 0, 100, list(range(100))),
}


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the stand-alone driver"
    exe = tmp_path_factory.mktemp("tags_host") / "tags_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "tags_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = []
    for name, (tags, allow, k) in _keep_cases().items():
        lines.append(" ".join(["keep", name, str(len(tags)), str(k)] + [f"{int(t):x}" for t in tags] + [f"{int(a):x}" for a in allow]))
    for name, (first, m, base, ln, tagged) in SET_CASES.items():
        ms = f"null {m[1]}" if isinstance(m, tuple) else str(m)
        lines.append(f"set {name} {first} {ms} {base} {ln} {tagged}")
    for name, (n, base, tagged, ids) in RM_CASES.items():
        lines.append(" ".join(["rm", name, str(n), str(base), str(tagged), str(len(ids))] + [str(i) for i in ids]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    out = {ln.split("|")[0]: ln.split("|")[1:] for ln in p.stdout.splitlines()}
    assert len(out) == len(lines)
    return out


def test_per_row_rule_matches_numpy(got):
    seen_kept = seen_dropped = 0
    for name, (tags, allow, _k) in _keep_cases().items():
        kept, words, _all, _a, _b = got[name]
        mask = tc.keep_mask(tags, allow)
        want = tc.bits_of(mask)
        have = np.array([int(w, 16) for w in words.split(",")], dtype=np.uint32)
        assert np.array_equal(have, want), name
        assert int(kept) == int(mask.sum()), name
        seen_kept += int(mask.sum())
        seen_dropped += int((~mask).sum())
    assert seen_kept > 1000 and seen_dropped > 1000       # the cases exercise both answers


def test_named_edges(got):
    cases = _keep_cases()
    assert got["edge_0_and_255_allowed"][0] == "5"
    assert got["edge_only_0"][0] == "1" and got["edge_only_0"][1] == "1"          # row 0 alone
    assert got["edge_only_255"][0] == "1" and got["edge_only_255"][1] == "2"      # row 1 alone
    assert got["all_but_one_bit"][0] == "3" and got["all_but_one_bit"][2] == "0"  # rows 1 and 3 carry 255 in field 3
    for n in (1, 33, 1000):
        assert got[f"n{n}_empty_field_2_k1"][0] == "0"
        assert got[f"n{n}_all_pass_k1"][0] == str(n)
        assert got[f"n{n}_first_row_k1"][0] == "1" and got[f"n{n}_last_row_k1"][0] == "1"
        tags = cases[f"n{n}_only_255_k1"][0]
        assert int(got[f"n{n}_only_255_k1"][0]) == int(((tags & 255) == 255).sum())


def test_all_pass_detection(got):
    for name, (_tags, allow, _k) in _keep_cases().items():
        assert got[name][2] == ("1" if bool(np.all(allow == 0xFFFFFFFF)) else "0"), name
    assert any(g[2] == "1" for g in got.values() if len(g) == 5)


def test_count_rule_is_plan_keep_on_the_bitset(got):
    answers = set()
    for name, (tags, allow, k) in _keep_cases().items():
        _kept, _words, _all, by_count, by_bits = got[name]
        assert by_count == by_bits, name
        kind, k_eff = (int(x) for x in by_count.split(":"))
        kept = int(tc.keep_mask(tags, allow).sum())
        want = EMPTY if kept == 0 else UNFILTERED if kept == len(tags) else FILTERED
        assert kind == want and k_eff == (min(k, kept) if want == FILTERED else k), name
        answers.add((kind, k_eff < k))
    assert answers == {(UNFILTERED, False), (EMPTY, False), (FILTERED, False), (FILTERED, True)}


def test_set_tags_range_rules(got):
    def ans(name):
        plan, why, first_local, new_tagged = got[name]
        return plan, why, int(first_local), int(new_tagged)
    assert ans("first_call_whole") == (WRITE, "", 0, 100)
    assert ans("first_call_part") == (WRITE, "", 0, 40)
    assert ans("overwrite_inside") == (WRITE, "", 10, 40)
    assert ans("overwrite_and_extend") == (WRITE, "", 30, 80)
    assert ans("extend_at_the_prefix_end") == (WRITE, "", 40, 100)
    assert ans("extend_to_exactly_len") == (WRITE, "", 40, 100)
    for name in ("gap", "gap_with_base"):
        assert ans(name) == (INVALID, "gap: first row past the tagged rows", 0, 40), name
    assert ans("gap_on_an_untagged_index") == (INVALID, "gap: first row past the tagged rows", 0, 0)
    assert ans("past_the_end") == (INVALID, "range past the end of the index", 0, 40)
    for name in ("past_the_end_inside_prefix", "past_the_end_huge_m"):
        assert ans(name) == (INVALID, "range past the end of the index", 0, 100), name
    assert ans("below_the_base") == (INVALID, "first row below this index", 0, 40)
    for name in ("nothing", "nothing_anywhere", "nothing_null"):
        assert ans(name) == (NOTHING, "", 0, 40), name
    assert ans("null_tags") == (INVALID, "null tags", 0, 40)
    assert ans("empty_index") == (INVALID, "range past the end of the index", 0, 0)


def test_prefix_after_a_removal(got):
    for name, (n, base, tagged, ids) in RM_CASES.items():
        plan, new_tagged, below = got[name]
        local = np.unique(np.asarray(ids, dtype=np.int64) - base)
        survivors = np.delete(np.arange(n), local)
        want = int((survivors < tagged).sum())
        assert plan == "1" and int(new_tagged) == want == int(below), name
    assert int(got["below_the_prefix"][1]) == 197 and int(got["above_the_prefix"][1]) == 200
    assert int(got["straddling"][1]) == 198 and int(got["duplicates"][1]) == 198
    assert int(got["whole_prefix"][1]) == 0 and int(got["everything"][1]) == 0


def test_tag_filter_bit_layout():
    """cqs_amd.tag_filter against the header's sentence: bit v of field f's set is bit v % 32 of word 8 f + v // 32; a
    field that is not named has all 256 bits set."""
    from cqs_amd import tag_filter
    assert tag_filter().dtype == np.uint32 and np.array_equal(tag_filter(), tc.ALL)
    for f in range(4):
        for v in (0, 1, 31, 32, 33, 63, 64, 200, 254, 255):
            args = [None] * 4
            args[f] = [v]
            a = tag_filter(*args)
            want = tc.ALL.copy()
            want[8 * f:8 * f + 8] = 0
            want[8 * f + v // 32] = 1 << (v % 32)
            assert np.array_equal(a, want), (f, v)
            tag = np.array([v << (8 * f)], dtype=np.uint32)
            assert tc.keep_mask(tag, a)[0] and not tc.keep_mask(tag ^ np.uint32(1 << (8 * f)), a)[0]
    a = tag_filter([0, 255], (3, 4, 5), set(), iter([7]))
    assert np.array_equal(a, tc.allow_of([0, 255], [3, 4, 5], [], [7]))
    assert not a[16:24].any()                               # an empty collection is an empty set, not "all"
    for bad in (256, -1):
        with pytest.raises(ValueError):
            tag_filter([bad])


def test_tag_symbols_without_a_device():
    """The library exports the entry points; a null handle is refused before any device work."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    tags = np.zeros(4, dtype=np.uint32)
    kept = C.c_uint64(7)
    cnt = C.c_uint32(9)
    assert lib.cqs_hip_index_set_tags(None, 0, tags.ctypes.data, 4) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_tagged_rows(None) == 0
    assert lib.cqs_hip_index_count_tagged(None, tc.ALL.ctypes.data, C.byref(kept)) == _lib.ERR_INVALID and kept.value == 7
    assert lib.cqs_hip_index_search_tagged(None, None, 1, 64, 5, tc.ALL.ctypes.data, 0, 0.0, None, None, None) == _lib.ERR_INVALID
    assert lib.cqs_hip_debug_index_tag_keep(None, tc.ALL.ctypes.data, None) == _lib.ERR_INVALID
    assert lib.cqs_hip_sparse_index_set_tags(None, 0, tags.ctypes.data, 4) == _lib.ERR_INVALID
    assert lib.cqs_hip_sparse_index_tagged_chunks(None) == 0
    assert lib.cqs_hip_sparse_index_search_tagged(None, None, None, 0, 5, tc.ALL.ctypes.data, None, None, C.byref(cnt)) == _lib.ERR_INVALID
    assert cnt.value == 9
