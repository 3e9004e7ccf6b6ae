"""The device-free rules of the host search path (cqs_amd/csrc/search_host.h) in a stand-alone program under ASAN + UBSan:
the argument plan step by step and in order, the kept-row count and k_eff, query staging, neighbours' clamp and
self-exclusion, the packed-key helpers and the last_error copy.  No GPU, no library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, EMPTY, RUN = "-1", "0", "1"
UNFILTERED, NOTHING, FILTERED = "0", "1", "2"


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("search_host") / "search_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "search_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    return {ln.split("|")[0]: ln.split("|")[1:] for ln in p.stdout.splitlines()}


@pytest.mark.parametrize("v", ["s", "f"])
def test_plan_search_steps_in_order(got, v):
    pre = "search_filtered: " if v == "f" else "search: "
    mismatch = "search: query dimension mismatch (empty result)"
    g = lambda name: got[f"{v}_{name}"]
    # 1. b == 0 answers before any pointer or argument is looked at
    assert g("b0_all_null") == [EMPTY, "-", ""] and g("b0_bad_everything") == [EMPTY, "-", ""]
    # 2. null inputs: refused with the counts as they were, whatever else is wrong
    for name in ("null_queries", "null_queries_k_over") + (("null_keep", "null_keep_k0") if v == "f" else ()):
        assert g(name) == [INVALID, "untouched", pre + "null buffer"], name
    assert g("null_counts") == [INVALID, "-", pre + "null buffer"]
    # 3. + 4. counts zeroed, then k == 0 / an empty index answer before the dimension, k, the outputs and the stride
    for name in ("k0_null_out", "k0_dim_mismatch", "k0_short_stride", "n0_k_over"):
        assert g(name) == [EMPTY, "zeroed", ""], name
    # 5. the mismatch is an empty answer with a message, before k, mode and the outputs
    assert g("dim_mismatch") == [EMPTY, "zeroed", mismatch] and g("dim_mismatch_k_over") == [EMPTY, "zeroed", mismatch]
    # 6. k
    assert g("k_max") == [RUN, "zeroed", ""]
    assert g("k_over") == [INVALID, "zeroed", pre + "k > max_k"] and g("k_over_bad_mode") == [INVALID, "zeroed", pre + "k > max_k"]
    # 7. mode
    assert g("pipeline_mode") == [RUN, "zeroed", ""]
    assert g("bad_mode") == [INVALID, "zeroed", pre + "bad mode"] and g("bad_mode_null_out") == [INVALID, "zeroed", pre + "bad mode"]
    # 8. outputs
    for name in ("null_rows", "null_scores", "null_out_short_stride"):
        assert g(name) == [INVALID, "zeroed", pre + "null output buffer"], name
    # 9. the stride, filtered variant only
    short = [INVALID, "zeroed", "search_filtered: bitset stride shorter than the index"] if v == "f" else [RUN, "zeroed", ""]
    assert g("short_stride") == short
    assert g("exact_stride") == [RUN, "zeroed", ""] and g("one_row") == [RUN, "zeroed", ""]


def test_kept_rows_and_k_eff(got):
    for n in (1, 31, 32, 33, 300):
        plan, k_eff, count, ref = got[f"keep_ones_{n}"]                       # garbage past n is not counted
        assert (plan, k_eff, int(count)) == (UNFILTERED, "20", n) and count == ref
        plan, k_eff, count, ref = got[f"keep_zero_{n}"]
        assert (plan, k_eff, count) == (NOTHING, "20", "0") and count == ref
        if n >= 4:
            plan, k_eff, count, ref = got[f"keep_three_{n}"]
            assert (plan, k_eff, count) == (FILTERED, "3", "3") and count == ref
    assert got["keep_null"] == [UNFILTERED, "20"]
    for name in ("shard_256_44", "shard_0_256", "shard_256_32"):
        assert got[name][0] == got[name][1] and int(got[name][0]) > 0, name
    assert got["shard_288_0"] == ["0"]


def test_query_staging(got):
    assert got["stage_finite"] == ["1", "copied", "1"] and got["stage_extremes"] == ["1", "copied", "1"]
    for kind in ("nan", "inf", "ninf"):
        for at in ("first", "last"):
            assert got[f"stage_{kind}_{at}"] == ["0", "zero", "0"], (kind, at)


def test_neighbors_clamp_and_self_exclusion(got):
    for limit in (0, 1, 5, 99, 100, 101, 1000, 0xFFFFFFFF):
        clamped = min(max(limit, 1), 100)                                   # limit.clamp(1, SIMILAR_LIMIT_MAX)
        for n in (0, 1, 2, 6, 101, 300):
            want_k = 0 if n <= 1 else min(clamped + 1, n)
            assert got[f"nk_{limit}_{n}"] == [str(clamped), str(want_k)], (limit, n)
    assert got["nk_0_300"] == ["1", "2"] and got["nk_1000_300"] == ["100", "101"] and got["nk_5_2"] == ["5", "2"]
    assert got["drop_first"] == ["3", "9:0.8,2:0.6,7:0.4"]
    assert got["drop_middle"] == ["3", "9:0.9,2:0.8,7:0.4"]
    assert got["drop_last"] == ["3", "9:0.9,2:0.8,7:0.7"]
    assert got["drop_absent"] == ["3", "9:0.9,2:0.8,7:0.7"]
    assert got["drop_tie"] == ["3", "3:0.5,8:0.5,6:0.25"]
    assert got["drop_short"] == ["1", "9:0.5"] and got["drop_none"] == ["0", ""]


def test_packed_keys(got):
    assert got["roundtrip"] == ["exact"] and got["key_order"] == ["1"]
    assert got["merge_k4"] == ["4", "2,5,9,1"]
    assert got["merge_k_large"] == ["5", "2,5,9,1,7"]
    assert got["merge_k0"] == ["0", ""] and got["merge_zero_counts"] == ["0", ""] and got["merge_no_lists"] == ["0", ""]
    assert got["merge_middle_empty"] == ["3", "5,9,7"]


def test_last_error_copy(got):
    text = "search: k > max_k"
    for cap in (1, 2, 17, 18, 100):
        m = min(len(text), cap - 1)
        assert got[f"error_cap_{cap}"] == [str(m), text[:m]], cap
