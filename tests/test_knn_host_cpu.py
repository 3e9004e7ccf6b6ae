"""The device-free rules of cqs_hip_index_knn_graph (cqs_amd/csrc/knn_host.h) in a stand-alone program under ASAN + UBSan:
the argument plan (every refusal, in its order; m == 0; the clamp of `limit` and k1), the cut of a range into the corpus's
fixed tiles, and the finish rule replayed on host arrays against cqs_search::drop_self.  Then the C ABI's
new symbol without a device.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOTHING, RUN = "-1", "0", "1"
NULL_HANDLE, NULL_OUT = "null handle", "null output buffer"
TOO_MANY, RANGE, SHARDED = "more than CQS_HIP_KNN_MAX_TARGETS targets in one call", "range not in this index", "not built for a row-sharded handle"
MAX_TARGETS = 65536


def _plan_cases():
    """name -> (present, sharded, row_base, len, max_block, first_row, m, limit, outputs)."""
    c = {}
    for base in (0, 5000):
        b = f"_base{base}"
        c["inside_one_tile" + b] = (1, 0, base, 1000, 1024, base + 10, 100, 15, 1)
        c["one_target" + b] = (1, 0, base, 1000, 1024, base + 255, 1, 15, 1)
        c["across_tiles" + b] = (1, 0, base, 1000, 1024, base + 200, 400, 15, 1)
        c["exact_tile" + b] = (1, 0, base, 1000, 1024, base + 256, 256, 15, 1)
        c["ends_in_ragged_tile" + b] = (1, 0, base, 700, 1024, base + 600, 100, 15, 1)
        c["whole_index" + b] = (1, 0, base, 700, 1024, base, 700, 15, 1)
        c["small_block" + b] = (1, 0, base, 450, 100, base + 50, 400, 15, 1)          # T = 100 < 256
        c["block_of_one" + b] = (1, 0, base, 5, 1, base + 1, 3, 15, 1)                # T = 1
        c["block_of_zero" + b] = (1, 0, base, 5, 0, base + 1, 3, 15, 1)               # (never below 1)
        c["most_targets" + b] = (1, 0, base, 70000, 1024, base + 100, MAX_TARGETS, 15, 1)
        # refusals, one at a time ...
        c["null_output" + b] = (1, 0, base, 1000, 1024, base, 10, 15, 0)
        c["too_many" + b] = (1, 0, base, 70000, 1024, base, MAX_TARGETS + 1, 15, 1)
        c["below_base" + b] = (1, 0, base, 1000, 1024, base - 1 if base else 2 ** 64 - 1, 2, 15, 1)
        c["starts_at_end" + b] = (1, 0, base, 1000, 1024, base + 1000, 1, 15, 1)
        c["ends_past_end" + b] = (1, 0, base, 1000, 1024, base + 990, 11, 15, 1)
        c["wraps" + b] = (1, 0, base, 1000, 1024, 2 ** 64 - 1, 2, 15, 1)
        c["empty_index" + b] = (1, 0, base, 0, 1024, base, 1, 15, 1)
        c["sharded" + b] = (1, 1, base, 1000, 0, base, 10, 15, 1)
        # ... and together: the first in the documented order answers
        c["null_output_first" + b] = (1, 1, base, 1000, 0, base + 2000, MAX_TARGETS + 1, 15, 0)
        c["too_many_before_range" + b] = (1, 1, base, 1000, 0, base + 2000, MAX_TARGETS + 1, 15, 1)
        c["range_before_sharded" + b] = (1, 1, base, 1000, 0, base + 995, 10, 15, 1)
        # m == 0 asks for nothing, whatever else is wrong
        c["nothing" + b] = (1, 0, base, 1000, 1024, base + 5, 0, 15, 1)
        c["nothing_null_out_of_range_sharded" + b] = (1, 1, base, 1000, 0, base + 9999, 0, 15, 0)
        c["nothing_empty_index" + b] = (1, 0, base, 0, 1024, base, 0, 15, 0)
        # the clamp and k1
        c["limit_0" + b] = (1, 0, base, 1000, 1024, base, 10, 0, 1)
        c["limit_1" + b] = (1, 0, base, 1000, 1024, base, 10, 1, 1)
        c["limit_100" + b] = (1, 0, base, 1000, 1024, base, 10, 100, 1)
        c["limit_101" + b] = (1, 0, base, 1000, 1024, base, 10, 101, 1)
        c["limit_max" + b] = (1, 0, base, 1000, 1024, base, 10, 2 ** 32 - 1, 1)
        c["fewer_rows_than_limit" + b] = (1, 0, base, 50, 1024, base, 50, 100, 1)
        c["len_1" + b] = (1, 0, base, 1, 1024, base, 1, 15, 1)
        c["len_2" + b] = (1, 0, base, 2, 1024, base, 2, 15, 1)
    c["null_handle"] = (0, 0, 0, 0, 0, 0, 10, 15, 1)
    c["null_handle_first"] = (0, 0, 0, 0, 0, 7, MAX_TARGETS + 1, 15, 0)
    c["null_handle_nothing"] = (0, 0, 0, 0, 0, 0, 0, 15, 0)
    rng = np.random.default_rng(31)
    for i in range(12):
        n = int(rng.integers(1, 3000))
        t = int(rng.choice([1, 7, 100, 255, 256, 1024]))
        first = int(rng.integers(0, n))
        c[f"random_{i}"] = (1, 0, 77, n, t, 77 + first, int(rng.integers(1, n - first + 1)), int(rng.integers(0, 130)), 1)
    return c


def _pack(score, row):
    b = int(np.float32(score).view(np.uint32))
    ok = (~b) & 0xFFFFFFFF if b >> 31 else b ^ 0x80000000
    return (ok << 32) | (0xFFFFFFFF - row)


def _finish_cases():
    """name -> (limit, target, [(score, row), ...] in the select's order: score desc, row asc)."""
    c = {}
    ten = [(1.0 - 0.125 * i, 40 + 3 * i) for i in range(10)]
    c["self_first"] = (9, 40, ten)
    c["self_in_the_middle"] = (9, 52, ten)
    c["self_last"] = (9, 67, ten)
    c["self_absent_full"] = (9, 5000, ten)                       # k1 = limit + 1 keys, none the target's: the last falls off
    c["few_rows_self_present"] = (15, 43, ten[:4])               # len - 1 < limit
    c["few_rows_self_absent"] = (15, 5000, ten[:4])              # (the target's own score was not finite)
    c["only_self"] = (15, 40, ten[:1])
    c["no_keys"] = (15, 40, [])
    c["limit_1_self_first"] = (1, 40, ten[:2])
    c["limit_1_self_second"] = (1, 43, ten[:2])
    c["negative_and_zero_scores"] = (5, 9, [(0.5, 3), (0.0, 9), (-0.0, 11), (-0.25, 2), (-1.5, 7), (-2.0 ** 100, 1)])
    # a run of rows equal to the target, longer than k1, all before it in row order: the target's own key is not among the
    # keys and every key is a duplicate's
    c["hidden_in_a_duplicate_run"] = (15, 900, [(1.0, 100 + i) for i in range(16)])
    # ... and one where the run ends just at the target: the target's key is the last one
    c["last_of_a_duplicate_run"] = (15, 115, [(1.0, 100 + i) for i in range(16)])
    big = [(2.0 - i / 128.0, 7 * i + 1) for i in range(101)]     # k1 = 101: both slots of a lane in use
    c["full_width_self_at_0"] = (100, 1, big)
    c["full_width_self_at_63"] = (100, 7 * 63 + 1, big)
    c["full_width_self_at_64"] = (100, 7 * 64 + 1, big)
    c["full_width_self_at_100"] = (100, 7 * 100 + 1, big)
    c["full_width_self_absent"] = (100, 3, big)
    c["row_near_2_32"] = (3, 0xFFFFFFFD, [(0.5, 0xFFFFFFFC), (0.5, 0xFFFFFFFD), (0.25, 0)])
    return c


PLANS = _plan_cases()
FINISHES = _finish_cases()


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("knn_host") / "knn_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "knn_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = [" ".join(["plan", name] + [str(v) for v in case]) for name, case in PLANS.items()]
    for name, (limit, target, pairs) in FINISHES.items():
        lines.append(" ".join(["finish", name, str(limit), str(target), str(len(pairs))] + [str(_pack(s, r)) for s, r in pairs]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    ints = lambda s: [int(x) for x in s.split(",") if x]
    plans, finishes = {}, {}
    for ln in p.stdout.splitlines():
        f = ln.split("|")
        if f[0] in PLANS:
            name, plan, why, lim, k1, tile, local_first, tiles, checks = f
            plans[name] = dict(plan=plan, why=why, limit=int(lim), k1=int(k1), tile=int(tile), local_first=int(local_first),
                               tiles=[tuple(int(x) for x in t.split(":")) for t in tiles.split(",") if t], checks=checks)
        else:
            name, count, rows, bits, ds, ds_rows, ds_bits = f
            finishes[name] = dict(count=int(count), rows=ints(rows), bits=ints(bits), ds=int(ds), ds_rows=ints(ds_rows), ds_bits=ints(ds_bits))
    assert set(plans) == set(PLANS) and set(finishes) == set(FINISHES)
    return plans, finishes


def _refused(g, why):
    return (g["plan"], g["why"], g["tiles"], g["limit"], g["k1"]) == (INVALID, why, [], 0, 0)


def test_every_refusal_and_their_order(got):
    plans, _ = got
    assert _refused(plans["null_handle"], NULL_HANDLE) and _refused(plans["null_handle_first"], NULL_HANDLE)
    assert _refused(plans["null_handle_nothing"], NULL_HANDLE)               # (before m == 0: there is nothing to ask)
    for base in (0, 5000):
        b = f"_base{base}"
        assert _refused(plans["null_output" + b], NULL_OUT)
        assert _refused(plans["too_many" + b], TOO_MANY)
        for stem in ("below_base", "starts_at_end", "ends_past_end", "wraps", "empty_index"):
            assert _refused(plans[stem + b], RANGE), stem + b
        assert _refused(plans["sharded" + b], SHARDED)
        assert _refused(plans["null_output_first" + b], NULL_OUT)
        assert _refused(plans["too_many_before_range" + b], TOO_MANY)
        assert _refused(plans["range_before_sharded" + b], RANGE)
        assert plans["most_targets" + b]["plan"] == RUN                        # the bound itself is allowed


def test_m_0_asks_for_nothing(got):
    plans, _ = got
    for base in (0, 5000):
        for stem in ("nothing", "nothing_null_out_of_range_sharded", "nothing_empty_index"):
            g = plans[f"{stem}_base{base}"]
            assert (g["plan"], g["why"], g["tiles"]) == (NOTHING, "", []), stem


def test_limit_clamp_and_k1(got):
    plans, _ = got
    for base in (0, 5000):
        b = f"_base{base}"
        lk = lambda name: (plans[name + b]["plan"], plans[name + b]["limit"], plans[name + b]["k1"])
        assert lk("limit_0") == (RUN, 1, 2) and lk("limit_1") == (RUN, 1, 2)
        assert lk("limit_100") == (RUN, 100, 101) and lk("limit_101") == (RUN, 100, 101) and lk("limit_max") == (RUN, 100, 101)
        assert lk("fewer_rows_than_limit") == (RUN, 100, 50)                   # k1 = len: out_counts <= len - 1
        assert lk("len_1") == (RUN, 15, 0)                                     # the only row has no neighbour: no device work
        assert plans["len_1" + b]["tiles"] == [(0, 1, 0, 1, 0)]
        assert lk("len_2") == (RUN, 15, 2) and plans["len_2" + b]["tiles"] == [(0, 2, 0, 2, 0)]


def test_tile_cuts(got):
    plans, _ = got
    for base in (0, 5000):
        b = f"_base{base}"
        t = lambda name: plans[name + b]["tiles"]
        assert t("inside_one_tile") == [(0, 256, 10, 100, 0)]
        assert t("one_target") == [(0, 256, 255, 1, 0)]
        assert t("across_tiles") == [(0, 256, 200, 56, 0), (256, 256, 0, 256, 56), (512, 256, 0, 88, 312)]
        assert t("exact_tile") == [(256, 256, 0, 256, 0)]
        assert t("ends_in_ragged_tile") == [(512, 188, 88, 100, 0)]
        assert t("whole_index") == [(0, 256, 0, 256, 0), (256, 256, 0, 256, 256), (512, 188, 0, 188, 512)]
        assert plans["small_block" + b]["tile"] == 100
        assert t("small_block") == [(0, 100, 50, 50, 0), (100, 100, 0, 100, 50), (200, 100, 0, 100, 150), (300, 100, 0, 100, 250),
                                    (400, 50, 0, 50, 350)]
        assert plans["block_of_one" + b]["tile"] == 1 and t("block_of_one") == [(1, 1, 0, 1, 0), (2, 1, 0, 1, 1), (3, 1, 0, 1, 2)]
        assert plans["block_of_zero" + b]["tile"] == 1
        assert plans["inside_one_tile" + b]["local_first"] == 10              # row_base taken off
        assert len(t("most_targets")) == 257 and plans["most_targets" + b]["tile"] == 256


def test_emitted_ranges_tile_every_request_exactly_once(got):
    plans, _ = got
    ran = 0
    for name, (_, _, base, n, max_block, first, m, _, _) in PLANS.items():
        g = plans[name]
        if g["plan"] != RUN:
            continue
        ran += 1
        assert g["checks"] == "1", name                                         # whole tiles, in range, once each, in order
        T = max(1, min(256, max_block))
        assert g["tile"] == T and g["local_first"] == first - base, name
        want = []                                                              # the same cut, written the other way round
        lo, hi = first - base, first - base + m
        for t0 in range(lo // T * T, hi, T):
            a, z = max(lo, t0), min(hi, t0 + T)
            want.append((t0, min(T, n - t0), a - t0, z - a, a - lo))
        assert g["tiles"] == want, name
        # the cut of a sub-range is the cut of the whole index restricted to it: how the caller cuts does not move a tile
        assert {(t[0], t[1]) for t in g["tiles"]} <= {(t0, min(T, n - t0)) for t0 in range(0, n, T)}, name
    assert ran == 2 * 18 + 12                                                  # (none of the plannable cases was refused)


def _expected_finish(limit, target, pairs):
    kept = [(s, r) for s, r in pairs if r != target][:limit]
    rows = [r for _, r in kept] + [0] * (limit - len(kept))
    bits = [int(np.float32(s).view(np.uint32)) for s, _ in kept] + [0] * (limit - len(kept))
    return len(kept), rows, bits


def test_finish_rule_is_drop_self(got):
    _, finishes = got
    for name, (limit, target, pairs) in FINISHES.items():
        g = finishes[name]
        count, rows, bits = _expected_finish(limit, target, pairs)
        assert (g["count"], g["rows"], g["bits"]) == (count, rows, bits), name     # every slot: zeros past the count
        assert g["ds"] == count and g["ds_rows"] == rows[:count] and g["ds_bits"] == bits[:count], name
    assert finishes["hidden_in_a_duplicate_run"]["rows"] == list(range(100, 115))      # the 16th duplicate fell off
    assert finishes["last_of_a_duplicate_run"]["rows"] == list(range(100, 115))
    assert finishes["self_absent_full"]["count"] == 9 and finishes["few_rows_self_absent"]["count"] == 4
    assert finishes["only_self"]["count"] == 0 and finishes["no_keys"]["count"] == 0
    assert finishes["negative_and_zero_scores"]["bits"][1] == 0x80000000                # -0.0 keeps its sign bit
    assert finishes["full_width_self_at_64"]["count"] == 100 and finishes["full_width_self_absent"]["rows"][-1] == 7 * 99 + 1


def test_knn_graph_symbol_without_a_device():
    """The library exports the entry point; a null handle is refused before any device work, the outputs untouched."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    rows = np.full((2, 15), 7, dtype=np.uint64)
    scores = np.full((2, 15), 7.0, dtype=np.float32)
    counts = np.full((2,), 7, dtype=np.uint32)
    assert lib.cqs_hip_index_knn_graph(None, 0, 2, 15, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data) == _lib.ERR_INVALID
    assert (rows == 7).all() and (scores == 7.0).all() and (counts == 7).all()
    assert lib.cqs_hip_index_knn_graph(None, 0, 0, 15, None, None, None) == _lib.ERR_INVALID
    assert _lib.KNN_MAX_TARGETS == MAX_TARGETS
