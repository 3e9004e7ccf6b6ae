"""The device-free plan of cqs_hip_index_update (cqs_amd/csrc/update_host.h) in a stand-alone program under ASAN + UBSan:
validation of the id list (range, duplicates, null arguments), the local rows, the staging order ascending by destination
row, the cut into passes, and the update itself replayed on a host array through a staging block of the largest pass's
size.  Then the C ABI's new symbols without a device.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOTHING, UPDATE = "-1", "0", "1"
OUT_OF_RANGE, TWICE = "row id not in this index", "row id named twice"


def _cases():
    """name -> (n, row_base, budget_rows, ids or None for a null list, m or None for len(ids), vectors present)."""
    c = {}
    n = 300
    for base in (0, 1000):
        b = f"_base{base}"
        c["unsorted" + b] = (n, base, 64, [base + i for i in (250, 3, 77, 4, 299, 0)], None, 1)
        c["below_base" + b] = (n, base, 64, [base + 5, base - 1 if base else 2 ** 63], None, 1)
        c["at_end" + b] = (n, base, 64, [base + 5, base + n], None, 1)
        c["dup_distance_1" + b] = (n, base, 64, [base + i for i in (9, 40, 40, 7, 100)], None, 1)
        c["dup_distance_m_minus_1" + b] = (n, base, 64, [base + i for i in (40, 9, 7, 100, 40)], None, 1)
        c["dup_and_out_of_range" + b] = (n, base, 64, [base + 3, base + 3, base + n], None, 1)
        c["more_entries_than_rows" + b] = (4, base, 64, [base + i for i in (0, 1, 2, 3, 1)], None, 1)
        c["nothing" + b] = (n, base, 64, [], None, 1)
        c["nothing_null" + b] = (n, base, 64, None, 0, 0)
        c["null_ids" + b] = (n, base, 64, None, 3, 1)
        c["null_vectors" + b] = (n, base, 64, [base + 1, base + 2], None, 0)
        c["first" + b] = (n, base, 64, [base], None, 1)
        c["last" + b] = (n, base, 64, [base + n - 1], None, 1)
        c["every_descending" + b] = (n, base, 64, [base + i for i in range(n - 1, -1, -1)], None, 1)
        c["every_second" + b] = (n, base, 37, [base + i for i in range(0, n, 2)], None, 1)
        block = [base + i for i in range(149, 99, -1)]
        c["block_budget_1" + b] = (n, base, 1, block, None, 1)
        c["block_budget_exact" + b] = (n, base, 50, block, None, 1)
        c["block_budget_minus" + b] = (n, base, 49, block, None, 1)       # a second pass of one entry
        c["block_budget_0" + b] = (n, base, 0, block, None, 1)            # (0 is cut as 1: the caller resolves its default)
        for seed in range(3):
            rng = np.random.default_rng(200 + seed)
            nn = int(rng.integers(200, 2000))
            ids = rng.choice(nn, size=max(1, int(nn * (0.05, 0.3, 1.0)[seed])), replace=False)
            for budget in (1, 37, 10 * nn):
                c[f"random_{seed}_{budget if budget < nn else 'all'}" + b] = (nn, base, budget, [base + int(i) for i in ids], None, 1)
    c["one_row_index"] = (1, 0, 64, [0], None, 1)
    c["empty_index"] = (0, 0, 64, [0], None, 1)
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("update_host") / "update_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "update_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = []
    for name, (n, base, budget, ids, m, vec) in CASES.items():
        toks = ["null"] if ids is None else [str(i) for i in ids]
        lines.append(" ".join([name, str(n), str(base), str(budget), str(len(ids) if m is None else m), str(vec)] + toks))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    ints = lambda s: [int(x) for x in s.split(",") if x]
    out = {}
    for ln in p.stdout.splitlines():
        name, plan, why, local, order, passes, values, shards, checks = ln.split("|")
        out[name] = dict(plan=plan, why=why, local=ints(local), order=ints(order),
                         passes=[tuple(int(x) for x in r.split(":")) for r in passes.split(",") if r],
                         values=np.array(ints(values), dtype=np.int64),
                         shards=[tuple(int(x) for x in r.split(":")) for r in shards.split(",") if r], checks=checks)
    assert set(out) == set(CASES)
    return out


def _untouched(g, name):
    assert (g["local"], g["order"], g["passes"]) == ([], [], []), name
    assert np.array_equal(g["values"], np.arange(CASES[name][0])), name


def test_ids_outside_the_index_are_refused_with_nothing_planned(got):
    for base in (0, 1000):
        for stem in ("below_base", "at_end", "dup_and_out_of_range"):
            name = f"{stem}_base{base}"
            assert (got[name]["plan"], got[name]["why"]) == (INVALID, OUT_OF_RANGE), name
            _untouched(got[name], name)
    assert (got["empty_index"]["plan"], got["empty_index"]["why"]) == (INVALID, OUT_OF_RANGE)


def test_an_id_named_twice_is_refused(got):
    for base in (0, 1000):
        for stem in ("dup_distance_1", "dup_distance_m_minus_1", "more_entries_than_rows"):
            name = f"{stem}_base{base}"
            assert (got[name]["plan"], got[name]["why"]) == (INVALID, TWICE), name
            _untouched(got[name], name)


def test_null_arguments_and_empty_lists(got):
    for base in (0, 1000):
        b = f"_base{base}"
        assert (got["null_ids" + b]["plan"], got["null_ids" + b]["why"]) == (INVALID, "null rows")
        assert (got["null_vectors" + b]["plan"], got["null_vectors" + b]["why"]) == (INVALID, "null vectors")
        for name in ("null_ids" + b, "null_vectors" + b, "nothing" + b, "nothing_null" + b):
            _untouched(got[name], name)
        assert got["nothing" + b]["plan"] == NOTHING and got["nothing_null" + b]["plan"] == NOTHING   # m == 0: whatever the pointers


def test_plans_stage_every_entry_once_in_ascending_destination_order(got):
    planned = 0
    for name, (n, base, budget, ids, _, _) in CASES.items():
        g = got[name]
        if g["plan"] != UPDATE:
            continue
        planned += 1
        assert g["checks"] == "1", name                                 # budget, tiling, once each, ascending, shard ranges
        local = np.asarray(ids, dtype=np.int64) - base
        assert g["local"] == local.tolist(), name                       # list order, row_base taken off
        assert sorted(g["order"]) == list(range(len(ids))), name        # a permutation of the list positions ...
        assert np.array_equal(local[g["order"]], np.sort(local)), name  # ... ascending by destination row
        want = np.arange(n)
        want[local] = 1000000 + np.arange(len(ids))                     # vectors[i] replaces row rows[i]
        assert np.array_equal(g["values"], want), name
        eff = max(budget, 1)
        assert all(1 <= cnt <= eff for _, cnt in g["passes"]), name
        assert len(g["passes"]) == -(-len(ids) // eff), name            # every pass but the last is full
        first = 0
        for f, cnt in g["passes"]:
            assert f == first, name
            first += cnt
        assert first == len(ids), name
        for s, (f, cnt) in enumerate(g["shards"]):                      # what a row-sharded handle hands each shard
            lo, hi = n * s // 3, n * (s + 1) // 3
            assert cnt == int(((local >= lo) & (local < hi)).sum()), (name, s)
    assert planned == 37                                                # (none of the plannable cases was refused)


def test_pass_cutting(got):
    for base in (0, 1000):
        b = f"_base{base}"
        assert got["block_budget_1" + b]["passes"] == [(i, 1) for i in range(50)]
        assert got["block_budget_0" + b]["passes"] == [(i, 1) for i in range(50)]
        assert got["block_budget_exact" + b]["passes"] == [(0, 50)]
        assert got["block_budget_minus" + b]["passes"] == [(0, 49), (49, 1)]
        assert got["block_budget_1" + b]["order"] == list(range(49, -1, -1))          # the block was named descending
        assert got["every_second" + b]["passes"] == [(0, 37), (37, 37), (74, 37), (111, 37), (148, 2)]
        assert got["first" + b]["passes"] == [(0, 1)] and got["last" + b]["local"] == [299]
    assert got["one_row_index"]["plan"] == UPDATE and got["one_row_index"]["values"].tolist() == [1000000]


def test_update_symbols_without_a_device():
    """The library exports the entry point and its test hook; a null handle is refused before any device work."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    rows = np.array([1, 2], dtype=np.uint64)
    vec = np.zeros((2, 4), dtype=np.float32)
    updated = C.c_uint64(7)
    assert lib.cqs_hip_index_update(None, rows.ctypes.data, vec.ctypes.data, 2, C.byref(updated)) == _lib.ERR_INVALID
    assert updated.value == 7
    lib.cqs_hip_debug_index_update_budget(None, 5)
