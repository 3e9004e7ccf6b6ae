"""The device-free plan of cqs_hip_index_remove (cqs_amd/csrc/remove_host.h) in a stand-alone program under ASAN + UBSan:
validation, sort and dedupe of the id list, the surviving runs, the cut into passes, the overlap invariant the in-place
compaction rests on, and the compaction itself replayed on a host array against `np.delete`.  Then the
C ABI's new symbol without a device.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOTHING, REMOVE = "-1", "0", "1"


def _cases():
    """name -> (n, row_base, budget_rows, ids or None for a null list, m)."""
    c = {}
    n = 300
    c["unsorted_dups"] = (n, 0, 64, [250, 3, 3, 77, 250, 4, 299, 3], None)
    c["unsorted_dups_base"] = (n, 1000, 64, [1250, 1003, 1003, 1077, 1250, 1004, 1299, 1003], None)
    c["below_base"] = (n, 1000, 64, [1005, 999], None)
    c["at_end"] = (n, 1000, 64, [1005, 1300], None)
    c["at_end_base0"] = (n, 0, 64, [300], None)
    c["null_ids"] = (n, 0, 64, None, 3)
    c["nothing"] = (n, 0, 64, [], None)
    c["nothing_null"] = (n, 0, 64, None, 0)
    c["first"] = (n, 0, 64, [0], None)
    c["last"] = (n, 0, 64, [n - 1], None)
    c["every"] = (n, 0, 64, list(range(n)), None)
    c["every_second"] = (n, 0, 64, list(range(0, n, 2)), None)
    c["every_second_odd"] = (n, 7, 64, list(range(8, n + 7, 2)), None)
    c["one_row_index"] = (1, 0, 64, [0], None)
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        nn = int(rng.integers(200, 2000))
        ids = rng.choice(nn, size=int(nn * (0.05, 0.3, 0.6, 0.95)[seed]), replace=False)
        for budget in (1, 37, 10 * nn):
            c[f"random_{seed}_{budget if budget < nn else 'all'}"] = (nn, 0, budget, [int(i) for i in ids], None)
    # one contiguous block out of the middle: a single run of 150 rows behind it
    block = list(range(100, 150))
    c["block_budget_1"] = (n, 0, 1, block, None)
    c["block_budget_run"] = (n, 0, 150, block, None)          # exactly the one run
    c["block_budget_run_minus"] = (n, 0, 149, block, None)    # the run cut one row short: a second pass of one row
    c["block_budget_all"] = (n, 0, 10 * n, block, None)
    c["two_runs_straddle"] = (n, 0, 100, [10, 200], None)     # runs of 189 and 99 rows: passes cut both
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("remove_host") / "remove_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "remove_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = []
    for name, (n, base, budget, ids, m) in CASES.items():
        toks = ["null"] if ids is None else [str(i) for i in ids]
        lines.append(" ".join([name, str(n), str(base), str(budget), str(len(ids) if m is None else m)] + toks))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    out = {}
    for ln in p.stdout.splitlines():
        name, plan, why, removed, runs, passes, values, checks = ln.split("|")
        out[name] = dict(plan=plan, why=why, removed=int(removed),
                         runs=[tuple(int(x) for x in r.split(":")) for r in runs.split(",") if r],
                         passes=[tuple(int(x) for x in r.split(":")) for r in passes.split(",") if r],
                         values=np.array([int(x) for x in values.split(",") if x], dtype=np.int64), checks=checks)
    assert set(out) == set(CASES)
    return out


def _expected(name):
    n, base, _, ids, _ = CASES[name]
    local = np.unique(np.asarray(ids, dtype=np.int64) - base)
    return local, np.delete(np.arange(n), local)


def test_unsorted_ids_with_duplicates(got):
    for name in ("unsorted_dups", "unsorted_dups_base"):
        g = got[name]
        assert g["plan"] == REMOVE and g["removed"] == 5 and g["checks"] == "1"
        # rows 3, 4, 77, 250, 299 go: runs (src, dst, rows) start after the first removed row, local rows either way
        assert g["runs"] == [(5, 3, 72), (78, 75, 172), (251, 247, 48)]
        assert np.array_equal(g["values"], _expected(name)[1])


def test_ids_outside_the_index_are_refused_with_nothing_planned(got):
    for name in ("below_base", "at_end", "at_end_base0"):
        g = got[name]
        assert (g["plan"], g["why"], g["removed"], g["runs"], g["passes"]) == (INVALID, "row id not in this index", 0, [], []), name
        assert np.array_equal(g["values"], np.arange(CASES[name][0]))
    g = got["null_ids"]
    assert (g["plan"], g["why"], g["removed"], g["runs"]) == (INVALID, "null rows", 0, [])


def test_edge_patterns(got):
    for name in ("nothing", "nothing_null"):
        assert (got[name]["plan"], got[name]["removed"], got[name]["runs"]) == (NOTHING, 0, [])
        assert np.array_equal(got[name]["values"], np.arange(300))
    assert got["first"]["runs"] == [(1, 0, 299)]
    assert got["last"]["runs"] == [] and got["last"]["passes"] == [] and got["last"]["removed"] == 1
    assert got["every"]["runs"] == [] and got["every"]["removed"] == 300 and len(got["every"]["values"]) == 0
    assert got["one_row_index"]["runs"] == [] and len(got["one_row_index"]["values"]) == 0
    assert got["every_second"]["runs"] == [(2 * i + 1, i, 1) for i in range(150)]
    for name in ("first", "last", "every", "every_second", "every_second_odd", "one_row_index"):
        g = got[name]
        assert g["plan"] == REMOVE and g["checks"] == "1", name
        assert np.array_equal(g["values"], _expected(name)[1]), name


def test_runs_reproduce_np_delete(got):
    for name in CASES:
        if not name.startswith("random_"):
            continue
        g = got[name]
        local, want = _expected(name)
        assert g["plan"] == REMOVE and g["removed"] == len(local) and g["checks"] == "1", name
        assert np.array_equal(g["values"], want), name
        # the runs themselves: consecutive destinations from the first removed row, sources = the survivors above it
        src = np.concatenate([np.arange(s, s + r) for s, _, r in g["runs"]]) if g["runs"] else np.zeros(0, np.int64)
        dst = np.concatenate([np.arange(d, d + r) for _, d, r in g["runs"]]) if g["runs"] else np.zeros(0, np.int64)
        assert np.array_equal(src, want[want > local[0]]), name
        assert np.array_equal(dst, np.arange(local[0], local[0] + len(src))), name
        assert all(s > d for s, d, _ in g["runs"]), name


def test_pass_cutting(got):
    assert got["block_budget_1"]["passes"] == [(100 + i, 1, 0, 1) for i in range(150)]
    assert got["block_budget_run"]["passes"] == [(100, 150, 0, 1)]
    assert got["block_budget_run_minus"]["passes"] == [(100, 149, 0, 1), (249, 1, 0, 1)]
    assert got["block_budget_all"]["passes"] == [(100, 150, 0, 1)]
    # runs (11, 10, 189) and (201, 199, 99): the second pass straddles them, the third starts inside the second run
    assert got["two_runs_straddle"]["runs"] == [(11, 10, 189), (201, 199, 99)]
    assert got["two_runs_straddle"]["passes"] == [(10, 100, 0, 1), (110, 100, 0, 2), (210, 88, 1, 1)]
    for name, (n, _, budget, _, _) in CASES.items():
        g = got[name]
        if g["plan"] != REMOVE:
            continue
        assert g["checks"] == "1", name                       # budget, tiling, overlap invariant, untouched prefix
        moved = sum(r for _, _, r in g["runs"])
        assert sum(r for _, r, _, _ in g["passes"]) == moved, name
        assert len(g["passes"]) == -(-moved // budget), name  # every pass but the last is full
        assert np.array_equal(g["values"], _expected(name)[1]), name


def test_remove_symbol_without_a_device():
    """The library exports the entry point; a null handle is refused before any device work."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    rows = np.array([1, 2], dtype=np.uint64)
    removed = C.c_uint64(7)
    assert lib.cqs_hip_index_remove(None, rows.ctypes.data, 2, C.byref(removed)) == _lib.ERR_INVALID
    assert removed.value == 7
    lib.cqs_hip_debug_index_remove_budget(None, 5)
