"""The device-free part of cqs_hip_index_diff (cqs_amd/csrc/diff_host.h) in a stand-alone program under ASAN + UBSan: the
argument plan (every refusal alone, and together for their order; m == 0; row_base 0 and 5000; rows at both ends of each
index), the cut into passes and the concatenation of their lists, one pair's arithmetic against numpy f64, the compaction
against a plain filter; the two-handle lock in a second build under TSan.  Then the C ABI's new symbol without a device,
the host logic of HipIndex.semantic_diff / detect_drift over a fake diff_rows, and tests/diff_cases.py's expected values
against the oracle.  No GPU."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diff_cases as dc  # noqa: E402

INVALID, NOTHING, RUN = "-1", "0", "1"
DRIVER = os.path.join(ROOT, "tests", "diff_host_driver.cpp")


def bits(x):
    return int(np.float32(x).view(np.uint32))


def side(present=1, sharded=0, device=0, dim=768, base=0, length=1000):
    return (present, sharded, device, dim, base, length)


def _plan_cases():
    """name -> (side a, side b, m, threshold, (rows_a, rows_b, counts, mod_pairs, mod_sims present), rows_a, rows_b, plan, why)."""
    c = {}
    all_out = (1, 1, 1, 1, 1)
    for base in (0, 5000):
        t = f"_base{base}"
        a, b = side(base=base, length=1000), side(base=base + 7, length=300)
        lo_a, hi_a, lo_b, hi_b = base, base + 999, base + 7, base + 306
        c["ends_of_both" + t] = (a, b, 4, 0.5, all_out, [lo_a, hi_a, lo_a, hi_a], [lo_b, hi_b, hi_b, lo_b], RUN, "")
        c["a_row_repeats" + t] = (a, b, 3, 0.5, all_out, [lo_a + 5] * 3, [lo_b, lo_b + 1, lo_b], RUN, "")
        c["same_handle" + t] = (a, a, 2, 0.5, all_out, [lo_a, hi_a], [hi_a, lo_a], RUN, "")
        c["no_lists" + t] = (a, b, 1, 0.5, (1, 1, 1, 0, 0), [lo_a], [lo_b], RUN, "")
        c["inf_threshold" + t] = (a, b, 1, np.inf, all_out, [lo_a], [lo_b], RUN, "")
        # every refusal alone
        c["null_a" + t] = (side(present=0), b, 1, 0.5, all_out, [lo_a], [lo_b], INVALID, "null handle")
        c["null_b" + t] = (a, side(present=0), 1, 0.5, all_out, [lo_a], [lo_b], INVALID, "null handle")
        c["null_rows_a" + t] = (a, b, 1, 0.5, (0, 1, 1, 1, 1), [lo_a], [lo_b], INVALID, "null rows_a")
        c["null_rows_b" + t] = (a, b, 1, 0.5, (1, 0, 1, 1, 1), [lo_a], [lo_b], INVALID, "null rows_b")
        c["null_counts" + t] = (a, b, 1, 0.5, (1, 1, 0, 1, 1), [lo_a], [lo_b], INVALID, "null out_counts")
        c["pairs_without_sims" + t] = (a, b, 1, 0.5, (1, 1, 1, 1, 0), [lo_a], [lo_b], INVALID, "out_mod_pairs and out_mod_sims go together")
        c["sims_without_pairs" + t] = (a, b, 1, 0.5, (1, 1, 1, 0, 1), [lo_a], [lo_b], INVALID, "out_mod_pairs and out_mod_sims go together")
        c["nan_threshold" + t] = (a, b, 1, np.nan, all_out, [lo_a], [lo_b], INVALID, "threshold is NaN")
        c["sharded_a" + t] = (side(sharded=1, base=base, length=0), b, 1, 0.5, all_out, [lo_a], [lo_b], INVALID, "not built for a row-sharded handle")
        c["sharded_b" + t] = (a, side(sharded=1, base=base, length=0), 1, 0.5, all_out, [lo_a], [lo_b], INVALID, "not built for a row-sharded handle")
        c["other_device" + t] = (a, side(device=1, base=base + 7, length=300), 1, 0.5, all_out, [lo_a], [lo_b], INVALID, "the two handles are on different devices")
        c["other_dim" + t] = (a, side(dim=252, base=base + 7, length=300), 1, 0.5, all_out, [lo_a], [lo_b], INVALID, "the two handles differ in dim")
        c["a_past_end" + t] = (a, b, 3, 0.5, all_out, [lo_a, hi_a + 1, lo_a], [lo_b, lo_b, lo_b], INVALID, "pair 1: row of a not in its index")
        c["b_past_end" + t] = (a, b, 3, 0.5, all_out, [lo_a, lo_a, hi_a], [lo_b, lo_b, hi_b + 1], INVALID, "pair 2: row of b not in its index")
        c["b_below_base" + t] = (a, b, 2, 0.5, all_out, [lo_a, lo_a], [lo_b - 1, lo_b], INVALID, "pair 0: row of b not in its index")
        c["a_wraps" + t] = (a, b, 1, 0.5, all_out, [2 ** 64 - 1], [lo_b], INVALID, "pair 0: row of a not in its index")
        c["first_bad_pair_a_before_b" + t] = (a, b, 3, 0.5, all_out, [lo_a, hi_a + 5, hi_a + 6], [hi_b + 9, hi_b + 9, lo_b], INVALID,
                                             "pair 0: row of b not in its index")
        c["both_sides_of_one_pair" + t] = (a, b, 2, 0.5, all_out, [lo_a, hi_a + 5], [lo_b, hi_b + 9], INVALID, "pair 1: row of a not in its index")
        c["empty_index" + t] = (side(base=base, length=0), b, 1, 0.5, all_out, [lo_a], [lo_b], INVALID, "pair 0: row of a not in its index")
        # ... and together: the first in the documented order answers.  Each case has everything wrong that comes after.
        wrong_b = side(sharded=1, device=1, dim=252, base=base + 7, length=0)
        c["order_1_null_handle" + t] = (side(present=0), wrong_b, 2, np.nan, (0, 0, 0, 1, 0), [9999999, 0], [0, 0], INVALID, "null handle")
        c["order_2_nothing" + t] = (a, wrong_b, 0, np.nan, (0, 0, 0, 1, 0), [], [], NOTHING, "")
        c["order_3_null_rows_a" + t] = (a, wrong_b, 2, np.nan, (0, 0, 0, 1, 0), [9999999, 0], [0, 0], INVALID, "null rows_a")
        c["order_3_null_rows_b" + t] = (a, wrong_b, 2, np.nan, (1, 0, 0, 1, 0), [9999999, 0], [0, 0], INVALID, "null rows_b")
        c["order_3_null_counts" + t] = (a, wrong_b, 2, np.nan, (1, 1, 0, 1, 0), [9999999, 0], [0, 0], INVALID, "null out_counts")
        c["order_4_lists" + t] = (a, wrong_b, 2, np.nan, (1, 1, 1, 1, 0), [9999999, 0], [0, 0], INVALID, "out_mod_pairs and out_mod_sims go together")
        c["order_5_nan" + t] = (a, wrong_b, 2, np.nan, all_out, [9999999, 0], [0, 0], INVALID, "threshold is NaN")
        c["order_6_sharded" + t] = (a, wrong_b, 2, 0.5, all_out, [9999999, 0], [0, 0], INVALID, "not built for a row-sharded handle")
        c["order_7_device" + t] = (a, side(device=1, dim=252, base=base + 7, length=0), 2, 0.5, all_out, [9999999, 0], [0, 0], INVALID,
                                   "the two handles are on different devices")
        c["order_8_dim" + t] = (a, side(dim=252, base=base + 7, length=0), 2, 0.5, all_out, [9999999, 0], [0, 0], INVALID, "the two handles differ in dim")
        # m == 0 asks for nothing, with or without outputs
        c["nothing" + t] = (a, b, 0, 0.5, all_out, [], [], NOTHING, "")
        c["nothing_no_outputs" + t] = (a, b, 0, 0.5, (0, 0, 0, 0, 0), [], [], NOTHING, "")
    return c


PLANS = _plan_cases()
PASSES = {"one_pair": (1, 1), "budget_1": (7, 1), "budget_64": (1000, 64), "budget_100": (1000, 100), "exact": (128, 64),
          "one_pass": (1000, 2 ** 20), "budget_0_is_1": (3, 0), "nothing": (0, 64), "more_than_a_pass": (2 ** 20 + 1, 2 ** 20)}
BUDGETS = (1, 64, 100, 2 ** 20)


def _write_call(path, a, b, ra, rb, base_a, base_b):
    with open(path, "wb") as f:
        f.write(struct.pack("<6Q", a.shape[0], b.shape[0], a.shape[1], len(ra), base_a, base_b))
        f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.ascontiguousarray(b, np.float32).tobytes())
        f.write((ra + np.uint64(base_a)).astype(np.uint64).tobytes())
        f.write((rb + np.uint64(base_b)).astype(np.uint64).tobytes())


def _random_call(dim, seed, unit):
    """(A, B, rows_a, rows_b): B = A perturbed, so that the cosines spread below 1; a zero row and a NaN row among them."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((40, dim)).astype(np.float32)
    b = (a[rng.permutation(40)] + rng.standard_normal((40, dim)).astype(np.float32) * np.float32(0.7)).astype(np.float32)
    if unit:
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
    else:
        a *= np.float32(37.5)
    b[3] = 0
    a[5, dim - 1] = np.nan
    ra, rb = rng.integers(0, 40, 150).astype(np.uint64), rng.integers(0, 40, 150).astype(np.uint64)
    ra[:4], rb[:4] = [0, 5, 5, 0], [3, 1, 3, 39]
    return a, b, ra, rb


def _numpy_sims(a, b, ra, rb):
    """The pair values computed here with numpy f64: (sims f32, undefined) as diff.rs:191-202 defines them."""
    x, y = a[ra.astype(np.int64)].astype(np.float64), b[rb.astype(np.int64)].astype(np.float64)
    with np.errstate(all="ignore"):
        dot, na, nb = np.einsum("ij,ij->i", x, y), np.einsum("ij,ij->i", x, x), np.einsum("ij,ij->i", y, y)
        denom = np.sqrt(na) * np.sqrt(nb)
        r = (dot / denom).astype(np.float32)
    undefined = (denom == 0.0) | ~np.isfinite(r)
    return np.where(undefined, np.float32(0.0), r).astype(np.float32), undefined


def _adjacent_or_equal(got_bits, want):
    """Each got f32 (as bits) is `want` or one of its two neighbours."""
    got = np.asarray(got_bits, np.uint32).view(np.float32)
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    """name -> (A, B, rows_a, rows_b, base_a, base_b, threshold, file)."""
    d = tmp_path_factory.mktemp("diff_calls")
    out = {}
    for dim in (4, 252, 768):
        a, b = dc.corpora(dim)
        ra, rb = dc.pairs(257)
        sims, undefined = dc.expected_sims(a, b, ra, rb)
        for ti, thr in enumerate(dc.thresholds(sims, undefined)):
            out[f"exact_{dim}_{ti}"] = (a, b, ra, rb, 0, 5000, thr)
    for dim, unit in ((768, True), (252, False), (4096, False), (4, True)):
        a, b, ra, rb = _random_call(dim, 9 + dim, unit)
        out[f"random_{dim}"] = (a, b, ra, rb, 5000, 0, np.float32(0.35))
    for name, v in list(out.items()):
        path = str(d / (name + ".bin"))
        _write_call(path, v[0], v[1], v[2], v[3], v[4], v[5])
        out[name] = v + (path,)
    return out


@pytest.fixture(scope="module")
def got(tmp_path_factory, calls):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("diff_host") / "diff_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", str(exe), "-pthread"], check=True, capture_output=True)
    lines = []
    for name, (a, b, m, thr, flags, ra, rb, _, _) in PLANS.items():
        lines.append(" ".join(str(v) for v in ("plan", name) + a + b + (m, bits(thr)) + flags + tuple(ra) + tuple(rb)))
    for name, (m, budget) in PASSES.items():
        lines.append(f"passes {name} {m} {budget}")
    for name, v in calls.items():
        for budget in BUDGETS:
            lines.append(f"run {name}@{budget} {v[7]} {budget} {bits(v[6])}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe), "cases"], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    ints = lambda s: [int(x) for x in s.split(",") if x]
    plans, passes, runs = {}, {}, {}
    for ln in p.stdout.splitlines():
        f = ln.split("|")
        if f[0] in PLANS:
            plans[f[0]] = (f[1], f[2])
        elif f[0] in PASSES:
            passes[f[0]] = [tuple(int(x) for x in t.split(":")) for t in f[1].split(",") if t]
        else:
            assert len(f) == 6, ln[:200]
            runs[f[0]] = dict(sims=ints(f[1]), cls=ints(f[2]), mod_pairs=ints(f[3]), mod_sims=ints(f[4]), counts=ints(f[5]))
    assert set(plans) == set(PLANS) and set(passes) == set(PASSES) and len(runs) == len(calls) * len(BUDGETS)
    return plans, passes, runs


def test_every_refusal_alone_and_their_order(got):
    plans, _, _ = got
    for name, case in PLANS.items():
        assert plans[name] == (case[7], case[8]), name
    assert sum(1 for c in PLANS.values() if c[7] == INVALID) >= 2 * 28 and sum(1 for c in PLANS.values() if c[7] == RUN) == 2 * 5


def test_pass_cuts(got):
    _, passes, _ = got
    assert passes["one_pair"] == [(0, 1)] and passes["budget_1"] == [(i, 1) for i in range(7)]
    assert passes["budget_64"] == [(64 * i, 64) for i in range(15)] + [(960, 40)]
    assert passes["budget_100"] == [(100 * i, 100) for i in range(10)]
    assert passes["exact"] == [(0, 64), (64, 64)] and passes["one_pass"] == [(0, 1000)]
    assert passes["budget_0_is_1"] == [(0, 1), (1, 1), (2, 1)] and passes["nothing"] == []
    assert passes["more_than_a_pass"] == [(0, 2 ** 20), (2 ** 20, 1)]


def test_passes_concatenate_to_the_one_pass_answer(got, calls):
    _, _, runs = got
    for name in calls:
        whole = runs[f"{name}@{2 ** 20}"]
        for budget in BUDGETS:
            assert runs[f"{name}@{budget}"] == whole, (name, budget)           # sims, classes, both lists, counts


def test_exact_pairs_are_the_expected_bits(got, calls):
    _, _, runs = got
    seen_thresholds = set()
    for name, (a, b, ra, rb, _, _, thr, _) in calls.items():
        if not name.startswith("exact_"):
            continue
        g = runs[f"{name}@64"]
        sims, undefined = dc.expected_sims(a, b, ra, rb)
        mod, mod_sims, counts = dc.expected_answer(sims, undefined, thr)
        assert g["sims"] == [bits(s) for s in sims], name
        assert g["mod_pairs"] == list(mod) and g["mod_sims"] == [bits(s) for s in mod_sims] and g["counts"] == counts, name
        assert [c >> 1 for c in g["cls"]] == [int(u) for u in undefined], name
        assert counts[2] >= 1 and g["sims"][0] == 0                             # the all-zero pair: undefined, 0.0
        seen_thresholds.add(float(thr))
        hit = set(np.flatnonzero(sims == thr))                                  # a pair whose sim equals the threshold is unchanged
        assert not hit & set(int(x) for x in g["mod_pairs"]), name
        if name.endswith("_2"):                                                 # the threshold taken from a pair's sim
            assert hit, name
    assert {-1.0, 0.0, 1.0, float("inf"), float("-inf")} <= seen_thresholds


def test_random_pairs_against_numpy_f64(got, calls):
    _, _, runs = got
    for name, (a, b, ra, rb, _, _, thr, _) in calls.items():
        if not name.startswith("random_"):
            continue
        g = runs[f"{name}@100"]
        want, undefined = _numpy_sims(a, b, ra, rb)
        assert _adjacent_or_equal(g["sims"], want).all(), name
        assert [c >> 1 for c in g["cls"]] == [int(u) for u in undefined], name
        assert undefined[:3].all() and not undefined[3] and g["sims"][:3] == [0, 0, 0], name   # zero row, NaN row: undefined, 0.0
        assert g["counts"][2] == int(undefined.sum()) and g["counts"][0] + g["counts"][1] == len(ra), name
        # the compaction against a plain filter over the driver's own sims and classes
        sims = np.asarray(g["sims"], np.uint32).view(np.float32)
        mod = [i for i in range(len(ra)) if sims[i] < thr]
        assert g["mod_pairs"] == mod and g["mod_sims"] == [g["sims"][i] for i in mod], name
        assert [c & 1 for c in g["cls"]] == [int(i in set(mod)) for i in range(len(ra))], name
        assert 0 < len(mod) < len(ra), name


def test_swapped_pair_gives_the_same_bits(tmp_path, got, calls):
    """sim(x, y) and sim(y, x): the same call with the two sides exchanged."""
    _, _, runs = got
    a, b, ra, rb, base_a, base_b, thr, _ = calls["random_252"]
    path = str(tmp_path / "swapped.bin")
    _write_call(path, b, a, rb, ra, base_b, base_a)
    cxx = shutil.which("g++")
    exe = tmp_path / "drv"
    subprocess.run([cxx, "-std=c++17", "-O1", DRIVER, "-o", str(exe), "-pthread"], check=True, capture_output=True)
    p = subprocess.run([str(exe), "cases"], input=f"run swapped {path} 64 {bits(thr)}\n", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.split("|")[1] == ",".join(str(s) for s in runs["random_252@64"]["sims"])


def test_lock_helper_under_tsan(tmp_path):
    """(x, y), (y, x) and (x, x) through PairLock from three threads: a lock-order inversion or an unprotected counter is
    ThreadSanitizer's to report."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "diff_host_driver_tsan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=thread", DRIVER, "-o", str(exe), "-pthread"],
                   check=True, capture_output=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66:detect_deadlocks=1:second_deadlock_stack=1")
    p = subprocess.run([str(exe), "lock", "4000"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["12000", "8000"], (p.returncode, p.stdout, p.stderr[-1500:])


def test_diff_symbol_without_a_device():
    """The library exports the entry point; a null handle is refused before any device work, the outputs untouched."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    rows = np.arange(4, dtype=np.uint64)
    sims = np.full((4,), 7.0, dtype=np.float32)
    mod_pairs = np.full((4,), 7, dtype=np.uint64)
    mod_sims = np.full((4,), 7.0, dtype=np.float32)
    counts = np.full((3,), 7, dtype=np.uint64)
    ptrs = (sims.ctypes.data, mod_pairs.ctypes.data, mod_sims.ctypes.data, counts.ctypes.data)
    assert lib.cqs_hip_index_diff(None, rows.ctypes.data, None, rows.ctypes.data, 4, 0.5, *ptrs) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_diff(None, rows.ctypes.data, None, rows.ctypes.data, 0, 0.5, *ptrs) == _lib.ERR_INVALID   # (before m == 0)
    assert (sims == 7.0).all() and (mod_pairs == 7).all() and (mod_sims == 7.0).all() and (counts == 7).all()
    lib.cqs_hip_debug_index_diff_budget(None, 5)


# ---- HipIndex.semantic_diff / detect_drift: matching and sorting on the host, over a fake diff_rows -------------------
class _FakeIndex:
    """What semantic_diff needs of a HipIndex, with diff_rows done by numpy over the oracle's values."""

    def __init__(self, ids, rows, base):
        self.id_map, self.rows, self.base, self.calls = ids, np.asarray(rows, np.float32), base, []

    def _all_ids(self):
        return self.id_map

    def _row_base(self):
        return self.base

    def diff_rows(self, other, rows_a, rows_b, threshold, want_sims=False):
        from oracle import oracle
        self.calls.append((list(map(int, rows_a)), list(map(int, rows_b))))
        sims, undefined = [], 0
        for ra, rb in zip(rows_a, rows_b):
            s = oracle.full_cosine_similarity(self.rows[int(ra) - self.base], other.rows[int(rb) - other.base])
            undefined += s is None
            sims.append(np.float32(0.0 if s is None else s))
        sims = np.asarray(sims, np.float32)
        mod = np.flatnonzero(sims < np.float32(threshold)).astype(np.uint64)
        return mod, sims[mod.astype(np.int64)], np.asarray([len(mod), len(sims) - len(mod), undefined], np.uint64)


def _fakes():
    from cqs_amd.index import HipIndex
    for name in ("semantic_diff", "detect_drift"):
        setattr(_FakeIndex, name, getattr(HipIndex, name))
    e = lambda *v: list(v) + [0.0] * (8 - len(v))
    src = _FakeIndex(["a.rs:keep", "a.rs:gone", "a.rs:turned", "a.rs:dup#1", "a.rs:dup#2", "a.rs:half", "a.rs:zero", "b.rs:half"],
                     [e(1, 0), e(0, 1), e(1, 0), e(1, 0), e(0, 1), e(1, 0), e(0, 0), e(1, 0)], 100)
    tgt = _FakeIndex(["b.rs:half", "a.rs:new", "a.rs:keep", "a.rs:turned", "a.rs:dup#7", "a.rs:half", "a.rs:zero"],
                     [e(1, 1), e(0, 0, 1), e(2, 0), e(0, 3), e(0, 5), e(1, 1), e(1, 0)], 0)
    return src, tgt


def test_semantic_diff_host_logic():
    src, tgt = _fakes()
    key = lambda cid: cid.split("#")[0]
    d = src.semantic_diff(tgt, 0.95, key=key)
    assert [x.id for x in d.added] == ["a.rs:new"] and [x.id for x in d.removed] == ["a.rs:gone"]
    assert all(x.similarity is None for x in d.added + d.removed)
    # last key wins: the source's "a.rs:dup" is row dup#2 = (0, 1), which equals the target's direction -> unchanged;
    # with dup#1 = (1, 0) it would be orthogonal and modified
    assert [x.id for x in d.modified] == ["a.rs:turned", "a.rs:zero", "a.rs:half", "b.rs:half"]
    assert [x.similarity for x in d.modified[:2]] == [0.0, 0.0]                   # an undefined pair counts through its 0.0; ties by id
    assert d.modified[2].similarity == d.modified[3].similarity == float(np.float32(1.0 / np.sqrt(2.0)))
    assert d.unchanged_count == 2                                                 # keep, dup
    assert src.calls == [([107, 100, 102, 104, 105, 106], [0, 2, 3, 4, 5, 6])]    # global rows: row_base added on each side
    # without the key the two dup ids match nothing
    d = src.semantic_diff(tgt, 0.95)
    assert [x.id for x in d.added] == ["a.rs:new", "a.rs:dup#7"] and [x.id for x in d.removed] == ["a.rs:gone", "a.rs:dup#1", "a.rs:dup#2"]


def test_modified_order_known_low_known_high_unknown():
    """src/diff.rs:340-342 and the tie-break."""
    from cqs_amd.index import DiffEntry, sort_modified
    got = sort_modified([DiffEntry("known_low", 0.3), DiffEntry("unknown", None), DiffEntry("known_high", 0.8)])
    assert [x.id for x in got] == ["known_low", "known_high", "unknown"]
    got = sort_modified([DiffEntry("z", 0.5), DiffEntry("m", None), DiffEntry("a", 0.5), DiffEntry("b", None), DiffEntry("neg0", -0.0),
                         DiffEntry("pos0", 0.0), DiffEntry("neg", -0.25)])
    assert [x.id for x in got] == ["neg", "neg0", "pos0", "a", "z", "b", "m"]       # f32 total order: -0.0 before 0.0


def test_detect_drift_host_logic():
    src, tgt = _fakes()
    r = src.detect_drift(tgt, 0.95, 0.0)
    assert [x.id for x in r.drifted] == ["a.rs:turned", "a.rs:zero", "a.rs:half", "b.rs:half"]
    assert [x.drift for x in r.drifted[:2]] == [1.0, 1.0]
    assert r.drifted[2].drift == float(np.float32(1.0) - np.float32(1.0 / np.sqrt(2.0)))   # 1.0 - sim in f32
    assert (r.total_compared, r.unchanged, r.threshold, r.min_drift) == (5, 1, 0.95, 0.0)   # (no key: the dup ids match nothing)
    r = src.detect_drift(tgt, 0.95, 0.5)                                          # min_drift keeps drift >= 0.5
    assert [x.id for x in r.drifted] == ["a.rs:turned", "a.rs:zero"] and r.total_compared == 5
    from cqs_amd.index import DiffEntry, drift_entries
    got = drift_entries([DiffEntry("edge", 0.75), DiffEntry("none", None), DiffEntry("under", 0.7500001)], 0.25)
    assert [x.id for x in got] == ["edge"]                                        # drift == min_drift stays; no similarity: skipped


def test_fixture_values_are_the_oracles():
    """tests/diff_cases.py's expected sims, pair by pair, against oracle.full_cosine_similarity (the reference's KATs pin it)."""
    from oracle import oracle
    for dim in dc.DIMS:
        a, b = dc.corpora(dim)
        ra, rb = dc.pairs(max(dc.MS))
        sims, undefined = dc.expected_sims(a, b, ra, rb)
        for i in range(len(ra)):
            s = oracle.full_cosine_similarity(a[int(ra[i])], b[int(rb[i])])
            assert (s is None) == bool(undefined[i]), (dim, i)
            assert bits(0.0 if s is None else s) == bits(sims[i]), (dim, i)
        assert undefined[0] and sims[1] == 1.0 and sims[2] == -1.0 and sims[3] == 0.0 and not undefined[3] and sims[4] == 1.0
        assert len(np.unique(sims)) >= 3 and (sims * 16 == np.round(sims * 16)).all(), dim
