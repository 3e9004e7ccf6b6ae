"""The device-free rules of the UMAP layout (cqs_amd/csrc/umap_host.h) in a stand-alone program under ASAN + UBSan: the
argument plan (every refusal alone, and together, where the first in the documented order answers), the adjacency builder
against the numpy restatement (tests/umap_cases.py), the active rule against numpy float32, the hash, the draw, the initial
coordinates and alpha against numpy uint32 / float32.  Then the C ABI's new symbols without a device, and
the restatement's own quality on the CPU.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import umap_cases as uc  # noqa: E402

NULL_OUT, NULL_PARAMS, NULL_ARRAY = "layout: null output handle", "layout: null params", "layout: null graph array"
TOO_MANY, STRIDE = "layout: more than 2^31 vertices", "layout: stride not in [1, CQS_HIP_NEIGHBORS_MAX]"
NONFINITE, NONPOSITIVE, EPOCHS = "layout: non-finite a, b, learning_rate or repulsion", "layout: a and b must be positive", "layout: more than 10000 epochs"
GOOD = dict(out=1, params=1, arrays=1, stride=2, a="1.5769434603", b="0.8950608779", lr="1", rep="1", neg=5, epochs=0, seed=42,
            counts=[2, 1, 0, 2], rows=[1, 2, 0, 0, 0, 0, 0, 1], n=None)


def _plan_cases():
    c = {}
    case = lambda **kw: dict(GOOD, **kw)
    c["good"] = case()
    c["good_epochs_10000"] = case(epochs=10000)
    c["good_big_default_epochs"] = case(counts=[0] * 10001, rows=[0] * 10001, stride=1)
    c["good_10000_vertices"] = case(counts=[0] * 10000, rows=[0] * 10000, stride=1)
    c["good_n0_null_arrays"] = case(arrays=0, counts=[], rows=[])
    c["good_n1"] = case(counts=[0], rows=[0, 0])
    c["good_stride_100"] = case(stride=100, counts=[1, 1], rows=[1] + [0] * 99 + [0] * 100)
    c["good_zero_lr_negative_repulsion"] = case(lr="0", rep="-1")
    # every refusal alone
    c["null_out"] = case(out=0)
    c["null_params"] = case(params=0)
    c["null_arrays"] = case(arrays=0)
    c["too_many"] = case(n=2 ** 31 + 1)
    c["most_vertices_pass_the_size_check"] = case(n=2 ** 31, stride=0)           # (2^31 itself is allowed: the next check answers)
    c["stride_0"] = case(stride=0, rows=[])
    c["stride_101"] = case(stride=101, rows=[0] * 404)
    c["count_over_stride"] = case(counts=[2, 1, 3, 2])
    c["id_past_n"] = case(rows=[1, 2, 0, 0, 0, 0, 0, 4])
    c["id_is_self"] = case(rows=[1, 2, 1, 0, 0, 0, 0, 1])
    c["id_past_n_beyond_count_is_not_read"] = case(rows=[1, 2, 0, 99, 99, 99, 0, 1])
    for field in ("a", "b", "lr", "rep"):
        for bad in ("nan", "inf", "-inf"):
            c[f"nonfinite_{field}_{bad}"] = case(**{field: bad})
    c["a_zero"] = case(a="0")
    c["a_negative"] = case(a="-1")
    c["b_zero"] = case(b="0")
    c["b_negative"] = case(b="-0.5")
    c["epochs_10001"] = case(epochs=10001)
    # together: the first in the documented order answers
    c["all_wrong"] = case(out=0, params=0, arrays=0, n=2 ** 31 + 1, stride=0)
    c["params_before_arrays"] = case(params=0, arrays=0, stride=0)
    c["arrays_before_size"] = case(arrays=0, n=2 ** 31 + 1)
    c["size_before_stride"] = case(n=2 ** 31 + 1, stride=0, a="nan", epochs=10001)
    c["stride_before_count"] = case(stride=101, rows=[0] * 404, counts=[200, 0, 0, 0], a="nan")
    c["count_before_id"] = case(counts=[2, 1, 3, 2], rows=[9, 2, 0, 0, 0, 0, 0, 1], a="nan")
    c["id_before_params"] = case(rows=[1, 2, 0, 0, 0, 0, 0, 3], a="nan", epochs=10001)
    c["nonfinite_before_sign"] = case(a="-1", b="nan")
    c["sign_before_epochs"] = case(b="0", epochs=10001)
    return c


def _hub(n_spokes, stride):
    return uc.hub_graph(n_spokes, stride)


def _adj_cases():
    c = {}
    z = lambda n, s: (np.zeros((n, s), np.uint64), np.full((n, s), 0.5, np.float32), np.zeros(n, np.uint32))
    r, s, k = z(2, 1); r[0, 0], r[1, 0], k[:] = 1, 0, 1
    c["mutual_pair_n2"] = (r, s, k)
    r, s, k = z(2, 1); r[0, 0], k[0] = 1, 1
    c["one_direction_n2"] = (r, s, k)
    r, s, k = z(3, 2); r[0, :2], k[0] = [2, 1], 2; r[2, 0], k[2] = 0, 1
    c["mixed_n3"] = (r, s, k)
    c["hub_500_stride1"] = _hub(500, 1)
    c["hub_500_stride100"] = _hub(500, 100)
    c["ragged_stride14"] = uc.ragged_graph(5, 65, 14, dup_every=3, empty_vertex=7)
    c["ragged_stride100"] = uc.ragged_graph(6, 130, 100, empty_vertex=0)
    c["ragged_stride1"] = uc.ragged_graph(7, 40, 1)
    c["all_empty"] = z(5, 3)
    c["n1"] = z(1, 4)
    c["n0"] = z(0, 4)
    r, s, k = uc.ragged_graph(8, 20, 5)
    r[3, :], k[3] = [0, 1, 2, 4, 5], 5
    s[3, :] = [1.5, np.nan, 1.0, -0.0, 2.0 ** -149]          # d: clamps to 0, NaN -> 0, 0, 1, 1 (rounded)
    c["odd_scores"] = (r, s, k)
    return c


def _p_sweep():
    f = lambda x: int(np.float32(x).view(np.uint32))
    ps = {"one": f(1.0), "just_below_one": f(np.nextafter(np.float32(1.0), np.float32(0.0))), "half": f(0.5), "third": f(1.0 / 3.0),
          "zero": 0, "smallest_denormal": 1, "largest_denormal": 0x007FFFFF, "smallest_normal": 0x00800000, "tenth": f(0.1)}
    for E in (10, 200, 500):
        inv = np.float32(1.0) / np.float32(E)
        ps[f"inv_{E}"] = f(inv)
        ps[f"below_inv_{E}"] = f(np.nextafter(inv, np.float32(0.0)))
        ps[f"above_inv_{E}"] = f(np.nextafter(inv, np.float32(1.0)))
    rng = np.random.default_rng(3)
    for i, v in enumerate(rng.uniform(0, 1, 12).astype(np.float32)):
        ps[f"random_{i}"] = f(v)
    return ps


def _hash_cases():
    c = {"zeros_n1": (0, 0, 0, 0, 0, 1), "zeros_n2": (0, 0, 0, 0, 0, 2), "seed42": (42, 1, 0, 0, 0, 480),
         "big_seed": (2 ** 64 - 1, 10000, 2 ** 31 - 1, 199, 4, 2 ** 31), "high_seed_word": (1 << 32, 3, 5, 7, 1, 1000),
         "low_seed_word": (1, 3, 5, 7, 1, 1000)}
    rng = np.random.default_rng(9)
    for i in range(24):
        n = int(rng.choice([1, 2, 3, 480, 17523, 10 ** 6, 2 ** 31]))
        c[f"hash_random_{i}"] = (int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 10001)), int(rng.integers(0, 2 ** 31)),
                            int(rng.integers(0, 5000)), int(rng.integers(0, 8)), n)
    return c


PLANS, ADJS, PS, HASHES = _plan_cases(), _adj_cases(), _p_sweep(), _hash_cases()
ALPHAS = {f"lr{lr}_e{e}_E{E}": (int(np.float32(lr).view(np.uint32)), e, E)
          for lr in (1.0, 0.37) for E in (1, 10, 200, 500, 10000) for e in sorted({1, 2, E // 3 + 1, E})}


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("umap_host") / "umap_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "umap_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = []
    for name, p in PLANS.items():
        n_real = len(p["counts"])
        lines.append(" ".join(str(v) for v in ["plan", name, p["out"], p["params"], p["arrays"], n_real if p["n"] is None else p["n"],
                                                n_real, p["stride"], p["a"], p["b"], p["lr"], p["rep"], p["neg"], p["epochs"], p["seed"]]
                              + p["counts"] + (p["rows"] + [0] * (n_real * p["stride"]))[:n_real * p["stride"]]))
    for name, (r, s, k) in ADJS.items():
        lines.append(" ".join(str(v) for v in ["adj", name, len(k), r.shape[1]] + k.tolist() + r.reshape(-1).tolist()
                              + np.ascontiguousarray(s).view(np.uint32).reshape(-1).tolist()))
    lines += [f"active {name} {bits} 500" for name, bits in PS.items()]
    lines += ["hash " + name + " " + " ".join(str(v) for v in h) for name, h in HASHES.items()]
    lines += [f"init s{seed}_v{v} {seed} {v}" for seed in (0, 42, 2 ** 64 - 1) for v in (0, 1, 479, 2 ** 31 - 1)]
    lines += [f"alpha {name} {lb} {e} {E}" for name, (lb, e, E) in ALPHAS.items()]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    out = {}
    for ln in p.stdout.splitlines():
        f = ln.split("|")
        out[f[0]] = f[1:]
    assert len(out) == len(lines)
    return out


def test_every_refusal_alone(got):
    why = lambda name: (got[name][0], got[name][1], got[name][2])
    assert why("null_out") == ("0", NULL_OUT, "0") and why("null_params") == ("0", NULL_PARAMS, "0")
    assert why("null_arrays") == ("0", NULL_ARRAY, "0") and why("too_many") == ("0", TOO_MANY, "0")
    assert why("most_vertices_pass_the_size_check") == ("0", STRIDE, "0")
    assert why("stride_0") == ("0", STRIDE, "0") and why("stride_101") == ("0", STRIDE, "0")
    assert why("count_over_stride") == ("0", "layout: vertex 2 has a count greater than the stride", "0")
    assert why("id_past_n") == ("0", "layout: vertex 3 lists a neighbour outside the graph", "0")
    assert why("id_is_self") == ("0", "layout: vertex 1 lists itself", "0")
    for field in ("a", "b", "lr", "rep"):
        for bad in ("nan", "inf", "-inf"):
            assert why(f"nonfinite_{field}_{bad}") == ("0", NONFINITE, "0"), (field, bad)
    for name in ("a_zero", "a_negative", "b_zero", "b_negative"):
        assert why(name) == ("0", NONPOSITIVE, "0"), name
    assert why("epochs_10001") == ("0", EPOCHS, "0")


def test_refusals_together_answer_in_the_documented_order(got):
    first = lambda name: got[name][:2]
    assert first("all_wrong") == ["0", NULL_OUT] and first("params_before_arrays") == ["0", NULL_PARAMS]
    assert first("arrays_before_size") == ["0", NULL_ARRAY] and first("size_before_stride") == ["0", TOO_MANY]
    assert first("stride_before_count") == ["0", STRIDE]
    assert first("count_before_id") == ["0", "layout: vertex 2 has a count greater than the stride"]
    assert first("id_before_params") == ["0", "layout: vertex 3 lists itself"]
    assert first("nonfinite_before_sign") == ["0", NONFINITE] and first("sign_before_epochs") == ["0", NONPOSITIVE]


def test_accepted_plans_and_the_default_epochs(got):
    ok = lambda name: got[name]
    assert ok("good") == ["1", "", "500"] and ok("good_epochs_10000") == ["1", "", "10000"]
    assert ok("good_10000_vertices") == ["1", "", "500"] and ok("good_big_default_epochs") == ["1", "", "200"]
    assert ok("good_n0_null_arrays") == ["1", "", "500"] and ok("good_n1") == ["1", "", "500"]
    assert ok("good_stride_100")[0] == "1" and ok("good_zero_lr_negative_repulsion")[0] == "1"
    assert ok("id_past_n_beyond_count_is_not_read")[0] == "1"


def test_adjacency_builder_against_numpy(got):
    ints = lambda s: [int(x) for x in s.split(",") if x]
    for name, (r, s, k) in ADJS.items():
        off, nbr, bits = (ints(x) for x in got[name])
        want_off, want_nbr = uc.adjacency(r, k)
        assert off == want_off.tolist() and nbr == want_nbr.tolist(), name
        d = uc.distances(s)
        want_bits = []
        for i in range(len(k) if len(k) >= 2 else 0):
            fwd = d[i, :int(k[i])].view(np.uint32).tolist()
            want_bits += fwd + [0] * (int(want_off[i + 1] - want_off[i]) - len(fwd))
        assert bits == want_bits, name
    ints_of = lambda name, i: ints(got[name][i])
    assert ints_of("mutual_pair_n2", 0) == [0, 1, 2] and ints_of("mutual_pair_n2", 1) == [1, 0]
    assert ints_of("one_direction_n2", 0) == [0, 1, 2] and ints_of("one_direction_n2", 1) == [1, 0]     # stored at both ends
    assert ints_of("mixed_n3", 1) == [2, 1, 0, 0]
    for name in ("hub_500_stride1", "hub_500_stride100"):
        assert ints_of(name, 0)[:2] == [0, 500] and ints_of(name, 1)[:500] == list(range(1, 501))      # ascending ids
    assert ints_of("all_empty", 0) == [0] * 6 and ints_of("n1", 0) == [0, 0] and ints_of("n0", 0) == [0]
    assert np.array(ints_of("odd_scores", 2)[ints_of("odd_scores", 0)[3]:][:5], np.uint32).view(np.float32).tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]


def test_active_rule_against_numpy_float32(got):
    for name, bits in PS.items():
        p = np.array([bits], dtype=np.uint32).view(np.float32)[0]
        want = "".join("1" if uc.active(e, p) else "0" for e in range(1, 501))
        assert got[name][0] == want, name
    assert got["one"][0] == "1" * 500 and got["zero"][0] == "0" * 500
    assert got["smallest_denormal"][0] == "0" * 500 and got["largest_denormal"][0] == "0" * 500
    assert got["half"][0] == "01" * 250
    assert got["below_inv_500"][0].count("1") <= 1 and got["inv_200"][0].count("1") in (2, 3)


def test_hash_draw_initial_coordinates_and_alpha_against_numpy(got):
    for name, (seed, epoch, vertex, slot, draw, n) in HASHES.items():
        h = int(uc.hash5(seed, epoch, vertex, slot, draw))
        q = int(uc.draw_vertex(h, n))
        assert got[name] == [str(h), str(q)], name
        assert q < n
    assert got["zeros_n1"][1] == "0" and got["high_seed_word"][0] != got["low_seed_word"][0]
    for seed in (0, 42, 2 ** 64 - 1):
        for v in (0, 1, 479, 2 ** 31 - 1):
            want = [np.float32(np.float32((int(uc.hash5(seed, 0, v, 0, c)) >> 8)) * np.float32(20.0 / 16777216.0)) - np.float32(10.0) for c in (0, 1)]
            assert got[f"s{seed}_v{v}"] == [str(int(np.float32(w).view(np.uint32))) for w in want]
            assert all(-10.0 <= w < 10.0 for w in want)
    xy = uc.initial_coords(42, 480)
    assert got["s42_v479"] == [str(int(b)) for b in xy[479].view(np.uint32)]
    for name, (lb, e, E) in ALPHAS.items():
        lr = np.array([lb], dtype=np.uint32).view(np.float32)[0]
        assert got[name] == [str(int(np.float32(uc.alpha_of(lr, e, E)).view(np.uint32)))], name


def test_layout_symbols_without_a_device():
    """The library exports the layout's entry points.  The argument plan answers before any device work: refusals come
    back as INVALID with their text, *out stays NULL."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    p = _lib.LayoutParams()
    lib.cqs_hip_layout_params_default(C.byref(p))
    assert (p.negative_samples, p.n_epochs, p.seed, p.learning_rate, p.repulsion) == (5, 0, 42, 1.0, 1.0)
    assert (np.float32(p.a), np.float32(p.b)) == (np.float32(1.5769434603), np.float32(0.8950608779))
    rows = np.array([[1], [5]], dtype=np.uint64)
    scores = np.zeros((2, 1), dtype=np.float32)
    counts = np.ones(2, dtype=np.uint32)
    h = C.c_void_p(7)
    assert lib.cqs_hip_layout_create(0, 2, 1, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data, C.byref(p), C.byref(h)) == _lib.ERR_INVALID
    assert not h.value
    buf = C.create_string_buffer(256)
    lib.cqs_hip_layout_last_error(None, buf, 256)
    assert buf.value == b"layout: vertex 1 lists a neighbour outside the graph"
    assert lib.cqs_hip_layout_create(0, 2, 1, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data, None, C.byref(h)) == _lib.ERR_INVALID
    assert lib.cqs_hip_layout_create(0, 2, 1, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data, C.byref(p), None) == _lib.ERR_INVALID
    assert lib.cqs_hip_layout_len(None) == 0 and lib.cqs_hip_layout_edges(None) == 0 and lib.cqs_hip_layout_epochs(None) == 0
    assert lib.cqs_hip_layout_run(None, 1, None) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_umap_project(None, 15, 0, 42, None) == _lib.ERR_INVALID
    lib.cqs_hip_layout_destroy(None)


def test_restatement_passes_its_own_quality_bars():
    """What tests/test_umap_gpu.py asks of the device, asked of the f64 restatement alone: 15-NN preservation at least 5x a
    random layout's, purity far above chance, finite coordinates - on one seed of the four-cluster corpus."""
    x, labels = uc.clusters(1)
    y = uc.restated_layout(x, seed=42)
    y0 = uc.initial_coords(42, len(x))
    assert np.isfinite(y).all()
    assert uc.preservation(x, y) >= 5 * uc.preservation(x, y0)
    assert uc.purity(labels, y) >= 0.95
