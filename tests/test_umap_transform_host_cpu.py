"""The device-free rules of the UMAP transform (cqs_amd/csrc/umap_transform_host.h) in a stand-alone program under ASAN +
UBSan: the argument plan (every refusal alone, and together, where the first in the documented order answers), m == 0, the
default epoch count, the quarter-rate alpha, the bisection's target, and the f32 weights and initial position against the
numpy restatement (tests/umap_transform_cases.py).  Then the restatement's own bars on the hold-out corpus for each seed,
and the C ABI's new symbols without a device.  No GPU."""
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
import umap_transform_cases as tc  # noqa: E402

NULL_PARAMS, NULL_OUT, NULL_ARRAY, NULL_ANCHORS = ("transform: null params", "transform: null output buffer",
                                                   "transform: null neighbour array", "transform: null anchors")
NO_ANCHORS, TOO_MANY_ANCHORS = "transform: no anchors", "transform: more than 2^31 anchors"
TOO_MANY_NEW, IDS = "transform: more than CQS_HIP_KNN_MAX_TARGETS new vertices", "transform: id_base + m is greater than 2^32"
STRIDE = "transform: stride not in [1, CQS_HIP_NEIGHBORS_MAX]"
COUNT2, ID3 = "transform: vertex 2 has a count greater than the stride", "transform: vertex 3 lists a neighbour outside the anchors"
NONFINITE, NONPOSITIVE, EPOCHS = ("transform: non-finite a, b, learning_rate or repulsion", "transform: a and b must be positive",
                                  "transform: more than 10000 epochs")
GOOD = dict(params=1, arrays=1, anchors=1, out=1, n=4, m=None, stride=2, a="1.5769434603", b="0.8950608779", lr="1", rep="1", neg=5,
            epochs=0, id_base=4, counts=[2, 1, 0, 2], rows=[1, 2, 0, 0, 0, 0, 3, 1])


def _plan_cases():
    c = {}
    case = lambda **kw: dict(GOOD, **kw)
    c["good"] = case()
    c["good_epochs_10000"] = case(epochs=10000)
    c["good_m_10000_default_epochs"] = case(counts=[0] * 10000, rows=[0] * 10000, stride=1)
    c["good_m_10001_default_epochs"] = case(counts=[0] * 10001, rows=[0] * 10001, stride=1)
    c["good_m_65536"] = case(counts=[0] * 65536, rows=[0] * 65536, stride=1)
    c["good_stride_100"] = case(stride=100, counts=[1, 1], rows=[3] + [0] * 99 + [0] * 100)
    c["good_n_2^31"] = case(n=2 ** 31)
    c["good_last_ids"] = case(id_base=2 ** 32 - 4)
    c["good_zero_lr_negative_repulsion"] = case(lr="0", rep="-1")
    c["good_an_id_equal_to_its_vertex_is_an_anchor"] = case(rows=[0, 2, 1, 0, 0, 0, 3, 1])
    c["id_past_n_beyond_count_is_not_read"] = case(rows=[1, 2, 0, 99, 99, 99, 3, 1])
    # m == 0 is answered after the NULL checks that hold for it (params) and before everything else
    empty = dict(counts=[], rows=[])
    c["m0"] = case(**empty)
    c["m0_null_everything_but_params"] = case(arrays=0, anchors=0, out=0, **empty)
    c["m0_before_n0_stride_and_epochs"] = case(n=0, stride=0, epochs=10001, a="nan", id_base=2 ** 64 - 1, **empty)
    c["m0_null_params"] = case(params=0, **empty)
    # every refusal alone
    c["null_params"] = case(params=0)
    c["null_out"] = case(out=0)
    c["null_arrays"] = case(arrays=0)
    c["null_anchors"] = case(anchors=0)
    c["n0"] = case(n=0)
    c["too_many_anchors"] = case(n=2 ** 31 + 1)
    c["too_many_new"] = case(m=65537)
    c["ids_past_2^32"] = case(id_base=2 ** 32 - 3)
    c["ids_overflow_u64"] = case(id_base=2 ** 64 - 1)
    c["stride_0"] = case(stride=0, rows=[])
    c["stride_101"] = case(stride=101, rows=[0] * 404)
    c["count_over_stride"] = case(counts=[2, 1, 3, 2])
    c["id_past_n"] = case(rows=[1, 2, 0, 0, 0, 0, 3, 4])
    for field in ("a", "b", "lr", "rep"):
        for bad in ("nan", "inf", "-inf"):
            c[f"nonfinite_{field}_{bad}"] = case(**{field: bad})
    c["a_zero"] = case(a="0")
    c["a_negative"] = case(a="-1")
    c["b_zero"] = case(b="0")
    c["b_negative"] = case(b="-0.5")
    c["epochs_10001"] = case(epochs=10001)
    # together: the first in the documented order answers
    wrong = dict(n=0, m=65537, id_base=2 ** 64 - 1, stride=0, a="nan", epochs=10001)
    c["all_wrong"] = case(params=0, arrays=0, anchors=0, out=0, **wrong)
    c["out_before_arrays"] = case(arrays=0, anchors=0, out=0, **wrong)
    c["arrays_before_anchors"] = case(arrays=0, anchors=0, **wrong)
    c["anchors_before_n0"] = case(anchors=0, **wrong)
    c["n0_before_the_rest"] = case(**wrong)
    c["anchors_size_before_m"] = case(**dict(wrong, n=2 ** 31 + 1))
    c["m_before_ids"] = case(**dict(wrong, n=4))
    c["ids_before_stride"] = case(**dict(wrong, n=4, m=None))
    c["stride_before_count"] = case(stride=101, rows=[0] * 404, counts=[200, 0, 0, 0], a="nan")
    c["count_before_id"] = case(counts=[2, 1, 3, 2], rows=[9, 2, 0, 0, 0, 0, 3, 1], a="nan")
    c["id_before_params"] = case(rows=[1, 2, 0, 0, 0, 0, 3, 4], a="nan", epochs=10001)
    c["nonfinite_before_sign"] = case(a="-1", b="nan")
    c["sign_before_epochs"] = case(b="0", epochs=10001)
    return c


def _place_cases():
    """name -> (anchors f32 [n, 2], scores f32 [c], ids [c])."""
    c = {}
    rng = np.random.default_rng(21)
    for k, count in enumerate((1, 2, 14, 64, 65, 100)):
        n = 1000
        anchors = tc.random_anchors(30 + k, n)
        rows, scores, _ = tc.random_lists(40 + k, n, 1, count, counts=[count], dup_every=5 if count > 2 else 0)
        c[f"list_of_{count}"] = (anchors, scores[0], rows[0])
        odd = scores[0].copy()
        odd[0], odd[-1] = 1.5, -0.75                                    # scores above 1 (d clamps to 0) and below 0 (d > 1)
        c[f"list_of_{count}_scores_above_1_and_below_0"] = (anchors, np.sort(odd)[::-1], rows[0])
        c[f"list_of_{count}_all_d_0"] = (anchors, np.ones(count, np.float32), rows[0])
    c["empty_list"] = (tc.random_anchors(1, 3), np.zeros(0, np.float32), np.zeros(0, np.uint64))
    c["one_anchor_n1"] = (tc.random_anchors(2, 1), np.array([0.25], np.float32), np.zeros(1, np.uint64))
    c["repeated_ids"] = (tc.random_anchors(3, 2), rng.uniform(0, 1, 9).astype(np.float32), rng.integers(0, 2, 9).astype(np.uint64))
    c["weights_that_all_underflow"] = (tc.random_anchors(4, 5), np.array([-1e30, -2e30], np.float32), np.array([1, 2], np.uint64))
    return c


PLANS, PLACES = _plan_cases(), _place_cases()
ALPHAS = {f"lr{lr}_e{e}_E{E}": (int(np.float32(lr).view(np.uint32)), e, E)
          for lr in (1.0, 0.37) for E in (1, 10, 30, 100, 10000) for e in sorted({1, max(1, E // 2), E})}
TARGETS = (1, 2, 15, 100)


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("umap_transform_host") / "umap_transform_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "umap_transform_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = []
    for name, p in PLANS.items():
        m_real = len(p["counts"])
        lines.append(" ".join(str(v) for v in ["plan", name, p["params"], p["arrays"], p["anchors"], p["out"], p["n"],
                                                m_real if p["m"] is None else p["m"], m_real, p["stride"], p["a"], p["b"], p["lr"],
                                                p["rep"], p["neg"], p["epochs"], p["id_base"]]
                              + p["counts"] + (p["rows"] + [0] * (m_real * p["stride"]))[:m_real * p["stride"]]))
    for name, (anchors, scores, ids) in PLACES.items():
        lines.append(" ".join(str(v) for v in ["place", name, len(anchors), len(scores)] + scores.view(np.uint32).tolist()
                              + ids.tolist() + anchors.reshape(-1).view(np.uint32).tolist()))
    lines += [f"epochs m{m} {m}" for m in (1, 10000, 10001, 65536)]
    lines += [f"run run_{ep}_of_{E} {ep} {E}" for ep, E in ((0, 100), (7, 100), (100, 100), (101, 100), (2 ** 32 - 1, 30))]
    lines += [f"alpha {name} {lb} {e} {E}" for name, (lb, e, E) in ALPHAS.items()]
    lines += [f"target c{c} {c}" for c in TARGETS]
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
    why = lambda name: tuple(got[name])
    refused = lambda text: ("0", text, "0", "0")
    assert why("null_params") == refused(NULL_PARAMS) and why("m0_null_params") == refused(NULL_PARAMS)
    assert why("null_out") == refused(NULL_OUT) and why("null_arrays") == refused(NULL_ARRAY)
    assert why("null_anchors") == refused(NULL_ANCHORS)
    assert why("n0") == refused(NO_ANCHORS) and why("too_many_anchors") == refused(TOO_MANY_ANCHORS)
    assert why("too_many_new") == refused(TOO_MANY_NEW)
    assert why("ids_past_2^32") == refused(IDS) and why("ids_overflow_u64") == refused(IDS)
    assert why("stride_0") == refused(STRIDE) and why("stride_101") == refused(STRIDE)
    assert why("count_over_stride") == refused(COUNT2) and why("id_past_n") == refused(ID3)
    for field in ("a", "b", "lr", "rep"):
        for bad in ("nan", "inf", "-inf"):
            assert why(f"nonfinite_{field}_{bad}") == refused(NONFINITE), (field, bad)
    for name in ("a_zero", "a_negative", "b_zero", "b_negative"):
        assert why(name) == refused(NONPOSITIVE), name
    assert why("epochs_10001") == refused(EPOCHS)


def test_refusals_together_answer_in_the_documented_order(got):
    first = lambda name: got[name][:2]
    assert first("all_wrong") == ["0", NULL_PARAMS] and first("out_before_arrays") == ["0", NULL_OUT]
    assert first("arrays_before_anchors") == ["0", NULL_ARRAY] and first("anchors_before_n0") == ["0", NULL_ANCHORS]
    assert first("n0_before_the_rest") == ["0", NO_ANCHORS] and first("anchors_size_before_m") == ["0", TOO_MANY_ANCHORS]
    assert first("m_before_ids") == ["0", TOO_MANY_NEW] and first("ids_before_stride") == ["0", IDS]
    assert first("stride_before_count") == ["0", STRIDE] and first("count_before_id") == ["0", COUNT2]
    assert first("id_before_params") == ["0", ID3]
    assert first("nonfinite_before_sign") == ["0", NONFINITE] and first("sign_before_epochs") == ["0", NONPOSITIVE]


def test_accepted_plans_m0_and_the_default_epochs(got):
    ok = lambda name: got[name]
    assert ok("good") == ["1", "", "0", "100"] and ok("good_epochs_10000") == ["1", "", "0", "10000"]
    assert ok("good_m_10000_default_epochs") == ["1", "", "0", "100"] and ok("good_m_10001_default_epochs") == ["1", "", "0", "30"]
    assert ok("good_m_65536") == ["1", "", "0", "30"]
    for name in ("good_stride_100", "good_n_2^31", "good_last_ids", "good_zero_lr_negative_repulsion",
                 "good_an_id_equal_to_its_vertex_is_an_anchor", "id_past_n_beyond_count_is_not_read"):
        assert ok(name) == ["1", "", "0", "100"], name
    for name in ("m0", "m0_null_everything_but_params", "m0_before_n0_stride_and_epochs"):
        assert ok(name) == ["1", "", "1", "0"], name                       # OK, nothing to do
    assert [got[f"m{m}"] for m in (1, 10000, 10001, 65536)] == [["100"], ["100"], ["30"], ["30"]]
    assert [tc.default_epochs(m) for m in (1, 10000, 10001, 65536)] == [100, 100, 30, 30]
    assert [got[f"run_{ep}_of_{E}"] for ep, E in ((0, 100), (7, 100), (100, 100), (101, 100), (2 ** 32 - 1, 30))] == \
        [["0"], ["7"], ["100"], ["100"], ["30"]]


def test_alpha_and_the_target_against_numpy_float32(got):
    for name, (lb, e, E) in ALPHAS.items():
        lr = np.array([lb], dtype=np.uint32).view(np.float32)[0]
        assert got[name] == [str(int(np.float32(tc.alpha_of(lr, e, E)).view(np.uint32)))], name
    bits = lambda x: str(int(np.float32(x).view(np.uint32)))
    assert got["lr1.0_e1_E100"] == [bits(0.25)] and got["lr1.0_e100_E100"] == [bits(np.float32(0.25) * (np.float32(1) - np.float32(99) / np.float32(100)))]
    assert got["lr1.0_e50_E100"] == [bits(np.float32(0.25) * (np.float32(1) - np.float32(49) / np.float32(100)))]
    for c in TARGETS:
        val = np.array([int(got[f"c{c}"][0])], dtype=np.uint32).view(np.float32)[0]
        assert abs(float(val) - np.log2(float(c))) <= 2.0 ** -22, c      # log2f: within an ulp or two of the f64 value
    assert got["c1"] == ["0"] and got["c2"] == [bits(1.0)]


def test_weights_and_initial_position_against_numpy(got):
    f32s = lambda s: np.array([int(x) for x in s.split(",") if x], dtype=np.uint32).view(np.float32)
    for name, (anchors, scores, ids) in PLACES.items():
        sigma_s, w_s, x_s, y_s, placed = got[name]
        sigma, w, xy = f32s(sigma_s)[0], f32s(w_s), np.concatenate([f32s(x_s), f32s(y_s)])
        want_sigma, want_w = tc.weights_of(scores)
        # The bar of the layout's weights (both sides stop the bisection within 1e-5 of the target): 1e-4.
        assert len(w) == len(scores) and np.all(np.abs(w.astype(np.float64) - want_w) <= 1e-4), name
        assert abs(float(sigma) - want_sigma) <= 1e-4 * max(1.0, want_sigma), name
        # The initial position in f64 over the program's own f32 weights: the form of the epoch bound.
        c = len(scores)
        y, mass, ok = tc.initial(anchors, ids[None, :].reshape(1, c), np.array([c]), w[None, :].reshape(1, c))
        assert placed == ("1" if ok[0] else "0"), name
        assert np.all(np.abs(xy.astype(np.float64) - y[0]) <= 1e-5 * (1.0 + mass[0])), name
    for count in (1, 2, 14, 64, 65, 100):
        assert np.all(f32s(got[f"list_of_{count}_all_d_0"][1]) == 1.0)                      # d = 0: weight 1, sigma's floor is 0
        if count > 1:
            assert f32s(got[f"list_of_{count}_scores_above_1_and_below_0"][1])[0] == 1.0    # a score above 1 is d = 0
    assert got["empty_list"] == ["0", "", "0", "0", "0"]                                     # (0, 0), never moves
    assert got["weights_that_all_underflow"][2:] == ["0", "0", "0"]
    anchors, _, ids = PLACES["list_of_1"]                                                    # one anchor: exactly on it
    assert [int(got["list_of_1"][2]), int(got["list_of_1"][3])] == anchors[int(ids[0])].view(np.uint32).tolist()
    assert [int(got["one_anchor_n1"][2]), int(got["one_anchor_n1"][3])] == PLACES["one_anchor_n1"][0][0].view(np.uint32).tolist()


@pytest.mark.parametrize("seed", tc.SEEDS)
def test_restatement_passes_its_own_bars(seed):
    """What tests/test_umap_transform_gpu.py asks of the device, asked of the f64 restatement alone on the hold-out corpus:
    the epochs improve on the initial position, the placement is far from random, a call may be cut anywhere, and a list
    of one starts exactly on its anchor."""
    xa, la, xn, ln, anchors, rows, scores, counts = tc.holdout(seed)
    assert xa.shape == (400, 32) and xn.shape == (80, 32) and anchors.shape == (400, 2) and rows.shape == (80, 15)
    y = tc.transform(anchors, rows, scores, counts, n_epochs=100, seed=seed)
    y0 = tc.transform(anchors, rows, scores, counts, n_epochs=100, epochs=0, seed=seed)
    kept, kept0 = tc.kept(rows, anchors, y), tc.kept(rows, anchors, y0)
    kept_random = tc.kept(rows, anchors, tc.random_placement(seed, anchors, len(xn)))
    print(f"seed {seed}: kept {kept:.3f}, initial only {kept0:.3f}, random {kept_random:.3f}, purity {tc.purity(la, ln, anchors, y):.3f}")
    assert np.isfinite(y).all()
    assert kept > kept0
    assert kept > 5 * kept_random
    assert round(kept, 3) == tc.RECORDED_SYNC_KEPT[seed - 1]                 # the table of DESIGN.md §3.18a
    cut = np.concatenate([tc.transform(anchors, rows[:33], scores[:33], counts[:33], n_epochs=100, seed=seed),
                          tc.transform(anchors, rows[33:], scores[33:], counts[33:], id_base=400 + 33, n_epochs=100, seed=seed)])
    assert cut.tobytes() == y.tobytes()
    one = tc.transform(anchors, rows[:, :1], scores[:, :1], np.ones(80, np.uint32), n_epochs=100, epochs=0, seed=seed)
    assert np.array_equal(one, anchors[rows[:, 0].astype(np.int64)].astype(np.float64))


def test_transform_symbols_without_a_device():
    """The library exports the transform's entry points.  The argument plan answers before any device work: refusals come
    back as INVALID with their text in the handle-less slot, the outputs untouched; m == 0 is OK."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    assert _lib.TRANSFORM_ALL == 0xFFFFFFFF
    p = _lib.LayoutParams()
    lib.cqs_hip_layout_params_default(C.byref(p))
    anchors = np.zeros((2, 2), dtype=np.float32)
    rows = np.array([[1], [5]], dtype=np.uint64)
    scores = np.zeros((2, 1), dtype=np.float32)
    counts = np.ones(2, dtype=np.uint32)
    out = np.full((2, 2), 7.0, dtype=np.float32)
    call = lambda n, m, params, id_base=2: lib.cqs_hip_umap_transform(
        0, n, anchors.ctypes.data, m, 1, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data, params, id_base, _lib.TRANSFORM_ALL,
        out.ctypes.data, None, None)
    buf = C.create_string_buffer(256)
    text = lambda: (lib.cqs_hip_layout_last_error(None, buf, 256), buf.value.decode())[1]
    assert call(2, 2, C.byref(p)) == _lib.ERR_INVALID and text() == "transform: vertex 1 lists a neighbour outside the anchors"
    assert call(2, 2, None) == _lib.ERR_INVALID and text() == NULL_PARAMS
    assert call(0, 2, C.byref(p)) == _lib.ERR_INVALID and text() == NO_ANCHORS
    assert call(2, 2, C.byref(p), id_base=2 ** 32 - 1) == _lib.ERR_INVALID and text() == IDS
    p.n_epochs = 10001
    assert call(2, 1, C.byref(p)) == _lib.ERR_INVALID and text() == EPOCHS
    assert call(0, 0, C.byref(p)) == _lib.OK and text() == ""              # m == 0: before the checks that read anything
    assert (out == 7.0).all()
    assert lib.cqs_hip_layout_transform(None, 0, 1, None, None, None, 0, 0, 0, None, None, None) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_umap_transform(None, 0, None, None, 0, 15, 0, 42, None) == _lib.ERR_INVALID
