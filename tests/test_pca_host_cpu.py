"""The device-free rules of the PCA of the stored rows (cqs_amd/csrc/pca_host.h) in a stand-alone program under ASAN +
UBSan: both argument plans (every refusal alone, and together, where the first in the documented order answers; m == 0),
the start matrix, the jitter and the scaling of the initial coordinates bit for bit against numpy, Gram-Schmidt with its
breakdown rule, the 8 x 8 eigen-solve, the sign rule and the finishing step against numpy (tests/pca_cases.py).  Then the
restatement's own bars on each corpus, and the C ABI's new symbols without a device.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pca_cases as pc  # noqa: E402
import umap_cases as uc  # noqa: E402

NULL_HANDLE, NULL_OUT = "pca: null handle", "pca: null output buffer"
COMPONENTS, PASSES = "pca: n_components not in [1, min(CQS_HIP_PCA_MAX_COMPONENTS, dim)]", "pca: more than 64 passes"
SHARDED, FEW = "pca: not built for a row-sharded handle", "pca: fewer than 2 rows"
P_NULL_HANDLE, P_NULL_IN, P_NULL_OUT = "pca_project: null handle", "pca_project: null mean or axes", "pca_project: null output buffer"
P_COMPONENTS = "pca_project: n_components not in [1, min(CQS_HIP_PCA_MAX_COMPONENTS, dim)]"
P_SHARDED, P_RANGE = "pca_project: not built for a row-sharded handle", "pca_project: range not in this index"

GOOD = dict(present=1, sharded=0, row_base=0, len=100, dim=32, nc=2, passes=0, outputs=1)
PGOOD = dict(present=1, sharded=0, row_base=10, len=100, dim=32, mean_axes=1, output=1, nc=2, first=10, m=100)


def _plans():
    case = lambda **kw: dict(GOOD, **kw)
    c = {"good": case(), "good_64_passes": case(passes=64), "good_4_components": case(nc=4), "good_2_rows": case(len=2),
         "good_dim_4": case(dim=4, nc=4), "good_dim_1": case(dim=1, nc=1), "good_row_base": case(row_base=1 << 40),
         "null_handle": case(present=0), "null_out": case(outputs=0), "nc_0": case(nc=0), "nc_5": case(nc=5),
         "nc_over_dim": case(dim=2, nc=3), "passes_65": case(passes=65), "sharded": case(sharded=1), "len_1": case(len=1),
         "len_0": case(len=0)}
    wrong = dict(outputs=0, nc=0, passes=65, sharded=1, len=1)
    c["all_wrong"] = case(present=0, **wrong)
    c["out_first"] = case(**wrong)
    c["components_before_passes"] = case(**dict(wrong, outputs=1))
    c["passes_before_sharded"] = case(**dict(wrong, outputs=1, nc=2))
    c["sharded_before_len"] = case(**dict(wrong, outputs=1, nc=2, passes=3))
    return c


def _projs():
    case = lambda **kw: dict(PGOOD, **kw)
    c = {"good": case(), "good_last_row": case(first=109, m=1), "good_inner": case(first=50, m=7),
         "m0": case(m=0), "m0_everything_else_wrong": case(m=0, mean_axes=0, output=0, nc=9, sharded=1, first=0),
         "m0_null_handle": case(m=0, present=0),
         "null_handle": case(present=0), "null_in": case(mean_axes=0), "null_out": case(output=0), "nc_0": case(nc=0),
         "nc_5": case(nc=5), "nc_over_dim": case(dim=1, nc=2), "sharded": case(sharded=1), "before_base": case(first=9, m=1),
         "past_end": case(first=110, m=1), "too_long": case(first=11, m=100), "overflow": case(first=10, m=2 ** 64 - 1)}
    wrong = dict(mean_axes=0, output=0, nc=0, sharded=1, first=0)
    c["all_wrong"] = case(present=0, **wrong)
    c["in_first"] = case(**wrong)
    c["out_before_components"] = case(**dict(wrong, mean_axes=1))
    c["components_before_sharded"] = case(**dict(wrong, mean_axes=1, output=1))
    c["sharded_before_range"] = case(**dict(wrong, mean_axes=1, output=1, nc=1))
    return c


def _gs_cases():
    rng = np.random.default_rng(11)
    c = {}
    for dim, p in ((32, 8), (8, 8), (4, 4), (1, 1), (96, 8)):
        c[f"random_{dim}_{p}"] = (rng.standard_normal((dim, 8)), p)
    a = rng.standard_normal((24, 8))
    a[:, 3] = 2.0 * a[:, 1] - a[:, 0]                          # column 3 in the span of the earlier ones
    c["dependent_column"] = (a, 8)
    a = rng.standard_normal((24, 8))
    a[:, 0] = 0.0                                              # a zero first column: e_0 takes its place
    a[:, 5] = 0.0
    c["zero_columns"] = (a, 8)
    c["all_zero"] = (np.zeros((16, 8)), 8)                     # e_0 .. e_7
    a = np.zeros((8, 8))
    a[:, 0] = 1.0
    c["e_d_in_the_span"] = (np.tile(a[:, :1], (1, 8)), 8)      # every column the same: the unit vectors fill in, none twice
    a = rng.standard_normal((12, 8))
    a[3, 2] = np.nan
    c["nan_column"] = (a, 8)
    a = rng.standard_normal((12, 8))
    a[:, 4] = np.inf
    c["inf_column"] = (a, 8)
    return c


def _eig_cases():
    rng = np.random.default_rng(12)
    c = {}
    for p in (1, 2, 4, 8):
        a = rng.standard_normal((p, p))
        c[f"random_{p}"] = a + a.T
    c["diagonal_unsorted"] = np.diag([1.0, 5.0, 3.0, 5.0, 0.0, -2.0, 4.0, 2.0])
    q, _ = np.linalg.qr(rng.standard_normal((8, 8)))
    c["planted"] = q @ np.diag([16.0, 4.0, 1.0, 0.5, 0.4, 0.3, 0.2, 0.1]) @ q.T
    c["zero"] = np.zeros((8, 8))
    return c


def _sign_cases():
    f = lambda *v: np.array(v, dtype=np.float32)
    return {"positive_stays": f(0.1, 0.9, -0.3), "negative_flips": f(0.1, -0.9, 0.3), "tie_lowest_index_negative": f(-0.5, 0.5, 0.1),
            "tie_lowest_index_positive": f(0.5, -0.5, 0.1), "zero": f(0.0, 0.0), "one": f(-1.0)}


SCALES = {"two_columns": (7, np.random.default_rng(13).standard_normal((50, 2)).astype(np.float32)),
          "one_column": (8, np.random.default_rng(14).standard_normal((33, 1)).astype(np.float32)),
          "duplicates": (9, np.tile(np.array([[0.25, -3.0]], np.float32), (6, 1))),
          "all_zero": (10, np.zeros((5, 2), np.float32)),
          "a_nan": (11, np.array([[1.0, np.nan], [2.0, 3.0]], np.float32)),
          "an_inf": (12, np.array([[1.0, 2.0], [np.inf, 3.0]], np.float32)),
          "denormal_top": (13, np.array([[1e-42, 0.0], [0.0, -1e-43]], np.float32))}
PLANS, PROJS, GS, EIG, SIGN = _plans(), _projs(), _gs_cases(), _eig_cases(), _sign_cases()
STARTS = {"s42_d32": (42, 32), "s1_d1": (1, 1), "s_big_d100": (2 ** 63 + 5, 100)}


def _fmt(v):
    return " ".join("nan" if np.isnan(x) else ("inf" if x == np.inf else repr(float(x))) for x in np.asarray(v, dtype=np.float64).reshape(-1))


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("pca_host") / "pca_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "pca_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = []
    for name, p in PLANS.items():
        lines.append(f"plan plan_{name} {p['present']} {p['sharded']} {p['row_base']} {p['len']} {p['dim']} {p['nc']} {p['passes']} {p['outputs']}")
    for name, p in PROJS.items():
        lines.append(f"proj proj_{name} {p['present']} {p['sharded']} {p['row_base']} {p['len']} {p['dim']} {p['mean_axes']} {p['output']} "
                     f"{p['nc']} {p['first']} {p['m']}")
    lines += [f"start start_{name} {seed} {dim}" for name, (seed, dim) in STARTS.items()]
    lines += [f"jitter jitter_{seed} {seed} 40" for seed in (1, 42, 2 ** 64 - 1)]
    for name, (seed, proj) in SCALES.items():
        lines.append(f"scale scale_{name} {seed} {proj.shape[0]} {proj.shape[1]} " + " ".join(str(v) for v in proj.reshape(-1).view(np.uint32)))
    for name, (a, p) in GS.items():
        lines.append(f"gs gs_{name} {a.shape[0]} {p} " + _fmt(a))
    for name, h in EIG.items():
        lines.append(f"eig eig_{name} {h.shape[0]} " + _fmt(h))
    for name, a in SIGN.items():
        lines.append(f"sign sign_{name} {len(a)} " + " ".join(str(v) for v in a.view(np.uint32)))
    rng = np.random.default_rng(15)
    v, _ = pc.gram_schmidt(rng.standard_normal((20, 8)), 8)
    cov = (lambda a: a @ a.T)(rng.standard_normal((20, 20)))
    y = cov @ v
    bad = y.copy()
    bad[0, 0] = np.nan
    trailing = y.copy()
    trailing[5, 7] = np.nan                                    # only the last column of H: the leading Rayleigh values stay finite
    huge = y * 1e45                                            # finite in f64, not as the f32 it is returned in
    for name, yy in (("finish_ok", y), ("finish_nan", bad), ("finish_nan_trailing", trailing), ("finish_huge", huge)):
        lines.append(f"finish {name} 20 8 50 3 " + _fmt(v) + " " + _fmt(yy))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-1500:])
    out = {}
    for ln in r.stdout.splitlines():
        f = ln.split("|")
        out[f[0]] = f[1:]
    assert len(out) == len(lines)
    out["_finish_inputs"] = (v, y, cov)
    return out


def _f32s(s):
    return np.array([int(x) for x in s.split(",") if x], dtype=np.uint32).view(np.float32)


def _f64s(s):
    return np.array([float(x) for x in s.split(",") if x], dtype=np.float64)


def test_every_refusal_of_pca_alone_and_in_order(got):
    why = lambda name: got["plan_" + name]
    refused = lambda text: ["0", text, "0", "0"]
    assert why("good") == ["1", "", "8", "16"] and why("good_64_passes") == ["1", "", "8", "64"]
    assert why("good_4_components") == ["1", "", "8", "16"] and why("good_2_rows") == ["1", "", "8", "16"]
    assert why("good_dim_4") == ["1", "", "4", "16"] and why("good_dim_1") == ["1", "", "1", "16"]
    assert why("good_row_base") == ["1", "", "8", "16"]
    assert why("null_handle") == refused(NULL_HANDLE) and why("null_out") == refused(NULL_OUT)
    assert why("nc_0") == refused(COMPONENTS) and why("nc_5") == refused(COMPONENTS) and why("nc_over_dim") == refused(COMPONENTS)
    assert why("passes_65") == refused(PASSES) and why("sharded") == refused(SHARDED)
    assert why("len_1") == refused(FEW) and why("len_0") == refused(FEW)
    assert why("all_wrong") == refused(NULL_HANDLE) and why("out_first") == refused(NULL_OUT)
    assert why("components_before_passes") == refused(COMPONENTS) and why("passes_before_sharded") == refused(PASSES)
    assert why("sharded_before_len") == refused(SHARDED)


def test_every_refusal_of_pca_project_alone_and_in_order(got):
    why = lambda name: got["proj_" + name]
    refused = lambda text: ["-1", text, "0"]
    assert why("good") == ["1", "", "0"] and why("good_last_row") == ["1", "", "99"] and why("good_inner") == ["1", "", "40"]
    assert why("m0") == ["0", "", "0"] and why("m0_everything_else_wrong") == ["0", "", "0"]
    assert why("m0_null_handle") == refused(P_NULL_HANDLE)
    assert why("null_handle") == refused(P_NULL_HANDLE) and why("null_in") == refused(P_NULL_IN) and why("null_out") == refused(P_NULL_OUT)
    assert why("nc_0") == refused(P_COMPONENTS) and why("nc_5") == refused(P_COMPONENTS) and why("nc_over_dim") == refused(P_COMPONENTS)
    assert why("sharded") == refused(P_SHARDED)
    for name in ("before_base", "past_end", "too_long", "overflow"):
        assert why(name) == refused(P_RANGE), name
    assert why("all_wrong") == refused(P_NULL_HANDLE) and why("in_first") == refused(P_NULL_IN)
    assert why("out_before_components") == refused(P_NULL_OUT) and why("components_before_sharded") == refused(P_COMPONENTS)
    assert why("sharded_before_range") == refused(P_SHARDED)


def test_start_matrix_jitter_and_scaling_bit_for_bit(got):
    for name, (seed, dim) in STARTS.items():
        want = pc.start_matrix(seed, dim)
        assert got["start_" + name][0] == ",".join(str(v) for v in want.reshape(-1).view(np.uint32)), name
        assert (want >= -1).all() and (want < 1).all()
    assert len(np.unique(pc.start_matrix(42, 32))) > 250                    # not a constant: 256 draws
    assert not np.array_equal(pc.start_matrix(42, 2)[:, :2], uc.initial_coords(42, 2) / 10)   # slot 2, not the coordinates' slot 0
    for seed in (1, 42, 2 ** 64 - 1):
        want = pc.jitter(seed, 40)
        assert got[f"jitter_{seed}"][0] == ",".join(str(v) for v in want.reshape(-1).view(np.uint32)), seed
        assert (np.abs(want) <= 1e-4).all() and len(np.unique(want)) == 80
    for name, (seed, proj) in SCALES.items():
        ok, bits = got["scale_" + name]
        want = pc.noisy_scale_coords(proj, seed)
        if want is None:
            assert ok == "0" and (_f32s(bits) == 7.0).all(), name                # refused: the output is untouched
        else:
            assert ok == "1" and bits == ",".join(str(v) for v in want.reshape(-1).view(np.uint32)), name
    assert [got["scale_" + n][0] for n in ("all_zero", "a_nan", "an_inf")] == ["0", "0", "0"]
    dup = _f32s(got["scale_duplicates"][1]).reshape(6, 2)
    assert len({tuple(r) for r in dup.tolist()}) == 6                           # duplicated rows do not start coincident
    assert np.abs(dup[:, 1]).max() <= 10.0001 and np.abs(dup[:, 1]).min() >= 9.9999
    one = _f32s(got["scale_one_column"][1]).reshape(33, 2)
    assert (np.abs(one[:, 1]) <= 1e-4).all()                                    # a missing second coordinate is 0 + jitter
    import cqs_amd.umap as product                                              # the Python layer's helper: the same bytes
    for name, (seed, proj) in SCALES.items():
        mine, want = product.pca_initial_coords(proj, seed), pc.noisy_scale_coords(proj, seed)
        assert (mine is None) == (want is None) and (mine is None or mine.tobytes() == want.tobytes()), name


def test_gram_schmidt_and_the_breakdown_rule(got):
    for name, (a, p) in GS.items():
        replaced, vals = got["gs_" + name]
        q = _f64s(vals).reshape(a.shape)
        want, want_replaced = pc.gram_schmidt(a, p)
        assert int(replaced) == len(want_replaced), name
        assert np.isfinite(q).all(), name
        assert np.abs(q[:, :p].T @ q[:, :p] - np.eye(p)).max() <= 1e-13, name
        assert (q[:, p:] == 0).all(), name
        assert np.abs(q - want).max() <= 1e-12, name
    q = _f64s(got["gs_all_zero"][1]).reshape(16, 8)
    assert got["gs_all_zero"][0] == "8" and np.array_equal(q, np.eye(16)[:, :8])        # e_0 .. e_7 in order
    assert got["gs_dependent_column"][0] == "1" and got["gs_zero_columns"][0] == "2"
    q = _f64s(got["gs_zero_columns"][1]).reshape(24, 8)
    assert np.array_equal(q[:, 0], np.eye(24)[:, 0])                                     # the first unit vector, whole
    q = _f64s(got["gs_e_d_in_the_span"][1]).reshape(8, 8)                                # column 0 = (1, .., 1) / sqrt 8
    assert got["gs_e_d_in_the_span"][0] == "7" and np.allclose(q[:, 0], 1 / np.sqrt(8))
    assert got["gs_nan_column"][0] == "1" and got["gs_inf_column"][0] == "1"
    assert got["gs_random_32_8"][0] == "0"
    a, _ = GS["random_32_8"]
    q = _f64s(got["gs_random_32_8"][1]).reshape(32, 8)
    qr, _ = np.linalg.qr(a)                                                              # the same spans column by column
    assert np.abs(np.abs(np.sum(q * qr, axis=0)) - 1).max() <= 1e-12


def test_small_eigen_solve_sign_rule_and_finish(got):
    for name, h in EIG.items():
        lam_s, w_s = got["eig_" + name]
        p = h.shape[0]
        lam, w = _f64s(lam_s), _f64s(w_s).reshape(p, p)
        want = np.linalg.eigvalsh(h)[::-1]
        scale = max(1.0, np.abs(want).max())
        assert np.abs(lam - want).max() <= 1e-12 * scale, name
        assert np.all(np.diff(lam) <= 0), name
        assert np.abs(w.T @ w - np.eye(p)).max() <= 1e-12, name
        assert np.abs(h @ w - w * lam[None, :]).max() <= 1e-11 * scale, name
    assert _f64s(got["eig_diagonal_unsorted"][0]).tolist() == [5.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.0, -2.0]
    for name, a in SIGN.items():
        assert got["sign_" + name][0] == ",".join(str(v) for v in pc.fix_sign(a).view(np.uint32)), name
    assert np.array_equal(_f32s(got["sign_tie_lowest_index_negative"][0]), np.array([0.5, -0.5, -0.1], np.float32))
    assert np.array_equal(_f32s(got["sign_tie_lowest_index_positive"][0]), np.array([0.5, -0.5, 0.1], np.float32))
    v, y, cov = got["_finish_inputs"]
    ok, axes_s, var_s = got["finish_ok"]
    axes, var = _f32s(axes_s).reshape(3, 20).astype(np.float64), _f32s(var_s).astype(np.float64)
    lam, w = pc.small_eigen(0.5 * (v.T @ y + (v.T @ y).T))
    assert ok == "1" and np.abs(var - lam[:3] / 49).max() <= 1e-6 * lam[0] / 49
    for k in range(3):
        assert np.abs(axes[k] - pc.fix_sign((v @ w[:, k]).astype(np.float32))).max() <= 1e-6, k
        assert abs(axes[k] @ cov @ axes[k] / 49 - var[k]) <= 1e-5 * var[0]             # the Rayleigh quotient it claims
    for name in ("finish_nan", "finish_nan_trailing", "finish_huge"):
        ok, axes_s, var_s = got[name]
        assert ok == "0" and (_f32s(axes_s) == 7.0).all() and (_f32s(var_s) == 7.0).all(), name   # refused, nothing written


@pytest.mark.parametrize("name", sorted(pc.RESTATED))
def test_restatement_passes_its_own_bars(name):
    """What tests/test_pca_gpu.py asks of the device, asked of the numpy restatement: its errors are the ones recorded in
    pca_cases.RESTATED (the device's bars are 100 times those), and the figures every answer must meet whatever its order
    of addition."""
    x = pc.corpora()[name]
    got = pc.pca(x)
    sin, deficit, var, mean, ortho = pc.errors(x, got)
    print(f"{name}: gap {pc.gap(pc.exact(x)[1]):.3f} sin {sin:.2e} deficit {deficit:.2e} variance {var:.2e} mean {mean:.2e} ortho {ortho:.2e}")
    rs, rd, rv = pc.RESTATED[name]
    assert deficit <= 1.5 * rd and var <= 1.5 * rv                       # as recorded (50 % for a numpy build's own sums)
    assert mean <= 1e-6 and ortho <= 1e-6
    if name == "isotropic":
        assert pc.gap(pc.exact(x)[1]) > pc.GAP_BAR                        # no gap to converge to: only the deficit is asked for
    else:
        assert pc.gap(pc.exact(x)[1]) <= pc.GAP_BAR and sin <= 1.5 * rs
    for k in range(2):
        assert got[1][k][np.argmax(np.abs(got[1][k]))] > 0                # the sign rule
    assert got[4] == []                                                   # no column broke down
    _, lam, _ = pc.exact(x)
    assert abs(got[3] - lam.sum()) <= 1e-9 * lam.sum()                    # the total variance is the covariance's trace


def test_restatement_on_the_degenerate_corpora():
    mean, axes, var, total, replaced = pc.pca(pc.identical())
    assert np.array_equal(mean, pc.identical()[0]) and (var == 0).all() and total == 0.0 and len(replaced) > 0
    assert np.array_equal(axes, np.eye(24, dtype=np.float32)[:2])          # the breakdown rule's unit vectors
    assert pc.pca_start(pc.identical(), 3) is None                         # nothing to scale: the hashed coordinates stay
    x = pc.rank_one()
    mean, axes, var, total, _ = pc.pca(x)
    _, lam, vec = pc.exact(x)
    assert abs(var[0] - lam[0]) <= 1e-6 * lam[0] and var[1] <= 1e-6 * lam[0] and abs(abs(axes[0] @ vec[:, 0]) - 1) <= 1e-6
    assert np.abs(axes.astype(np.float64) @ axes.T.astype(np.float64) - np.eye(2)).max() <= 1e-6
    x = pc.isotropic(8, 50, 4)                                             # dim < 8: p = dim, exact after one pass
    assert pc.errors(x, pc.pca(x, 2, 1))[1] <= 1e-9


def test_global_rho_and_the_recorded_layout_table():
    x, labels = pc.ring(2)
    assert x.shape == (480, 32) and np.allclose(np.linalg.norm(x, axis=1), 1.0, atol=1e-6)
    start = pc.pca_start(x, 2)
    assert pc.global_rho(x, labels, start) >= 0.99                         # the PCA projection alone keeps the centroids' order
    assert abs(pc.global_rho(x, labels, uc.initial_coords(2, 480))) <= 0.5
    assert np.abs(start).max() <= 10.0002
    y = pc.restated_layout(x, 2, "pca")
    # The table of DESIGN.md §3.18b, to what a rounding-level change may move it (another BLAS adds in another order, and
    # the layout is chaotic in its roundings): the margins the device is given in tests/test_pca_gpu.py, both ways.
    rho, kept, purity = pc.global_rho(x, labels, y), uc.preservation(x, y), uc.purity(labels, y)
    print(f"seed 2: rho {rho:.3f} kept {kept:.3f} purity {purity:.3f}")
    assert abs(rho - pc.RECORDED_PCA_RHO[1]) <= pc.RHO_MARGIN
    assert abs(kept - pc.RECORDED_PCA_KEPT[1]) <= 3 * uc.SPREAD and abs(purity - pc.RECORDED_PCA_PURITY[1]) <= 0.03
    assert round(max(pc.RECORDED_PCA_RHO) - min(pc.RECORDED_PCA_RHO), 3) == 0.073   # the table's own spread, as pca_cases says


def test_pca_symbols_without_a_device():
    """The library exports the new entry points; a NULL handle is INVALID from each of them."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    assert _lib.PCA_MAX_COMPONENTS == 4 and (_lib.UMAP_INIT_RANDOM, _lib.UMAP_INIT_PCA) == (0, 1)
    out = np.full(8, 7.0, dtype=np.float32)
    assert lib.cqs_hip_index_pca(None, 2, 0, 42, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_pca_project(None, out.ctypes.data, out.ctypes.data, 2, 0, 1, out.ctypes.data) == _lib.ERR_INVALID
    assert lib.cqs_hip_index_umap_project_init(None, 15, 0, 42, 1, out.ctypes.data) == _lib.ERR_INVALID
    assert (out == 7.0).all()
    header = open(os.path.join(ROOT, "include", "cqs_hip.h")).read()
    assert "#define CQS_HIP_PCA_MAX_COMPONENTS 4" in header and "#define CQS_HIP_UMAP_INIT_PCA    1" in header
    assert f"kSlabRows = {pc.SLAB};" in open(os.path.join(ROOT, "cqs_amd", "csrc", "pca_host.h")).read()
