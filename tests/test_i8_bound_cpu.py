"""Host-side arithmetic of the int8 copy's certificate (cqs_amd/csrc/scan_i8.h), without a device: the k' policy, gamma', and
B_q checked against a numpy f32 emulation, step for step, of what i8_build_kernel stores and scan_i8_kernel computes.
The header's host functions are compiled into a tiny driver with the system C++ compiler."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from shadow_emul import adversarial_rows, build_i8, f32_dot_chain, r_and_norm, scan_i8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cqs_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "scan_i8.h"
int main(int argc, char** argv) {
    if (!strcmp(argv[1], "kprime")) { for (int i = 2; i < argc; ++i) printf("%u %d\n", cqs::i8_kprime((uint32_t)atoi(argv[i])), (int)cqs::i8_k_ok((uint32_t)atoi(argv[i]))); }
    else if (!strcmp(argv[1], "gamma")) { printf("%.17g\n", cqs::i8_gamma((uint32_t)atoi(argv[2]))); }
    else if (!strcmp(argv[1], "dimok")) { for (int i = 2; i < argc; ++i) printf("%d\n", (int)cqs::i8_dim_ok((uint32_t)atoi(argv[i]))); }
    else if (!strcmp(argv[1], "bound"))   // q_norm2 r_max norm_max dim
        printf("%a\n", (double)cqs::i8_query_bound(strtod(argv[2], 0), strtod(argv[3], 0), strtod(argv[4], 0), (uint32_t)atoi(argv[5])));
    else if (!strcmp(argv[1], "bound16"))
        printf("%a\n", (double)cqs::shadow_query_bound(strtod(argv[2], 0), strtod(argv[3], 0), strtod(argv[4], 0), (uint32_t)atoi(argv[5])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    d = tmp_path_factory.mktemp("i8bound")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", CSRC, str(src), "-o", str(exe), "-lm"])

    def run(*args):
        return subprocess.check_output([str(exe)] + [str(a) for a in args], text=True).split()
    return run


def bound(driver, q, r_max, n_max, dim, which="bound"):
    q2 = float(np.dot(q.astype(np.float64), q.astype(np.float64)))
    return float.fromhex(driver(which, repr(q2), repr(float(r_max)), repr(float(n_max)), dim)[0])


# the kernels' arithmetic in numpy: shadow_emul.py (shared with the device test of the same premises)


@pytest.mark.parametrize("dim", [16, 128, 768, 1040, 2048])
def test_bound_covers_the_kernel_arithmetic(driver, dim):
    rng = np.random.default_rng(1000 + dim)
    x = adversarial_rows(rng, dim)
    codes, scale = build_i8(x)
    assert np.all(np.abs(codes) <= 127) and np.all(codes == np.rint(codes))
    assert scale[12] == 0 and scale[13] == 0 and not codes[12].any() and not codes[13].any()
    # the rows go in groups of comparable magnitude: one index-wide R over rows 30 orders of magnitude apart proves little
    groups = [np.r_[0:12], np.r_[12:16], np.r_[16:17], np.r_[17:19], np.r_[19:20], np.r_[20:64]]
    queries = [rng.standard_normal(dim).astype(np.float32), np.ones(dim, np.float32) * np.float32(0.5),
               (rng.standard_normal(dim) * 1e-20).astype(np.float32), (rng.standard_normal(dim) * 1e12).astype(np.float32)]
    for g in groups:
        r_max, n_max = r_and_norm(driver, x[g], codes[g], scale[g], dim)
        for q in queries:
            bq = bound(driver, q, r_max, n_max, dim)
            st = scan_i8(codes[g], scale[g], q).astype(np.float64)
            s = f32_dot_chain(x[g], q).astype(np.float64)
            exact = x[g].astype(np.float64) @ q.astype(np.float64)
            if not np.isfinite(bq):
                continue                 # no certificate for this (query, index): nothing is claimed
            assert np.all(np.isfinite(st)) and np.all(np.isfinite(s))
            assert np.all(np.abs(s - st) <= bq), (dim, g[0], np.abs(s - st).max(), bq)
            assert np.all(np.abs(exact - st) <= bq)
    # the whole set under one R as well (what an index holding all of them would use), moderate queries
    r_max, n_max = r_and_norm(driver, x[:17], codes[:17], scale[:17], dim)
    for q in queries[:2]:
        bq = bound(driver, q, r_max, n_max, dim)
        assert np.isfinite(bq)
        assert np.all(np.abs(f32_dot_chain(x[:17], q).astype(np.float64) - scan_i8(codes[:17], scale[:17], q)) <= bq)


def test_bound_is_not_vacuous(driver):
    """On unit rows the bound is the quantisation error, not orders above it: R_8 ~ 0.0134 at 768-d."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2000, 768)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    codes, scale = build_i8(x)
    r_max, n_max = r_and_norm(driver, x, codes, scale, 768)
    q = x[0]
    bq = bound(driver, q, r_max, n_max, 768)
    assert 0.008 < bq < 0.02
    err = np.abs(f32_dot_chain(x, q).astype(np.float64) - scan_i8(codes, scale, q))
    assert err.max() <= bq and err.max() > bq / 50


def test_bound_monotone_and_inf_where_bf16_is(driver):
    base = dict(q2=1.0, r=1e-2, nm=1.0, dim=768)
    def b(which="bound", **kw):
        a = dict(base, **kw)
        return float.fromhex(driver(which, repr(a["q2"]), repr(a["r"]), repr(a["nm"]), a["dim"])[0])
    for key, vals in (("q2", [0.0, 1e-30, 1e-3, 1.0, 7.0, 1e20, 1e60]), ("r", [0.0, 1e-9, 1e-2, 1.0, 1e10]),
                      ("nm", [0.0, 1e-3, 1.0, 1e10, 1e25]), ("dim", [16, 128, 768, 2048])):
        got = [b(**{key: v}) for v in vals]
        assert all(x <= y for x, y in zip(got, got[1:])), (key, got)
    for q2 in (1e-10, 1.0, 1e30, 1e50, 1e60, 1e70):
        for nm in (1e-20, 1.0, 1e10, 1e19, 1e25):
            if not np.isfinite(b("bound16", q2=q2, nm=nm)):
                assert not np.isfinite(b(q2=q2, nm=nm)), (q2, nm)
    assert not np.isfinite(b(q2=1e60, nm=1e10))
    # the unscaled code sum could overflow although the scaled score does not: tiny rows, huge query
    assert np.isfinite(b("bound16", q2=2.0 ** 180, nm=1e-20)) and not np.isfinite(b(q2=2.0 ** 180, nm=1e-20))
    assert b() >= 1e-2 and b(q2=float("nan")) == float("inf")


def test_gamma_and_dim_rule(driver):
    for dim in (16, 768, 2048):
        u = (dim + 2) * 2.0 ** -24
        assert float(driver("gamma", dim)[0]) == pytest.approx(u / (1 - u), rel=1e-15)
    dims = [8, 16, 24, 264, 768, 1040, 2048, 2064]
    assert [int(v) for v in driver("dimok", *dims)] == [0, 1, 0, 0, 1, 1, 1, 0]


def test_kprime_policy_against_the_measurements(driver):
    ks = [1, 5, 20, 50, 87, 88, 100, 500, 1024]
    out = driver("kprime", *ks)
    kp, ok = [int(v) for v in out[0::2]], [int(v) for v in out[1::2]]
    assert kp == [10 * k + 150 for k in ks]
    assert ok == [1 if 10 * k + 150 <= 1023 else 0 for k in ks] and ok[4] == 1 and ok[5] == 0
    assert all(p >= k for p, k in zip(kp, ks))
    # at least 1.5x the largest k' any measured query needed, everywhere it was measured (profiles/i8_scan_bench.json)
    with open(os.path.join(ROOT, "profiles", "i8_scan_bench.json")) as f:
        meas = json.load(f)["needed_kprime"]["rows"]
    assert {"1000000", "10000000"} <= set(meas)
    for n, per_k in meas.items():
        for k in (1, 5, 20, 50, 100):
            need = per_k[str(k)]["max"]
            assert 10 * k + 150 >= 1.5 * need, (n, k, need)


def test_new_kernel_sources_have_no_inline_assembly():
    """The int8 files add no inline assembly (scan_bf16_kernel's opaque zero is not needed without a work queue): every store
    is a vector store written in plain C++."""
    for name in ("scan_i8.hip", "scan_i8.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "asm" not in text.replace("__builtin_amdgcn", ""), name
