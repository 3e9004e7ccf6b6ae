"""Host-side arithmetic of the bf16 shadow's certificate (cqs_amd/csrc/scan_bf16.h), without a device: the k' policy,
gamma, rounding up to f32, and B_q = ||q|| R checked against f32 dot products of f32 rows and of their bf16 roundings.
The header's host functions are compiled into a tiny driver with the system C++ compiler."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from shadow_emul import bf16_round, f32_dot_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "cqs_amd", "csrc", "scan_bf16.h")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "scan_bf16.h"
int main(int argc, char** argv) {
    if (!strcmp(argv[1], "kprime")) { for (int i = 2; i < argc; ++i) printf("%u\n", cqs::shadow_kprime((uint32_t)atoi(argv[i]))); }
    else if (!strcmp(argv[1], "gamma")) { printf("%.17g\n", cqs::shadow_gamma((uint32_t)atoi(argv[2]))); }
    else if (!strcmp(argv[1], "roundup")) { for (int i = 2; i < argc; ++i) printf("%a\n", (double)cqs::round_up_f32(strtod(argv[i], 0))); }
    else if (!strcmp(argv[1], "bound"))   // q_norm2 r_max norm_max dim
        printf("%a\n", (double)cqs::shadow_query_bound(strtod(argv[2], 0), strtod(argv[3], 0), strtod(argv[4], 0), (uint32_t)atoi(argv[5])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    d = tmp_path_factory.mktemp("bf16bound")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe), "-lm"])

    def run(*args):
        return subprocess.check_output([str(exe)] + [str(a) for a in args], text=True).split()
    return run


def test_kprime_policy(driver):
    ks = [1, 20, 100, 495, 496, 500, 1000, 1023, 1024]
    got = [int(v) for v in driver("kprime", *ks)]
    assert got == [min(2 * k + 32, 1023) for k in ks]
    assert all(kp >= k for k, kp in zip(ks, got) if k <= 1023)   # every k but max_k can be certified
    assert got[-1] < 1024                                          # k = max_k: the shadow cannot answer


def test_gamma(driver):
    for dim in (8, 768, 2048):
        u = dim * 2.0 ** -24
        assert float(driver("gamma", dim)[0]) == pytest.approx(u / (1 - u), rel=1e-15)


def test_round_up_is_the_smallest_f32_above(driver):
    rng = np.random.default_rng(3)
    vals = list(rng.uniform(0, 1, 50)) + list(rng.uniform(0, 1e-3, 50)) + [0.0, 1.0, 2.0 ** -126, 3.4e38]
    got = [float.fromhex(v) for v in driver("roundup", *[repr(float(v)) for v in vals])]
    for v, f in zip(vals, got):
        f32 = np.float32(f)
        assert float(f32) == f and f >= v
        assert float(np.nextafter(f32, np.float32(0))) < v or f == v
    assert driver("roundup", "1e39") == ["inf"]


@pytest.mark.parametrize("dim,scale", [(64, 1.0), (768, 1.0), (768, 37.0), (2048, 0.01)])
def test_bound_covers_f32_dot_products(driver, dim, scale):
    rng = np.random.default_rng(dim)
    x = (rng.standard_normal((400, dim)) * scale * rng.uniform(0.1, 3.0, (400, 1))).astype(np.float32)
    x[:8] = np.abs(x[:8])                                        # rows whose signs align with q: every error adds up
    xt = bf16_round(x)
    gam = float(driver("gamma", dim)[0])
    nx = np.linalg.norm(x.astype(np.float64), axis=1)
    nt = np.linalg.norm(xt.astype(np.float64), axis=1)
    r = np.linalg.norm(x.astype(np.float64) - xt.astype(np.float64), axis=1) + gam * (nx + nt)
    r_max, n_max = float(r.max()) * (1 + 2.0 ** -30), float(max(nx.max(), nt.max())) * (1 + 2.0 ** -30)
    for q in (rng.standard_normal(dim).astype(np.float32), np.ones(dim, np.float32) * np.float32(0.5)):
        bq = float.fromhex(driver("bound", repr(float(np.dot(q.astype(np.float64), q.astype(np.float64)))), repr(r_max), repr(n_max), dim)[0])
        s, st = f32_dot_chain(x, q), f32_dot_chain(xt, q)
        assert np.all(np.abs(s.astype(np.float64) - st.astype(np.float64)) <= bq)
        exact = x.astype(np.float64) @ q.astype(np.float64)
        assert np.all(np.abs(s.astype(np.float64) - exact) <= bq)   # (the f32 score itself is within the bound)


def test_bound_refuses_overflow_range(driver):
    assert driver("bound", repr(1e60), "1e-3", "1e10", 768) == ["inf"]
    assert float.fromhex(driver("bound", "1.0", "1e-3", "1.0", 768)[0]) >= 1e-3
