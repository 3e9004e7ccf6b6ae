"""MMR re-rank, the parts that need no GPU: the numpy restatement of the reference's `mmr_rerank`
(tests/mmr_cases.py) against the reference's own unit-test data (tests/golden/mmr_kats.json), the algebraic shortcut
the device kernel takes (running maximum == per-step re-fold), the binding table, and the device-free part of the
two entry points (cqs_amd/csrc/mmr_host.h) under ASAN + UBSan."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import mmr_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kats():
    with open(os.path.join(ROOT, "tests", "golden", "mmr_kats.json")) as f:
        return json.load(f)["cases"]


def test_golden_file_is_complete_and_cited():
    cases = _kats()
    assert [c["name"] for c in cases] == ["lambda_one_is_noop", "diversifies_same_file_crowding", "lambda_zero_pure_diversity",
                                          "handles_empty", "limit_zero_returns_empty", "pool_smaller_than_limit"]
    for c in cases:
        assert c["source"].startswith("src/search/mmr.rs:"), c["name"]
        n = len(c["scores"])
        sim = np.array(c["similarity"], dtype=np.float64).reshape(n, n)
        assert np.array_equal(sim, sim.T) and set(np.unique(sim)) <= {0.0, 0.15, 0.2, 0.4}


@pytest.mark.parametrize("running_max", [False, True])
@pytest.mark.parametrize("case", _kats(), ids=lambda c: c["name"])
def test_restatement_satisfies_the_reference_unit_tests(case, running_max):
    picks = mc.mmr_rerank(case["scores"], case["similarity"], case["limit"], case["lambda"], running_max=running_max)
    exp = case["expect"]
    if "picks" in exp:
        assert picks == exp["picks"]
    if "count" in exp:
        assert len(picks) == exp["count"]
    for pos, idx in exp.get("at", []):
        assert picks[pos] == idx, picks
    for idx in exp.get("contains", []):
        assert idx in picks, picks
    assert len(set(picks)) == len(picks)


def test_running_max_equals_the_per_step_refold():
    """`max` over finite values is exact and order-free, so folding only the LAST pick's similarities into a running
    maximum gives the value mmr.rs:83-90 re-folds from 0.0 at every step: same picks on 200 random pools (negative
    similarities, exact ties, every lambda regime)."""
    rng = np.random.default_rng(20)
    for trial in range(200):
        m = int(rng.integers(2, 80))
        scores, sim = mc.random_pool(rng, m)
        limit = int(rng.integers(1, m))
        lam = [0.0, 0.25, 0.5, 0.7, 0.95, float(rng.uniform(0, 1))][trial % 6]
        a = mc.mmr_rerank(scores, sim, limit, lam, running_max=False)
        b = mc.mmr_rerank(scores, sim, limit, lam, running_max=True)
        assert a == b, (trial, m, limit, lam)
        assert len(a) == limit and len(set(a)) == limit
        assert a[0] == 0     # max_sim is 0 at the first step: lam * score is monotone in the (descending) scores, ties to index 0


def test_restatement_total_order_and_ties():
    # -0.0 sorts below +0.0 under total_cmp; equal values go to the lowest index
    k = mc.total_order_keys(np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32))
    assert list(k) == sorted(k) and len(set(k)) == 6
    assert mc.mmr_rerank([0.5, 0.5, 0.5], np.zeros((3, 3)), 2, 0.5) == [0, 1]
    # negative similarities count as 0 (the fold starts at 0.0): candidate 2's -0.9 is no bonus over candidate 1's 0.0,
    # the two tie and the lower index wins
    sim = np.array([[1, 0.0, -0.9], [0.0, 1, 0], [-0.9, 0, 1]], np.float32)
    assert mc.mmr_rerank([0.9, 0.5, 0.5], sim, 2, 0.5) == [0, 1]
    sim[0, 1] = sim[1, 0] = 0.1
    assert mc.mmr_rerank([0.9, 0.5, 0.5], sim, 2, 0.5) == [0, 2]


def test_binding_table_carries_both_symbols():
    from cqs_amd import _lib
    names = {s[0] for s in _lib.SIGNATURES}
    assert {"cqs_hip_index_pairwise", "cqs_hip_index_mmr"} <= names
    assert _lib.MMR_MAX == _lib.MAX_K == 1024


def test_host_part_under_sanitizers(tmp_path):
    """mmr_host.h (argument checks, the early answers of mmr.rs:64-69) in a stand-alone program under ASAN + UBSan."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "mmr_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "mmr_host_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    got = {ln.split()[0]: ln.split(None, 4)[1:] for ln in p.stdout.splitlines()}
    INVALID, EMPTY, IDENTITY, DEVICE = "-1", "0", "1", "2"
    assert got["device"][:3] == [DEVICE, "20", "0.7"]
    assert got["clamp_low"][:3] == [DEVICE, "5", "0"]
    assert got["clamp_high"][:3] == [IDENTITY, "5", "1"]
    assert got["lambda_one"][:3] == [IDENTITY, "5", "1"]
    assert got["limit_zero"][0] == EMPTY and got["empty"][0] == EMPTY
    assert got["limit_ge_m"][:2] == [IDENTITY, "33"] and got["limit_huge"][:2] == [IDENTITY, "33"]
    assert got["m_max"][:2] == [DEVICE, "100"]
    for name, why in (("m_over", "CQS_HIP_MMR_MAX"), ("nan_lambda", "lambda"), ("inf_lambda", "lambda"), ("inf_score", "score"),
                      ("ninf_score", "score"), ("row_past_end", "row"), ("row_below_base", "row"), ("bad_row_identity", "row"),
                      ("null_rows", "rows"), ("null_scores", "scores"), ("empty_index", "row")):
        assert got[name][0] == INVALID and why in got[name][3], (name, got[name])
    assert got["pairwise_ok"] == [DEVICE] and got["pairwise_past"] == [INVALID]
    assert got["pairwise_empty"] == [EMPTY] and got["pairwise_null"] == [INVALID]
