"""The launch plans of the search-time chain, device-free (cqs_amd/csrc/query_plan.h): tests/query_plan_driver.cpp, a
stand-alone program built with ASAN + UBSan, sweeps T = 1..128 x both hidden sizes x heads x kv heads x every subset of the
four switches x the K classes and checks every plan against the kernels' LDS layouts and tiling rules, and the chain's
longest length against the plans.  Here: the lengths at which a form changes are query_state.BREAKS, and the form of
every step equals tests/golden/query_plan_forms.json - kernel instantiation, grid and workgroup size per (geometry,
switches, T, step), extracted from a kernel trace of the commit before the plans existed (the trace reports no dynamic
LDS size, so the table holds none)."""
import json
import os
import shutil
import subprocess

import pytest

import query_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("query_plan") / "query_plan_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "query_plan_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    for v in [k for k in env if k.startswith("CQS_HIP_QUERY_")]:
        del env[v]
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-1500:])
    return p.stdout.splitlines()


def test_plans_under_sanitizers(out):
    assert out[0].startswith("checks ok ") and int(out[0].split()[2]) > 1_000_000, out[0]
    assert out[-1] == "all ok"


def test_header_is_device_free():
    """query_plan.h compiles without HIP: the driver is the proof for g++; this pins what it may include (nothing of HIP: its
    constexpr layouts are usable from device code as they are)."""
    src = open(os.path.join(ROOT, "cqs_amd", "csrc", "query_plan.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ["<stddef.h>", "<stdint.h>", "<stdlib.h>"], incs
    assert "__device__" not in src and "__global__" not in src and "hip_runtime" not in src


def test_form_changes_are_the_break_lengths(out):
    assert [int(x) for x in out[1].split()[1:]] == query_state.BREAKS and out[1].startswith("breaks ")


def test_forms_equal_the_golden_table(out):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "query_plan_forms.json")))
    got, unsupported = {}, set()
    for ln in out:
        f = ln.split("|")
        if f[0] != "g":
            continue
        if f[2] == "unsupported":
            unsupported.add(f[1])
        elif f[2] == "rope":
            got.setdefault(f[1], {})["rope"] = True
        elif f[2] == "launches":
            got.setdefault(f[1], {})["launches"] = int(f[3])
        else:
            got.setdefault(f[1], {})[f[2]] = "|".join(f[3:])
    assert len(gold) == 282                                            # 2 geometries x 5 switch sets x 36 lengths - 78 past a 64-token chain
    for geom in ("small", "full"):
        for cfg in ("all", "staged0", "split0", "attn80_0", "fuse0"):
            for T in query_state.LENS:
                key = f"{geom}/{cfg}/{T}"
                if key not in gold:                                    # the traced engine sent this length to the batch chain
                    assert key in unsupported and T > 64, key
                    continue
                want = dict(gold[key])
                rope = want.pop("rope", None)                          # (its grid is launch_qk_norm_rope's, not a plan's)
                have = dict(got[key])
                assert have.pop("rope", False) == (rope is not None), key
                assert have == want, (key, have, want)
