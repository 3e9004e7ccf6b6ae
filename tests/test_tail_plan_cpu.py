"""The tiers of the shadow search's tail kernel, device-free (cqs_amd/csrc/tail_plan.h; DESIGN.md §3.11, "Prefix first"):
tests/tail_plan_driver.cpp, a stand-alone program built with ASAN + UBSan, sweeps the header the host launcher and the kernel
share over k in [1, 128], the k' of both copies, blocks of 1..8 queries and 1 / 8 / 256 CUs: tier 1 never has more slots
than the tail without tiers, the grid is never 0 and never above the cap, no proper prefix means the old numbers exactly,
and j1 is tail_prefix_first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "tail_plan_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "tail_plan_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-1500:])
    lines = p.stdout.splitlines()
    assert lines[0].startswith("plan ok ") and lines[0].endswith("(tiered 87)"), lines
    assert lines[1:] == ["headline ok", "default ok", "all ok"], lines


def test_header_is_device_free():
    """tail_plan.h adds nothing but tail_prefix.h, which compiles without HIP (tests/test_tail_prefix_cpu.py)."""
    src = open(os.path.join(ROOT, "cqs_amd", "csrc", "tail_plan.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ['"tail_prefix.h"'], incs
