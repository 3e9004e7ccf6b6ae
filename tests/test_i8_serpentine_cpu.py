"""The int8 scan's serpentine sweep, device-free (cqs_amd/csrc/i8_sweep.h; DESIGN.md §3.11, "Serpentine sweep"):
tests/i8_sweep_driver.cpp, a stand-alone program built with ASAN + UBSan.  For both parities the map from launched workgroups
to the workgroups whose tasks they take is a bijection and the waves' tasks cover every padded row exactly once - over the
tier regimes of plan_tiers and hand-built tiers with every n_tasks mod 4, a partial last group and a group across the
64 / 32-row boundary.  The plain-load window is exactly the workgroups whose bytes meet the first or the last W bytes of the
copy, for W = 0 (none), W inside the copy (edges on, one byte before and one byte after a workgroup's boundary) and W at
least the copy's size (all), at n equal to the pad and below it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_map_and_window_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "i8_sweep_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "i8_sweep_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-1500:])
    lines = p.stdout.splitlines()
    assert len(lines) == 3 and lines[-1] == "all ok", lines
    assert lines[0].startswith("mapping ok ") and int(lines[0].split()[-1]) >= 200, lines
    assert lines[1].startswith("window ok ") and int(lines[1].split()[-1]) >= 10000, lines


def test_header_is_device_free():
    """i8_sweep.h compiles without HIP: the driver above is the proof for g++; this pins what it may include."""
    src = open(os.path.join(ROOT, "cqs_amd", "csrc", "i8_sweep.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ['"group_map.h"'], incs
