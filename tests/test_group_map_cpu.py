"""The map behind the int8 shadow scan's workgroup maxima, device-free (cqs_amd/csrc/group_map.h; DESIGN.md §3.11, "Workgroup
maxima"): tests/group_map_driver.cpp, a stand-alone program built with ASAN + UBSan.  The groups of 1, 2 and 4 tasks over every
tier regime of plan_tiers (16-row tasks, 64-row tasks, 64 + 32) and over hand-built tiers with every n_tasks mod 4 - they
partition [0, n_pad) in order, hold <= 256 rows and agree with their tasks, across the 64 / 32-row boundary and in a partial
last group; the rule that combines up to four wave triples against brute force over the group's rows (ties at the maximum
inside a wave and across waves, all -inf, one finite row, the maximum in the last task); and the select's premise restated
on the host with four tasks per group: every top-k entry is a candidate, and the candidates are the entries at or above T."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_map_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "group_map_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "group_map_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-1500:])
    lines = p.stdout.splitlines()
    assert len(lines) == 4 and lines[-1] == "all ok", lines
    assert lines[0].startswith("map ok ") and int(lines[0].split()[-1]) > 3000, lines
    assert lines[1] == "combine ok 4000" and lines[2] == "premise ok 480", lines


def test_header_is_device_free():
    """group_map.h compiles without HIP: the driver above is the proof for g++; this pins what it may include."""
    src = open(os.path.join(ROOT, "cqs_amd", "csrc", "group_map.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ["<stdint.h>", "<hip/hip_runtime.h>"], incs
    assert src.index("#if defined(__HIPCC__)") < src.index("<hip/hip_runtime.h>")
