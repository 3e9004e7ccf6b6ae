"""The prefix certificate of the shadow search's tail, device-free (cqs_amd/csrc/tail_prefix.h; DESIGN.md §3.11, "Prefix
certificate"): tests/tail_prefix_driver.cpp, a stand-alone program built with ASAN + UBSan, sorting a prefix of a query's rescored
candidates first (the kernel's 6k + 40 and every other length) and trying the certificate on it, against sorting all k' at once and against brute force - random lists,
errors at the edge of the bound, B = 0, exact ties across the cut, all-equal keys, a crowd below the k-th, rows dropped by
the f32 epilogue so that a prefix fails, fewer rows than k', B = +inf - and the prefix length itself."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prefix_certificate_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "tail_prefix_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "tail_prefix_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-1500:])
    lines = p.stdout.splitlines()
    assert lines[0] == "scalars ok" and lines[1] == "rule ok" and lines[-1] == "all ok", lines
    assert lines[2].startswith("random ok 3000") and lines[3] == "adversarial ok 1500", lines


def test_header_is_device_free():
    """tail_prefix.h compiles without HIP: the driver above is the proof for g++; this pins what it may include."""
    src = open(os.path.join(ROOT, "cqs_amd", "csrc", "tail_prefix.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ["<math.h>", "<stdint.h>", "<string.h>", "<hip/hip_runtime.h>"], incs
    assert src.index("#if defined(__HIPCC__)") < src.index("<hip/hip_runtime.h>")
