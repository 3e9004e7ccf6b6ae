"""The combining queue (cqs_amd/csrc/combine_queue.h) in a stand-alone program over a toy request, once under ThreadSanitizer and
once under ASAN + UBSan: the lone caller, the oldest-first seal with its overflow, a storm of 8 threads, the two failure
rules (poisoned: riders and everybody parked get POISONED; not poisoned: the block alone fails) and the straggler window
anchored at the end of the previous pass.  No GPU, no library."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {"tsan": ["-fsanitize=thread"], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def run_driver(exe, env):
    """Older ThreadSanitizer runtimes cannot start where the kernel places the program under high-entropy address randomisation
    ("FATAL: ThreadSanitizer: unexpected memory mapping", before main).  So the driver runs without randomisation where the
    machine allows that, and is started again, with a fresh layout, when the runtime still could not start.  A run that
    started counts as it ends."""
    cmd = [str(exe)]
    setarch = shutil.which("setarch")
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        cmd = [setarch, platform.machine(), "-R"] + cmd
    for _ in range(8):
        p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=120)
        if "unexpected memory mapping" not in p.stderr:
            break
    return p


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def got(request, tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("combine_queue_" + request.param) / "combine_queue_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", *SANITIZERS[request.param],
                    os.path.join(ROOT, "tests", "combine_queue_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24",
               TSAN_OPTIONS="halt_on_error=0:exitcode=66")
    p = run_driver(exe, env)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    return {ln.split("|")[0]: ln.split("|")[1:] for ln in p.stdout.splitlines()}


def test_lone_caller_never_waits(got):
    # wait_us is 5 s; expect is 1, so the wait loop is not entered: one block of one, back in under a second
    assert got["lone"] == ["A7", "OK", "1", "1"]


def test_seal_is_oldest_first_and_keeps_the_rest_in_order(got):
    blocks, expects, own, parked = got["seal"]
    # held A0, then A A B A A A B A parked as 1..8: four A's in arrival order, B stays in front of the overflow A's
    assert blocks == "A0;A1,A2,A4,A5;B3,B7;A6,A8"
    # expect while each block runs = its members + the like requests it left behind: the A x 4 seal left two
    assert expects == "1,6,2,2"
    assert (own, parked) == ("9", "0")


def test_storm_every_answer_is_the_callers_own(got):
    own, n_blocks, members, largest, mixed, parked = (int(v) for v in got["storm"])
    assert own == 16000 and members == 16000
    assert 1 <= largest <= 4 and 4000 <= n_blocks <= 16000
    assert mixed == 0 and parked == 0


def test_failure_on_a_poisoned_handle_wakes_everybody(got):
    blocks, rcs, answered, parked, leader = got["poison"]
    assert blocks == "C0;A1,A2,A3"                                  # run is never called for the B's
    assert rcs == "OK,DEVICE,POISONED,POISONED,POISONED,POISONED"   # the oldest A reports it; riders and the parked get POISONED
    assert answered == "100000"
    assert (parked, leader) == ("0", "0")


def test_failure_without_poison_stays_in_its_block(got):
    blocks, rcs, answered, parked, leader = got["nomem"]
    assert blocks == "C0;A1,A2;B3"
    assert rcs == "OK,NOMEM,NOMEM,OK" and answered == "1001"
    assert (parked, leader) == ("0", "0")


def test_straggler_window_is_anchored_at_the_previous_pass_end(got):
    blocks, expect, waited_us, expect2, late_us, wait_us = got["window"]
    assert blocks == "C0;A1,A2,A3,A4;A50;C0;A1,A2,A3,A4;A51"
    assert (expect, expect2, wait_us) == ("4", "4", "300000")
    # right after a burst of 4 a lone caller is sealed no earlier than the window's end (the loop condition, not scheduling) ...
    assert int(waited_us) >= 300000
    # ... and 400 ms after one it does not wait at all
    assert int(late_us) < 300000
