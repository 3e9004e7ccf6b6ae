"""The ticket pool of the two transformer engines (cqs_amd/csrc/ticket_pool.h) in a stand-alone program over a toy payload,
once under ThreadSanitizer and once under ASAN + UBSan: slots fill up and are refused, ticket numbers are never reused, the
context sequence of batch_tables.h's rule, who may collect a ticket, the reserved slot's wait and wake-up between two threads,
and a storm of 8 threads; plus the weights' bf16 rounding (engine_common.h) on the inputs where two spellings of its NaN
test could differ.  Every expected value is written out by hand.  No GPU, no library."""
import os
import shutil
import subprocess

import pytest

from test_combine_queue_cpu import ROOT, SANITIZERS, run_driver

ROUNDS = 2000                                           # per thread of the storm (the driver's default)


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def got(request, tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("ticket_pool_" + request.param) / "ticket_pool_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", *SANITIZERS[request.param],
                    os.path.join(ROOT, "tests", "ticket_pool_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24",
               TSAN_OPTIONS="halt_on_error=0:exitcode=66")
    p = run_driver(exe, env)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    return {ln.split("|")[0]: ln.split("|")[1:] for ln in p.stdout.splitlines()}


def test_slots_fill_up_are_refused_and_numbers_are_never_reused(got):
    tickets, fourth, reserved_slot, own, next_ticket, next_slot, slot_of_2 = got["fill"]
    assert tickets == "1,2,3" and fourth == "none"
    assert reserved_slot == "3"                         # with every ticket slot in flight the reserved one is still there
    assert own == "1"                                   # ticket 2 collects to what its submit wrote
    assert (next_ticket, next_slot, slot_of_2) == ("4", "1", "1")


def test_context_sequences_follow_the_rule_of_batch_tables(got):
    pipelined, blocking, forced = got["contexts"]
    assert pipelined == "0,1,0,1"                       # fewer in flight wins; a tie alternates; an idle pool takes 0
    assert blocking == "0,0,0,0"                        # one call at a time: always the same context
    assert forced == "0,0,1"                            # force0 on the second submit: it goes to 0, the third to the emptier 1


def test_one_collector_per_ticket_and_only_of_its_kind(got):
    answers, in_flight = got["collect"]
    # ticket 0, a never-issued ticket, the other kind, the first collector, a second one meanwhile, the same ticket once released
    assert answers == "unknown,unknown,unknown,ok,busy,unknown"
    assert in_flight == "0"


def test_reserved_slot_blocks_a_second_thread_until_the_first_collects(got):
    blocked, ticket_a, ticket_b, own_a, own_b, in_flight = got["reserved"]
    assert blocked == "1"
    assert (ticket_a, ticket_b) == ("1", "2")
    assert (own_a, own_b, in_flight) == ("1", "1", "0")


def test_storm_every_collect_reads_its_own_submit(got):
    expected, own, distinct, in_flight = (int(v) for v in got["storm"])
    assert expected == 8 * ROUNDS == 16000
    assert own == 16000 and distinct == 16000 and in_flight == 0


def test_bf16_rounding_ties_to_even_and_keeps_every_nan_a_nan(got):
    # +0, -0, 1.0, the ties 0x3F808000 (down to even) and 0x3F818000 (up to even), +inf, a quiet NaN, the signalling NaN 0x7F800001
    assert got["bf16"] == ["0000,8000,3F80,3F80,3F82,7F80,7FC0,7FC0"]
