"""The batch tables of both transformer engines and the ticket-context rule, device-free (cqs_amd/csrc/batch_tables.h):
tests/batch_tables_driver.cpp, a stand-alone program built with ASAN + UBSan, fills the blocks of a few hundred batches per
layout kind into allocations of exactly `table_words` and prints them; every word is compared with the numpy restatement of the
layouts in tests/batch_tables_cases.py.  The refusals each have their own code, a refused fill is clean under the sanitizers,
and the two context rules are swept against their restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import batch_tables_cases as btc
from batch_tables_cases import BERT, GEMMA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, TYPE_VOCAB, MAX_LEN = 1000, 3, 300
KINDS = (GEMMA, BERT)


def _fill_line(kind, lens, tok, ty, max_len=MAX_LEN):
    f = ["fill", kind, max_len, VOCAB, TYPE_VOCAB, len(lens), *lens, *tok]
    if kind == BERT:
        f += list(ty)
    return " ".join(str(int(x)) if not isinstance(x, str) else x for x in f)


def _layout_cases():
    rng = np.random.default_rng(0x7AB1E5)
    cases = []
    for kind in KINDS:
        for lens in btc.layout_batches(kind):
            M = sum(lens)
            cases.append((kind, lens, rng.integers(0, VOCAB, size=M), rng.integers(0, TYPE_VOCAB, size=M)))
    return cases


def _bad(kind, lens, at, tok_value=None, ty_value=None):
    """A fill line whose token (or type) at packed row `at` is out of range."""
    M = sum(lens)
    tok, ty = np.full(M, 5), np.full(M, 1)
    if tok_value is not None:
        tok[at] = tok_value
    if ty_value is not None:
        ty[at] = ty_value
    return _fill_line(kind, lens, tok, ty)


REFUSALS = [  # (line, the answer's fields after the command word)
    *[(f"shape {k} {MAX_LEN} 3 5 {MAX_LEN + 1} 7", [btc.TOO_LONG]) for k in KINDS],
    *[(f"shape {k} {MAX_LEN} 3 5 {MAX_LEN} 7", [btc.OK, *btc.expected_shape(k, [5, MAX_LEN, 7])]) for k in KINDS],
    *[(f"shape {k} {0x40000000} 2 {0x40000000} {0x40000000}", [btc.TOO_MANY_TOKENS]) for k in KINDS],      # sum = 0x80000000
    *[(f"shape {k} {0x40000000} 2 {0x40000000} {0x3FFFFFFF}", [btc.OK, 2, 0x7FFFFFFF]) for k in KINDS],     # sum = 0x7FFFFFFF
    *[(_fill_line(k, [5, MAX_LEN + 1], [], []), [btc.TOO_LONG]) for k in KINDS],
    *[(_bad(k, [3, 0, 70], at, tok_value=v), [btc.OK, *btc.expected_shape(k, [3, 0, 70]), "refused", btc.BAD_TOKEN])
      for k in KINDS for at in (0, 72) for v in (-1, VOCAB)],
    *[(_bad(BERT, [3, 0, 70], at, ty_value=v), [btc.OK, *btc.expected_shape(BERT, [3, 0, 70]), "refused", btc.BAD_TYPE])
      for at in (0, 72) for v in (-1, TYPE_VOCAB)],
    ("mask 2 4 8  1 1 0 1  1 0 0 0", [btc.MASK_NOT_PREFIX]),                 # a hole
    ("mask 2 4 8  1 1 0 0  0 1 0 0", [btc.MASK_NOT_PREFIX]),                 # a row that starts with its hole
    ("mask 2 4 3  1 1 1 0  1 1 1 1", [btc.TOO_LONG]),                        # longer than max_seq
    ("mask 3 4 4  1 1 1 1  0 0 0 0  7 -1 0 0", [btc.OK, 4, 0, 2]),           # full, empty, any non-zero counts as set
]
N_CUS = (256, 304, 64)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("batch_tables") / "batch_tables_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "batch_tables_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    lines = [_fill_line(*c) for c in _layout_cases()] + [ln for ln, _ in REFUSALS]
    lines += ["ctx", *[f"rounds {n} 70000" for n in N_CUS], "props 12345 400"]
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    return dict(zip(lines, out))


def test_every_word_of_both_layouts(answers):
    cases = _layout_cases()
    assert len(cases) == 2 * (6 + 5 + 3 + 300)
    for kind, lens, tok, ty in cases:
        got = answers[_fill_line(kind, lens, tok, ty)].split()
        B, M, nblk, vt_cols, words = btc.expected_shape(kind, lens)
        assert got[:7] == ["fill", "0", str(B), str(M), str(nblk), str(vt_cols), str(words)], (kind, lens, got[:7])
        block = np.array(got[7:], np.int64)
        assert block.size == words, (kind, lens)                             # (the driver allocated exactly this many)
        assert np.array_equal(block, btc.expected_block(kind, lens, tok, ty)), (kind, lens)


def test_refusals_have_their_own_codes(answers):
    assert len({btc.TOO_LONG, btc.TOO_MANY_TOKENS, btc.BAD_TOKEN, btc.BAD_TYPE, btc.MASK_NOT_PREFIX, btc.OK}) == 6
    for line, want in REFUSALS:
        got = answers[line].split()
        assert got[0] == line.split()[0]
        assert got[1:1 + len(want)] == [str(w) for w in want], (line[:80], got[:10], want)
        if want[0] != btc.OK or "refused" in want:
            assert len(got) == 1 + len(want), (line[:80], got[:12])           # a refusal hands out no table


def test_layout_properties_under_sanitizers(answers):
    """table_words monotone, carve inside the block / disjoint / adding up to table_words / tok == base at the capacity shape
    and at the batch shape: checked by the driver itself (it exits non-zero otherwise) on 400 random shape pairs per kind, and
    on every filled block above."""
    assert answers["props 12345 400"] == "props ok 400"


def test_pick_context_against_the_restatement(answers):
    want = "".join(str(btc.expected_context(a, b, last)) for a in range(5) for b in range(5) for last in (0, 1))
    assert answers["ctx"] == "ctx " + want
    assert btc.expected_context(0, 0, 0) == 0 and btc.expected_context(0, 0, 1) == 0       # an idle engine takes context 0
    assert want[0] == "0" and want[1] == "0"


def test_exact_rounds_against_the_restatement(answers):
    """Every token count 1..70 000 at 256, 304 and 64 CUs, and the counts the rule's comment names at 256 CUs.

    The engine's expression before this header existed was `wgs >= n_cu && (last == 0 || last * 32 >= n_cu * 31)` with
    wgs = ceil(M / 128) * 2, and the header keeps it bit for bit.  Under it 16 384 - 500 = 15 884 tokens (250 workgroups, fewer
    than the 256 CUs) and 15 745 tokens (248) are NOT pinned: the `wgs >= n_cu` term refuses a single partial round.  The old
    comment claimed 16 384 - 500 "still is" exact rounds; the comment was wrong about its own code and has been corrected.  The
    pair at which the expression does switch below 16 384 is 16 256 (254 workgroups) / 16 257 (256)."""
    for n_cu in N_CUS:
        got = answers[f"rounds {n_cu} 70000"].split()[1]
        want = "".join("1" if btc.expected_exact_rounds(M, n_cu) else "0" for M in range(1, 70001))
        assert got == want, n_cu
    got = answers["rounds 256 70000"].split()[1]
    pinned = {M: got[M - 1] == "1" for M in (16384, 32768, 32768 - 500, 15884, 12288, 14336, 18432, 24576, 15744, 15745, 16256, 16257)}
    assert pinned == {16384: True, 32768: True, 32768 - 500: True, 15884: False, 12288: False, 14336: False, 18432: False,
                      24576: False, 15744: False, 15745: False, 16256: False, 16257: True}


def test_header_is_device_free():
    """batch_tables.h compiles without HIP: the driver is the proof for g++; this pins what it may include."""
    src = open(os.path.join(ROOT, "cqs_amd", "csrc", "batch_tables.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ["<stddef.h>", "<stdint.h>"], incs
    assert "__device__" not in src and "__global__" not in src and "hip_runtime" not in src
