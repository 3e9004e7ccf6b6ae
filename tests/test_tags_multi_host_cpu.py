"""The transposed filter table (cqs_amd/csrc/tags_host.h) in a stand-alone program under ASAN + UBSan:
`transpose_filters` + `tag_verdicts` against the numpy restatement of the per-row rule (tags_cases.keep_mask).  The law:
bit j of tag_verdicts(tag, table) == tag_kept(tag, filter j) for every tag and every j < f, and no table word has a bit
>= f.  Then the new C-ABI symbols without a device.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tags_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = (1, 2, 31, 32)


def filters(tags, f, seed):
    """f filters [f, 32]: tags_cases.filters_for (all-pass, an empty field, single values, half-full, ...) in a seeded
    order, repeated / extended with seeded random half-full ones to reach f."""
    rng = np.random.default_rng(seed)
    named = list(tc.filters_for(tags, seed).values())
    order = rng.permutation(len(named))
    out = [named[i] for i in order][:f]
    while len(out) < f:
        out.append(tc.allow_of(*[[int(v) for v in np.flatnonzero(rng.random(256) < 0.5)] for _ in range(4)]))
    return np.stack(out).astype(np.uint32)


def _cases():
    """name -> (tags, allows [f, 32])."""
    c = {}
    for f in FS:
        for n in (1, 33, 1000):
            tags = tc.unique_end_tags(n, 40 + n)
            c[f"f{f}_n{n}"] = (tags, filters(tags, f, 50 + n + f))
        tags = tc.random_tags(700, 60 + f)
        # the three named kinds at fixed places of one table: all-pass first, an empty field last, single values between
        named = tc.filters_for(tags, 61 + f)
        pick = [named["all_pass"], named["one_value_field_0"], named["one_value_field_3"], named["only_255"], named["empty_field_2"]]
        a = filters(tags, f, 62 + f)
        for slot, flt in zip(np.linspace(0, f - 1, num=min(f, len(pick)), dtype=int), pick if f >= len(pick) else pick[:f]):
            a[slot] = flt
        c[f"f{f}_named"] = (tags, a)
        rng = np.random.default_rng(70 + f)             # fully random tags and filters: every field value 0 .. 255 occurs
        tags = rng.integers(0, 2**32, size=600, dtype=np.uint64).astype(np.uint32)
        a = rng.integers(0, 2**32, size=(f, 32), dtype=np.uint64).astype(np.uint32)
        a |= rng.integers(0, 2**32, size=(f, 32), dtype=np.uint64).astype(np.uint32)
        c[f"f{f}_random"] = (tags, a)
    edge = np.array([0x00000000, 0xFFFFFFFF, 0x000000FF, 0xFF000000, 0x00FF00FF], dtype=np.uint32)
    c["edge_values"] = (edge, np.stack([tc.allow_of([0, 255], [0, 255], [0, 255], [0, 255]), tc.allow_of([0], [0], [0], [0]),
                                        tc.allow_of([255], [255], [255], [255]), tc.ALL]))
    return c


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the stand-alone driver"
    exe = tmp_path_factory.mktemp("tags_multi_host") / "tags_multi_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "tags_multi_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = []
    for name, (tags, allows) in _cases().items():
        lines.append(" ".join(["multi", name, str(len(allows)), str(len(tags))] + [f"{int(t):x}" for t in tags] +
                              [f"{int(a):x}" for a in allows.reshape(-1)]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    out = {ln.split("|")[0]: ln.split("|")[1:] for ln in p.stdout.splitlines()}
    assert len(out) == len(lines)
    return out


def test_verdict_bits_are_the_per_row_rule(got):
    """Against numpy: bit j of a row's verdict word is keep_mask(tags, filter j) - for every row, every j < f."""
    seen_kept = seen_dropped = 0
    for name, (tags, allows) in _cases().items():
        _bad, _high, verdicts = got[name]
        v = np.array([int(w, 16) for w in verdicts.split(",")], dtype=np.uint32)
        assert len(v) == len(tags), name
        for j, allow in enumerate(allows):
            mask = tc.keep_mask(tags, allow)
            assert np.array_equal(((v >> np.uint32(j)) & np.uint32(1)).astype(bool), mask), (name, j)
            seen_kept += int(mask.sum())
            seen_dropped += int((~mask).sum())
        if len(allows) < 32:
            assert not (v >> np.uint32(len(allows))).any(), name       # no verdict for a filter that is not there
    assert seen_kept > 10000 and seen_dropped > 10000                  # the cases exercise both answers


def test_verdicts_agree_with_tag_kept_and_high_bits_are_zero(got):
    """The same law inside the driver, against tags_host.h's own tag_kept; and bits >= f of every table word are zero."""
    for name in _cases():
        bad, high, _verdicts = got[name]
        assert bad == "0", (name, bad)
        assert high == "0", (name, high)


def test_named_filters_in_a_table(got):
    for f in FS:
        tags, allows = _cases()[f"f{f}_named"]
        v = np.array([int(w, 16) for w in got[f"f{f}_named"][2].split(",")], dtype=np.uint32)
        assert (v & np.uint32(1)).all()                                 # slot 0 is all-pass
        if f >= 5:
            assert not ((v >> np.uint32(f - 1)) & np.uint32(1)).any()   # the last slot has an empty field
    v = [int(w, 16) for w in got["edge_values"][2].split(",")]
    assert v == [0b1011, 0b1101, 0b1001, 0b1001, 0b1001]


def test_new_symbols_without_a_device():
    """The library exports the new entry points; a null handle is refused before any device work."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    p, q = C.c_uint64(7), C.c_uint64(7)
    lib.cqs_hip_index_combine_tagged_stats(None, C.byref(p), C.byref(q))
    assert (p.value, q.value) == (0, 0)
    assert lib.cqs_hip_index_search_tagged_multi(None, None, 1, 64, 5, tc.ALL.ctypes.data, 0, 0.0, None, None, None) == _lib.ERR_INVALID
    assert lib.cqs_hip_debug_index_tag_keep_multi(None, tc.ALL.ctypes.data, 1, 0, None, None) == _lib.ERR_INVALID
    assert lib.cqs_hip_debug_client_storm_tagged(None, None, 0, 64, 5, None, 1, 1, None, None, None) < 0
