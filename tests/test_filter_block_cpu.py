"""cqs_hip_index_search_filtered / cqs_hip_index_combine_filter_stats without a GPU: the built library exports them behind
the ABI guard, a null handle is INVALID with the outputs untouched, and the Python mirror checks the bitset array."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cqs_amd import HipIndex, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cqs_hip_index_search_filtered", "cqs_hip_index_combine_filter_stats")


def test_the_library_exports_the_entry_points():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NEW + ("cqs_hip_debug_client_storm_filtered",):
        assert n in names, n
    assert {n for n, _, _ in _lib.SIGNATURES} >= set(NEW)


def test_both_definitions_carry_the_abi_guard():
    src = open(os.path.join(ROOT, "cqs_amd", "csrc", "index.hip")).read()
    for n in NEW:
        m = re.search(r"\b%s\([^)]*\)\s*CQS_ABI_TRY\s*\{" % n, src)
        assert m, f"{n}: no CQS_ABI_TRY at its definition"
        nxt = re.search(r"\)\s*CQS_ABI_TRY\s*\{", src[m.end():])
        body = src[m.end(): m.end() + nxt.start()] if nxt else src[m.end():]
        assert re.search(r"\}\s*CQS_ABI_CATCH", body), f"{n}: no CQS_ABI_CATCH closing its definition"


def test_null_handle_is_invalid_and_touches_nothing():
    lib = _lib.load()
    q = np.ones((2, 8), np.float32)
    bits = np.full((2, 4), 0xFFFFFFFF, np.uint32)
    rows = np.full((2, 3), 77, np.uint64); scores = np.full((2, 3), 5.0, np.float32); counts = np.full((2,), 9, np.uint32)
    rc = lib.cqs_hip_index_search_filtered(None, q.ctypes.data, 2, 8, 3, bits.ctypes.data, 4, 0, 0.0,
                                           rows.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    assert rc == _lib.ERR_INVALID
    assert (rows == 77).all() and (scores == 5.0).all() and (counts == 9).all()
    p, n = C.c_uint64(3), C.c_uint64(4)
    lib.cqs_hip_index_combine_filter_stats(None, C.byref(p), C.byref(n))
    assert (p.value, n.value) == (0, 0)


def test_the_python_mirror_checks_the_bitset_array():
    class Fake(HipIndex):            # no device: the checks run before the library is called
        def __init__(self):
            self._lib, self._h = None, None

        def __len__(self):
            return 100

        def close(self):
            pass

    idx = Fake()
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError):
        idx.search_batch_filtered(q, 5, np.zeros((2, 3), np.uint32))        # 100 rows need 4 words
    with pytest.raises(ValueError):
        idx.search_batch_filtered(q, 5, np.zeros((4,), np.uint32))          # rank 1
    with pytest.raises(ValueError):
        idx.search_batch_filtered(q, 5, np.zeros((3, 4), np.uint32))        # one row per query
