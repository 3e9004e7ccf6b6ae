"""The device-free plan of cqs_hip_sparse_index_remove / _extend (cqs_amd/csrc/sparse_update_host.h) in a stand-alone
program under ASAN + UBSan: validation, renumbering of chunks and ranks, the new token table, and the three position rules
the kernels implement, replayed over host arrays (tests/sparse_update_host_driver.cpp).  Every result is compared with a
from-scratch build, written here in Python, of the resulting documents with the resulting id order.
Then the C ABI's two new symbols without a device.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from sparse_host_cases import _csr, _docs, _ranks, canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOTHING, UPDATE = -1, 0, 1
RESERVED = 0xFFFFFFFF


def expect_remove(docs, id_rank, chunks):
    gone = sorted(set(chunks))
    keep = [i for i in range(len(docs)) if i not in set(gone)]
    new_rank = None
    if id_rank is not None:
        new_rank = [int(x) for x in np.argsort(np.argsort(np.asarray([id_rank[i] for i in keep], dtype=np.int64)))]
    return canonical([docs[i] for i in keep], new_rank)


def expect_extend(docs, id_rank, new_docs, new_rank):
    n_old, total = len(docs), len(docs) + len(new_docs)
    rank = None
    if id_rank is not None:
        if new_rank is None:
            rank = list(id_rank) + list(range(n_old, total))
        else:
            free = sorted(set(range(total)) - set(new_rank))     # the existing chunks keep their relative order in these
            rank = [free[r] for r in id_rank] + list(new_rank)
    return canonical(docs + new_docs, rank)


def _cases():
    c = {}
    rng = np.random.default_rng(7)
    docs = _docs(rng, 40, 12, lo=1)
    docs[5] = docs[5] + [(7, 1), (7, 2)]           # token 7 lives in chunks 5, 6 and 30 alone: it dies with them
    docs[6] = [(7, 3)] + docs[6]
    docs[30] = [(7, 4)]
    for ranked in (False, True):
        rk = _ranks(rng, 40) if ranked else None
        s = "_ranked" if ranked else ""

        def rem(name, chunks, m=None, d=docs, r=rk):
            c[name + s] = dict(kind="remove", docs=d, id_rank=r, chunks=chunks, m=m)
        rem("unsorted_dups", [31, 3, 3, 17, 31, 4, 39, 3])
        rem("first", [0])
        rem("last", [39])
        rem("every", list(range(40)))
        rem("none_empty_list", [])
        rem("none_null", None, 0)
        rem("every_second", list(range(0, 40, 2)))
        rem("dying_token", [30, 5, 6])
        one = _docs(rng, 1, 4, lo=2)
        rem("one_chunk_index", [0], d=one, r=[0] if ranked else None)
        for i, frac in enumerate((0.05, 0.3, 0.6, 0.95)):
            nn = int(rng.integers(60, 200))
            dd = _docs(rng, nn, 25)
            rem(f"random_{i}", [int(x) for x in rng.choice(nn, size=max(1, int(nn * frac)), replace=False)], d=dd,
                r=_ranks(rng, nn) if ranked else None)
        rem("out_of_range", [3, 40])
        rem("null_chunks", None, 3)

        def ext(name, new_docs, new_rank=None, d=docs, r=rk, null=False):
            c[name + s] = dict(kind="extend", docs=d, id_rank=r, new_docs=new_docs, new_rank=new_rank if ranked or name.startswith("bad_") else None,
                               null=null)
        ext("one_doc", _docs(rng, 1, 12, lo=3), [20])
        ext("doubling", _docs(rng, 40, 12), [int(x) for x in rng.choice(80, size=40, replace=False)])
        ext("empty_doc", [[]], [11])
        ext("tokens_below", [[(1, 5), (2, 6)]], [0])                      # below every existing token id (>= 7)
        ext("tokens_above", [[(4000000000, 5), (RESERVED, 6)]], [40])
        ext("tokens_between", [[(101, 5), (104, 6), (104, 7)]], [7])      # existing ids are 100, 103, 106, ...
        ext("ranks_in_front", _docs(rng, 5, 12, lo=1), [4, 0, 2, 1, 3])
        ext("ranks_behind", _docs(rng, 5, 12, lo=1), [44, 40, 42, 41, 43])
        ext("ranks_every_other", _docs(rng, 40, 12, lo=1), list(range(1, 80, 2)))
        ext("ranks_one_block", _docs(rng, 6, 12, lo=1), [15, 13, 12, 14, 17, 16])
        ext("repeated_token", [[(103, 1), (103, 2), (106, 3), (103, 4)], [(103, 9), (103, 8)]], [9, 8])
        ext("rank_null", _docs(rng, 7, 12), None)
        ext("after_remove_everything", _docs(rng, 9, 12, lo=1), [int(x) for x in rng.permutation(9)], d=[], r=[] if ranked else None)
        ext("nothing", [], None)
        ext("bad_doc_off_descending", [[(1, 1), (2, 2)], [(3, 3)]], None, null="descending")
        ext("bad_doc_off_start", [[(1, 1)]], None, null="start")
        ext("bad_null_tokens", [[(1, 1)]], None, null="tokens")
        ext("bad_reserved_nan", [[(1, RESERVED)]], [3] if ranked else None)
    rk = c["one_doc_ranked"]["id_rank"]
    c["bad_rank_twice"] = dict(kind="extend", docs=docs, id_rank=rk, new_docs=[[(1, 1)], [(2, 2)]], new_rank=[5, 5], null=False)
    c["bad_rank_range"] = dict(kind="extend", docs=docs, id_rank=rk, new_docs=[[(1, 1)], [(2, 2)]], new_rank=[5, 42], null=False)
    c["bad_rank_unranked"] = dict(kind="extend", docs=docs, id_rank=None, new_docs=[[(1, 1)]], new_rank=[5], null=False)
    return c


CASES = _cases()


def _fmt(xs):
    return "null" if xs is None else " ".join(str(int(x)) for x in xs)


def _line(name, c):
    off, tok, w = _csr(c["docs"])
    head = [name, c["kind"], str(len(c["docs"])), _fmt(off), _fmt(tok), _fmt(w), _fmt(c["id_rank"])]
    if c["kind"] == "remove":
        return "|".join(head + [_fmt(c["chunks"]), str(len(c["chunks"]) if c["m"] is None else c["m"])])
    noff, ntok, nw = _csr(c["new_docs"])
    if c["null"] == "descending":
        noff = [0, 2, 1]
    elif c["null"] == "start":
        noff = [1, 2]
    elif c["null"] == "tokens":
        ntok = None
    if not c["new_docs"]:
        noff = None
    return "|".join(head + [str(len(c["new_docs"])), _fmt(noff), _fmt(ntok), _fmt(nw), _fmt(c["new_rank"])])


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("sparse_update_host") / "sparse_update_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "sparse_update_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    text = "\n".join(_line(name, c) for name, c in CASES.items()) + "\n"
    p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    out = {}
    for ln in p.stdout.splitlines():
        name, plan, why, n, tok, off, post, cor, checks = ln.split("|")
        out[name] = dict(plan=int(plan), why=why, checks=checks,
                         index=(int(n), [int(x) for x in tok.split()], [int(x) for x in off.split()],
                                [tuple(int(y) for y in x.split(":")) for x in post.split()], [int(x) for x in cor.split()]))
    assert set(out) == set(CASES)
    return out


def _both(name):
    return (name, name + "_ranked")


def _check_updated(got, name):
    c, g = CASES[name], got[name]
    want = expect_remove(c["docs"], c["id_rank"], c["chunks"]) if c["kind"] == "remove" else \
        expect_extend(c["docs"], c["id_rank"], c["new_docs"], c["new_rank"])
    assert g["plan"] == UPDATE and g["checks"] == "1", (name, g["plan"], g["why"], g["checks"])
    assert g["index"] == want, name


def _check_untouched(got, name, plan, why=None):
    c, g = CASES[name], got[name]
    assert g["plan"] == plan and g["checks"] == "1", (name, g["plan"], g["why"], g["checks"])     # checks: nothing planned
    if why is not None:
        assert g["why"] == why, (name, g["why"])
    assert g["index"] == canonical(c["docs"], c["id_rank"]), name


def test_remove_patterns(got):
    for base in ("unsorted_dups", "first", "last", "every_second", "one_chunk_index"):
        for name in _both(base):
            _check_updated(got, name)
    n, tok, off, post, cor = got["unsorted_dups_ranked"]["index"]
    assert n == 35 and len(cor) == 35 and sorted(cor) == list(range(35))


def test_remove_everything_and_nothing(got):
    for name in _both("every"):
        _check_updated(got, name)
        assert got[name]["index"] == (0, [], [0], [], [])
    for base in ("none_empty_list", "none_null"):
        for name in _both(base):
            _check_untouched(got, name, NOTHING)


def test_a_token_dies_with_its_chunks(got):
    for name in _both("dying_token"):
        _check_updated(got, name)
        assert 7 in canonical(CASES[name]["docs"], CASES[name]["id_rank"])[1]
        assert 7 not in got[name]["index"][1]


def test_random_removals(got):
    for i in range(4):
        for name in _both(f"random_{i}"):
            _check_updated(got, name)


def test_extend_documents(got):
    for base in ("one_doc", "doubling", "empty_doc", "repeated_token", "rank_null", "after_remove_everything"):
        for name in _both(base):
            _check_updated(got, name)
    for name in _both("nothing"):
        _check_untouched(got, name, NOTHING)
    # the repeated token's postings stay separate and in document order inside their chunk
    n, tok, off, post, _ = got["repeated_token"]["index"]
    s = tok.index(103)
    mine = [w for pos, w in post[off[s]:off[s + 1]] if pos == 40]
    assert mine == [1, 2, 4]


def test_extend_new_tokens_anywhere_in_the_table(got):
    for base in ("tokens_below", "tokens_above", "tokens_between"):
        for name in _both(base):
            _check_updated(got, name)
    assert got["tokens_below"]["index"][1][:2] == [1, 2]
    assert got["tokens_above"]["index"][1][-2:] == [4000000000, RESERVED]
    t = got["tokens_between"]["index"][1]
    assert t.index(101) == t.index(100) + 1 and t.index(104) == t.index(103) + 1


def test_extend_rank_patterns(got):
    for base in ("ranks_in_front", "ranks_behind", "ranks_every_other", "ranks_one_block"):
        for name in _both(base):
            _check_updated(got, name)
    cor = got["ranks_in_front_ranked"]["index"][4]
    assert sorted(cor[:5]) == [40, 41, 42, 43, 44]
    cor = got["ranks_every_other_ranked"]["index"][4]
    assert all(c >= 40 for c in cor[1::2]) and all(c < 40 for c in cor[0::2])


def test_refusals_plan_nothing(got):
    for name in _both("out_of_range"):
        _check_untouched(got, name, INVALID, "chunk index not in this index")
    for name in _both("null_chunks"):
        _check_untouched(got, name, INVALID, "null chunks")
    for name in _both("bad_doc_off_descending"):
        _check_untouched(got, name, INVALID, "doc_off not ascending")
    for name in _both("bad_doc_off_start"):
        _check_untouched(got, name, INVALID, "doc_off does not start at 0")
    for name in _both("bad_null_tokens"):
        _check_untouched(got, name, INVALID, "null tokens / weights")
    for name in _both("bad_reserved_nan"):
        _check_untouched(got, name, INVALID, "reserved NaN payload in a weight")
    _check_untouched(got, "bad_rank_twice", INVALID, "new_rank given twice")
    _check_untouched(got, "bad_rank_range", INVALID, "new_rank out of range")
    _check_untouched(got, "bad_rank_unranked", INVALID, "new_rank on an index created without id_rank")


def test_update_symbols_without_a_device():
    """The library exports both entry points; a null handle is refused before any device work."""
    import __graft_entry__ as g
    g.build()
    from cqs_amd import _lib
    lib = _lib.load()
    chunks = np.array([1, 2], dtype=np.uint64)
    removed = C.c_uint64(7)
    assert lib.cqs_hip_sparse_index_remove(None, chunks.ctypes.data, 2, C.byref(removed)) == _lib.ERR_INVALID
    assert removed.value == 7
    off = np.array([0, 1], dtype=np.uint64)
    tok = np.array([5], dtype=np.uint32)
    w = np.array([1.0], dtype=np.float32)
    assert lib.cqs_hip_sparse_index_extend(None, off.ctypes.data, tok.ctypes.data, w.ctypes.data, 1, None) == _lib.ERR_INVALID
