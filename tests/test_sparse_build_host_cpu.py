"""The device-free half of the sparse index's constructors, search and persistence (cqs_amd/csrc/sparse_build_host.h,
sparse_file_host.h) in a stand-alone program under ASAN + UBSan (tests/sparse_build_host_driver.cpp): the two posting
builders against the from-scratch build in Python (sparse_host_cases.canonical), the directory fill against its definition,
the term resolution of a batch, and the file - written bytes against the Python writer of the format, and the reader's every
refusal of a forged, cut or grown file.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sparse_host_cases import _csr, _docs, _forge_sparse_file, _ranks, canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESERVED = 0xFFFFFFFF
ONE = int(np.float32(1.0).view(np.uint32))
SWITCH = 1 << 24                 # kDenseTokenLimit: token ids all below it take the counting path, else the sort path
MAX_TERMS = 1 << 16              # kMaxTerms


def _fmt(xs):
    return "null" if xs is None else " ".join(str(int(x)) for x in xs)


def _fmt_post(post):
    return " ".join("%d:%d" % (p, w) for p, w in post)


def _shift(docs, by):
    return [[(t + by, w) for t, w in d] for d in docs]


def _docs_line(name, docs, id_rank, off=None, tok=None, w=None, n=None):
    o, t, ww = _csr(docs)
    return "|".join([name, "docs", str(len(docs) if n is None else n), _fmt(o if off is None else off[0]), _fmt(t if tok is None else tok[0]),
                     _fmt(ww if w is None else w[0]), _fmt(id_rank)])


def _postings_map(docs):
    """SpladeIndex::build's loop: token -> [(chunk, weight bits)] in chunk order."""
    m = {}
    for c, d in enumerate(docs):
        for t, w in d:
            m.setdefault(t, []).append((c, w))
    return m


def _inverted_line(name, n, lists, id_rank):
    """lists: [(token, [(chunk, weight bits), ...]), ...] in the order they are handed over."""
    off = [0]
    for _t, l in lists:
        off.append(off[-1] + len(l))
    return "|".join([name, "inverted", str(n), str(len(lists)), _fmt([t for t, _l in lists]), _fmt(off),
                     _fmt([c for _t, l in lists for c, _w in l]), _fmt([w for _t, l in lists for _c, w in l]), _fmt(id_rank)])


def _build_cases(rng):
    """name -> (line, expected status, expected why, expected canonical index or None)"""
    c = {}

    def docs_case(name, docs, ranked_too=True):
        for ranked in ((False, True) if ranked_too else (False,)):
            rk = _ranks(rng, len(docs)) if ranked else None
            c[name + ("_ranked" if ranked else "")] = (_docs_line(name + ("_ranked" if ranked else ""), docs, rk), "ok", "", canonical(docs, rk))

    docs_case("n0", [])
    docs_case("n1", _docs(rng, 1, 5, lo=3))
    docs_case("n1_empty", [[]])
    some = _docs(rng, 14, 6, lo=0, hi=4)
    some[0], some[7], some[13] = [], [], []
    docs_case("documents_without_postings", some)
    docs_case("all_empty", [[], [], []])
    docs_case("token_repeated_in_a_document", [[(5, 1), (5, 2), (7, 3), (5, 4)], [(5, 9)], [(7, 8), (7, 7)]])
    base = _docs(rng, 30, 9, lo=1, hi=5, base=10, step=7)
    docs_case("counting_path", base)
    docs_case("sort_path", _shift(base, SWITCH))                         # every id at or above the switch
    docs_case("last_counted_id", base + [[(SWITCH - 1, ONE)]])           # the largest id of the counting path
    docs_case("first_sorted_id", base + [[(SWITCH, ONE)]])               # one id at the switch sends all of them down the sort path
    docs_case("id_zero_and_all_ones", base + [[(0, ONE), (RESERVED, ONE), (0, 5)]])
    # refusals
    two = [[(1, ONE), (2, ONE)], [(3, ONE)]]
    c["rank_repeat"] = (_docs_line("rank_repeat", two, [1, 1]), "rank", "", None)
    c["rank_past_the_end"] = (_docs_line("rank_past_the_end", two, [0, 2]), "rank", "", None)
    c["csr_null_offsets"] = (_docs_line("csr_null_offsets", two, None, off=[None]), "csr", "null doc_off", None)
    c["csr_start"] = (_docs_line("csr_start", two, None, off=[[1, 2, 3]]), "csr", "doc_off does not start at 0", None)
    c["csr_descending"] = (_docs_line("csr_descending", two, None, off=[[0, 3, 2]]), "csr", "doc_off not ascending", None)
    c["csr_null_tokens"] = (_docs_line("csr_null_tokens", two, None, tok=[None]), "csr", "null tokens / weights", None)
    c["csr_null_weights"] = (_docs_line("csr_null_weights", two, None, w=[None]), "csr", "null tokens / weights", None)
    c["csr_reserved_weight"] = (_docs_line("csr_reserved_weight", [[(1, ONE), (2, RESERVED)]], None), "csr", "reserved NaN payload in a weight", None)
    c["csr_nothing_at_all"] = (_docs_line("csr_nothing_at_all", [], None, off=[None], tok=[None], w=[None]), "ok", "", canonical([], None))
    c["csr_empty_documents_null_payload"] = (_docs_line("csr_empty_documents_null_payload", [[], []], None, tok=[None], w=[None]), "ok", "",
                                             canonical([[], []], None))

    # the postings map as input: the same index as from the documents
    inv_docs = _docs(rng, 25, 8, lo=1, hi=5)
    inv_docs[3] = [(121, 11), (200, 12), (121, 13)]                      # token 200: chunks 3 and 1 alone; 121 twice in chunk 3
    inv_docs[1] = inv_docs[1] + [(200, 14)]
    m = _postings_map(inv_docs)
    for ranked in (False, True):
        rk = _ranks(rng, 25) if ranked else None
        s = "_ranked" if ranked else ""
        keys = [int(k) for k in rng.permutation(sorted(m))]
        lists = [(k, list(m[k])) for k in keys]
        c["inverted_keys_in_random_order" + s] = (_inverted_line("inverted_keys_in_random_order" + s, 25, lists, rk), "ok", "", canonical(inv_docs, rk))
        lists = [(k, list(m[k])) for k in keys]
        at = keys.index(200)
        lists[at] = (200, [(3, 12), (1, 14)])                             # descending
        other = next(i for i, (k, l) in enumerate(lists) if k != 200 and len({ch for ch, _w in l}) == len(l) and len(l) >= 3)
        lists[other] = (lists[other][0], lists[other][1][::-1])           # (distinct chunks: reversing keeps every chunk's own order)
        c["inverted_list_not_ascending" + s] = (_inverted_line("inverted_list_not_ascending" + s, 25, lists, rk), "ok", "", canonical(inv_docs, rk))
        # a chunk's two postings under one token keep their order through the sort: 121 of chunk 3 handed over in front
        lists = [(k, list(m[k])) for k in keys]
        at = keys.index(121)
        mine = [p for p in lists[at][1] if p[0] == 3]
        lists[at] = (121, mine + [p for p in lists[at][1] if p[0] != 3])
        c["inverted_stable_inside_a_chunk" + s] = (_inverted_line("inverted_stable_inside_a_chunk" + s, 25, lists, rk), "ok", "", canonical(inv_docs, rk))
        lists = [(k, list(m[k])) for k in keys]
        lists[0] = (lists[0][0], [(25, 5)] + lists[0][1][:1] + [(4000000000, 6)] + lists[0][1][1:] + [(26, 7)])
        lists.insert(2, (77, [(25, 1), (99, 2)]))                         # only chunks past the end: no list, token 77 unknown
        lists.append((5, []))                                             # an empty list: no list either
        c["inverted_chunks_past_the_end" + s] = (_inverted_line("inverted_chunks_past_the_end" + s, 25, lists, rk), "ok", "", canonical(inv_docs, rk))
        lists = [(k, list(m[k])) for k in keys] + [(keys[4], [(0, ONE)])]
        c["inverted_key_twice" + s] = (_inverted_line("inverted_key_twice" + s, 25, lists, rk), "twice", "", None)
    c["inverted_nothing"] = (_inverted_line("inverted_nothing", 0, [], None), "ok", "", canonical([], None))
    c["inverted_bad_rank"] = (_inverted_line("inverted_bad_rank", 2, [(1, [(0, ONE)])], [0, 0]), "rank", "", None)
    c["inverted_reserved_weight"] = (_inverted_line("inverted_reserved_weight", 2, [(1, [(0, RESERVED)])], None), "csr",
                                     "reserved NaN payload in a weight", None)
    return c


def _dirs_docs():
    """300 chunks; token 1 in 31 of them (no directory), token 2 in 32 (the shortest list with one), token 3 in 199 with one
    chunk naming it twice (200 postings)."""
    rng = np.random.default_rng(300)
    docs = [[] for _ in range(300)]
    for t, cnt in ((1, 31), (2, 32), (3, 199)):
        for ch in sorted(int(x) for x in rng.choice(300, size=cnt, replace=False)):
            docs[ch].append((t, ONE + t))
    twice = next(i for i, d in enumerate(docs) if any(t == 3 for t, _w in d))
    docs[twice].append((3, ONE))
    docs[299].append((4, ONE))                                            # the last chunk holds a posting
    return docs


def _resolve_cases(rng):
    docs = _docs(rng, 60, 4, lo=2, hi=4)                                  # ids 100, 103, 106, 109: lists long enough for directories
    off, tok, w = _csr(docs)
    head = [str(len(docs)), _fmt(off), _fmt(tok), _fmt(w)]
    c = {}

    def case(name, queries, status="ok", why="", q_off=None, q_tok=0, q_w=0, b=None):
        qo = [0]
        for q in queries:
            qo.append(qo[-1] + len(q))
        qt = [t for q in queries for t, _w in q]
        qw = [x for q in queries for _t, x in q]
        line = "|".join([name, "resolve"] + head + [str(len(queries) if b is None else b), _fmt(qo if q_off is None else q_off),
                                                    _fmt(qt if q_tok == 0 else q_tok), _fmt(qw if q_w == 0 else q_w)])
        c[name] = (line, status, why, queries)

    case("mixed_batch", [[(101, 5), (1, 6), (999999, 7), (100, 8), (RESERVED, 9)], [], [(2, 1), (104, 2)], [(109, 3), (103, 4), (109, 5)]])
    case("nothing_resolves", [[(101, 5)], [(0, 6), (110, 7)]])
    case("empty_queries_only", [[], []])
    case("one_term", [[(106, ONE)]])
    case("reserved_query_weight", [[(100, ONE)], [(103, ONE), (999, RESERVED)]], "terms", "reserved NaN payload in a query weight")
    case("too_many_terms", [[(100 + 3 * (i % 4), ONE) for i in range(MAX_TERMS + 1)]], "queries", "too many query terms")
    case("most_terms_allowed", [[(100 + 3 * (i % 5), ONE) for i in range(MAX_TERMS)]])
    case("offsets_descending", [[(100, ONE)] * 3, [(103, ONE)] * 2], "queries", "query offsets not ascending", q_off=[3, 5, 4])
    case("too_many_queries", [[(100, ONE)]] * 65, "queries", "more than 64 queries in a batch")
    case("most_queries_allowed", [[(100, ONE)]] * 64)
    case("null_tokens", [[(100, ONE)]], "queries", "null query", q_tok=None)
    case("null_weights", [[(100, ONE)]], "queries", "null query", q_w=None)
    case("null_arrays_without_terms", [[], []], q_tok=None, q_w=None)
    return docs, c


GOOD = dict(chunks=6, tok=[3, 9], off=[0, 3, 5], post=[(0, ONE), (2, ONE), (5, ONE), (1, ONE), (2, ONE)])
# every defect of test_sparse_index_gpu.py::test_loader_rejects_forged_structure, and the step that has to refuse it
FORGED = {
    "position past the end": (dict(GOOD, post=[(0, ONE), (2, ONE), (6, ONE), (1, ONE), (2, ONE)]), "structure"),
    "descending list": (dict(GOOD, post=[(2, ONE), (0, ONE), (5, ONE), (1, ONE), (2, ONE)]), "structure"),
    "offsets do not tile": (dict(GOOD, off=[0, 4, 4]), "structure"),
    "offsets run past the postings": (dict(GOOD, off=[0, 6, 5]), "structure"),
    "repeated token": (dict(GOOD, tok=[3, 3]), "structure"),
    "descending tokens": (dict(GOOD, tok=[9, 3]), "structure"),
    "reserved weight pattern": (dict(GOOD, post=[(0, ONE), (2, RESERVED), (5, ONE), (1, ONE), (2, ONE)]), "structure"),
    "rank repeats": (dict(GOOD, rank=[0, 1, 2, 3, 4, 4]), "structure"),
    "rank past the end": (dict(GOOD, rank=[0, 1, 2, 3, 4, 9]), "structure"),
    "checksum": (dict(GOOD, fix_checksum=False), "sections"),
    "good": (GOOD, "ok"),
    "good ranked": (dict(GOOD, rank=[5, 4, 3, 2, 1, 0]), "ok"),
}


def _file_cases(rng):
    """The written files: ranked and unranked, an odd and an even number of tokens, an odd number of chunks - every pad path."""
    c = {}
    for vocab in (7, 8):
        for ranked in (False, True):
            docs = _docs(rng, 71, vocab, lo=vocab, hi=vocab + 3)
            for i in range(vocab):
                docs[i] = docs[i] + [(100 + 3 * i, ONE)]                  # every token of the vocabulary is there
            rk = _ranks(rng, 71) if ranked else None
            n, tok, off, post, cor = canonical(docs, rk)
            assert len(tok) == vocab and n % 2 == 1
            c["file_%dtokens%s" % (vocab, "_ranked" if ranked else "")] = dict(n=n, tok=tok, off=off, post=post, rank=cor if ranked else None)
    c["file_empty"] = dict(n=0, tok=[], off=[0], post=[], rank=None)
    c["file_empty_ranked"] = dict(n=0, tok=[], off=[0], post=[], rank=[])
    return c


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("sparse_build_host")
    exe = tmp / "sparse_build_host_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "sparse_build_host_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    rng = np.random.default_rng(19)
    build = _build_cases(rng)
    dirs_docs = _dirs_docs()
    off, tok, w = _csr(dirs_docs)
    resolve_docs, resolve = _resolve_cases(rng)
    files = _file_cases(rng)
    lines = [v[0] for v in build.values()]
    lines.append("|".join(["dirs", "dirs", "300", "256", _fmt(off), _fmt(tok), _fmt(w)]))
    lines += [v[0] for v in resolve.values()]
    GEN = 5
    for name, f in files.items():
        lines.append("|".join([name, "write", str(tmp / (name + ".bin")), "1" if f["rank"] is not None else "0", str(f["n"]), str(GEN),
                               _fmt(f["tok"]), _fmt(f["off"]), _fmt_post(f["post"]), _fmt(f["rank"] or [])]))
        lines.append("|".join([name + "/back", "read", str(tmp / (name + ".bin")), str(f["n"]), str(GEN)]))
    for name, (spec, _stage) in FORGED.items():
        _forge_sparse_file(tmp / (name + ".bin"), **spec)
        lines.append("|".join(["forged/" + name, "read", str(tmp / (name + ".bin")), "0", "1"]))
    _forge_sparse_file(tmp / "good.bin", **GOOD)
    raw = (tmp / "good.bin").read_bytes()
    other = {"truncated": raw[:-16], "cut inside the header": raw[:40], "empty file": b"", "grown by 8 bytes": raw + b"\0" * 8,
             "bad magic": b"NOTASPDX" + raw[8:], "version 2": raw[:8] + b"\x02" + raw[9:], "ranked flag 2": raw[:12] + b"\x02" + raw[13:]}
    for name, data in other.items():
        (tmp / (name + ".bin")).write_bytes(data)
        lines.append("|".join(["header/" + name, "read", str(tmp / (name + ".bin")), "0", "1"]))
    lines.append("|".join(["header/wrong generation", "read", str(tmp / "good.bin"), "0", "2"]))
    lines.append("|".join(["header/another chunk count", "read", str(tmp / "good.bin"), "7", "1"]))
    lines.append("|".join(["header/expected chunks", "read", str(tmp / "good.bin"), "6", "1"]))
    lines.append("|".join(["header/missing", "read", str(tmp / "nothing.bin"), "0", "1"]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:exitcode=24")
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    out = {}
    for ln in p.stdout.splitlines():
        f = ln.split("|")
        out[f[0]] = f[1:]
    assert len(out) == len(lines)
    return dict(out=out, build=build, dirs_docs=dirs_docs, resolve=resolve, resolve_docs=resolve_docs, files=files, tmp=tmp, gen=GEN)


def _ints(s):
    return [int(x) for x in s.split()]


def _post(s):
    return [tuple(int(y) for y in x.split(":")) for x in s.split()]


def _index(f):
    """(n, tokens, offsets, postings, chunk_of_rank) of a printed index: fields n|tokens|offsets|postings|chunk_of_rank"""
    return int(f[0]), _ints(f[1]), _ints(f[2]), _post(f[3]), _ints(f[4])


def _check_build(run, names):
    assert names
    for name in names:
        _line, status, why, want = run["build"][name]
        got = run["out"][name]
        assert (got[0], got[1]) == (status, why), (name, got[:2])
        if want is not None:
            assert _index(got[2:7]) == want, name
        else:
            assert _index(got[2:7])[1:4] == ([], [], []), name             # a refusal builds nothing


def test_from_documents_equals_the_python_build(run):
    _check_build(run, [n for n in run["build"] if not n.startswith(("inverted", "csr", "rank"))])
    n, tok, off, post, _ = _index(run["out"]["token_repeated_in_a_document"][2:7])
    assert tok == [5, 7] and post[:4] == [(0, 1), (0, 2), (0, 4), (1, 9)] and post[4:] == [(0, 3), (2, 8), (2, 7)]   # document order kept


def test_both_token_table_paths_build_the_same_arrays(run):
    for s in ("", "_ranked"):
        a, b = _index(run["out"]["counting_path" + s][2:7]), _index(run["out"]["sort_path" + s][2:7])
        assert [t + SWITCH for t in a[1]] == b[1] and a[2] == b[2]
    a, b = _index(run["out"]["counting_path"][2:7]), _index(run["out"]["sort_path"][2:7])
    assert a[3] == b[3] and a[3]                                          # (the ranked pair draws two id orders)
    assert _index(run["out"]["last_counted_id"][2:7])[1][-1] == SWITCH - 1
    assert _index(run["out"]["first_sorted_id"][2:7])[1][-1] == SWITCH
    t = _index(run["out"]["id_zero_and_all_ones"][2:7])[1]
    assert t[0] == 0 and t[-1] == RESERVED


def test_every_refusal_of_the_constructors_arguments(run):
    names = [n for n in run["build"] if n.startswith(("csr", "rank"))]
    assert len(names) == 10
    _check_build(run, names)


def test_from_inverted_equals_from_documents(run):
    _check_build(run, [n for n in run["build"] if n.startswith("inverted")])
    for s in ("", "_ranked"):
        assert 77 not in _index(run["out"]["inverted_chunks_past_the_end" + s][2:7])[1]
        assert run["out"]["inverted_key_twice" + s][0] == "twice"


def test_directories_by_their_definition(run):
    status, _why, rw, n_pad, used, dir_off, dirs, off, post = run["out"]["dirs"][:9]
    rw, n_pad, off, post, dirs = int(rw), int(n_pad), _ints(off), _post(post), _ints(dirs)
    assert status == "ok" and rw == 64 and n_pad == 1024
    R1 = n_pad // rw + 1
    lens = [off[t + 1] - off[t] for t in range(len(off) - 1)]
    assert lens == [31, 32, 200, 1]
    dir_off = dir_off.split()
    assert dir_off == ["-", str(R1), "0", "-"]                            # longest first; 31 postings: none
    assert int(used) == 2 * R1 == len(dirs)
    for t in (1, 2):
        mine = [p for p, _w in post[off[t]:off[t + 1]]]
        want = [sum(1 for p in mine if p < r * rw) for r in range(R1)]
        assert dirs[int(dir_off[t]):int(dir_off[t]) + R1] == want, t
        assert want[0] == 0 and want[-1] == lens[t] and len(set(want)) > 3    # several ranges hold postings


def test_terms_resolve_like_a_lookup_in_the_token_table(run):
    n, tok, off, _post_, _ = canonical(run["resolve_docs"], None)
    for name, (_line, status, why, queries) in run["resolve"].items():
        g = run["out"][name]
        assert (g[0], g[1]) == (status, why), (name, g[:2])
        if status != "ok":
            assert g[2] == "" and g[3] == "", name
            continue
        assert _ints(g[5]) == tok and _ints(g[6]) == off
        dir_off = g[7].split()
        assert any(d != "-" for d in dir_off)
        want_terms, want_qoff, touched = [], [], 0
        for q in queries:
            want_qoff.append(len(want_terms))
            for t, w in q:
                if t in tok and off[tok.index(t) + 1] > off[tok.index(t)]:
                    s = tok.index(t)
                    want_terms.append("%d:%s:%d:%d" % (off[s], dir_off[s], off[s + 1] - off[s], w))
                    touched += off[s + 1] - off[s]
        want_qoff.append(len(want_terms))
        assert _ints(g[2]) == want_qoff and g[3].split() == want_terms and int(g[4]) == touched, name
    assert _ints(run["out"]["mixed_batch"][2]) == [0, 1, 1, 1, 4]
    assert _ints(run["out"]["nothing_resolves"][2]) == [0, 0, 0] and run["out"]["nothing_resolves"][3] == ""


def test_written_bytes_are_the_python_writers(run):
    for name, f in run["files"].items():
        assert run["out"][name][0] == "ok", name
        want = run["tmp"] / (name + ".forged")
        _forge_sparse_file(want, f["n"], f["tok"], f["off"], f["post"], rank=f["rank"], generation=run["gen"])
        got = (run["tmp"] / (name + ".bin")).read_bytes()
        assert got == want.read_bytes(), name
        assert int(run["out"][name][2]) == int.from_bytes(got[48:56], "little")       # the checksum handed back
        back = run["out"][name + "/back"]
        assert back[0] == "ok" and int(back[2]) == (1 if f["rank"] is not None else 0), name
        assert _index(back[3:8]) == (f["n"], f["tok"], f["off"], f["post"], f["rank"] or []), name


def test_reader_refuses_every_forged_cut_or_grown_file(run):
    for name, (spec, stage) in FORGED.items():
        g = run["out"]["forged/" + name]
        assert g[0] == stage, (name, g[0])
        if stage == "ok":
            assert _index(g[3:8]) == (6, spec["tok"], spec["off"], spec["post"], spec.get("rank") or [])
        else:
            assert _index(g[3:8]) == (0, [], [], [], [])
    for name in ("truncated", "cut inside the header", "empty file", "grown by 8 bytes", "bad magic", "version 2", "ranked flag 2",
                 "wrong generation", "another chunk count"):
        assert run["out"]["header/" + name][0] == "header", name
    assert run["out"]["header/expected chunks"][0] == "ok"
    assert run["out"]["header/missing"][0] == "open"
