"""Seeded operation walks over one dense index handle ("Operation walks"): the exact row source, the model a
walk is checked against, the generator of the walks and the per-step checks.  No GPU and no library here:
tests/test_walk_gpu.py drives a `HipIndex` through these functions, tests/test_walk_cases_cpu.py drives a numpy handle with
planted faults through the same ones and holds the model to the oracle.

Data.  The rows and queries have the properties of `exact_cases.dyadic`: entries are small integers times 2^-e, every
product and every partial sum is an exact f32 in any order, and every total is odd (never +0 / -0).  Column 0 is odd on both
sides; every other base column of a ROW is even, so the queries' other columns may be anything - and the dot of two rows is
odd as well, which the kNN checks need (`knn_cases` has the same rule).

Groups instead of windows.  A row range does not survive a removal, so the boost travels in the row: the last W columns
are reserved, a row of group g holds the boost in reserved column g, query i aims at group i % W.  boost^2 exceeds twice
the largest base |score| over the whole pool a walk draws from (asserted), so the unfiltered top-|group| of a query is
exactly its group, wherever the group's rows lie after removes and renumbering, with a clear gap below it.
"""
import math

import numpy as np

import exact_cases as X
import knn_cases as K
import tags_cases as T

W = 8                      # groups = reserved columns
NQ = 40                    # queries of a walk: the largest block the checks send
MAX_ROWS = 6000
MAX_K = X.MAX_K
MODE_RAW, MODE_PIPELINE = 0, 1
EDGES = (0, 1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
REMOVE_PATTERNS = ("one", "row0", "last", "block", "every_second", "random30", "all")
UPDATE_PATTERNS = ("one", "row0", "last", "block", "every_second", "random30", "all")
KNN_LIMIT = 15
KNN_EVERY = 4
STEPS = 40                 # more than any program holds: the walks of both test files run to their end


class Flavour:
    """What a walk's handle is and supports.  program: "up" / "down" by seed for the full walks, "short" (edges up to
    1025: the 768-dimensional handle with string ids), "sharded" (extend, update, save / load and the refused calls)."""

    def __init__(self, name, dim, dot=False, row_base=0, ids=False, tags=True, sharded=False, program="full", max_edge=4097):
        self.name, self.dim, self.dot, self.row_base, self.ids = name, dim, dot, row_base, ids
        self.tags, self.sharded, self.program, self.max_edge = tags and not sharded, sharded, program, max_edge


FLAVOURS = {f.name: f for f in (
    Flavour("f32", 64),
    Flavour("shadow", 64),
    Flavour("shadow_dot72", 72, dot=True, row_base=1000),
    Flavour("ids768", 768, ids=True, program="short", max_edge=1025),
    Flavour("sharded", 64, sharded=True, program="sharded"),
)}
SEEDS = (0, 1, 2)


def _signed(rng, shape, values):
    return rng.choice(np.asarray(values, dtype=np.int64), size=shape) * rng.choice(np.asarray([-1, 1], dtype=np.int64), size=shape)


class RowSource:
    """The pool a walk draws its rows from (builds, extends and updates alike, so group sizes move) and its NQ queries.
    C int64 [pool, dim], group [pool], Q int64 [NQ, dim], target [NQ]; e, boost as `exact_cases.dyadic` fixes them, from the
    largest base |score| of the whole pool."""

    def __init__(self, dim, seed, pool, dot=False):
        D = dim - W
        assert D >= 2
        for s in range(seed, seed + 16):
            rng = np.random.default_rng([s, dim, 977])
            C = np.zeros((pool, dim), dtype=np.int64)
            Q = np.zeros((NQ, dim), dtype=np.int64)
            C[:, :D] = _signed(rng, (pool, D), [2, 4])
            C[:, 0] = _signed(rng, (pool,), [1, 3])
            Q[:, :D] = _signed(rng, (NQ, D), [1, 2, 3, 4])
            Q[:, 0] = _signed(rng, (NQ,), [1, 3])
            p = 1.0 + rng.random(W)                       # uneven groups, the largest at most twice the smallest
            group = rng.choice(W, size=pool, p=p / p.sum())
            base = np.rint(C[:, :D].astype(np.float64) @ Q[:, :D].T.astype(np.float64)).astype(np.int64)
            top = int(np.abs(base).max())
            if dot:
                e, boost = 0, 2
                while boost * boost <= 2 * top:
                    boost *= 2
            else:
                e = max(2, math.ceil(math.log2(16 * dim) / 2))
                while (1 << (2 * e - 2)) <= 2 * top:
                    e += 1
                boost = 1 << (e - 1)
            assert boost * boost > 2 * top, "the boost must exceed twice the largest base |score|"
            assert 16 * D + boost * boost < 2 ** 24, "a partial sum could leave the exact f32 integers"
            target = np.arange(NQ) % W
            C[np.arange(pool), D + group] = boost
            Q[np.arange(NQ), D + target] = boost
            S = base + (boost * boost) * (group[:, None] == target[None, :])
            if (S == 0).any():
                continue
            assert (S % 2 != 0).all(), "every total must be odd"
            assert dot or int(np.abs(S).max()) <= 1 << (2 * e), "a cosine walk's |score| must stay <= 1"
            self.dim, self.dot, self.e, self.boost, self.top, self.seed = dim, dot, e, boost, top, s
            self.C, self.group, self.Q, self.target, self.at = C, group, Q, target, 0
            self.queries = self.f32(Q)
            return
        raise AssertionError("no seed without a zero total")

    def f32(self, ints):
        return np.ldexp(np.asarray(ints, dtype=np.int64).astype(np.float32), -self.e)

    def take(self, m):
        assert self.at + m <= self.C.shape[0], "the walk outran its pool"
        lo, self.at = self.at, self.at + m
        return self.C[lo:self.at].copy(), self.group[lo:self.at].copy()


# ---- the model ----------------------------------------------------------------------------------------------------------
class DenseModel:
    """What the handle should hold, in integers: C int64 [n, dim], group [n], the tagged prefix and its u32 tags, optional
    string ids, row_base, and the mirror of cap_rows (build: n, 1 when empty; remove leaves it; extend takes
    max(2 cap, n + m) when n + m exceeds it; load: n).  Shares no code with the library."""

    def __init__(self, src, C, group, ids=None, row_base=0, sharded=False):
        self.src, self.C, self.group = src, np.array(C, dtype=np.int64), np.array(group)
        self.ids = None if ids is None else list(ids)
        self.row_base, self.sharded = row_base, sharded
        self.tags = np.zeros(0, dtype=np.uint32)
        self.cap = max(1, self.n)

    @property
    def n(self):
        return self.C.shape[0]

    @property
    def tagged(self):
        return self.tags.shape[0]

    def rows_f32(self):
        return self.src.f32(self.C)

    def extend(self, C, group, ids=None):
        m = C.shape[0]
        if m and self.n + m > self.cap:
            self.cap = max(2 * self.cap, self.n + m)
        self.C = np.concatenate([self.C, C])
        self.group = np.concatenate([self.group, group])
        if self.ids is not None:
            self.ids = self.ids + list(ids)

    def remove(self, rows):
        """rows: local, any order, duplicates count once.  Survivors keep their order; tags compact with the rows."""
        gone = np.unique(np.asarray(rows, dtype=np.int64))
        assert gone.size == 0 or (gone[0] >= 0 and gone[-1] < self.n)
        keep = np.ones(self.n, dtype=bool)
        keep[gone] = False
        self.tags = self.tags[keep[:self.tagged]]
        self.C, self.group = self.C[keep], self.group[keep]
        if self.ids is not None:
            self.ids = [cid for cid, k in zip(self.ids, keep) if k]
        return int(gone.size)

    def update(self, rows, C, group):
        rows = np.asarray(rows, dtype=np.int64)
        assert np.unique(rows).size == rows.size
        self.C[rows], self.group[rows] = C, group

    def set_tags(self, first, tags):
        """The prefix rule of include/cqs_hip.h: overwrite inside the prefix and / or extend it; no gap, not past n."""
        tags = np.asarray(tags, dtype=np.uint32)
        assert first <= self.tagged and first + tags.size <= self.n
        if tags.size:
            self.tags = np.concatenate([self.tags[:first], tags, self.tags[first + tags.size:]])

    def save_load(self, row_base=0):
        """Tags are not persisted; a loaded handle's capacity is its row count."""
        self.tags = np.zeros(0, dtype=np.uint32)
        self.cap = max(1, self.n)
        self.row_base = row_base

    # ---- answers --------------------------------------------------------------------------------------------------------
    def scores(self, qis):
        """int64 [len(qis), n] = Q C^T (through f64: every total is far below 2^53)."""
        return np.rint(self.src.Q[list(qis)].astype(np.float64) @ self.C.T.astype(np.float64)).astype(np.int64)

    def group_size(self, g):
        return int((self.group == g).sum())

    def expected(self, S_row, k, keep=None, mode=MODE_RAW, thr=0.0):
        ids, sc = X.expected(S_row, self.src.e, k, keep=keep, mode=mode, thr=thr)
        return ids + np.uint64(self.row_base), sc

    def tag_bits(self, allow):
        """The host keep-bitset of a tag filter over the (fully tagged) rows, through `tags_cases.keep_mask`."""
        assert self.tagged == self.n
        return T.bits_of(T.keep_mask(self.tags, allow))

    def gram_f32(self, g):
        exact = np.ldexp(np.asarray(g, dtype=np.float64), -2 * self.src.e)
        s = exact.astype(np.float32)
        assert np.array_equal(s.astype(np.float64), exact), "a total is no exact f32"
        return s

    def neighbors(self, t, limit):
        """(rows u64, scores f32) of local row t's neighbours as `knn_cases.expected_graph` states them: the other rows
        by (score descending, row ascending) from the integer Gram row, the first clamp(limit)."""
        c = min(K.clamp(limit), self.n - 1)
        g = np.rint(self.C.astype(np.float64) @ self.C[t].astype(np.float64)).astype(np.int64)
        assert (g % 2 != 0).all(), "every total must be odd"
        cand = np.delete(np.arange(self.n), t)
        order = cand[np.lexsort((cand, -g[cand]))[:c]]
        return order.astype(np.uint64) + np.uint64(self.row_base), self.gram_f32(g[order])


# ---- the walk -----------------------------------------------------------------------------------------------------------
def pattern(name, n, rng):
    """The row patterns of tests/test_remove_gpu.py / test_update_gpu.py over n rows (local), sorted; `block` is clipped to
    the rows there are."""
    if name == "one":
        return np.array([n // 3])
    if name == "row0":
        return np.array([0])
    if name == "last":
        return np.array([n - 1])
    if name == "block":
        lo = min(200, n // 3)
        return np.arange(lo, max(lo + 1, min(600, n)))
    if name == "every_second":
        return np.arange(0, n, 2)
    if name == "random30":
        return np.sort(rng.choice(n, size=max(1, int(0.3 * n)), replace=False))
    if name == "all":
        return np.arange(n)
    raise KeyError(name)


class Walk:
    """seed, flavour, src, the build (C0, group0, ids0) and ops: a list of tuples
      ("extend", C, group, ids | None)        ("remove", rows local unsorted with duplicates, pattern name)
      ("update", rows local unsorted, C, group, pattern name)      ("set_tags", first local, tags u32)
      ("save_load",)                          ("refused",)  - a sharded handle's refused calls, made once."""


PROGRAMS = {
    # (move, argument[, pattern]); "slot": one of them, by seed, becomes the save / load
    "up": [("build", 33), ("tags", "full"), ("rm_to", 31, "one"), ("ext_to", 32), ("tags", "cover"), ("rm", "all"), ("ext_to", 1),
           ("upd", "row0"), ("ext_to", 257), ("tags", "full"), ("rm_to", 255, "last"), ("ext_to", 256), ("slot",), ("upd", "every_second"),
           ("ext_to", 1025), ("tags", "cover"), ("rm_to", 1023, "random30"), ("ext_to", 1024), ("slot",), ("ext_to", 4097),
           ("tags", "full"), ("rm_to", 4095, "row0"), ("ext_to", 4096), ("slot",), ("upd", "block"), ("rm", "every_second"),
           ("ext", (300, 900)), ("tags", "cover"), ("rm", "random30"), ("upd", "all"), ("rm", "block"), ("upd", "random30")],
    "down": [("build", 4097), ("tags", "full"), ("rm_to", 4095, "last"), ("ext_to", 4096), ("tags", "cover"), ("upd", "block"),
             ("rm", "every_second"), ("ext", (300, 900)), ("tags", "cover"), ("rm", "random30"), ("rm_to", 1025, "block"), ("upd", "all"),
             ("rm_to", 1023, "one"), ("ext_to", 1024), ("rm_to", 257, "every_second"), ("rm_to", 255, "row0"), ("ext_to", 256),
             ("upd", "random30"), ("rm_to", 33, "random30"), ("rm_to", 31, "last"), ("ext_to", 32), ("slot",), ("rm", "all"), ("ext_to", 1),
             ("slot",), ("ext", (300, 400)), ("tags", "full"), ("rm", "one"), ("ext", (300, 400)), ("tags", "cover"), ("upd", "last"),
             ("ext", (100, 150)), ("ext", (3500, 3700)), ("tags", "cover"), ("rm", "block")],
    "short": [("build", 33), ("tags", "full"), ("rm_to", 31, "one"), ("ext_to", 32), ("tags", "cover"), ("rm", "all"), ("ext_to", 1),
              ("upd", "row0"), ("ext_to", 257), ("tags", "full"), ("rm_to", 255, "last"), ("ext_to", 256), ("slot",), ("upd", "every_second"),
              ("ext_to", 1025), ("tags", "cover"), ("rm_to", 1023, "block"), ("ext_to", 1024), ("slot",), ("upd", "random30"),
              ("rm", "random30"), ("upd", "all")],
    "sharded": [("build", 31), ("ext_to", 32), ("ext_to", 33), ("upd", "all"), ("ext_to", 255), ("ext_to", 256), ("ext_to", 257),
                ("refused",), ("upd", "every_second"), ("ext_to", 1023), ("ext_to", 1024), ("ext_to", 1025), ("slot",), ("upd", "random30"),
                ("ext_to", 4095), ("ext_to", 4096), ("slot",), ("ext_to", 4097), ("upd", "block"), ("ext", (300, 800)), ("upd", "last")],
}


def walk(seed, steps, flavour):
    """The seeded walk of `flavour` (a Flavour or its name): at most `steps` operations after the build.  Sizes and
    patterns come from the edge lists of the program, the seed decides the program of a full walk (up / down first), the
    rows named by each pattern, the padding of a removal to its edge, the sizes between the edges, the tags and where
    the one save / load falls."""
    fl = FLAVOURS[flavour] if isinstance(flavour, str) else flavour
    rng = np.random.default_rng([seed, 4242, fl.dim])
    name = fl.program if fl.program != "full" else ("up", "down")[seed % 2]
    prog = list(PROGRAMS[name])
    slots = [i for i, mv in enumerate(prog) if mv[0] == "slot"]
    chosen = slots[int(rng.integers(len(slots)))]
    prog = [(("save_load",) if i == chosen else mv) for i, mv in enumerate(prog) if mv[0] != "slot" or i == chosen]
    src = RowSource(fl.dim, 100 + seed, 16000 if fl.max_edge > 1025 else 5000, dot=fl.dot)
    w = Walk()
    w.seed, w.flavour, w.src, w.program, w.ops = seed, fl, src, name, []
    serial = [0]

    def new_ids(m):
        if not fl.ids:
            return None
        serial[0] += m
        return ["r%06d" % i for i in range(serial[0] - m, serial[0])]

    assert prog[0][0] == "build"
    C, g = src.take(prog[0][1])
    w.C0, w.group0, w.ids0 = C, g, new_ids(C.shape[0])
    m = DenseModel(src, C, g, w.ids0, fl.row_base, fl.sharded)
    for mv in prog[1:]:
        if len(w.ops) >= steps:
            break
        kind, n = mv[0], m.n
        if kind in ("ext_to", "ext"):
            add = mv[1] - n if kind == "ext_to" else int(rng.integers(mv[1][0], mv[1][1] + 1))
            assert add > 0 and n + add <= MAX_ROWS, (mv, n)
            C, g = src.take(add)
            op = ("extend", C, g, new_ids(add))
            m.extend(C, g, op[3])
        elif kind in ("rm_to", "rm"):
            rows = pattern(mv[2] if kind == "rm_to" else mv[1], n, rng)
            if kind == "rm_to":
                need = n - mv[1]
                assert 0 < need <= n, (mv, n)
                if rows.size > need:                                   # keep the pattern's first and last row
                    rows = np.unique(np.concatenate([rows[:1], rows[-1:], rng.choice(rows, size=need, replace=False)]))[:need]
                if rows.size < need:
                    rest = np.setdiff1d(np.arange(n), rows)
                    rows = np.concatenate([rows, rng.choice(rest, size=need - rows.size, replace=False)])
            rows = rng.permutation(rows)                               # unsorted ...
            rows = np.concatenate([rows, rows[:3]])                    # ... with duplicates
            op = ("remove", rows, mv[-1])
            m.remove(rows)
        elif kind == "upd":
            rows = rng.permutation(pattern(mv[1], n, rng))
            C, g = src.take(rows.size)
            op = ("update", rows, C, g, mv[1])
            m.update(rows, C, g)
        elif kind == "tags":
            if not fl.tags:
                continue
            first = m.tagged if mv[1] == "cover" else (m.tagged // 2 if m.tagged == n else 0)
            first = max(0, first - (3 if first >= 3 and mv[1] == "cover" else 0))     # (cover: overwrites three inside the prefix too)
            tags = T.random_tags(n - first, int(rng.integers(1 << 30)))
            op = ("set_tags", first, tags)
            m.set_tags(first, tags)
        elif kind == "save_load":
            assert n > 0
            op = ("save_load",)
            m.save_load()
        elif kind == "refused":
            op = ("refused",)
        else:
            raise KeyError(kind)
        w.ops.append(op)
    return w


def start(w):
    return DenseModel(w.src, w.C0, w.group0, w.ids0, w.flavour.row_base, w.flavour.sharded)


def advance(m, op):
    """Apply one operation to the model alone."""
    if op[0] == "extend":
        m.extend(op[1], op[2], op[3])
    elif op[0] == "remove":
        m.remove(op[1])
    elif op[0] == "update":
        m.update(op[1], op[2], op[3])
    elif op[0] == "set_tags":
        m.set_tags(op[1], op[2])
    elif op[0] == "save_load":
        m.save_load()


def coverage(w):
    """What the walk does, from a replay of the model: see `claims`."""
    m = start(w)
    c = dict(kinds={}, up=set(), down=set(), zero_then_extend=False, grows=0, grows_after_removal=0,
             removal_fully_tagged=False, extend_with_tags=False, inside_cap=0, max_rows=m.n, save_load_at=None)
    removed = False
    for i, op in enumerate(w.ops):
        n0, cap0, tagged0 = m.n, m.cap, m.tagged
        advance(m, op)
        c["kinds"][op[0]] = c["kinds"].get(op[0], 0) + 1
        for e in EDGES:
            if n0 < m.n and n0 <= e <= m.n:
                c["up"].add(e)
            if n0 > m.n and n0 >= e >= m.n:
                c["down"].add(e)
        if op[0] == "extend":
            c["zero_then_extend"] |= n0 == 0
            c["extend_with_tags"] |= tagged0 > 0
            if m.cap > cap0:
                c["grows"] += 1
                c["grows_after_removal"] += removed
            else:
                c["inside_cap"] += 1
        if op[0] == "remove":
            c["removal_fully_tagged"] |= tagged0 == n0 and n0 > 0
            removed = True
        if op[0] == "save_load":
            c["save_load_at"], removed = i, False          # (a loaded handle starts a new life)
        c["max_rows"] = max(c["max_rows"], m.n)
    return c


def claims(w):
    """The coverage a walk of this flavour claims; tests/test_walk_cases_cpu.py asserts every entry."""
    fl = w.flavour
    edges = {e for e in EDGES if e <= fl.max_edge}
    if fl.sharded:       # no removal on a sharded handle: upward only, from 31 rows
        return dict(kinds=("extend", "update"), up={e for e in edges if e >= 31}, down=set(), zero_then_extend=False, grows=0,
                    grows_after_removal=0, removal_fully_tagged=False, extend_with_tags=False)
    kinds = ("extend", "remove", "update") + (("set_tags",) if fl.tags else ())
    return dict(kinds=kinds, up=edges, down=edges, zero_then_extend=True, grows=2, grows_after_removal=1,
                removal_fully_tagged=fl.tags, extend_with_tags=fl.tags)


# ---- applying an operation to a handle ----------------------------------------------------------------------------------
class WalkMismatch(AssertionError):
    def __init__(self, walk_, step, op, cause):
        super().__init__("walk %s seed %d step %d (%s%s): %s" % (walk_.flavour.name, walk_.seed, step, op[0],
                                                                 " " + op[-1] if len(op) > 1 and isinstance(op[-1], str) else "", cause))
        self.step, self.op = step, op


def apply(h, m, op, adapter):
    """One operation on the handle `h` (the methods of `cqs_amd.HipIndex`) and on the model; returns the handle to go on
    with (`save_load` replaces it, through `adapter.save_load(h, m)`)."""
    src, base = m.src, m.row_base
    if op[0] == "extend":
        h.extend(op[3], src.f32(op[1]))
    elif op[0] == "remove":
        want = int(np.unique(op[1]).size)
        if m.ids is not None:
            asked = [m.ids[int(r)] for r in op[1]] + ["never-indexed"]
            assert h.remove(asked) == want
        else:
            assert h.remove_rows(op[1].astype(np.uint64) + np.uint64(base)) == want
    elif op[0] == "update":
        if m.ids is not None:
            assert h.update([m.ids[int(r)] for r in op[1]], src.f32(op[2])) == op[1].size
        else:
            assert h.update_rows(op[1].astype(np.uint64) + np.uint64(base), src.f32(op[2])) == op[1].size
    elif op[0] == "set_tags":
        h.set_tags(op[2], first=base + op[1])
    elif op[0] == "save_load":
        h = adapter.save_load(h, m)
    elif op[0] == "refused":
        adapter.refused(h, m)
    advance(m, op)
    if m.ids is not None:
        assert h.id_map == m.ids, "id_map"
    return h


# ---- the checks after every step ----------------------------------------------------------------------------------------
def scattered_bits(n, seed):
    """A keep-bitset with about half the rows, the last one among them."""
    keep = np.random.default_rng(seed).integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    return (keep | X.range_bits(n, n - 1, n)) & X.range_bits(n, 0, n)


def _block(m, what, got, qis, S, k, keeps=None, mode=MODE_RAW, thr=0.0, full=None):
    r, s, cnt = got
    for j, qi in enumerate(qis):
        if full is not None:
            eid, esc = full[qi][0][:k], full[qi][1][:k]
        else:
            eid, esc = m.expected(S[qi], k, keep=None if keeps is None else keeps[j], mode=mode, thr=thr)
        X.assert_exact(r[j], s[j], cnt[j], eid, esc, what="%s: %d rows, block of %d, slot %d (query %d, group %d), k %d"
                       % (what, m.n, len(qis), j, qi, m.src.target[qi], k))


def check_step(h, m, step, probe=None, blocks=(1, 8, 32, 40), knn=None):
    """Everything the issue lists after a step, against the model, no tolerance.  probe(name): called with "group_singles"
    before and "group_singles_done" after the eight single-query searches at k = |group| (the GPU file reads the shadow
    counters around them)."""
    src, n = m.src, m.n
    assert len(h) == n, "len %d, expected %d" % (len(h), n)
    assert not h.is_poisoned(), "poisoned"
    if not m.sharded:
        assert h.tagged_rows() == m.tagged, "tagged_rows %d, expected %d" % (h.tagged_rows(), m.tagged)
    q = src.queries
    S = m.scores(range(NQ))
    kmax = min(MAX_K, n)
    full = [m.expected(S[i], kmax) for i in range(NQ)]                       # (a top-k is a prefix of the top-kmax)
    sizes = [m.group_size(g) for g in range(W)]
    # the eight groups, one query each, k = |group|: the answer is the group, in exact score order
    if probe:
        probe("group_singles")
    for g in range(W):
        k = min(MAX_K, sizes[g])
        got = h.search_batch(q[g:g + 1], k)
        _block(m, "single, k = |group|", got, [g], S, k, full=full)
        if 0 < sizes[g] <= MAX_K:
            assert sorted(full[g][0][:k].tolist()) == sorted((np.flatnonzero(m.group == g) + m.row_base).tolist()), "the group is not the top"
    if probe:
        probe("group_singles_done")
    for b in blocks:
        kg = min(MAX_K, max(sizes[g] for g in set(src.target[:b].tolist())))
        for k in sorted({1, 20, kg, kmax}):
            _block(m, "search_batch", h.search_batch(q[:b], k), range(b), S, k, full=full)
    kg = min(MAX_K, max(sizes))
    if n:
        # one shared bitset
        keep = scattered_bits(n, 31 * (step + 1) + n)
        _block(m, "shared bitset", h.search_batch(q[:8], kg, keep_bitset=keep), range(8), S, kg, keeps=[keep] * 8)
        # a bitset per query: the rows of the next group, plus scattered rows and the last one
        nb = blocks[-1]
        keeps = [T.bits_of(m.group == (src.target[i] + 1) % W) | (scattered_bits(n, 977 * (step + 1) + i) & np.uint32(0x80010001))
                 for i in range(nb)]
        k = min(300, kmax)
        _block(m, "per-query bitsets", h.search_batch_filtered(q[:nb], k, np.stack(keeps)), range(nb), S, k, keeps=keeps)
    # tags
    if not m.sharded and m.tagged == n and n and m.tagged:
        filters = T.filters_for(m.tags, 13 * (step + 1) + 1)
        for name in ("half_full", ("one_value_field_0", "one_value_field_1", "first_row", "last_row")[step % 4]):
            allow = filters[name]
            bits = m.tag_bits(allow)
            kept = int(X.bits_of(bits, n).sum())
            assert h.count_tagged(allow) == kept, "count_tagged(%s)" % name
            _block(m, "tagged (%s)" % name, h.search_tagged_batch(q[:8], kg, allow), range(8), S, kg, keeps=[bits] * 8)
        # a tag filter per query: the block's bitsets are written into the per-query table by one kernel
        nb = blocks[-1]
        names = sorted(filters)
        allows = np.stack([filters[names[(i + step) % len(names)]] for i in range(nb)])
        k = min(300, kmax)
        _block(m, "tag filter per query", h.search_tagged_multi(q[:nb], k, allows), range(nb), S, k, keeps=[m.tag_bits(a) for a in allows])
    elif not m.sharded and n:
        # rows without a tag: the tagged search is refused, says why, and (the checks below) changes nothing
        try:
            h.search_tagged_batch(q[:1], 1, T.ALL)
            refused = None
        except Exception as e:          # (HipError from the library)
            refused = str(e)
        assert refused is not None and "tags cover %d of %d rows" % (m.tagged, n) in refused, "tagged search with %d of %d rows tagged: %s" % (m.tagged, n, refused)
    # PIPELINE: clamp to [0, 1], keep `score >= thr`, thr a score that occurs
    if n:
        mid = full[0][1][min(len(full[0][1]) - 1, max(0, sizes[0] // 2))]
        thr = float(np.clip(mid, np.float32(0), np.float32(1)))
        got = h.search_batch(q[:8], kg, mode=MODE_PIPELINE, threshold=thr)
        _block(m, "PIPELINE thr %r" % thr, got, range(8), S, kg, mode=MODE_PIPELINE, thr=thr)
    # neighbours of a moved row and the graph over the last rows
    if knn is None:
        knn = step % KNN_EVERY == KNN_EVERY - 1
    if knn and n:
        for t in sorted({n - 1, n // 2}):
            r, s = h.neighbors_rows(m.row_base + t, KNN_LIMIT)
            er, es = m.neighbors(t, KNN_LIMIT)
            X.assert_exact(r, s, len(r), er, es, what="neighbors_rows(%d) of %d rows" % (t, n))
        if not m.sharded:
            first = max(0, n - 40)
            gr, gs, gc = h.knn_graph_rows(KNN_LIMIT, first=first, count=n - first)
            for t in range(first, n):
                er, es = m.neighbors(t, KNN_LIMIT)
                X.assert_exact(gr[t - first], gs[t - first], gc[t - first], er, es, what="knn_graph_rows row %d of %d" % (t, n))


def run(w, adapter, probe=None, after_step=None, blocks=(1, 8, 32, 40)):
    """Build the handle, walk, check after every step.  A disagreement raises WalkMismatch naming walk, seed and step.
    Returns (handle, model)."""
    m = start(w)
    h = adapter.build(m)
    try:
        check_step(h, m, -1, probe, blocks)
    except AssertionError as e:
        raise WalkMismatch(w, -1, ("build",), e) from e
    for step, op in enumerate(w.ops):
        try:
            h = apply(h, m, op, adapter)
            check_step(h, m, step, probe, blocks)
        except WalkMismatch:
            raise
        except AssertionError as e:
            raise WalkMismatch(w, step, op, e) from e
        if after_step:
            after_step(step, op, h, m)
    return h, m


# ---- the shadow scans' certificates on a walk's data (tests/shadow_emul.py restates the arithmetic) ------------------------
class ShadowMirror:
    """R and the norm bound of the bf16 and the int8 copy as a handle holds them along a walk: maxima that take rows in
    (build, load: all rows; extend, update: the new rows) and let nothing out (remove, the rows an update overwrote)."""

    def __init__(self, dim, i8):
        self.dim, self.i8 = dim, i8 and dim % 16 == 0
        self.reset()

    def reset(self):
        self.r16 = self.norm16 = self.r8 = self.norm8 = 0.0

    def take_in(self, x):
        import shadow_emul as E
        if x.shape[0] == 0:
            return
        r, nm = E.r_and_norm_bf16(x, E.bf16_round(x), self.dim)
        self.r16, self.norm16 = max(self.r16, r), max(self.norm16, nm)
        if self.i8:
            codes, scale = E.build_i8(x)
            r, nm = E.r_and_norm(None, x, codes, scale, self.dim)
            self.r8, self.norm8 = max(self.r8, r), max(self.norm8, nm)

    def follow(self, m, op):
        """After `advance(m, op)`."""
        if op[0] in ("extend", "update"):
            self.take_in(m.src.f32(op[1] if op[0] == "extend" else op[2]))
        elif op[0] == "save_load":
            self.reset()
            self.take_in(m.rows_f32())


def _round_up_f32(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < v else f


def query_bound(q, r_max, norm_max, dim, i8):
    """scan_bf16.h shadow_query_bound / scan_i8.h i8_query_bound, the same f64 operations."""
    import shadow_emul as E
    qn = math.sqrt(float((q.astype(np.float64) ** 2).sum())) * (1.0 + 2.0 ** -40)
    gam = E.i8_gamma(dim) if i8 else E.shadow_gamma(dim)
    if not qn * norm_max * (1.0 + gam) < 2.0 ** 100 or (i8 and not qn * 128.0 * math.sqrt(dim) < 2.0 ** 100):
        return np.float32(np.inf)
    return _round_up_f32(qn * r_max * (1.0 + 2.0 ** -40) + dim * 2.0 ** -140 * ((1.0 + norm_max) if i8 else 1.0))


def certifies(m, mirror, qi, k, b=1):
    """The verdict of DESIGN.md 3.11 for query qi of the walk at this k in a block of b on the model's rows, RAW mode:
    "i8" / "bf16" + (" certified" | " fallback"), or "f32" where no copy serves (k' < k).  The copy: the int8 one for
    b <= 4 and 10 k + 150 <= 1023 where it exists, else the bf16 one for 2 k + 32 >= k."""
    import shadow_emul as E
    x, q, n = m.rows_f32(), m.src.queries[qi], m.n
    i8 = mirror.i8 and b <= 4 and 10 * k + 150 <= MAX_K - 1
    kp = 10 * k + 150 if i8 else min(2 * k + 32, MAX_K - 1)
    if k == 0 or n == 0 or kp < k:
        return "f32"
    if i8:
        codes, scale = E.build_i8(x)
        approx = E.scan_i8(codes, scale, q)
        bq = query_bound(q, mirror.r8, mirror.norm8, m.src.dim, True)
    else:
        approx = E.scan_bf16(E.bf16_round(x), q)
        bq = query_bound(q, mirror.r16, mirror.norm16, m.src.dim, False)
    name = "i8" if i8 else "bf16"
    idx = np.arange(n)
    order = idx[np.lexsort((idx, -approx.astype(np.float64)))]
    if n <= kp:                                              # (a) every row was rescored
        return name + " certified"
    exact = np.ldexp(m.scores([qi])[0][order[:kp]].astype(np.float64), -2 * m.src.e).astype(np.float32)
    s_k = np.sort(exact)[::-1][k - 1]
    return name + (" certified" if np.float32(approx[order[kp]] + bq) < s_k else " fallback")


def group_singles_verdicts(m, mirror):
    """The verdicts of the eight single-query searches at k = |group| that `check_step` sends first."""
    out = []
    for g in range(W):
        k = min(MAX_K, m.group_size(g))
        if k:
            out.append(certifies(m, mirror, g, k))
    return out
