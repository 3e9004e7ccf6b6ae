"""A seeded operation walk over one sparse index handle ("Operation walks"): `remove`, `extend_csr`, `set_tags`
and one save / load interleaved on the `Model` of tests/test_sparse_update_gpu.py, about twenty steps, ranked and unranked.
After every step every query - single and batched, plain, under a keep mask and under a tag filter - is held to
`oracle.SpladeIndex` built from the model's documents: the same chunks in the same order, equal score bits.  The sizes cross
31 / 32 / 33 (a bitset word) and 1023 / 1024 / 1025 (an n_pad granule) in both directions; the removals are the dense
index's patterns, unsorted with duplicates, and "everything"; the extends bring 1, 300 and 3000 chunks, tokens nobody had,
a document without postings and ids that sort before, between and after the held ones.  `assert_rule` (the handle against a
fresh build, and the saved file) once at the end."""
import numpy as np
import pytest

import sparse_cases as sc
import tags_cases as tc
import walk_cases as WC
from cqs_amd import _lib
from test_sparse_update_gpu import RANKED, VOCAB, Model, S, assert_rule, csr_take  # noqa: F401  (S: the module's fixture)

pytestmark = pytest.mark.gpu

POOL = 4800
# (move, argument): the sizes in between follow from the patterns; "slot": one of them, by seed, is the save / load
PROGRAM = [("build", 33), ("tags", "full"), ("rm_to", 31, "one"), ("ext", 1, "before"), ("special",), ("tags", "cover"), ("rm", "all"),
           ("ext", 300, "between"), ("slot",), ("ext_to", 1025, "plain"), ("tags", "full"), ("rm_to", 1023, "random30"), ("ext", 1, "after"),
           ("slot",), ("rm", "block"), ("ext", 3000, "plain"), ("tags", "cover"), ("rm", "every_second"), ("slot",), ("rm", "random30"),
           ("rm", "last"), ("ext", 300, "between"), ("tags", "cover"), ("rm", "row0")]


@pytest.fixture(scope="module")
def pool():
    """Documents to build and extend with, never modified: 1-8 postings each over a vocabulary of 200 (token ids 1 .. 200:
    0 stays free for a token nobody has), the special weights of `sparse_cases.corpus` among them; and four queries."""
    rng = np.random.default_rng(20260301)
    off, tok, w = sc.corpus(rng, POOL, VOCAB, 1, 8, dup_frac=0.3, special=True)
    tok = tok + np.uint32(1)
    queries = [sc.query(rng, VOCAB, t, dups=d, absent=a) for t, d, a in ((3, 0, 0), (24, 2, 1), (64, 0, 3), (150, 5, 0))]
    queries = [(t + np.uint32(1), w_) for t, w_ in queries]
    for a in (off, tok, w):
        a.setflags(write=False)
    return dict(doc=(off, tok, w), queries=queries)


class SparseWalk:
    """The model, the tags beside it (the tagged chunks are a prefix; remove compacts them with the chunks; save / load
    drops them) and the position in the pool."""

    def __init__(self, S, pool, ranked, seed):
        self.S, self.pool, self.ranked = S, pool, ranked
        self.rng = np.random.default_rng([seed, 555])
        self.at, self.serial = 0, 0
        self.tags = np.zeros(0, np.uint32)
        self.m = None

    def take(self, count):
        docs = np.arange(self.at, self.at + count)
        assert self.at + count <= POOL, "the walk outran its pool"
        self.at += count
        return csr_take(self.pool["doc"], docs)

    def ids(self, count, where):
        """Ids no chunk has had: "c..." like the build's, or sorting before every held id, after every one, or between them
        (a held id with a suffix sorts right behind it)."""
        if not self.ranked:
            return None
        self.serial += count
        nums = range(self.serial - count, self.serial)
        if where == "before":
            return ["a%06d" % i for i in nums]
        if where == "after":
            return ["z%06d" % i for i in nums]
        if where == "between" and self.m is not None and self.m.n:
            held = sorted(self.m.ids)
            return ["%s+%06d" % (held[int(self.rng.integers(len(held)))], i) for i in nums]
        return ["c%06d" % i for i in self.rng.permutation(np.asarray(nums))]

    def step(self, mv, tmp_path):
        m, rng = self.m, self.rng
        n = m.n if m is not None else 0
        if mv[0] == "build":
            self.m = Model(self.S, self.take(mv[1]), self.ids(mv[1], "plain"))
        elif mv[0] in ("ext", "ext_to"):
            count = mv[1] if mv[0] == "ext" else mv[1] - n
            m.extend(self.take(count), self.ids(count, mv[2]))
        elif mv[0] == "special":          # tokens nobody had (0 and the largest id) and a document without postings
            off = np.array([0, 2, 2, 5], dtype=np.uint64)
            tok = np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 7], dtype=np.uint32)
            w = np.array([1.5, 0.25, 2.0, -1.0, 0.5], dtype=np.float32)
            before = m.ix.unique_tokens()
            m.extend((off, tok, w), self.ids(3, "between"))
            assert m.ix.unique_tokens() == before + 2 + (7 not in m.csr[1][:-5])
        elif mv[0] in ("rm", "rm_to"):
            rows = WC.pattern(mv[-1], n, rng)
            if mv[0] == "rm_to":
                need = n - mv[1]
                rows = rows[:need]
                if rows.size < need:
                    rows = np.concatenate([rows, rng.choice(np.setdiff1d(np.arange(n), rows), size=need - rows.size, replace=False)])
            rows = rng.permutation(rows)
            rows = np.concatenate([rows, rows[:3]])                      # unsorted, with duplicates
            keep = np.ones(n, dtype=bool)
            keep[rows] = False
            m.remove(rows)
            self.tags = self.tags[keep[:self.tags.size]]
        elif mv[0] == "tags":
            tagged = self.tags.size
            first = max(0, tagged - 3) if mv[1] == "cover" else (tagged // 2 if tagged == n else 0)
            tags = tc.random_tags(n - first, int(rng.integers(1 << 30)))
            m.ix.set_tags(tags, first=first)
            self.tags = np.concatenate([self.tags[:first], tags])
        elif mv[0] == "save_load":
            path = str(tmp_path / "walk.bin")
            m.ix.save(path, 7)
            back = self.S.HipSpladeIndex.load(path, 7, m.ids)
            assert back is not None and len(back) == n
            m.ix.close()
            m.ix = back
            self.tags = np.zeros(0, np.uint32)
        else:
            raise KeyError(mv)


def same(got_chunks, got_scores, want, what):
    assert np.array_equal(np.asarray(got_chunks, dtype=np.uint64), want[0]), what
    assert np.array_equal(np.ascontiguousarray(got_scores, dtype=np.float32).view(np.uint32), want[1].view(np.uint32)), what


def check(walk, oracle, step):
    m, ix = walk.m, walk.m.ix
    n = m.n
    assert len(ix) == n and ix.postings() == int(m.csr[0][-1]) and ix.tagged_chunks() == walk.tags.size
    assert ix.unique_tokens() == np.unique(m.csr[1]).size
    qs = walk.pool["queries"]
    if n == 0:
        for qt, qw in qs:
            ch, _s, rc = ix.search_raw(qt, qw, 20)
            assert rc == _lib.OK and ch.size == 0
        return
    o = oracle.SpladeIndex(*m.csr, ids=m.ids, id_rank=m.rank)
    rng = np.random.default_rng(1000 + step)
    masks = [None, rng.random(n) < 0.5, rng.random(n) < 0.05]
    for i, (qt, qw) in enumerate(qs):
        for k in (1, 20, 1024):
            for j, keep in enumerate(masks):
                ch, s, rc = ix.search_raw(qt, qw, k, keep)
                assert rc == _lib.OK, ix.last_error
                same(ch, s, o.search_raw(qt, qw, k, keep), ("single", step, i, k, j))
    for j, keep in enumerate(masks):
        ch, s, cnt, rc = ix.search_batch_raw(qs, 500, keep)
        assert rc == _lib.OK, ix.last_error
        for i, (qt, qw) in enumerate(qs):
            same(ch[i, :cnt[i]], s[i, :cnt[i]], o.search_raw(qt, qw, 500, keep), ("batch", step, i, j))
    if walk.tags.size == n:
        filters = tc.filters_for(walk.tags, 17 * step + 3)
        for name in ("half_full", ("one_value_field_0", "one_value_field_1", "first_row", "last_row")[step % 4]):
            mask = tc.keep_mask(walk.tags, filters[name])
            for i, (qt, qw) in enumerate(qs):
                for k in (1, 500):
                    ch, s, rc = ix.search_tagged_raw(qt, qw, k, filters[name])
                    assert rc == _lib.OK, ix.last_error
                    same(ch, s, o.search_raw(qt, qw, k, mask), ("tagged", name, step, i, k))
    else:
        ch, _s, rc = ix.search_tagged_raw(qs[0][0], qs[0][1], 20, tc.allow_of([1], None, None, None))
        assert rc == _lib.ERR_INVALID and "tags cover %d of %d chunks" % (walk.tags.size, n) in ix.last_error


def program(seed):
    slots = [i for i, mv in enumerate(PROGRAM) if mv[0] == "slot"]
    chosen = slots[seed % len(slots)]
    return [(("save_load",) if i == chosen else mv) for i, mv in enumerate(PROGRAM) if mv[0] != "slot" or i == chosen]


@RANKED
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_sparse_walk(S, oracle, pool, tmp_path, ranked, seed):
    walk = SparseWalk(S, pool, ranked, seed)
    step = -1
    try:
        for step, mv in enumerate(program(seed)):
            walk.step(mv, tmp_path)
            check(walk, oracle, step)
    except AssertionError as e:
        raise AssertionError("sparse walk %s seed %d step %d %s: %s" % ("ranked" if ranked else "unranked", seed, step, mv, e)) from e
    assert_rule(walk.m, oracle, tmp_path)
    walk.m.close()
