"""Keeps tests/walk_cases.py honest without a GPU ("Operation walks"): for every walk tests/test_walk_gpu.py
uses, the model's expected answers against the CPU oracle at every step, the exactness of f32 accumulation on the walk's
data, the coverage each walk claims, the share of certified queries the shadow walks will see; then a numpy "handle" with
planted faults through the very functions the GPU file calls (`walk_cases.run` / `apply` / `check_step`), each of which
must be rejected at the step where the fault first acts."""
import numpy as np
import pytest

import exact_cases as X
import knn_cases as K
import tags_cases as T
import test_sparse_walk_gpu as SW
import walk_cases as WC
from test_exact_cases_cpu import f32_orders

STEPS = WC.STEPS
WALKS = [(name, seed) for name in WC.FLAVOURS for seed in WC.SEEDS]
WALK_IDS = ["%s-%d" % w for w in WALKS]


# ---- the model against the oracle, exactness, coverage ------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", WALKS, ids=WALK_IDS)
def test_model_matches_the_oracle_at_every_step(oracle, name, seed):
    w = WC.walk(seed, STEPS, name)
    m = WC.start(w)
    src = w.src
    assert src.queries.dtype == np.float32 and np.array_equal(src.queries.astype(np.float64), src.Q * 2.0 ** -src.e)
    rng = np.random.default_rng(7)
    for step, op in enumerate([("build",)] + w.ops):
        WC.advance(m, op)
        n, rows = m.n, m.rows_f32()
        assert rows.dtype == np.float32 and np.array_equal(rows.astype(np.float64), m.C * 2.0 ** -src.e)
        assert n <= WC.MAX_ROWS and m.tagged <= n
        if n == 0:
            assert X.expected(np.zeros(0, np.int64), src.e, 5)[0].shape[0] == 0
            continue
        D = src.dim - WC.W
        assert (m.C[:, :D] != 0).all() and (m.C[:, 1:D] % 2 == 0).all() and (m.C[:, 0] % 2 != 0).all()
        assert np.array_equal(m.C[np.arange(n), D + m.group], np.full(n, src.boost)) and (m.C[:, D:] != 0).sum() == n
        qis = [step % WC.W, (step + 3) % WC.NQ]
        S = m.scores(qis)
        assert not (S == 0).any() and (S % 2 != 0).all()
        for j, qi in enumerate(qis):
            what = "%s-%d step %d q%d" % (name, seed, step - 1, qi)
            want = np.ldexp(S[j].astype(np.float64), -2 * src.e).astype(np.float32)
            for got in f32_orders(rows, src.queries[qi], rng):
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
            # the boosted query's top-|group| is its group
            g = int(src.target[qi])
            size = m.group_size(g)
            if 0 < size <= WC.MAX_K:
                ids, _ = X.expected(S[j], src.e, size)
                assert sorted(ids.tolist()) == np.flatnonzero(m.group == g).tolist(), what
            k = min(WC.MAX_K, n)
            oid, osc = oracle.index_search(rows, src.queries[qi], k)
            X.assert_exact(oid, osc, len(oid), *X.expected(S[j], src.e, k), what=what + " plain")
            keep = T.bits_of(m.group == (g + 1) % WC.W) | (WC.scattered_bits(n, step) & np.uint32(0x80010001))
            oid, osc = oracle.index_search(rows, src.queries[qi], k, keep)
            X.assert_exact(oid, osc, len(oid), *X.expected(S[j], src.e, k, keep=keep), what=what + " bitset")
            full = X.expected(S[j], src.e, k)[1]
            thr = float(np.clip(full[min(len(full) - 1, size // 2)], np.float32(0), np.float32(1)))
            oid, osc = oracle.index_search(rows, src.queries[qi], k, None, 1, thr)
            eid, esc = X.expected(S[j], src.e, k, mode=1, thr=thr)
            assert thr == 0.0 or np.float32(thr) in esc
            X.assert_exact(oid, osc, len(oid), eid, esc, what=what + " pipeline")
        # the neighbours of the last row, against the oracle's find_neighbors (raw dots; exact on this data)
        if step % WC.KNN_EVERY == 0 and n > 1:
            oid, osc = oracle.find_neighbors(rows, n - 1, WC.KNN_LIMIT)
            er, es = m.neighbors(n - 1, WC.KNN_LIMIT)
            X.assert_exact(oid + np.uint64(m.row_base), osc, len(oid), er, es, what="%s-%d step %d neighbours" % (name, seed, step - 1))


@pytest.mark.parametrize("name,seed", WALKS, ids=WALK_IDS)
def test_walk_covers_what_it_claims(name, seed):
    w = WC.walk(seed, STEPS, name)
    c, want = WC.coverage(w), WC.claims(w)
    print("walk %s-%d (%s): %d steps, %s, capacity grows %d (%d after a removal), %d extends inside the capacity, at most %d rows, save/load at step %s"
          % (name, seed, w.program, len(w.ops), c["kinds"], c["grows"], c["grows_after_removal"], c["inside_cap"], c["max_rows"], c["save_load_at"]))
    for kind in want["kinds"]:
        assert c["kinds"].get(kind, 0) >= 2, "operation %s occurs %d times" % (kind, c["kinds"].get(kind, 0))
    assert c["kinds"].get("save_load", 0) == 1
    assert want["up"] <= c["up"], "edges never passed upward: %s" % sorted(want["up"] - c["up"])
    assert want["down"] <= c["down"], "edges never passed downward: %s" % sorted(want["down"] - c["down"])
    assert c["max_rows"] <= WC.MAX_ROWS
    if not w.flavour.sharded:
        assert c["zero_then_extend"], "n == 0 with an extend after it"
        assert c["grows"] >= want["grows"] and c["grows_after_removal"] >= want["grows_after_removal"]
        assert c["inside_cap"] >= 2, "extends that stay inside the mirrored capacity"
        assert c["removal_fully_tagged"] and c["extend_with_tags"]
        names = {op[-1] for op in w.ops if op[0] == "remove"}
        assert {"all", "one", "last"} <= names and len(names) >= 4, names
        assert all(np.unique(op[1]).size < op[1].size for op in w.ops if op[0] == "remove"), "removes carry duplicates"
        assert any((np.diff(op[1]) < 0).any() for op in w.ops if op[0] == "remove"), "removes are given unsorted"
    else:
        assert c["kinds"].get("refused", 0) == 1 and "remove" not in c["kinds"] and "set_tags" not in c["kinds"]
    assert len({op[-1] for op in w.ops if op[0] == "update"}) >= 3


@pytest.mark.parametrize("name,seed", [(n, s) for n in ("shadow", "shadow_dot72") for s in WC.SEEDS])
def test_shadow_walks_certify_a_third_of_the_group_queries(name, seed):
    """Otherwise the GPU walk would exercise only the fallback.  Printed: the verdicts the emulation predicts for the eight
    single-query searches at k = |group| of every step, which tests/test_walk_gpu.py counts on the device."""
    w = WC.walk(seed, STEPS, name)
    m = WC.start(w)
    mirror = WC.ShadowMirror(w.src.dim, i8=name == "shadow")
    mirror.take_in(m.rows_f32())
    total = {}
    worst = 1.0
    for step, op in enumerate([("build",)] + w.ops):
        WC.advance(m, op)
        mirror.follow(m, op)
        v = WC.group_singles_verdicts(m, mirror)
        for x in v:
            total[x] = total.get(x, 0) + 1
        if v:
            share = sum(x.endswith("certified") for x in v) / len(v)
            worst = min(worst, share)
            assert 3 * sum(x.endswith("certified") for x in v) >= len(v), "step %d: %s" % (step - 1, v)
    asked = sum(total.values())
    cert = sum(c for x, c in total.items() if x.endswith("certified"))
    print("shadow walk %s-%d: %d group queries, predicted %s; certified share %.3f overall, %.3f at the worst step"
          % (name, seed, asked, dict(sorted(total.items())), cert / asked, worst))
    assert total.get("bf16 certified", 0) > 0 and (name != "shadow" or total.get("i8 certified", 0) > 0)


# ---- sensitivity: a numpy handle with planted faults ----------------------------------------------------------------------
class Refused(Exception):
    pass


class NumpyHandle:
    """The methods of `cqs_amd.HipIndex` the walk uses, over a row buffer of `cap` rows laid out as the library's: rows
    [0, n) live, what lies past n is whatever an earlier life left there.  Scores in float64 from the f32 rows (exact on
    this data), sorted by (score descending, row ascending).  `fault`: one of FAULTS, planted where its name says;
    `fired_at`: the step (operations so far - 1) at which it first changed anything."""

    def __init__(self, rows, ids, row_base, fault=None, ops=0, fired_at=None):
        n, dim = rows.shape
        self.n, self.cap, self.dim, self.row_base = n, max(1, n), dim, row_base
        self.buf = np.zeros((self.cap, dim), np.float32)
        self.buf[:n] = rows
        self.tags, self.tagged = np.zeros(self.cap, np.uint32), 0
        self.id_map = None if ids is None else list(ids)
        self.fault, self.ops, self.fired_at = fault, ops, fired_at
        self.stale_n, self.tab_stride, self._cache = n, None, {}

    def _fire(self):
        if self.fired_at is None:
            self.fired_at = self.ops - 1

    def _mutated(self):
        self.ops += 1
        self._cache = {}

    # ---- operations ---------------------------------------------------------------------------------------------------
    def extend(self, ids, rows):
        self._mutated()
        m, at = rows.shape[0], self.n
        if self.n + m > self.cap:
            cap = max(2 * self.cap, self.n + m)
            buf, tags = np.zeros((cap, self.dim), np.float32), np.zeros(cap, np.uint32)
            buf[:self.n], tags[:self.tagged] = self.buf[:self.n], self.tags[:self.tagged]
            self.buf, self.tags, self.cap, self.stale_n = buf, tags, cap, self.n
            if self.tab_stride is not None and self.fault != "bitset read with the stride of the old capacity":
                self.tab_stride = (cap + 31) // 32
        elif self.fault == "rows appended at cap instead of n after a shrink" and self.stale_n > self.n:
            at = min(self.stale_n, self.cap - m)
            self._fire()
        self.buf[at:at + m] = rows
        self.n += m
        self.stale_n = max(self.stale_n, self.n)
        if ids is not None:
            self.id_map.extend(ids)

    def remove_rows(self, rows):
        self._mutated()
        local = np.unique(np.asarray(rows, dtype=np.int64) - self.row_base)
        if local.size and (local[0] < 0 or local[-1] >= self.n):
            raise Refused("remove: row id not in this index")
        keep = np.ones(self.n, dtype=bool)
        keep[local] = False
        n_new = int(keep.sum())
        tags = self.tags[:self.tagged][keep[:self.tagged]]
        if self.fault == "a removed row left in place" and local.size:
            right = self.buf[:self.n][keep][:n_new]
            keep[local[0]] = True                                      # (it stays; the last survivor falls off the end)
            if not np.array_equal(self.buf[:self.n][keep][:n_new], right):
                self._fire()
        if self.fault == "the tag column shifted by one after a removal" and tags.size >= 2 and not np.array_equal(tags, np.roll(tags, 1)):
            tags = np.roll(tags, 1)
            self._fire()
        self.stale_n = max(self.stale_n, self.n)
        self.buf[:n_new] = self.buf[:self.n][keep][:n_new]
        self.tags[:tags.size], self.tagged, self.n = tags, tags.size, n_new
        return int(local.size)

    def remove(self, ids):
        row_of = {cid: i for i, cid in enumerate(self.id_map)}
        local = sorted({row_of[cid] for cid in ids if cid in row_of})
        if not local:
            return 0
        removed = self.remove_rows(np.asarray(local) + self.row_base)
        gone = set(local)
        self.id_map[:] = [cid for i, cid in enumerate(self.id_map) if i not in gone]
        return removed

    def update_rows(self, rows, vectors):
        self._mutated()
        local = np.asarray(rows, dtype=np.int64) - self.row_base
        if np.unique(local).size != local.size or (local.size and (local.min() < 0 or local.max() >= self.n)):
            raise Refused("update")
        todo = np.arange(local.size)
        if self.fault == "one updated row skipped" and local.size and not np.array_equal(self.buf[local[0]], vectors[0]):
            todo = todo[1:]
            self._fire()
        self.buf[local[todo]] = vectors[todo]
        return int(local.size)

    def update(self, ids, vectors):
        row_of = {cid: i for i, cid in enumerate(self.id_map)}
        return self.update_rows(np.asarray([row_of[cid] for cid in ids]) + self.row_base, vectors)

    def set_tags(self, tags, first=0):
        self._mutated()
        tags, first = np.asarray(tags, dtype=np.uint32), first - self.row_base
        if first > self.tagged or first + tags.size > self.n:
            raise Refused("set_tags")
        self.tags[first:first + tags.size] = tags
        self.tagged = max(self.tagged, first + tags.size)

    # ---- properties and searches ----------------------------------------------------------------------------------------
    def __len__(self):
        return self.n

    def is_poisoned(self):
        return False

    def tagged_rows(self):
        return self.tagged

    def _mask_of_tags(self, allow):
        if self.tagged < self.n:
            raise Refused("tags cover %d of %d rows" % (self.tagged, self.n))
        return T.keep_mask(self.tags[:self.n], allow)

    def count_tagged(self, allow):
        return int(self._mask_of_tags(allow).sum())

    def _search(self, q, k, masks=None, mode=0, thr=0.0):
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        b, n = q.shape[0], self.n
        rows, scores, counts = np.zeros((b, max(k, 1)), np.uint64), np.zeros((b, max(k, 1)), np.float32), np.zeros(b, np.uint32)
        if n == 0 or k == 0:
            return rows[:, :k], scores[:, :k], counts
        S = (q.astype(np.float64) @ self.buf[:n].astype(np.float64).T).astype(np.float32)
        for j in range(b):
            s, kk, key = S[j], k, None
            alive = np.ones(n, dtype=bool)
            if masks is not None:
                alive = masks[j].copy()
                kk = min(k, int(alive.sum()))
            elif mode == 0:
                key = q[j].tobytes()
            if mode == 1:
                s = np.clip(s, np.float32(0), np.float32(1))
                alive &= s >= np.float32(thr)
            if key is not None and key in self._cache:
                order = self._cache[key]
            else:
                idx = np.flatnonzero(alive)
                order = idx[np.lexsort((idx, -s[idx].astype(np.float64)))]
                if key is not None:
                    self._cache[key] = order
            order = order[:kk]
            rows[j, :order.size], scores[j, :order.size], counts[j] = order.astype(np.uint64) + np.uint64(self.row_base), s[order], order.size
        return rows[:, :k], scores[:, :k], counts

    def search_batch(self, q, k, keep_bitset=None, mode=0, threshold=0.0):
        q = np.atleast_2d(q)
        masks = None if keep_bitset is None else [X.bits_of(keep_bitset, self.n)] * q.shape[0]
        return self._search(q, k, masks, mode, threshold)

    def search_batch_filtered(self, q, k, keep_bitsets, mode=0, threshold=0.0):
        b, words = keep_bitsets.shape
        stride = (max(self.cap, self.n) + 31) // 32
        if self.tab_stride is None or (self.tab_stride < stride and self.fault != "bitset read with the stride of the old capacity"):
            self.tab_stride = stride                                   # (made on first use, regrown with the capacity)
        table = np.zeros(b * max(stride, self.tab_stride) + words, np.uint32)
        for j in range(b):
            table[j * stride:j * stride + words] = keep_bitsets[j]         # staged with the stride of this capacity ...
        read = [table[j * self.tab_stride:j * self.tab_stride + words] for j in range(b)]       # ... read with the table's
        if any(not np.array_equal(r, kb) for r, kb in zip(read, keep_bitsets)):
            self._fire()
        return self._search(q, k, [X.bits_of(r, self.n) for r in read], mode, threshold)

    def search_tagged_batch(self, q, k, allow, mode=0, threshold=0.0):
        q = np.atleast_2d(q)
        return self._search(q, k, [self._mask_of_tags(allow)] * q.shape[0], mode, threshold)

    def search_tagged_multi(self, q, k, allows, mode=0, threshold=0.0):
        return self._search(q, k, [self._mask_of_tags(a) for a in allows], mode, threshold)

    def neighbors_rows(self, target_row, limit):
        t = int(target_row) - self.row_base
        x = self.buf[:self.n].astype(np.float64)
        s = (x @ x[t]).astype(np.float32)
        cand = np.delete(np.arange(self.n), t)
        order = cand[np.lexsort((cand, -s[cand].astype(np.float64)))[:K.clamp(limit)]]
        return order.astype(np.uint64) + np.uint64(self.row_base), s[order]

    def knn_graph_rows(self, limit, first=0, count=None):
        count = self.n - first if count is None else count
        L = K.clamp(limit)
        rows, scores, counts = np.zeros((count, L), np.uint64), np.zeros((count, L), np.float32), np.zeros(count, np.uint32)
        for i in range(count):
            r, s = self.neighbors_rows(self.row_base + first + i, limit)
            rows[i, :r.size], scores[i, :r.size], counts[i] = r, s, r.size
        return rows, scores, counts


class NumpyAdapter:
    def __init__(self, fault=None):
        self.fault, self.h = fault, None

    def build(self, m):
        self.h = NumpyHandle(m.rows_f32(), m.ids, m.row_base, self.fault)
        return self.h

    def save_load(self, h, m):
        """What the handle holds goes to the file and comes back: capacity = rows, no tags, row_base 0."""
        self.h = NumpyHandle(h.buf[:h.n].copy(), h.id_map, 0, h.fault, h.ops + 1, h.fired_at)
        return self.h

    def refused(self, h, m):
        pass


FAULTS = ("a removed row left in place", "one updated row skipped", "the tag column shifted by one after a removal",
          "rows appended at cap instead of n after a shrink", "bitset read with the stride of the old capacity")
FAULT_WALKS = (("f32", 0), ("f32", 1))          # the "up" and the "down" program


@pytest.mark.parametrize("name,seed", FAULT_WALKS + (("ids768", 0),), ids=lambda v: str(v))
def test_numpy_handle_without_a_fault_walks_to_the_end(name, seed):
    w = WC.walk(seed, STEPS, name)
    h, m = WC.run(w, NumpyAdapter())
    assert len(h) == m.n and h.fired_at is None and h.ops == len(w.ops)
    assert h.cap == m.cap, "the model's mirror of cap_rows"


@pytest.mark.parametrize("name,seed", FAULT_WALKS, ids=lambda v: str(v))
@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_rejected_where_they_act(fault, name, seed):
    w = WC.walk(seed, STEPS, name)
    adapter = NumpyAdapter(fault)
    with pytest.raises(WC.WalkMismatch) as e:
        WC.run(w, adapter)
    print("planted fault %r on walk %s-%d: first acts at step %s, rejected at step %d: %s"
          % (fault, name, seed, adapter.h.fired_at, e.value.step, str(e.value)[:200]))
    assert adapter.h.fired_at is not None and e.value.step == adapter.h.fired_at


# ---- the sparse walk ------------------------------------------------------------------------------------------------------
def test_the_sparse_walk_crosses_its_edges():
    """The sizes pass 31 / 32 / 33 and 1023 / 1024 / 1025 upward and downward, reach zero, and every operation of the issue
    occurs (the program of tests/test_sparse_walk_gpu.py, whatever the patterns remove in between)."""
    n, up, down, seen = 0, set(), set(), []
    for mv in SW.program(0):
        n0 = n
        if mv[0] in ("build", "ext_to"):
            n = mv[1]
        elif mv[0] == "ext":
            n += mv[1]
        elif mv[0] == "special":
            n += 3
        elif mv[0] == "rm_to":
            n = mv[1]
        elif mv[0] == "rm":
            n -= WC.pattern(mv[1], n, np.random.default_rng(0)).size
        seen.append(mv[0] if mv[0] not in ("rm", "rm_to") else mv[-1])
        for e in (0, 31, 32, 33, 1023, 1024, 1025):
            if n0 < n and n0 <= e <= n:
                up.add(e)
            if n0 > n and n0 >= e >= n:
                down.add(e)
    assert up >= {0, 31, 32, 33, 1023, 1024, 1025} and down >= {0, 31, 32, 33, 1023, 1024, 1025}, (up, down)
    assert {"all", "one", "row0", "last", "block", "every_second", "random30", "special", "save_load", "tags"} <= set(seen)
    assert {mv[1] for mv in SW.PROGRAM if mv[0] == "ext"} == {1, 300, 3000} and {mv[2] for mv in SW.PROGRAM if mv[0] == "ext"} >= {"before", "between", "after"}
