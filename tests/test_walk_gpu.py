"""Seeded operation walks over one dense index handle ("Operation walks").

A daemon keeps one handle for days and interleaves extend, remove, update, set_tags and save / load in whatever order file
edits arrive; every other test of those calls starts from a fresh handle and applies one of them.  Here one handle walks
through about thirty seeded operations (tests/walk_cases.py: sizes from the edge lists, the removal and update patterns of
test_remove_gpu.py / test_update_gpu.py, extends inside and past the capacity) and after every one its searches are held
to a model in integers that shares no code with the library: an equal count, an identical id list, equal score bits
(`exact_cases.assert_exact`), no tolerance anywhere.  tests/test_walk_cases_cpu.py holds the model to the oracle and shows
that the same check functions reject planted faults.  Run on an MI355X with `pytest -m gpu -s` to see the counters."""
import json

import numpy as np
import pytest

import walk_cases as WC
from cqs_amd import DistanceMetric, HipError, HipIndex, _lib
from test_update_gpu import hooks, read_bf16, read_i8  # noqa: F401  (hooks: the fixture that types cqs_hip_debug_shadow_rows)

pytestmark = pytest.mark.gpu

SHARDS = [0, 0, 0]
BUDGET = 1000                      # rows per pass of remove / update on the dot-metric walk: the passes straddle
ENV = {"f32": {"CQS_HIP_SCAN_BF16": "0"},
       "shadow": {"CQS_HIP_SCAN_BF16": "1", "CQS_HIP_SCAN_I8": "1"},
       "shadow_dot72": {"CQS_HIP_SCAN_BF16": "1", "CQS_HIP_SCAN_I8": "1"},        # dim % 16 != 0: the bf16 copy alone
       "ids768": {"CQS_HIP_SCAN_BF16": "0"},
       "sharded": {"CQS_HIP_SCAN_BF16": "0"}}


class GpuAdapter:
    """build / save_load / refused of `walk_cases.run` over `HipIndex`, and the shadow counters along the walk."""

    def __init__(self, hip, fl, tmp_path):
        self.hip, self.fl, self.tmp = hip, fl, tmp_path
        self.shadow = fl.name.startswith("shadow")
        self.h = None
        self.closed = np.zeros(4, np.int64)          # certified / fallback of handles already closed: bf16, then int8
        self.singles = np.zeros(4, np.int64)         # ... of the single-query searches at k = |group|
        self.asked = 0

    def _make(self, m):
        metric = DistanceMetric.DotProduct if m.src.dot else DistanceMetric.Cosine
        ids = None if m.ids is None else list(m.ids)
        if self.fl.sharded:
            return HipIndex.build_sharded(ids, m.rows_f32(), SHARDS, metric, row_base=m.row_base)
        return HipIndex.build_from_flat(ids, m.rows_f32(), metric, row_base=m.row_base)

    def _adopt(self, h, n):
        if self.fl.name == "shadow_dot72":
            self.hip.cqs_hip_debug_index_remove_budget(h._h, BUDGET)
            self.hip.cqs_hip_debug_index_update_budget(h._h, BUDGET)
        if self.shadow:
            dim = self.fl.dim
            assert h.bf16_stats()[0] == n * dim * 2 and (h.i8_stats()[0] > 0) == (dim % 16 == 0), h.last_error()
        else:
            assert h.bf16_stats()[0] == 0
        self.h = h
        return h

    def build(self, m):
        return self._adopt(self._make(m), m.n)

    def counters(self):
        return np.array(self.h.bf16_stats()[1:] + self.h.i8_stats()[1:], np.int64)

    def probe(self, name):
        if name == "group_singles":
            self._before = self.counters()
        else:
            self.singles += self.counters() - self._before

    def save_load(self, h, m):
        """The saved bytes are those of a fresh build of the model's rows; the walk goes on with the loaded handle."""
        pa, pf = str(self.tmp / "walk.hipflat"), str(self.tmp / "fresh.hipflat")
        fresh = self._make(m)
        h.save(pa); fresh.save(pf)
        fresh.close()
        assert open(pa, "rb").read() == open(pf, "rb").read(), "the saved blob is not a fresh build's"
        ma, mf = json.load(open(pa + ".meta")), json.load(open(pf + ".meta"))
        assert ma == mf and ma["chunk_count"] == m.n and ma["id_map"] == m.ids
        self.closed += self.counters()
        h.close()
        loaded = HipIndex.load(pa, self.fl.dim, m.n, devices=SHARDS if self.fl.sharded else None)
        assert loaded.metric is (DistanceMetric.DotProduct if m.src.dot else DistanceMetric.Cosine)
        return self._adopt(loaded, m.n)

    def refused(self, h, m):
        """What a row-sharded handle does not support, each called once: its error, and (the checks that follow) no change."""
        for call, words in ((lambda: h.remove_rows([m.row_base + 5]), "remove: not supported on a row-sharded handle"),
                            (lambda: h.set_tags(np.zeros(4, np.uint32)), "row-sharded handle"),
                            (lambda: h.knn_graph_rows(5, first=0, count=10), "row-sharded handle")):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID and words in str(e.value), str(e.value)
        assert h.tagged_rows() == 0 and len(h) == m.n and not h.is_poisoned()


def compare_with_a_fresh_build(adapter, h, m, hooks, seed):
    """At the end of a walk: the shadow copies hold the bytes a fresh build of the model's rows holds, and the dots of a
    pool of rows - all of them moved and most of them rewritten by then - have its bits, which are the integer Gram's."""
    fresh = adapter._make(m)
    try:
        assert len(h) == len(fresh) == m.n
        if adapter.shadow:
            assert np.array_equal(read_bf16(hooks, h), read_bf16(hooks, fresh)), "bf16 words"
            if adapter.fl.dim % 16 == 0:
                (ca, sa), (cf, sf) = read_i8(hooks, h), read_i8(hooks, fresh)
                assert np.array_equal(ca, cf) and np.array_equal(sa.view(np.uint32), sf.view(np.uint32)), "int8 codes / scales"
        if not adapter.fl.sharded:
            pool = np.unique(np.concatenate([[0, m.n - 1], np.random.default_rng(seed).choice(m.n, size=38)]))
            rows = pool.astype(np.uint64) + np.uint64(m.row_base)
            got = h.pairwise_rows(rows)
            assert np.array_equal(got.view(np.uint32), fresh.pairwise_rows(rows).view(np.uint32)), "pairwise_rows against the fresh build"
            gram = np.rint(m.C[pool].astype(np.float64) @ m.C[pool].T.astype(np.float64)).astype(np.int64)
            assert np.array_equal(got.view(np.uint32), m.gram_f32(gram).view(np.uint32)), "pairwise_rows against the integer Gram matrix"
    finally:
        fresh.close()


@pytest.mark.parametrize("seed", WC.SEEDS)
@pytest.mark.parametrize("name", sorted(WC.FLAVOURS))
def test_walk(hooks, monkeypatch, tmp_path, name, seed):
    for var, value in ENV[name].items():
        monkeypatch.setenv(var, value)
    w = WC.walk(seed, WC.STEPS, name)
    adapter = GpuAdapter(hooks, w.flavour, tmp_path)
    h, m = WC.run(w, adapter, probe=adapter.probe if adapter.shadow else None)
    try:
        total = adapter.closed + adapter.counters()
        print("walk %s-%d (%s, %d steps, %d rows at the end): shadow counters over the walk: bf16 certified %d, fallback %d, of them "
              "through int8 %d, %d; the single-query searches at k = |group|: bf16 certified %d, fallback %d, through int8 %d, %d"
              % ((name, seed, w.program, len(w.ops), m.n) + tuple(int(x) for x in total) + tuple(int(x) for x in adapter.singles)))
        if adapter.shadow:
            assert total[0] > 0 and adapter.singles[0] > 0, "the bf16 copy certified nothing over the walk"
            assert w.flavour.dim % 16 != 0 or (total[2] > 0 and adapter.singles[2] > 0), "the int8 copy certified nothing over the walk"
        else:
            assert not total.any()
        compare_with_a_fresh_build(adapter, h, m, hooks, seed)
    finally:
        h.close()
