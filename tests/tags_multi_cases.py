"""Shared cases of tests/test_tags_multi_gpu.py: blocks of tag filters, one per query, and the native
storm of single tagged callers.  Also runnable in a child process (`python -c "import tags_multi_cases as c; c.child_shadow()"`)
for handles whose environment is read at create."""
import numpy as np

import tags_cases as tc
from cqs_amd import DistanceMetric, HipIndex, _lib, synth

DIM = 64
N_BIG = 70001
SEVEN = 0x0B0B0B0B          # the tag seven rows below 5 000 carry and no other row does
STORM_N, STORM_DIM = 140_005, 768      # the corpus filter_block_cases.storm_case runs on


def half_full(rng):
    return tc.allow_of(*[[int(v) for v in np.flatnonzero(rng.random(256) < 0.5)] for _ in range(4)])


def kernel_filters(tags, f, seed):
    """[f, 32]: tags_cases.filters_for (10 named filters), cut to f or extended to f with seeded random half-full ones and,
    from 12 on, two repeats of named ones (identical filters in one table)."""
    rng = np.random.default_rng(seed)
    named = list(tc.filters_for(tags, seed).values())
    out = named[:f]
    while len(out) < f:
        out.append(named[len(out) % 7] if len(out) in (11, 20) else half_full(rng))
    return np.ascontiguousarray(np.stack(out), dtype=np.uint32)


def data(n=N_BIG, dim=DIM, nq=40, seed=9100):
    rows = synth.gaussian_unit(n, dim, seed=seed)
    q = synth.gaussian_unit(nq, dim, seed=seed + 1)
    tags = tc.unique_end_tags(n, seed + 2)
    tags[[3, 64, 65, 2047, 2048, 4095, 4999]] = SEVEN
    return rows, q, tags


def block_case(q, tags, seed):
    """40 queries and a filter for each, [40, 32].  The first nine mix half-full, all-pass, keeps-nothing, a NON-FINITE query
    (index 3), keeps-7-rows, one-row (first / last), a single value and only-255; the rest are random half-full ones with
    the three special kinds repeated further back (so that the second block of b = 33 / 40 has some too)."""
    rng = np.random.default_rng(seed)
    named = tc.filters_for(tags, seed)
    nothing = tc.allow_of(None, None, [], None)
    seven = tc.allow_of([11], None, None, None)
    allows = [named["half_full"], tc.ALL.copy(), nothing, half_full(rng), seven, named["first_row"], named["last_row"],
              named["one_value_field_0"], named["only_255"]]
    while len(allows) < len(q):
        allows.append({33: nothing, 35: tc.ALL.copy(), 36: seven, 38: named["first_row"]}.get(len(allows)) if len(allows) in (33, 35, 36, 38)
                      else half_full(rng))
    q = np.array(q, dtype=np.float32)
    q[3, 5] = np.nan
    q[34, 0] = np.inf
    return q, np.ascontiguousarray(np.stack(allows), dtype=np.uint32)


def tagged_index(rows, tags, metric=DistanceMetric.Cosine):
    idx = HipIndex.build_from_flat(None, rows, metric)
    idx.set_tags(tags)
    assert idx.tagged_rows() == len(tags) == len(idx)
    return idx


def same_query(got, want, ctx):
    """rows, score bits and count of ONE query's answer."""
    (ra, sa, ca), (rb, sb, cb) = got, want
    c = int(cb)
    assert int(ca) == c, (ctx, int(ca), c)
    assert np.array_equal(ra[:c], rb[:c]), ctx
    assert np.array_equal(sa[:c].view(np.uint32), sb[:c].view(np.uint32)), ctx


class Lone:
    """The lone tagged answers of one handle, computed once per (query, k, mode, threshold) and left unchanged."""

    def __init__(self, idx, q, allows):
        self.idx, self.q, self.allows, self._got = idx, q, allows, {}

    def __call__(self, i, k, mode=_lib.MODE_RAW, thr=0.0):
        key = (i, k, mode, thr)
        if key not in self._got:
            r, s, c = self.idx.search_tagged_batch(self.q[i], k, self.allows[i], mode=mode, threshold=thr)
            self._got[key] = (r[0].copy(), s[0].copy(), int(c[0]))
        return self._got[key]


def check_block(idx, lone, q, allows, bits, b, k, mode=_lib.MODE_RAW, thr=0.0):
    """search_tagged_multi over the first b queries: per query the lone tagged call's bytes, and the bytes of
    search_batch_filtered with the host bitsets of the same predicates."""
    r, s, c = idx.search_tagged_multi(q[:b], k, allows[:b], mode=mode, threshold=thr)
    hr, hs, hc = idx.search_batch_filtered(q[:b], k, bits[:b], mode=mode, threshold=thr)
    for i in range(b):
        same_query((r[i], s[i], c[i]), lone(i, k, mode, thr), ("lone tagged", len(idx), b, k, mode, thr, i))
        same_query((r[i], s[i], c[i]), (hr[i], hs[i], hc[i]), ("host bitsets", len(idx), b, k, mode, thr, i))
    return c


def host_bits(tags, allows):
    return np.ascontiguousarray(np.stack([tc.bits_of(tc.keep_mask(tags, a)) for a in allows]))


def storm_tagged(idx, qs, allows, k, n_threads, per_thread):
    """cqs_hip_debug_client_storm_tagged: native threads, one query and its tag filter per call.  -> (rows, scores, counts)."""
    q = np.ascontiguousarray(qs, dtype=np.float32)
    a = np.ascontiguousarray(allows, dtype=np.uint32)
    nq = len(q)
    assert a.shape == (nq, 32)
    r = np.zeros((nq, k), np.uint64); s = np.zeros((nq, k), np.float32); c = np.zeros((nq,), np.uint32)
    el = idx._lib.cqs_hip_debug_client_storm_tagged(idx._h, q.ctypes.data, nq, q.shape[1], k, a.ctypes.data, n_threads, per_thread,
                                                   r.ctypes.data, s.ctypes.data, c.ctypes.data)
    assert el > 0, ("a storm call failed", idx.last_error())
    return r, s, c


def storm_corpus(nq=16):
    """The storm's corpus, queries, tags and one filter per query row - none of them all-pass (an all-pass tagged call IS
    an unfiltered search and would move the unfiltered counters): the named ones but all-pass, then random half-full ones."""
    rows = synth.gaussian_unit(STORM_N, dim=STORM_DIM, seed=7100)
    qs = synth.gaussian_unit(nq, dim=STORM_DIM, seed=7101)
    tags = tc.unique_end_tags(STORM_N, 7102)
    rng = np.random.default_rng(7103)
    allows = [a for name, a in tc.filters_for(tags, 7104).items() if name != "all_pass"]
    while len(allows) < nq:
        allows.append(half_full(rng))
    return rows, qs, tags, np.ascontiguousarray(np.stack(allows[:nq]), dtype=np.uint32)


def storm_case(idx, qs, allows, want, k=20, rounds=((8, 6), (16, 6))):
    """Every answer of the storm equals want[i]; -> (tagged passes, tagged queries, total calls)."""
    p0, q0 = idx.combine_tagged_stats()
    u0, f0 = idx.combine_stats(), idx.combine_filter_stats()
    total = 0
    for n_threads, per_thread in rounds:
        r, s, c = storm_tagged(idx, qs, allows, k, n_threads, per_thread)
        total += n_threads * per_thread
        for i in range(len(qs)):
            same_query((r[i], s[i], c[i]), want[i], ("storm", n_threads, i))
    p1, q1 = idx.combine_tagged_stats()
    assert idx.combine_stats() == u0 and idx.combine_filter_stats() == f0, "tagged traffic moved another class's counters"
    return p1 - p0, q1 - q0, total


# ---- children: the environment is read when the handle is made -----------------------------------------------------
def child_shadow():
    """CQS_HIP_SCAN_BF16=1 CQS_HIP_SCAN_I8=1: the blocks go through the shadow copies; the f32 handle is the yardstick."""
    rows, q, tags = data()
    q, allows = block_case(q, tags, 9400)
    bits = host_bits(tags, allows)
    idx = tagged_index(rows, tags)
    assert idx.bf16_stats()[0] > 0 and idx.i8_stats()[0] > 0, "the shadow copies were not built"
    f32 = tagged_index(rows, tags)
    f32.set_bf16_scan(False)
    assert f32.bf16_stats()[0] == 0
    lone = Lone(f32, q, allows)                        # lone tagged calls on the f32 scan
    kept = np.array([int(tc.keep_mask(tags, a).sum()) for a in allows])
    finite = np.isfinite(q).all(axis=1)
    for b in (1, 2, 9, 32, 33, 40):
        for k in (1, 20, 500):
            for mode, thr in ((_lib.MODE_RAW, 0.0), (_lib.MODE_PIPELINE, 0.3)):
                _, c0, f0 = idx.bf16_stats()
                check_block(idx, lone, q, allows, bits, b, k, mode, thr)
                _, c1, f1 = idx.bf16_stats()
                # (check_block also runs search_batch_filtered on the same handle: twice the block's queries)
                answered = int((finite[:b] & (kept[:b] > 0)).sum())
                if k == 20:
                    assert (c1 - c0) + (f1 - f0) == 2 * answered, (b, k, mode, c1 - c0, f1 - f0, answered)
    _, c0, f0 = idx.bf16_stats()
    idx.search_tagged_multi(q[:40], 20, allows[:40])
    _, c1, f1 = idx.bf16_stats()
    assert (c1 - c0) + (f1 - f0) == int((finite & (kept > 0)).sum()) and c1 > c0, (c0, c1, f0, f1)
    idx.close(); f32.close()
    print("child_shadow ok")


def child_opt_out():
    """CQS_HIP_COMBINE_TAGGED=0: the serial path - no tagged pass, the same answers (yardstick: the host-bitset call)."""
    rows, qs, tags, allows = storm_corpus()
    idx = tagged_index(rows, tags)
    want = []
    for i in range(len(qs)):
        r, s, c = idx.search_batch(qs[i], 20, keep_bitset=tc.bits_of(tc.keep_mask(tags, allows[i])))
        want.append((r[0].copy(), s[0].copy(), int(c[0])))
    p, q, total = storm_case(idx, qs, allows, want, rounds=((8, 4),))
    assert (p, q) == (0, 0) and idx.combine_tagged_stats() == (0, 0), (p, q)
    idx.close()
    print("child_opt_out ok")
