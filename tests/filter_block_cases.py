"""Shared cases of tests/test_filter_block_gpu.py: one keep-bitset per query (cqs_hip_index_search_filtered and the
combining queue's filtered blocks) against the lone filtered call on the same handle.  Also runnable in a child process
(`python -c "import filter_block_cases as c; c.child_shadow()"`) for handles whose environment is read at create."""
import ctypes as C

import numpy as np

from cqs_amd import DistanceMetric, HipIndex, _lib, synth

FAMILY = 13          # bitsets per corpus, see family()
BLOCKS = (1, 2, 3, 4, 5, 8, 9, 13)
KS = (1, 20, 100, 500)
MODES = ((_lib.MODE_RAW, 0.0), (_lib.MODE_PIPELINE, 0.05))


def pack(keep):
    """bool [n] -> u32 words (bit i % 32 of word i / 32)."""
    b = np.packbits(np.asarray(keep, bool), bitorder="little")
    return np.concatenate([b, np.zeros((-len(b)) % 4, dtype=np.uint8)]).view(np.uint32)


def family(rows, qs, seed):
    """FAMILY bitsets for the queries qs[0, FAMILY): bool [FAMILY, n].
      0, 1, 10  independent random, density 1/2          2, 11  density 1/64 (most batches are skipped)
      3, 4      disjoint halves of every 64-row task (3: rows 0..31, 4: rows 32..63 of each)
      5         one row                                   6      7 rows (fewer than k from k = 20 on)
      7         all-pass                                  8      empty
      9         of every 64 rows only the one that scores highest for query 10 (a neighbour in every block of >= 2 that
                holds both): the maximum of 10's task must not leak into 9's gmax / gaux, nor 9's single row into 10's
      12        every other 64-row task whole (a pass of <= 2 queries takes the pipelined path there)"""
    n = rows.shape[0]
    rng = np.random.default_rng(seed)
    r = np.arange(n)
    f = np.zeros((FAMILY, n), bool)
    for i in (0, 1, 10):
        f[i] = rng.random(n) < 0.5
    for i in (2, 11):
        f[i] = rng.random(n) < 1 / 64
    f[3] = (r % 64) < 32
    f[4] = (r % 64) >= 32
    f[5, int(rng.integers(n))] = True
    f[6, rng.choice(n, 7, replace=False)] = True
    f[7] = True
    s10 = rows @ qs[10]
    pad = np.full((-n) % 64, -np.inf, np.float32)
    arg = np.concatenate([s10, pad]).reshape(-1, 64).argmax(axis=1) + 64 * np.arange((n + 63) // 64)
    f[9, arg[arg < n]] = True
    f[12] = (r // 64) % 2 == 0
    return f


def same(got, want, ctx):
    """rows, score bits and counts of two (rows, scores, counts) answers of ONE query each."""
    (ra, sa, ca), (rb, sb, cb) = got, want
    c = int(cb)
    assert int(ca) == c, (ctx, int(ca), c)
    assert np.array_equal(ra[:c], rb[:c]), ctx
    assert np.array_equal(sa[:c].view(np.uint32), sb[:c].view(np.uint32)), ctx


class Corpus:
    """A handle, FAMILY queries with their bitsets, and the lone filtered answers, computed once per (query, k, mode)."""

    def __init__(self, n, dim, metric=DistanceMetric.Cosine, seed=0):
        self.rows = synth.gaussian_unit(n, dim=dim, seed=7000 + seed + n + dim)
        if metric is DistanceMetric.DotProduct:
            self.rows *= np.random.default_rng(seed).uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        self.qs = synth.gaussian_unit(FAMILY, dim=dim, seed=8000 + seed + n + dim)
        self.keep = family(self.rows, self.qs, 9000 + seed)
        self.bits = np.stack([pack(k) for k in self.keep])
        self.idx = HipIndex.build_from_flat(None, self.rows, metric)
        self._lone = {}

    def lone(self, i, k, mode, thr):
        key = (i, k, mode)
        if key not in self._lone:
            r, s, c = self.idx.search_batch(self.qs[i], k, keep_bitset=self.bits[i], mode=mode, threshold=thr)
            self._lone[key] = (r[0].copy(), s[0].copy(), c[0])
        return self._lone[key]

    def check_block(self, b, k, mode, thr, off=None):
        sel = [((3 * b if off is None else off) + j) % FAMILY for j in range(b)]
        r, s, c = self.idx.search_batch_filtered(self.qs[sel], k, self.bits[sel], mode=mode, threshold=thr)
        for j, i in enumerate(sel):
            same((r[j], s[j], c[j]), self.lone(i, k, mode, thr), (self.rows.shape, b, k, mode, j, i))
            assert self.keep[i][r[j, :c[j]].astype(np.int64)].all(), ("a filtered-out row was returned", b, k, j, i)
        return sel

    def sweep(self, blocks=BLOCKS, ks=KS, modes=MODES):
        for b in blocks:
            for k in ks:
                for mode, thr in modes:
                    self.check_block(b, k, mode, thr)

    def close(self):
        self.idx.close()


def storm_filtered(idx, qs, bits, k, n_threads, per_thread):
    """cqs_hip_debug_client_storm_filtered: native threads, one query and its bitset per call.  -> (rows, scores, counts)."""
    fn = idx._lib.cqs_hip_debug_client_storm_filtered
    fn.restype = C.c_double
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                   C.c_void_p, C.c_void_p, C.c_void_p]
    q = np.ascontiguousarray(qs, dtype=np.float32)
    kb = np.ascontiguousarray(bits, dtype=np.uint32)
    nq = len(q)
    r = np.zeros((nq, k), np.uint64); s = np.zeros((nq, k), np.float32); c = np.zeros((nq,), np.uint32)
    el = fn(idx._h, q.ctypes.data, nq, q.shape[1], k, kb.ctypes.data, kb.shape[1], n_threads, per_thread,
            r.ctypes.data, s.ctypes.data, c.ctypes.data)
    assert el > 0, "a storm call failed"
    return r, s, c


def storm_case(c, k=20, rounds=((8, 6), (16, 6))):
    """The filtered storm over corpus c: every answer equals the lone call's; -> (filtered passes, filtered queries)."""
    want = [c.lone(i, k, _lib.MODE_RAW, 0.0) for i in range(FAMILY)]
    p0, q0 = c.idx.combine_filter_stats()
    u0 = c.idx.combine_stats()
    total = 0
    for n_threads, per_thread in rounds:
        r, s, cnt = storm_filtered(c.idx, c.qs, c.bits, k, n_threads, per_thread)
        total += n_threads * per_thread
        for i in range(FAMILY):
            same((r[i], s[i], cnt[i]), want[i], ("storm", n_threads, i))
    p1, q1 = c.idx.combine_filter_stats()
    assert c.idx.combine_stats() == u0, "filtered traffic moved the unfiltered counters"
    return p1 - p0, q1 - q0, total


# ---- children: the environment is read when the handle is made -----------------------------------------------------
def child_shadow():
    """CQS_HIP_SCAN_BF16=1 CQS_HIP_SCAN_I8=1: the blocks go through the shadow copies and are certified there."""
    c = Corpus(140_005, 768)
    by, by8 = c.idx.bf16_stats()[0], c.idx.i8_stats()[0]
    assert by > 0 and by8 > 0, "the shadow copies were not built"
    c.sweep(blocks=(2, 5, 9), ks=(20, 500))
    c.sweep(blocks=(3, 13), ks=(100,), modes=MODES[:1])

    def deltas(b, k):   # (certified, fallbacks, int8-certified) of ONE block, its lone answers computed beforehand
        for j in range(b):
            c.lone((3 * b + j) % FAMILY, k, _lib.MODE_RAW, 0.0)
        (_, c0, f0), (_, e0, _) = c.idx.bf16_stats(), c.idx.i8_stats()
        c.check_block(b, k, _lib.MODE_RAW, 0.0)
        (_, c1, f1), (_, e1, _) = c.idx.bf16_stats(), c.idx.i8_stats()
        return c1 - c0, f1 - f0, e1 - e0

    cert, fb, _ = deltas(13, 100)
    assert cert + fb == 12 and cert >= 1, ("a block of 13 (one empty bitset) did not go through the shadow", cert, fb)
    cert, fb, cert8 = deltas(4, 20)
    assert cert + fb == 4 and cert8 >= 1, ("a block of 4 at k = 20 was not served by the int8 copy", cert, fb, cert8)
    c.close()
    small = Corpus(5003, 768)
    small.sweep(ks=(20, 500))
    small.close()
    print("child_shadow ok")


def child_adversarial():
    """The half-ulp rows of test_bf16_scan_gpu.py, crowded scores: queries whose k-th and (k'+1)-th kept scores are closer
    than B_q cannot be certified and are redone on the f32 scan with their own bitsets."""
    from test_bf16_scan_gpu import adversarial_corpus
    rng = np.random.default_rng(61)
    dim = 768
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    rows = adversarial_corpus(rng, sign, 1500, 2.0 ** -5, 1.05 * 2.0 ** -5)
    n = len(rows)
    q_adv = (sign * np.float32(1 / 32)).astype(np.float32)
    qs = np.stack([q_adv, -q_adv, q_adv, synth.gaussian_unit(1, seed=62)[0], -q_adv])
    keep = np.stack([np.ones(n, bool), np.random.default_rng(1).random(n) < 0.5, np.random.default_rng(2).random(n) < 0.9,
                     np.random.default_rng(3).random(n) < 0.5, np.arange(n) % 3 != 0])
    bits = np.stack([pack(k) for k in keep])
    idx = HipIndex.build_from_flat(None, rows)
    f32 = HipIndex.build_from_flat(None, rows)
    f32.set_bf16_scan(False)                                   # the yardstick: lone calls on the f32 scan
    assert idx.bf16_stats()[0] > 0 and f32.bf16_stats()[0] == 0
    for k in (20, 100):
        want = [f32.search_batch(qs[i], k, keep_bitset=bits[i]) for i in range(len(qs))]
        _, _, fb0 = idx.bf16_stats()
        r, s, c = idx.search_batch_filtered(qs, k, bits)
        _, _, fb1 = idx.bf16_stats()
        print("adversarial k", k, "fallbacks of the block", fb1 - fb0)
        assert fb1 - fb0 >= 1, "the adversarial block never fell back to the f32 scan"
        for i in range(len(qs)):
            same((r[i], s[i], c[i]), (want[i][0][0], want[i][1][0], want[i][2][0]), ("adversarial", k, i))
    idx.close(); f32.close()
    print("child_adversarial ok")


def child_opt_out():
    """CQS_HIP_COMBINE_FILTERED=0: the parent's serial path - no filtered pass, the same answers."""
    c = Corpus(140_005, 768)
    p, q, total = storm_case(c, rounds=((8, 4),))
    assert (p, q) == (0, 0), (p, q)
    c.close()
    print("child_opt_out ok")
