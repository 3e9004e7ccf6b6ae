"""The premises of the shadow scans' certificate, observed on the device row by row ("Tests").

The other shadow tests compare final answers with an f32 handle; on Gaussian rows the bound has an order or two of slack, so
an unsound certificate passes them.  Here the library's test hooks (index_shadow.hip: cqs_hip_debug_shadow_stats / _rows /
_scores / _bound_i8) expose what the certificate rests on, and numpy in f64 plus the integer / f32 definition of the stored
copies (shadow_emul.py) is the reference:

  (a) the stored copies, bit for bit;          (b) R and norm are maxima over every finite row, through create, extend
  (c) |s - s~| <= B_q on every row, no slack;      (with and without a regrow), load, disable / re-enable;
  (d) the one-sided PIPELINE drop rules;       (e) B_q of the int8 copy, device against host;
  (f) the numpy emulation against the kernels' score bits, for every NV the launchers use.

Run on an MI355X with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import shadow_emul as em
from cqs_amd import DistanceMetric, HipIndex, _lib, synth

pytestmark = pytest.mark.gpu
ENV_BF16, ENV_I8 = "CQS_HIP_SCAN_BF16", "CQS_HIP_SCAN_I8"
F32, BF16, I8 = 0, 1, 2
I8_MAX_Q = 4                       # scan_i8.h: kI8MaxQ
NT_BYTES = 200 << 20               # index_internal.h: kNtBytes
BUILD_WAVES = 8192 * 4             # launch_shadow_build / launch_i8_build: at most 8192 blocks of 4 waves, one row per wave
FLT_MAX = float(np.finfo(np.float32).max)
DIMS = (16, 128, 264, 272, 768, 1024, 1040, 2048)       # 264: the bf16 copy alone (the int8 copy needs dim % 16 == 0)
NS = (1, 3, 255, 257, 4097)
BIG = ((20_000, 768), (100_003, 128), (300_000, 768))   # the last: above kNtBytes for both copies
BS = {BF16: (1, 2, 3, 4, 5, 8), I8: (1, 2, 3, 4)}


# ---- the hooks --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooks(hip):
    hip.cqs_hip_debug_shadow_stats.restype = C.c_int32
    hip.cqs_hip_debug_shadow_stats.argtypes = [C.c_void_p, C.c_void_p]
    hip.cqs_hip_debug_shadow_rows.restype = C.c_int32
    hip.cqs_hip_debug_shadow_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    hip.cqs_hip_debug_shadow_scores.restype = C.c_int32
    hip.cqs_hip_debug_shadow_scores.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    hip.cqs_hip_debug_shadow_bound_i8.restype = C.c_int32
    hip.cqs_hip_debug_shadow_bound_i8.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return hip


def stats(hooks, h):
    out = np.zeros(4, np.float64)
    assert hooks.cqs_hip_debug_shadow_stats(h._h, out.ctypes.data) == _lib.OK
    return tuple(float(v) for v in out)


def read_bf16(hooks, h, row0=0, rows=None):
    rows = len(h) - row0 if rows is None else rows
    out = np.zeros((rows, h.dim()), np.uint16)
    assert hooks.cqs_hip_debug_shadow_rows(h._h, BF16, row0, rows, out.ctypes.data, None) == _lib.OK
    return out


def read_i8(hooks, h, row0=0, rows=None):
    rows = len(h) - row0 if rows is None else rows
    codes, scales = np.zeros((rows, h.dim()), np.int8), np.zeros(rows, np.float32)
    assert hooks.cqs_hip_debug_shadow_rows(h._h, I8, row0, rows, codes.ctypes.data, scales.ctypes.data) == _lib.OK
    return codes, scales


def score_rows(hooks, h, copy, q, k=20, keep=None, mode=_lib.MODE_RAW, thr=0.0):
    q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float32)
    b, n = q.shape[0], len(h)
    out, bq = np.full((b, n), np.nan, np.float32), np.full(b, np.nan, np.float32)
    rc = hooks.cqs_hip_debug_shadow_scores(h._h, copy, q.ctypes.data, b, k, keep.ctypes.data if keep is not None else None,
                                           mode, thr, out.ctypes.data, bq.ctypes.data)
    assert rc == _lib.OK, (rc, h.last_error())
    assert not np.isnan(out).any() and not np.isnan(bq).any()      # every slot written; dropped rows are -inf
    return out, bq


def setenv(monkeypatch, bf16, i8):
    for name, v in ((ENV_BF16, bf16), (ENV_I8, i8)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def build(monkeypatch, rows, metric=DistanceMetric.DotProduct, shadow=True):
    """Owned handle with both copies (the bf16 one alone where dim % 16 != 0), or on f32 alone."""
    setenv(monkeypatch, "1" if shadow else "0", "1" if shadow else "0")
    h = HipIndex.build_from_flat(None, rows, metric)
    setenv(monkeypatch, None, None)
    n, dim = rows.shape
    if shadow:
        assert h.bf16_stats()[0] == n * dim * 2, h.last_error()
        assert (h.i8_stats()[0] > 0) == (dim % 16 == 0), h.last_error()
    return h


# ---- references -------------------------------------------------------------------------------------------------------
def bf16_values(words):
    return (words.astype(np.uint32) << 16).view(np.float32)


def ref_r_norm(x, xt, gamma):
    """max over the finite rows of ||x - x~|| + gamma (||x|| + ||x~||) and of max(||x||, ||x~||), numpy f64, per row."""
    fin = np.isfinite(x).all(axis=1)
    xd, td = x[fin].astype(np.float64), xt[fin].astype(np.float64)
    nx, nt = np.sqrt((xd * xd).sum(axis=1)), np.sqrt((td * td).sum(axis=1))
    d = xd - td
    return np.sqrt((d * d).sum(axis=1)) + gamma * (nx + nt), np.maximum(nx, nt), fin


def check_stats(hooks, h, x, ctx=""):
    """(b): R_ref <= r <= R_ref (1 + 2^-29), the same for norm, both copies, against the copies read back."""
    r, nm, r8, nm8 = stats(hooks, h)
    dim = x.shape[1]
    up = 1 + 2.0 ** -29          # shadow_convert's own 1 + 2^-30, and f64 summation order (relative error < 2^-40)
    rr, nn, _ = ref_r_norm(x, bf16_values(read_bf16(hooks, h)), em.shadow_gamma(dim))
    assert rr.max() <= r <= rr.max() * up, (ctx, "r", r, rr.max())
    assert nn.max() <= nm <= nn.max() * up, (ctx, "norm", nm, nn.max())
    if dim % 16 == 0:
        codes, scales = read_i8(hooks, h)
        xt = codes.astype(np.float64) * scales.astype(np.float64)[:, None]
        rr8, nn8, fin = ref_r_norm(x, np.where(np.isfinite(xt), xt, 0), em.i8_gamma(dim))
        assert rr8.max() <= r8 <= rr8.max() * up, (ctx, "r8", r8, rr8.max())
        assert nn8.max() <= nm8 <= nn8.max() * up, (ctx, "norm8", nm8, nn8.max())
    return r, nm, r8, nm8


BAD_ROWS = {70: np.nan, 71: np.inf, 72: -np.inf}     # planted where n allows: rows with one non-finite component


def corpus(n, dim, huge=False):
    """adversarial_rows (the rows at rounding midpoints first, then the zero / denormal rows) followed by Gaussian rows of
    mixed norms, with NaN / inf rows from row 70 on.  huge = False leaves out the rows of magnitude 1e17 and 2^64, which
    sit in corpora of their own as in the CPU test."""
    rng = np.random.default_rng(7000 + n + dim)
    adv = em.adversarial_rows(rng, dim)
    order = [8, 13, 19, 12, 9, 10, 11, 14, 15] + ([16, 17, 18] if huge else []) + list(range(8)) + list(range(20, 64))
    g = (rng.standard_normal((max(n, 1), dim)) * rng.uniform(0.1, 3.0, (max(n, 1), 1))).astype(np.float32)
    x = np.concatenate([adv[order], g])[:n].copy()
    for r, v in BAD_ROWS.items():
        if r < n:
            x[r, (r * 7) % dim] = v
    return np.ascontiguousarray(x)


# ---- (a) stored copies ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", NS)
def test_stored_copies_bit_for_bit(hooks, monkeypatch, n, dim):
    x = corpus(n, dim, huge=True)
    h = build(monkeypatch, x)
    words = read_bf16(hooks, h)
    nan = np.isnan(x)
    assert np.array_equal(words[~nan], em.bf16_words(x)[~nan])                      # +-inf included
    assert (((words[nan] & 0x7F80) == 0x7F80) & ((words[nan] & 0x7F) != 0)).all()   # a NaN stays a NaN
    if dim % 16 == 0:
        codes, scales = read_i8(hooks, h)
        fin = np.isfinite(x).all(axis=1)
        want_c, want_s = em.build_i8(x[fin])
        assert np.array_equal(scales[fin].view(np.uint32), want_s.view(np.uint32))
        bad = np.argwhere(codes[fin] != want_c.astype(np.int8))
        assert len(bad) == 0, (n, dim, bad[:5])
        assert np.isnan(scales[~fin]).all() and not codes[~fin].any()               # NaN scale, codes 0
        if n >= 4:
            assert scales[1] == 0 and scales[3] == 0 and 0 < scales[2] < 2.0 ** -126   # denormal / zero rows as designed
    check_stats(hooks, h, x, (n, dim))
    h.close()


# ---- (b) R and norm follow one planted row everywhere -------------------------------------------------------------------
def planted(dim, kind, rng):
    """A row that alone determines R: norm in the thousands against unit rows, every component at a rounding midpoint of the
    int8 codes (kind 0: half-integers times 8 under a maximum of 127 * 8) or of bf16 (kind 1: odd integers of 9 bits)."""
    if kind == 0:
        v = (rng.integers(-126, 126, dim) + 0.5).astype(np.float32) * np.float32(8.0)
        v[0] = 127.0 * 8.0
    else:
        v = (2 * rng.integers(128, 256, dim) + 1).astype(np.float32) * rng.choice([-1.0, 1.0], dim).astype(np.float32)
    return v


def assert_follows(hooks, h, x, pos, ctx):
    r, nm, r8, nm8 = check_stats(hooks, h, x, ctx)
    dim = x.shape[1]
    p = x[pos:pos + 1]
    rr, nn, _ = ref_r_norm(p, em.bf16_round(p), em.shadow_gamma(dim))
    c, s = em.build_i8(p)
    rr8, nn8, _ = ref_r_norm(p, c.astype(np.float64) * s.astype(np.float64)[:, None], em.i8_gamma(dim))
    up = 1 + 2.0 ** -29
    assert rr[0] <= r <= rr[0] * up and rr8[0] <= r8 <= rr8[0] * up, (ctx, r, rr[0], r8, rr8[0])
    assert nn[0] <= nm <= nn[0] * up and nn8[0] <= nm8 <= nn8[0] * up, ctx
    others = np.delete(x, pos, axis=0)
    ro, _, _ = ref_r_norm(others, em.bf16_round(others), em.shadow_gamma(dim))
    assert rr[0] > 10 * ro.max(initial=0), ctx                       # the planted row alone determines R


@pytest.mark.parametrize("kind", [0, 1])
def test_r_follows_a_planted_row_at_create(hooks, monkeypatch, kind):
    rng = np.random.default_rng(90 + kind)
    for n in (1, 5, 6, 7, 4097):
        base = synth.gaussian_unit(n, dim=128, seed=91 + n)
        for pos in sorted({0, n - 1}):
            x = base.copy(); x[pos] = planted(128, kind, rng)
            h = build(monkeypatch, x)
            assert_follows(hooks, h, x, pos, ("create", kind, n, pos))
            h.close()
    # around the build launchers' grid cap: from row BUILD_WAVES on a wave strides to its second, third, fourth row
    n = 100_003
    base = synth.gaussian_unit(n, dim=128, seed=92)
    assert BUILD_WAVES == 32_768
    for pos in (BUILD_WAVES - 1, BUILD_WAVES, 3 * BUILD_WAVES + 1, n - 1):
        x = base.copy(); x[pos] = planted(128, kind, rng)
        h = build(monkeypatch, x)
        assert_follows(hooks, h, x, pos, ("cap", kind, pos))
        h.close()


def test_r_follows_a_planted_row_through_extend(hooks, monkeypatch):
    rng = np.random.default_rng(93)
    dim, n0, m1, m2 = 128, 1000, 500, 300          # cap_rows = 1000 at create; the first extend regrows to 2000, the second fits
    base = synth.gaussian_unit(n0 + m1 + m2, dim=dim, seed=94)
    for pos in (n0, n0 + m1 - 1, n0 + m1, n0 + m1 + m2 - 1, 17):
        x = base.copy(); x[pos] = planted(dim, 0, rng)
        h = build(monkeypatch, x[:n0])
        w0, (c0, s0) = read_bf16(hooks, h), read_i8(hooks, h)
        h.extend(None, x[n0:n0 + m1])
        assert h.bf16_stats()[0] == 2 * n0 * dim * 2                                # regrown to the doubled cap_rows
        assert np.array_equal(read_bf16(hooks, h, 0, n0), w0)                       # the old rows' copies moved unchanged
        c1, s1 = read_i8(hooks, h, 0, n0)
        assert np.array_equal(c1, c0) and np.array_equal(s1.view(np.uint32), s0.view(np.uint32))
        if pos < n0 + m1:
            assert_follows(hooks, h, x[:n0 + m1], pos, ("extend 1", pos))
        else:
            check_stats(hooks, h, x[:n0 + m1], ("extend 1", pos))
        h.extend(None, x[n0 + m1:])
        assert h.bf16_stats()[0] == 2 * n0 * dim * 2                                # ... and this one fitted
        assert_follows(hooks, h, x, pos, ("extend 2", pos))                         # (pos 17: R must not shrink)
        words = read_bf16(hooks, h)
        assert np.array_equal(words, em.bf16_words(x))
        codes, scales = read_i8(hooks, h)
        wc, ws = em.build_i8(x)
        assert np.array_equal(codes, wc.astype(np.int8)) and np.array_equal(scales.view(np.uint32), ws.view(np.uint32))
        fresh = build(monkeypatch, x)
        assert stats(hooks, h) == stats(hooks, fresh), pos
        fresh.close(); h.close()


def test_stats_equal_a_fresh_handle_after_reenable_and_load(hooks, monkeypatch, tmp_path):
    x = corpus(4097, 768)
    fresh = build(monkeypatch, x)
    want = stats(hooks, fresh)
    assert all(np.isfinite(want)) and min(want) > 0
    setenv(monkeypatch, "1", "1")
    fresh.set_bf16_scan(False)
    assert hooks.cqs_hip_debug_shadow_stats(fresh._h, np.zeros(4).ctypes.data) == _lib.ERR_INVALID   # no shadow
    fresh.set_bf16_scan(True)
    assert stats(hooks, fresh) == want
    path = str(tmp_path / "idx.hipflat")
    fresh.save(path)
    loaded = HipIndex.load(path, 768, 4097)
    setenv(monkeypatch, None, None)
    assert stats(hooks, loaded) == want
    check_stats(hooks, loaded, x, "load")
    # a row with a non-finite component and a huge finite remainder takes no part in R
    y = x.copy(); y[100] = np.float32(1e30); y[100, 5] = np.nan
    z = x.copy(); z[100] = 0.0
    hy, hz = build(monkeypatch, y), build(monkeypatch, z)
    assert stats(hooks, hy) == stats(hooks, hz)
    check_stats(hooks, hy, y, "non-finite")
    for h in (fresh, loaded, hy, hz):
        h.close()


# ---- (c) + (f) the premise on every row, and the emulation against the kernels -------------------------------------------
def queries(dim, seed):
    rng = np.random.default_rng(seed)
    qs = []
    for c in (dim - 1, dim - 16, 767, 768, 1023, 1024):      # partial-chunk lanes of either copy
        if 0 <= c < dim and not any(q[c] == 1 and q.sum() == 1 for q in qs):
            q = np.zeros(dim, np.float32); q[c] = 1.0
            qs.append(q)
    qs.append(np.ones(dim, np.float32))
    for s in (1e-3, 1.0, 37.0):
        qs.append((rng.standard_normal(dim) * s).astype(np.float32))
    return np.ascontiguousarray(np.stack(qs))


def dots64(x, qs, step=16384):
    """x [n, dim] (f32 or f64) times qs^T in f64, in row chunks."""
    q64 = qs.astype(np.float64).T
    out = np.empty((x.shape[0], qs.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, x.shape[0], step):
            out[lo:lo + step] = np.where(np.isfinite(x[lo:lo + step]), x[lo:lo + step], 0).astype(np.float64) @ q64
    return out


def norms64(x, step=16384):
    """Row norms in f64; a non-finite component counts as 0 (such rows are checked apart)."""
    out = np.empty(x.shape[0], np.float64)
    for lo in range(0, x.shape[0], step):
        c = np.where(np.isfinite(x[lo:lo + step]), x[lo:lo + step], 0).astype(np.float64)
        out[lo:lo + step] = np.sqrt((c * c).sum(axis=1))
    return out


def instances(copy, b, dim, n):
    """The <NCH, BQ, RI, NT, FULL> instances launch_scan_bf16 / launch_scan_i8 launch for a block of b queries."""
    chunk, elem = (512, 2) if copy == BF16 else (1024, 1)
    nch = (dim + chunk - 1) // chunk
    nt, full = n * dim * elem > NT_BYTES, dim == nch * chunk
    out, left = set(), b
    while left:
        if copy == I8:
            bq, ri, g = (4, 4, min(left, 4)) if left >= 3 else ((2, 8, 2) if left == 2 else (1, 16, 1))
        elif nch <= 2:
            bq, ri, g = (8, 2, min(left, 8)) if left >= 5 else ((4, 4, 4) if left == 4 else ((2, 8, 2) if left >= 2 else (1, 16, 1)))
        else:
            bq, ri, g = (2, 4, 2) if left >= 2 else (1, 8, 1)
        out.add((nch, bq, ri, nt, full))
        left -= g
    return out


# then FULL bf16 chunks at NCH 1 and 3 and a partial one at NCH 4, and the corpora above kNtBytes that reach the non-temporal
# variants of the other chunk counts (bf16: n dim 2 bytes, int8: n dim bytes)
PREMISE = [(n, d) for d in DIMS for n in NS] + list(BIG) + [(257, 512), (257, 1536), (257, 2032)] + \
          [(204_900, 1024), (102_500, 2048), (201_700, 1040), (70_000, 1536), (52_000, 2032), (205_000, 512), (386_000, 272)]


@pytest.mark.parametrize("n,dim", PREMISE)
def test_premise_on_every_row(hooks, monkeypatch, n, dim):
    x = corpus(n, dim)
    qs = queries(dim, 8000 + n + dim)
    nq = len(qs)
    qn = np.sqrt((qs.astype(np.float64) ** 2).sum(axis=1))
    fin = np.isfinite(x).all(axis=1)
    exact = dots64(x, qs)
    rng = np.random.default_rng(n + dim)
    sub = np.unique(np.r_[np.arange(min(n, 160)), np.arange(max(0, n - 96), n), rng.integers(0, n, 256)])   # (f): rows emulated
    emul = {}
    for metric in (DistanceMetric.DotProduct, DistanceMetric.Cosine):
        h = build(monkeypatch, x, metric)
        r, nm, r8, nm8 = stats(hooks, h)
        copies = {BF16: dict(xt=bf16_values(read_bf16(hooks, h)), gamma=em.shadow_gamma(dim), absolute=dim * 2.0 ** -140)}
        copies[BF16]["emul"] = lambda qi, c=copies[BF16]: em.scan_bf16(c["xt"][sub], qs[qi])
        if dim % 16 == 0:
            codes, scales = read_i8(hooks, h)
            copies[I8] = dict(xt=None, gamma=em.i8_gamma(dim), absolute=dim * 2.0 ** -140 * (1 + nm8))
            copies[I8]["emul"] = lambda qi: em.scan_i8(codes[sub].astype(np.float32), scales[sub], qs[qi])
            copies[I8]["stored"] = np.empty((n, nq)); copies[I8]["tn"] = np.empty(n)
            for lo in range(0, n, 16384):
                t = codes[lo:lo + 16384].astype(np.float64) * scales[lo:lo + 16384].astype(np.float64)[:, None]
                t = np.where(np.isfinite(t), t, 0)
                copies[I8]["stored"][lo:lo + 16384] = t @ qs.astype(np.float64).T
                copies[I8]["tn"][lo:lo + 16384] = np.sqrt((t * t).sum(axis=1))
        copies[BF16]["stored"] = dots64(copies[BF16]["xt"], qs)
        copies[BF16]["tn"] = norms64(copies[BF16]["xt"])
        for copy, c in copies.items():
            for b in BS[copy]:
                for i0 in range(0, nq, b):
                    idx = [(i0 + j) % nq for j in range(b)]
                    sa, bq = score_rows(hooks, h, copy, qs[idx])
                    sf, _ = score_rows(hooks, h, F32, qs[idx])
                    assert np.isfinite(bq).all(), (n, dim, copy, idx, bq)         # every B_q here is finite: nothing is skipped
                    for j, qi in enumerate(idx):
                        ctx = (n, dim, metric, copy, b, qi)
                        s, st, B = sf[j].astype(np.float64), sa[j].astype(np.float64), float(bq[j])
                        live = np.isfinite(s)
                        assert np.array_equal(live, fin), ctx                     # the f32 scan keeps exactly the finite rows
                        assert np.isfinite(st[live]).all(), ctx                   # ... and the approximate scan keeps them too
                        assert not np.isfinite(st[~fin]).any(), ctx
                        d1, d2 = np.abs(s[live] - st[live]), np.abs(exact[live, qi] - st[live])
                        assert d1.max(initial=0) <= B, ctx + (d1.max(), B)        # the design's inequality, no tolerance
                        assert d2.max(initial=0) <= B, ctx + (d2.max(), B)
                        # the kernel's own share: rounding of its chain against the f64 dot of the stored copy (whose own
                        # error is < dim 2^-52 ||x~|| ||q||)
                        own = (c["gamma"] + dim * 2.0 ** -52) * c["tn"][live] * qn[qi] + c["absolute"]
                        d3 = np.abs(st[live] - c["stored"][live, qi])
                        assert (d3 <= own).all(), ctx + (int(np.argmax(d3 - own)), d3.max())
                        # (f) the numpy emulation, bit for bit, whatever pass (NV = RI x BQ) carried the query
                        if (copy, qi) not in emul:
                            emul[copy, qi] = c["emul"](qi)
                        want = np.where(np.abs(emul[copy, qi]) <= FLT_MAX, emul[copy, qi], -np.inf).astype(np.float32)
                        same = em.same_scores(sa[j][sub], want)
                        assert same.all(), ctx + (sub[~same][:5], sa[j][sub][~same][:5], want[~same][:5])
        h.close()


def test_the_table_hits_every_scan_instance():
    """The (b, dim, n) table of test_premise_on_every_row reaches every <NCH, BQ, RI, NT, FULL> instance launch_scan_bf16 and
    launch_scan_i8 can pick."""
    pairs = {BF16: {1: ((1, 16), (2, 8), (4, 4), (8, 2)), 2: ((1, 16), (2, 8), (4, 4), (8, 2)), 3: ((1, 8), (2, 4)), 4: ((1, 8), (2, 4))},
             I8: {1: ((1, 16), (2, 8), (4, 4)), 2: ((1, 16), (2, 8), (4, 4))}}
    for copy in (BF16, I8):
        hit = set()
        for n, dim in PREMISE:
            if copy == BF16 or dim % 16 == 0:
                for b in BS[copy]:
                    hit |= instances(copy, b, dim, n)
        every = {(nch, bq, ri, nt, full) for nch, pr in pairs[copy].items() for bq, ri in pr for nt in (False, True) for full in (False, True)}
        assert hit == every, (copy, sorted(every - hit), sorted(hit - every))


@pytest.mark.parametrize("dim,rows_of", [(768, (16,)), (768, (17, 18)), (128, (16,)), (2048, (17, 18))])
def test_premise_on_huge_rows(hooks, monkeypatch, dim, rows_of):
    """The rows of magnitude 1e17 and just under 2^64 in corpora of their own, as the CPU test groups them."""
    rng = np.random.default_rng(1000 + dim)
    adv = em.adversarial_rows(rng, dim)
    x = np.ascontiguousarray(np.concatenate([adv[list(rows_of)]] * 40))
    x *= rng.uniform(0.5, 1.0, (len(x), 1)).astype(np.float32)
    qs = queries(dim, 8100 + dim)
    exact = dots64(x, qs)
    h = build(monkeypatch, x)
    for copy in (BF16, I8):
        for b in (1, 4):
            for i0 in range(0, len(qs), b):
                idx = [(i0 + j) % len(qs) for j in range(b)]
                sa, bq = score_rows(hooks, h, copy, qs[idx])
                sf, _ = score_rows(hooks, h, F32, qs[idx])
                assert np.isfinite(bq).all() and np.isfinite(sf).all() and np.isfinite(sa).all()
                for j, qi in enumerate(idx):
                    s, st = sf[j].astype(np.float64), sa[j].astype(np.float64)
                    assert np.abs(s - st).max() <= float(bq[j]) and np.abs(exact[:, qi] - st).max() <= float(bq[j]), (dim, copy, qi)
    h.close()


def host_bound(q, r, nm, dim, i8):
    """shadow_query_bound / i8_query_bound: where the documented rule refuses a certificate."""
    qn = float(np.sqrt((q.astype(np.float64) ** 2).sum())) * (1 + 2.0 ** -40)
    gam = em.i8_gamma(dim) if i8 else em.shadow_gamma(dim)
    if not qn * nm * (1 + gam) < 2.0 ** 100:
        return np.inf
    if i8 and not qn * 128.0 * np.sqrt(float(dim)) < 2.0 ** 100:
        return np.inf
    return 0.0


def test_bq_is_inf_exactly_where_the_rule_says(hooks, monkeypatch):
    dim = 768
    rng = np.random.default_rng(31)
    unit = synth.gaussian_unit(3000, dim=dim, seed=32)
    g = synth.gaussian_unit(1, dim=dim, seed=33)[0]
    seen = {}
    for scale_rows, scale_q in ((2.0 ** 40, 2.0 ** 60), (2.0 ** -30, 2.0 ** 88)):    # ||q|| norm_max, then 128 sqrt(dim) ||q||, near 2^100
        x = (unit * np.float32(scale_rows)).astype(np.float32)
        a, f = build(monkeypatch, x), build(monkeypatch, x, shadow=False)
        r, nm, r8, nm8 = stats(hooks, a)
        seen[scale_rows] = set()
        for fac in (0.25, 0.9, 1.1, 4.0, 64.0, 2.0 ** 14):
            q = (g * np.float32(scale_q * fac)).astype(np.float32)
            for copy, rr, nn in ((BF16, r, nm), (I8, r8, nm8)):
                _, bq = score_rows(hooks, a, copy, q)
                want = host_bound(q, rr, nn, dim, copy == I8)
                assert np.isinf(bq[0]) == np.isinf(want), (scale_rows, fac, copy, bq)
                seen[scale_rows].add((copy, bool(np.isinf(bq[0]))))
            for k in (1, 20, 100):
                ga, gf = a.search_batch(q, k), f.search_batch(q, k)
                assert np.array_equal(ga[2], gf[2]) and np.array_equal(ga[0], gf[0])
                assert np.array_equal(ga[1].view(np.uint32), gf[1].view(np.uint32))
        # both outcomes for both copies under the first rule; the second refuses the int8 copy alone
        want = {(BF16, False), (I8, False), (I8, True)} | ({(BF16, True)} if scale_rows > 1 else set())
        assert seen[scale_rows] == want, seen
        for bad in (np.nan, np.inf):
            q = g.copy(); q[7] = bad
            for copy in (BF16, I8):
                q2 = np.ascontiguousarray(np.stack([g, q]))
                out = np.zeros((2, len(a)), np.float32); bq = np.zeros(2, np.float32)
                assert hooks.cqs_hip_debug_shadow_scores(a._h, copy, q2.ctypes.data, 2, 20, None, 0, 0.0, out.ctypes.data, bq.ctypes.data) == _lib.OK
                assert np.isfinite(bq[0]) and np.isinf(bq[1]) and bq[1] > 0
        a.close(); f.close()


def test_bound_is_not_vacuous_on_the_device(hooks, monkeypatch):
    """Gaussian unit rows at 768-d (the corpus of test_i8_bound_cpu.py::test_bound_is_not_vacuous): the observed error is within
    the floor of the bound.  bf16: the numpy emulation of the same corpus gives max |s - s~| / B_q = 0.135 (B_q = 0.00198;
    computed again below) and the device must reach a quarter of it."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2000, 768)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[0]
    h = build(monkeypatch, x)
    sf, _ = score_rows(hooks, h, F32, q)
    s8, b8 = score_rows(hooks, h, I8, q)
    err8 = np.abs(sf[0].astype(np.float64) - s8[0]).max()
    print("int8: max |s - s~| = %.6g, B_q = %.6g, ratio %.4f" % (err8, b8[0], err8 / b8[0]))
    assert 0.008 < b8[0] < 0.02 and b8[0] / 50 < err8 <= b8[0]
    s16, b16 = score_rows(hooks, h, BF16, q)
    err16 = np.abs(sf[0].astype(np.float64) - s16[0]).max()
    xt = em.bf16_round(x)
    r_max, _ = em.r_and_norm_bf16(x, xt, 768)
    qn = float(np.sqrt((q.astype(np.float64) ** 2).sum())) * (1 + 2.0 ** -40)
    bq_emul = qn * r_max * (1 + 2.0 ** -40) + 768 * 2.0 ** -140
    ratio_emul = np.abs(em.f32_dot_chain(x, q).astype(np.float64) - em.scan_bf16(xt, q)).max() / bq_emul
    print("bf16: device ratio %.4f, emulated ratio %.4f" % (err16 / b16[0], ratio_emul))
    assert err16 <= b16[0] and err16 / b16[0] >= ratio_emul / 4      # emulated ratio on this corpus: 0.135
    h.close()


# ---- (d) one-sided drop rules -------------------------------------------------------------------------------------------
def test_pipeline_drop_rules_are_one_sided(hooks, monkeypatch):
    n = 30_000
    x = synth.gaussian_unit(n, seed=41)
    qs = synth.gaussian_unit(3, seed=42)
    h = build(monkeypatch, x, DistanceMetric.Cosine)
    raw, _ = score_rows(hooks, h, F32, qs)
    top = np.float32(raw[0].max())
    rng = np.random.default_rng(43)
    keeps = {"absent": None, "1 %": rng.random(n) < 0.01, "90 %": rng.random(n) < 0.9, "all": np.ones(n, bool), "none": np.zeros(n, bool)}
    thrs = [-0.5, 0.0, 0.05, float(np.float32(0.9) * top), float(top), float(np.nextafter(top, np.float32(-1))),
            float(np.nextafter(top, np.float32(2))), 0.999]
    for name, keep in keeps.items():
        words = None
        if keep is not None:
            words = np.zeros((n + 31) // 32, dtype=np.uint32)
            idx = np.nonzero(keep)[0]
            np.bitwise_or.at(words, idx // 32, (np.uint32(1) << (idx % 32).astype(np.uint32)))
        for thr in thrs:
            sf, _ = score_rows(hooks, h, F32, qs, keep=words, mode=_lib.MODE_PIPELINE, thr=thr)
            lf = np.isfinite(sf)
            if keep is not None:
                assert not lf[:, ~keep].any(), (name, thr)
            if thr <= 0.0 and name in ("absent", "all"):
                assert lf.all(), (name, thr)                     # clamp(s) >= thr for every row
            for copy in (BF16, I8):
                sa, bq = score_rows(hooks, h, copy, qs, keep=words, mode=_lib.MODE_PIPELINE, thr=thr)
                la = np.isfinite(sa)
                assert np.isfinite(bq).all()
                if keep is not None:
                    assert not la[:, ~keep].any(), (name, thr, copy)
                assert not (lf & ~la).any(), (name, thr, copy, int((lf & ~la).sum()))   # kept by f32: kept by the copy
                t = np.clip((sa + bq[:, None]).astype(np.float32), np.float32(0), np.float32(1))
                assert (t[lf] >= sf[lf]).all(), (name, thr, copy)                       # clamp(s~ + B_q) >= the stored clamp(s)
                assert (t[la] >= np.float32(thr)).all(), (name, thr, copy)              # and the copy drops what its rule says
    h.close()


# ---- (e) B_q of the int8 copy, device against host -------------------------------------------------------------------------
def test_i8_device_bound_matches_host(hooks, monkeypatch):
    for dim in (16, 128, 768, 2048):
        rows = synth.gaussian_unit(3000, dim=dim, seed=60 + dim)
        rng = np.random.default_rng(dim)
        qs = [rng.standard_normal(dim).astype(np.float32) * s for s in (1.0, 1e-3, 37.0)]
        qs += [np.zeros(dim, np.float32), np.full(dim, 1e30, np.float32), rng.standard_normal(dim).astype(np.float32) * 1e18]
        nan = rng.standard_normal(dim).astype(np.float32); nan[3] = np.nan
        inf = rng.standard_normal(dim).astype(np.float32); inf[5] = np.inf
        qs += [nan, inf]
        q = np.ascontiguousarray(np.stack(qs))
        for tiny in (False, True):
            # tiny rows: a query whose unscaled code sum (<= 127 sqrt(dim) ||q||) could overflow while the scaled score could not
            h = build(monkeypatch, (rows * np.float32(1e-20)).astype(np.float32) if tiny else rows)
            if tiny:
                q[5] = rng.standard_normal(dim).astype(np.float32) * np.float32(2.0 ** 95)
                _, nm, _, nm8 = stats(hooks, h)
                assert np.isinf(host_bound(q[5], 0, nm8, dim, True)) and not np.isinf(host_bound(q[5], 0, nm, dim, False))
            dev, host = np.zeros(len(qs), np.float32), np.zeros(len(qs), np.float32)
            assert hooks.cqs_hip_debug_shadow_bound_i8(h._h, q.ctypes.data, len(qs), dev.ctypes.data, host.ctypes.data) == _lib.OK
            for i in range(len(qs)):
                if np.isinf(host[i]):
                    assert np.isinf(dev[i]) and dev[i] > 0, (dim, i, dev[i], host[i])
                else:
                    assert np.isfinite(dev[i]) and host[i] >= 0, (dim, i)
                    assert dev[i] >= host[i] and dev[i] <= np.nextafter(host[i], np.float32(np.inf)), (dim, i, dev[i], host[i])
            assert np.isinf(host[6]) and np.isinf(host[7])   # non-finite queries: no certificate
            assert np.isinf(host[4])                          # ||q|| past the range
            if tiny:
                assert np.isinf(host[5]) and np.isinf(dev[5])
            h.close()


# ---- the hooks leave a handle as a search leaves it -------------------------------------------------------------------------
def test_hooks_leave_the_scratch_as_a_search_leaves_it(hooks, monkeypatch):
    import torch
    n = 120_000                                              # enough tasks for the bf16 scan's work queue
    x = synth.gaussian_unit(n, seed=51)
    qs = synth.gaussian_unit(8, seed=52)
    h = build(monkeypatch, x, DistanceMetric.Cosine)
    d_q = torch.from_numpy(qs).cuda()

    def dev(nb, k):
        keys = torch.full((nb, k), -1, dtype=torch.int64, device="cuda")
        counts = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        h.search_device(d_q.data_ptr(), nb, k, keys.data_ptr(), counts.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return keys.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes()

    def host(nb, k):
        r, s, c = h.search_batch(qs[:nb], k)
        return r.tobytes(), s.tobytes(), c.tobytes()

    for nb, k in ((1, 20), (4, 80), (8, 200)):
        before = host(nb, k), dev(nb, k)
        for copy in (BF16, I8, F32):
            if copy == I8 and (nb > I8_MAX_Q or k > 87):
                continue
            for mode, thr in ((_lib.MODE_RAW, 0.0), (_lib.MODE_PIPELINE, 0.05)):
                score_rows(hooks, h, copy, qs[:nb], k=k, mode=mode, thr=thr)
                assert (host(nb, k), dev(nb, k)) == before, (nb, k, copy, mode)
    # refused where the handle has no such copy or the copy does not serve the block
    out, bq = np.zeros((5, n), np.float32), np.zeros(5, np.float32)
    assert hooks.cqs_hip_debug_shadow_scores(h._h, I8, qs.ctypes.data, 5, 20, None, 0, 0.0, out.ctypes.data, bq.ctypes.data) == _lib.ERR_INVALID
    f = build(monkeypatch, x[:1000], shadow=False)
    assert hooks.cqs_hip_debug_shadow_scores(f._h, F32, qs.ctypes.data, 1, 20, None, 0, 0.0, out.ctypes.data, bq.ctypes.data) == _lib.ERR_INVALID
    assert hooks.cqs_hip_debug_shadow_rows(f._h, BF16, 0, 1, out.ctypes.data, None) == _lib.ERR_INVALID
    assert hooks.cqs_hip_debug_shadow_rows(h._h, BF16, n, 1, out.ctypes.data, None) == _lib.ERR_INVALID
    h.close(); f.close()
