"""Numpy emulation of the shadow scans' arithmetic (cqs_amd/csrc/scan_bf16.hip, scan_i8.hip), shared by the
CPU bound tests (test_bf16_bound_cpu.py, test_i8_bound_cpu.py) and the device test of the certificate's premises
(test_shadow_premises_gpu.py), which compares it with what the kernels store and compute.

What is emulated, step for step:
  bf16_round        shadow_build_kernel's stored words (round to nearest even, NaN stays NaN).
  build_i8          i8_build_kernel's codes and scales (f32 max, f32 division by 127, f32 x / scale, rint, clamp).
  scan_i8           scan_i8_kernel's score: per lane an (even, odd) f32 FMA chain over the chunks in order, even + odd, the xor
                    butterfly 32 -> 1 (the tree treduce<NV> builds for every NV: each node adds the same two partial sums
                    and IEEE addition commutes), times the row's scale.
  scan_bf16         scan_bf16_kernel's score: the same with 512-component chunks of 8 components per lane and no scale.
`fma32` is exact (one rounding, as the hardware FMA): the f64 sum is rounded to odd before the conversion to f32.

One step is not reproduced: a lane of a partial last chunk multiplies the clamped in-row components by a +0 query
fragment, which can give -0 where the emulation's zero padding gives +0.  A sum can differ in the sign of a zero only;
`same_scores` compares bits up to that.
"""
import numpy as np


def shadow_gamma(dim):
    """scan_bf16.h shadow_gamma, the same f64 operations."""
    du = float(dim) * 2.0 ** -24
    return du / (1.0 - du)


def i8_gamma(dim):
    """scan_i8.h i8_gamma."""
    return shadow_gamma(dim + 2)


def bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def bf16_words(x):
    """The stored 16-bit words of shadow_build_kernel: bf16_round for every finite or infinite value; a NaN stays a NaN
    (which NaN is the converter's business: compare with np.isnan on both sides)."""
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def build_i8(x):
    """i8_build_kernel: scale = max|x_i| / 127 in f32 (0 when that underflows), codes = clamp(rint(x_i / scale)) in f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    scale = (np.abs(x).max(axis=1) / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = np.rint((x / scale[:, None]).astype(np.float32))
    c = np.where(scale[:, None] > 0, c, np.float32(0))
    return np.clip(c, -127, 127).astype(np.float32), scale


def fma32(a, b, acc):
    """f32 fma(a, b, acc) for `a` of at most 8 significant bits (an int8 code, a bf16 value): the product is exact in f64
    (8 + 24 bits).  The f64 sum is rounded to odd (TwoSum gives its error), so the conversion to f32 rounds once."""
    c = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        t = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, t, s).astype(np.float32)


def _butterfly(v):
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lanes ^ m]).astype(np.float32)
    return v[:, 0]


def scan_i8(codes, scale, q):
    """scan_i8_kernel for one query: lane L owns components [c*1024 + 16 L, +16) of chunk c; per 4-byte word two packed FMAs
    into an (even, odd) accumulator pair, chunk after chunk; even + odd; xor butterfly 32 -> 1; times the row's scale."""
    n, dim = codes.shape
    nch = (dim + 1023) // 1024
    pad = nch * 1024
    cp = np.zeros((n, pad), np.float32); cp[:, :dim] = codes
    qp = np.zeros(pad, np.float32); qp[:dim] = q                      # a partial chunk meets a zero query fragment
    cp = cp.reshape(n, nch, 64, 4, 4)                                 # [row, chunk, lane, word, byte]
    qp = qp.reshape(nch, 64, 4, 4)
    ax = np.zeros((n, 64), np.float32); ay = np.zeros((n, 64), np.float32)
    for c in range(nch):
        for w in range(4):
            ax = fma32(cp[:, c, :, w, 0], qp[c, :, w, 0][None], ax); ay = fma32(cp[:, c, :, w, 1], qp[c, :, w, 1][None], ay)
            ax = fma32(cp[:, c, :, w, 2], qp[c, :, w, 2][None], ax); ay = fma32(cp[:, c, :, w, 3], qp[c, :, w, 3][None], ay)
    with np.errstate(invalid="ignore", over="ignore"):
        v = _butterfly((ax + ay).astype(np.float32))
        return (v * scale).astype(np.float32)


def scan_bf16(xt, q):
    """scan_bf16_kernel for one query, xt = the bf16 copy as f32 values: lane L owns components [c*512 + 8 L, +8) of chunk c,
    four packed FMAs (components 0 2 4 6 into the even accumulator, 1 3 5 7 into the odd one), chunk after chunk; even + odd;
    xor butterfly 32 -> 1."""
    n, dim = xt.shape
    nch = (dim + 511) // 512
    pad = nch * 512
    xp = np.zeros((n, pad), np.float32); xp[:, :dim] = xt
    qp = np.zeros(pad, np.float32); qp[:dim] = q
    xp = xp.reshape(n, nch, 64, 4, 2)                                 # [row, chunk, lane, word, half]
    qp = qp.reshape(nch, 64, 4, 2)
    ax = np.zeros((n, 64), np.float32); ay = np.zeros((n, 64), np.float32)
    for c in range(nch):
        for w in range(4):
            ax = fma32(xp[:, c, :, w, 0], qp[c, :, w, 0][None], ax)
            ay = fma32(xp[:, c, :, w, 1], qp[c, :, w, 1][None], ay)
    with np.errstate(invalid="ignore", over="ignore"):
        return _butterfly((ax + ay).astype(np.float32))


def same_scores(got, want):
    """Bit equality of two f32 arrays up to the sign of a zero (module docstring) and to which NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))


def f32_dot_chain(x, q):
    """Sequential f32 dot (one rounding per product and per add): the worst order the bound must cover for the f32 scan."""
    acc = np.zeros(x.shape[0], np.float32)
    for i in range(x.shape[1]):
        acc = (acc + (x[:, i] * q[i]).astype(np.float32)).astype(np.float32)
    return acc


def r_and_norm(driver, x, codes, scale, dim):
    """What the int8 build folds into stats[0..1], from the stored codes and scale, in f64, with shadow_convert's 2^-30
    slack.  driver: the C++ header driver of test_i8_bound_cpu.py, or None for the same formula in Python."""
    gam = float(driver("gamma", dim)[0]) if driver is not None else i8_gamma(dim)
    xd = x.astype(np.float64)
    td = codes.astype(np.float64) * scale.astype(np.float64)[:, None]
    nx, nt = np.linalg.norm(xd, axis=1), np.linalg.norm(td, axis=1)
    r = np.linalg.norm(xd - td, axis=1) + gam * (nx + nt)
    return float(r.max()) * (1 + 2.0 ** -30), float(max(nx.max(), nt.max())) * (1 + 2.0 ** -30)


def r_and_norm_bf16(x, xt, dim):
    """The bf16 counterpart: R = max ||x - x~|| + gamma (||x|| + ||x~||), norm = max(||x||, ||x~||), gamma = shadow_gamma(dim),
    f64, with the same 2^-30 slack."""
    gam = shadow_gamma(dim)
    xd, td = x.astype(np.float64), xt.astype(np.float64)
    nx, nt = np.linalg.norm(xd, axis=1), np.linalg.norm(td, axis=1)
    r = np.linalg.norm(xd - td, axis=1) + gam * (nx + nt)
    return float(r.max()) * (1 + 2.0 ** -30), float(max(nx.max(), nt.max())) * (1 + 2.0 ** -30)


def adversarial_rows(rng, dim):
    x = (rng.standard_normal((64, dim)) * rng.uniform(0.1, 3.0, (64, 1))).astype(np.float32)
    x[:8] = np.abs(x[:8])                                                   # signs aligned with an all-positive query
    half = (rng.integers(-126, 126, dim) + 0.5).astype(np.float32)          # every component at a rounding midpoint
    half[0] = 127.0
    x[8] = half * np.float32(1.0 / 127)
    x[9] = half * np.float32(3.0)
    x[10] = 0.0; x[10, dim // 2] = 5.0                                      # one dominant component, the rest zero
    x[11] = rng.standard_normal(dim).astype(np.float32) * np.float32(1e-3); x[11, 1] = 40.0   # ... the rest below half a step
    x[12] = 0.0                                                             # a zero row (scale 0, codes 0)
    x[13] = np.float32(1e-44)                                               # denormal: max / 127 underflows to 0, codes 0
    x[19] = np.float32(1e-42); x[19, 3] = np.float32(3e-42)                 # denormal row with a denormal, nonzero scale
    x[14] = x[14] * np.float32(1e-30)                                       # tiny scale
    x[15] = x[15] * np.float32(1e-36)                                       # products with q underflow
    x[16] = x[16] * np.float32(1e17)                                        # huge scale
    x[17] = (x[17] / np.abs(x[17]).max()) * np.float32(2.0 ** 64 * (1 - 2.0 ** -20))   # just under the 2^64 refusal
    x[18] = -x[17]
    return x
