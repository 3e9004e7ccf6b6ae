"""Shared by the row-tag tests (test_tags_host_cpu.py, test_tags_gpu.py, test_sparse_tags_gpu.py): the per-row rule of
include/cqs_hip.h ("row tags") restated in numpy, the host bitset of a predicate, and the filters every row count is
checked under.  Nothing here calls the library."""
import numpy as np

ALL = np.full(32, 0xFFFFFFFF, dtype=np.uint32)


def allow_of(*sets):
    """32 words from up to four collections of allowed codes (None: the field is unconstrained) - written against the
    header's sentence, not through cqs_amd.tag_filter: bit v of field f's set is bit v % 32 of word 8 f + v // 32."""
    a = np.zeros(32, dtype=np.uint32)
    sets = list(sets) + [None] * (4 - len(sets))
    for f, s in enumerate(sets):
        for v in (range(256) if s is None else s):
            a[8 * f + v // 32] |= np.uint32(1) << np.uint32(v % 32)
    return a


def keep_mask(tags, allow):
    """bool [n]: row i is kept iff, for every field f, bit (tag_i >> 8 f) & 255 of field f's set is set."""
    tags = np.asarray(tags, dtype=np.uint32)
    allow = np.asarray(allow, dtype=np.uint32)
    keep = np.ones(tags.shape, dtype=bool)
    for f in range(4):
        v = (tags >> np.uint32(8 * f)) & np.uint32(255)
        keep &= ((allow[8 * f + (v >> np.uint32(5))] >> (v & np.uint32(31))) & np.uint32(1)).astype(bool)
    return keep


def bits_of(mask):
    """The host keep-bitset of a bool mask: ceil(n / 32) u32 words, little-endian bit order, bits past n zero."""
    packed = np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
    out = np.zeros((len(mask) + 31) // 32 * 4, dtype=np.uint8)
    out[:packed.size] = packed
    return out.view(np.uint32)


def random_tags(n, seed):
    """Tags whose every field is drawn from a handful of codes that include 0 and 255, so that filters over single
    codes keep a sizeable share of the rows and the two edge values are always present at larger n."""
    rng = np.random.default_rng(seed)
    codes = np.array([0, 1, 2, 31, 32, 33, 128, 254, 255], dtype=np.uint32)
    t = np.zeros(n, dtype=np.uint32)
    for f in range(4):
        t |= codes[rng.integers(0, len(codes), size=n)] << np.uint32(8 * f)
    return t


def filters_for(tags, seed):
    """name -> allow, the filters of the issue for one tag array: all-pass; an empty set in one field; one value in each
    field in turn; random half-full sets in all four fields; only value 255; only the first row kept; only the last."""
    rng = np.random.default_rng(seed)
    tags = np.asarray(tags, dtype=np.uint32)
    out = {"all_pass": ALL.copy(), "empty_field_2": allow_of(None, None, [], None)}
    for f in range(4):
        sets = [None] * 4
        sets[f] = [int((tags[len(tags) // 2] >> np.uint32(8 * f)) & np.uint32(255))]
        out[f"one_value_field_{f}"] = allow_of(*sets)
    out["half_full"] = allow_of(*[[int(v) for v in np.flatnonzero(rng.random(256) < 0.5)] for _ in range(4)])
    out["only_255"] = allow_of([255], None, None, None)
    for name, row in (("first_row", 0), ("last_row", len(tags) - 1)):
        out[name] = allow_of(*[[int((tags[row] >> np.uint32(8 * f)) & np.uint32(255))] for f in range(4)])
    return out


def unique_end_tags(n, seed):
    """random_tags with the first and the last row given tags no other row has, so that `first_row` / `last_row` of
    filters_for keep exactly one row."""
    t = random_tags(n, seed)
    t[0] = 0x07070707
    t[-1] = 0x09090909 if n > 1 else t[-1]
    return t
