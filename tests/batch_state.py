"""Shared by tests/test_batch_state_gpu.py and tests/test_batch_state_sensitivity_cpu.py (test infrastructure, next to
query_state.py whose oracle-side helpers it reuses): the batch chain (`run_layers` in cqs_amd/csrc/embedder_run.hip) token by
token.  `HipEmbedEngine.run_hidden` returns the f32 final-norm row of every token of a packed ragged batch; the oracle
side is built one sequence at a time.

Two instruments:
  * the MASK PROBE - crafted one-layer weights under which a token's final hidden row spells out which keys it attended
    (uniform attention, a key's value is one-hot at a dim that tags its position and its sequence), checked by a derived
    ratio band; random weights cannot show a mask error at the real window of 257;
  * random weights on narrow-window geometries, every row held to `query_state.measures` bounds = 3 x the device's measured
    worst distance to the fp32 oracle."""
import contextlib
import ctypes as C
import json
import os

import numpy as np

import query_state as Q
from oracle import gemma3_ref as G


def variant(cfg, **kw):
    d = dict(cfg.__dict__)
    d.update(kw)
    return G.GemmaConfig(**d)


# ---- Part B: random weights ---------------------------------------------------------------------------------------------
SMALL = variant(Q.SMALL, max_seq=512)                 # query_state.SMALL's tensors (max_seq only sizes the RoPE table)
GEOMS = {"small": (SMALL, 31), "full_w32": (Q.FULL_W32, 35)}
# above the 512-row few-rows limit, partly filled 128- and 256-row tiles (1259 tokens); and under it (268 tokens)
BATCHES = {"over": [300, 257, 129, 64, 33, 1, 273, 200, 2], "under": [70, 1, 33, 64, 100]}


def weights(cfg, seed, wset):
    w = G.seeded_weights(cfg, seed=seed)
    return Q.peaked(cfg, w) if wset == "peaked" else w


def seq_ids(cfg, lens, seed=5000):
    """One (ids [1, n], mask [1, n]) per sequence of the batch - what the oracle-side helpers take."""
    return [Q.ids_for(cfg, n, seed=seed + 97 * b + n) for b, n in enumerate(lens)]


def padded(seqs):
    """The same sequences as one right-padded [B, L] batch - what the engine takes."""
    L = max(i.shape[1] for i, _ in seqs)
    ids = np.zeros((len(seqs), L), np.int64)
    mask = np.zeros((len(seqs), L), np.int64)
    for b, (i, _) in enumerate(seqs):
        ids[b, : i.shape[1]] = i[0]
        mask[b, : i.shape[1]] = 1
    return ids, mask


def head_from_rows(w, rows):
    """The head on its own: mean of the given token rows in float64, Dense 1, Dense 2 (bf16 operands, as the device's
    GEMMs take them).  A pool that reads one packed row too many or too few differs from this at full size."""
    pooled = np.asarray(rows, np.float64).mean(0)
    d1 = G.round_bf16(pooled.astype(np.float32)).astype(np.float64) @ w["dense1.weight"].astype(np.float64).T
    return G.round_bf16(d1.astype(np.float32)).astype(np.float64) @ w["dense2.weight"].astype(np.float64).T


def leak_plant(cfg, w, layer, neighbour_qkv_row, neighbour_pos, n_queries=16):
    """Plant for record(): in `layer`, the first `n_queries` queries also attend one key of the neighbouring packed
    sequence (its row of the same layer's qkv tap, at its own position)."""
    import torch
    keep = {}

    def plant(s, l, t):
        if s == "qkv":
            keep[l] = t[0].numpy().copy()
        if s == "attn" and l == layer:
            a = Q.attn_from_qkv(cfg, w, l, keep[l], leak=(neighbour_qkv_row(l), neighbour_pos, n_queries))
            return torch.from_numpy(a.astype(np.float32))[None]
        return None
    return plant


# ---- Part A: the mask probe ---------------------------------------------------------------------------------------------
# one packed ragged batch: both sides of the 16-query tiles, the 32-key blocks (register kernel), the 64-key blocks (DMA
# kernel), the 128-query super-blocks and the window of 257; 6462 tokens, 64 super-blocks: the planner's defaults apply
# (head-sharing DMA attention, pair-split add-norm)
PROBE_LENS = [1, 2, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 272, 273, 300,
              511, 512, 513, 600]
# the same lengths in another order: every seq_start / vt_start falls at another offset
PROBE_LENS_2 = PROBE_LENS[::-2] + PROBE_LENS[-2::-2]
# forced forms: one length of each boundary class
PROBE_SUBSET = [17, 600, 1, 64, 257, 33, 129, 16, 258, 193, 513, 65, 273, 2]
PROBE_ONE = [300]                                     # too few blocks for the shared layout by default
HEAD_LAYOUTS = {"3:1": (3, 1), "2:1": (2, 1), "4:1": (4, 1), "4:2": (4, 2), "2:2": (2, 2)}
WINDOWS = {"w17": (32, 2), "w257": (512, 2), "full": (512, 1)}        # (sliding_window, sliding_pattern) of the one layer


def probe_config(layout, wcase):
    heads, kv = HEAD_LAYOUTS[layout]
    sw, pat = WINDOWS[wcase]
    return G.GemmaConfig(vocab_size=512, hidden=heads * 256, layers=1, heads=heads, kv_heads=kv, head_dim=256, intermediate=1152,
                         dense_hidden=256, sliding_window=sw, sliding_pattern=pat, max_seq=1024)


def probe_weights(cfg, seed=3):
    """Every norm weight 0; embed_tokens[t] one-hot at dim t % 256; q_proj = 0 (every score 0: attention is uniform over
    the allowed keys); k_proj seeded (no influence); v_proj[d, d] = 1/32 on each kv head; o_proj the identity (the heads
    stay side by side); down_proj = 0 (the FFN branch adds exactly 0).  All values are bf16-exact."""
    assert cfg.layers == 1 and cfg.hidden == cfg.heads * 256 and cfg.head_dim == 256
    w = G.seeded_weights(cfg, seed=seed)
    for k in w:
        if k.endswith("norm.weight") or k.endswith("layernorm.weight"):
            w[k] = np.zeros_like(w[k])
    e = np.zeros_like(w["embed_tokens.weight"])
    e[np.arange(cfg.vocab_size), np.arange(cfg.vocab_size) % 256] = 1.0
    w["embed_tokens.weight"] = e
    p = "layers.0."
    w[p + "self_attn.q_proj.weight"] = np.zeros_like(w[p + "self_attn.q_proj.weight"])
    v = np.zeros_like(w[p + "self_attn.v_proj.weight"])
    for j in range(cfg.kv_heads):
        v[j * 256 + np.arange(256), np.arange(256)] = 1.0 / 32.0
    w[p + "self_attn.v_proj.weight"] = v
    w[p + "self_attn.o_proj.weight"] = np.eye(cfg.hidden, dtype=np.float32)
    w[p + "mlp.down_proj.weight"] = np.zeros_like(w[p + "mlp.down_proj.weight"])
    return w


def probe_seq(b, n):
    """Sequence `b` of a probe batch, `n` tokens: position p carries token 256 + (p + 37 b) % 256 - a key is tagged by its
    position and its sequence, so a row of the neighbouring packed sequence that leaks in lights another dim."""
    return (256 + (np.arange(n) + 37 * b) % 256).astype(np.int64)[None], np.ones((1, n), np.int64)


def probe_batch(lens):
    return padded([probe_seq(b, n) for b, n in enumerate(lens)])


# The band is derived, not measured.  A dim's level = (attended keys that map to it) / (keys attended).  One key too few
# moves a dim by a factor 0, 1/2 or 2/3; one key too many by inf, 2 or 3/2; the renormalisation by the changed key count
# shifts every dim by at most 1/17 (17 = the fewest keys a window-17 token attends: 1.5 x 17/18 = 1.42, 2/3 x 18/17 = 0.71
# stay outside); bf16 rounding of the operands is below 1 %.
PROBE_BAND = (0.8, 1.25)
PROBE_ZERO = 0.25            # an oracle-zero element stays below this fraction of the row-and-region's smallest non-zero one


def probe_violations(got, ref, ids, mask, heads):
    """got / ref [B, L, H] final hidden rows, per token row and per head region of 256 dims.  -> list of
    (sequence, position, head, dim, got, ref), empty if the band accepts.  A dim names a key: dim d of sequence b is the
    key(s) at positions p with (p + 37 b) % 256 == d.  The token's own dim is skipped in head 0's region (the residual
    stream adds there); heads 1 and up show it cleanly."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    live = np.asarray(mask).astype(bool)
    bad_rows = []
    if np.any(got[~live] != 0):
        b, p = np.argwhere(np.any(got != 0, -1) & ~live)[0]
        bad_rows.append((int(b), int(p), -1, -1, float(np.abs(got[b, p]).max()), 0.0))         # a padded row is exactly 0
    own = (np.asarray(ids) % 256)[..., None]
    regions = []
    for r in range(heads):
        f = ref[..., r * 256:(r + 1) * 256]
        use = np.broadcast_to(live[..., None], f.shape).copy()
        if r == 0:
            np.put_along_axis(use, own, False, axis=-1)
        regions.append((f, use))
    rowmin = np.min([np.where(u & (f != 0), np.abs(f), np.inf).min(-1) for f, u in regions], 0)      # [B, L]
    for r, (f, use) in enumerate(regions):
        g = got[..., r * 256:(r + 1) * 256]
        nz = use & (f != 0)
        floor = np.where(nz, np.abs(f), np.inf).min(-1)
        floor = np.where(np.isfinite(floor), floor, rowmin)[..., None]         # (a region left empty by the skipped own dim)
        ratio = np.where(nz, g / np.where(nz, f, 1.0), 1.0)
        bad = (nz & ((ratio < PROBE_BAND[0]) | (ratio > PROBE_BAND[1]))) | (use & (f == 0) & ~(np.abs(g) < PROBE_ZERO * floor))
        for b, p, d in np.argwhere(bad)[:6]:
            bad_rows.append((int(b), int(p), r, int(d), float(g[b, p, d]), float(f[b, p, d])))
    return bad_rows


# ---- the engine side ----------------------------------------------------------------------------------------------------
def engine(cfg, w):
    from cqs_amd.embedder import HipEmbedEngine, default_config
    c = default_config()
    c.vocab_size, c.hidden, c.layers, c.heads, c.kv_heads = cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads
    c.head_dim, c.intermediate, c.dense_hidden = cfg.head_dim, cfg.intermediate, cfg.dense_hidden
    c.sliding_window, c.sliding_pattern, c.max_seq = cfg.sliding_window, cfg.sliding_pattern, cfg.max_seq
    c.query_pre_attn_scalar = cfg.query_pre_attn_scalar
    eng = HipEmbedEngine(c)
    eng.set_weights(w)
    return eng


def _hook(eng, name, *args):
    f = getattr(eng._lib, name)
    f.restype = None
    f.argtypes = [C.c_void_p] + [C.c_uint32 if isinstance(a, tuple) else C.c_int32 for a in args]
    f(eng._h, *[a[0] if isinstance(a, tuple) else int(a) for a in args])


ENV = {"layout": "CQS_HIP_ATT_LAYOUT", "kernel": "CQS_HIP_ATT_KERNEL", "tile": "CQS_HIP_GEMM_TILE"}   # all read per call
FUSE_NORM_DEFAULT = (2, 4096)                          # cqs_hip_embedder's own: the pair-split kernel from 4096 tokens on


@contextlib.contextmanager
def form(eng, layout=None, kernel=None, tile=None, fuse_qkv=True, fuse_norm=FUSE_NORM_DEFAULT, geglu4=True):
    """Run the engine in one kernel form: the three per-call environment switches and the three debug hooks; the
    environment and the engine's defaults are put back on the way out."""
    saved = {v: os.environ.get(v) for v in ENV.values()}
    try:
        for k, val in (("layout", layout), ("kernel", kernel), ("tile", tile)):
            if val is None:
                os.environ.pop(ENV[k], None)
            else:
                os.environ[ENV[k]] = val
        _hook(eng, "cqs_hip_debug_embedder_set_fuse_qkv", fuse_qkv)
        _hook(eng, "cqs_hip_debug_embedder_set_fuse_norm", fuse_norm[0], (fuse_norm[1],))
        _hook(eng, "cqs_hip_debug_embedder_set_geglu4", geglu4)
        yield eng
    finally:
        for v, old in saved.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old
        _hook(eng, "cqs_hip_debug_embedder_set_fuse_qkv", True)
        _hook(eng, "cqs_hip_debug_embedder_set_fuse_norm", FUSE_NORM_DEFAULT[0], (FUSE_NORM_DEFAULT[1],))
        _hook(eng, "cqs_hip_debug_embedder_set_geglu4", True)


# ---- bounds -------------------------------------------------------------------------------------------------------------
# (1 - cos, element, column) per (geometry, weight set) and place, each 3 x the worst distance of the device to the fp32
# oracle measured on an MI355X over every form tests/test_batch_state_gpu.py runs (DESIGN.md 3.8c holds the table; the
# margin is the search-time check's, for the same reason: box-to-box and association differences).  "hidden" = the
# final-norm row of a token; "pool" = eng.run's sentence vector against the head applied to the device's own rows.
# MEASURED = the device's worst over all forms; beside each line the bf16-operand emulation of a correct device on the same
# inputs (forward_emulated, on a CPU; full depth): the device sits where a correct one is expected.
MEASURED = {
    ("full_w32", "plain"): {"hidden": (3.091e-05, 0.04686, 0.02124), "pool": (4.196e-07, 3.785e-03, 3.785e-03)},    # emulated 3.083e-05 0.0407 0.0165
    ("full_w32", "peaked"): {"hidden": (3.344e-03, 0.3785, 0.03981), "pool": (3.636e-09, 3.530e-04, 3.530e-04)},    # emulated 2.868e-03 0.3615 0.0443
    ("small", "plain"): {"hidden": (6.170e-05, 0.05437, 0.02740), "pool": (3.553e-15, 6.475e-07, 6.475e-07)},       # emulated 7.233e-05 0.0498 0.0274
    ("small", "peaked"): {"hidden": (4.891e-03, 0.4010, 0.04231), "pool": (8.216e-15, 4.716e-07, 4.716e-07)},       # emulated 5.592e-03 0.4383 0.0423
    # the probe, worst over the five head layouts (the figures depend on the hidden size only: 2:1 = 2:2, 4:1 = 4:2)
    ("probe", "w17"): {"hidden": (1.905e-10, 1.373e-03, 3.349e-05)},      # emulated 1.894e-10 1.366e-03 3.351e-05 (worst of 512 / 768 / 1024 wide)
    ("probe", "w257"): {"hidden": (6.520e-08, 8.098e-03, 2.495e-04)},     # emulated 6.520e-08 8.098e-03 2.496e-04
    ("probe", "full"): {"hidden": (1.049e-06, 8.329e-03, 2.423e-03)},     # emulated 1.049e-06 8.329e-03 2.423e-03
}
BOUNDS = {k: {place: tuple(3.0 * x for x in m) for place, m in v.items()} for k, v in MEASURED.items()}


class Tally:
    """Collects every comparison of one test, prints each figure (visible with pytest -s), and asserts at the end - after
    the worst figures were reported, so that one run shows all of them (CQS_BATCH_STATE_REPORT=<file> appends them as JSON
    lines: how the MEASURED table above was taken)."""

    def __init__(self, name, bounds=None, tag="BSTATE", report_env="CQS_BATCH_STATE_REPORT"):
        self.name, self.worst, self.failed = name, {}, []
        self.bounds, self.tag, self.report_env = BOUNDS if bounds is None else bounds, tag, report_env     # (bert_state.py brings its own table)

    def add(self, place, key, got, ref, what):
        m = Q.measures(got, ref)
        w0 = self.worst.setdefault((key, place), [0.0, 0.0, 0.0])
        for i in range(3):
            w0[i] = max(w0[i], m[i])
        b = self.bounds[key][place]
        print("%s-ROW %s %s %s 1-cos=%.3e elem=%.4f col=%.4f (bounds %.3e %.4f %.4f)" % (self.tag, what, "/".join(key), place, *m, *b))
        if not (m[0] < b[0] and m[1] < b[1] and m[2] < b[2]):
            self.failed.append((what, place, key, m, b))
        return m

    def fail(self, what):
        self.failed.append(what)

    def finish(self):
        path = os.environ.get(self.report_env)
        for (key, place), m in sorted(self.worst.items()):
            print("%s %s %s %s 1-cos=%.3e elem=%.4f col=%.4f" % (self.tag, self.name, "/".join(key), place, m[0], m[1], m[2]))
            if path:
                with open(path, "a") as f:
                    f.write(json.dumps({"test": self.name, "key": list(key), "place": place, "one_minus_cos": m[0], "elem": m[1], "col": m[2]}) + "\n")
        assert not self.failed, (len(self.failed), self.failed[:8])


def passes(key, got_hidden, ref_hidden, place="hidden"):
    m, b = Q.measures(got_hidden, ref_hidden), BOUNDS[key][place]
    return m[0] < b[0] and m[1] < b[1] and m[2] < b[2]
