"""Shared by tests/test_query_state_gpu.py, tests/test_query_state_sensitivity_cpu.py and tests/batch_state.py (test infrastructure, like
shadow_emul.py): the per-token measures, their committed bounds, the oracle-side recording through
`gemma3_ref.forward(tap=...)`, the planted errors, and a bf16-operand emulation of a correct device.

The search-time chain (cqs_amd/csrc/query_forward.hip) pools its token rows on the device; a mean over T tokens divides
a one-row error by about T, which is why the pooled-vector bounds of test_query_path_gpu.py (cos > 0.999) let every
error below through except the window ones.  Here each token row is compared on its own."""
import math

import numpy as np

from oracle import gemma3_ref as G

SMALL = G.GemmaConfig(vocab_size=512, hidden=256, layers=3, heads=2, kv_heads=1, head_dim=256, intermediate=384,
                      dense_hidden=512, sliding_window=32, sliding_pattern=3, max_seq=256)
# EmbeddingGemma's per-layer geometry, 4 layers incl. one full-attention layer (test_query_path_full_geometry's)
FULL = G.GemmaConfig(vocab_size=4096, hidden=768, layers=4, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                     dense_hidden=3072, sliding_window=512, sliding_pattern=2, max_seq=2048)
# the same with a window (17) that cuts inside every key tile and across the seam between the two key halves
FULL_W32 = G.GemmaConfig(vocab_size=4096, hidden=768, layers=4, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                         dense_hidden=3072, sliding_window=32, sliding_pattern=2, max_seq=2048)
GEOMS = {"small": (SMALL, 31), "full": (FULL, 35), "full_w32": (FULL_W32, 35)}

# every length where a plan of cqs_amd/csrc/query_plan.h changes form (tests/test_query_plan_cpu.py holds the two together), and one on either side of each ...
BREAKS = [1, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 128]
# ... and partly filled last blocks: T % 8 and T % 16 zero and non-zero inside every class
PARTIAL = [2, 3, 7, 12, 13, 24, 27, 40, 43, 56, 59, 72, 75, 88, 91, 104, 112, 123]
LENS = sorted(BREAKS + PARTIAL)


def cut(cfg, layers):
    """`cfg` with its first `layers` layers: seeded_weights draws one stream per tensor index, so the layer tensors are
    those of the full config (the final norm and the Dense head are the cut config's own)."""
    d = dict(cfg.__dict__)
    d["layers"] = layers
    return G.GemmaConfig(**d)


def peaked(cfg, w):
    """The second weight set: every q_norm weight moved so that (1 + w) is 4 x larger - scores 4 x larger, softmax sharp:
    position and mask errors dominate the attention output instead of being averaged away."""
    out = dict(w)
    for i in range(cfg.layers):
        k = f"layers.{i}.self_attn.q_norm.weight"
        out[k] = (np.float32(4.0) * (np.float32(1.0) + w[k]) - np.float32(1.0)).astype(np.float32)
    return out


def ids_for(cfg, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, cfg.vocab_size, size=(1, n)).astype(np.int64), np.ones((1, n), np.int64)


def rms64(x, wt, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * (1.0 + np.asarray(wt, np.float64))


# ---- the oracle side ---------------------------------------------------------------------------------------------------
def record(cfg, w, ids, mask, plant=None):
    """fp32 oracle forward with every tapped tensor of every layer recorded: {(stage, layer): [T, *]} + "hidden" [T, H]
    (final norm) + "pooled" [H] (mean over tokens of hidden) + "out" [H].  `plant(stage, layer, tensor)` may replace values."""
    rec = {}

    def tap(stage, layer, t):
        r = plant(stage, layer, t) if plant else None
        rec[(stage, layer)] = (t if r is None else r)[0].numpy().copy()
        return r

    rec["out"] = G.forward(cfg, w, ids, mask, tap=tap)[0]
    last = cfg.layers - 1
    rec["hidden"] = rms64(rec[("layer_out", last)], w["norm.weight"], cfg.rms_eps)
    rec["pooled"] = rec["hidden"].mean(0)
    return rec


def attn_from_qkv(cfg, w, layer, qkv, window_delta=0, late_from=None, mask_last_key_for=None, rnd=lambda a: a, leak=None):
    """The attention of `layer` restated from its (tapped) qkv rows [T, (nh + 2 nkv) D] -> [T, nh D], in float64, with
    switches for the errors a kernel can make: the window compare off by `window_delta`; keys at positions >= late_from
    rotated one position late; the last key masked for the queries >= mask_last_key_for; leak = (qkv row of another
    sequence, its position there, n): that row attended as one more key by the queries < n (a packed batch's neighbour
    read past a sequence's end).  rnd rounds the MFMA operands."""
    n_own = qkv.shape[0]
    if leak is not None:
        qkv = np.concatenate([qkv, np.asarray(leak[0], qkv.dtype)[None]], 0)     # (the row rides along as token T; dropped below)
    T = qkv.shape[0]
    D, nh, nkv = cfg.head_dim, cfg.heads, cfg.kv_heads
    p = f"layers.{layer}."
    q = qkv[:, : nh * D].reshape(T, nh, D).astype(np.float64)
    k = qkv[:, nh * D: (nh + nkv) * D].reshape(T, nkv, D).astype(np.float64)
    v = qkv[:, (nh + nkv) * D:].reshape(T, nkv, D).astype(np.float64)
    q = rms64(q, w[p + "self_attn.q_norm.weight"], cfg.rms_eps)
    k = rms64(k, w[p + "self_attn.k_norm.weight"], cfg.rms_eps)
    full = cfg.is_full(layer)
    theta = cfg.rope_theta_global if full else cfg.rope_theta_local
    inv = 1.0 / (theta ** (np.arange(0, D, 2, dtype=np.float64) / D))

    def rope(t, pos):
        fr = pos[:, None] * inv[None, :]
        c, s = np.cos(np.concatenate([fr, fr], -1))[:, None, :], np.sin(np.concatenate([fr, fr], -1))[:, None, :]
        rot = np.concatenate([-t[..., D // 2:], t[..., : D // 2]], -1)
        return t * c + rot * s

    pos = np.arange(T, dtype=np.float64)
    if leak is not None:
        pos[-1] = float(leak[1])
    kpos = pos.copy()
    if late_from is not None:
        kpos[late_from:] -= 1.0
    q = rnd(rope(q, pos) * cfg.query_pre_attn_scalar ** -0.5)
    k = rnd(rope(k, kpos))
    v = rnd(v)
    dist = np.abs(np.arange(T)[:, None] - np.arange(T)[None, :])
    allow = np.ones((T, T), bool) if full else dist < cfg.window + window_delta
    if mask_last_key_for is not None:
        allow = allow.copy()
        allow[mask_last_key_for:, n_own - 1] = False           # (the last token loses itself too; it keeps its other keys)
    if leak is not None:
        allow = allow.copy()
        allow[:, -1] = False
        allow[-1, :] = False
        allow[: leak[2], -1] = True
        allow[-1, -1] = True
    out = np.zeros((T, nh, D))
    for h in range(nh):
        s = q[:, h] @ k[:, h // (nh // nkv)].T
        s = np.where(allow, s, -np.inf)
        e = rnd(np.exp(s - s.max(-1, keepdims=True)))
        out[:, h] = (e @ v[:, h // (nh // nkv)]) / e.sum(-1, keepdims=True)
    return out.reshape(T, nh * D)[:n_own]


def forward_emulated(cfg, w, ids, rnd=G.round_bf16):
    """A correct device, emulated: the forward restated in float64 with every GEMM operand (activations, softmax weights;
    the weights already are bf16) passed through `rnd`.  rnd = identity restates the fp32 oracle (pinned in the CPU test).
    -> the same dictionary as record()."""
    r64 = lambda a: rnd(np.asarray(a, np.float32)).astype(np.float64) if rnd is not None else np.asarray(a, np.float64)
    W = {k: v.astype(np.float64) for k, v in w.items()}
    x = W["embed_tokens.weight"][ids[0]] * np.float64(np.float32(math.sqrt(cfg.hidden)))
    rec = {}
    for i in range(cfg.layers):
        p = f"layers.{i}."
        h = r64(rms64(x, w[p + "input_layernorm.weight"], cfg.rms_eps))
        qkv = r64(np.concatenate([h @ W[p + "self_attn.q_proj.weight"].T, h @ W[p + "self_attn.k_proj.weight"].T,
                                  h @ W[p + "self_attn.v_proj.weight"].T], -1))
        rec[("qkv", i)] = qkv
        a = r64(attn_from_qkv(cfg, w, i, qkv, rnd=r64))
        rec[("attn", i)] = a
        x = x + rms64(r64(a @ W[p + "self_attn.o_proj.weight"].T), w[p + "post_attention_layernorm.weight"], cfg.rms_eps)
        rec[("post_attn", i)] = x
        h = r64(rms64(x, w[p + "pre_feedforward_layernorm.weight"], cfg.rms_eps))
        g = h @ W[p + "mlp.gate_proj.weight"].T
        g = 0.5 * g * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))
        m = r64(r64(g * (h @ W[p + "mlp.up_proj.weight"].T)) @ W[p + "mlp.down_proj.weight"].T)
        rec[("ffn", i)] = m
        x = x + rms64(m, w[p + "post_feedforward_layernorm.weight"], cfg.rms_eps)
        rec[("layer_out", i)] = x
    rec["hidden"] = rms64(x, w["norm.weight"], cfg.rms_eps)
    rec["pooled"] = rec["hidden"].mean(0)
    rec["out"] = (r64(r64(rec["pooled"]) @ W["dense1.weight"].T) @ W["dense2.weight"].T)
    return rec


# ---- the planted errors (section 5 of the issue's table + one stage-level error per tap point) ------------------------
def planted_errors(cfg, w, layer, T):
    """name -> plant callback for record(), for a query of T tokens.  One layer unless the name says otherwise."""
    import torch
    D = cfg.head_dim
    keep = {}

    def at(stage, fn):
        def plant(s, l, t):
            if s == "post_attn" and l == layer:
                keep["post_attn"] = t.clone()
            return fn(t.clone()) if (s == stage and l == layer) else None
        return plant

    def attn_with(every_layer=False, **kw):
        def plant(s, l, t):
            if s == "qkv":
                keep[("qkv", l)] = t[0].numpy().copy()
            if s == "attn" and (every_layer or l == layer):
                return torch.from_numpy(attn_from_qkv(cfg, w, l, keep[("qkv", l)], **kw).astype(np.float32))[None]
            return None
        return plant

    def zero_last(t): t[:, -1] = 0; return t
    def swap_heads(t):
        a = t[:, -1, :D].clone(); t[:, -1, :D] = t[:, -1, D:2 * D]; t[:, -1, D:2 * D] = a; return t
    def copy_row(t): t[:, -1] = t[:, -2]; return t
    def skip_ffn(t): t[:, -1] = keep["post_attn"][:, -1]; return t

    errs = {
        "last token's attention output zeroed": at("attn", zero_last),
        "two heads swapped on the last token": at("attn", swap_heads),
        "last token's FFN row copied from its neighbour": at("ffn", copy_row),
        "last key masked for the last 16-query block": attn_with(mask_last_key_for=16 * ((T - 1) // 16)),
        "stage qkv: last token's row copied from its neighbour": at("qkv", copy_row),
        "stage post_attn: last token's row copied from its neighbour": at("post_attn", copy_row),
        "stage layer_out: last token's FFN branch not added": at("layer_out", skip_ffn),
    }
    if T > 64:
        errs["keys >= 64 rotated one position late (every layer)"] = attn_with(every_layer=True, late_from=64)
    if not cfg.is_full(layer) and cfg.window < T:
        errs["window one too wide"] = attn_with(window_delta=1)
        errs["window one too narrow"] = attn_with(window_delta=-1)
    return errs


# ---- the measures ------------------------------------------------------------------------------------------------------
def measures(got, ref):
    """[T, H] against [T, H], in float64.  -> (worst 1 - cos over the token rows, largest element error / mean |ref|,
    largest per-column error / mean |ref|).  A column's error is its MEAN |error| over the tokens: the largest single
    element of a column is the global maximum again, while a column tile written wrong is wrong in every row - its mean
    stands out of the per-row rounding noise by a factor that grows with T."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    cs = (got * ref).sum(-1) / (np.linalg.norm(got, axis=-1) * np.linalg.norm(ref, axis=-1) + 1e-300)
    err = np.abs(got - ref)
    scale = np.abs(ref).mean()
    return float(1.0 - cs.min()), float(err.max() / scale), float(err.mean(0).max() / scale)


# Bounds per (geometry, weight set): place -> (1 - cos, element, column), each 3 x the worst distance of the device to
# the fp32 oracle measured over the whole grid (every depth, every length of LENS) on an MI355X - DESIGN.md, "Per-token
# check of the search-time chain", holds the measured values.  "resid" = the f32 residual stream (entering the head, and
# after the last layer), "hidden" = the final-norm hidden state rebuilt from it, "pool" = pooled vector / Dense 1 / output.
# Measured worst distances (1 - cos, element, column) of the grid test, MI355X, every depth x every length of LENS:
#   small    plain   resid 6.66e-5 0.0499 0.0271 | hidden 6.60e-5 0.0590 0.0272 | pool 1.62e-6 0.0149
#   full     plain   resid 2.63e-5 0.0397 0.0207 | hidden 2.58e-5 0.0419 0.0220 | pool 1.48e-6 0.0200
#   full_w32 plain   resid 2.87e-5 0.0376 0.0207 | hidden 2.84e-5 0.0402 0.0220 | pool 1.50e-6 0.0200
#   small    peaked  resid 7.25e-3 0.4982 0.0468 | hidden 7.01e-3 0.5038 0.0477 | pool 1.67e-6 0.0154
#   full     peaked  resid 3.34e-3 0.3943 0.0396 | hidden 3.41e-3 0.3866 0.0452 | pool 1.48e-6 0.0162
#   full_w32 peaked  resid 2.04e-3 0.2728 0.0396 | hidden 2.07e-3 0.3132 0.0452 | pool 1.49e-6 0.0180
# (the bf16-operand emulation of a correct device, forward_emulated, gives 2.3e-5 - 6.0e-5 and 0.036 - 0.041 for the plain
# sets at 33 tokens: the device sits where a correct one is expected).  Each bound = 3 x its measured value.
def _x3(*m):
    return tuple(3.0 * v for v in m)


BOUNDS = {
    ("small", "plain"): {"resid": _x3(6.66e-5, 0.0499, 0.0271), "hidden": _x3(6.60e-5, 0.0590, 0.0272), "pool": _x3(1.62e-6, 0.0149, 0.0149)},
    ("full", "plain"): {"resid": _x3(2.63e-5, 0.0397, 0.0207), "hidden": _x3(2.58e-5, 0.0419, 0.0220), "pool": _x3(1.48e-6, 0.0200, 0.0200)},
    ("full_w32", "plain"): {"resid": _x3(2.87e-5, 0.0376, 0.0207), "hidden": _x3(2.84e-5, 0.0402, 0.0220), "pool": _x3(1.50e-6, 0.0200, 0.0200)},
    ("small", "peaked"): {"resid": _x3(7.25e-3, 0.4982, 0.0468), "hidden": _x3(7.01e-3, 0.5038, 0.0477), "pool": _x3(1.67e-6, 0.0154, 0.0154)},
    ("full", "peaked"): {"resid": _x3(3.34e-3, 0.3943, 0.0396), "hidden": _x3(3.41e-3, 0.3866, 0.0452), "pool": _x3(1.48e-6, 0.0162, 0.0162)},
    ("full_w32", "peaked"): {"resid": _x3(2.04e-3, 0.2728, 0.0396), "hidden": _x3(2.07e-3, 0.3132, 0.0452), "pool": _x3(1.49e-6, 0.0180, 0.0180)},
}


def check(place, key, got, ref, what, worst=None):
    """Print the three figures (visible with pytest -s), fold them into `worst` (a dict), assert BOUNDS[key][place]."""
    m = measures(got, ref)
    if worst is not None:
        w0 = worst.setdefault((key, place), [0.0, 0.0, 0.0])
        for i in range(3):
            w0[i] = max(w0[i], m[i])
    b = BOUNDS[key][place]
    print("QSTATE-ROW %s %s %s 1-cos=%.3e elem=%.4f col=%.4f (bounds %.3e %.4f %.4f)" % (what, "/".join(key), place, *m, *b))
    assert m[0] < b[0] and m[1] < b[1] and m[2] < b[2], (what, place, key, m, b)
    return m


def passes(key, got_rec, ref_rec, layers):
    """Do the per-token bounds accept `got_rec` against `ref_rec` (both record() dictionaries)?"""
    last = layers - 1
    for place, g, r in (("resid", got_rec[("post_attn", last)], ref_rec[("post_attn", last)]),
                        ("resid", got_rec[("layer_out", last)], ref_rec[("layer_out", last)]),
                        ("hidden", got_rec["hidden"], ref_rec["hidden"])):
        m, b = measures(g, r), BOUNDS[key][place]
        if not (m[0] < b[0] and m[1] < b[1] and m[2] < b[2]):
            return False
    return True
