"""Shared by tests/test_bert_state_gpu.py and tests/test_bert_state_sensitivity_cpu.py (test infrastructure, next to
query_state.py / batch_state.py whose `measures` and `Tally` it reuses): the three BERT-family engines (bert_run.hip,
bert_kernels.hip, the bias / GELU / ROWMAX epilogues of gemm_kernels.hip and embed_gemm.hip, query_gemm.hip's small-rows
forms) token row by token row.  `HipBertEngine.hidden` returns the final hidden row of every live token of a packed
ragged batch (bf16 on the device, widened); the oracle side is oracle/bert_ref.encode (fp32).

  * `forward64` - the encoder restated in numpy float64 with a `rnd` hook at every place the device stores bf16 and a
    `plant` hook at every stage.  rnd = identity restates the oracle (pinned on the CPU); rnd = bf16 IS THE EMULATION OF A
    CORRECT DEVICE, and every bound below is 3 x the emulation's own worst distance to the fp32 oracle (EMULATED): no
    figure measured on a device feeds a bound (DESIGN.md 3.8d records where the device sits).
  * the MASK PROBE - crafted one-layer weights under which a token's final hidden row spells out which keys it attended,
    checked per row and head region by a derived band (PROBE_KEYS, PROBE_REL).
  * the heads on their own (`pool64`, `rerank64`, `splade64`), computed from the device's own hidden rows."""
import contextlib
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                # (as tests/conftest.py does: `python tests/bert_state.py` prints the table)
    sys.path.insert(0, ROOT)

import query_state as Q
from oracle import bert_ref as R


def ident(a):
    return np.asarray(a, np.float64)


def bf16(a):
    """A value as the device stores it: rounded to bf16 (from its f32 value, as the kernels' epilogues do)."""
    return R.bf16_round(np.asarray(a, np.float64).astype(np.float32)).astype(np.float64)


def gelu64(x):
    import torch
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())


def ln64(x, g, b, eps, no_mean_in_variance=False):
    """LayerNorm in float64.  no_mean_in_variance: the planted error "the variance without the mean subtracted"."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = (x * x).mean(-1, keepdims=True) if no_mean_in_variance else ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def lin64(w, name, x):
    return np.asarray(x, np.float64) @ w[name + ".weight"].astype(np.float64).T + w[name + ".bias"].astype(np.float64)


def attention64(cfg, qkv, rnd=ident, keys=None, allow=None):
    """Bidirectional attention of one sequence restated from its qkv rows [T, 3H] -> [T, H], the way the kernels compute
    it: scores from the stored q and k (the 1 / sqrt(d) scale rides in the exponent), p = rnd(exp(s - max)) - the
    resident-key kernel feeds bf16 probabilities to the matrix cores - and numerator and row sum from the same p.
    keys [E, 3H]: further qkv rows that ride along as keys T .. T + E - 1; allow [T, T + E] bool: who attends what
    (default: every query its own sequence's T keys) - the switches of the planted mask errors."""
    qkv = np.asarray(qkv, np.float64)
    T, H, nh, d = qkv.shape[0], cfg.hidden, cfg.heads, cfg.head_dim
    kv = qkv if keys is None else np.concatenate([qkv, np.asarray(keys, np.float64)], 0)
    if allow is None:
        allow = np.zeros((T, kv.shape[0]), bool)
        allow[:, :T] = True
    q = qkv[:, :H].reshape(T, nh, d)
    k = kv[:, H:2 * H].reshape(-1, nh, d)
    v = kv[:, 2 * H:].reshape(-1, nh, d)
    out = np.zeros((T, nh, d))
    for h in range(nh):
        s = np.where(allow, q[:, h] @ k[:, h].T, -np.inf)
        p = rnd(np.exp((s - s.max(-1, keepdims=True)) / math.sqrt(d)))
        out[:, h] = (p @ v[:, h]) / p.sum(-1, keepdims=True)
    return out.reshape(T, H)


STAGES = ("emb", "qkv", "attn", "attn_proj", "ln1", "ffn1", "ffn2", "ln2")      # every bf16 store of the encoder, in order


def forward64(cfg, w, ids, tt=None, rnd=ident, plant=None):
    """One sequence (ids [T], token types [T]) through the encoder in float64.  `rnd` is applied wherever the device
    stores bf16: the embedding LN output, qkv, the attention probabilities (inside attention64) and output, each
    projection's output, the GELU output, each LN output.  `plant(stage, layer, tensor, rec)` may return a replacement
    for any stage of STAGES (rec = what was recorded so far: a plant can redo a stage from its inputs).
    -> {(stage, layer): [T, *]} + "hidden" [T, H]."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    T = ids.shape[0]
    tt = np.zeros(T, np.int64) if tt is None else np.asarray(tt, np.int64).reshape(-1)
    rec = {}

    def tap(stage, layer, t):
        r = plant(stage, layer, t, rec) if plant else None
        rec[(stage, layer)] = t if r is None else np.asarray(r, np.float64)
        return rec[(stage, layer)]

    e = "embeddings."
    x = (w[e + "word_embeddings.weight"][ids].astype(np.float64) + w[e + "position_embeddings.weight"][:T].astype(np.float64) +
         w[e + "token_type_embeddings.weight"][tt].astype(np.float64))
    rec[("emb_raw", -1)] = x
    x = tap("emb", -1, rnd(ln64(x, w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], cfg.ln_eps)))
    for l in range(cfg.layers):
        p = f"encoder.layer.{l}."
        qkv = tap("qkv", l, rnd(np.concatenate([lin64(w, p + "attention.self." + n, x) for n in ("query", "key", "value")], -1)))
        a = tap("attn", l, rnd(attention64(cfg, qkv, rnd)))
        y = tap("attn_proj", l, rnd(lin64(w, p + "attention.output.dense", a)))
        x1 = tap("ln1", l, rnd(ln64(x + y, w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"], cfg.ln_eps)))
        h = tap("ffn1", l, rnd(gelu64(lin64(w, p + "intermediate.dense", x1))))
        y2 = tap("ffn2", l, rnd(lin64(w, p + "output.dense", h)))
        x = tap("ln2", l, rnd(ln64(x1 + y2, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], cfg.ln_eps)))
    rec["hidden"] = x
    return rec


def layer_input(rec, layer):
    """The residual stream that enters `layer` (what ln1's residual add reads)."""
    return rec[("emb", -1)] if layer == 0 else rec[("ln2", layer - 1)]


# ---- the heads, from given packed rows [M, H] + the packing (starts, lens) ----------------------------------------------
def packing(lens):
    lens = np.asarray(lens, np.int64)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), lens


def pool64(rows, lens, mode, plant=None):
    """`mean_pool` / `cls_pool` of every sequence, float64; an empty sequence gives zeros.  plant("pool_span", b, (lo,
    hi)) may return another row range."""
    rows = np.asarray(rows, np.float64)
    starts, lens = packing(lens)
    out = np.zeros((len(lens), rows.shape[1]))
    for b, (lo, n) in enumerate(zip(starts, lens)):
        if n == 0:
            continue
        lo, hi = int(lo), int(lo + n)
        r = plant("pool_span", b, (lo, hi)) if plant else None
        lo, hi = (lo, hi) if r is None else r
        out[b] = rows[lo] if mode == "cls" else rows[lo:hi].mean(0)
    return out


def rerank64(cfg, w, rows, lens, rnd=ident):
    """BertPooler on each sequence's first row (dense + tanh, stored bf16: `rnd`) + the classifier -> [B, num_labels]."""
    starts, _ = packing(lens)
    pooled = rnd(np.tanh(lin64(w, "pooler.dense", np.asarray(rows, np.float64)[starts])))
    return lin64(w, "classifier", pooled)


def vocab_pad(cfg):
    return (cfg.vocab_size + 191) // 192 * 192                  # bert_engine.hip: the decoder's N, a multiple of its 192-wide tile


def splade64(cfg, w, rows, lens, rnd=ident, plant=None):
    """The masked-LM head + SPLADE pooling: transform + GELU (bf16), its LN (bf16), the decoder tied to the zero-padded
    word embeddings with the ROWMAX epilogue (max over a sequence's rows of max(0, logit), f32), ln(1 + .) -> [B, vocab].
    plant("logits", None, [M, vpad]) may replace the padded logits, plant("rowmax_span", b, (lo, hi)) the row range."""
    V, vp = cfg.vocab_size, vocab_pad(cfg)
    t = rnd(gelu64(lin64(w, "cls.predictions.transform.dense", rows)))
    r = plant("mlm_ln", None, t) if plant else None      # (gets the LN's INPUT, returns its output)
    t = rnd(ln64(t, w["cls.predictions.transform.LayerNorm.weight"], w["cls.predictions.transform.LayerNorm.bias"], cfg.ln_eps)) if r is None else r
    logits = np.zeros((t.shape[0], vp))
    logits[:, :V] = t @ w["embeddings.word_embeddings.weight"].astype(np.float64).T + w["cls.predictions.bias"].astype(np.float64)
    r = plant("logits", None, logits) if plant else None
    logits = logits if r is None else r
    starts, lens = packing(lens)
    pooled = np.zeros((len(lens), vp))
    for b, (lo, n) in enumerate(zip(starts, lens)):
        lo, hi = int(lo), int(lo + n)
        r = plant("rowmax_span", b, (lo, hi)) if plant else None
        lo, hi = (lo, hi) if r is None else r
        if hi > lo:
            pooled[b] = np.maximum(logits[lo:hi].max(0), 0.0)
    return np.log1p(pooled)[:, :V]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def config(hidden, heads, inter, layers=2, vocab=500, num_labels=1):
    return R.BertConfig(vocab_size=vocab, hidden=hidden, layers=layers, heads=heads, intermediate=inter, max_pos=512, num_labels=num_labels)


def weights(cfg, head, seed, wset="plain"):
    """"plain" = bert_ref.seeded_weights; "peaked" = the same with every layer's query weight and bias 4 x larger (exact
    in bf16): scores 4 x larger, the softmax sharp - position and mask errors dominate a token's attention output instead
    of being averaged away (what query_state.peaked does for the gemma chain); "shifted" = plain with rows that have a
    MEAN, as a real checkpoint's do: + 0.125 on the word embeddings (1.4 deviations of a raw embedding row), + 0.25 on every
    LN beta, + 0.5 on the biases of attention.output.dense and output.dense - every LayerNorm input then has a mean of
    0.3 - 1.4 of its deviation.  Seeded weights alone give zero-mean rows, on which a variance taken as E[x^2] is right."""
    w = R.seeded_weights(cfg, head, seed=seed)
    if wset == "peaked":
        for l in range(cfg.layers):
            for s in ("weight", "bias"):
                k = f"encoder.layer.{l}.attention.self.query.{s}"
                w[k] = (np.float32(4.0) * w[k]).astype(np.float32)
    if wset == "shifted":
        for k in w:
            if k == "embeddings.word_embeddings.weight":
                w[k] = R.bf16_round(w[k] + np.float32(0.125))
            elif k.endswith("LayerNorm.bias"):
                w[k] = (w[k] + np.float32(0.25)).astype(np.float32)
            elif k.endswith("attention.output.dense.bias") or k.endswith(".output.dense.bias"):
                w[k] = (w[k] + np.float32(0.5)).astype(np.float32)
    return w


WSETS = ("plain", "peaked", "shifted")


def seqs_for(cfg, lens, seed):
    """(ids int32 [n], token types int32 [n]) per sequence; the token type changes inside every sequence of 2+ tokens."""
    out = []
    for b, n in enumerate(lens):
        rng = np.random.default_rng(seed + 97 * b + n)
        out.append((rng.integers(1, cfg.vocab_size, size=n).astype(np.int32), (np.arange(n) >= (n + 1) // 2).astype(np.int32)))
    return out


def oracle_rows(cfg, w, seqs):
    """fp32 oracle (bert_ref.encode on the right-padded live sequences) -> one [n, H] array per sequence (empty: [0, H])."""
    live = [i for i, (s, _) in enumerate(seqs) if len(s)]
    L = max(len(seqs[i][0]) for i in live)
    ids, mask, tt = (np.zeros((len(live), L), np.int64) for _ in range(3))
    for j, i in enumerate(live):
        s, t = seqs[i]
        ids[j, :len(s)], mask[j, :len(s)], tt[j, :len(s)] = s, 1, t
    ref = R.encode(cfg, w, ids, mask, tt).numpy()
    out = [np.zeros((0, cfg.hidden), np.float32) for _ in seqs]
    for j, i in enumerate(live):
        out[i] = ref[j, :len(seqs[i][0])]
    return out


def split_rows(rows, lens):
    starts, lens = packing(lens)
    return [rows[int(s):int(s + n)] for s, n in zip(starts, lens)]


# ---- Part B: every GEMM regime --------------------------------------------------------------------------------------------
def gemm_regime(M, N, K):
    """`launch_gemm_bias`'s choice restated (embed_gemm.hip; test_bert_state_sensitivity_cpu.py holds the constants to
    the source)."""
    if M <= SMALL_ROWS_MAX:
        return "small-rows"
    if M * min(N, K) <= FEW_ROWS_MH and N % 64 == 0:
        return "few-rows"
    if N % 128 == 0 and M <= GEMM_BF16_MAX:
        return "gemm_bf16"
    return "p8"


SMALL_ROWS_MAX, FEW_ROWS_MH, GEMM_BF16_MAX = 64, 640 * 1024, 1536
FUSED_HIDDEN = (768, 1024, 256)                       # run_encoder's fused add-LayerNorm chain (M <= 64, I % 16 == 0)


def thresholds_in_source():
    """The three constants as embed_gemm.hip states them inside launch_gemm_bias, and run_encoder's fused set."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cqs_amd", "csrc")
    src = open(os.path.join(here, "embed_gemm.hip")).read()
    body = src[src.index("hipError_t launch_gemm_bias("):]
    body = body[:body.index("\n}\n")]
    small = int(re.search(r"if \(M <= (\d+)u\) \{", body).group(1))
    few = re.search(r"CQS_HIP_GEMM_BIAS_FEWROWS_MH\"\); return f \? \(uint64_t\)atoll\(f\) : (\d+)ull \* (\d+)ull;", body)
    bf = int(re.search(r"N % 128u == 0 && M <= (\d+)u\) return launch_gemm_bf16", body).group(1))
    eng = open(os.path.join(here, "bert_run.hip")).read()
    fused = re.search(r"const bool fused = M <= (\d+)u && .*?\(H == (\d+)u \|\| H == (\d+)u \|\| H == (\d+)u\)", eng)
    return small, int(few.group(1)) * int(few.group(2)), bf, int(fused.group(1)), tuple(int(fused.group(i)) for i in (2, 3, 4))


def regimes_of(cfg, M):
    """The regime of each of a layer's four projections at M tokens: (qkv, attention output, FFN 1, FFN 2)."""
    H, I = cfg.hidden, cfg.intermediate
    return tuple(gemm_regime(M, N, K) for N, K in ((3 * H, H), (H, H), (I, H), (H, I)))


GEOMS = {                                              # name -> (hidden, heads, intermediate), seed of the weights
    "h256x4": ((256, 4, 512), 61), "h256x8": ((256, 8, 512), 62), "h384": ((384, 12, 768), 63),
    "h768": ((768, 12, 1536), 64), "h1024": ((1024, 16, 1024), 65),
    # not a model at hand: the one BERT geometry family whose projections 320 divides (1920, 640, 1280), so that a forced
    # pp:5 runs the 256 x 320 tiles under a bias and the GELU epilogue instead of falling back; its rows go through the
    # generic 4-byte-lane LayerNorm kernels
    "h640": ((640, 10, 1280), 66),
}
SMALLEST = "h256x4"

# up to 64 tokens: the search-time kernels (and run_encoder's fused add-LN chain where the hidden size has one); both
# sides of their 16-row tiles, two- and three-sequence batches
TINY = {"t1": [1], "t16": [16], "t17": [17], "t33": [33], "t49": [49], "t64": [64], "t20+30+14": [20, 30, 14], "t3+2": [3, 2],
        "t31+0+33": [31, 0, 33]}
_L2700 = [512, 300, 257, 129, 64, 33, 1, 511, 384, 255, 200, 54]
_L300 = [70, 1, 33, 64, 100, 0, 32]                      # (an empty sequence)
# geometry -> batch -> (lengths, the regime all four projections of a layer are meant to reach).  Ragged, partly filled
# 128- and 256-row tiles; test_the_batch_table_reaches_the_regimes_it_names holds the names to gemm_regime.
BATCHES = {
    "h256x4": {"300": (_L300, "few-rows"), "2700": (_L2700, "p8")},                 # few-rows holds to 2560 tokens at 256
    "h256x8": {"300": (_L300, "few-rows"), "2700": (_L2700, "p8")},
    "h384": {"500": ([129, 64, 33, 1, 200, 0, 73], "few-rows"), "1800": ([512, 300, 257, 129, 64, 33, 1, 384, 120], "p8")},
    "h768": {"400": ([70, 1, 33, 64, 100, 0, 132], "few-rows"), "1000": ([300, 257, 129, 64, 33, 1, 200, 16], "gemm_bf16"),
             "1700": ([512, 300, 257, 129, 64, 33, 1, 384, 20], "p8")},
    "h1024": {"300": (_L300, "few-rows"), "700": ([257, 129, 64, 33, 1, 200, 16], "gemm_bf16"),
              "1600": ([512, 300, 257, 129, 64, 33, 1, 284, 20], "p8")},
    "h640": {"500": ([129, 64, 33, 1, 200, 0, 73], "few-rows"), "1200": ([300, 257, 129, 64, 33, 1, 200, 216], "gemm_bf16"),
             "1700": ([512, 300, 257, 129, 64, 33, 1, 384, 20], "p8")},
}
TILES = ("small", "pp:3", "pp:4", "pp:5")              # CQS_HIP_GEMM_TILE under the gemm_bf16 batches (a width that does not divide N falls back)


def reordered(lens):
    """The same multiset in another order: every seq_start falls at another offset."""
    return lens[::-2] + lens[-2::-2]


def all_batches(geom):
    d = {k: v for k, v in TINY.items()}
    d.update({k: v[0] for k, v in BATCHES[geom].items()})
    return d


def batch_seed(geom, batch):
    return 7000 + 131 * sorted(GEOMS).index(geom) + 17 * sorted(all_batches(geom)).index(batch)


def emulate_rows(cfg, w, seqs):
    return [forward64(cfg, w, s, t, rnd=bf16)["hidden"] if len(s) else np.zeros((0, cfg.hidden)) for s, t in seqs]


SHORT = 33                                             # sequences below this many rows are held to the "hidden_short" line


def place_of(n):
    """A column's error is its mean over the rows: its rounding noise falls with the row count, and a bound taken over
    1-token sequences (where column = element) would be 3 - 5 x slack for a 300-token one.  Two lines per table key."""
    return "hidden_short" if n < SHORT else "hidden"


def emulated_worst(geom, wset, batches=None):
    """The emulation's worst `measures` distance to the fp32 oracle over a geometry's batches, per place: how EMULATED
    was made (python tests/bert_state.py prints the table)."""
    (h, nh, inter), seed = GEOMS[geom]
    cfg = config(h, nh, inter)
    w = weights(cfg, "none", seed, wset)
    worst = {}
    for name, lens in all_batches(geom).items():
        if batches is not None and name not in batches:
            continue
        seqs = seqs_for(cfg, lens, batch_seed(geom, name))
        for e, r in zip(emulate_rows(cfg, w, seqs), oracle_rows(cfg, w, seqs)):
            if len(r):
                w0 = worst.setdefault(place_of(len(r)), [0.0, 0.0, 0.0])
                worst[place_of(len(r))] = [max(a, b) for a, b in zip(w0, Q.measures(e, r))]
    return {k: tuple(v) for k, v in worst.items()}


def emulated_probe(case):
    cfg = probe_config(case)
    w = probe_weights(cfg)
    worst = [0.0, 0.0, 0.0]
    for lens in PROBE_BATCHES.values():
        seqs = probe_seqs(lens)
        m = Q.measures(np.concatenate(emulate_rows(cfg, w, seqs)), np.concatenate(oracle_rows(cfg, w, seqs)))
        worst = [max(a, b) for a, b in zip(worst, m)]
    return {"hidden": tuple(worst)}


# ---- bounds ---------------------------------------------------------------------------------------------------------------
# (1 - cos, element, column) of `query_state.measures`, per (geometry, weight set) and place: the EMULATION's worst
# distance to the fp32 oracle over every batch of all_batches(geometry) (emulated_worst, on a CPU - `python tests/bert_state.py` from anywhere prints the table; the probe lines:
# over the probe batches).  A bound is 3 x its line - the project's margin for f32 association and box-to-box differences.
# The device's measured worst is recorded in DESIGN.md 3.8d beside each line and feeds nothing.
EMULATED = {
    ('h1024', 'plain'): {'hidden': (1.141e-05, 0.0482, 0.0102), 'hidden_short': (1.195e-05, 0.0361, 0.0223)},
    ('h1024', 'peaked'): {'hidden': (5.689e-05, 0.0739, 0.0141), 'hidden_short': (4.461e-05, 0.0560, 0.0223)},
    ('h1024', 'shifted'): {'hidden': (1.136e-05, 0.0517, 0.0103), 'hidden_short': (1.255e-05, 0.0472, 0.0264)},
    ('h256x4', 'plain'): {'hidden': (1.299e-05, 0.0410, 0.0083), 'hidden_short': (1.627e-05, 0.0400, 0.0205)},
    ('h256x4', 'peaked'): {'hidden': (8.566e-05, 0.0574, 0.0134), 'hidden_short': (1.285e-04, 0.0665, 0.0288)},
    ('h256x4', 'shifted'): {'hidden': (1.449e-05, 0.0449, 0.0087), 'hidden_short': (1.621e-05, 0.0350, 0.0230)},
    ('h256x8', 'plain'): {'hidden': (1.452e-05, 0.0386, 0.0085), 'hidden_short': (1.562e-05, 0.0339, 0.0219)},
    ('h256x8', 'peaked'): {'hidden': (9.958e-05, 0.0621, 0.0140), 'hidden_short': (8.169e-05, 0.0630, 0.0237)},
    ('h256x8', 'shifted'): {'hidden': (1.456e-05, 0.0457, 0.0094), 'hidden_short': (1.610e-05, 0.0362, 0.0214)},
    ('h384', 'plain'): {'hidden': (1.251e-05, 0.0444, 0.0092), 'hidden_short': (1.521e-05, 0.0357, 0.0357)},
    ('h384', 'peaked'): {'hidden': (6.627e-05, 0.0585, 0.0135), 'hidden_short': (4.936e-05, 0.0551, 0.0357)},
    ('h384', 'shifted'): {'hidden': (1.348e-05, 0.0417, 0.0092), 'hidden_short': (1.663e-05, 0.0361, 0.0276)},
    ('h640', 'plain'): {'hidden': (1.304e-05, 0.0518, 0.0089), 'hidden_short': (1.478e-05, 0.0370, 0.0229)},
    ('h640', 'peaked'): {'hidden': (7.405e-05, 0.0588, 0.0156), 'hidden_short': (4.906e-05, 0.0490, 0.0262)},
    ('h640', 'shifted'): {'hidden': (1.216e-05, 0.0454, 0.0097), 'hidden_short': (1.423e-05, 0.0415, 0.0314)},
    ('h768', 'plain'): {'hidden': (1.146e-05, 0.0525, 0.0094), 'hidden_short': (1.523e-05, 0.0335, 0.0246)},
    ('h768', 'peaked'): {'hidden': (7.379e-05, 0.0687, 0.0149), 'hidden_short': (7.915e-05, 0.0802, 0.0259)},
    ('h768', 'shifted'): {'hidden': (1.176e-05, 0.0509, 0.0099), 'hidden_short': (1.693e-05, 0.0378, 0.0346)},
    # the probe's rows on the same measures (its own check is the band below), worst over PROBE_BATCHES
    ('probe', 'hd32'): {'hidden': (2.650e-06, 0.04818, 0.02970)},
    ('probe', 'hd64'): {'hidden': (3.383e-06, 0.12375, 0.03337)},
}
BOUNDS = {k: {place: tuple(3.0 * x for x in m) for place, m in v.items()} for k, v in EMULATED.items()}


def tally(name):
    import batch_state as BS
    return BS.Tally(name, bounds=BOUNDS, tag="BERTSTATE", report_env="CQS_BERT_STATE_REPORT")     # (=<file>: the figures as JSON lines)


def passes(key, got, ref, place="hidden"):
    m, b = Q.measures(got, ref), BOUNDS[key][place]
    return m[0] < b[0] and m[1] < b[1] and m[2] < b[2]


# ---- Part A: the mask probe -----------------------------------------------------------------------------------------------
# packed ragged batches with both sides of every edge the two attention kernels have: the 16-query tiles, the 8- and
# 16-wave passes (128 / 256 queries), the 128-key groups, the 256 / 512 max_len switch between the <*, 8, 2> and
# <*, 16 / 8, 4> instantiations, the first-generation kernel's 64-query blocks
PROBE_LENS = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512]
PROBE_BATCHES = {
    "lens": PROBE_LENS, "lens-reordered": reordered(PROBE_LENS),
    "to-256": [256, 1, 129, 255, 16, 128, 17, 65, 2, 127, 64, 33],        # max_len <= 256: the two-group instantiations
    "one": [300], "tiny": [1, 2, 15, 16, 17, 13],                           # 64 tokens: the fused add-LN small-rows chain
}
PROBE_HEADS = {"hd64": 4, "hd32": 8}                   # hidden 256
PROBE_SCALE = 256.0                                    # value projection: a tag is worth 256 x (one - zero) of the embedding LN


def probe_config(case):
    return R.BertConfig(vocab_size=64, hidden=256, layers=1, heads=PROBE_HEADS[case], intermediate=512, max_pos=512)


def probe_tags(cfg, b, n):
    """The dims that tag key p of sequence b, per head region r (hd = head dim):
      even r: position tag  r hd + p % hd                  (modulus hd: up to ceil(n / hd) keys share a tag)
      odd r:  position tag  r hd + p // hd                 (n <= 512: below 16 for hd 32, below 8 for hd 64)
              sequence tag  r hd + hd/2 + (5 b + r) % (hd/2)   (dims the position tags of an odd region never use)
    so a key is named by the pair (p % hd, p // hd) and its sequence by the sequence tag; neighbours in a batch differ
    by 5 in the sequence tag.  -> (position-tag dims [n, heads], sequence-tag dims [heads / 2])."""
    hd, nh = cfg.head_dim, cfg.heads
    p = np.arange(n)
    pos = np.stack([r * hd + (p % hd if r % 2 == 0 else p // hd) for r in range(nh)], 1)
    seq = np.array([r * hd + hd // 2 + (5 * b + r) % (hd // 2) for r in range(1, nh, 2)])
    return pos, seq


def probe_weights(cfg, seed=3):
    """Every value bf16-exact.  Position embedding p: 1 at its `heads` position-tag dims; word embedding 1 + b: 1 at
    sequence b's heads / 2 sequence-tag dims; token-type embeddings 0.  (The sequence has to come in through the token
    id: the engine numbers positions from 0 in every sequence, so with all-zero word embeddings the rows of two sequences
    at the same position would be the same row, and a neighbour's key that leaks in could not be told from an own one.)
    Every raw row then holds exactly 1.5 heads ones at distinct dims, so the embedding LayerNorm (gamma 1, beta 0) maps
    0 -> z and 1 -> o with the SAME z, o in every token.  Query weight and bias 0: every score is 0, attention is uniform
    over the allowed keys, p = exp2(0) = 1 exactly.  Key weights seeded (no influence).  Value = PROBE_SCALE x identity
    with bias - PROBE_SCALE z: an untagged dim is exactly 0, a tagged one A = PROBE_SCALE (o - z).  attention.output.dense
    = identity, zero bias; output.dense = 0, zero bias (the FFN branch adds exactly 0); LN gammas 1, betas 0."""
    w = R.seeded_weights(cfg, "none", seed=seed)
    H, nh = cfg.hidden, cfg.heads
    for k in w:
        if k.endswith("LayerNorm.weight"):
            w[k] = np.ones_like(w[k])
        elif k.endswith("LayerNorm.bias") or k.endswith(".bias"):
            w[k] = np.zeros_like(w[k])
    e = "embeddings."
    pe = np.zeros_like(w[e + "position_embeddings.weight"])
    pos, _ = probe_tags(cfg, 0, cfg.max_pos)
    pe[np.arange(cfg.max_pos)[:, None], pos] = 1.0
    we = np.zeros_like(w[e + "word_embeddings.weight"])
    for b in range(cfg.vocab_size - 1):
        we[1 + b, probe_tags(cfg, b, 1)[1]] = 1.0
    w[e + "position_embeddings.weight"], w[e + "word_embeddings.weight"] = pe, we
    w[e + "token_type_embeddings.weight"] = np.zeros_like(w[e + "token_type_embeddings.weight"])
    m = 1.5 * nh / H                                     # the embedding LN of a row with 1.5 heads ones among H dims
    z = float(np.ravel(bf16(-m / math.sqrt(m * (1.0 - m) + cfg.ln_eps)))[0])
    p = "encoder.layer.0."
    w[p + "attention.self.query.weight"] = np.zeros((H, H), np.float32)
    w[p + "attention.self.value.weight"] = (PROBE_SCALE * np.eye(H)).astype(np.float32)
    w[p + "attention.self.value.bias"] = np.full(H, np.float32(-PROBE_SCALE * z), np.float32)      # (exact: 2^8 x a bf16 value)
    w[p + "attention.output.dense.weight"] = np.eye(H, dtype=np.float32)
    w[p + "output.dense.weight"] = np.zeros((H, cfg.intermediate), np.float32)
    return w


def probe_seqs(lens):
    """Sequence b of a probe batch: every token carries id 1 + b (the sequence tag); token types 0."""
    return [(np.full(n, 1 + b, np.int32), np.zeros(n, np.int32)) for b, n in enumerate(lens)]


def probe_counts(cfg, b, n):
    """[n, H]: for every query of sequence b (all the same), how many of its n keys tag each dim."""
    pos, seq = probe_tags(cfg, b, n)
    c = np.zeros(cfg.hidden)
    np.add.at(c, pos.ravel(), 1.0)
    c[seq] += n
    return np.broadcast_to(c, (n, cfg.hidden))


# The band is derived, not measured.  With uniform attention over n keys the attention output of a dim is A c / n (c = the
# attended keys that tag it); the residual adds the token's own z / o (A = 256 (o - z): 1/256 of ONE key's level per
# attended key); LN1 and LN2 map the row affinely, f = (y - mu) / sigma, the same map for every dim of a row.  The LEVEL of
# a dim is read as f - (the row's smallest element): an odd region always holds untagged dims, they share one value, the
# row's floor, and the difference is (A c / n + own) / sigma.  Levels are counted in KEYS: one key's level = the level of
# the row's own sequence tag (which every one of the n keys carries) / n.  Against the oracle's level of the same dim:
#   one key too few   c -> c - 1 of n - 1 keys: the level falls by c - (c - 1) n / (n - 1) = (n - c) / (n - 1) keys; in an
#                     even region c <= ceil(n / hd) <= 16, so by at least 0.97 keys (the whole level for n <= hd) - for
#                     every query that does not share the key's own tag, i.e. at least 15 of the 16 queries of any tile;
#   one key too many  of the own sequence cannot happen (every key is attended); of the NEIGHBOUR: its sequence tag has
#                     c = 0 in the oracle and rises to n / (n + 1) >= 0.5 keys; its position tag rises by (n - c) / (n + 1)
#                     >= 0.96 keys;
#   a padded key      (zero value) scales every level by n / (n + 1) - and LN2 takes a common scale out again: the probe
#                     CANNOT see it (test_bert_state_sensitivity_cpu.py records that); it rests on the random-weight rows,
#                     where the key's score 0 competes with the real ones (peaked weights: 1 - cos 14 x the emulation);
#   LN renormalisation sigma moves with the sum of c^2: a changed key shifts every level of the row alike, by under 0.3 %
#                     at n >= 256 - 0.05 keys on a 16-key tag;
#   bf16 rounding     LN1's output and the final row are stored with relative error 2^-9 each, of f and of the floor; both
#                     are at most the row's mean level mu = 1.5 heads n / 256 keys (24 keys: 8 heads, n = 512) or c: an
#                     absolute 2 x 2 x 2^-9 x 24 = 0.19 keys at the worst, + 2^-9 c of the attention output's own store:
#                     under 0.22 keys for c <= 16; for the big tags (a sequence tag: c = n) under 3 x 2^-9 = 0.6 %.
# So a correct device keeps every level within max(0.22 keys, 0.6 %) of the oracle's, and one key moves a level of an even
# region by at least 0.96 - 0.05 - 0.22 = 0.69 keys.  The band sits between: a level may differ from the oracle's by
# PROBE_KEYS of a key or PROBE_REL of itself, whichever is larger (as a ratio band: 1 +- max(PROBE_REL, PROBE_KEYS / level
# in keys); the relative arm takes over above 20 keys, which no even-region tag reaches).
PROBE_KEYS = 0.4
PROBE_REL = 0.02


def probe_levels(cfg, rows, lens):
    """Packed final hidden rows [M, H] -> per sequence (levels [n, H], one key's level [n, 1])."""
    out = []
    for b, r in enumerate(split_rows(np.asarray(rows, np.float64), lens)):
        lv = r - r.min(-1, keepdims=True) if len(r) else r
        out.append((lv, (lv[:, probe_tags(cfg, b, len(r))[1][0]] / max(len(r), 1))[:, None]))
    return out


def probe_violations(cfg, got, ref, lens):
    """got / ref: packed final hidden rows [M, H].  -> list of (sequence, position, head region, dim, level got, level
    ref) in keys, empty if the band accepts.  A dim names a key (probe_tags)."""
    bad = []
    for b, ((lg, _), (lr, key)) in enumerate(zip(probe_levels(cfg, got, lens), probe_levels(cfg, ref, lens))):
        if len(lr) == 0:
            continue
        wrong = ~(np.abs(lg - lr) <= np.maximum(PROBE_KEYS * key, PROBE_REL * lr))
        for p, d in np.argwhere(wrong)[:6]:
            bad.append((b, int(p), int(d) // cfg.head_dim, int(d), float(lg[p, d] / key[p, 0]), float(lr[p, d] / key[p, 0])))
    return bad


def probe_worst(cfg, got, ref, lens):
    """The largest |level difference| in keys over the dims the absolute arm holds, and the largest relative one over
    the others: what a run prints beside the band."""
    wk = wr = 0.0
    for (lg, _), (lr, key) in zip(probe_levels(cfg, got, lens), probe_levels(cfg, ref, lens)):
        if len(lr):
            small = PROBE_KEYS * key >= PROBE_REL * lr
            wk = max(wk, float(np.where(small, np.abs(lg - lr) / key, 0.0).max()))
            wr = max(wr, float(np.where(~small, np.abs(lg - lr) / np.where(small, 1.0, lr), 0.0).max()))
    return wk, wr


# ---- the engine side ------------------------------------------------------------------------------------------------------
def engine(cfg, head, w):
    from cqs_amd import _lib
    from cqs_amd.splade import HipBertEngine, bert_config
    kind = {"mlm": _lib.BERT_HEAD_MLM, "classifier": _lib.BERT_HEAD_CLASSIFIER, "none": _lib.BERT_HEAD_NONE}[head]
    eng = HipBertEngine(bert_config(kind, vocab_size=cfg.vocab_size, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                                    intermediate=cfg.intermediate, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab,
                                    num_labels=cfg.num_labels, ln_eps=cfg.ln_eps))
    eng.set_weights(w)
    return eng


ENV = {"qsplit": "CQS_HIP_BERT_ATTN_QSPLIT", "resident": "CQS_HIP_BERT_ATTN_RESIDENT", "small_rows": "CQS_HIP_GEMM_SMALL_ROWS",
       "tile": "CQS_HIP_GEMM_TILE"}                    # all read per call


@contextlib.contextmanager
def form(**kw):
    """Run the engines in one kernel form: the per-call environment switches; the environment is put back on the way out."""
    saved = {v: os.environ.get(v) for v in ENV.values()}
    try:
        for k, v in ENV.items():
            if kw.get(k) is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = str(kw[k])
        yield
    finally:
        for v, old in saved.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old


# ---- the planted errors (test_bert_state_sensitivity_cpu.py) --------------------------------------------------------------
def encoder_plants(cfg, w, layer, T, neighbour_qkv):
    """name -> (class, plant callback for forward64) for a sequence of T tokens.  The attention errors are planted in
    EVERY layer and hold for every query (the attention kernel is one piece of code, run by every layer); the others in
    `layer` alone.  neighbour_qkv(l, row) = a qkv row of the sequence packed behind (row 0: what a kernel that reads one
    key past a sequence's end fetches; row -1: its last)."""
    H = cfg.hidden
    p = f"encoder.layer.{layer}."

    def at(stage, fn):
        return lambda s, l, t, rec: fn(np.array(t, np.float64), rec) if (s == stage and l == layer) else None

    def attn(edit, keys=None):
        def plant(s, l, t, rec):
            if s != "attn":
                return None
            k = None if keys is None else np.asarray(keys(l), np.float64).reshape(1, -1)
            allow = np.zeros((T, T + (0 if k is None else 1)), bool)
            allow[:, :T] = True
            allow[:, edit[0]] = edit[1]
            return attention64(cfg, rec[("qkv", l)], keys=k, allow=allow)
        return plant

    def bias_slice(t, rec):
        b = w[p + "attention.output.dense.bias"].astype(np.float64)
        t[:, 32:48] += b[48:64] - b[32:48]
        return t

    def no_gelu_tile(t, rec):
        t[:, 64:96] = lin64(w, p + "intermediate.dense", rec[("ln1", layer)])[:, 64:96]
        return t

    def ln1(x=None, g="attention.output", **kw):
        def redo(t, rec):
            res = layer_input(rec, layer) if x is None else x(layer_input(rec, layer))
            return ln64(res + rec[("attn_proj", layer)], w[p + g + ".LayerNorm.weight"], w[p + g + ".LayerNorm.bias"], cfg.ln_eps, **kw)
        return at("ln1", redo)

    def emb_ln(s, l, t, rec):
        if s != "emb":
            return None
        return ln64(rec[("emb_raw", -1)], w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], cfg.ln_eps, no_mean_in_variance=True)

    def ln2_var(t, rec):
        return ln64(rec[("ln1", layer)] + rec[("ffn2", layer)], w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], cfg.ln_eps,
                    no_mean_in_variance=True)

    def shifted_tile(x):
        x = x.copy()
        x[64:128] = x[0:len(x[64:128])]
        return x

    errs = {
        "the last key of the sequence masked": ("attention", attn((T - 1, False))),
        "the first key masked": ("attention", attn((0, False))),
        "the key at the 128-group edge masked": ("attention", attn((128, False))),
        "one key of the next packed sequence attended: its first row": ("attention", attn((T, True), lambda l: neighbour_qkv(l, 0))),
        "one key of the next packed sequence attended: its last row": ("attention", attn((T, True), lambda l: neighbour_qkv(l, -1))),
        "one padded key beyond seq_len attended, with a zero value": ("attention", attn((T, True), lambda l: np.zeros(3 * H))),
        "a 16-column slice of the attention output bias taken from the neighbouring slice": ("gemm", at("attn_proj", bias_slice)),
        "GELU left out for one 32-column tile": ("gemm", at("ffn1", no_gelu_tile)),
        "one 64-row tile's residual taken from the previous tile": ("gemm", ln1(x=shifted_tile)),
        "the embedding LayerNorm's variance without the mean subtracted": ("layernorm", emb_ln),
        "the attention LayerNorm's variance without the mean subtracted": ("layernorm", ln1(no_mean_in_variance=True)),
        "the output LayerNorm's variance without the mean subtracted": ("layernorm", at("ln2", ln2_var)),
        "gamma and beta of the other LayerNorm of the layer": ("layernorm", ln1(g="output")),
    }
    if T <= 129:
        del errs["the key at the 128-group edge masked"], errs["one 64-row tile's residual taken from the previous tile"]
    return errs


def head_plants(cfg, w, b):
    """name -> (head, plant callback for pool64 / splade64) around sequence b of a packed batch (b + 1 exists)."""
    V = cfg.vocab_size

    def span(stage, d_lo, d_hi):
        return lambda s, i, v: (v[0] + d_lo, v[1] + d_hi) if (s == stage and i == b) else None

    def leak(s, i, logits):
        if s != "logits":
            return None
        logits = logits.copy()
        logits[:, V - 1] = logits[:, V]                 # column n_valid lands in the last valid column's slot
        return logits

    def mlm_ln(s, i, t):
        if s != "mlm_ln":
            return None
        return ln64(t, w["cls.predictions.transform.LayerNorm.weight"], w["cls.predictions.transform.LayerNorm.bias"], cfg.ln_eps,
                    no_mean_in_variance=True)

    return {
        "the ROWMAX without the last row of a sequence": ("splade", span("rowmax_span", 0, -1)),
        "the ROWMAX with the first row of the next sequence": ("splade", span("rowmax_span", 0, 1)),
        "a column >= n_valid leaking into the last valid column": ("splade", leak),
        "the MLM transform's LayerNorm variance without the mean subtracted": ("splade", mlm_ln),
        "a mean pool over one row too many": ("mean", span("pool_span", 0, 1)),
        "the cls pool from row start + 1": ("cls", span("pool_span", 1, 0)),
    }


def live_measures(got, ref, lens):
    """`measures` over the rows of the non-empty sequences (an all-zero row has no cosine)."""
    live = np.asarray(lens) > 0
    return Q.measures(np.asarray(got)[live], np.asarray(ref)[live])


def splade_bound(cfg, w, rows, lens):
    """The SPLADE head's bound by the rule of EMULATED, for the head alone: 3 x the distance of the head with its two
    bf16 stores to the head without them, on the same rows.  -> (bound, the reference WITH the stores)."""
    emu = splade64(cfg, w, rows, lens, rnd=bf16)
    return tuple(3.0 * x for x in live_measures(emu, splade64(cfg, w, rows, lens), lens)), emu


def rerank_bound(cfg, w, rows, lens):
    """The same for the reranker head (one bf16 store: the pooled vector): 3 x the largest |logit| distance."""
    emu = rerank64(cfg, w, rows, lens, rnd=bf16)
    return 3.0 * float(np.abs(emu - rerank64(cfg, w, rows, lens)).max()), emu


def pool_bound(rows, lens, mode):
    """|device - float64| allowed per element of `embed`, [B, H].  mean: the kernel adds a column's T rows in f32 in
    token order and divides: |error| <= (T - 1) u sum|x_t| for the sum (u = 2^-24, each of the T - 1 additions rounds a
    partial sum that is at most sum|x_t|), / T, + u |mean| for the division -> T u mean_t|x_t[d]|; the constant 2 covers
    the second-order terms and the float32 the result is returned in.  cls: a bf16 row widened - exact."""
    out = np.zeros((len(lens), np.asarray(rows).shape[1]))
    if mode == "mean":
        for b, r in enumerate(split_rows(np.asarray(rows, np.float64), lens)):
            if len(r):
                out[b] = 2.0 * len(r) * 2.0 ** -24 * np.abs(r).mean(0)
    return out


if __name__ == "__main__":                              # prints the EMULATED table (a few seconds per line, on a CPU)
    for g in sorted(GEOMS):
        for ws in WSETS:
            print("    (%r, %r): {%s}," % (g, ws, ", ".join("%r: (%.3e, %.4f, %.4f)" % ((k,) + v) for k, v in sorted(emulated_worst(g, ws).items()))))
    for case in sorted(PROBE_HEADS):
        print("    (%r, %r): {%s}," % ("probe", case, ", ".join("%r: (%.3e, %.5f, %.5f)" % ((k,) + v) for k, v in emulated_probe(case).items())))
