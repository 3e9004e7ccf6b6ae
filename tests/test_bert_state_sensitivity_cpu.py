"""Keeps the per-token check of the BERT engines (tests/bert_state.py, tests/test_bert_state_gpu.py) honest, on a CPU - the
twin of test_batch_state_sensitivity_cpu.py.  The float64 restatement with rnd = identity is the fp32 oracle; with rnd =
bf16 it is a correct device, and the committed table EMULATED is its distance to the oracle; the batch table reaches the
GEMM regimes it names; the band and the bounds accept the emulation and reject every planted error - each planted
through the restatement's `plant` hook into the reference side only.  INSTRUMENT lists which instrument catches which."""
import numpy as np
import pytest

import bert_state as S
import query_state as Q
from oracle import bert_ref as R

(_H, _NH, _I), _SEED = S.GEOMS[S.SMALLEST]
PLANT_T, NEIGHBOUR_T, PLANT_LAYER = 300, 129, 0


def test_the_restatement_with_no_rounding_is_the_oracle():
    cfg = S.config(_H, _NH, _I, vocab=300, num_labels=3)
    lens = [70, 1, 33, 129]
    for head in ("mlm", "classifier", "none"):
        w = S.weights(cfg, head, _SEED)
        seqs = S.seqs_for(cfg, lens, 11)
        ref = S.oracle_rows(cfg, w, seqs)
        rows = [S.forward64(cfg, w, s, t)["hidden"] for s, t in seqs]
        for a, r in zip(rows, ref):
            assert np.abs(a - r).max() < 2e-5, (head, len(r), np.abs(a - r).max())          # fp32 noise on O(1) values
        ids, mask, tt = (np.zeros((len(lens), max(lens)), np.int64) for _ in range(3))
        for b, (s, t) in enumerate(seqs):
            ids[b, :len(s)], mask[b, :len(s)], tt[b, :len(s)] = s, 1, t
        packed = np.concatenate(ref)
        if head == "mlm":
            hid = R.encode(cfg, w, ids, mask, tt)
            want = np.stack([R.activate(R.splade_pool(R.mlm_logits(cfg, w, hid)[b], n)) for b, n in enumerate(lens)])
            assert np.abs(S.splade64(cfg, w, packed, lens) - want).max() < 2e-5
        elif head == "classifier":
            want = R.classifier_logits(cfg, w, R.encode(cfg, w, ids, mask, tt))
            assert np.abs(S.rerank64(cfg, w, packed, lens) - want).max() < 2e-5
        else:
            for mode in ("mean", "cls"):
                assert np.abs(S.pool64(packed, lens, mode) - R.pooled_embedding(cfg, w, ids, mask, tt, mode)).max() < 2e-5


def test_the_batch_table_reaches_the_regimes_it_names():
    """`launch_gemm_bias`'s thresholds as embed_gemm.hip states them, and the batch of every regime on the right side."""
    assert S.thresholds_in_source() == (S.SMALL_ROWS_MAX, S.FEW_ROWS_MH, S.GEMM_BF16_MAX, S.SMALL_ROWS_MAX, S.FUSED_HIDDEN)
    for geom, ((h, nh, inter), _) in S.GEOMS.items():
        cfg = S.config(h, nh, inter)
        assert inter % 16 == 0
        for name, lens in S.TINY.items():
            assert set(S.regimes_of(cfg, sum(lens))) == {"small-rows"}, (geom, name)
        reached = set()
        for name, (lens, regime) in S.BATCHES[geom].items():
            assert set(S.regimes_of(cfg, sum(lens))) == {regime}, (geom, name, S.regimes_of(cfg, sum(lens)))
            assert sum(lens) % 128 and sum(lens) % 256 and len(set(lens)) > 4, (geom, name)      # ragged, a partly filled last tile
            assert sorted(S.reordered(lens)) == sorted(lens) and S.reordered(lens) != lens
            reached.add(regime)
        # every regime the geometry has: few-rows ends at 640 Ki / hidden tokens - above 1536 for 256 and 384, where
        # launch_gemm_bf16 is therefore never taken from launch_gemm_bias
        has_bf16 = S.FEW_ROWS_MH // h < S.GEMM_BF16_MAX
        want = {"few-rows", "gemm_bf16", "p8"} if has_bf16 else {"few-rows", "p8"}
        assert reached == want, (geom, reached)
        assert any(0 in lens for lens, _ in S.BATCHES[geom].values())                             # one empty sequence
    assert S.config(384, 12, 768).hidden not in S.FUSED_HIDDEN                                     # small-rows, unfused


@pytest.mark.parametrize("wset", S.WSETS)
def test_the_committed_table_is_the_emulation(wset):
    """Recomputed for the smallest geometry (every batch the GPU test runs); the other lines are made the same way
    (python tests/bert_state.py).  A correct bf16 device passes its bounds by construction - with a margin of 3."""
    got = S.emulated_worst(S.SMALLEST, wset)
    tab = S.EMULATED[(S.SMALLEST, wset)]
    assert set(got) == set(tab) == {"hidden", "hidden_short"}
    for place, m in got.items():
        print("EMULATED", S.SMALLEST, wset, place, "1-cos=%.3e elem=%.4f col=%.4f" % m)
        assert abs(m[0] / tab[place][0] - 1.0) < 1e-3 and abs(m[1] - tab[place][1]) < 6e-5 and abs(m[2] - tab[place][2]) < 6e-5, (place, m, tab[place])
    assert set(S.EMULATED) == {(g, w) for g in S.GEOMS for w in S.WSETS} | {("probe", c) for c in S.PROBE_HEADS}
    assert all(S.BOUNDS[k][p] == tuple(3.0 * x for x in v) for k, d in S.EMULATED.items() for p, v in d.items())


@pytest.mark.parametrize("case", sorted(S.PROBE_HEADS))
def test_the_probe_band_accepts_a_correct_device(case):
    cfg = S.probe_config(case)
    w = S.probe_weights(cfg)
    assert all(np.array_equal(v, R.bf16_round(v)) for v in w.values())                             # every value bf16-exact
    worst = [0.0, 0.0, 0.0]
    for name, lens in S.PROBE_BATCHES.items():
        seqs = S.probe_seqs(lens)
        ref, emu = np.concatenate(S.oracle_rows(cfg, w, seqs)), np.concatenate(S.emulate_rows(cfg, w, seqs))
        # the oracle's levels ARE the key counts (+ the token's own residual: n / 256 keys on its own tags)
        for b, (lv, key) in enumerate(S.probe_levels(cfg, ref, lens)):
            assert np.abs(lv / key - S.probe_counts(cfg, b, len(lv))).max() < len(lv) / 256.0 + 0.02, (case, name, b)
        assert S.probe_violations(cfg, emu, ref, lens) == [], (case, name)
        wk, wr = S.probe_worst(cfg, emu, ref, lens)
        print("PROBE", case, name, "emulated device: worst level error %.3f keys (band %.2f), %.4f relative (band %.2f)" % (wk, S.PROBE_KEYS, wr, S.PROBE_REL))
        assert wk < 0.22 and wr < 0.006                                                               # the derivation's own figures
        worst = [max(a, b) for a, b in zip(worst, Q.measures(emu, ref))]
    assert np.allclose(worst, S.EMULATED[("probe", case)]["hidden"], rtol=2e-3), worst


# ---- the planted errors ---------------------------------------------------------------------------------------------------
# Which instrument rejects which planted error (asserted below, both ways): "rows" = the random-weight bounds of the
# smallest geometry at 300 tokens (P = with plain weights, K = peaked, S = shifted), "probe" = the mask probe's band on
# hd 64 AND hd 32 at EVERY length planted (15, 300, 512), "head" = the head's own bound on the same geometry's rows.
INSTRUMENT = {
    "the last key of the sequence masked": ("attention", {"rows:PKS", "probe"}),
    "the first key masked": ("attention", {"rows:PKS", "probe"}),
    "the key at the 128-group edge masked": ("attention", {"rows:PKS", "probe"}),
    "one key of the next packed sequence attended: its first row": ("attention", {"rows:PKS", "probe"}),
    "one key of the next packed sequence attended: its last row": ("attention", {"rows:PKS", "probe"}),
    # a zero-value key scales the attention output; the probe's LN2 takes a common scale out again, and with plain weights
    # the key's weight among 300 is rounding noise (1.4 x the emulation on 1 - cos): peaked and shifted weights show it
    "one padded key beyond seq_len attended, with a zero value": ("attention", {"rows:KS"}),
    "a 16-column slice of the attention output bias taken from the neighbouring slice": ("gemm", {"rows:PKS"}),
    "GELU left out for one 32-column tile": ("gemm", {"rows:PKS"}),
    "one 64-row tile's residual taken from the previous tile": ("gemm", {"rows:PKS"}),      # (the probe's hd 32 sees it too)
    "gamma and beta of the other LayerNorm of the layer": ("layernorm", {"rows:PKS"}),
    # E[x^2] for the variance is wrong by mean^2.  Seeded weights give every LayerNorm input a mean of a few percent of its
    # deviation, the probe's LN2 takes a common scale out again: on plain and peaked weights the error is invisible - which
    # is why the "shifted" set exists (bert_state.weights): its rows have a mean, as a real checkpoint's do
    "the embedding LayerNorm's variance without the mean subtracted": ("layernorm", {"rows:S"}),
    "the attention LayerNorm's variance without the mean subtracted": ("layernorm", {"rows:S"}),
    "the output LayerNorm's variance without the mean subtracted": ("layernorm", {"rows:S"}),
    "the MLM transform's LayerNorm variance without the mean subtracted": ("layernorm", {"head"}),
    "the ROWMAX without the last row of a sequence": ("heads", {"head"}),
    "the ROWMAX with the first row of the next sequence": ("heads", {"head"}),
    "a column >= n_valid leaking into the last valid column": ("heads", {"head"}),
    "a mean pool over one row too many": ("heads", {"head"}),
    "the cls pool from row start + 1": ("heads", {"head"}),
}
PROBE_ONLY_CAP = 2                                     # attention errors that may rest on the probe alone


def _rows_reject():
    """-> {name: "rows:" + the letters of the weight sets whose bounds reject it, or None} on the smallest geometry."""
    cfg = S.config(_H, _NH, _I)
    hit = {}
    for wset, letter in (("plain", "P"), ("peaked", "K"), ("shifted", "S")):
        w = S.weights(cfg, "none", _SEED, wset)
        (s, t), (ns, nt) = S.seqs_for(cfg, [PLANT_T, NEIGHBOUR_T], 1000)
        clean, nb = S.forward64(cfg, w, s, t), S.forward64(cfg, w, ns, nt)
        emu = S.forward64(cfg, w, s, t, rnd=S.bf16)["hidden"]
        b = S.BOUNDS[(S.SMALLEST, wset)]["hidden"]
        print("PLANT rows %-7s %-85s 1-cos=%.3e elem=%.4f col=%.4f (bounds %.3e %.4f %.4f)" % (wset, "none: the emulated device", *Q.measures(emu, clean["hidden"]), *b))
        assert S.passes((S.SMALLEST, wset), emu, clean["hidden"])
        for name, (cls, pl) in S.encoder_plants(cfg, w, PLANT_LAYER, PLANT_T, lambda l, r: nb[("qkv", l)][r]).items():
            hid = S.forward64(cfg, w, s, t, plant=pl)["hidden"]
            print("PLANT rows %-7s %-85s 1-cos=%.3e elem=%.4f col=%.4f (bounds %.3e %.4f %.4f)" % (wset, name, *Q.measures(hid, clean["hidden"]), *b))
            hit[name] = hit.get(name, "") + ("" if S.passes((S.SMALLEST, wset), hid, clean["hidden"]) else letter)
    return {k: ("rows:" + v if v else None) for k, v in hit.items()}


PROBE_PLANT_T = (15, PLANT_T, 512)                     # 512: the worst case of the band's derivation (16 keys per tag at hd 32)


def _probe_reject():
    """-> {name: rejected on hd 64 AND on hd 32 at EVERY length of PROBE_PLANT_T at which the plant exists}."""
    hit = {}
    for case in sorted(S.PROBE_HEADS):
        cfg = S.probe_config(case)
        w = S.probe_weights(cfg)
        for T in PROBE_PLANT_T:
            (s, t), (ns, nt) = S.probe_seqs([T, NEIGHBOUR_T])
            clean, nb = S.forward64(cfg, w, s, t), S.forward64(cfg, w, ns, nt)
            for name, (cls, pl) in S.encoder_plants(cfg, w, 0, T, lambda l, r: nb[("qkv", l)][r]).items():
                bad = S.probe_violations(cfg, S.forward64(cfg, w, s, t, plant=pl)["hidden"], clean["hidden"], [T])
                print("PLANT probe %s T=%-3d %-85s violations %d, first (seq, pos, head, dim, level got, ref in keys) %s" % (case, T, name, len(bad), bad[:1]))
                hit[name] = hit.get(name, True) and bool(bad)
    return hit


def _head_reject():
    """The heads on the EMULATED rows of a packed batch of the smallest geometry (sequence 1 of [33, 64, 65, 20])."""
    cfg = S.config(_H, _NH, _I, vocab=1000)
    w = S.weights(cfg, "mlm", _SEED)
    lens = [33, 64, 65, 20]
    rows = np.concatenate(S.emulate_rows(cfg, w, S.seqs_for(cfg, lens, 2000)))
    bound, _ = S.splade_bound(cfg, w, rows, lens)
    clean = S.splade64(cfg, w, rows, lens)
    hit = {}
    for name, (head, pl) in S.head_plants(cfg, w, 1).items():
        if head == "splade":
            m = S.live_measures(S.splade64(cfg, w, rows, lens, plant=pl), clean, lens)
            print("PLANT head  %-85s 1-cos=%.3e elem=%.4f col=%.4f (bounds %.3e %.4f %.4f)" % (name, *m, *bound))
            hit[name] = not all(x < y for x, y in zip(m, bound))
        else:
            err = np.abs(S.pool64(rows, lens, head, plant=pl) - S.pool64(rows, lens, head))
            lim = S.pool_bound(rows, lens, head)
            print("PLANT head  %-85s largest error %.3e against its bound %.3e" % (name, err.max(), lim.flat[err.argmax()]))
            hit[name] = bool(np.any(err > lim))
    return hit


def test_every_planted_error_is_rejected_by_the_instrument_listed():
    rows, probe, head = _rows_reject(), _probe_reject(), _head_reject()
    got = {}
    for name in set(rows) | set(head):
        got[name] = {x for x in (rows.get(name), "probe" if probe.get(name) else None, "head" if head.get(name) else None) if x}
    assert got == {k: v for k, (_, v) in INSTRUMENT.items()}, {k: (got.get(k), v) for k, (_, v) in INSTRUMENT.items() if got.get(k) != v}
    escaped = [k for k, v in got.items() if not v]
    assert not escaped, escaped
    attention = [k for k, (c, _) in INSTRUMENT.items() if c == "attention"]
    assert len(attention) == 6 and sum(got[k] == {"probe"} for k in attention) <= PROBE_ONLY_CAP
    assert len(INSTRUMENT) >= 16
