"""The three BERT-family engines (bert_run.hip, bert_kernels.hip, the bias / GELU / ROWMAX epilogues of gemm_kernels.hip
and embed_gemm.hip, query_gemm.hip's small-rows forms) token row by token row, through the entry points that exist:
`HipBertEngine.hidden`, `embed`, `rerank_logits`, `splade_dense`.  tests/test_bert_gpu.py holds them to sequence-wide
cosines; here every row is compared with the fp32 oracle (oracle/bert_ref.py) within 3 x the distance of an EMULATED
correct device (tests/bert_state.py: the forward restated in float64 with every bf16 store), the kernel forms selected by
batch size and the per-call switches (CQS_HIP_BERT_ATTN_QSPLIT / _RESIDENT, CQS_HIP_GEMM_SMALL_ROWS, CQS_HIP_GEMM_TILE).

Part A, the mask probe: crafted one-layer weights under which a row spells out which keys the token attended.  Part B:
seeded weights, 2 layers, every GEMM regime `launch_gemm_bias` has for each geometry, byte identity under reordering.
Then the heads on their own, in float64 from the device's own rows.  tests/test_bert_state_sensitivity_cpu.py keeps band
and bounds honest on a CPU.  Every comparison prints its figures (pytest -s); DESIGN.md 3.8d holds the record."""
import numpy as np
import pytest

import bert_state as S

pytestmark = pytest.mark.gpu


def run_hidden(eng, seqs):
    return eng.hidden([s for s, _ in seqs], [t for _, t in seqs])


# ---- Part A: the mask probe -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_oracle():
    """(case, batch) -> (sequences, fp32 oracle rows packed [M, H]), computed once."""
    cache = {}

    def get(case, batch):
        if (case, batch) not in cache:
            cfg = S.probe_config(case)
            seqs = S.probe_seqs(S.PROBE_BATCHES[batch])
            cache[(case, batch)] = (seqs, np.concatenate(S.oracle_rows(cfg, S.probe_weights(cfg), seqs)))
        return cache[(case, batch)]
    return get


PROBE_FORMS = {                                        # name -> (switches, batches)
    "launcher's choice": ({}, ["lens", "lens-reordered", "to-256", "one", "tiny"]),
    "qsplit 1": (dict(qsplit=1), ["lens", "to-256", "one"]),
    "qsplit 2": (dict(qsplit=2), ["lens", "to-256", "one"]),
    "qsplit 4": (dict(qsplit=4), ["lens", "to-256", "one"]),
    "first-generation kernel": (dict(resident=0), ["lens", "lens-reordered", "to-256", "one", "tiny"]),
    "no small-rows chain": (dict(small_rows=0), ["tiny"]),
    "no small-rows chain, first-generation kernel": (dict(small_rows=0, resident=0), ["tiny"]),
}


@pytest.mark.parametrize("case", sorted(S.PROBE_HEADS))
def test_probe_every_token_attends_exactly_its_keys(hip, probe_oracle, case):
    cfg = S.probe_config(case)
    eng = S.engine(cfg, "none", S.probe_weights(cfg))
    tally = S.tally("probe " + case)
    for name, (kw, batches) in PROBE_FORMS.items():
        for batch in batches:
            seqs, ref = probe_oracle(case, batch)
            lens = S.PROBE_BATCHES[batch]
            with S.form(**kw):
                got = run_hidden(eng, seqs)
            # (the wrapper sizes the output itself, [sum(lens), hidden]: the shape says nothing about the device.)  Live rows
            # only, in packing order: a row's highest tag in the first odd region names its sequence
            for b, (lv, _) in enumerate(S.probe_levels(cfg, got, lens)):
                hd = cfg.head_dim
                own = S.probe_tags(cfg, b, 1)[1][0]
                if not np.all(hd + hd // 2 + lv[:, hd + hd // 2: 2 * hd].argmax(-1) == own):
                    tally.fail(("row order", case, name, batch, "sequence", b))
            bad = S.probe_violations(cfg, got, ref, lens)
            wk, wr = S.probe_worst(cfg, got, ref, lens)
            print("BERTSTATE-PROBE %s %s %s worst level error %.3f keys (band %.2f), %.4f relative (band %.2f)" % (case, name, batch, wk, S.PROBE_KEYS, wr, S.PROBE_REL))
            if bad:
                tally.fail(("probe band", case, name, batch, "(sequence, position, head, dim, level got, level ref in keys)", bad[:4]))
            tally.add("hidden", ("probe", case), got, ref, (name, batch))
    eng.close()
    tally.finish()


# ---- Part B: token rows against the fp32 oracle on seeded weights, every GEMM regime -------------------------------------
@pytest.fixture(scope="module")
def rows_oracle():
    """(geometry, weight set, batch) -> (sequences, [oracle rows [n, H] per sequence]), computed once, left unchanged."""
    cache = {}

    def get(geom, wset, batch):
        key = (geom, wset, batch)
        if key not in cache:
            (h, nh, inter), seed = S.GEOMS[geom]
            cfg = S.config(h, nh, inter)
            seqs = S.seqs_for(cfg, S.all_batches(geom)[batch], S.batch_seed(geom, batch))
            cache[key] = (seqs, S.oracle_rows(cfg, S.weights(cfg, "none", seed, wset), seqs))
        return cache[key]
    return get


def rows_against_oracle(eng, case, tally, key, what):
    """One run of a batch in the current form: every sequence's rows against the oracle's (the wrapper sizes the output
    itself, so its shape is no check of the device; a row that is not where the packing puts it fails its bounds).
    -> the rows per sequence (bytes are compared across orders)."""
    seqs, ref = case
    got = run_hidden(eng, seqs)
    assert np.all(np.isfinite(got)), what
    per = S.split_rows(got, [len(s) for s, _ in seqs])
    for b, (g, r) in enumerate(zip(per, ref)):
        if len(r):
            tally.add(S.place_of(len(r)), key, g, r, what + (b, len(r)))
    return per


def order_index(n):
    return list(range(n))[::-2] + list(range(n))[-2::-2]                  # bert_state.reordered, as indices


@pytest.mark.parametrize("wset", S.WSETS)
@pytest.mark.parametrize("geom", sorted(S.GEOMS))
def test_rows_match_the_oracle_in_every_gemm_regime(hip, rows_oracle, geom, wset):
    """Every batch of bert_state.all_batches(geometry) - up to 64 tokens (the search-time kernels; the fused add-LN chain
    for 256 / 768 / 1024) also with CQS_HIP_GEMM_SMALL_ROWS=0, the launch_gemm_bf16 batches also under every
    CQS_HIP_GEMM_TILE - and again with the sequences in another order: the same multiset, M, max_len and switches must
    give every sequence the same BYTES in every row."""
    (h, nh, inter), seed = S.GEOMS[geom]
    cfg = S.config(h, nh, inter)
    eng = S.engine(cfg, "none", S.weights(cfg, "none", seed, wset))
    tally = S.tally("regimes %s %s" % (geom, wset))
    key = (geom, wset)
    for batch, lens in S.all_batches(geom).items():
        case = rows_oracle(geom, wset, batch)
        regime = S.BATCHES[geom][batch][1] if batch in S.BATCHES[geom] else "small-rows"
        forms = {"default": {}}
        if batch in S.TINY:
            forms["small-rows off"] = dict(small_rows=0)
        if regime == "gemm_bf16":
            forms.update({"tile " + t: dict(tile=t) for t in S.TILES})
        for name, kw in forms.items():
            with S.form(**kw):
                per = rows_against_oracle(eng, case, tally, key, (geom, wset, batch, regime, name))
                if len(lens) > 1:
                    idx = order_index(len(lens))
                    again = run_hidden(eng, [case[0][i] for i in idx])
                    for j, rows in zip(idx, S.split_rows(again, [lens[i] for i in idx])):
                        if rows.tobytes() != per[j].tobytes():
                            tally.fail(("bytes differ in another order", geom, wset, batch, name, "sequence", j, float(np.abs(rows - per[j]).max())))
    eng.close()
    tally.finish()


# ---- the heads on their own, from the device's own rows -------------------------------------------------------------------
POOL_LENS = [512, 1, 63, 2, 64, 0, 65]                 # (1 token behind 512: one row too many would add a foreign row to a mean of one)


@pytest.mark.parametrize("geom", ["h256x4", "h384"])  # 8- and 4-byte lanes of the row kernels
def test_pooling_is_the_mean_or_first_row_of_the_device_rows(hip, geom):
    (h, nh, inter), seed = S.GEOMS[geom]
    cfg = S.config(h, nh, inter)
    eng = S.engine(cfg, "none", S.weights(cfg, "none", seed))
    seqs = S.seqs_for(cfg, POOL_LENS, 3000)
    rows = run_hidden(eng, seqs)
    for mode in ("mean", "cls"):
        got = eng.embed([s for s, _ in seqs], [t for _, t in seqs], pooling=mode)
        err, lim = np.abs(got - S.pool64(rows, POOL_LENS, mode)), S.pool_bound(rows, POOL_LENS, mode)
        for b, n in enumerate(POOL_LENS):
            print("BERTSTATE-POOL %s %s %d tokens: largest error %.3e, bound there %.3e" % (geom, mode, n, err[b].max(), lim[b][err[b].argmax()]))
        assert np.all(got[POOL_LENS.index(0)] == 0)
        assert np.all(err <= lim), (geom, mode, np.argwhere(err > lim)[:4])
    eng.close()


@pytest.mark.parametrize("num_labels", [1, 3])
def test_reranker_head_from_the_device_rows(hip, num_labels):
    """BertPooler (the first row of every sequence through `row_index`, dense + tanh, stored bf16) + classifier, in
    float64 from `hidden`'s rows of the same batch; 1, 16, 17 and 40 sequences (both sides of the 16-row tile)."""
    cfg = S.config(384, 12, 768, num_labels=num_labels)
    w = S.weights(cfg, "classifier", 71)
    eng = S.engine(cfg, "classifier", w)
    for nseq in (1, 16, 17, 40):
        lens = [int(x) for x in np.random.default_rng(nseq).integers(1, 40, size=nseq)]
        seqs = S.seqs_for(cfg, lens, 3100 + nseq)
        rows = run_hidden(eng, seqs)
        got = eng.rerank_logits([s for s, _ in seqs], [t for _, t in seqs])
        bound, ref = S.rerank_bound(cfg, w, rows, lens)
        err = float(np.abs(got - ref).max())
        print("BERTSTATE-RERANK labels %d, %d sequences: largest |logit error| %.3e (bound %.3e)" % (num_labels, nseq, err, bound))
        assert got.shape == (nseq, num_labels) and err < bound, (num_labels, nseq, err, bound)
    eng.close()


# sequence boundaries at every offset inside the ROWMAX epilogue's 32-row runs and across the 64-, 128- and 256-row tile
# edges, three sequences inside one run, an empty one, a tail that ends in a partly filled last tile
SPLADE_BATCHES = {"edges": [1, 1, 1, 30, 2, 31, 33, 64, 1, 127, 129, 5, 0, 256, 3, 77], "tiny": [3, 1, 20, 0, 9],
                  "2700": [512, 300, 257, 129, 64, 33, 1, 511, 384, 255, 200, 54]}


@pytest.mark.parametrize("vocab", [130, 1000, 1536])  # under one 192-wide tile, padded, a whole number of tiles
def test_splade_head_from_the_device_rows(hip, vocab):
    cfg = S.config(256, 4, 512, layers=1, vocab=vocab)
    w = S.weights(cfg, "mlm", 72)
    eng = S.engine(cfg, "mlm", w)
    for batch, lens in SPLADE_BATCHES.items():
        if batch == "2700" and vocab != 1000:
            continue
        seqs = [(s, np.zeros_like(t)) for s, t in S.seqs_for(cfg, lens, 3200)]        # (the SPLADE entry point takes no token types)
        rows = run_hidden(eng, seqs)
        got = eng.splade_dense([s for s, _ in seqs])
        bound, ref = S.splade_bound(cfg, w, rows, lens)
        m = S.live_measures(got, ref, lens)
        print("BERTSTATE-SPLADE vocab %d %s: 1-cos=%.3e elem=%.4f col=%.4f (bounds %.3e %.4f %.4f)" % (vocab, batch, *m, *bound))
        assert got.shape == (len(lens), vocab) and all(np.all(got[b] == 0) for b, n in enumerate(lens) if n == 0)
        assert all(x < y for x, y in zip(m, bound)), (vocab, batch, m, bound)
    eng.close()
