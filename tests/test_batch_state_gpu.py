"""The batch chain (`run_layers` in cqs_amd/csrc/embedder_run.hip with embed_attention.hip, embed_gemm.hip, gemm_kernels.hip,
gemm_rowfuse.hip and embed_rows.hip) token by token, in every kernel form.  tests/test_embed_gpu.py holds it to the POOLED
sentence vector (a mean over T tokens divides a one-row error by T) and ties its fused forms only to the unfused chain;
here `HipEmbedEngine.run_hidden` - which runs `run_layers` and returns the f32 final-norm row of every token - is compared
row by row with the fp32 oracle (oracle/gemma3_ref.py), the forms selected through the switches the engine already has:
CQS_HIP_ATT_LAYOUT / CQS_HIP_ATT_KERNEL / CQS_HIP_GEMM_TILE (read per call) and the fuse_norm / fuse_qkv / geglu4 hooks.

Part A, the mask probe (tests/batch_state.py): crafted one-layer weights under which a row spells out which keys the token
attended - the mask, window, tile-edge and packed-sequence logic of every attention and QKV form, checked by a derived
ratio band that names token, head and key.  Part B: seeded random weights on narrow-window geometries, every row against
`query_state.measures` bounds (3 x the device's measured worst), and the head on its own.
tests/test_batch_state_sensitivity_cpu.py keeps band and bounds honest on a CPU."""
import numpy as np
import pytest

import batch_state as B
import query_state as Q
from oracle import gemma3_ref as G

pytestmark = pytest.mark.gpu

ATT_FORMS = {"per-head": dict(layout="per-head"), "shared-dma": dict(layout="shared", kernel="dma"), "shared-reg": dict(layout="shared", kernel="reg")}


# ---- Part A: the mask probe ---------------------------------------------------------------------------------------------
PROBE_BATCHES = {"lens": B.PROBE_LENS, "lens-reordered": B.PROBE_LENS_2, "subset": B.PROBE_SUBSET, "one": B.PROBE_ONE}


@pytest.fixture(scope="module")
def probe_oracle():
    """(layout, window case, batch) -> (ids, mask, fp32 oracle hidden rows [B, L, H]), computed once."""
    cache = {}

    def get(layout, wcase, batch):
        key = (layout, wcase, batch)
        if key not in cache:
            cfg = B.probe_config(layout, wcase)
            ids, mask = B.probe_batch(PROBE_BATCHES[batch])
            cache[key] = (ids, mask, G.forward(cfg, B.probe_weights(cfg), ids, mask, return_hidden=True))
        return cache[key]
    return get


def probe_forms(layout):
    """name -> (form, batches).  The planner's own choice runs the whole ragged batch in both orders; forced forms run the
    subset; everything also runs the one-sequence batch.  2:2 has one q head per kv head: att_plan gives it the per-head
    workgroups only, and no fused QKV epilogue (that needs the DMA kernel)."""
    heads, kv = B.HEAD_LAYOUTS[layout]
    forms = {"default": ({}, ["lens", "lens-reordered", "one"]), "per-head": (ATT_FORMS["per-head"], ["subset", "one"]),
             "per-head, 256-row tiles": (dict(layout="per-head", tile="pp:4"), ["subset"])}
    if heads // kv > 1:
        dma = ATT_FORMS["shared-dma"]
        forms.update({
            "shared-dma": (dma, ["subset", "one"]),
            "shared-reg": (ATT_FORMS["shared-reg"], ["subset", "one"]),
            "shared-dma, kv_prep": (dict(dma, fuse_qkv=False), ["subset", "one"]),
            "shared-dma, kv_prep under pp:4": (dict(dma, tile="pp:4", fuse_qkv=False), ["subset"]),
            "shared-dma, fused QKV pp:4": (dict(dma, tile="pp:4"), ["subset", "one"]),
            "shared-reg under pp:4": (dict(ATT_FORMS["shared-reg"], tile="pp:4"), ["subset"]),
        })
        if heads == 3 * kv:
            forms["shared-dma, fused QKV pp:5"] = (dict(dma, tile="pp:5"), ["subset", "one"])
            forms["shared-dma, kv_prep under pp:5"] = (dict(dma, tile="pp:5", fuse_qkv=False), ["subset"])
    return forms


@pytest.mark.parametrize("wcase", sorted(B.WINDOWS))
@pytest.mark.parametrize("layout", sorted(B.HEAD_LAYOUTS))
def test_probe_every_token_attends_exactly_its_keys(hip, probe_oracle, layout, wcase):
    cfg = B.probe_config(layout, wcase)
    eng = B.engine(cfg, B.probe_weights(cfg))
    tally = B.Tally("probe %s %s" % (layout, wcase))
    for name, (kw, batches) in probe_forms(layout).items():
        for batch in batches:
            ids, mask, ref = probe_oracle(layout, wcase, batch)
            with B.form(eng, **kw):
                got = eng.run_hidden(ids, mask)
            bad = B.probe_violations(got, ref, ids, mask, cfg.heads)
            if bad:
                tally.fail(("probe band", layout, wcase, name, batch, "(sequence, position, head, dim, got, ref)", bad[:4]))
            live = mask.astype(bool)
            tally.add("hidden", ("probe", wcase), got[live], ref[live], (layout, name, batch))
    eng.close()
    tally.finish()


# ---- Part B: token rows against the fp32 oracle on random weights -------------------------------------------------------
@pytest.fixture(scope="module")
def rows_oracle():
    """(geometry, weight set, depth, batch) -> (cut config, weights, per-sequence (ids, mask), padded ids, padded mask,
    [oracle hidden rows [T, H] per sequence]), computed once and left unchanged."""
    cache = {}

    def get(geom, wset, depth, batch):
        key = (geom, wset, depth, batch)
        if key not in cache:
            cfg, seed = B.GEOMS[geom]
            c = Q.cut(cfg, depth)
            w = B.weights(c, seed, wset)
            seqs = B.seq_ids(c, B.BATCHES[batch])
            ids, mask = B.padded(seqs)
            cache[key] = (c, w, seqs, ids, mask, [Q.record(c, w, i, m)["hidden"] for i, m in seqs])
        return cache[key]
    return get


def rows_against_oracle(eng, case, tally, what):
    """One run of the batch in the engine's current form: every sequence's rows against the oracle's; padded rows exactly
    0; and the head on its own - eng.run's sentence vector against mean / Dense 1 / Dense 2 of the device's own rows.
    -> the raw [B, L, H] rows (bytes are compared across forms)."""
    c, w, seqs, ids, mask, ref = case
    key = (what[0], what[1])
    got = eng.run_hidden(ids, mask)
    out = eng.run(ids, mask)
    if np.any(got[~mask.astype(bool)] != 0):
        tally.fail((what, "a padded row is not zero"))
    for b, (i, _m) in enumerate(seqs):
        n = i.shape[1]
        tally.add("hidden", key, got[b, :n], ref[b], what + (b, n))
        tally.add("pool", key, out[b][None], B.head_from_rows(w, got[b, :n])[None], what + (b, n))
    return got


@pytest.mark.parametrize("wset", ["plain", "peaked"])
def test_rows_match_the_oracle_at_every_depth(hip, rows_oracle, wset):
    """The planner's own forms at depth 1 - 4 (one engine per cut config: the layer tensors are the full model's), so that
    the last-layer FINAL form of each projection runs at each depth; both batches (above the few-rows limit: the tiled
    GEMMs; under it: the few-rows GEMM and the per-head attention)."""
    tally = B.Tally("depths " + wset)
    for depth in range(1, Q.FULL_W32.layers + 1):
        eng = None
        for batch in B.BATCHES:
            case = rows_oracle("full_w32", wset, depth, batch)
            eng = eng or B.engine(case[0], case[1])
            rows_against_oracle(eng, case, tally, ("full_w32", wset, "depth %d" % depth, batch))
        eng.close()
    tally.finish()


FULL_FORMS = {
    "tile small": dict(tile="small"), "tile pp:3": dict(tile="pp:3"), "tile pp:4": dict(tile="pp:4"), "tile pp:5": dict(tile="pp:5"),
    "add-norm two launches": dict(fuse_norm=(0, 64)), "add-norm 64-row kernel": dict(fuse_norm=(1, 64)), "add-norm pair-split": dict(fuse_norm=(2, 64)),
    "pp:5 fused QKV": dict(ATT_FORMS["shared-dma"], tile="pp:5"), "pp:5 kv_prep": dict(ATT_FORMS["shared-dma"], tile="pp:5", fuse_qkv=False),
    "pp:4 fused QKV": dict(ATT_FORMS["shared-dma"], tile="pp:4"), "pp:4 kv_prep": dict(ATT_FORMS["shared-dma"], tile="pp:4", fuse_qkv=False),
    "pp:4 GeGLU through LDS": dict(tile="pp:4", geglu4=False), "pp:3 GeGLU through LDS": dict(tile="pp:3", geglu4=False),
    "pp:4 pair-split": dict(tile="pp:4", fuse_norm=(2, 64)),
}
FULL_FORMS.update(ATT_FORMS)


@pytest.mark.parametrize("wset", ["plain", "peaked"])
def test_rows_match_the_oracle_in_every_form(hip, rows_oracle, wset):
    """Full depth (sliding and full-attention layers alternating, window 17), every form behind a switch, on the batch
    above the few-rows limit (partly filled 128- and 256-row tiles); the attention forms also on the one under it.
    Forms documented as bit-identical must give the same BYTES in every hidden row, not only in the pooled vectors: the
    few-rows GEMM and the 128 x 128 kernel; the pair-split add-norm and the two-launch chain.  The fused QKV epilogue sums
    a head's squares in another order: it must NOT be the same bytes (or it did not run)."""
    tally = B.Tally("forms " + wset)
    over, under = (rows_oracle("full_w32", wset, Q.FULL_W32.layers, b) for b in ("over", "under"))
    eng = B.engine(over[0], over[1])
    raw = {}
    for name, kw in FULL_FORMS.items():
        for batch, case in (("over", over), ("under", under)):
            if batch == "under" and name not in ATT_FORMS and name != "tile small":
                continue
            with B.form(eng, **kw):
                raw[(name, batch)] = rows_against_oracle(eng, case, tally, ("full_w32", wset, name, batch))
    raw[("default", "under")] = rows_against_oracle(eng, under, tally, ("full_w32", wset, "default", "under"))
    eng.close()
    assert raw[("tile small", "under")].tobytes() == raw[("default", "under")].tobytes(), "few-rows GEMM vs the 128 x 128 kernel"
    assert raw[("add-norm pair-split", "over")].tobytes() == raw[("add-norm two launches", "over")].tobytes(), "pair-split add-norm vs two launches"
    for t in ("pp:5", "pp:4"):
        assert raw[(t + " fused QKV", "over")].tobytes() != raw[(t + " kv_prep", "over")].tobytes(), t + ": the fused QKV epilogue did not run"
    tally.finish()


@pytest.mark.parametrize("wset", ["plain", "peaked"])
def test_rows_match_the_oracle_small_geometry(hip, rows_oracle, wset):
    """256-wide, 2 q heads on one kv head, 3 layers (2 sliding with window 17, 1 full): the planner's own forms and the
    three attention forms, both batches."""
    tally = B.Tally("small " + wset)
    cases = [(b, rows_oracle("small", wset, B.SMALL.layers, b)) for b in B.BATCHES]
    eng = B.engine(cases[0][1][0], cases[0][1][1])
    for name, kw in dict(ATT_FORMS, default={}).items():
        for batch, case in cases:
            with B.form(eng, **kw):
                rows_against_oracle(eng, case, tally, ("small", wset, name, batch))
    eng.close()
    tally.finish()
