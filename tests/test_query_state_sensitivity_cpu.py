"""Keeps the per-token bounds of tests/query_state.py honest, on a CPU.  Each error a search-time kernel could make is
planted into the fp32 oracle through `gemma3_ref.forward(tap=...)` - one value or one comparison wrong, in ONE layer unless
stated - and the planted forward is measured against the clean one exactly as tests/test_query_state_gpu.py measures
the device against the oracle.  With the committed bounds every planted error must be rejected at 33, 80 and 128 tokens,
and a correct device - the forward with every GEMM operand rounded to bf16 - must pass.  If a bound is ever loosened past
the point where it stops telling the two apart, this fails without a GPU.

Why the per-token check exists - what the POOLED bound of tests/test_query_path_gpu.py (cos > 0.999 against the oracle)
lets through, measured with these same plants: the zeroed attention row, the head swap, the FFN row copy and the masked last
key at every one of the three lengths, on all three geometries (pooled cosines 0.99930 - 1.0); the keys rotated late on
the 768-wide geometry with its real window (0.99936 - 0.99955).  It catches the window errors.  On the 768-wide geometries
the head swap and the FFN row copy at 80 and 128 tokens also pass that file's comparison with the batch chain (cos > 0.9999,
largest difference < 3 % of the largest component).  `test_the_pooled_bound_misses_them` asserts that record, so that it
stays true to the code."""
import numpy as np
import pytest

import query_state as Q
from oracle import gemma3_ref as G

LENS = [33, 80, 128]
PLANT_LAYER = {"small": 1, "full": 2, "full_w32": 2}          # a sliding-window layer in the middle of each model


def _cos(a, b):
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.fixture(scope="module")
def planted():
    """{(geom, T): (clean record, {name: planted record})}"""
    out = {}
    for geom, (cfg, seed) in Q.GEOMS.items():
        w = G.seeded_weights(cfg, seed=seed)
        for T in LENS:
            ids, mask = Q.ids_for(cfg, T, seed=1000 + T)
            clean = Q.record(cfg, w, ids, mask)
            errs = Q.planted_errors(cfg, w, PLANT_LAYER[geom], T)
            out[(geom, T)] = (clean, {name: Q.record(cfg, w, ids, mask, plant=pl) for name, pl in errs.items()})
    return out


def test_restated_forward_is_the_oracle():
    """forward_emulated without rounding = gemma3_ref.forward (so that WITH rounding it is a correct device and nothing else);
    attn_from_qkv without switches = the oracle's attention."""
    for geom in ("small", "full_w32"):
        cfg, seed = Q.GEOMS[geom]
        w = G.seeded_weights(cfg, seed=seed)
        ids, mask = Q.ids_for(cfg, 80, seed=5)
        ref = Q.record(cfg, w, ids, mask)
        emu = Q.forward_emulated(cfg, w, ids, rnd=None)
        for k in [("attn", 1), ("layer_out", cfg.layers - 1), "hidden"]:
            m = Q.measures(emu[k], ref[k])
            assert m[0] < 1e-9 and m[1] < 1e-4, (geom, k, m)
        assert np.max(np.abs(emu["out"] - ref["out"])) < 1e-4 * np.abs(ref["out"]).max()


@pytest.mark.parametrize("geom", sorted(Q.GEOMS))
def test_a_correct_bf16_device_passes(geom):
    cfg, seed = Q.GEOMS[geom]
    w = G.seeded_weights(cfg, seed=seed)
    for T in LENS:
        ids, mask = Q.ids_for(cfg, T, seed=1000 + T)
        clean = Q.record(cfg, w, ids, mask)
        emu = Q.forward_emulated(cfg, w, ids)
        print(geom, T, "bf16 emulation: hidden", Q.measures(emu["hidden"], clean["hidden"]))
        assert Q.passes((geom, "plain"), emu, clean, cfg.layers), (geom, T)


@pytest.mark.parametrize("geom", sorted(Q.GEOMS))
def test_every_planted_error_is_rejected(planted, geom):
    cfg, _ = Q.GEOMS[geom]
    missed = []
    for T in LENS:
        clean, errs = planted[(geom, T)]
        assert len(errs) >= 7
        for name, rec in errs.items():
            print(geom, T, name, "hidden", Q.measures(rec["hidden"], clean["hidden"]),
                  "resid", Q.measures(rec[("layer_out", cfg.layers - 1)], clean[("layer_out", cfg.layers - 1)]))
            if Q.passes((geom, "plain"), rec, clean, cfg.layers):
                missed.append((T, name))
    assert not missed, missed


TABLE = ("last token's attention output zeroed", "two heads swapped on the last token",
         "last token's FFN row copied from its neighbour", "last key masked for the last 16-query block")


def test_the_pooled_bound_misses_them(planted):
    """The record of why the per-token check exists.  cos > 0.999 on the pooled vector accepts each per-token error of
    TABLE at every geometry and length (lowest pooled cosine 0.99930: the zeroed attention row at 33 tokens); on the 768-wide
    geometries at 80 and 128 tokens the head swap and the FFN row copy also pass the comparison with the batch chain
    (cos > 0.9999, largest difference < 3 % of the largest component).  The per-token measure rejects all of them
    (test_every_planted_error_is_rejected)."""
    for (geom, T), (clean, errs) in planted.items():
        for name in TABLE:
            c = _cos(errs[name]["out"], clean["out"])
            d = float(np.max(np.abs(errs[name]["out"] - clean["out"])) / np.abs(clean["out"]).max())
            print("POOLED", geom, T, name, c, d)
            assert c > 0.999, (geom, T, name, c)
            if geom != "small" and T >= 80 and name in TABLE[1:3]:
                assert c > 0.9999 and d < 3e-2, (geom, T, name, c, d)
