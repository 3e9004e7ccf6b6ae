"""Keeps the per-token check of the batch chain (tests/batch_state.py, tests/test_batch_state_gpu.py) honest, on a CPU - the
twin of test_query_state_sensitivity_cpu.py.  A correct device - the forward with every GEMM operand rounded to bf16,
`query_state.forward_emulated` - must pass the committed bounds at every length the GPU test runs; every error of
`query_state.planted_errors`, and a key of the neighbouring packed sequence attended by a sequence's first 16-query tile,
planted into the fp32 oracle, must be rejected.  For the mask probe: its ratio band accepts the emulation on all three
window cases and rejects window +-1, the masked last key and the neighbour leak.

Why the probe exists: `test_mask_plants_hide_in_rounding_noise_at_the_real_window` asserts the record that at the real
window of 257 the mask plants move the final hidden state of a random-weight model by about as much as bf16 rounding does
(0.0 - 3.6 x on the element measure), so that a hidden-state bound with its 3 x margin cannot be relied on to tell them from
a correct device."""
import numpy as np
import pytest

import batch_state as B
import query_state as Q

PLANT_AT = {"full_w32": (300, 2), "small": (257, 1)}           # tokens, and a sliding-window layer in the middle of the model
MASK_PLANTS = ("window one too wide", "window one too narrow", "last key masked for the last 16-query block")
LEAK = "a key of the neighbouring packed sequence attended by the first 16-query tile"
NEIGHBOUR = 129                                                # tokens of the sequence packed in front


def plants_for(cfg, w, layer, T, neighbour):
    """planted_errors + the neighbour leak.  `neighbour` = a record() of the sequence packed in front: its last row is the
    one a kernel that reads one key before a sequence's start would fetch."""
    errs = dict(Q.planted_errors(cfg, w, layer, T))
    n = neighbour[("qkv", 0)].shape[0]
    errs[LEAK] = B.leak_plant(cfg, w, layer, lambda l: neighbour[("qkv", l)][-1], n - 1)
    return errs


@pytest.mark.parametrize("wset", ["plain", "peaked"])
@pytest.mark.parametrize("geom", sorted(B.GEOMS))
def test_a_correct_bf16_device_passes(geom, wset):
    cfg, seed = B.GEOMS[geom]
    w = B.weights(cfg, seed, wset)
    worst = [0.0, 0.0, 0.0]
    for name, lens in B.BATCHES.items():
        for ids, mask in B.seq_ids(cfg, lens):
            clean = Q.record(cfg, w, ids, mask)["hidden"]
            emu = Q.forward_emulated(cfg, w, ids)["hidden"]
            m = Q.measures(emu, clean)
            worst = [max(a, b) for a, b in zip(worst, m)]
            assert B.passes((geom, wset), emu, clean), (geom, wset, name, ids.shape[1], m, B.BOUNDS[(geom, wset)]["hidden"])
    print("EMULATED", geom, wset, "hidden 1-cos=%.3e elem=%.4f col=%.4f" % tuple(worst))


@pytest.mark.parametrize("wset", ["plain", "peaked"])
@pytest.mark.parametrize("geom", sorted(B.GEOMS))
def test_every_planted_error_is_rejected(geom, wset):
    """On `small` with peaked weights the masked last key is invisible (the sharp softmax of the last block's queries puts
    no weight on that key: the planted forward equals the clean one to 1e-6); it is left to the probe, which shows it at
    any weights (test_the_probe_band_accepts_a_correct_device_and_rejects_the_mask_plants)."""
    cfg, seed = B.GEOMS[geom]
    T, layer = PLANT_AT[geom]
    w = B.weights(cfg, seed, wset)
    ids, mask = Q.ids_for(cfg, T, seed=1000 + T)
    nids, nmask = Q.ids_for(cfg, NEIGHBOUR, seed=1000 + NEIGHBOUR)
    clean = Q.record(cfg, w, ids, mask)
    emu = Q.measures(Q.forward_emulated(cfg, w, ids)["hidden"], clean["hidden"])
    errs = plants_for(cfg, w, layer, T, Q.record(cfg, w, nids, nmask))
    assert len(errs) >= 11
    missed = []
    for name, pl in errs.items():
        rec = Q.record(cfg, w, ids, mask, plant=pl)
        m = Q.measures(rec["hidden"], clean["hidden"])
        print("PLANT", geom, wset, name, "1-cos=%.3e elem=%.4f col=%.4f" % m, "x emulation: %.1f %.1f" % (m[0] / emu[0], m[1] / emu[1]))
        if B.passes((geom, wset), rec["hidden"], clean["hidden"]):
            missed.append(name)
    if (geom, wset) == ("small", "peaked"):
        assert MASK_PLANTS[2] in missed, "the masked last key became visible on small / peaked: hold it to the bounds too"
        missed.remove(MASK_PLANTS[2])
    assert not missed, missed


PROBE_T = {"w17": 300, "w257": 700, "full": 700}


@pytest.mark.parametrize("wcase", sorted(B.WINDOWS))
def test_the_probe_band_accepts_a_correct_device_and_rejects_the_mask_plants(wcase):
    cfg = B.probe_config("3:1", wcase)
    w = B.probe_weights(cfg)
    T = PROBE_T[wcase]
    ids, mask = B.probe_seq(1, T)
    nids, nmask = B.probe_seq(0, NEIGHBOUR)
    clean = Q.record(cfg, w, ids, mask)
    emu = Q.forward_emulated(cfg, w, ids)
    m = Q.measures(emu["hidden"], clean["hidden"])
    print("PROBE", wcase, T, "emulated device 1-cos=%.3e elem=%.4f col=%.4f" % m)
    assert B.probe_violations(emu["hidden"][None], clean["hidden"][None], ids, mask, cfg.heads) == []
    assert B.passes(("probe", wcase), emu["hidden"], clean["hidden"]), (m, B.BOUNDS[("probe", wcase)])
    errs = plants_for(cfg, w, 0, T, Q.record(cfg, w, nids, nmask))
    names = [n for n in MASK_PLANTS + (LEAK,) if n in errs]
    assert len(names) == (2 if wcase == "full" else 4)
    for name in names:
        rec = Q.record(cfg, w, ids, mask, plant=errs[name])
        bad = B.probe_violations(rec["hidden"][None], clean["hidden"][None], ids, mask, cfg.heads)
        print("PROBE", wcase, T, name, "elem=%.4f" % Q.measures(rec["hidden"], clean["hidden"])[1], "violations", len(bad), bad[:2])
        assert bad, (wcase, name)
        rows = {p for _, p, _, _, _, _ in bad}
        if name == LEAK:
            assert rows <= set(range(16)), rows                      # the band names the tokens that read the wrong key
        elif name == MASK_PLANTS[2]:
            assert rows <= set(range(16 * ((T - 1) // 16), T)), rows


# the mask plants that a bound of 3 x the EMULATION's own distance accepts on all three measures at window 257
HIDDEN_AT_257 = {"plain": MASK_PLANTS[1:], "peaked": MASK_PLANTS[2:]}


@pytest.mark.parametrize("wset", ["plain", "peaked"])
def test_mask_plants_hide_in_rounding_noise_at_the_real_window(wset):
    """The record behind the probe.  768-wide, 4 layers, 300 tokens, window 257 (query_state.FULL).  As multiples of what
    bf16 rounding moves the final hidden state (element measure / 1 - cos):
      plain   window one too wide 1.7 / 4.3   too narrow 1.4 / 2.5   last key masked 0.8 / 1.2
      peaked  window one too wide 2.4 / 5.4   too narrow 3.6 / 10.8  last key masked 0.02 / 0.00
    A bound sits 3 x above a device that itself may sit up to 2 x above the emulation.  Even a bound of 3 x the emulation
    accepts the plants of HIDDEN_AT_257 on every measure, and no plant reaches 4 x on the element measure - the smallest
    plant the random-weight check is built to catch stands at 5.4 x.  The probe separates all of them by 90 x and more."""
    cfg, seed = Q.GEOMS["full"]
    w = B.weights(cfg, seed, wset)
    ids, mask = Q.ids_for(cfg, 300, seed=1300)
    clean = Q.record(cfg, w, ids, mask)
    emu = Q.measures(Q.forward_emulated(cfg, w, ids)["hidden"], clean["hidden"])
    errs = Q.planted_errors(cfg, w, 2, 300)
    for name in MASK_PLANTS:
        m = Q.measures(Q.record(cfg, w, ids, mask, plant=errs[name])["hidden"], clean["hidden"])
        print("WINDOW-257", wset, name, "elem %.4f = %.2f x emulation, 1-cos %.3e = %.2f x, col %.2f x" % (m[1], m[1] / emu[1], m[0], m[0] / emu[0], m[2] / emu[2]))
        assert m[1] < 4.0 * emu[1], (wset, name, m, emu)
        if name in HIDDEN_AT_257[wset]:
            assert all(m[i] < 3.0 * emu[i] for i in range(3)), (wset, name, m, emu)
