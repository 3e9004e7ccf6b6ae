"""The search-time chain (cqs_amd/csrc/query_forward.hip) token by token.  tests/test_query_path_gpu.py compares the POOLED
sentence vector; a mean over T tokens divides what a kernel gets wrong on one row - a partly filled row block, the last
key of a tile, the seam between the key halves, the window compare, which of x0 / x1 holds the residual - by about T.
Here the test hook `cqs_hip_debug_embedder_query_state` reads the chain's per-token state off the device after a blocking
query: the f32 residual stream entering the head and the last layer's down projection.  From them the residual stream
after the last layer, the final-norm hidden state and the pooled vector are rebuilt in float64 and compared, row by row,
with the fp32 oracle (oracle/gemma3_ref.py, its `tap` recording the same points) - for every depth (one engine per
depth: the layer tensors of a cut config are those of the full one), at every length where a launcher changes form.

Bounds: tests/query_state.py BOUNDS (3 x the device's measured worst distance to the oracle; DESIGN.md "Per-token check of
the search-time chain").  tests/test_query_state_sensitivity_cpu.py keeps them honest on a CPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import query_state as Q
from cqs_amd.embedder import HipEmbedEngine, bf16_to_f32, default_config
from oracle import gemma3_ref as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def engine(cfg, w):
    c = default_config()
    c.vocab_size, c.hidden, c.layers, c.heads, c.kv_heads = cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads
    c.head_dim, c.intermediate, c.dense_hidden = cfg.head_dim, cfg.intermediate, cfg.dense_hidden
    c.sliding_window, c.sliding_pattern, c.max_seq = cfg.sliding_window, cfg.sliding_pattern, cfg.max_seq
    c.query_pre_attn_scalar = cfg.query_pre_attn_scalar
    eng = HipEmbedEngine(c)
    eng.set_weights(w)
    return eng


def weights(cfg, seed, wset):
    w = G.seeded_weights(cfg, seed=seed)
    return Q.peaked(cfg, w) if wset == "peaked" else w


def raw_state(eng, ids, mask):
    """One blocking query + the hooked state, as raw arrays (bytes are compared across runs)."""
    out = eng.run(ids, mask)[0]
    st = eng.debug_query_state(ids.shape[1])
    st["out"] = out
    return st


def same_bytes(a, b):
    return a["which_x"] == b["which_x"] and all(a[k].tobytes() == b[k].tobytes() for k in ("x", "y", "qkv", "h", "d1", "out"))


def rebuild(cfg, w, st):
    """The hooked state -> the tensors the oracle records, rebuilt on the host in float64."""
    last = cfg.layers - 1
    x = st["x"].astype(np.float64)
    y = bf16_to_f32(st["y"]).astype(np.float64)
    lo = x + Q.rms64(y, w[f"layers.{last}.post_feedforward_layernorm.weight"], cfg.rms_eps)
    hidden = Q.rms64(lo, w["norm.weight"], cfg.rms_eps)
    pooled = hidden.mean(0)
    d1 = G.round_bf16(pooled.astype(np.float32)).astype(np.float64) @ w["dense1.weight"].astype(np.float64).T
    out = bf16_to_f32(st["d1"]).astype(np.float64) @ w["dense2.weight"].astype(np.float64).T
    return {("post_attn", last): x, ("ffn", last): y, ("layer_out", last): lo, "hidden": hidden, "pooled": pooled,
            "d1_from_pooled": d1, "d1": bf16_to_f32(st["d1"]).astype(np.float64), "out_from_d1": out, "out": st["out"].astype(np.float64)}


def against_oracle(cfg, w, key, ids, mask, st, what, worst):
    """The per-token comparison of one query: residual stream, final-norm hidden state; and the head on its own - the
    pooled vector rebuilt from the device's own rows against the device's Dense 1 input / output."""
    last = cfg.layers - 1
    ref = Q.record(cfg, w, ids, mask)
    got = rebuild(cfg, w, st)
    assert st["which_x"] == 1, "launch_query_forward ends on q_x1 for every depth"
    Q.check("resid", key, got[("post_attn", last)], ref[("post_attn", last)], what, worst)
    Q.check("resid", key, got[("layer_out", last)], ref[("layer_out", last)], what, worst)
    Q.check("hidden", key, got["hidden"], ref["hidden"], what, worst)
    # the head: the device pooled ITS rows (mean over exactly T of them, bf16) and multiplied by Dense 1 / Dense 2
    Q.check("pool", key, got["d1"][None], got["d1_from_pooled"][None], what, worst)
    Q.check("pool", key, got["out"][None], got["out_from_d1"][None], what, worst)


def report(worst, name):
    for (key, place), m in sorted(worst.items()):
        print("QSTATE %s %s %s 1-cos=%.3e elem=%.4f col=%.4f" % (name, "/".join(key), place, m[0], m[1], m[2]))
    path = os.environ.get("CQS_QUERY_STATE_REPORT")
    if path:
        with open(path, "a") as f:
            for (key, place), m in sorted(worst.items()):
                f.write(json.dumps({"test": name, "key": list(key), "place": place, "one_minus_cos": m[0], "elem": m[1], "col": m[2]}) + "\n")


@pytest.mark.parametrize("wset", ["plain", "peaked"])
@pytest.mark.parametrize("geom", ["small", "full", "full_w32"])
def test_token_rows_match_the_oracle_at_every_depth_and_length(hip, geom, wset):
    """Every depth x every length of Q.LENS.  Each query runs twice - the first launches the chain eagerly, the second
    captures and replays its graph - and the hooked state must be the same bytes both times (the hook itself only reads)."""
    cfg, seed = Q.GEOMS[geom]
    worst = {}
    for depth in range(1, cfg.layers + 1):
        c = Q.cut(cfg, depth)
        w = weights(c, seed, wset)
        eng = engine(c, w)
        for n in Q.LENS:
            ids, mask = Q.ids_for(c, n, seed=1000 + n)
            a = raw_state(eng, ids, mask)
            b = raw_state(eng, ids, mask)
            assert same_bytes(a, b), (geom, wset, depth, n)
            against_oracle(c, w, (geom, wset), ids, mask, a, (depth, n), worst)
        st = eng.query_graph_stats()
        assert st["failed"] == 0 and st["captured"] == len(Q.LENS) and st["eager"] == len(Q.LENS), st
        eng.close()
    report(worst, "grid")


# ---- the forms behind documented switches: one child process per setting (the variables are read once per process) -------
FORMS = [("CQS_HIP_QUERY_STAGED", 64), ("CQS_HIP_QUERY_ROW_SPLIT", 64), ("CQS_HIP_QUERY_ATTN80", 128), ("CQS_HIP_QUERY_FUSE_ATTN", 64)]
FORM_GEOMS = ["small", "full_w32"]
_child_failed = []                      # once a child process has failed, no further one is started in this session


def child_dump(path):
    """Runs in the child: the per-token state of the form this process's environment selects, at every length of Q.LENS
    that form serves, full depth; then a length above the form's cap, which must take the batch chain."""
    cap = int(os.environ["QSTATE_CAP"])
    dump = {}
    for geom in FORM_GEOMS:
        cfg, seed = Q.GEOMS[geom]
        w = weights(cfg, seed, "plain")
        eng = engine(cfg, w)
        for n in [n for n in Q.LENS if n <= cap]:
            ids, mask = Q.ids_for(cfg, n, seed=1000 + n)
            st = raw_state(eng, ids, mask)
            for k in ("x", "y", "d1", "out"):
                dump["%s.%d.%s" % (geom, n, k)] = st[k]
            dump["%s.%d.which_x" % (geom, n)] = np.int64(st["which_x"])
        ids, mask = Q.ids_for(cfg, cap + 1, seed=77)
        over = eng.run(ids, mask)
        try:
            eng.debug_query_state(cap + 1)
            hooked = True
        except Exception:
            hooked = False
        os.environ["CQS_HIP_QUERY_PATH"] = "0"
        eng_b = engine(cfg, w)
        del os.environ["CQS_HIP_QUERY_PATH"]
        dump["%s.over_cap_is_batch_chain" % geom] = np.int64(np.array_equal(over, eng_b.run(ids, mask)) and not hooked)
        eng.close(); eng_b.close()
    np.savez(path, **dump)


@pytest.mark.parametrize("var,cap", FORMS)
def test_forms_behind_switches_match_the_oracle(hip, tmp_path, var, cap):
    """`var`=0 selects kernels the default never runs (gather-load GEMMs; one workgroup per 8 columns; the two-halves
    kernel at 65-80 tokens; attention and o_proj as two launches).  Each is held to the oracle bounds of the default form."""
    assert not _child_failed, "not started: the child for %s failed before this one" % _child_failed[0]
    path = str(tmp_path / "dump.npz")
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_query_state_gpu as t\nt.child_dump(%r)\n" % (ROOT, os.path.join(ROOT, "tests"), path)
    env = dict(os.environ, QSTATE_CAP=str(cap))
    env[var] = "0"
    _child_failed.append(var)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    _child_failed.pop()
    d = np.load(path)
    worst = {}
    for geom in FORM_GEOMS:
        cfg, seed = Q.GEOMS[geom]
        w = weights(cfg, seed, "plain")
        assert int(d["%s.over_cap_is_batch_chain" % geom]) == 1, (var, geom, "a length above the form's cap must take the batch chain")
        for n in [n for n in Q.LENS if n <= cap]:
            ids, mask = Q.ids_for(cfg, n, seed=1000 + n)
            st = {k: d["%s.%d.%s" % (geom, n, k)] for k in ("x", "y", "d1", "out")}
            st["which_x"] = int(d["%s.%d.which_x" % (geom, n)])
            against_oracle(cfg, w, (geom, "plain"), ids, mask, st, (var, n), worst)
    report(worst, var + "=0")


# ---- geometries that take the unfused attention + plain o_proj, capped at 64 tokens -----------------------------------------
def _variant(cfg, **kw):
    d = dict(cfg.__dict__)
    d.update(kw)
    return G.GemmaConfig(**d)


FALLBACKS = {
    "heads1_kv1": (_variant(Q.SMALL, heads=1, kv_heads=1), "small"),
    "heads4_kv1": (_variant(Q.SMALL, heads=4, kv_heads=1), "small"),
    "heads4_kv2": (_variant(Q.SMALL, heads=4, kv_heads=2), "small"),
    "heads2_kv2": (_variant(Q.SMALL, heads=2, kv_heads=2), "small"),
    "inter640": (_variant(Q.SMALL, intermediate=640), "small"),            # a multiple of 128, not a staged K class
    "hidden768_heads2": (_variant(Q.FULL_W32, heads=2), "full_w32"),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_geometry_fallbacks_match_the_oracle(hip, monkeypatch, name):
    """Head layouts other than 2 or 3 q heads on one kv head, and an intermediate size outside the staged K classes:
    query_forward_supported admits them, the chain serves them up to 64 tokens.  Held to the bounds of the geometry they
    were cut from (same hidden size, same number formats, same depth); 65 tokens must take the batch chain."""
    cfg, like = FALLBACKS[name]
    w = weights(cfg, 41, "plain")
    eng = engine(cfg, w)
    worst = {}
    for n in [n for n in Q.BREAKS if n <= 64]:
        ids, mask = Q.ids_for(cfg, n, seed=1000 + n)
        a = raw_state(eng, ids, mask)
        assert same_bytes(a, raw_state(eng, ids, mask)), (name, n)
        against_oracle(cfg, w, (like, "plain"), ids, mask, a, (name, n), worst)
    monkeypatch.setenv("CQS_HIP_QUERY_PATH", "0")
    eng_b = engine(cfg, w)
    monkeypatch.delenv("CQS_HIP_QUERY_PATH")
    ids, mask = Q.ids_for(cfg, 65, seed=77)
    if name != "hidden768_heads2":                       # (2 heads on one kv head keep the fused kernels: 128 tokens)
        assert np.array_equal(eng.run(ids, mask), eng_b.run(ids, mask))
        with pytest.raises(Exception):
            eng.debug_query_state(65)
    else:
        for n in (65, 80, 81, 97, 128):
            ids, mask = Q.ids_for(cfg, n, seed=1000 + n)
            against_oracle(cfg, w, (like, "plain"), ids, mask, raw_state(eng, ids, mask), (name, n), worst)
    eng.close(); eng_b.close()
    report(worst, "fallback " + name)


# ---- rows past T left by a longer query are never read ------------------------------------------------------------------------
HISTORY = [128, 5, 96, 1, 64, 17, 80]


@pytest.mark.parametrize("geom", ["small", "full_w32"])
def test_state_does_not_depend_on_earlier_queries(hip, geom):
    cfg, seed = Q.GEOMS[geom]
    w = weights(cfg, seed, "plain")
    used = engine(cfg, w)
    for n in HISTORY:
        ids, mask = Q.ids_for(cfg, n, seed=2000 + n)
        a = raw_state(used, ids, mask)
        fresh = engine(cfg, w)
        b = raw_state(fresh, ids, mask)
        fresh.close()
        assert same_bytes(a, b), (geom, n)
    used.close()


def test_graph_and_eager_engines_agree_on_the_hooked_state(hip, monkeypatch):
    """test_graph_replay_equals_eager_across_lengths compares the pooled vector; here both engines get the same history
    and every hooked row must be the same bytes - a replayed graph whose kernels read or wrote other rows than the eager
    launches would differ here first."""
    cfg, seed = Q.GEOMS["small"]
    w = weights(cfg, seed, "plain")
    eng_g = engine(cfg, w)
    monkeypatch.setenv("CQS_HIP_QUERY_GRAPH", "0")
    eng_e = engine(cfg, w)
    monkeypatch.delenv("CQS_HIP_QUERY_GRAPH")
    for j, n in enumerate(HISTORY + HISTORY + [33, 128, 33]):
        ids, mask = Q.ids_for(cfg, n, seed=3000 + j)
        assert same_bytes(raw_state(eng_g, ids, mask), raw_state(eng_e, ids, mask)), (j, n)
    st = eng_g.query_graph_stats()
    assert st["failed"] == 0 and st["captured"] >= len(HISTORY) and st["replays"] >= len(HISTORY), st
    assert eng_e.query_graph_stats()["captured"] == 0
    eng_g.close(); eng_e.close()
