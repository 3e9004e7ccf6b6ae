"""GPU parity of the HIP EmbeddingGemma forward against the CPU oracle (oracle/gemma3_ref.py, itself
pinned to transformers' Gemma3TextModel) on seeded weights.  The reference holds no golden vector for
this path: numerics vs the real ONNX model are "parity unpinned"; what is checked is the
operator semantics.  Tolerances: bf16 matrix-core operands vs an fp32 oracle -> cosine >= 0.999
(SURVEY §7 hard part (e)); written in each test."""
import numpy as np
import pytest

from cqs_amd import _lib
from cqs_amd.embedder import (DOC_PREFIX, QUERY_PREFIX, Embedder, EmbedderError, HipEmbedEngine, default_config,
                              embed_batch_size, normalize_l2)
from oracle import gemma3_ref as G

pytestmark = pytest.mark.gpu


def make(cfg: G.GemmaConfig, seed=1):
    c = default_config()
    c.vocab_size, c.hidden, c.layers, c.heads, c.kv_heads = cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads
    c.head_dim, c.intermediate, c.dense_hidden = cfg.head_dim, cfg.intermediate, cfg.dense_hidden
    c.sliding_window, c.sliding_pattern, c.max_seq = cfg.sliding_window, cfg.sliding_pattern, cfg.max_seq
    c.query_pre_attn_scalar = cfg.query_pre_attn_scalar
    w = G.seeded_weights(cfg, seed=seed)      # bf16-exact values: both sides start from identical weights
    eng = HipEmbedEngine(c)
    eng.set_weights(w)
    return eng, w


def batch(cfg, lens, seed=0):
    rng = np.random.default_rng(seed)
    L = max(lens)
    ids = np.zeros((len(lens), L), np.int64)
    mask = np.zeros((len(lens), L), np.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(1, cfg.vocab_size, size=n)
        mask[i, :n] = 1
    return ids, mask


def cos(a, b):
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


SMALL = G.GemmaConfig(vocab_size=512, hidden=256, layers=3, heads=2, kv_heads=1, head_dim=256, intermediate=384,
                      dense_hidden=512, sliding_window=32, sliding_pattern=3, max_seq=256)


def test_hidden_states_small_model(hip):
    """3 layers (2 sliding with window 17, 1 full), ragged batch: final-norm hidden states vs the fp32 oracle."""
    eng, w = make(SMALL)
    ids, mask = batch(SMALL, [70, 1, 33, 64, 100])
    got = eng.run_hidden(ids, mask)
    ref = G.forward(SMALL, w, ids, mask, return_hidden=True)
    live = mask.astype(bool)
    assert np.all(got[~live] == 0)
    err = np.abs(got[live] - ref[live])
    scale = np.abs(ref[live]).mean()
    assert err.mean() / scale < 0.02 and err.max() / scale < 0.35, (err.mean() / scale, err.max() / scale)
    cs = [cos(got[b, t], ref[b, t]) for b in range(len(ids)) for t in range(int(mask[b].sum()))]
    assert min(cs) > 0.995, min(cs)
    eng.close()


def test_sentence_embeddings_gemma_dims(hip):
    """Real per-layer dims (768 / 3x256 / 1152, window 257) with 6 layers incl. one full-attention layer,
    sequences up to 600 tokens (crosses the sliding window): pooled + dense embeddings, cosine >= 0.999."""
    cfg = G.GemmaConfig(vocab_size=4096, layers=6, max_seq=1024)
    eng, w = make(cfg, seed=3)
    ids, mask = batch(cfg, [600, 37, 300, 2], seed=4)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    for i in range(len(ids)):
        assert cos(got[i], ref[i]) > 0.999, (i, cos(got[i], ref[i]))
        assert abs(np.linalg.norm(got[i]) / np.linalg.norm(ref[i]) - 1) < 0.03
    eng.close()


def test_padding_and_batch_invariance(hip):
    """Packed execution: a sequence's embedding does not depend on its batch neighbours or on padding.  Rows that
    take the same kernels agree to 1e-6; ONE row of <= 128 tokens takes the search-time kernels (query_forward.hip,
    another f32 association of the same products): cosine >= 0.9999 there (tests/test_query_path_gpu.py)."""
    eng, w = make(SMALL, seed=5)
    ids, mask = batch(SMALL, [50, 9, 120, 200], seed=6)
    full = eng.run(ids, mask)
    for i, n in enumerate([50, 9, 120, 200]):
        alone = eng.run(ids[i:i + 1, :n], mask[i:i + 1, :n])
        if n <= 128:
            assert cos(alone[0], full[i]) > 0.9999
        else:
            assert np.max(np.abs(alone[0] - full[i])) < 1e-6
    wide = eng.run(np.pad(ids, ((0, 0), (0, 40))), np.pad(mask, ((0, 0), (0, 40))))
    assert np.max(np.abs(wide - full)) < 1e-6
    a, b = eng.run(ids, mask), eng.run(ids, mask)      # determinism (tests/embedding_test.rs:108-122)
    assert np.array_equal(a, b)
    eng.close()


def test_io_contract_and_errors(hip):
    eng, w = make(SMALL, seed=7)
    ids, mask = batch(SMALL, [10, 0, 5], seed=8)
    out = eng.run(ids, mask)
    assert out.shape == (3, 256) and np.all(out[1] == 0) and np.all(np.isfinite(out))   # zero mask -> zero vector
    bad = mask.copy(); bad[0, 3] = 0                                                       # hole in the mask
    with pytest.raises(EmbedderError):
        eng.run(ids, bad)
    oob = ids.copy(); oob[0, 0] = SMALL.vocab_size
    with pytest.raises(EmbedderError):
        eng.run(oob, mask)
    long_ids, long_mask = batch(SMALL, [SMALL.max_seq + 1], seed=9)
    with pytest.raises(EmbedderError):
        eng.run(long_ids, long_mask)
    assert eng.dim() == 256 and eng.max_seq() == 256
    eng.close()


def test_embedder_surface(hip):
    """embed_documents / embed_query mirror: prefixes, batching by embed_batch_size, unit norm, cache, EmptyQuery."""
    eng, w = make(SMALL, seed=11)
    seen = []

    def tok(texts):   # deterministic stand-in tokenizer: BOS=2, EOS=1 framing like the Gemma post-processor
        seen.extend(texts)
        return [[2] + [3 + (ord(c) % 500) for c in t][:200] + [1] for t in texts]

    emb = Embedder(eng, tok, batch_size=4)
    docs = [f"fn item_{i}() {{ return {i}; }}" for i in range(10)]
    vecs = emb.embed_documents(docs)
    assert len(vecs) == 10 and all(s.startswith(DOC_PREFIX) for s in seen[:10])
    for v in vecs:
        assert v.shape == (256,) and abs(float(np.linalg.norm(v)) - 1.0) < 1e-4          # embedding_test.rs:47-56
    q = emb.embed_query("  find the item  ")
    assert seen[-1] == QUERY_PREFIX + "find the item"
    n = len(seen)
    q2 = emb.embed_query("find the item")
    assert len(seen) == n and np.array_equal(q, q2)                                      # LRU hit
    assert not np.allclose(q, emb.embed_documents(["find the item"])[0])                 # query != doc prefix
    with pytest.raises(EmbedderError):
        emb.embed_query("   ")
    one = emb.embed_documents([docs[3]])[0]              # alone: the search-time kernels; in the batch of 4: the batch chain
    assert cos(one, vecs[3]) > 0.9999
    assert embed_batch_size(768, 2048) == 32 and embed_batch_size(1024, 512) == 64
    assert np.allclose(normalize_l2(np.array([3.0, 4.0])), [0.6, 0.8], atol=1e-6)
    eng.close()


def test_load_dir_safetensors(hip, tmp_path):
    """cqs_hip_embedder_load_dir reads the Hugging Face layout (model.safetensors + 2_Dense + 3_Dense)."""
    import torch
    from safetensors.torch import save_file
    w = G.seeded_weights(SMALL, seed=13)
    (tmp_path / "2_Dense").mkdir(); (tmp_path / "3_Dense").mkdir()
    body = {("model." + k): torch.from_numpy(v) for k, v in w.items() if not k.startswith("dense")}
    body["model.layers.0.self_attn.q_proj.weight"] = body["model.layers.0.self_attn.q_proj.weight"].to(torch.bfloat16)
    save_file(body, str(tmp_path / "model.safetensors"), metadata={"format": "pt"})
    save_file({"linear.weight": torch.from_numpy(w["dense1.weight"])}, str(tmp_path / "2_Dense" / "model.safetensors"))
    save_file({"linear.weight": torch.from_numpy(w["dense2.weight"]).to(torch.float16)},
              str(tmp_path / "3_Dense" / "model.safetensors"))
    eng, _ = make(SMALL, seed=13)
    eng2 = HipEmbedEngine.load_dir(str(tmp_path), eng.cfg)
    ids, mask = batch(SMALL, [40, 17], seed=14)
    a, b = eng.run(ids, mask), eng2.run(ids, mask)
    assert all(cos(a[i], b[i]) > 0.9999 for i in range(2))   # dense2 went through f16 on disk
    eng.close(); eng2.close()


def _write_onnx_dir(root, w, cfg, flat):
    """The reference's local artefact (CQS_ONNX_DIR, download.rs:12-41) in the shape exporters produce: named
    parameters for the embedding table and the norm scales, `Linear` weights folded into anonymous TRANSPOSED MatMul
    initialisers found through the consuming node's name, big tensors in the `model.onnx_data` sidecar."""
    import onnx_bytes as ob
    d = root if flat else root / "onnx"
    d.mkdir(parents=True, exist_ok=True)
    side = bytearray(b"\0" * 24)                      # offsets do not start at 0
    nodes, inits, n_anon = [], [], [0]

    def ext(arr, dtype=ob.FLOAT):
        raw = ob.encode_values(arr, dtype)
        off = len(side)
        side.extend(raw)
        side.extend(b"\0" * ((-len(side)) % 16))
        return ("model.onnx_data", off, len(raw))

    def linear(path, wt, dtype=ob.FLOAT, external=False, name_hint=None):
        n_anon[0] += 1
        iname = f"onnx::MatMul_{1000 + n_anon[0]}"
        t = np.ascontiguousarray(wt.T)                # [in, out]: the MatMul operand
        nodes.append(ob.node("MatMul", f"/model/{path.replace('.', '/', 9).replace('layers/', 'layers.')}/MatMul" if name_hint is None else name_hint,
                             [f"h{n_anon[0]}", iname], [f"o{n_anon[0]}"]))
        inits.append(ob.tensor(iname, t, dtype, "external" if external else "raw", external=ext(t, dtype) if external else None))

    inits.append(ob.tensor("model.embed_tokens.weight", w["embed_tokens.weight"], ob.FLOAT, "external",
                           external=ext(w["embed_tokens.weight"])))
    nodes.append(ob.node("Gather", "/model/embed_tokens/Gather", ["model.embed_tokens.weight", "input_ids"], ["emb"]))
    for l in range(cfg.layers):
        p = f"layers.{l}."
        for nm in ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm"):
            inits.append(ob.tensor("model." + p + nm + ".weight", w[p + nm + ".weight"], ob.FLOAT,
                                   "float_data" if l == 0 else "raw", packed_dims=(l != 1)))
        for nm in ("q_norm", "k_norm"):
            inits.append(ob.tensor("model." + p + "self_attn." + nm + ".weight", w[p + "self_attn." + nm + ".weight"],
                                   ob.BFLOAT16 if nm == "k_norm" else ob.FLOAT))
        for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
            wt = w[p + "self_attn." + nm + ".weight"]
            linear(None, wt, ob.FLOAT16 if (nm == "v_proj" and l == 0) else ob.FLOAT, external=(nm == "q_proj"),
                   name_hint=f"/model/layers.{l}/self_attn/{nm}/MatMul")
        for nm in ("gate_proj", "up_proj", "down_proj"):
            linear(None, w[p + "mlp." + nm + ".weight"], external=(nm == "down_proj"), name_hint=f"/model/layers.{l}/mlp/{nm}/MatMul")
    inits.append(ob.tensor("model.norm.weight", w["norm.weight"]))
    linear(None, w["dense1.weight"], name_hint="/dense/linear/MatMul")             # recognised by shape
    linear(None, w["dense2.weight"], name_hint="/dense_1/linear/MatMul", external=True)
    # things a real graph also holds and the reader must ignore
    inits.append(ob.tensor("onnx::Reshape_77", np.array([1, -1, 256]), ob.INT64))
    inits.append(ob.tensor("scalar_eps", np.float32(1e-6).reshape(()), ob.FLOAT))
    nodes.append(ob.node("MatMul", "/model/rotary/MatMul", ["a", "b_not_an_initialiser"], ["c"]))
    (d / "model.onnx").write_bytes(ob.model(nodes, inits))
    (d / "model.onnx_data").write_bytes(bytes(side))
    return d


@pytest.mark.parametrize("flat", [False, True])
def test_load_dir_onnx_initialisers(hip, tmp_path, flat):
    """cqs_hip_embedder_load_dir on `onnx/model.onnx` (+ `model.onnx_data`) - what CQS_ONNX_DIR holds for the
    reference (src/embedder/download.rs:12-41,82) - gives the same embeddings as the same weights set tensor by
    tensor.  The file is written by the byte-level encoder in tests/onnx_bytes.py (no `onnx` package)."""
    w = G.seeded_weights(SMALL, seed=21)
    _write_onnx_dir(tmp_path, w, SMALL, flat)
    eng, _ = make(SMALL, seed=21)
    eng2 = HipEmbedEngine.load_dir(str(tmp_path), eng.cfg)
    ids, mask = batch(SMALL, [40, 17, 3], seed=22)
    a, b = eng.run(ids, mask), eng2.run(ids, mask)
    # f16 on disk for one v_proj; everything else is bit-identical after the bf16 conversion
    assert all(cos(a[i], b[i]) > 0.9999 for i in range(3))
    assert np.max(np.abs(a - b)) <= 2e-2 * np.abs(a).max()
    eng.close(); eng2.close()


def test_load_dir_onnx_rejects_broken_files(hip, tmp_path):
    import onnx_bytes as ob
    w = G.seeded_weights(SMALL, seed=23)
    cfg = default_config()
    c = make(SMALL, seed=23)[0]
    d = _write_onnx_dir(tmp_path / "ok", w, SMALL, flat=True)
    # truncated sidecar -> error, not a crash
    side = (d / "model.onnx_data").read_bytes()
    (d / "model.onnx_data").write_bytes(side[: len(side) // 2])
    with pytest.raises(Exception):
        HipEmbedEngine.load_dir(str(d), c.cfg)
    # a tensor missing -> finalize names it
    d2 = tmp_path / "missing"
    d2.mkdir()
    (d2 / "model.onnx").write_bytes(ob.model([], [ob.tensor("model.norm.weight", w["norm.weight"])]))
    with pytest.raises(Exception):
        HipEmbedEngine.load_dir(str(d2), c.cfg)
    # garbage bytes
    d3 = tmp_path / "garbage"
    d3.mkdir()
    (d3 / "model.onnx").write_bytes(b"\xff" * 100)
    with pytest.raises(Exception):
        HipEmbedEngine.load_dir(str(d3), c.cfg)
    # an external location that climbs out of the directory is refused (download.rs:17-29)
    d4 = tmp_path / "escape"
    d4.mkdir()
    t = ob.tensor("model.norm.weight", w["norm.weight"], ob.FLOAT, "external", external=("../ok/model.onnx_data", 0, None))
    (d4 / "model.onnx").write_bytes(ob.model([], [t]))
    with pytest.raises(Exception):
        HipEmbedEngine.load_dir(str(d4), c.cfg)
    c.close()


def test_long_sequences_and_many_rows(hip):
    """max_seq-long inputs (2048 tokens: many key blocks, window edges on both sides, multi-tile GEMMs) and a
    64-sequence ragged batch, against the fp32 oracle."""
    cfg = G.GemmaConfig(vocab_size=1024, hidden=256, layers=3, heads=3, kv_heads=1, head_dim=256, intermediate=384,
                        dense_hidden=256, sliding_window=512, sliding_pattern=3, max_seq=2048)
    eng, w = make(cfg, seed=21)
    ids, mask = batch(cfg, [2048, 1500], seed=22)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    for i in range(2):
        assert cos(got[i], ref[i]) > 0.999, (i, cos(got[i], ref[i]))
    rng = np.random.default_rng(23)
    lens = [int(x) for x in rng.integers(1, 200, size=64)]
    ids, mask = batch(cfg, lens, seed=24)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    cs = [cos(got[i], ref[i]) for i in range(64)]
    assert min(cs) > 0.998, min(cs)
    eng.close()


def test_gqa_two_kv_heads(hip):
    """heads / kv_heads grouping other than 3:1 (4 q-heads over 2 kv-heads)."""
    cfg = G.GemmaConfig(vocab_size=512, hidden=256, layers=2, heads=4, kv_heads=2, head_dim=256, intermediate=256,
                        dense_hidden=256, sliding_window=64, sliding_pattern=2, max_seq=256)
    eng, w = make(cfg, seed=31)
    ids, mask = batch(cfg, [130, 7, 64], seed=32)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    for i in range(3):
        assert cos(got[i], ref[i]) > 0.999, (i, cos(got[i], ref[i]))
    eng.close()


@pytest.mark.parametrize("kernel", ["dma", "reg"])
@pytest.mark.parametrize("layout,heads,kv", [("shared", 3, 1), ("per-head", 3, 1), ("shared", 4, 2), ("shared", 4, 1)])
def test_attention_workgroup_layouts(hip, layout, heads, kv, kernel, monkeypatch):
    """The attention kernel has two workgroup layouts (all q-heads of a kv head share one staged K / V^T tile
    when the batch is large enough to fill the chip; one q-head per workgroup otherwise).  Both against the
    fp32 oracle on the real head geometry (3 q-heads, 1 kv head) and the 2:1 / 4:1 sharing variants,
    sliding + full layers, ragged lengths."""
    monkeypatch.setenv("CQS_HIP_ATT_LAYOUT", layout)
    # head-sharing workgroups have two kernels: "dma" (64-key blocks fetched by LDS-DMA into a double buffer; the
    # default) and "reg" (32-key blocks staged through registers); per-head workgroups always run the latter
    monkeypatch.setenv("CQS_HIP_ATT_KERNEL", kernel)
    if layout == "per-head" and kernel == "dma":
        pytest.skip("per-head workgroups have one kernel")
    cfg = G.GemmaConfig(vocab_size=512, hidden=256, layers=3, heads=heads, kv_heads=kv, head_dim=256, intermediate=256,
                        dense_hidden=256, sliding_window=64, sliding_pattern=3, max_seq=512)
    eng, w = make(cfg, seed=41)
    ids, mask = batch(cfg, [300, 65, 64, 1, 129, 200, 33, 96, 511, 512, 63, 31], seed=42)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    for i in range(len(ids)):
        assert cos(got[i], ref[i]) > 0.999, (layout, heads, kv, i, cos(got[i], ref[i]))
    eng.close()


@pytest.mark.parametrize("kernel", ["dma", "reg"])
def test_attention_real_window_shared_layout(hip, kernel, monkeypatch):
    """The production window (|q - k| < 257) on sequences around it, head-sharing workgroups, both kernels."""
    monkeypatch.setenv("CQS_HIP_ATT_LAYOUT", "shared")
    monkeypatch.setenv("CQS_HIP_ATT_KERNEL", kernel)
    cfg = G.GemmaConfig(vocab_size=512, hidden=256, layers=2, heads=3, kv_heads=1, head_dim=256, intermediate=256,
                        dense_hidden=256, sliding_window=512, sliding_pattern=2, max_seq=1024)
    eng, w = make(cfg, seed=43)
    ids, mask = batch(cfg, [1024, 700, 512, 258, 257, 256, 321, 40], seed=44)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    for i in range(len(ids)):
        assert cos(got[i], ref[i]) > 0.999, (kernel, i, cos(got[i], ref[i]))
    eng.close()


def test_full_depth_full_geometry(hip):
    """All 24 layers at the real EmbeddingGemma-300m geometry (768 | 3 x 256 q, 1 kv | 1152 | dense 3072; window
    512, every 6th layer full attention) with a small vocabulary: bf16 operand error accumulated over the whole
    depth stays within cosine 0.999 of the fp32 oracle on the sentence embedding."""
    cfg = G.GemmaConfig(vocab_size=2048, hidden=768, layers=24, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                        dense_hidden=3072, sliding_window=512, sliding_pattern=6, max_seq=2048)
    eng, w = make(cfg, seed=51)
    ids, mask = batch(cfg, [300, 17, 130, 64], seed=52)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    cs = [cos(got[i], ref[i]) for i in range(len(ids))]
    print("cosines", cs)
    assert min(cs) > 0.999, cs
    eng.close()


def test_default_config_real_vocabulary(hip):
    """`cqs_hip_embed_config_default` as it ships - the 262 144-row token table (403 MB in bf16: the gather reaches rows
    far apart), 24 layers, max_seq 2048 - on a small ragged batch that includes the highest token ids, against the fp32
    oracle.  (bench.py's e2e leg checks the same configuration on hundreds of chunks; this is the unit-test twin.)"""
    cfg = G.GemmaConfig()
    assert cfg.vocab_size == 262144 and cfg.layers == 24
    eng, w = make(cfg, seed=53)
    ids, mask = batch(cfg, [70, 9, 257], seed=54)
    ids[0, :4] = [262143, 262142, 1, 131072]
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    cs = [cos(got[i], ref[i]) for i in range(len(ids))]
    assert min(cs) > 0.999, cs
    eng.close()


@pytest.mark.parametrize("tile", ["small", "pp:3", "pp:4", "pp:5"])
def test_gemm_tile_kernels(hip, tile, monkeypatch):
    """The forward has two GEMM kernels (128 x 128 tiles; the 256 x {192, 256, 320} ping-pong kernel where it fills whole
    rounds of CUs).  Small test batches never pick the big tiles by themselves: force each and compare with the
    fp32 oracle at hidden = 768 (ragged M: the last 256-row tile is partly empty)."""
    monkeypatch.setenv("CQS_HIP_GEMM_TILE", tile)
    cfg = G.GemmaConfig(vocab_size=1024, hidden=768, layers=4, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                        dense_hidden=768, sliding_window=128, sliding_pattern=2, max_seq=512)
    eng, w = make(cfg, seed=61)
    ids, mask = batch(cfg, [257, 300, 31, 200], seed=62)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    for i in range(len(ids)):
        assert cos(got[i], ref[i]) > 0.999, (tile, i, cos(got[i], ref[i]))
    hid = eng.run_hidden(ids, mask)
    href = G.forward(cfg, w, ids, mask, return_hidden=True)
    live = mask.astype(bool)
    err = np.abs(hid[live] - href[live])
    assert err.mean() / np.abs(href[live]).mean() < 0.02
    eng.close()


@pytest.mark.parametrize("tile", ["small", "pp:3", "pp:4", "pp:5"])
def test_gemm_kernels_exact_integer_data(hip, tile, monkeypatch):
    """Each GEMM kernel alone against torch on small-integer bf16 operands (every product and partial sum is exact in
    f32, so the comparison is bit-exact and a transposed / permuted fragment cannot hide): asymmetric operands,
    ragged M, the three epilogues, K from one K-tile (64) up to 1152."""
    import ctypes as C
    import torch
    monkeypatch.setenv("CQS_HIP_GEMM_TILE", tile)
    f = _lib.load().cqs_hip_debug_gemm_run
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_int32, C.c_void_p]
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    shapes = [(256, 768, 64), (1, 768, 128), (300, 1280, 768), (1000, 2304, 768), (513, 768, 1152), (2048, 3840, 192), (255, 3840, 320)]
    for M, N, K in shapes:
        A = torch.randint(-4, 5, (M, K), generator=g, device="cuda").to(torch.bfloat16)
        W = torch.randint(-3, 4, (N, K), generator=g, device="cuda").to(torch.bfloat16)
        ref = A.float() @ W.float().T                                      # exact: |sum| < 2^24
        for kind in (0, 1, 2):
            if kind == 2:
                out = torch.full((M, N // 2), 7.0, device="cuda", dtype=torch.bfloat16)
                ldc = N // 2
            else:
                out = torch.full((M, N), 7.0, device="cuda", dtype=torch.float32 if kind == 1 else torch.bfloat16)
                ldc = N
            assert f(A.data_ptr(), W.data_ptr(), out.data_ptr(), M, N, K, ldc, kind, None) == 0
            torch.cuda.synchronize()
            if kind == 1:
                assert torch.equal(out, ref), (tile, M, N, K, float((out - ref).abs().max()))
            elif kind == 0:
                assert torch.equal(out, ref.to(torch.bfloat16)), (tile, M, N, K)
            else:
                r = ref.view(M, N // 64, 2, 32)                             # per 64 columns: 32 gate | 32 up
                want = (torch.nn.functional.gelu(r[:, :, 0], approximate="tanh") * r[:, :, 1]).reshape(M, N // 2)
                err = (out.float() - want).abs().max().item()
                assert err <= 0.02 * want.abs().max().item() + 1e-3, (tile, M, N, K, err)


@pytest.mark.parametrize("dual", ["dual", "two-launches"])
def test_gemm_planner_choices_at_full_batch_shapes(hip, dual, monkeypatch):
    """The planner's own picks (nothing forced) at the shapes of a 16 384-token batch - whole rounds of one tile width +
    the rest with another, both parts in ONE launch (`gemm_pp_dual_kernel`) or, with CQS_HIP_GEMM_NO_DUAL, in two -
    bit-exact against torch on small-integer operands; ragged M too (the planner then mixes in the 128 x 128 kernel)."""
    import ctypes as C
    import torch
    if dual != "dual":
        monkeypatch.setenv("CQS_HIP_GEMM_NO_DUAL", "1")
    f = _lib.load().cqs_hip_debug_gemm_run
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_int32, C.c_void_p]
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    for M, N, K, kind in [(16384, 2304, 768, 2), (16384, 1280, 768, 0), (16384, 768, 1152, 0), (16384, 2304, 768, 0),
                          (16000, 2304, 768, 2), (8192, 2304, 768, 2), (24576, 1280, 768, 0),
                          # a few rows x a big matrix (the Dense head: M = sequences of the batch): the skinny kernel
                          # (kind + 0x100; beyond 256 rows it hands over to the tiled kernels)
                          (32, 3072, 768, 0x100), (1, 768, 3072, 0x101), (100, 3072, 768, 0x100), (256, 768, 3072, 0x101),
                          (17, 768, 64, 0x100), (300, 768, 3072, 0x101)]:
        A = torch.randint(-4, 5, (M, K), generator=g, device="cuda").to(torch.bfloat16)
        W = torch.randint(-3, 4, (N, K), generator=g, device="cuda").to(torch.bfloat16)
        ref = A.float() @ W.float().T
        ldc = N // 2 if kind == 2 else N
        out = torch.full((M, ldc), 7.0, device="cuda", dtype=torch.float32 if (kind & 0xff) == 1 else torch.bfloat16)
        assert f(A.data_ptr(), W.data_ptr(), out.data_ptr(), M, N, K, ldc, kind, None) == 0
        torch.cuda.synchronize()
        if (kind & 0xff) == 1:
            assert torch.equal(out, ref), (dual, M, N, K)
        elif (kind & 0xff) == 0:
            assert torch.equal(out, ref.to(torch.bfloat16)), (dual, M, N, K)
        else:
            r = ref.view(M, N // 64, 2, 32)
            want = (torch.nn.functional.gelu(r[:, :, 0], approximate="tanh") * r[:, :, 1]).reshape(M, N // 2)
            err = (out.float() - want).abs().max().item()
            assert err <= 0.02 * want.abs().max().item() + 1e-3, (dual, M, N, K, err)


def test_fewrows_gemm_is_bit_identical_to_the_tiled_kernel(hip, monkeypatch):
    """Small batches run `gemm_fewrows_kernel` (one wave per 32 x 32 tile, no LDS); it must agree BIT FOR BIT with the
    128 x 128 kernel on arbitrary data (same MFMA, operand roles and K order), or a chunk's embedding would depend on
    how many tokens share its batch."""
    import ctypes as C
    import torch
    f = _lib.load().cqs_hip_debug_gemm_run
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_int32, C.c_void_p]
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    for M, N, K in [(1, 1280, 768), (9, 768, 768), (33, 2304, 768), (64, 768, 1152), (100, 1280, 768), (512, 2304, 768), (300, 768, 64)]:
        A = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
        W = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(torch.bfloat16)
        for kind in (0, 1, 2):
            ldc = N // 2 if kind == 2 else N
            dt = torch.float32 if kind == 1 else torch.bfloat16
            a = torch.zeros(M, ldc, device="cuda", dtype=dt)
            b = torch.zeros(M, ldc, device="cuda", dtype=dt)
            monkeypatch.delenv("CQS_HIP_GEMM_TILE", raising=False)
            assert f(A.data_ptr(), W.data_ptr(), a.data_ptr(), M, N, K, ldc, kind, None) == 0      # few-rows kernel
            monkeypatch.setenv("CQS_HIP_GEMM_TILE", "small")
            assert f(A.data_ptr(), W.data_ptr(), b.data_ptr(), M, N, K, ldc, kind, None) == 0      # 128 x 128 kernel
            torch.cuda.synchronize()
            assert torch.equal(a, b), (M, N, K, kind, float((a.float() - b.float()).abs().max()))
            if kind == 1:
                ref = A.float() @ W.float().T
                assert float((a - ref).abs().max()) < 2e-2


def set_fuse_norm(eng, on, min_rows=0):
    """The engine reads CQS_HIP_GEMM_FUSE_NORM* once, at finalize; tests switch the fused kernels through the debug hook."""
    import ctypes as C
    f = eng._lib.cqs_hip_debug_embedder_set_fuse_norm
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
    f(eng._h, int(on), min_rows)                # 0 = two launches, 1 = round 3's 64-row kernel, 2 = the pair-split kernel


def test_fused_projection_addnorm_is_bit_identical_to_the_two_launch_chain(hip):
    """gemm_rowfuse.hip: o_proj / down + residual add + both RMSNorms in one launch.  Round 4's kernel gives 128 token rows
    to a PAIR of workgroups, each computing one 384-column half; the partners exchange their halves of every row's sum of
    squares inside the launch (twice).  Same MFMA and k order as the 256-row GEMM, and the row sums are taken half by
    half, left + right - the order add_norm_kernel uses too - so the embeddings must equal the two-launch chain's BIT FOR
    BIT: ragged token counts (last row block partly filled, odd pair counts, a tail group of fewer than 8 pairs), both the
    xn and the final-norm output forms (4 layers: the last `down` runs FINAL), twice in a row on the same engine (the
    granules' launch tags must tell a fresh value from the previous launch's).  Also against the fp32 oracle."""
    cfg = G.GemmaConfig(vocab_size=4096, hidden=768, layers=4, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                        dense_hidden=3072, sliding_window=512, sliding_pattern=2, max_seq=2048)
    eng, w = make(cfg, seed=41)
    for lens in ([700, 650, 33, 517], [64] * 20, [1000, 3], [128], [129], [2047, 2048, 1, 300]):   # 1900, 1280, 1003, 128, 129, 4396 tokens
        ids, mask = batch(cfg, lens, seed=sum(lens))
        set_fuse_norm(eng, 0)
        plain = eng.run(ids, mask)
        set_fuse_norm(eng, 2, 64)                                        # (default threshold: the test batches are smaller)
        fused = eng.run(ids, mask)
        assert np.array_equal(fused, plain), (lens, float(np.max(np.abs(fused - plain))))
        assert np.array_equal(eng.run(ids, mask), plain), lens            # again: stale granules of the launch before
        t = [eng.submit(ids, mask) for _ in range(3)]                     # both execution contexts, three tickets in flight
        for tk in t:
            assert np.array_equal(eng.collect(tk, len(lens)), plain), lens
    ids, mask = batch(cfg, [300, 41], seed=5)
    got = eng.run(ids, mask)
    ref = G.forward(cfg, w, ids, mask)
    for i in range(2):
        assert cos(got[i], ref[i]) > 0.999
    # round 3's 64-row kernel (kept for A/B): its row sums run over whole rows, so it agrees to rounding, not bit for bit
    set_fuse_norm(eng, 1, 64)
    old = eng.run(ids, mask)
    set_fuse_norm(eng, 0)
    plain = eng.run(ids, mask)
    for i in range(2):
        assert cos(old[i], plain[i]) > 0.99999
    eng.close()


def test_a_pair_exchange_timeout_falls_back_instead_of_poisoning(hip):
    """the pair-split projection kernel makes workgroup b wait (bounded) for granules of workgroup b ^ 8 of the
    same launch; a timeout used to leave garbage rows and poison the engine at collect.  Now the engine drops to the
    two-launch chain (same bits, no cross-workgroup exchange) and recomputes every batch-chain ticket that was in flight:
    three tickets in flight, the timeout word set by the debug hook, every collect returns the rows of an undisturbed run,
    the engine stays usable and has fallen back exactly once."""
    import ctypes as C
    cfg = G.GemmaConfig(vocab_size=4096, hidden=768, layers=4, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                        dense_hidden=3072, sliding_window=512, sliding_pattern=2, max_seq=2048)
    eng, _w = make(cfg, seed=45)
    fake = eng._lib.cqs_hip_debug_embedder_fake_fuse_timeout
    fake.restype = None
    fake.argtypes = [C.c_void_p]
    nfb = eng._lib.cqs_hip_debug_embedder_fuse_fallbacks
    nfb.restype = C.c_uint32
    nfb.argtypes = [C.c_void_p]
    set_fuse_norm(eng, 2, 64)
    batches = [batch(cfg, lens, seed=sum(lens)) for lens in ([700, 650, 33, 517], [300] * 6, [1000, 3])]
    want = [eng.run(i, m) for i, m in batches]
    assert nfb(eng._h) == 0
    t = [eng.submit(i, m) for i, m in batches]
    fake(eng._h)
    for tk, w_, (i, _m) in zip(t, want, batches):
        assert np.array_equal(eng.collect(tk, i.shape[0]), w_)
    assert nfb(eng._h) == 1 and eng._lib.cqs_hip_embedder_poisoned(eng._h) == 0
    for (i, m), w_ in zip(batches, want):                      # the engine keeps serving, now on the two-launch chain
        assert np.array_equal(eng.run(i, m), w_)
    assert nfb(eng._h) == 1
    eng.close()


def set_fuse_qkv(eng, on):
    import ctypes as C
    f = eng._lib.cqs_hip_debug_embedder_set_fuse_qkv
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int32]
    f(eng._h, 1 if on else 0)


def test_fused_qkv_epilogue_matches_the_three_launch_chain_and_the_oracle(hip, monkeypatch):
    """Round 4: the QKV projection's 256 x 320 tiles each hold one whole q / k head + a 64-column slice of v (weights in tile
    order), and the GEMM's epilogue applies the head's RMSNorm (1 + w), RoPE and the q scale itself - `kv_prep_kernel` and
    the attention kernel's own Q norm disappear (5 launches per layer).  Same formulas on the same bf16-rounded projection;
    only the order in which a head's 256 squares are summed differs, so the embeddings agree to rounding (cosine >= 0.99999),
    not bit for bit - and the path must really be a different one (not equal bitwise).  The planner takes the fused kernel
    by itself only where 256 x 320 tiles make full rounds (32 x 512 tokens); CQS_HIP_GEMM_TILE=pp:5 forces it on a batch small
    enough for the fp32 oracle.  Full and sliding-window layers, ragged lengths, a partly filled last row tile."""
    cfg = G.GemmaConfig(vocab_size=4096, hidden=768, layers=4, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                        dense_hidden=3072, sliding_window=512, sliding_pattern=2, max_seq=2048)
    eng, w = make(cfg, seed=43)
    lens = [512, 400, 300, 200, 150, 128, 100, 64, 33, 1, 700]
    ids, mask = batch(cfg, lens, seed=77)
    monkeypatch.setenv("CQS_HIP_GEMM_TILE", "pp:5")
    set_fuse_qkv(eng, False)
    plain = eng.run(ids, mask)
    set_fuse_qkv(eng, True)
    fused = eng.run(ids, mask)
    assert not np.array_equal(fused, plain), "the fused epilogue did not run (bitwise equal to the three-launch chain)"
    ref = G.forward(cfg, w, ids, mask)
    for i in range(len(lens)):
        assert cos(fused[i], plain[i]) > 0.99999, (i, cos(fused[i], plain[i]))
        assert np.max(np.abs(fused[i] - plain[i])) < 2e-2 * np.abs(plain[i]).max(), i
        assert cos(fused[i], ref[i]) > 0.999, (i, cos(fused[i], ref[i]))
    # 256 x 256 tiles (partly filled rounds: ragged batches of up to ~13k tokens): a tile = one head, or 256 columns of v
    monkeypatch.setenv("CQS_HIP_GEMM_TILE", "pp:4")
    fused4 = eng.run(ids, mask)
    set_fuse_qkv(eng, False)
    plain4 = eng.run(ids, mask)
    set_fuse_qkv(eng, True)
    assert not np.array_equal(fused4, plain4)
    for i in range(len(lens)):
        assert cos(fused4[i], plain4[i]) > 0.99999 and cos(fused4[i], ref[i]) > 0.999, i
    monkeypatch.delenv("CQS_HIP_GEMM_TILE")
    ids, mask = batch(cfg, [512] * 32, seed=78)             # the planner's own choice: one full round of 256 x 320 tiles
    set_fuse_qkv(eng, False)
    plain = eng.run(ids, mask)
    set_fuse_qkv(eng, True)
    fused = eng.run(ids, mask)
    assert not np.array_equal(fused, plain)
    for i in range(32):
        assert cos(fused[i], plain[i]) > 0.99999, (i, cos(fused[i], plain[i]))
    eng.close()


def test_geglu_in_register_pairing_matches_the_f32_stage(hip, monkeypatch):
    """Round 4: the 256-row GEMM kernel's GeGLU epilogue reads gate / up rows interleaved per 4 and pairs them in registers
    (`v_permlane16_swap`), gelu on the accumulators (packed f32 arithmetic, the sigmoid form of the tanh approximation),
    bf16 stage - instead of staging f32 pairs through LDS.  Same accumulators; the gelu's last bits differ (with the scalar
    formula - build flag P8_GEGLU4_SCALAR_GELU - the two epilogues were bit-identical: that is how the pairing was checked),
    so the embeddings agree to rounding: cosine >= 0.99999, max |d| tiny.  32 x 512 tokens (the dual launch of 256 x 320 and
    256 x 256 tiles), a ragged batch (other tile plans, a partly filled row tile) and forced tile widths."""
    import ctypes as C
    cfg = G.GemmaConfig(vocab_size=4096, hidden=768, layers=2, heads=3, kv_heads=1, head_dim=256, intermediate=1152,
                        dense_hidden=3072, sliding_window=512, sliding_pattern=2, max_seq=2048)
    eng, w = make(cfg, seed=47)
    f = eng._lib.cqs_hip_debug_embedder_set_geglu4
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int32]
    for lens, tile in (([512] * 32, None), ([700, 650, 33, 517, 2048, 1900, 1000], None), ([400, 300, 277], "pp:3"), ([400, 300, 277], "pp:4")):
        if tile:
            monkeypatch.setenv("CQS_HIP_GEMM_TILE", tile)
        ids, mask = batch(cfg, lens, seed=sum(lens))
        f(eng._h, 0)
        old = eng.run(ids, mask)
        f(eng._h, 1)
        new = eng.run(ids, mask)
        for i in range(len(lens)):
            assert cos(old[i], new[i]) > 0.99999, (lens, tile, i, cos(old[i], new[i]))
        assert np.max(np.abs(old - new)) < 1e-2 * np.abs(old).max(), (lens, tile, float(np.max(np.abs(old - new))))
        if tile:
            monkeypatch.delenv("CQS_HIP_GEMM_TILE")
    eng.close()
