"""The batch tables of both transformer engines (cqs_amd/csrc/batch_tables.h) on the device: one engine runs a sequence of
batches whose (B, M, nblk) change, so its pinned slots and its contexts' device blocks are re-carved again and again, and
every result must be byte-equal to the same batch on a freshly made engine with the same weights (same shapes, same kernel
choices, no kernel is non-deterministic; test_padding_and_batch_invariance asserts run-to-run equality of the same kind).
What a misplaced table would break and the existing suite does not pin directly.  Empty rows are exact zeros."""
import numpy as np
import pytest

from oracle import bert_ref as R
from test_bert_gpu import _engine as bert_engine, _seqs
from test_embed_gpu import SMALL, batch, make

pytestmark = pytest.mark.gpu


def test_gemma_tables_recarved_on_reused_slots_and_contexts(hip):
    """Lengths with a block edge on either side (127 / 128 / 129 / 130 / 200 of 128-row blocks) and empty rows; only the
    [130] step has B = 1, and 130 is past the search-time chain's length, so every batch takes the batch chain.  Each step
    is followed by run_hidden of the same batch (the diagnostic twin packs into a slot of its own and runs on context 0)."""
    steps = [[200, 0, 129], [130], [127, 128, 129, 0, 1], [200, 0, 129]]
    batches = [batch(SMALL, lens, seed=40 + i) for i, lens in enumerate(steps[:3])]
    batches.append(batches[0])

    def fresh(ids, mask):
        eng, _ = make(SMALL, seed=9)
        out = eng.run(ids, mask), eng.run_hidden(ids, mask)
        eng.close()
        return out

    want = [fresh(*b) for b in batches[:3]]
    want.append(want[0])
    eng, _ = make(SMALL, seed=9)
    for lens, (ids, mask), (emb, hid) in zip(steps, batches, want):
        got, got_hid = eng.run(ids, mask), eng.run_hidden(ids, mask)
        assert np.array_equal(got, emb), lens
        assert np.array_equal(got_hid, hid), lens
        for b, n in enumerate(lens):
            assert np.all(got_hid[b, n:] == 0), (lens, b)
            if n == 0:
                assert np.all(got[b] == 0), (lens, b)
            else:
                assert np.any(got[b] != 0) and np.any(got_hid[b, :n] != 0), (lens, b)
    eng.close()


def _bert_run(eng, head, s, t):
    """Every entry point of the head, as a list of arrays; the first `_ZERO_ROWS[head]` of them have one row per sequence."""
    if head == "mlm":
        ids, wts, cnt = eng.splade_sparse(s, 0.01, cap=64)
        kept = [np.concatenate([a[b, :min(int(c), 64)] for b, c in enumerate(cnt)]) for a in (ids, wts)]   # (past a row's count: unwritten)
        return [eng.splade_dense(s), cnt, *kept]
    if head == "none":
        return [eng.embed(s, t, "mean"), eng.embed(s, t, "cls"), eng.hidden(s, t)]
    live = [i for i, q in enumerate(s) if len(q)]
    return [eng.hidden(s, t), eng.rerank_logits([s[i] for i in live], [t[i] for i in live])]


_ZERO_ROWS = {"mlm": 2, "none": 2, "classifier": 0}


def test_bert_tables_recarved_on_reused_slots_and_contexts(hip):
    """Lengths with a block edge on either side (63 / 64 / 65 / 130 of 64-row blocks; [64] also takes the fused small-batch
    chain) and empty rows, for every head; type ids are present for the heads that take them.  The reranker refuses an empty
    sequence, so the classifier engine runs the diagnostic hidden states on the whole batch and its logits on the non-empty rows."""
    cfg = R.BertConfig(vocab_size=400, hidden=256, layers=1, heads=4, intermediate=256, max_pos=512)
    steps = [[63, 0, 65], [64], [1, 0, 130, 64, 0], [63, 0, 65]]
    seqs = [_seqs(cfg, lens, seed=70 + i) for i, lens in enumerate(steps[:3])]
    seqs.append(seqs[0])
    types = [[np.r_[np.zeros(n // 2, np.int32), np.ones(n - n // 2, np.int32)].astype(np.int32) for n in lens] for lens in steps]
    for head in ("mlm", "none", "classifier"):
        want = []
        for s, t in zip(seqs[:3], types[:3]):
            eng, _ = bert_engine(cfg, head, seed=11)
            want.append(_bert_run(eng, head, s, t))
            eng.close()
        want.append(want[0])
        eng, _ = bert_engine(cfg, head, seed=11)
        for lens, s, t, ref in zip(steps, seqs, types, want):
            got = _bert_run(eng, head, s, t)
            assert len(got) == len(ref)
            for g, r in zip(got, ref):
                assert np.array_equal(g, r), (head, lens)
            for g in got[:_ZERO_ROWS[head]]:                               # activations + counts / both poolings: zero rows when empty
                for b, n in enumerate(lens):
                    assert np.any(g[b] != 0) == (n != 0), (head, lens, b)
        eng.close()
