"""The two packed int32 table layouts of the transformer engines and the ticket-context rule, restated in numpy from their
description (DESIGN.md "Batch tables and the context rule"), not from cqs_amd/csrc/batch_tables.h:

  Gemma kind: [tok M][pos M][seq_start B][seq_len B][vt_start B][blk 2 nblk]          attention blocks of 128 rows
  BERT kind:  [tok M][pos M][tt M][seq_start B][seq_len B][blk 2 nblk][row_seq M]     attention blocks of 64 rows

tests/test_batch_tables_cpu.py compares the header's output with these word by word."""
import numpy as np

GEMMA, BERT = 0, 1
BLOCK = {GEMMA: 128, BERT: 64}
OK, TOO_LONG, TOO_MANY_TOKENS, BAD_TOKEN, BAD_TYPE, MASK_NOT_PREFIX = range(6)


def expected_shape(kind, lens):
    """(B, M, nblk, vt_cols, words)"""
    lens = np.asarray(lens, np.int64)
    B, M = len(lens), int(lens.sum())
    nblk = int(np.sum(-(-lens // BLOCK[kind])))
    vt_cols = int(np.sum(-(-lens // 32) * 32)) + 32 if kind == GEMMA else 0
    words = 2 * M + 3 * B + 2 * nblk if kind == GEMMA else 4 * M + 2 * B + 2 * nblk
    return B, M, nblk, vt_cols, words


def expected_block(kind, lens, tok, ty=None):
    lens = np.asarray(lens, np.int64)
    B = len(lens)
    seq_start = np.concatenate([[0], np.cumsum(lens)[:-1]]) if B else np.zeros(0, np.int64)
    pos = np.concatenate([np.arange(n) for n in lens] + [np.zeros(0, np.int64)])
    row_seq = np.repeat(np.arange(B), lens)
    blk = np.array([(b, q) for b, n in enumerate(lens) for q in range(-(-int(n) // BLOCK[kind]))], np.int64).reshape(-1)
    if kind == GEMMA:
        padded = -(-lens // 32) * 32
        vt_start = np.concatenate([[0], np.cumsum(padded)[:-1]])
        parts = [tok, pos, seq_start, lens, vt_start, blk]
    else:
        parts = [tok, pos, ty, seq_start, lens, blk, row_seq]
    return np.concatenate([np.asarray(p, np.int64) for p in parts]).astype(np.int64)


def expected_context(load0, load1, last_ctx):
    """The context with fewer tickets in flight; a tie goes to the one the previous ticket did not take; idle engine: 0."""
    if load0 != load1:
        return 0 if load0 < load1 else 1
    return 0 if load0 == 0 else 1 - last_ctx


def expected_exact_rounds(M, n_cu):
    """Two workgroups per 128 token rows; at least one round of the CUs, and the last round full or within 1/32 of full."""
    wgs = -(-M // 128) * 2
    last = wgs % n_cu
    return wgs >= n_cu and (last == 0 or last * 32 >= n_cu * 31)


def layout_batches(kind, seed=0xBA7C4):
    """The batches of the layout cases: lists of lengths."""
    blk = BLOCK[kind]
    edge = [1, blk - 1, blk, blk + 1, 2 * blk + 1]
    out = [[n] for n in edge] + [edge]                                       # B = 1 and B = 5
    out += [[0, 7, 40], [7, 0, 40], [7, 40, 0], [0], [0, 0, 0, 0, 0]]        # an empty sequence first / middle / last; all empty
    out += [[32, 64, 96], [31, 33, 1, 95], [32, 5, 64]]                       # multiples of 32 and not (vt_start)
    rng = np.random.default_rng(seed + kind)
    for _ in range(300):
        out.append([int(n) for n in rng.integers(0, 301, size=int(rng.integers(1, 13)))])
    return out
