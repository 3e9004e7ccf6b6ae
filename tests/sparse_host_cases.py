"""Case helpers shared by the sparse index's host tests (test_sparse_build_host_cpu.py, test_sparse_update_host_cpu.py) and
its GPU tests (test_sparse_index_gpu.py): seeded documents, the from-scratch build of what cqs_hip_sparse_index_create
builds, and a writer of the library's sparse-index file format, both restated in Python."""
import numpy as np


def _docs(rng, n, vocab, lo=0, hi=6, base=100, step=3):
    """n documents of lo..hi postings over token ids base, base + step, ...; about a third repeat one of their tokens."""
    docs = []
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        t = np.sort(rng.integers(0, vocab, size=k)) * step + base
        if k >= 2 and rng.random() < 0.35:
            t[1] = t[0]
        w = (rng.random(k, dtype=np.float32) * 3 - 1).astype(np.float32).view(np.uint32)
        docs.append([(int(a), int(b)) for a, b in zip(t, w)])
    return docs


def _ranks(rng, n):
    return [int(x) for x in rng.permutation(n)]


def canonical(docs, id_rank):
    """What cqs_hip_sparse_index_create builds: (n, tokens, offsets, postings [(position, weight bits)], chunk_of_rank)."""
    n = len(docs)
    cor = list(np.argsort(np.asarray(id_rank, dtype=np.int64))) if id_rank is not None else list(range(n))
    lists = {}
    for r in range(n):
        for t, w in docs[cor[r]]:
            lists.setdefault(t, []).append((r, w))
    tok = sorted(lists)
    off, post = [0], []
    for t in tok:
        post += lists[t]
        off.append(len(post))
    return n, tok, off, post, ([int(c) for c in cor] if id_rank is not None else [])


def _csr(docs):
    off = [0]
    for d in docs:
        off.append(off[-1] + len(d))
    return off, [t for d in docs for t, _ in d], [w for d in docs for _, w in d]


def _forge_sparse_file(path, chunks, tok, off, post, rank=None, generation=1, fix_checksum=True):
    """A file in the library's sparse-index format with a VALID checksum (the multiply-rotate hash of persist_util.h restated
    here), whatever its sections hold - to reach the loader's structure checks behind the checksum."""
    import struct
    M = (1 << 64) - 1
    P1, P2 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F

    def pad8(b):
        return b + b"\0" * (-len(b) % 8)

    secs = [pad8(np.asarray(tok, np.uint32).tobytes()), pad8(np.asarray(off, np.uint64).tobytes()),
            pad8(np.asarray(post, np.uint32).reshape(-1, 2).tobytes() if len(post) else b""),
            pad8(np.asarray(rank, np.uint32).tobytes()) if rank is not None else b""]
    body = b"".join(secs)
    h = 0x27D4EB2F165667C5 ^ len(body)
    for (w,) in struct.iter_unpack("<Q", body):
        h ^= (w * P1) & M
        h = ((((h << 31) | (h >> 33)) & M) * P2) & M
    h ^= h >> 29; h = (h * P2) & M; h ^= h >> 32
    if not fix_checksum:
        h ^= 1
    header = struct.pack("<8sIIQQQQQ8s", b"CQSHIPS1", 1, 1 if rank is not None else 0, chunks, len(tok), len(post), generation, h, b"\0" * 8)
    assert len(header) == 64
    open(path, "wb").write(header + body)
