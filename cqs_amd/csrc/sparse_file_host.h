// sparse_file_host.h — the sparse index's file (the role of `SpladeIndex::save` / `load`, src/splade/index.rs:346-1072: skip
// the rebuild after a restart; invalidated by the store's `splade_generation` counter).  Own format - the reference's file
// is not read or written: 64-byte header {magic "CQSHIPS1", version, ranked, chunks, tokens, postings, generation,
// checksum} + four sections, each zero-padded to 8 bytes: token ids (u32, ascending), list offsets (u64, tokens + 1),
// postings ({position, weight bits}, 8 B each), and - ranked indexes only - chunk_of_rank (u32 per chunk).  The checksum
// covers the sections.
//
// Plain C++ over POSIX file descriptors, no HIP, no handle.  The reader is the library's one parser of untrusted bytes - the
// kernels index LDS by the positions it lets through - and tests/sparse_build_host_driver.cpp runs it under ASAN + UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "persist_util.h"
#include "sparse_build_host.h"

namespace cqs_sparse_file {

using cqs_sparse_build::Posting;

struct SparseFileHeader {
    char magic[8];
    uint32_t version, ranked;
    uint64_t chunks, tokens, postings, generation, checksum;
    uint8_t reserved[8];
};
static_assert(sizeof(SparseFileHeader) == 64, "header is 64 bytes");
const char kSparseMagic[8] = {'C', 'Q', 'S', 'H', 'I', 'P', 'S', '1'};
inline size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

struct Layout {
    size_t bytes[4];     // token ids, list offsets, postings, chunk_of_rank - before padding
    size_t total;        // the four sections, padded
};

inline Layout layout(const SparseFileHeader& h) {
    Layout l{{(size_t)h.tokens * 4, ((size_t)h.tokens + 1) * 8, (size_t)h.postings * 8, h.ranked ? (size_t)h.chunks * 4 : 0}, 0};
    for (const size_t b : l.bytes) l.total += pad8(b);
    return l;
}

inline SparseFileHeader make_header(bool ranked, uint64_t chunks, uint64_t tokens, uint64_t postings, uint64_t generation) {
    SparseFileHeader h{};
    memcpy(h.magic, kSparseMagic, 8);
    h.version = 1;
    h.ranked = ranked ? 1u : 0u;
    h.chunks = chunks; h.tokens = tokens; h.postings = postings; h.generation = generation;
    return h;
}

// A header read from a file of file_size bytes: ours, of this generation and chunk count (0 = any), of sizes the library
// builds, and exactly as long as it says.
inline bool check_header(const SparseFileHeader& h, uint64_t file_size, uint64_t expected_chunks, uint64_t generation) {
    if (memcmp(h.magic, kSparseMagic, 8) != 0 || h.version != 1 || h.ranked > 1) return false;
    if (h.generation != generation) return false;         // the store changed since the file was written (index.rs:1011-1019)
    if (expected_chunks && h.chunks != expected_chunks) return false;
    if (h.chunks >= cqs::kSparseMaxChunks || h.tokens > 0xFFFFFFFFull || h.postings > (1ull << 40)) return false;
    return file_size == sizeof h + layout(h).total;       // truncated or grown
}

// Header and sections to fd (at its start); h.checksum and *checksum = the sections' checksum.  sections[i] holds
// layout(h).bytes[i] bytes.
inline bool write_file(int fd, SparseFileHeader& h, const void* const sections[4], uint64_t* checksum) {
    const Layout l = layout(h);
    cqs_persist::Checksum ck(l.total);
    bool ok = cqs_persist::write_all(fd, &h, sizeof h);           // checksum patched in below
    const uint64_t zero = 0;
    for (int i = 0; i < 4 && ok; ++i) {
        const size_t bytes = l.bytes[i], padded = pad8(bytes);
        if (padded == bytes) {
            ck.update(sections[i], bytes, false);
            ok = cqs_persist::write_all(fd, sections[i], bytes);
        } else {                                                  // (only a u32 section of odd length: copy its last word)
            const size_t whole = bytes & ~(size_t)7;
            ck.update(sections[i], whole, false);
            uint64_t tail = 0;
            memcpy(&tail, (const uint8_t*)sections[i] + whole, bytes - whole);
            ck.update(&tail, 8, false);
            ok = cqs_persist::write_all(fd, sections[i], bytes) && cqs_persist::write_all(fd, &zero, padded - bytes);
        }
    }
    ck.update(nullptr, 0, true);
    h.checksum = ck.finish();
    if (checksum) *checksum = h.checksum;
    return ok && lseek(fd, 0, SEEK_SET) == 0 && cqs_persist::write_all(fd, &h, sizeof h);
}

// The four sections behind a header that passed check_header (fd stands behind the header).  false: short read, or the
// bytes do not have the header's checksum (corrupt body, index.rs:1035-1049).
inline bool read_sections(int fd, const SparseFileHeader& h, std::vector<uint32_t>* tok, std::vector<uint64_t>* off, std::vector<Posting>* post,
                          std::vector<uint32_t>* chunk_of_rank) {
    const Layout l = layout(h);
    std::vector<uint64_t> tokbuf(pad8(l.bytes[0]) / 8), rankbuf(pad8(l.bytes[3]) / 8);
    off->resize((size_t)h.tokens + 1);
    post->resize((size_t)h.postings);
    if (!cqs_persist::read_all(fd, tokbuf.data(), tokbuf.size() * 8) || !cqs_persist::read_all(fd, off->data(), l.bytes[1]) ||
        !cqs_persist::read_all(fd, post->data(), l.bytes[2]) || !cqs_persist::read_all(fd, rankbuf.data(), rankbuf.size() * 8))
        return false;
    cqs_persist::Checksum ck(l.total);
    ck.update(tokbuf.data(), tokbuf.size() * 8, false);
    ck.update(off->data(), l.bytes[1], false);
    ck.update(post->data(), l.bytes[2], false);
    ck.update(rankbuf.data(), rankbuf.size() * 8, false);
    ck.update(nullptr, 0, true);
    if (ck.finish() != h.checksum) return false;
    tok->resize((size_t)h.tokens);
    if (l.bytes[0]) memcpy(tok->data(), tokbuf.data(), l.bytes[0]);
    chunk_of_rank->resize(l.bytes[3] / 4);
    if (l.bytes[3]) memcpy(chunk_of_rank->data(), rankbuf.data(), l.bytes[3]);
    return true;
}

// What the kernels rely on: ascending distinct tokens, offsets that tile the postings, positions inside the index and
// ascending inside every list, no reserved weight pattern, a permutation for the id order.
inline bool check_structure(const SparseFileHeader& h, const std::vector<uint32_t>& tok, const std::vector<uint64_t>& off,
                            const std::vector<Posting>& post, const std::vector<uint32_t>& chunk_of_rank) {
    for (size_t t = 1; t < tok.size(); ++t)
        if (tok[t] <= tok[t - 1]) return false;
    if (off[0] != 0 || off[(size_t)h.tokens] != h.postings) return false;
    for (size_t t = 0; t < (size_t)h.tokens; ++t) {
        if (off[t + 1] < off[t] || off[t + 1] > h.postings) return false;
        for (uint64_t e = off[t]; e < off[t + 1]; ++e)
            if (post[e].x >= h.chunks || (e > off[t] && post[e].x < post[e - 1].x) || post[e].y == cqs::kUnscored) return false;
    }
    if (h.ranked) {
        std::vector<uint8_t> seen((size_t)h.chunks, 0);
        for (const uint32_t c : chunk_of_rank) {
            if (c >= h.chunks || seen[c]) return false;
            seen[c] = 1;
        }
    }
    return true;
}

// The whole reader over an open file: which step refused it, or Ok with the header and the four arrays.
enum class Read { Ok, Header, Sections, Structure };

inline Read read_file(int fd, uint64_t expected_chunks, uint64_t generation, SparseFileHeader* h, std::vector<uint32_t>* tok,
                      std::vector<uint64_t>* off, std::vector<Posting>* post, std::vector<uint32_t>* chunk_of_rank) {
    struct stat st;
    if (fstat(fd, &st) != 0 || !cqs_persist::read_all(fd, h, sizeof *h)) return Read::Header;
    if (!check_header(*h, (uint64_t)st.st_size, expected_chunks, generation)) return Read::Header;
    if (!read_sections(fd, *h, tok, off, post, chunk_of_rank)) return Read::Sections;
    return check_structure(*h, *tok, *off, *post, *chunk_of_rank) ? Read::Ok : Read::Structure;
}

}  // namespace cqs_sparse_file
