// sparse_index_persist.hip — cqs_hip_sparse_index_save / _load.  The file's format, its writer and its reader with every check
// on bytes from disk are sparse_file_host.h (no device); save adds the copy of the postings off the device and the
// tmp / fsync / rename sequence, load the handle.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "persist_util.h"
#include "sparse_file_host.h"
#include "sparse_internal.h"

namespace sf = cqs_sparse_file;
using cqs_sparse::sfail;

extern "C" {

int32_t cqs_hip_sparse_index_save(cqs_hip_sparse_index* s, const char* path, uint64_t generation, uint64_t* out_checksum) CQS_ABI_TRY {
    if (!s || !path) return CQS_HIP_ERR_INVALID;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;
    S_TRY(s, hipSetDevice(s->device));
    S_TRY(s, hipStreamSynchronize(s->stream));
    std::vector<sf::Posting> post((size_t)s->n_postings);
    if (s->n_postings) S_TRY(s, hipMemcpy(post.data(), s->d_post, (size_t)s->n_postings * sizeof(uint2), hipMemcpyDeviceToHost));
    sf::SparseFileHeader h = sf::make_header(s->ranked, s->n, s->tok.size(), s->n_postings, generation);
    const void* const sections[4] = {s->tok.data(), s->off.data(), post.data(), s->chunk_of_rank.data()};
    const std::string live(path), tmp = live + ".tmp";
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return sfail(s, CQS_HIP_ERR_INVALID, "sparse save: cannot create " + tmp);
    const bool ok = sf::write_file(fd, h, sections, nullptr) && fsync(fd) == 0;
    close(fd);
    if (!ok) { unlink(tmp.c_str()); return sfail(s, CQS_HIP_ERR_INVALID, "sparse save: write failed"); }
    if (rename(tmp.c_str(), live.c_str()) != 0) { unlink(tmp.c_str()); return sfail(s, CQS_HIP_ERR_INVALID, "sparse save: rename failed"); }
    cqs_persist::fsync_parent(live);
    if (out_checksum) *out_checksum = h.checksum;
    return CQS_HIP_OK;
} CQS_ABI_CATCH(s)

int32_t cqs_hip_sparse_index_load(const char* path, uint64_t expected_chunks, uint64_t generation, int32_t device,
                                  cqs_hip_sparse_index** out) CQS_ABI_TRY {
    if (!out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    if (!path) return CQS_HIP_ERR_INVALID;
    return cqs_sparse::create_handle(device, [&](cqs_hip_sparse_index* s, std::vector<sf::Posting>* post) {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return false;                                  // missing file: the caller builds (index.rs:1073-1107)
        struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
        sf::SparseFileHeader h;
        if (sf::read_file(fd, expected_chunks, generation, &h, &s->tok, &s->off, post, &s->chunk_of_rank) != sf::Read::Ok) return false;
        s->n = h.chunks;
        s->ranked = h.ranked != 0;
        return true;
    }, out);
} CQS_ABI_CATCH_NOHANDLE

}  // extern "C"
