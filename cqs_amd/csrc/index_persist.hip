// index_persist.hip — the on-disk blob of the exact index: a 64-byte header and the f32 rows, streamed between HBM and
// the file through two pinned 64 MiB pieces, over one or more device segments in row order (a single-device handle is
// one segment, a row-sharded parent one per shard: sharded.hip).  Entry points: cqs_hip_index_save / cqs_hip_index_load.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "abi_guard.h"
#include "index_internal.h"
#include "persist_util.h"

using namespace cqs_idx;
using namespace cqs_persist;

namespace {

struct FlatHeader {
    char magic[8];
    uint32_t version, dim, metric, pad;
    uint64_t rows, checksum;
    uint8_t reserved[24];
};
static_assert(sizeof(FlatHeader) == 64, "header is 64 bytes");
const char kFlatMagic[8] = {'C', 'Q', 'S', 'H', 'I', 'P', 'F', '1'};

constexpr size_t kIoPiece = 64ull << 20;   // pinned staging piece (x2: copy of piece i+1 overlaps file I/O of piece i)

// The rows of one or more device segments (row order) cut into pieces of <= 64 MiB that never straddle a segment.
struct Piece { const cqs_idx::Segment* seg; size_t off, len; };
std::vector<Piece> cut_pieces(const std::vector<cqs_idx::Segment>& segs, uint32_t dim) {
    std::vector<Piece> out;
    for (const cqs_idx::Segment& sg : segs) {
        const size_t bytes = (size_t)sg.rows * dim * sizeof(float);
        for (size_t off = 0; off < bytes; off += kIoPiece) out.push_back({&sg, off, bytes - off < kIoPiece ? bytes - off : kIoPiece});
    }
    return out;
}
struct PinPair {
    uint8_t* p[2] = {nullptr, nullptr};
    hipError_t alloc(size_t bytes) {
        for (int i = 0; i < 2; ++i) {
            hipError_t e = hipHostMalloc((void**)&p[i], bytes ? bytes : 8, hipHostMallocPortable);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    ~PinPair() { if (p[0]) hipHostFree(p[0]); if (p[1]) hipHostFree(p[1]); }
};
}  // namespace

namespace cqs_idx {

// Blob write = `save_blob_atomic_with_rollback` (src/cagra.rs:1468-1592): refuse on a stale `.bak`; stream the rows
// HBM -> pinned pieces -> `<path>.tmp` (checksummed on the way, fsync); move a live blob to `.bak`; rename tmp ->
// live; on failure restore `.bak`; on success drop it.  Host memory: two 64 MiB pinned pieces, whatever the corpus.
int32_t save_segments(cqs_hip_index* x, const std::vector<Segment>& segs, uint32_t dim, uint32_t metric, const char* path,
                      uint64_t* out_checksum) {
    const std::string live(path), bak = live + ".bak", tmp = live + ".tmp";
    if (exists(bak)) return fail(x, CQS_HIP_ERR_INVALID, "save: stale .bak from a prior failed save; manual recovery required");
    uint64_t rows = 0;
    for (const Segment& sg : segs) rows += sg.rows;
    const size_t bytes = (size_t)rows * dim * sizeof(float);
    const std::vector<Piece> pieces = cut_pieces(segs, dim);
    PinPair pin;
    hipError_t he = pin.alloc(bytes < kIoPiece ? bytes : kIoPiece);
    if (he != hipSuccess) return fail(x, CQS_HIP_ERR_NOMEM, "save: pinned staging", he);
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(x, CQS_HIP_ERR_INVALID, "save: cannot create temp file");
    FlatHeader h{};
    memcpy(h.magic, kFlatMagic, 8);
    h.version = 1; h.dim = dim; h.metric = metric; h.rows = rows;
    bool ok = write_all(fd, &h, sizeof h);   // checksum patched in below
    Checksum ck(bytes);
    auto issue = [&](size_t i) -> hipError_t {
        const Piece& pc = pieces[i];
        hipError_t e = hipSetDevice(pc.seg->device);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(pin.p[i & 1], (const uint8_t*)pc.seg->d_rows + pc.off, pc.len, hipMemcpyDeviceToHost, pc.seg->stream);
    };
    if (ok && !pieces.empty()) he = issue(0);
    for (size_t i = 0; ok && he == hipSuccess && i < pieces.size(); ++i) {
        he = hipStreamSynchronize(pieces[i].seg->stream);            // piece i is in pin[i & 1]
        if (he != hipSuccess) break;
        if (i + 1 < pieces.size() && (he = issue(i + 1)) != hipSuccess) break;
        ck.update(pin.p[i & 1], pieces[i].len, i + 1 == pieces.size());
        ok = write_all(fd, pin.p[i & 1], pieces[i].len);
    }
    if (pieces.empty()) ck.update(nullptr, 0, true);
    for (const Segment& sg : segs) (void)hipStreamSynchronize(sg.stream);
    h.checksum = ck.finish();
    ok = ok && he == hipSuccess && lseek(fd, 0, SEEK_SET) == 0 && write_all(fd, &h, sizeof h) && fsync(fd) == 0;
    close(fd);
    if (!ok) {
        unlink(tmp.c_str());
        return he != hipSuccess ? fail(x, CQS_HIP_ERR_DEVICE, "save: device copy", he) : fail(x, CQS_HIP_ERR_INVALID, "save: write failed");
    }
    const bool backed_up = exists(live);
    if (backed_up) {
        if (rename(live.c_str(), bak.c_str()) != 0) { unlink(tmp.c_str()); return fail(x, CQS_HIP_ERR_INVALID, "save: cannot back up the live blob"); }
        fsync_parent(live);
    }
    if (rename(tmp.c_str(), live.c_str()) != 0) {
        unlink(tmp.c_str());
        if (backed_up) {
            if (rename(bak.c_str(), live.c_str()) != 0) return fail(x, CQS_HIP_ERR_INVALID, "save failed and rollback failed: rename .bak back by hand");
            fsync_parent(live);
        }
        return fail(x, CQS_HIP_ERR_INVALID, "save: rename failed");
    }
    if (backed_up) unlink(bak.c_str());
    fsync_parent(live);
    if (out_checksum) *out_checksum = h.checksum;
    return CQS_HIP_OK;
}

// `CagraIndex::load` (src/cagra.rs:1174-1330), part 1: header / size checks.  Leaves the file open at the rows.
int32_t open_blob(const char* path, uint32_t expected_dim, uint64_t expected_rows, int* fd_out, uint64_t* rows,
                  uint32_t* metric, uint64_t* checksum) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return CQS_HIP_ERR_INVALID;
    FlatHeader h{};
    struct stat st;
    const bool ok = read_all(fd, &h, sizeof h) && memcmp(h.magic, kFlatMagic, 8) == 0 && h.version == 1 &&
                    h.dim == expected_dim && (expected_rows == 0 || h.rows == expected_rows) && h.metric <= CQS_HIP_METRIC_DOT &&
                    fstat(fd, &st) == 0 && h.dim != 0 && h.rows <= (UINT64_MAX - sizeof h) / ((uint64_t)h.dim * 4u) &&
                    (uint64_t)st.st_size == sizeof h + h.rows * h.dim * 4u;
    if (!ok) { close(fd); return CQS_HIP_ERR_INVALID; }
    *fd_out = fd; *rows = h.rows; *metric = h.metric; *checksum = h.checksum;
    return CQS_HIP_OK;
}

// part 2: the rows stream file -> pinned pieces -> HBM (the segments' buffers are allocated by the caller) while
// the checksum is recomputed.  Closes fd.  A mismatch returns CQS_HIP_ERR_INVALID and the caller discards the index.
int32_t read_blob_into(int fd, uint64_t checksum, uint32_t dim, const std::vector<Segment>& segs) {
    uint64_t rows = 0;
    for (const Segment& sg : segs) rows += sg.rows;
    const size_t bytes = (size_t)rows * dim * sizeof(float);
    const std::vector<Piece> pieces = cut_pieces(segs, dim);
    PinPair pin;
    hipError_t he = pin.alloc(bytes < kIoPiece ? bytes : kIoPiece);
    Checksum ck(bytes);
    bool ok = true;
    for (size_t i = 0; ok && he == hipSuccess && i < pieces.size(); ++i) {
        const Piece& pc = pieces[i];
        if (i >= 2) he = hipStreamSynchronize(pieces[i - 2].seg->stream);   // pin[i & 1] was the source of piece i-2's copy
        if (he != hipSuccess) break;
        ok = read_all(fd, pin.p[i & 1], pc.len);                            // overlaps the H2D copy of piece i-1
        if (!ok) break;
        ck.update(pin.p[i & 1], pc.len, i + 1 == pieces.size());
        he = hipSetDevice(pc.seg->device);
        if (he == hipSuccess) he = hipMemcpyAsync((uint8_t*)pc.seg->d_rows + pc.off, pin.p[i & 1], pc.len, hipMemcpyHostToDevice, pc.seg->stream);
    }
    if (pieces.empty()) ck.update(nullptr, 0, true);
    for (const Segment& sg : segs) {
        const hipError_t hs = hipStreamSynchronize(sg.stream);
        if (he == hipSuccess) he = hs;
    }
    close(fd);
    if (he != hipSuccess) return he == hipErrorOutOfMemory ? CQS_HIP_ERR_NOMEM : CQS_HIP_ERR_DEVICE;
    return ok && ck.finish() == checksum ? CQS_HIP_OK : CQS_HIP_ERR_INVALID;
}

}  // namespace cqs_idx

extern "C" {

int32_t cqs_hip_index_save(cqs_hip_index* x, const char* path, uint64_t* out_checksum) CQS_ABI_TRY {
    if (!x || !path) return CQS_HIP_ERR_INVALID;
    if (x->sh) return cqs_sharded::save(x, path, out_checksum);
    std::lock_guard<std::mutex> g(x->mu);
    if (x->poisoned.load(std::memory_order_acquire)) return CQS_HIP_ERR_POISONED;  // src/cagra.rs:1103-1107
    HIP_TRY(x, hipSetDevice(x->device));
    HIP_TRY(x, quiesce(x));
    return save_segments(x, {Segment{x->device, x->d_rows, x->n, x->stream}}, x->dim, x->metric, path, out_checksum);
} CQS_ABI_CATCH(x)

int32_t cqs_hip_index_load(const char* path, uint32_t expected_dim, uint64_t expected_rows, int32_t device,
                           uint64_t row_base, cqs_hip_index** out) CQS_ABI_TRY {
    if (!path || !out) return CQS_HIP_ERR_INVALID;
    *out = nullptr;
    int fd = -1;
    uint64_t rows = 0, checksum = 0;
    uint32_t metric = 0;
    int32_t rc = open_blob(path, expected_dim, expected_rows, &fd, &rows, &metric, &checksum);
    if (rc != CQS_HIP_OK) return rc;
    cqs_hip_index* x = nullptr;
    rc = create_common(rows, expected_dim, metric, device, row_base, out, &x);
    if (rc != CQS_HIP_OK) { close(fd); return rc; }
    x->cap_rows = rows ? rows : 1;
    if (hipMalloc(&x->d_rows, (size_t)x->cap_rows * expected_dim * sizeof(float)) != hipSuccess) {
        close(fd);
        cqs_hip_index_destroy(x);
        return CQS_HIP_ERR_NOMEM;
    }
    rc = read_blob_into(fd, checksum, expected_dim, {Segment{device, x->d_rows, rows, x->stream}});
    if (rc == CQS_HIP_OK) rc = shadow_auto(x);   // (the shadow is never persisted: rebuilt from the loaded rows)
    if (rc != CQS_HIP_OK) { cqs_hip_index_destroy(x); return rc; }
    *out = x;
    return CQS_HIP_OK;
} CQS_ABI_CATCH_NOHANDLE

}  // extern "C"
