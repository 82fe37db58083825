// aqc_pipe_out.hpp — where the pipe's bytes go: an output file written by one thread in large sequential writes, the BGZF member
// the host codec wraps .gz output in, and the host buffers (page-locked, or plain memory) the chunks travel through.  Part of
// aqc_pipe.cpp's translation unit (included there only).
#pragma once

#include <fcntl.h>
#include <sys/uio.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/afterqc_hip.h"
#include "aqc_gz.hpp"

namespace {

// An output file.  Measured on the MI355X host (tools/ubench/file_write_rate.cpp): ONE thread issuing large sequential
// write()s fills a file at 6 GB/s (tmpfs) .. 11 GB/s (page cache); several threads pwrite()-ing disjoint ranges of the same
// file, or storing into a shared mapping of it, are 2-5x SLOWER (they fight over the file's page-cache lock).  So every
// output file gets its own writer thread and sees nothing but big sequential writes.
//
// Round 6 (tools/ubench/dma_write_rate.hip, profiles/r06_dma_write_rate.txt: what the round-5 review's "26 % the writers lose" is):
// two files at once take 9.7 - 10.7 GB/s each whatever the source buffer is — lying still or just filled by a D2H copy, on either
// socket, in pieces of 1 / 4 / 16 / 45 MiB — and 12.0 - 13.0 GB/s once the file's blocks exist: write() into a fresh file spends a
// fifth of its time allocating them.  So the writer keeps the file's blocks reserved 1 GiB ahead of its position
// (fallocate(FALLOC_FL_KEEP_SIZE): the size stays what has been written) and gives back what is left over when it closes.
// AQC_FALLOC=0 switches that off; a filesystem without fallocate does so by itself.
struct OutFile {
    int fd = -1;
    uint64_t pos = 0;
    uint64_t reserved = 0;       // blocks exist up to here
    int prealloc = 1;            // 0 off, 1 keep-size, 2 size-extending (the file is cut to `pos` when it closes)
    bool open_(const char* path) {
        fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (const char* e = getenv("AQC_FALLOC")) prealloc = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
        reserved = 0;
        return fd >= 0;
    }
    void reserve_ahead(size_t n) {
        const uint64_t STEP = 1ull << 30;
        if (!prealloc || pos + n + (STEP >> 2) <= reserved) return;
        const uint64_t want = std::max<uint64_t>(reserved, pos) , len = std::max<uint64_t>(STEP, pos + n + (STEP >> 2) - want);
        if (fallocate(fd, prealloc == 1 ? FALLOC_FL_KEEP_SIZE : 0, (off_t)want, (off_t)len) == 0) reserved = want + len;
        else prealloc = 0;       // (not supported here / no space for the reservation: plain writes will say what is wrong, if anything)
    }
    bool append(const uint8_t* p, size_t n) {
        reserve_ahead(n);
        while (n) {
            const ssize_t w = ::write(fd, p, std::min<size_t>(n, 1u << 30));
            if (w <= 0) return false;
            p += w; n -= (size_t)w; pos += (uint64_t)w;
        }
        return true;
    }
    // the same for a list of pieces (writev, IOV_MAX at a time; pieces of length 0 are the caller's business)
    bool appendv(std::vector<struct iovec>& iov) {
        size_t total = 0;
        for (const struct iovec& v : iov) total += v.iov_len;
        reserve_ahead(total);
        size_t i = 0;
        while (i < iov.size()) {
            const int cnt = (int)std::min<size_t>(iov.size() - i, 1024);
            ssize_t w = ::writev(fd, iov.data() + i, cnt);
            if (w <= 0) return false;
            pos += (uint64_t)w;
            while (w > 0 && i < iov.size()) {
                if ((size_t)w >= iov[i].iov_len) { w -= (ssize_t)iov[i].iov_len; ++i; }
                else { iov[i].iov_base = (uint8_t*)iov[i].iov_base + w; iov[i].iov_len -= (size_t)w; w = 0; }
            }
        }
        return true;
    }
    void close_() {
        if (fd >= 0) {
            if (reserved > pos && ftruncate(fd, (off_t)pos) != 0) {}   // (gives the unused reservation back; a size-extending one is cut)
            close(fd);
        }
        fd = -1;
    }
};

inline void bgzf_block(const uint8_t* src, size_t n, int level, std::vector<uint8_t>& out) {
    // one gzip member with the BGZF extra field (BC: total block size - 1); members concatenate into one valid .gz.
    // The deflate stream is the pipe's own (aqc_deflate.cpp); `--compression 0` stores.
    out.resize(18 + aqcgz::deflate_bound(n) + 8);
    const size_t clen = aqcgz::deflate_block(src, n, level, out.data() + 18);
    const size_t bsize = 18 + clen + 8;
    static const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(out.data(), hdr, 16);
    out[16] = (uint8_t)((bsize - 1) & 0xff);
    out[17] = (uint8_t)((bsize - 1) >> 8);
    const uint32_t crc = aqcgz::crc32_fast(0u, src, n);
    uint8_t* t = out.data() + 18 + clen;
    for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
    out.resize(bsize);
}

// A host buffer: page-locked (aqc_host_alloc) or, where no GPU runtime is involved, plain memory.  Move-only; it frees itself —
// for a pipe's buffers that is inside aqc_pipe_destroy, while the HIP runtime is up.
struct HostBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    bool pageable = false;       // plain memory: the assembled good output, and everything of aqc_pipe_split
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    HostBuf(HostBuf&& o) noexcept : p(o.p), cap(o.cap), pageable(o.pageable) { o.p = nullptr; o.cap = 0; }
    HostBuf& operator=(HostBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap; pageable = o.pageable;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~HostBuf() { release(); }
    // room for n bytes; what was in it is NOT kept (p == nullptr: the allocation failed)
    void ensure(size_t n) {
        if (n <= cap) return;
        release();
        cap = n + n / 8 + (1 << 20);
        p = pageable ? (uint8_t*)malloc(cap) : (uint8_t*)aqc_host_alloc(cap);
        if (!p) cap = 0;
    }
    // room for ncap bytes, keeping the first `fill`; false: the allocation failed, the buffer is as it was
    bool grow(size_t ncap, size_t fill) {
        if (ncap <= cap) return true;
        HostBuf n;
        n.pageable = pageable;
        n.ensure(ncap);
        if (!n.p) return false;
        memcpy(n.p, p, fill);
        *this = std::move(n);
        return true;
    }
    void release() {
        if (p) { if (pageable) free(p); else aqc_host_free(p); }
        p = nullptr;
        cap = 0;
    }
};

}  // namespace
