// aqc_pipe_source.hpp — where the pipe's bytes come from: newline counting (a chunk ends at its 4K-th newline) and the byte
// sources behind the readers — a plain file (parallel pread), a bzip2 file (libbz2 on threads of its own), a gzip file (BGZF
// members or one big member, inflated in parallel: aqc_gunzip.cpp), or host memory.  Part of aqc_pipe.cpp's translation unit
// (included there only); aqc_source_* of the C ABI hands the same sources out on their own.
#pragma once

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "aqc_bz2.hpp"
#include "aqc_gz.hpp"
#include "aqc_pool.hpp"

namespace {

using aqc_host::Pool;      // aqc_pool.hpp: parallel_for (front lane) + submit (background lane for speculative work)

// ---------------------------------------------------------------------------------------------------------------
// newline counting (the chunk boundary is "the 4K-th newline"): 8 bytes per step, portable; an AVX2 twin where the CPU has it
// ---------------------------------------------------------------------------------------------------------------
uint64_t count_nl_generic(const uint8_t* p, size_t n) {
    uint64_t c = 0;
    size_t i = 0;
    for (; i < n && ((uintptr_t)(p + i) & 7); ++i) c += p[i] == '\n';
    const uint64_t k = 0x0a0a0a0a0a0a0a0aull, lo7 = 0x7f7f7f7f7f7f7f7full;
    for (; i + 8 <= n; i += 8) {
        uint64_t x;
        memcpy(&x, p + i, 8);
        x ^= k;
        const uint64_t z = ~(((x & lo7) + lo7) | x | lo7);      // 0x80 in every zero byte
        c += (uint64_t)__builtin_popcountll(z);
    }
    for (; i < n; ++i) c += p[i] == '\n';
    return c;
}

#if defined(__x86_64__)
__attribute__((target("avx2"))) uint64_t count_nl_avx2(const uint8_t* p, size_t n) {
    uint64_t c = 0;
    size_t i = 0;
    const __m256i nl = _mm256_set1_epi8('\n');
    for (; i + 128 <= n; i += 128) {
        const unsigned m0 = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i*)(p + i)), nl));
        const unsigned m1 = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i*)(p + i + 32)), nl));
        const unsigned m2 = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i*)(p + i + 64)), nl));
        const unsigned m3 = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i*)(p + i + 96)), nl));
        c += (uint64_t)__builtin_popcountll(((uint64_t)m1 << 32) | m0) + (uint64_t)__builtin_popcountll(((uint64_t)m3 << 32) | m2);
    }
    return c + count_nl_generic(p + i, n - i);
}
#endif

uint64_t count_nl(const uint8_t* p, size_t n) {
#if defined(__x86_64__)
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
    if (have_avx2) return count_nl_avx2(p, n);
#endif
    return count_nl_generic(p, n);
}

constexpr size_t SUB = 256 << 10;        // newline counts are kept per 256 KiB block

// position just behind the `want`-th newline of p[0, n) (want >= 1) given the per-block counts; n if there are fewer
size_t locate_nl(const uint8_t* p, size_t n, const std::vector<uint32_t>& cnt, uint64_t want) {
    uint64_t seen = 0;
    for (size_t b = 0; b < cnt.size(); ++b) {
        if (seen + cnt[b] >= want) {
            size_t i = b * SUB;
            const size_t end = std::min(n, i + SUB);
            while (i < end) {
                const uint8_t* q = (const uint8_t*)memchr(p + i, '\n', end - i);
                if (!q) break;
                i = (size_t)(q - p) + 1;
                if (++seen == want) return i;
            }
            return n;      // (counts and bytes disagree: cannot happen)
        }
        seen += cnt[b];
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------
// byte sources: a plain file (parallel pread), a gzip stream (zlib; BGZF / multi-member inputs are inflated
// member-parallel), or host memory
// ---------------------------------------------------------------------------------------------------------------
struct Source {
    virtual ~Source() {}
    // fill dst[0, want) with the next bytes of the stream; returns the bytes delivered (< want only at the end)
    virtual size_t read(uint8_t* dst, size_t want) = 0;
    // the same, into base[fill, fill + want), ALSO counting the newlines of every SUB-sized block of `base` the new bytes
    // touch (cnt[b] = newlines in base[b * SUB, min((b + 1) * SUB, fill + got)); the block the old bytes end in is recounted)
    virtual size_t read_counted(uint8_t* base, size_t fill, size_t want, std::vector<uint32_t>& cnt, Pool* pool) {
        const size_t got = want ? read(base + fill, want) : 0;
        count_blocks(base, fill, fill + got, cnt, pool);
        return got;
    }
    virtual bool failed() const { return false; }
    virtual const char* why() const { return "read error"; }
    static void count_blocks(const uint8_t* base, size_t from, size_t to, std::vector<uint32_t>& cnt, Pool* pool) {
        const size_t nb = (to + SUB - 1) / SUB, b0 = std::min(nb, from / SUB);
        cnt.resize(nb);
        pool->parallel_for(nb - b0, [&](size_t i) {
            const size_t o = (b0 + i) * SUB;
            cnt[b0 + i] = (uint32_t)count_nl(base + o, std::min(SUB, to - o));
        });
    }
};

struct FileSource : Source {
    int fd = -1;
    uint64_t pos = 0, size = 0;
    Pool* pool;
    bool bad = false;            // sticky: a failed pread is an error, never "end of file"
    FileSource(const char* path, Pool* p) : pool(p) {
        fd = open(path, O_RDONLY);
        if (fd >= 0) {
            struct stat st;
            if (fstat(fd, &st) == 0) size = (uint64_t)st.st_size;
            (void)posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
        }
    }
    ~FileSource() override { if (fd >= 0) close(fd); }
    bool failed() const override { return fd < 0 || bad; }
    size_t read(uint8_t* dst, size_t want) override {
        std::vector<uint32_t> none;
        return read_impl(dst, 0, want, nullptr);
    }
    // the pieces are cut at multiples of 4 * SUB of `base`, so the thread that pread a piece counts its newlines while
    // the bytes are still in its cache: one pass, one parallel_for
    size_t read_counted(uint8_t* base, size_t fill, size_t want, std::vector<uint32_t>& cnt, Pool*) override {
        return read_impl(base, fill, want, &cnt);
    }
    size_t read_impl(uint8_t* base, size_t fill, size_t want, std::vector<uint32_t>* cnt) {
        const uint64_t left = size > pos ? size - pos : 0;
        const size_t take = (size_t)std::min<uint64_t>(want, left);
        const size_t end = fill + take;
        const size_t PIECE = 4 * SUB;
        const size_t p0 = fill / PIECE, p1 = (end + PIECE - 1) / PIECE;
        if (cnt) cnt->resize((end + SUB - 1) / SUB);
        std::atomic<bool> err{false};
        pool->parallel_for(p1 > p0 ? p1 - p0 : 0, [&](size_t k) {
            const size_t lo = std::max(fill, (p0 + k) * PIECE), hi = std::min(end, (p0 + k + 1) * PIECE);
            size_t off = lo;
            while (off < hi) {
                const ssize_t got = pread(fd, base + off, hi - off, (off_t)(pos + (off - fill)));
                if (got <= 0) { err = true; return; }
                off += (size_t)got;
            }
            if (cnt)
                for (size_t b = lo / SUB; b * SUB < hi; ++b) (*cnt)[b] = (uint32_t)count_nl(base + b * SUB, std::min(SUB, end - b * SUB));
        });
        if (err) { bad = true; return 0; }
        pos += take;
        return take;
    }
};

// A bzip2 file (fastq.py:25-26: bz2.BZ2File upstream).  libbz2 does the decoding — loaded at run time (dlopen: the image carries the
// library Python's bz2 module links, not its header) — on threads of its own, so that the pipe's readers, GPUs and writers work
// while it does: the file is mapped and cut at its STREAM starts ("BZh1".."BZh9" + the block magic, byte aligned: pbzip2 and
// concatenated files have many, plain bzip2 one); a producer thread decodes windows of streams in parallel on the pool and queues
// their text in order.  A file that ends inside a stream, or that libbz2 rejects, is an error.  (Every stream is decoded, as
// python 3's BZ2File does — the path the serial loop takes for .bz2; python 2's reads only the first, qualitycontrol.py:77-78
// warns about pbzip2 files.)
using aqcbz::Bz2Api;       // aqc_bz2.hpp: shared with the device driver, which hands blocks back to libbz2

std::atomic<uint64_t> g_bz2_in_stats[4];     // blocks of the streams a device decoder was given / of them decoded on a GPU / text bytes of every bzip2 input / of them from a GPU (process-wide)

struct Bz2Source : Source {
    int fd = -1;
    Pool* pool;
    const uint8_t* map = nullptr;
    size_t size = 0;
    std::atomic<bool> bad{false}, stop{false};
    char err[200] = "";
    std::mutex err_mu;
    std::vector<size_t> starts;                 // stream starts + the file's size
    std::thread producer;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::vector<uint8_t>> q;         // decoded text, in order
    size_t q_bytes = 0, front_off = 0;
    bool done = false;
    // a big stream's blocks go to this decoder in groups (aqc_bunzip2_offload.hip) when it is at least dev_min bytes compressed
    aqcbz::StreamDecoder* dec = nullptr;
    size_t dev_min = 0;
    aqcbz::StreamStats dev_stats;
    uint64_t text_bytes = 0;

    void fail(const char* msg) {
        {
            std::lock_guard<std::mutex> g(err_mu);
            if (!bad) snprintf(err, sizeof(err), "%s", msg);
        }
        {
            std::lock_guard<std::mutex> g(mu);
            bad = true;
        }
        cv.notify_all();
    }
    Bz2Source(const char* path, Pool* p, aqcbz::StreamDecoder* device_decoder = nullptr, size_t device_min = 0) : pool(p), dec(device_decoder), dev_min(device_min) {
        fd = open(path, O_RDONLY);
        if (fd < 0) { fail("cannot open the file"); return; }
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { fail("not a regular file"); return; }
        size = (size_t)st.st_size;
        if (!Bz2Api::get().ok) { fail("libbz2 could not be loaded (dlopen libbz2.so.1.0)"); return; }
        if (size) {
            void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { fail("cannot map the file"); return; }
            map = (const uint8_t*)m;
            (void)madvise(m, size, MADV_SEQUENTIAL);
            if (size < 10 || memcmp(map, "BZh", 3) != 0) { fail("not a bzip2 file"); return; }
        }
        producer = std::thread([this] { produce(); });
    }
    ~Bz2Source() override {
        {
            std::lock_guard<std::mutex> g(mu);          // (under the lock the producer evaluates its wait predicate with: no lost wake-up)
            stop = true;
        }
        cv.notify_all();
        if (producer.joinable()) producer.join();
        g_bz2_in_stats[2] += text_bytes;         // (every bzip2 source; libbz2 does not say how many blocks it decoded, so blocks are counted for device decoders' streams only)
        if (dec) {
            g_bz2_in_stats[0] += dev_stats.dev_blocks + dev_stats.host_blocks; g_bz2_in_stats[1] += dev_stats.dev_blocks;
            g_bz2_in_stats[3] += dev_stats.dev_bytes;
            if (getenv("AQC_PIPE_DEBUG"))
                fprintf(stderr, "pipe: bunzip2 — %llu blocks from the device (%.1f MB of text), %llu handed back to libbz2 (%.1f MB)\n", (unsigned long long)dev_stats.dev_blocks,
                        1e-6 * (double)dev_stats.dev_bytes, (unsigned long long)dev_stats.host_blocks, 1e-6 * (double)dev_stats.host_bytes);
        }
        if (map) munmap((void*)map, size);
        if (fd >= 0) close(fd);
    }
    bool failed() const override { return bad; }
    const char* why() const override { return err; }

    static bool stream_start(const uint8_t* p) { return aqcbz::is_stream_start(p); }
    // one stream -> text; false: libbz2 rejected it or it ends early (aqcbz::host_decode: the one libbz2 loop, shared with the
    // device decoder's hand-back).  *garbage: bytes follow the stream's end inside [a, b) that are not a stream — python's
    // BZ2File reads up to there and ignores the rest of the FILE (its _compression.DecompressReader treats data that does not
    // decompress as trailing garbage), so the caller stops behind this stream.
    // sink != nullptr: the text is handed over in pieces of PIECE bytes as they fill (a big stream never sits in memory whole:
    // round-5 advisory — a plain `bzip2` file is ONE stream, and the queue's 1 GiB bound only counted whole streams)
    static constexpr size_t PIECE = 16u << 20;
    bool decode(size_t a, size_t b, std::vector<uint8_t>& out, bool* garbage, const std::function<bool(std::vector<uint8_t>&&)>* sink = nullptr) {
        out.clear();
        out.reserve(sink ? PIECE : std::max<size_t>(1u << 20, (b - a) * 5));
        const aqcbz::Sink put = [&](const uint8_t* p, size_t n) {
            if (!sink) { out.insert(out.end(), p, p + n); return true; }
            while (n) {
                const size_t k = std::min(n, PIECE - out.size());
                out.insert(out.end(), p, p + k);
                p += k; n -= k;
                if (out.size() == PIECE) {
                    if (!(*sink)(std::move(out))) return false;                       // (stopped)
                    out = std::vector<uint8_t>();
                    out.reserve(PIECE);
                }
            }
            return true;
        };
        size_t end = b;
        if (aqcbz::host_decode(map, a, b, 0, put, &end, nullptr, &stop) != 0) return false;
        if (garbage) *garbage = end != b;
        if (sink && !out.empty()) return (*sink)(std::move(out));
        return true;
    }
    // decoded text into the queue, in order; false: the reader has gone
    bool enqueue(std::vector<uint8_t>&& text) {
        if (text.empty()) return true;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop.load() || q_bytes < (1u << 30); });
        if (stop) return false;
        q_bytes += text.size();
        text_bytes += text.size();
        q.push_back(std::move(text));
        lk.unlock();
        cv.notify_all();
        return true;
    }
    void produce() {
        // stream starts: byte aligned (a stream is padded to a whole byte); ten fixed bytes make a chance hit a 2^-80 event
        if (size) {
            const size_t nb = (size + (4u << 20) - 1) / (4u << 20);
            std::vector<std::vector<size_t>> hits(nb);
            pool->parallel_for(nb, [&](size_t i) {
                const size_t lo = i * (4u << 20), hi = std::min(size, lo + (4u << 20));
                for (size_t o = lo; o < hi && o + 10 <= size; ++o) {
                    const uint8_t* hit = (const uint8_t*)memchr(map + o, 'B', hi - o);
                    if (!hit) break;
                    o = (size_t)(hit - map);
                    if (o + 10 <= size && stream_start(map + o)) hits[i].push_back(o);
                }
            });
            for (auto& h : hits) starts.insert(starts.end(), h.begin(), h.end());
            if (starts.empty() || starts[0] != 0) { fail("not a bzip2 file"); starts.clear(); }
            starts.push_back(size);
        }
        // small streams (pbzip2's blocks: <= 900 KB of text each) are decoded whole, a window of them in parallel on the pool; a
        // big one — the single stream of a plain `bzip2` file — is decoded here, piece by piece, straight into the queue, or, when
        // the source was given a device decoder and the stream is at least dev_min bytes, block by block on the device
        const size_t window = (size_t)std::max(2, pool->size());
        const size_t BIG = 8u << 20;
        bool cut = false;                         // garbage behind a stream: python's reader ends the file there
        for (size_t k = 0; k + 1 < starts.size() && !stop && !bad && !cut;) {
            if (dec && starts[k + 1] - starts[k] >= dev_min) {
                // the device decodes the stream's blocks in groups; their text is queued in order, under the same back-pressure
                const aqcbz::Sink sink = [this](const uint8_t* p, size_t n) {
                    for (size_t o = 0; o < n; o += PIECE)
                        if (!enqueue(std::vector<uint8_t>(p + o, p + std::min(n, o + PIECE)))) return false;
                    return true;
                };
                size_t end = starts[k + 1];
                const int rc = dec->decode(map, starts[k], starts[k + 1], sink, &end, &dev_stats, &stop);
                if (rc != 0) { if (!stop) fail("corrupt or truncated bzip2 stream"); break; }
                cut = end != starts[k + 1];
                ++k;
                continue;
            }
            if (starts[k + 1] - starts[k] > BIG) {
                std::vector<uint8_t> out;
                bool garbage = false;
                const std::function<bool(std::vector<uint8_t>&&)> sink = [this](std::vector<uint8_t>&& t) { return enqueue(std::move(t)); };
                if (!decode(starts[k], starts[k + 1], out, &garbage, &sink)) { if (!stop) fail("corrupt or truncated bzip2 stream"); break; }
                cut = garbage;
                ++k;
                continue;
            }
            size_t n = 0;
            while (n < window && k + n + 1 < starts.size() && starts[k + n + 1] - starts[k + n] <= BIG && !(dec && starts[k + n + 1] - starts[k + n] >= dev_min)) ++n;
            std::vector<std::vector<uint8_t>> outs(n);
            std::vector<char> good(n, 0), junk(n, 0);
            pool->parallel_for(n, [&](size_t i) { bool g = false; good[i] = decode(starts[k + i], starts[k + i + 1], outs[i], &g) ? 1 : 0; junk[i] = g ? 1 : 0; });
            for (size_t i = 0; i < n && !bad; ++i) {
                if (!good[i]) { fail("corrupt or truncated bzip2 stream"); break; }
                if (!enqueue(std::move(outs[i]))) break;
                if (junk[i]) { cut = true; break; }
            }
            k += n;
        }
        {
            std::lock_guard<std::mutex> g(mu);
            done = true;
        }
        cv.notify_all();
    }
    size_t read(uint8_t* dst, size_t want) override {
        size_t got = 0;
        while (got < want) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !q.empty() || done || bad; });
            if (bad) return 0;
            if (q.empty()) break;                                  // done
            std::vector<uint8_t>& f = q.front();
            const size_t take = std::min(want - got, f.size() - front_off);
            lk.unlock();
            memcpy(dst + got, f.data() + front_off, take);         // (the front buffer is only ever popped by this thread)
            got += take;
            lk.lock();
            front_off += take;
            if (front_off == f.size()) { q_bytes -= f.size(); q.pop_front(); front_off = 0; lk.unlock(); cv.notify_all(); }
        }
        return bad ? 0 : got;
    }
};

// A gzip file (fastq.py:23-24 opens it with gzip.open upstream).  The file is mapped; then
//   * members that carry the BGZF extra field ("BC": the member's compressed size) are located by walking the headers and
//     inflated independently, in parallel;
//   * anything else — one big member as gzip / pigz / Python write it, or members without sizes — goes through
//     aqcgz::ParallelGunzip: speculative sections from block boundaries found in the middle of the stream, committed in order.
// Every member's CRC-32 and length are checked; a file that ends inside a member is an error (gzip.open raises EOFError).
std::atomic<uint64_t> g_gz_in_stats[4];      // sections committed / of them from the device / text bytes / of them from the device (process-wide)

struct GzSource : Source {
    int fd = -1;
    Pool* pool;
    const uint8_t* map = nullptr;
    size_t size = 0;
    bool bgzf = false, bad = false, mapped = false;
    char err[200] = "";
    std::unique_ptr<aqcgz::ParallelGunzip> pg;
    // BGZF walk
    size_t pos = 0;
    std::vector<uint8_t> spill;
    size_t spill_lo = 0;
    // fallback for files that cannot be mapped (pipes): one zlib stream
    std::vector<uint8_t> in;
    size_t in_lo = 0, in_hi = 0;
    bool file_eof = false, stream_end = true, any_in_member = false;
    z_stream zs{};
    bool zs_init = false;

    GzSource(const char* path, Pool* p, size_t section_bytes = 0, aqcgz::SectionOffload* offload = nullptr) : pool(p) {
        fd = open(path, O_RDONLY);
        if (fd < 0) return;
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            size = (size_t)st.st_size;
            if (size == 0) { mapped = true; return; }
            void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                map = (const uint8_t*)m;
                mapped = true;
                (void)madvise(m, size, MADV_SEQUENTIAL);
                bgzf = is_bgzf_header(map, size);
                if (!bgzf) {
                    const int threads = std::max(1, pool->size());
                    // sections in flight: two per pool thread (a thread decodes two sections alternately, aqc_gunzip.cpp; a single-end
                    // run has only this stream to keep the pool busy); more only means more symbol buffers touched for the first
                    // time (tools/gpu_gzrate.sh, GZ_MATRIX)
                    const int inflight = std::max(4, std::min(2 * threads, 64));
                    size_t sec = section_bytes;
                    if (!sec) {
                        if (const char* e = getenv("AQC_GZ_SECTION")) sec = (size_t)atoll(e);
                    }
                    if (!sec) sec = std::min<size_t>(offload ? (1u << 20) : (2u << 20), std::max<size_t>(256u << 10, size / (size_t)(4 * inflight)));
                    pg.reset(new aqcgz::ParallelGunzip(map, size, pool, inflight, sec, offload));
                }
                return;
            }
        }
        in.resize(8 << 20);
    }
    ~GzSource() override {
        if (pg) {
            g_gz_in_stats[0] += pg->sections_accepted; g_gz_in_stats[1] += pg->offloaded_accepted;
            g_gz_in_stats[2] += pg->total_out; g_gz_in_stats[3] += pg->offloaded_bytes;
            if (getenv("AQC_PIPE_DEBUG"))
                fprintf(stderr, "pipe: gunzip — %llu sections committed (%llu from the device of %llu handed to it), %llu discarded, %.1f MB of %.1f MB decoded sequentially\n",
                        (unsigned long long)pg->sections_accepted, (unsigned long long)pg->offloaded_accepted, (unsigned long long)pg->sections_offloaded,
                        (unsigned long long)pg->sections_discarded, 1e-6 * (double)pg->bridged_bytes, 1e-6 * (double)pg->total_out);
            if (getenv("AQC_PIPE_DEBUG"))
                fprintf(stderr, "pipe: gunzip consumer, ms inside read() — waiting for a pool section %.1f, for a device section %.1f, for the device to resolve a run %.1f (%.1f MB of text resolved there), for the translation of what it committed + the copies from the device %.1f, handing out work %.1f, committing %.1f, decoding sequentially %.1f\n",
                        pg->us_wait_pool / 1e3, pg->us_wait_device / 1e3, pg->us_resolve / 1e3, 1e-6 * (double)pg->resident_bytes, pg->us_drain / 1e3, pg->us_top_up / 1e3, pg->us_accept / 1e3, pg->us_bridge / 1e3);
        }
        pg.reset();
        if (map) munmap((void*)map, size);
        if (zs_init) inflateEnd(&zs);
        if (fd >= 0) close(fd);
    }
    bool failed() const override { return fd < 0 || bad; }
    const char* why() const override { return err[0] ? err : "read error"; }
    void fail(const char* what) { if (!bad) snprintf(err, sizeof(err), "%s", what); bad = true; }
    static bool is_bgzf_header(const uint8_t* h, size_t n) {
        return n >= 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' &&
               h[14] == 2 && h[15] == 0;
    }
    size_t read(uint8_t* dst, size_t want) override {
        if (bad) return 0;
        if (!mapped) return read_stream(dst, want);
        if (size == 0) return 0;
        if (bgzf) return read_bgzf(dst, want);
        const size_t got = pg->read(dst, want);
        if (pg->failed()) { fail(pg->error()); return 0; }
        return got;
    }

    // read(), but text that is in device memory stays there and is listed in *segs (one-member files with a device decoder only)
    bool takes_segments() const { return mapped && !bgzf && pg != nullptr && size != 0; }
    size_t read_segments(uint8_t* dst, size_t want, std::vector<aqcgz::DevSegment>* segs) {
        if (bad) return 0;
        if (!takes_segments()) return read(dst, want);
        const size_t got = pg->read(dst, want, segs);
        if (pg->failed()) { fail(pg->error()); return 0; }
        return got;
    }

    size_t read_bgzf(uint8_t* dst, size_t want) {
        size_t out = 0;
        if (spill_lo < spill.size()) {
            const size_t k = std::min(want, spill.size() - spill_lo);
            memcpy(dst, spill.data() + spill_lo, k);
            spill_lo += k;
            out = k;
            if (spill_lo == spill.size()) { spill.clear(); spill_lo = 0; }
        }
        struct Blk { size_t coff, clen, isize, ooff; uint32_t crc; };
        while (out < want && !bad && pos < size) {
            // walk the members until they cover what is asked for
            std::vector<Blk> blks;
            size_t p = pos, total = 0;
            bool foreign = false;
            while (p < size && total < (want - out) + (1u << 20)) {
                // zero bytes between / behind members are padding (Python's gzip module, which upstream reads through, skips them)
                while (p < size && map[p] == 0) ++p;
                if (p == size) break;
                if (!is_bgzf_header(map + p, size - p)) { foreign = true; break; }
                const size_t bsize = (size_t)(map[p + 16] | (map[p + 17] << 8)) + 1;
                if (bsize < 26 || p + bsize > size) { fail("truncated BGZF member"); break; }
                const uint8_t* t = map + p + bsize - 8;
                uint32_t crc, isz;
                memcpy(&crc, t, 4); memcpy(&isz, t + 4, 4);
                // (a BGZF member holds at most 64 KiB of data: a larger ISIZE is a damaged trailer, not a reason to allocate gigabytes)
                if (isz > 65536u) { fail("corrupt BGZF member (ISIZE beyond 64 KiB)"); break; }
                blks.push_back(Blk{p + 18, bsize - 18 - 8, (size_t)isz, total, crc});
                total += isz;
                p += bsize;
            }
            if (bad) break;
            if (blks.empty()) {
                if (foreign) {
                    // a member without the size field behind BGZF ones (cat of different writers): the general decoder takes over
                    pg.reset(new aqcgz::ParallelGunzip(map + pos, size - pos, pool, std::max(4, pool->size()), 1u << 20));
                    bgzf = false;
                    const size_t got = pg->read(dst + out, want - out);
                    if (pg->failed()) { fail(pg->error()); return 0; }
                    return out + got;
                }
                pos = p;
                break;
            }
            const size_t room = want - out;
            size_t fit_total = 0;
            for (auto& b : blks) if (b.ooff + b.isize <= room) fit_total = b.ooff + b.isize;
            spill.assign(total - fit_total, 0);
            spill_lo = 0;
            std::atomic<bool> e{false};
            uint8_t* const d0 = dst + out;
            // two members per task, decoded alternately (aqcgz::decode_pair: two dependency chains share one core's issue slots)
            pool->parallel_for((blks.size() + 1) / 2, [&](size_t t) {
                const size_t i0 = 2 * t, i1 = std::min(2 * t + 1, blks.size() - 1);
                uint8_t* o[2];
                const uint8_t* src[2];
                size_t n[2], cap[2];
                int64_t got[2];
                for (int k = 0; k < 2; ++k) {
                    const Blk& b = blks[k ? i1 : i0];
                    o[k] = b.ooff + b.isize <= room ? d0 + b.ooff : spill.data() + (b.ooff - fit_total);
                    src[k] = map + b.coff; n[k] = b.clen; cap[k] = b.isize;
                }
                if (i1 != i0) aqcgz::inflate_raw2(src, n, o, cap, got);
                else got[0] = got[1] = aqcgz::inflate_raw(src[0], n[0], o[0], cap[0]);
                for (int k = 0; k < 2; ++k) {
                    const Blk& b = blks[k ? i1 : i0];
                    if (got[k] != (int64_t)b.isize || aqcgz::crc32_fast(0u, o[k], b.isize) != b.crc) e = true;
                }
            });
            if (e) { fail("corrupt BGZF member (inflate / CRC-32 / length)"); break; }
            pos = p;
            out += fit_total;
            if (!spill.empty()) {
                const size_t k = std::min(want - out, spill.size());
                memcpy(dst + out, spill.data(), k);
                spill_lo = k;
                out += k;
                if (spill_lo == spill.size()) { spill.clear(); spill_lo = 0; }
            }
        }
        return bad ? 0 : out;
    }

    void refill() {
        if (in_lo > 0 && in_lo < in_hi) memmove(in.data(), in.data() + in_lo, in_hi - in_lo);
        in_hi -= in_lo;
        in_lo = 0;
        while (!file_eof && in_hi < in.size()) {
            const ssize_t got = ::read(fd, in.data() + in_hi, in.size() - in_hi);
            if (got < 0) { fail("read error"); file_eof = true; break; }
            if (got == 0) { file_eof = true; break; }
            in_hi += (size_t)got;
        }
    }
    size_t read_stream(uint8_t* dst, size_t want) {
        size_t out = 0;
        while (out < want && !bad) {
            if (in_lo == in_hi) {
                refill();
                if (in_lo == in_hi) break;          // end of the file
            }
            if (stream_end) {
                // next member (concatenated members are one gzip file); zero padding behind the last one is ignored
                while (in_lo < in_hi && in[in_lo] == 0) ++in_lo;
                if (in_lo == in_hi) continue;
                if (zs_init) inflateEnd(&zs);
                memset(&zs, 0, sizeof(zs));
                if (inflateInit2(&zs, 15 + 16) != Z_OK) { fail("inflateInit2 failed"); break; }
                zs_init = true;
                stream_end = false;
            }
            zs.next_in = in.data() + in_lo;
            zs.avail_in = (uInt)std::min<size_t>(in_hi - in_lo, 1u << 30);
            zs.next_out = dst + out;
            zs.avail_out = (uInt)std::min<size_t>(want - out, 1u << 30);
            const uInt ai = zs.avail_in, ao = zs.avail_out;
            const int rc = inflate(&zs, Z_NO_FLUSH);      // (zlib checks the member's CRC-32 / length itself)
            in_lo += ai - zs.avail_in;
            out += ao - zs.avail_out;
            if (rc == Z_STREAM_END) stream_end = true;
            else if (rc != Z_OK && rc != Z_BUF_ERROR) { fail("corrupt gzip data"); break; }
            else if (rc == Z_BUF_ERROR && ai == zs.avail_in && ao == zs.avail_out) {
                if (file_eof && in_lo == in_hi) break;
                refill();
                if (in_lo == in_hi) break;
            }
        }
        // the file ended inside a member: gzip.open raises EOFError there, so do we
        if (out < want && !bad && !stream_end && file_eof && in_lo == in_hi) fail("gzip stream ends before its trailer (truncated file)");
        return bad ? 0 : out;
    }
};

}  // namespace
