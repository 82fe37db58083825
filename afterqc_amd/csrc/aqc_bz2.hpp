// aqc_bz2.hpp — the host side of bzip2 input that the pipe (aqc_pipe_source.hpp: Bz2Source), the device driver
// (aqc_bunzip2_offload.hip) and the CPU self-test (tests/native/bzb_selftest.cpp) share: libbz2 loaded at run time, one stream
// decoded with it, and the walk over one stream's blocks that a block decoder — the device, or the self-test's plain loops over
// the same functions — is driven by (decode_stream: windows, groups, the chain rule's host half, the hand-back).
#pragma once

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

namespace aqcbz {

// libbz2 — loaded at run time (dlopen: the image carries the library Python's bz2 module links, not its header)
struct Bz2Api {
    struct Stream {
        char* next_in; unsigned int avail_in, total_in_lo32, total_in_hi32;
        char* next_out; unsigned int avail_out, total_out_lo32, total_out_hi32;
        void* state; void* (*bzalloc)(void*, int, int); void (*bzfree)(void*, void*); void* opaque;
    };
    int (*init)(Stream*, int, int) = nullptr;
    int (*step)(Stream*) = nullptr;
    int (*end)(Stream*) = nullptr;
    bool ok = false;
    Bz2Api() {
        void* h = nullptr;
        for (const char* name : {"libbz2.so.1.0", "libbz2.so.1", "libbz2.so"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) return;
        init = (int (*)(Stream*, int, int))dlsym(h, "BZ2_bzDecompressInit");
        step = (int (*)(Stream*))dlsym(h, "BZ2_bzDecompress");
        end = (int (*)(Stream*))dlsym(h, "BZ2_bzDecompressEnd");
        ok = init && step && end;
    }
    static const Bz2Api& get() { static Bz2Api api; return api; }
};

// a stream starts here: "BZh1".."BZh9" and a block or end-of-stream magic (byte aligned: a stream is padded to a whole byte; ten
// fixed bytes make a chance hit a 2^-80 event)
inline bool is_stream_start(const uint8_t* p) {
    static const uint8_t blk[6] = {0x31, 0x41, 0x59, 0x26, 0x53, 0x59}, eos[6] = {0x17, 0x72, 0x45, 0x38, 0x50, 0x90};
    return p[0] == 'B' && p[1] == 'Z' && p[2] == 'h' && p[3] >= '1' && p[3] <= '9' && (memcmp(p + 4, blk, 6) == 0 || memcmp(p + 4, eos, 6) == 0);
}
// the stream starts of a file image, then its size
inline void stream_starts(const uint8_t* data, size_t size, std::vector<size_t>& starts) {
    for (size_t o = 0; o + 10 <= size; ++o) {
        const uint8_t* hit = (const uint8_t*)memchr(data + o, 'B', size - o);
        if (!hit) break;
        o = (size_t)(hit - data);
        if (o + 10 <= size && is_stream_start(data + o)) starts.push_back(o);
    }
    starts.push_back(size);
}

// text in order; false: the reader has gone
using Sink = std::function<bool(const uint8_t*, size_t)>;

constexpr int BZ_ERR_DATA = -1;        // libbz2 rejected the stream, or it ends early
constexpr int BZ_ERR_STOPPED = -2;     // the sink, or *stop, said so
constexpr int BZ_ERR_NOLIB = -3;

// The stream at data[a, b) decoded with libbz2; the first `skip` bytes of its text are dropped (the caller has them).
// *end_byte: the byte behind the stream's trailer; *produced: bytes handed to the sink.
inline int host_decode(const uint8_t* data, size_t a, size_t b, uint64_t skip, const Sink& sink, size_t* end_byte, uint64_t* produced,
                       const std::atomic<bool>* stop) {
    const Bz2Api& api = Bz2Api::get();
    if (!api.ok) return BZ_ERR_NOLIB;
    Bz2Api::Stream z{};
    if (api.init(&z, 0, 0) != 0) return BZ_ERR_DATA;
    std::vector<uint8_t> out(4u << 20);
    z.next_in = (char*)(data + a);
    size_t in_left = b - a;
    int rc = BZ_ERR_DATA;
    for (;;) {
        if (z.avail_in == 0 && in_left) { z.avail_in = (unsigned)std::min<size_t>(in_left, 1u << 30); in_left -= z.avail_in; }
        z.next_out = (char*)out.data();
        z.avail_out = (unsigned)out.size();
        const int r = api.step(&z);
        size_t got = out.size() - z.avail_out;
        const uint8_t* p = out.data();
        const size_t drop = (size_t)std::min<uint64_t>(skip, got);
        skip -= drop; p += drop; got -= drop;
        if (got) {
            if (!sink(p, got)) { rc = BZ_ERR_STOPPED; break; }
            if (produced) *produced += got;
        }
        if (r == 4) {                                                       // BZ_STREAM_END
            rc = 0;
            if (end_byte) *end_byte = b - in_left - z.avail_in;
            break;
        }
        if (r != 0 || (z.avail_in == 0 && in_left == 0 && z.avail_out != 0)) break;      // error, or the stream ends early
        if (stop && stop->load()) { rc = BZ_ERR_STOPPED; break; }
    }
    api.end(&z);
    return rc;
}

struct StreamStats { uint64_t dev_blocks = 0, host_blocks = 0, host_bytes = 0, dev_bytes = 0; };

// What a block decoder hands back for one group of candidates: the blocks that chained up from the bit it was given.
struct GroupResult {
    uint32_t n = 0;                       // chained blocks
    uint32_t stop_status = 0;             // aqc::BzbChain::stop_status
    std::vector<uint32_t> crc_hdr, crc_txt;
    std::vector<uint64_t> end_bit;        // relative to the window
    std::vector<uint64_t> off;            // [n + 1] the blocks' places in text
    const uint8_t* text = nullptr;
};

// One stream, data[a, b) with "BZh1".."BZh9" at a, through a block decoder B:
//   B.scan(window, bytes, cands, &overflow)      every block / end-of-stream magic of the window, sorted (bit << 1 | end-of-stream)
//   B.group(first, g, cur, level, R)             candidates [first, first + g) decoded, chained from bit `cur`, their text expanded
//   B.default_group(level)                       the group size its buffers are made for
// The chain rule's host half lives here: a block counts only if its CRC matches; the stream ends where the end-of-stream magic
// stands at the bit the last block ended on and the combined CRC equals the trailer's.  Whatever does not chain — damage, a
// randomised block, a block the decoder refuses — is handed back: libbz2 decodes the stream and the text the blocks before have
// delivered is dropped from its output, so what it reports is what the caller reports.
// (bit positions 0 relative to data; a window is cut where the chain stands and slid on when its end cuts a block short)
template <class Backend>
int decode_stream(Backend& B, const uint8_t* data, size_t a, size_t b, size_t window_bytes, size_t group_blocks, const Sink& sink, size_t* end_byte,
                  StreamStats& st, const std::atomic<bool>* stop) {
    if (b < a + 4 || data[a + 3] < '1' || data[a + 3] > '9') return BZ_ERR_DATA;
    const uint32_t level = (uint32_t)(data[a + 3] - '0');
    const size_t G = group_blocks ? std::min(group_blocks, B.default_group(level)) : B.default_group(level);
    uint64_t cur = (uint64_t)a * 8u + 32u, delivered = 0, blocks_left = 0;
    uint32_t combined = 0;
    std::vector<uint64_t> cands;
    GroupResult R;
    for (bool handback = false; !handback;) {
        const size_t win0 = (size_t)(cur >> 3), wlen = std::min(b - win0, std::max<size_t>(window_bytes, 1u << 16));
        const bool last = win0 + wlen == b;
        bool overflow = false;
        if (!B.scan(data + win0, wlen, cands, &overflow)) break;
        if (overflow) {
            // more magics than the list holds: a smaller window, or the host
            if (wlen <= (1u << 20)) break;
            window_bytes = wlen / 8;
            continue;
        }
        const uint64_t start_rel = cur - (uint64_t)win0 * 8u;
        uint64_t rel = start_rel;
        size_t idx = (size_t)(std::lower_bound(cands.begin(), cands.end(), rel << 1) - cands.begin());
        while (idx < cands.size() && (cands[idx] >> 1) == rel) {
            if (stop && stop->load()) return BZ_ERR_STOPPED;
            if (cands[idx] & 1ull) {
                // the end of the stream: the combined CRC behind the magic, then padding to a whole byte
                if (rel + 80u > (uint64_t)wlen * 8u) break;
                const uint64_t at = (uint64_t)win0 * 8u + rel + 48u;
                uint64_t w = 0;
                for (size_t k = 0; k < 5; ++k) w = (w << 8) | ((size_t)(at >> 3) + k < b ? data[(size_t)(at >> 3) + k] : 0u);
                const uint32_t stored = (uint32_t)(w >> (8u - (at & 7u)));
                if (stored != combined) { handback = true; break; }
                if (end_byte) *end_byte = (size_t)((at + 32u + 7u) >> 3);
                return 0;
            }
            if (!B.group(idx, std::min(G, cands.size() - idx), rel, level, R)) { handback = true; break; }
            uint32_t good = 0;
            for (; good < R.n && R.crc_txt[good] == R.crc_hdr[good]; ++good) combined = ((combined << 1) | (combined >> 31)) ^ R.crc_hdr[good];
            if (good) {
                if (R.off[good] && !sink(R.text, (size_t)R.off[good])) return BZ_ERR_STOPPED;
                delivered += R.off[good];
                st.dev_blocks += good; st.dev_bytes += R.off[good];
                rel = R.end_bit[good - 1];
            }
            if (good < R.n || R.stop_status == 1u /* BZB_RANDOMISED */) { handback = true; break; }
            if (R.n == 0) break;                  // the block at `rel` did not decode: cut short by the window, or damaged
            idx = (size_t)(std::lower_bound(cands.begin(), cands.end(), rel << 1) - cands.begin());
        }
        cur = (uint64_t)win0 * 8u + rel;
        for (size_t k = 0; k < cands.size(); ++k) blocks_left += (cands[k] >> 1) >= rel && !(cands[k] & 1ull) ? 1u : 0u;
        // nothing chains at `cur` in this window: slide it there if that is news to the window, else it is the host's
        if (handback || last || rel < start_rel + 128u) break;
        blocks_left = 0;
    }
    st.host_blocks += std::max<uint64_t>(blocks_left, 1u);       // (block magics from the hand-back bit on, in the window it happened in)
    uint64_t produced = 0;
    const int rc = host_decode(data, a, b, delivered, sink, end_byte, &produced, stop);
    st.host_bytes += produced;
    return rc;
}

// A decoder of whole streams that outlives one file (the device's: aqc_bunzip2_offload.hip)
struct StreamDecoder {
    virtual ~StreamDecoder() {}
    // data[a, b): one stream; its text to the sink, in order.  0, or BZ_ERR_*
    virtual int decode(const uint8_t* data, size_t a, size_t b, const Sink& sink, size_t* end_byte, StreamStats* st, const std::atomic<bool>* stop) = 0;
    virtual bool gave_up() = 0;       // a device call failed: the decoder hands every stream to libbz2 from now on
};
// group_blocks 0: sized from the buffer budget
StreamDecoder* make_device_bunzip2(int device, size_t group_blocks);
// microseconds in the scan, entropy, BWT and expand kernels and in the copies, then the BWT figure's scatter and chase parts, of
// every decoder of the process so far
void device_bunzip2_stats(uint64_t out[7]);

}  // namespace aqcbz
