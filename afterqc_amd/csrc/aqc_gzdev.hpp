// aqc_gzdev.hpp — gzip output built ON THE DEVICE: the good / bad / overlap text streams that aqc_format leaves in HBM
// become BGZF-compatible gzip members there, so `-z` output costs no host CPU and a third of the PCIe traffic
// (fastq.py:63-68 + `--compression`, after.py:91-92 upstream: Python's gzip module on the one CPU thread).
//
// The host's CPU budget is what bounds the pipe's own codec (aqc_deflate.cpp): the MI355X boxes grant a container 16 CPUs'
// worth of run time, ~4 GB/s of deflate in total — which the inflate side of a .gz -> .gz run needs for itself.
//
//   member     <= 0xff00 = 255 x 256 bytes of text -> one gzip member with the BGZF extra field, ONE final dynamic-Huffman
//              block.  A workgroup of 256 threads per member, a thread per 255-byte segment: the text is staged in LDS, every
//              thread tokenises its own segment (so no token crosses a segment border), a block scan of the segments' bit
//              counts places them, the threads write their bits (whole words stored, border words OR-ed in).
//   matches    two kinds, both found without any search structure: RUNS (distance 1: quality strings) and the SAME COLUMN OF
//              THE LINE FOUR LINES UP (the previous record's name / strand line; the distance is that line's start + column).
//              A match is taken when its code is shorter than the literals' it replaces, by the actual code lengths.
//   code       ONE literal/length + distance code per stream and launch, shared by all its members (every symbol has a code):
//              gz_hist_kernel tokenises a sample of the members, the HOST builds the code from the counts with the same
//              routines as its own encoder (aqc_deflate.cpp: code_lengths / canonical codes / run-length header) and hands back
//              the codes + the ready-made block header bits.
//   CRC-32     per segment byte-wise from a 256-entry table, then a tree of "advance by 255 * 2^k bytes" operators (32 x 32 bit
//              matrices precomputed on the host); the member's first four bytes are complemented instead of starting the
//              register at ~0, which makes leading padding harmless (the last member of a stream is right-aligned in the grid).
//   compaction member sizes -> exclusive scan per stream -> contiguous stream (gz_pack_kernel).
//
// Three encoders write this format: gz_encode_kernel (above; AQC_GZ_ENCODER=seg), gz_encode_wave_kernel (the default: a wave per
// member of 64 x 255 bytes, see there) and gz_encode_lz_kernel (aqc_gzlz.hpp, levels 6 - 9).  What they do the same way is stated
// once, in front of them: gz_member_of / gz_sample_of, gz_load_code, gz_store_member, gz_crc_segment / gz_crc_short, gz_frame_member
// for all three; gzw_open_block, gzw_parse, gzw_token_bits, gzw_ring_put, gzw_close_block, gzw_crc for the two that walk a member
// in windows of 64 bytes.  The length / distance symbols of RFC 1951 3.2.5: aqc_deflate_sym.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aqc_deflate_sym.hpp"
#include "aqc_prim.hpp"

namespace aqc {

constexpr int GZ_TEXT = 0xff00;                  // text bytes per member = GZ_THREADS * GZ_SEG
constexpr int GZ_THREADS = 256, GZ_SEG = 255;
constexpr int GZ_SLOT = 65536;                   // staging bytes per member; the member starts at byte 2 (deflate data 4-aligned)
constexpr int GZ_MAX_LINES = 4096;
constexpr int GZ_HDR_WORDS = 192;
constexpr int GZ_SAMPLES = 16;                   // pieces of GZ_TEXT bytes sampled per stream (evenly spaced)
constexpr int GZW_TEXT = 64 * 255;               // gz_encode_wave_kernel: 16320 text bytes per member
constexpr int GZW_SLOT = 16896;                  // staging bytes per member (its text stored + headers, and a window's worth of slack)
constexpr int GZW_MAX_LINES = 512;
constexpr int GZW_RING = 128;                    // staging words of a wave's bit ring

struct GzCodebookDev {
    uint32_t lit[286];       // bit-reversed code | length << 16
    uint32_t dist[30];
    uint32_t hdr[GZ_HDR_WORDS];   // BFINAL, BTYPE and the dynamic header, LSB first
    uint32_t hdr_bits;
    uint32_t pad_[3];
};

struct GzCrcTables {
    uint32_t byte_table[256];
    uint32_t shift[8][32];   // operator "advance the register by 255 * 2^k zero bytes", column j = image of bit j
};

struct GzJob {
    const uint8_t* text[6];
    uint64_t bytes[6];
    uint32_t first_block[7];     // members of stream q: [first_block[q], first_block[q + 1])
    uint8_t* stage;              // n_members * GZ_SLOT
    uint32_t* sizes;             // bytes of each member
    const GzCodebookDev* code;   // [6]
    uint32_t* hist;              // [6][320]: 286 literal/length counts, then 30 distance counts
    const GzCrcTables* crc;
    uint32_t member_text;        // text bytes per member: GZ_TEXT (gz_encode_kernel) or GZW_TEXT (gz_encode_wave_kernel)
    uint32_t slot_bytes;         // staging bytes per member: GZ_SLOT or GZW_SLOT
    uint8_t* packed[6];          // contiguous streams (gz_pack_kernel)
    uint64_t* offsets;           // [n_members] start of each member inside its packed stream; totals in total[6]
    uint64_t* total;
};

// which member is this, and of which stream
__device__ __forceinline__ int gz_stream_of(const GzJob& J, uint32_t member) {
    int q = 0;
#pragma unroll
    for (int k = 1; k < 6; ++k) q += member >= J.first_block[k] ? 1 : 0;
    return q;
}

// ---- what every encoder does the same way: the member and its frame -----------------------------------------------------------------
// member `member` of the launch, cut from its stream in pieces of member_text bytes: the stream q, the text J.text[q] + off, n bytes
__device__ __forceinline__ void gz_member_of(const GzJob& J, uint32_t member, int member_text, int& q, uint64_t& off, int& n) {
    q = gz_stream_of(J, member);
    const uint32_t local = member - J.first_block[q];
    off = (uint64_t)local * member_text;
    n = (int)min<uint64_t>(member_text, J.bytes[q] - off);
}
// workgroup (q, k) of a sampling pass: piece k * stride of stream q in pieces of GZ_TEXT bytes, whatever the encoder's members are.
// false: the stream has no such piece
__device__ __forceinline__ bool gz_sample_of(const GzJob& J, int& q, uint64_t& off, int& n) {
    q = blockIdx.x / GZ_SAMPLES;
    const int k = blockIdx.x % GZ_SAMPLES;
    const uint32_t nb = (uint32_t)((J.bytes[q] + GZ_TEXT - 1) / GZ_TEXT);
    const uint32_t stride = nb > GZ_SAMPLES ? nb / GZ_SAMPLES : 1u;
    const uint32_t local = (uint32_t)k * stride;
    off = (uint64_t)local * GZ_TEXT;
    n = (int)min<uint64_t>(GZ_TEXT, J.bytes[q] - off);
    return local < nb;
}
// the member's place in the staging buffer; its deflate data at +18 is 4-byte aligned
__device__ __forceinline__ uint8_t* gz_member_slot(const GzJob& J, uint32_t member, int slot_bytes) { return J.stage + (uint64_t)member * slot_bytes + 2; }
__device__ __forceinline__ uint32_t* gz_member_data(uint8_t* mem) { return reinterpret_cast<uint32_t*>(mem + 18); }

// the stream's code and the CRC byte table into LDS, by a workgroup of NT threads
template <int NT>
__device__ __forceinline__ void gz_load_code(const GzCodebookDev& cb, const uint32_t* byte_table, uint32_t* lc, uint32_t* dc, uint32_t* crc_tab) {
    for (int i = threadIdx.x; i < 286; i += NT) lc[i] = cb.lit[i];
    if (threadIdx.x < 30) dc[threadIdx.x] = cb.dist[threadIdx.x];
    static_assert(256 % NT == 0, "the byte table in whole rounds of the workgroup");
#pragma unroll
    for (int i = 0; i < 256; i += NT) crc_tab[i + threadIdx.x] = byte_table[i + threadIdx.x];
}

// incompressible with this code: one stored block (BFINAL = 1, BTYPE = 0, LEN, ~LEN, bytes), n + 5 bytes of deflate data
__device__ __forceinline__ void gz_store_member(uint8_t* mem, const uint8_t* text, int n, int tid, int nthreads) {
    if (tid == 0) {
        mem[18] = 1;
        mem[19] = (uint8_t)n; mem[20] = (uint8_t)(n >> 8); mem[21] = (uint8_t)~n; mem[22] = (uint8_t)(~n >> 8);
    }
    for (int i = tid; i < n; i += nthreads) mem[23 + i] = text[i];
}

// raw CRC-32 register over text[a, b) from 0, the member's first four bytes complemented: that equals starting the member's
// register at 0xffffffff, in a form zeros in front of the member do not disturb
__device__ __forceinline__ uint32_t gz_crc_segment(const uint32_t* crc_tab, const uint8_t* text, int a, int b) {
    uint32_t c = 0;
    for (int p = a; p < b; ++p) {
        uint32_t x = text[p];
        if (p < 4) x ^= 0xffu;
        c = crc_tab[(c ^ x) & 0xffu] ^ (c >> 8);
    }
    return c;
}
// the same register for a member of fewer than four bytes, where the complement trick does not apply: the plain way.  (Of all
// three functions here the CRC-32 is the complement of what they return: gz_frame_member(.., ~c, ..))
__device__ __forceinline__ uint32_t gz_crc_short(const uint32_t* crc_tab, const uint8_t* text, int n) {
    uint32_t c = 0xffffffffu;
    for (int p = 0; p < n; ++p) c = crc_tab[(c ^ text[p]) & 0xffu] ^ (c >> 8);
    return c;
}

// the BGZF header in front of dbytes of deflate data and the trailer (CRC-32, ISIZE) behind them.  -> bytes of the member
__device__ __forceinline__ uint32_t gz_frame_member(uint8_t* mem, uint32_t dbytes, uint32_t crc, int n) {
    const uint32_t bsize = 18u + dbytes + 8u;
    static const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) mem[i] = hdr[i];
    mem[16] = (uint8_t)((bsize - 1) & 0xffu);
    mem[17] = (uint8_t)((bsize - 1) >> 8);
    uint8_t* t = mem + 18 + dbytes;
    for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
    return bsize;
}

// ---- what the two one-wave-per-member encoders (gz_encode_wave_kernel, gz_encode_lz_kernel) do the same way: a window of 64
// consecutive bytes, a lane per byte, is parsed into tokens, the tokens' bits go through a ring of GZW_RING words in LDS to the
// member, front to back ------------------------------------------------------------------------------------------------------------
// bits of the lanes before this one
__device__ __forceinline__ unsigned long long gzw_lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// the block header: the ring emptied, whole words straight to the member, the partial one opens the ring.  -> the bit position
__device__ __forceinline__ uint32_t gzw_open_block(const GzCodebookDev& cb, uint32_t* dwords, uint32_t* ring, int lane) {
    const uint32_t hdr_bits = cb.hdr_bits;
    static_assert(GZW_RING == 2 * WAVE, "two ring words per lane");
#pragma unroll
    for (int r = 0; r < 2; ++r) ring[lane + WAVE * r] = 0;
    for (uint32_t i = (uint32_t)lane; i < (hdr_bits >> 5); i += WAVE) dwords[i] = cb.hdr[i];
    if (lane == 0 && (hdr_bits & 31u)) ring[0] = cb.hdr[hdr_bits >> 5] & ((1u << (hdr_bits & 31u)) - 1u);
    return hdr_bits;
}

// the greedy parse: the lanes of this window a token starts at.  vmask = lanes inside the member, blen = the token a lane would
// start (1: a literal), `skip` = bytes at the window's front that an earlier token covers (< 64), carried on to the next window.
// A walk over the token starts with scalar steps; a window without a match takes none: every lane is a literal
__device__ __forceinline__ unsigned long long gzw_parse(unsigned long long vmask, bool has_match, int blen, int& skip) {
    unsigned long long marks;
    int e = skip;
    if (!has_match) {
        marks = vmask & ~((1ull << skip) - 1ull);
        e = 64;
    } else {
        marks = 0;
        const int last = 64 - (int)__builtin_clzll(vmask | 1ull);        // one behind the last valid lane
        while (e < last) {
            marks |= 1ull << e;
            e += __builtin_amdgcn_readlane(blen, e);
        }
        if (e < 64) e = 64;                                              // (the member ends inside this window)
    }
    skip = e - 64;
    return marks;
}

// a lane's token in bits (tok: it has one): the literal `lit`, or length blen > 1 at distance dist; and the lane scan that places it
struct GzwBits {
    unsigned long long bits;     // LSB first
    uint32_t nb;                 // how many (<= 48)
    uint32_t inc, total;         // inclusive sum of nb over the lanes; the window's sum
};
__device__ __forceinline__ GzwBits gzw_token_bits(const uint32_t* lc, const uint32_t* dc, bool tok, uint32_t lit, int blen, int dist, int lane) {
    GzwBits t{0, 0, 0, 0};
    if (tok) {
        if (blen == 1) {
            const uint32_t a = lc[lit];
            t.bits = a & 0xffffu; t.nb = a >> 16;
        } else {
            const int lsym = len_sym(blen), dsym = dist_sym(dist);
            const uint32_t a = lc[257 + lsym], d = dc[dsym];
            t.bits = a & 0xffffu; t.nb = a >> 16;
            t.bits |= (unsigned long long)(uint32_t)(blen - len_base(lsym)) << t.nb; t.nb += (uint32_t)len_extra(lsym);
            t.bits |= (unsigned long long)(d & 0xffffu) << t.nb; t.nb += d >> 16;
            t.bits |= (unsigned long long)(uint32_t)(dist - dist_base(dsym)) << t.nb; t.nb += (uint32_t)dist_extra(dsym);
        }
    }
    t.inc = wave_incl_sum_shfl(t.nb, lane);
    t.total = (uint32_t)__builtin_amdgcn_readlane((int)t.inc, 63);
    return t;
}

// the window's bits into the ring at bitpos (OR-ed: neighbours share words), whole words out to the member with one coalesced store
// per lane, the open word to the ring's front; bitpos moves on.  t.total <= 64 x 48 bits = 96 words: the ring holds them
__device__ __forceinline__ void gzw_ring_put(uint32_t* ring, uint32_t* dwords, uint32_t& bitpos, bool tok, const GzwBits& t, int lane) {
    if (tok) {
        const uint32_t at = bitpos + t.inc - t.nb;
        const uint32_t wi = (at >> 5) - (bitpos >> 5), sh = at & 31u;
        const unsigned long long lo = t.bits << sh;
        atomicOr(&ring[wi], (uint32_t)lo);
        if (sh + t.nb > 32u) atomicOr(&ring[wi + 1], (uint32_t)(lo >> 32));
        if (sh + t.nb > 64u) atomicOr(&ring[wi + 2], (uint32_t)(t.bits >> (64u - sh)));
    }
    const uint32_t w0 = bitpos >> 5, w1 = (bitpos + t.total) >> 5, nfull = w1 - w0;
    __builtin_amdgcn_s_waitcnt(0xc07f);                                  // lgkmcnt(0): the ring's atomics are done
    uint32_t keep[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t j = (uint32_t)lane + 64u * (uint32_t)r;
        keep[r] = ring[j];
        if (j < nfull) dwords[w0 + j] = keep[r];
    }
    const uint32_t open = nfull < (uint32_t)GZW_RING ? (uint32_t)__builtin_amdgcn_readlane((int)keep[nfull >> 6], (int)(nfull & 63u)) : 0u;
#pragma unroll
    for (int r = 0; r < 2; ++r) ring[(uint32_t)lane + 64u * (uint32_t)r] = 0;
    if (lane == 0) ring[0] = open;
    bitpos += t.total;
}

// behind the last window: end of block and the open word, unless the member is `stored` already; a stored block when that is no
// larger.  -> bytes of deflate data
__device__ __forceinline__ uint32_t gzw_close_block(const uint32_t* ring, const uint32_t* lc, uint8_t* mem, const uint8_t* text, uint32_t bitpos, int n, int lane, bool stored) {
    uint32_t dbytes = 0;
    if (!stored) {
        uint32_t* const dwords = gz_member_data(mem);
        const uint32_t eob = lc[256];
        if (lane == 0) {
            const uint32_t sh = bitpos & 31u;
            const unsigned long long v = (unsigned long long)ring[0] | ((unsigned long long)(eob & 0xffffu) << sh);
            dwords[bitpos >> 5] = (uint32_t)v;
            if (sh + (eob >> 16) > 32u) dwords[(bitpos >> 5) + 1] = (uint32_t)(v >> 32);
        }
        bitpos += eob >> 16;
        dbytes = (bitpos + 7u) >> 3;
        stored = dbytes >= (uint32_t)n + 5u;
    }
    if (stored) {
        dbytes = (uint32_t)n + 5u;
        gz_store_member(mem, text, n, lane, WAVE);
    }
    return dbytes;
}

// CRC-32 register of the member's text[0, n): the member right-aligned in a grid of segments of GZ_SEG bytes, a lane takes 2^K0 of them
// (gz_crc_segment), then the combine tree over the lanes from the operator "advance by 2^K0 x 255 bytes" (T.shift[K0]) on
template <int K0>
__device__ __forceinline__ uint32_t gzw_crc(const uint8_t* text, int n, const uint32_t* crc_tab, const GzCrcTables& T, int lane) {
    constexpr int PER_LANE = GZ_SEG << K0;
    const int pad = WAVE * PER_LANE - n;
    uint32_t c = gz_crc_segment(crc_tab, text, max(0, lane * PER_LANE - pad), max(0, (lane + 1) * PER_LANE - pad));
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const int step = 1 << k;
        const uint32_t right = (uint32_t)__shfl_down((int)c, step);
        if ((lane & (2 * step - 1)) == 0) {
            const uint32_t* M = T.shift[k + K0];
            uint32_t r = right;
            for (int j = 0; j < 32; ++j) r ^= ((c >> j) & 1u) ? M[j] : 0u;
            c = r;
        }
    }
    return c;
}

// ---- gz_encode_kernel's tokens: a thread per 255-byte segment ------------------------------------------------------------------------
struct GzSinkHist {
    uint32_t* h;     // LDS [320]
    __device__ __forceinline__ void lit(uint32_t b) { atomicAdd(&h[b], 1u); }
    __device__ __forceinline__ void match(int len, int dist) { atomicAdd(&h[257 + len_sym(len)], 1u); atomicAdd(&h[286 + dist_sym(dist)], 1u); }
};
struct GzSinkSize {
    const uint32_t* lc; const uint32_t* dc;     // LDS codebook
    uint32_t bits = 0;
    __device__ __forceinline__ void lit(uint32_t b) { bits += lc[b] >> 16; }
    __device__ __forceinline__ void match(int len, int dist) {
        const int ls = len_sym(len), ds = dist_sym(dist);
        bits += (lc[257 + ls] >> 16) + len_extra(ls) + (dc[ds] >> 16) + dist_extra(ds);
    }
};
struct GzSinkEmit {
    const uint32_t* lc; const uint32_t* dc;
    uint32_t* out;            // deflate data as words (zeroed)
    uint32_t w;               // next word
    unsigned long long acc = 0;
    int nacc;
    bool first = true;
    __device__ __forceinline__ void flush_words() {
        while (nacc >= 32) {
            const uint32_t v = (uint32_t)acc;
            if (first) { atomicOr(&out[w], v); first = false; }
            else out[w] = v;
            ++w;
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void put(uint32_t code, int len) { acc |= (unsigned long long)code << nacc; nacc += len; flush_words(); }
    __device__ __forceinline__ void lit(uint32_t b) { const uint32_t c = lc[b]; put(c & 0xffffu, (int)(c >> 16)); }
    __device__ __forceinline__ void match(int len, int dist) {
        const int ls = len_sym(len), ds = dist_sym(dist);
        const uint32_t a = lc[257 + ls], d = dc[ds];
        put(a & 0xffffu, (int)(a >> 16));
        if (len_extra(ls)) put((uint32_t)(len - len_base(ls)), len_extra(ls));
        put(d & 0xffffu, (int)(d >> 16));
        if (dist_extra(ds)) put((uint32_t)(dist - dist_base(ds)), dist_extra(ds));
    }
    __device__ __forceinline__ void finish() { if (nacc > 0) atomicOr(&out[w], (uint32_t)acc); }
};

// What the size pass decided, for the emit pass: bit i of `start` = a token begins at byte a + i of the segment (its length is the
// distance to the next one: 1 = literal, >= 3 = match), bit i of `col` = that match copies the column four lines up (else the
// byte before: distance 1), bit i of `nl` = byte a + i is a line end.  Four 64-bit words each, never indexed by a variable (that
// would put them in scratch memory): the emit pass costs a few instructions per TOKEN instead of the whole search per byte again.
struct GzTokMask {
    unsigned long long start[4] = {0, 0, 0, 0}, col[4] = {0, 0, 0, 0}, nl[4] = {0, 0, 0, 0};
};
__device__ __forceinline__ void gz_mask_set(unsigned long long (&m)[4], int i) {
    const unsigned long long bit = 1ull << (i & 63);
    const int w = i >> 6;
    m[0] |= w == 0 ? bit : 0ull; m[1] |= w == 1 ? bit : 0ull; m[2] |= w == 2 ? bit : 0ull; m[3] |= w == 3 ? bit : 0ull;
}
__device__ __forceinline__ bool gz_mask_test(const unsigned long long (&m)[4], int i) {
    const int w = i >> 6;
    const unsigned long long v = w == 0 ? m[0] : w == 1 ? m[1] : w == 2 ? m[2] : m[3];
    return (v >> (i & 63)) & 1ull;
}
// set bits below position i
__device__ __forceinline__ int gz_mask_count_below(const unsigned long long (&m)[4], int i) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int k = i - 64 * w;                          // bits of word w below i: all (k >= 64), none (k <= 0), the low k
        const unsigned long long v = k >= 64 ? m[w] : k <= 0 ? 0ull : m[w] & ((1ull << k) - 1ull);
        c += __popcll(v);
    }
    return c;
}

// Tokens of the segment s[a, b) of a member's text s[0, n): the same decisions whatever the sink.  EXACT: matches are judged
// by the code lengths (size / emit passes, which therefore agree); otherwise by fixed thresholds (the sampling pass, before a
// code exists).  ls[0 .. n_lines) = line starts (ls[l + 1] - 1 is line l's '\n'), line = index of the line position `a` is in.
template <bool EXACT, class Sink, bool REC = false>
__device__ __forceinline__ void gz_tokenize(const uint8_t* s, int a, int b, int line, const uint16_t* ls, int n_lines, bool use_lines,
                                            const uint32_t* lc, const uint32_t* dc, Sink& sink, GzTokMask* rec = nullptr) {
    int p = a;
    while (p < b) {
        const uint32_t c0 = s[p];
        int best_len = 0, best_dist = 0, best_gain = 0;
        // a run of the byte before
        if (p > 0 && c0 == s[p - 1]) {
            int r = 1;
            const int lim = min(b - p, 258);
            while (r < lim && s[p + r] == c0) ++r;
            if (r >= 3) {
                int gain;
                if (EXACT) {
                    const int lsym = len_sym(r);
                    gain = r * (int)(lc[c0] >> 16) - (int)((lc[257 + lsym] >> 16) + len_extra(lsym) + (dc[0] >> 16));
                } else gain = r >= 5 ? r : 0;
                if (gain > best_gain) { best_gain = gain; best_len = r; best_dist = 1; }
            }
        }
        // the same column four lines up
        if (use_lines && line >= 4) {
            const int q0 = (int)ls[line - 4] + (p - (int)ls[line]);
            const int dist = p - q0;
            if (q0 < (int)ls[line - 3] && dist <= 32768 && s[q0] == c0) {
                int m = 1, lit_bits = EXACT ? (int)(lc[c0] >> 16) : 0;
                const int lim = min(b - p, 258);
                while (m < lim && s[p + m] == s[q0 + m]) { if (EXACT) lit_bits += (int)(lc[s[p + m]] >> 16); ++m; }
                if (m >= 3) {
                    int gain;
                    if (EXACT) {
                        const int lsym = len_sym(m), dsym = dist_sym(dist);
                        gain = lit_bits - (int)((lc[257 + lsym] >> 16) + len_extra(lsym) + (dc[dsym] >> 16) + dist_extra(dsym));
                    } else gain = m >= 6 ? m : 0;
                    if (gain > best_gain) { best_gain = gain; best_len = m; best_dist = dist; }
                }
            }
        }
        if (REC) {
            gz_mask_set(rec->start, p - a);
            if (best_len && best_dist != 1) gz_mask_set(rec->col, p - a);
        }
        if (best_len) {
            sink.match(best_len, best_dist);
            if (use_lines)
                for (int i = 0; i < best_len; ++i) {
                    const bool e = s[p + i] == '\n';
                    line += e ? 1 : 0;
                    if (REC && e) gz_mask_set(rec->nl, p + i - a);
                }
            p += best_len;
        } else {
            sink.lit(c0);
            const bool e = use_lines && c0 == '\n';
            line += e ? 1 : 0;
            if (REC && e) gz_mask_set(rec->nl, p - a);
            ++p;
        }
        if (line >= n_lines) line = n_lines - 1;       // (cannot happen: kept so that a bad table can never index past ls)
    }
}

// The emit pass: the tokens the size pass recorded, replayed.  line_a = the line byte `a` is in.
template <class Sink>
__device__ __forceinline__ void gz_replay(const uint8_t* s, int a, int b, int line_a, const uint16_t* ls, const GzTokMask& M, Sink& sink) {
    const int nseg = b - a;
    int prev = -1;                       // start of the token waiting for its end
    auto emit = [&](int at, int len) {
        if (len == 1) { sink.lit(s[a + at]); return; }
        int dist = 1;
        if (gz_mask_test(M.col, at)) {
            const int p = a + at;
            const int line = line_a + gz_mask_count_below(M.nl, at);
            dist = p - ((int)ls[line - 4] + (p - (int)ls[line]));
        }
        sink.match(len, dist);
    };
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        unsigned long long m = M.start[w];
        while (m) {
            const int at = 64 * w + (int)__builtin_ctzll(m);
            m &= m - 1;
            if (prev >= 0) emit(prev, at - prev);
            prev = at;
        }
    }
    if (prev >= 0) emit(prev, nseg - prev);
}

// text of one member into LDS + its line table.  The member's n bytes are RIGHT-aligned in the 256 x 255 grid: thread t owns
// the text bytes [seg_a, seg_b) = grid positions [255 t, 255 (t + 1)) minus the padding in front.
struct alignas(16) GzStage {
    uint8_t text[GZ_TEXT + 16];
    uint16_t ls[GZ_MAX_LINES + 8];
    uint32_t scan[GZ_THREADS / WAVE + 1];
    uint32_t n_lines;
};

__device__ __forceinline__ uint32_t gz_block_excl_scan(uint32_t v, uint32_t* lds /* [5] */, uint32_t& total) {
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const uint32_t inc = wave_incl_sum_shfl(v, lane);
    __syncthreads();
    if (lane == WAVE - 1) lds[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < GZ_THREADS / WAVE; ++w) {
        const uint32_t t = lds[w];
        if (w < wave) base += t;
        total += t;
    }
    return base + inc - v;
}

// returns this thread's segment [a, b), the line its first byte is in, and whether the line table is usable
__device__ __forceinline__ void gz_stage_member(GzStage& S, const uint8_t* src, int n, int& a, int& b, int& line, bool& use_lines) {
    for (int i = threadIdx.x * 16; i < n; i += GZ_THREADS * 16) {
        const uint4 v = load16u(src + i);        // (the formatted streams are followed by 64 readable bytes)
        *reinterpret_cast<uint4*>(S.text + i) = v;
    }
    const int pad = GZ_TEXT - n;
    a = max(0, (int)threadIdx.x * GZ_SEG - pad);
    b = max(0, ((int)threadIdx.x + 1) * GZ_SEG - pad);
    __syncthreads();
    uint32_t nl = 0;
    for (int p = a; p < b; ++p) nl += S.text[p] == '\n' ? 1u : 0u;
    uint32_t total;
    const uint32_t before = gz_block_excl_scan(nl, S.scan, total);
    // line starts: ls[0] = 0, ls[k] = position behind the k-th '\n'
    use_lines = total + 2 <= GZ_MAX_LINES;
    if (threadIdx.x == 0) { S.ls[0] = 0; S.n_lines = total + 1; }
    if (use_lines) {
        uint32_t k = before + 1;
        for (int p = a; p < b; ++p)
            if (S.text[p] == '\n') S.ls[k++] = (uint16_t)(p + 1);
    }
    line = (int)before;
    __syncthreads();
    if (use_lines && threadIdx.x == 0) S.ls[total + 1] = (uint16_t)n;      // (sentinel: end of the last line)
    __syncthreads();
}

// ---- sampling pass: symbol counts of some members of every stream -------------------------------------------------------------
__global__ __launch_bounds__(GZ_THREADS) void gz_hist_kernel(GzJob J) {
    __shared__ GzStage S;
    __shared__ uint32_t h[320];
    int q, n; uint64_t off;
    if (!gz_sample_of(J, q, off, n)) return;
    for (int i = threadIdx.x; i < 320; i += GZ_THREADS) h[i] = 0;
    int a, b, line; bool use_lines;
    gz_stage_member(S, J.text[q] + off, n, a, b, line, use_lines);
    GzSinkHist sink{h};
    gz_tokenize<false>(S.text, a, b, line, S.ls, (int)S.n_lines, use_lines, nullptr, nullptr, sink);
    __syncthreads();
    for (int i = threadIdx.x; i < 320; i += GZ_THREADS)
        if (h[i]) atomicAdd(&J.hist[q * 320 + i], h[i]);
}

// ---- one gzip member per workgroup ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GZ_THREADS) void gz_encode_kernel(GzJob J) {
    __shared__ GzStage S;
    __shared__ uint32_t lc[286], dc[30];
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t crc_part[GZ_THREADS];
    const uint32_t member = blockIdx.x;
    int q, n; uint64_t off;
    gz_member_of(J, member, GZ_TEXT, q, off, n);
    const GzCodebookDev& cb = J.code[q];
    gz_load_code<GZ_THREADS>(cb, J.crc->byte_table, lc, dc, crc_tab);
    int a, b, line; bool use_lines;
    gz_stage_member(S, J.text[q] + off, n, a, b, line, use_lines);
    // ---- sizes -> positions
    GzSinkSize sz{lc, dc};
    GzTokMask tm;
    gz_tokenize<true, GzSinkSize, true>(S.text, a, b, line, S.ls, (int)S.n_lines, use_lines, lc, dc, sz, &tm);
    uint32_t total_bits;
    const uint32_t my_bit = gz_block_excl_scan(sz.bits, S.scan, total_bits);
    const uint32_t hdr_bits = cb.hdr_bits;
    const uint32_t eob = lc[256];
    const uint32_t all_bits = hdr_bits + total_bits + (eob >> 16);
    uint32_t dbytes = (all_bits + 7) >> 3;
    const bool stored = dbytes >= (uint32_t)n + 5u;
    if (stored) dbytes = (uint32_t)n + 5u;
    uint8_t* const mem = gz_member_slot(J, member, GZ_SLOT);
    uint32_t* const dwords = gz_member_data(mem);
    if (!stored) {
        const uint32_t nw = (all_bits + 31) >> 5;
        for (uint32_t i = threadIdx.x; i <= nw; i += GZ_THREADS) dwords[i] = 0;
        __threadfence();
        __syncthreads();
        GzSinkEmit em{lc, dc, dwords, (hdr_bits + my_bit) >> 5};
        em.nacc = (int)((hdr_bits + my_bit) & 31u);
        gz_replay(S.text, a, b, line, S.ls, tm, em);
        if (threadIdx.x == GZ_THREADS - 1) em.put(eob & 0xffffu, (int)(eob >> 16));       // end of block, behind the last segment
        em.finish();
        // the shared block header: whole words stored, the last (partial) one OR-ed in
        for (uint32_t i = threadIdx.x; i * 32 < hdr_bits; i += GZ_THREADS) {
            const uint32_t v = cb.hdr[i];
            if ((i + 1) * 32 <= hdr_bits) atomicOr(&dwords[i], v);         // (word 0 .. may be shared with nobody, OR is simply safe)
            else atomicOr(&dwords[i], v & ((1u << (hdr_bits & 31u)) - 1u));
        }
    } else gz_store_member(mem, S.text, n, (int)threadIdx.x, GZ_THREADS);
    // ---- CRC-32 of the member's text: raw CRCs of the 256 grid segments, combined through LDS
    {
        crc_part[threadIdx.x] = gz_crc_segment(crc_tab, S.text, a, b);
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < 8; ++k) {
            const int step = 1 << k;
            uint32_t r = 0;
            const bool active = (threadIdx.x & (2 * step - 1)) == 0;
            if (active) {
                const uint32_t left = crc_part[threadIdx.x];
                const uint32_t* M = J.crc->shift[k];
                for (int j = 0; j < 32; ++j) r ^= ((left >> j) & 1u) ? M[j] : 0u;
                r ^= crc_part[threadIdx.x + step];
            }
            __syncthreads();
            if (active) crc_part[threadIdx.x] = r;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        uint32_t c = crc_part[0];
        if (n < 4) c = gz_crc_short(crc_tab, S.text, n);
        J.sizes[member] = gz_frame_member(mem, dbytes, ~c, n);
    }
}

// ---- member sizes -> offsets inside each packed stream (one workgroup per stream) ------------------------------------------------
__global__ __launch_bounds__(GZ_THREADS) void gz_offsets_kernel(GzJob J) {
    __shared__ unsigned long long lds[4];
    const int q = blockIdx.x;
    const uint32_t m0 = J.first_block[q], m1 = J.first_block[q + 1];
    unsigned long long carry = 0;
    for (uint32_t t0 = m0; t0 < m1; t0 += GZ_THREADS) {
        const uint32_t m = t0 + threadIdx.x;
        const unsigned long long v = m < m1 ? (unsigned long long)J.sizes[m] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_excl_scan(v, lds, total);
        if (m < m1) J.offsets[m] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) J.total[q] = carry;
}

__global__ __launch_bounds__(GZ_THREADS) void gz_pack_kernel(GzJob J) {
    const uint32_t member = blockIdx.x;
    const int q = gz_stream_of(J, member);
    const uint8_t* src = J.stage + (uint64_t)member * J.slot_bytes + 2;
    uint8_t* dst = J.packed[q] + J.offsets[member];
    const int n = (int)J.sizes[member];
    for (int i = threadIdx.x * 16; i < n; i += GZ_THREADS * 16) {
        if (i + 16 <= n) store16u(dst + i, load16u(src + i));
        else for (int k = i; k < n; ++k) dst[k] = src[k];
    }
}


// ---- round 6: one gzip member per WAVE, 64 bytes per step ------------------------------------------------------------------------
// gz_encode_kernel gives every thread 255 bytes of its own: 64 lanes, each in a state of its own (inside a run, comparing a column,
// emitting a literal) — the wave executes every path for every step, 142 K vector instructions per wave and 16 KB, and a
// .gz -> .gz run spends a third of the GPU's time in it (profiles/r06_gz_prof_summary.txt).  Here a wave owns a member of
// GZW_TEXT = 64 x 255 bytes and walks it in windows of 64 consecutive bytes, a lane per byte:
//   * what can match — the byte before (runs), the same column four lines up — is one comparison per lane and a ballot: a match's
//     length is the run of ones in that mask from the lane's bit on (masks of the next four windows are kept ahead, so a match may
//     be 258 long; a column match ends with its line);
//   * the greedy parse is a walk over the window's token starts with scalar steps (v_readlane of "my token ends at"); a window
//     without a match — the bases of a read — takes none: every lane is a literal;
//   * the tokens' bits are placed by a lane scan of their lengths and OR-ed into a 128-word staging ring in LDS, whole words go out
//     to the member with one coalesced store per lane.  The wave writes its member front to back: no sizing pass.
// Same format as before — BGZF-compatible members, ONE final dynamic block with the stream's shared code, stored when that is
// smaller — with members a quarter the size: +~2.5 % bytes (header and code per 16 KB, no column match in a member's first record).
__device__ __forceinline__ int gzw_ctz64(unsigned long long x) { return x ? (int)__builtin_ctzll(x) : 64; }
// ones of the masks M[0..5) from bit l of M[0] on, up to the first zero
__device__ __forceinline__ int gzw_ones_from(const unsigned long long (&M)[5], int l) {
    int t = gzw_ctz64(~(M[0] >> l) | (l ? 0ull : 0ull));
    if (l == 0 && M[0] == ~0ull) t = 64;
    bool go = t >= 64 - l;
    t = min(t, 64 - l);
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const int ck = gzw_ctz64(~M[k]);            // (wave-uniform)
        if (go) { t += ck; go = ck == 64; }
    }
    return t;
}
// zeros of the masks from bit l of M[0] on, up to the first one (the distance to the next set bit)
__device__ __forceinline__ int gzw_zeros_from(const unsigned long long (&M)[5], int l) {
    const unsigned long long x = M[0] >> l;
    int t = x ? (int)__builtin_ctzll(x) : 64 - l;
    bool go = x == 0;
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const int ck = gzw_ctz64(M[k]);
        if (go) { t += ck; go = ck == 64; }
    }
    return t;
}

struct alignas(16) GzwStage {
    uint8_t text[GZW_TEXT + 64];
    uint16_t ls[GZW_MAX_LINES];
    uint32_t lc[286], dc[30];
    uint32_t crc_tab[256];
    uint32_t ring[GZW_RING];
};

__global__ __launch_bounds__(WAVE) void gz_encode_wave_kernel(GzJob J) {
    __shared__ GzwStage S;
    const int lane = (int)threadIdx.x;
    const uint32_t member = blockIdx.x;
    int q, n; uint64_t off;
    gz_member_of(J, member, GZW_TEXT, q, off, n);
    const GzCodebookDev& cb = J.code[q];
    gz_load_code<WAVE>(cb, J.crc->byte_table, S.lc, S.dc, S.crc_tab);
    {
        const uint8_t* src = J.text[q] + off;
        for (int i = lane * 16; i < n; i += WAVE * 16) *reinterpret_cast<uint4*>(S.text + i) = load16u(src + i);      // (64 readable bytes follow a stream)
        // what lies behind the member's end never matches anything
        for (int i = n + lane; i < ((n + 15) & ~15) + 64 && i < GZW_TEXT + 64; i += WAVE) S.text[i] = 0;
    }
    if (lane == 0) S.ls[0] = 0;
    __syncthreads();
    uint8_t* const mem = gz_member_slot(J, member, GZW_SLOT);
    uint32_t* const dwords = gz_member_data(mem);
    const unsigned long long lt = gzw_lanes_below(lane);
    uint32_t bitpos = gzw_open_block(cb, dwords, S.ring, lane);
    // beyond this a stored block is smaller; tested AFTER a window is written: GZW_SLOT has a window's worth of slack
    const uint32_t limit_bits = ((uint32_t)n + 5u) * 8u;
    bool stored = false;
    // ---- masks of window f: what matches its predecessor byte, what matches the column four lines up, where lines end
    unsigned long long M1[5], Mc[5], NL[5];
    int line_far = 0;                                                        // line of window f's first byte
    bool use_lines = true;
    auto far_masks = [&](int f, unsigned long long& m1, unsigned long long& mc, unsigned long long& nlm) {
        const int p = 64 * f + lane;
        const bool valid = p < n;
        const uint32_t c = valid ? S.text[p] : 0u;
        const uint32_t prev = (valid && p > 0) ? S.text[p - 1] : 0x100u;
        const bool nl = valid && c == '\n';
        nlm = __ballot(nl);
        m1 = __ballot(valid && c == prev);
        const int line = line_far + __popcll(nlm & lt);
        // this window's line ends become line starts (a later lane of this very window may need the one an earlier lane writes)
        if (nl && line + 1 < GZW_MAX_LINES) S.ls[line + 1] = (uint16_t)(p + 1);
        bool eq = false;
        if (valid && line >= 4 && line < GZW_MAX_LINES) {
            const int l0 = (int)S.ls[line], l4 = (int)S.ls[line - 4], l3 = (int)S.ls[line - 3];
            const int q0 = l4 + (p - l0);
            eq = q0 < l3 && S.text[q0] == c;
        }
        mc = __ballot(eq);
        line_far += __popcll(nlm);
        if (line_far >= GZW_MAX_LINES - 1) use_lines = false;               // (too many short lines: no column matches from here on)
    };
    const int n_win = (n + 63) >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) far_masks(k, M1[k], Mc[k], NL[k]);
    int line_cur = 0, skip = 0;
    for (int w = 0; w < n_win && !stored; ++w) {
        const int p = 64 * w + lane;
        const bool valid = p < n;
        if (skip >= 64) skip -= 64;
        else {
            const uint32_t c = valid ? S.text[p] : 0u;
            // ---- the best match at every byte
            int blen = 1, dist = 0;
            {
                const uint32_t lb = S.lc[c] >> 16;
                const int r = min(gzw_ones_from(M1, lane), 258);
                int best_gain = 0;
                if (r >= 3) {
                    const int lsym = len_sym(r);
                    const int gain = r * (int)lb - (int)((S.lc[257 + lsym] >> 16) + len_extra(lsym) + (S.dc[0] >> 16));
                    if (gain > 0) { best_gain = gain; blen = r; dist = 1; }
                }
                if (use_lines && ((Mc[0] >> lane) & 1ull)) {
                    const int m = min(min(gzw_ones_from(Mc, lane), gzw_zeros_from(NL, lane) + 1), 258);
                    if (m >= 3) {
                        const int line = line_cur + __popcll(NL[0] & lt);
                        const int d = (int)S.ls[line] - (int)S.ls[line - 4];
                        const int lsym = len_sym(m), dsym = dist_sym(d);
                        // (the literals' bits taken as the first one's: exact for the long matches of a name against the name before
                        //  it would need the window's prefix sums and four more windows' — the decision is not close there)
                        const int gain = m * (int)max(lb, 5u) - (int)((S.lc[257 + lsym] >> 16) + len_extra(lsym) + (S.dc[dsym] >> 16) + dist_extra(dsym));
                        if (gain > best_gain) { best_gain = gain; blen = m; dist = d; }
                    }
                }
            }
            // ---- the greedy parse, the tokens' bits, the ring
            const unsigned long long marks = gzw_parse(__ballot(valid), __ballot(valid && blen > 1) != 0ull, blen, skip);
            const bool tok = (marks >> lane) & 1ull;
            const GzwBits t = gzw_token_bits(S.lc, S.dc, tok, c, blen, dist, lane);
            gzw_ring_put(S.ring, dwords, bitpos, tok, t, lane);
            if (bitpos > limit_bits) stored = true;
        }
        // ---- the masks move on by a window
        line_cur += __popcll(NL[0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) { M1[k] = M1[k + 1]; Mc[k] = Mc[k + 1]; NL[k] = NL[k + 1]; }
        far_masks(w + 5, M1[4], Mc[4], NL[4]);
    }
    const uint32_t dbytes = gzw_close_block(S.ring, S.lc, mem, S.text, bitpos, n, lane, stored);
    static_assert(GZW_TEXT == WAVE * GZ_SEG, "a segment of the CRC grid per lane");
    uint32_t c = gzw_crc<0>(S.text, n, S.crc_tab, *J.crc, lane);
    if (lane == 0) {
        if (n < 4) c = gz_crc_short(S.crc_tab, S.text, n);
        J.sizes[member] = gz_frame_member(mem, dbytes, ~c, n);
    }
}

}  // namespace aqc
