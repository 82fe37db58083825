// aqc_bunzip2_dev.hpp — bzip2 INPUT decoded on the device: the unit of work is the bzip2 BLOCK (fastq.py:25-26 upstream:
// bz2.BZ2File on the one CPU thread).
//
// A bzip2 stream is a chain of independent blocks of at most level x 100,000 bytes: each starts with a 48-bit magic at an
// arbitrary bit position and carries its own Huffman tables, BWT origin and CRC.  So:
//
//   bzb_scan_kernel     EVERY bit position of the uploaded window is tested for the block magic and the end-of-stream magic
//                       (a lane per 8 bytes = 64 positions); the hits are appended to a list ...
//   bzb_sort_kernel     ... and ranked into one sorted candidate list (position << 1 | end-of-stream).
//   bzb_entropy_kernel  a WAVE per candidate (its tables in LDS, BzbTables: 6,032 bytes — 27 such workgroups would fit the 160 KB
//                       of a CU, so LDS is not the limit: the CU's slots for one-wave workgroups are): header, symbol map,
//                       selectors, code lengths, then the Huffman decode with a table switch every 50 symbols, MTF and RUNA / RUNB undone on the way — the block's BWT bytes, its 256 byte counts and the bit
//                       it ends on.  The chain bit -> code -> next bit is serial: one lane reads, the parallelism is the number
//                       of blocks in flight.
//   bzb_scatter_kernel  a wave per candidate: the successor vector from the counts (stable counting sort: tt[j] = i << 8 | byte,
//                       plain stores);
//   bzb_chase_kernel    ... the chase from origPtr for nblock steps (dependent loads: the stage to watch, timed on its own);
//   bzb_size_kernel     ... and the size the block has once its RLE1 runs are expanded (a block that ends on a run of four with
//                       no count byte behind it is damaged: it does not chain).
//   bzb_chain_kernel    one lane: from the bit the previous group ended on it follows  end of block == start of a candidate,
//                       keeps what decoded, and sums the expanded sizes into the blocks' places in the group's text.
//   bzb_expand_kernel   a wave per chained block: the runs expanded into the group's contiguous text, bzip2's CRC-32 (polynomial
//                       0x04c11db7, MSB first) computed on the way.
//
// A candidate is never trusted on its own: a block counts only if it starts at the very bit its predecessor ended on and its
// CRC matches (the host checks the latter and the stream's combined CRC: aqc_bz2.hpp).  A randomised block (an encoder option
// no bzip2 since 0.9.5 writes) is not decoded here: it ends the chain and the host takes over.
//
// Every loop is bounded by the block (its size, level x 100,000, or the widths of its header's fields: bzb_entropy_block),
// the scan and the sort by the window: damaged input ends in a status.
//
// Everything a LANE does is a plain __host__ __device__ function (BZB_HD): tests/native/bzb_selftest.cpp compiles this header
// with the host compiler and deals the same functions out with plain loops (`-m "not gpu"`); the kernels below only deal the
// work out.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BZB_HD __host__ __device__
#else
#define BZB_HD
#endif

namespace aqc {

constexpr uint64_t BZB_MAGIC_BLOCK = 0x314159265359ull, BZB_MAGIC_EOS = 0x177245385090ull;
constexpr uint32_t BZB_MAX_SELECTORS = 18002u, BZB_SEL_BYTES = 18016u, BZB_MAX_ALPHA = 258u, BZB_MAX_LEN = 20u, BZB_G_SIZE = 50u, BZB_MAX_DELTAS = 64u;
constexpr uint32_t BZB_PAD = 16u;              // zero bytes behind the window's last byte (the bit reader loads 8 bytes at a time)
constexpr int BZB_SCAN_THREADS = 256;
// a block's status
constexpr uint32_t BZB_OK = 0u, BZB_RANDOMISED = 1u, BZB_BAD = 2u, BZB_PAST_END = 3u, BZB_EOS = 4u;

struct BzbBlock {
    uint64_t end_bit;            // the bit behind the block's last code (where the next block's magic must stand)
    uint64_t out_size;           // bytes once the RLE1 runs are expanded (bzb_size_kernel)
    uint32_t status, crc, orig_ptr, nblock;
};
struct BzbChain {
    uint64_t cur;                // the bit the chain stopped on
    uint64_t total;              // bytes of text of the chained blocks
    uint32_t n;                  // chained blocks
    uint32_t stop_status;        // why it stopped: BZB_OK (the group's candidates ran out, or none stands at `cur`), BZB_EOS, or the failed block's status
};

// ---- bits, MSB first ---------------------------------------------------------------------------------------------------------------
BZB_HD inline uint64_t bzb_be64(const uint8_t* p) {
    uint64_t x;
    memcpy(&x, p, 8);
    return __builtin_bswap64(x);
}
struct BzbBits {
    const uint8_t* p;
    uint64_t end, pos, w, wbase;
    uint32_t over;               // a read went past `end`: everything read since is zero
};
BZB_HD inline void bzb_bits_init(BzbBits& b, const uint8_t* p, uint64_t end, uint64_t pos) {
    b.p = p; b.end = end; b.pos = pos; b.over = pos > end ? 1u : 0u;
    if (b.over) b.pos = end;
    b.wbase = b.pos & ~7ull;
    b.w = bzb_be64(p + (b.wbase >> 3));
}
// the next n bits (1 <= n <= 32)
BZB_HD inline uint32_t bzb_get(BzbBits& b, uint32_t n) {
    if (b.pos + n > b.end) { b.over = 1u; return 0u; }
    if (b.pos + n > b.wbase + 64u) {
        b.wbase = b.pos & ~7ull;
        b.w = bzb_be64(b.p + (b.wbase >> 3));
    }
    const uint32_t v = (uint32_t)((b.w << (b.pos - b.wbase)) >> (64u - n));
    b.pos += n;
    return v;
}

// ---- block scan: the 64 bit positions that start in the 8 bytes at `byte` -----------------------------------------------------------
// bit s of *blk / *eos: the block / end-of-stream magic stands at bit byte * 8 + s (and fits the window's nbits)
BZB_HD inline void bzb_scan64(const uint8_t* comp, uint64_t nbits, uint64_t byte, uint64_t* blk, uint64_t* eos) {
    const uint64_t hi = bzb_be64(comp + byte), lo = bzb_be64(comp + byte + 8);
    uint64_t mb = 0, me = 0;
    for (uint32_t s = 0; s < 64u; ++s) {
        const uint64_t v = (s ? (hi << s) | (lo >> (64u - s)) : hi) >> 16;
        if (v == BZB_MAGIC_BLOCK) mb |= 1ull << s;
        if (v == BZB_MAGIC_EOS) me |= 1ull << s;
    }
    // (positions whose 48 bits do not fit the window)
    if (mb | me)
        for (uint32_t s = 0; s < 64u; ++s)
            if (byte * 8u + s + 48u > nbits) { mb &= ~(1ull << s); me &= ~(1ull << s); }
    *blk = mb;
    *eos = me;
}

// ---- entropy stage -------------------------------------------------------------------------------------------------------------------
// What a block's decoder keeps at hand (LDS on the device): six tables of <= 258 symbols as limit / base / perm, the MTF list,
// the symbol map and the byte counts.  6,032 bytes (the other kernels keep 1 KB: cf[] / crc_tab[]).
struct BzbTables {
    int32_t limit[6][23];
    int32_t base[6][23];
    uint16_t perm[6][260];
    uint8_t len[260];
    uint8_t min_len[6], max_len[6];
    uint8_t mtf[256];
    uint8_t seq[256];            // symbol index -> byte value
    uint32_t counts[256];
};

// limit / base / perm of table t from T.len[0, alpha)
BZB_HD inline void bzb_make_table(BzbTables& T, uint32_t t, uint32_t alpha) {
    uint32_t mn = 32, mx = 0;
    for (uint32_t i = 0; i < alpha; ++i) { const uint32_t l = T.len[i]; if (l > mx) mx = l; if (l < mn) mn = l; }
    T.min_len[t] = (uint8_t)mn; T.max_len[t] = (uint8_t)mx;
    uint32_t pp = 0;
    for (uint32_t l = mn; l <= mx; ++l)
        for (uint32_t i = 0; i < alpha; ++i) if (T.len[i] == l) T.perm[t][pp++] = (uint16_t)i;
    int32_t* const base = T.base[t];
    int32_t* const limit = T.limit[t];
    for (uint32_t i = 0; i < 23u; ++i) { base[i] = 0; limit[i] = -1; }       // (-1: no code of that length — a longer code than max_len never decodes)
    for (uint32_t i = 0; i < alpha; ++i) base[T.len[i] + 1u]++;
    for (uint32_t i = 1; i < 23u; ++i) base[i] += base[i - 1];
    int32_t vec = 0;
    for (uint32_t l = mn; l <= mx; ++l) {
        vec += base[l + 1] - base[l];
        limit[l] = vec - 1;
        vec <<= 1;
    }
    for (uint32_t l = mn + 1; l <= mx; ++l) base[l] = ((limit[l - 1] + 1) << 1) - base[l];
}

// One block whose 48-bit magic stands at `start`: its BWT bytes into bw[0, nblock), the byte counts into counts[256], the rest
// into *out.  `sel`: BZB_SEL_BYTES of scratch (global memory on the device).  Loops: the header's are bounded by their field
// widths (selectors: nSelectors < 2^15 times <= 6 bits; code lengths: BZB_MAX_DELTAS per symbol), the symbol loop by the
// selectors (<= 18,002 x 50 symbols, a run by 21 of them) and its stores by level x 100,000; a read past the window's end
// returns zero bits, which end every one of them.
BZB_HD inline void bzb_entropy_block(const uint8_t* comp, uint64_t nbits, uint64_t start, uint32_t level, BzbTables& T, uint8_t* sel,
                                     uint8_t* bw, uint32_t* counts, BzbBlock* out) {
    BzbBits br;
    bzb_bits_init(br, comp, nbits, start + 48u);
    out->end_bit = 0; out->out_size = 0; out->nblock = 0; out->orig_ptr = 0;
    out->status = BZB_BAD;
    out->crc = bzb_get(br, 32);
    const uint32_t randomised = bzb_get(br, 1);
    const uint32_t orig = bzb_get(br, 24);
    if (br.over) { out->status = BZB_PAST_END; return; }
    if (randomised) { out->status = BZB_RANDOMISED; return; }
    // symbol map: 16 bits, then 16 for each that is set
    uint32_t n_in_use = 0;
    {
        const uint32_t in16 = bzb_get(br, 16);
        for (uint32_t i = 0; i < 16u; ++i)
            if ((in16 >> (15u - i)) & 1u) {
                const uint32_t m = bzb_get(br, 16);
                for (uint32_t j = 0; j < 16u; ++j)
                    if ((m >> (15u - j)) & 1u) T.seq[n_in_use++] = (uint8_t)(i * 16u + j);
            }
    }
    if (br.over) { out->status = BZB_PAST_END; return; }
    if (n_in_use == 0) return;
    const uint32_t alpha = n_in_use + 2u;
    const uint32_t n_groups = bzb_get(br, 3);
    const uint32_t n_sel = bzb_get(br, 15);
    if (n_groups < 2u || n_groups > 6u || n_sel < 1u) { if (br.over) out->status = BZB_PAST_END; return; }
    // selectors: MTF positions in unary (those beyond 18,002 are read and dropped, as bzip2 1.0.8 does)
    {
        uint8_t pos[6];
        for (uint32_t v = 0; v < n_groups; ++v) pos[v] = (uint8_t)v;
        for (uint32_t i = 0; i < n_sel; ++i) {
            uint32_t j = 0;
            while (bzb_get(br, 1)) { if (++j >= n_groups) return; }
            if (br.over) { out->status = BZB_PAST_END; return; }
            const uint8_t tmp = pos[j];
            for (; j > 0; --j) pos[j] = pos[j - 1];
            pos[0] = tmp;
            if (i < BZB_MAX_SELECTORS) sel[i] = tmp;
        }
    }
    const uint32_t n_sel_used = n_sel < BZB_MAX_SELECTORS ? n_sel : BZB_MAX_SELECTORS;
    // code lengths, delta coded
    for (uint32_t t = 0; t < n_groups; ++t) {
        uint32_t curr = bzb_get(br, 5);
        for (uint32_t i = 0; i < alpha; ++i) {
            // (an encoder steps straight from one length to the next: <= 19 deltas.  A symbol with more than BZB_MAX_DELTAS is
            //  refused — the host's libbz2 judges it — so the header's loops are bounded by the block, 6 x 258 x 64 steps,
            //  not by the window)
            for (uint32_t steps = 0;; ++steps) {
                if (curr < 1u || curr > BZB_MAX_LEN || steps > BZB_MAX_DELTAS) { if (br.over) out->status = BZB_PAST_END; return; }
                if (!bzb_get(br, 1)) break;
                curr += bzb_get(br, 1) ? 0xffffffffu : 1u;
            }
            T.len[i] = (uint8_t)curr;
        }
        if (br.over) { out->status = BZB_PAST_END; return; }
        bzb_make_table(T, t, alpha);
    }
    for (uint32_t i = 0; i < 256u; ++i) { T.mtf[i] = (uint8_t)i; T.counts[i] = 0; }
    const uint32_t eob = n_in_use + 1u, nblock_max = level * 100000u;
    uint32_t nblock = 0, group_no = 0, group_left = 0, g = 0;
    // the next symbol: BZB_MAX_ALPHA = failed (st set)
    uint32_t st = BZB_OK;
    auto next_sym = [&]() -> uint32_t {
        if (group_left == 0) {
            if (group_no >= n_sel_used) { st = BZB_BAD; return BZB_MAX_ALPHA; }
            g = sel[group_no++];
            group_left = BZB_G_SIZE;
        }
        --group_left;
        uint32_t zn = T.min_len[g];
        int32_t zvec = (int32_t)bzb_get(br, zn);
        while (zvec > T.limit[g][zn]) {
            if (++zn > BZB_MAX_LEN) { st = br.over ? BZB_PAST_END : BZB_BAD; return BZB_MAX_ALPHA; }
            zvec = (zvec << 1) | (int32_t)bzb_get(br, 1);
        }
        if (br.over) { st = BZB_PAST_END; return BZB_MAX_ALPHA; }
        const int32_t idx = zvec - T.base[g][zn];
        if (idx < 0 || idx >= (int32_t)alpha) { st = BZB_BAD; return BZB_MAX_ALPHA; }
        return T.perm[g][idx];
    };
    uint32_t sym = next_sym();
    for (;;) {
        if (sym == BZB_MAX_ALPHA) { out->status = st; return; }
        if (sym == eob) break;
        if (sym < 2u) {
            // RUNA / RUNB: a run length in bijective base 2
            uint32_t es = 0, n = 1;
            do {
                if (n >= (2u << 20)) return;
                es += n << sym;
                n <<= 1;
                sym = next_sym();
            } while (sym < 2u);
            const uint8_t uc = T.seq[T.mtf[0]];
            if (es > nblock_max - nblock) return;
            T.counts[uc] += es;
            for (uint32_t k = 0; k < es; ++k) bw[nblock + k] = uc;
            nblock += es;
            continue;
        }
        if (nblock >= nblock_max) return;
        const uint32_t nn = sym - 1u;
        const uint8_t m = T.mtf[nn];
        for (uint32_t k = nn; k > 0; --k) T.mtf[k] = T.mtf[k - 1];
        T.mtf[0] = m;
        const uint8_t uc = T.seq[m];
        T.counts[uc]++;
        bw[nblock++] = uc;
        sym = next_sym();
    }
    if (orig >= nblock) return;
    for (uint32_t i = 0; i < 256u; ++i) counts[i] = T.counts[i];
    out->end_bit = br.pos; out->nblock = nblock; out->orig_ptr = orig;
    out->status = BZB_OK;
}

// ---- inverse BWT ---------------------------------------------------------------------------------------------------------------------
// tt[j] = i << 8 | byte: row j of the sorted matrix is followed by row i, and starts with `byte` (a stable counting sort of
// bw[0, nblock) by the counts).  cf: 256 words of scratch.  false: the counts do not add up (cannot happen after bzb_entropy_block).
BZB_HD inline bool bzb_bwt_scatter(const uint8_t* bw, uint32_t* tt, uint32_t nblock, uint32_t orig, const uint32_t* counts, uint32_t* cf) {
    uint32_t sum = 0;
    for (uint32_t c = 0; c < 256u; ++c) { cf[c] = sum; sum += counts[c]; }
    if (sum != nblock || orig >= nblock) return false;
    for (uint32_t i = 0; i < nblock; ++i) {
        const uint32_t uc = bw[i];
        const uint32_t j = cf[uc]++;
        if (j >= nblock) return false;
        tt[j] = (i << 8) | uc;
    }
    return true;
}
// the chase from orig for nblock steps writes the block's bytes (still RLE1-coded) over bw
BZB_HD inline bool bzb_bwt_chase(uint8_t* bw, const uint32_t* tt, uint32_t nblock, uint32_t orig) {
    uint32_t t = orig;
    for (uint32_t i = 0; i < nblock; ++i) {
        if (t >= nblock) return false;
        const uint32_t x = tt[t];
        bw[i] = (uint8_t)x;
        t = x >> 8;
    }
    return true;
}

// ---- RLE1 and CRC --------------------------------------------------------------------------------------------------------------------
// four equal bytes MUST be followed, inside the same block, by a count byte 0..255 of further repeats; behind the count byte the
// run state starts afresh, and it never crosses a block boundary.  A block whose last four bytes are a run still waiting for
// its count byte is damaged (libbz2 reads the count byte before it looks for the block's end and rejects the stream).
// The size of pre[0, n) with its runs expanded, or BZB_NO_SIZE: the block ends on four equal bytes without a count byte.
constexpr uint64_t BZB_NO_SIZE = ~0ull;
BZB_HD inline uint64_t bzb_rle1_size(const uint8_t* pre, uint32_t n) {
    uint64_t size = 0;
    uint32_t run = 0, last = 256u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = pre[i];
        if (run == 4u) { size += c; run = 0; last = 256u; continue; }
        run = c == last ? run + 1u : 1u;
        last = c;
        ++size;
    }
    return run == 4u ? BZB_NO_SIZE : size;
}
BZB_HD inline uint32_t bzb_crc_entry(uint32_t i) {
    uint32_t c = i << 24;
    for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04c11db7u : c << 1;
    return c;
}
// the runs expanded into out[0, cap); returns the block's CRC (bzip2's: 0x04c11db7, MSB first); *written = bytes written.
// (Only blocks that chained come here, and a block that ends on a run without its count byte never chains — it has no size,
//  bzb_size_kernel makes it BZB_BAD — so the rule is not stated a second time.)
BZB_HD inline uint32_t bzb_rle1_write(const uint8_t* pre, uint32_t n, uint8_t* out, uint64_t cap, const uint32_t* crc_tab, uint64_t* written) {
    uint32_t crc = 0xffffffffu, run = 0, last = 256u;
    uint64_t o = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = pre[i];
        if (run == 4u) {
            uint32_t k = c;
            if (k > cap - o) k = (uint32_t)(cap - o);
            for (uint32_t r = 0; r < k; ++r) { out[o + r] = (uint8_t)last; crc = (crc << 8) ^ crc_tab[(crc >> 24) ^ last]; }
            o += k;
            run = 0; last = 256u;
            continue;
        }
        run = c == last ? run + 1u : 1u;
        last = c;
        if (o < cap) { out[o++] = (uint8_t)c; crc = (crc << 8) ^ crc_tab[(crc >> 24) ^ c]; }
    }
    *written = o;
    return ~crc;
}

// ---- chain ---------------------------------------------------------------------------------------------------------------------------
// cand[0, g): the group's candidates (sorted, position << 1 | end-of-stream), blk[0, g) what they decoded to.  From bit `cur`:
// a candidate before it is skipped (a chance hit inside a block), the one AT it must have decoded; idx[k] / off[k] are the k-th
// chained block's candidate and its place in the group's text (off[n] = total).  The chain stops in front of a block that does
// not fit out_cap any more — unless it is the first.
BZB_HD inline void bzb_chain(const uint64_t* cand, uint32_t g, const BzbBlock* blk, uint64_t cur, uint64_t out_cap, BzbChain* ch, uint32_t* idx, uint64_t* off) {
    uint32_t n = 0, stop = BZB_OK;
    uint64_t total = 0;
    for (uint32_t j = 0; j < g; ++j) {
        const uint64_t pos = cand[j] >> 1;
        if (pos < cur) continue;
        if (pos > cur) break;
        if (cand[j] & 1ull) { stop = BZB_EOS; break; }
        if (blk[j].status != BZB_OK) { stop = blk[j].status; break; }
        if (n && total + blk[j].out_size > out_cap) break;
        idx[n] = j; off[n] = total;
        total += blk[j].out_size;
        cur = blk[j].end_bit;
        ++n;
    }
    off[n] = total;
    ch->cur = cur; ch->total = total; ch->n = n; ch->stop_status = stop;
}

#if defined(__HIPCC__)
// ---- the kernels: they only deal the work out -------------------------------------------------------------------------------------------
struct BzbJob {
    const uint8_t* comp;         // the window, BZB_PAD zero bytes behind it
    uint64_t nbits;
    // scan
    uint64_t* cand_raw;          // [cand_cap] hits in the order they were found
    uint64_t* cand;              // [cand_cap] sorted
    uint32_t* n_cand;            // hits (may exceed cand_cap: the list is then incomplete and not used)
    uint32_t cand_cap;
    // a group: candidates [first, first + g)
    uint32_t first, g, level;
    uint32_t slot;               // bytes of a candidate's place in bw (>= level x 100,000, a multiple of 16); tt has as many words
    uint8_t* sel;                // [g][BZB_SEL_BYTES]
    uint8_t* bw;                 // [g][slot]
    uint32_t* tt;                // [g][slot]
    uint32_t* counts;            // [g][256]
    BzbBlock* blk;               // [g]
    uint64_t cur, out_cap;
    BzbChain* chain;
    uint32_t* chain_idx;         // [g]
    uint64_t* chain_off;         // [g + 1]
    uint32_t* crc_out;           // [g] CRC of the k-th chained block's text
    uint8_t* out;                // the group's text
};

__global__ __launch_bounds__(BZB_SCAN_THREADS) void bzb_scan_kernel(BzbJob J) {
    const uint64_t word = (uint64_t)blockIdx.x * BZB_SCAN_THREADS + threadIdx.x;
    if (word * 64u >= J.nbits) return;
    uint64_t mb, me;
    bzb_scan64(J.comp, J.nbits, word * 8u, &mb, &me);
    for (uint64_t m = mb | me; m; m &= m - 1) {
        const uint32_t s = (uint32_t)__builtin_ctzll(m);
        const uint32_t k = atomicAdd(J.n_cand, 1u);
        if (k < J.cand_cap) J.cand_raw[k] = ((word * 64u + s) << 1) | ((me >> s) & 1ull);
    }
}

// positions are distinct: an entry's rank is the number of smaller ones (n <= cand_cap <= 65,536)
__global__ __launch_bounds__(256) void bzb_sort_kernel(BzbJob J) {
    const uint32_t n = min(J.n_cand[0], J.cand_cap);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = J.cand_raw[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) rank += J.cand_raw[j] < v ? 1u : 0u;
    J.cand[rank] = v;
}

__global__ __launch_bounds__(64) void bzb_entropy_kernel(BzbJob J) {
    __shared__ BzbTables T;
    const uint32_t c = blockIdx.x;
    if (threadIdx.x != 0 || c >= J.g) return;
    const uint64_t cd = J.cand[J.first + c];
    BzbBlock* const b = J.blk + c;
    if (cd & 1ull) { b->end_bit = 0; b->out_size = 0; b->status = BZB_EOS; b->crc = 0; b->orig_ptr = 0; b->nblock = 0; return; }
    bzb_entropy_block(J.comp, J.nbits, cd >> 1, J.level, T, J.sel + (size_t)c * BZB_SEL_BYTES, J.bw + (size_t)c * J.slot, J.counts + (size_t)c * 256u, b);
}

__global__ __launch_bounds__(64) void bzb_scatter_kernel(BzbJob J) {
    __shared__ uint32_t cf[256];
    const uint32_t c = blockIdx.x;
    if (threadIdx.x != 0 || c >= J.g) return;
    BzbBlock* const b = J.blk + c;
    if (b->status != BZB_OK) return;
    if (b->nblock > J.slot || !bzb_bwt_scatter(J.bw + (size_t)c * J.slot, J.tt + (size_t)c * J.slot, b->nblock, b->orig_ptr, J.counts + (size_t)c * 256u, cf)) b->status = BZB_BAD;
}

__global__ __launch_bounds__(64) void bzb_chase_kernel(BzbJob J) {
    const uint32_t c = blockIdx.x;
    if (threadIdx.x != 0 || c >= J.g) return;
    BzbBlock* const b = J.blk + c;
    if (b->status != BZB_OK) return;
    if (!bzb_bwt_chase(J.bw + (size_t)c * J.slot, J.tt + (size_t)c * J.slot, b->nblock, b->orig_ptr)) b->status = BZB_BAD;
}

__global__ __launch_bounds__(64) void bzb_size_kernel(BzbJob J) {
    const uint32_t c = blockIdx.x;
    if (threadIdx.x != 0 || c >= J.g) return;
    BzbBlock* const b = J.blk + c;
    if (b->status != BZB_OK) return;
    b->out_size = bzb_rle1_size(J.bw + (size_t)c * J.slot, b->nblock);
    if (b->out_size == BZB_NO_SIZE) { b->out_size = 0; b->status = BZB_BAD; }
}

__global__ void bzb_chain_kernel(BzbJob J) {
    if (blockIdx.x == 0 && threadIdx.x == 0) bzb_chain(J.cand + J.first, J.g, J.blk, J.cur, J.out_cap, J.chain, J.chain_idx, J.chain_off);
}

__global__ __launch_bounds__(64) void bzb_expand_kernel(BzbJob J) {
    __shared__ uint32_t crc_tab[256];
    const uint32_t k = blockIdx.x;
    if (k >= J.chain->n) return;
    for (uint32_t i = threadIdx.x; i < 256u; i += 64u) crc_tab[i] = bzb_crc_entry(i);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t c = J.chain_idx[k];
    const uint64_t o = J.chain_off[k], size = J.chain_off[k + 1] - o;
    uint64_t written = 0;
    const uint32_t crc = bzb_rle1_write(J.bw + (size_t)c * J.slot, J.blk[c].nblock, J.out + o, size, crc_tab, &written);
    J.crc_out[k] = written == size ? crc : ~J.blk[c].crc;        // (a size that does not come out again never passes for a match)
}
#endif  // __HIPCC__

}  // namespace aqc
