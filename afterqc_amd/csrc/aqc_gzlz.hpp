// aqc_gzlz.hpp — the device gzip encoder of `--compression 6 .. 9`: a hash-chain match search in front of the format, the code
// and the bit writer of aqc_gzdev.hpp.  The two encoders there only see a run of the byte before and the same column four lines
// up; this one sees a repeated read, an adapter, a primer, a quality string from 30 records back — whatever lies in the 32 KiB
// before a position and is reachable over `depth(level)` links of its hash chain.
//
//   member   GZ_TEXT = 0xff00 bytes of text in a GZ_SLOT staging slot, as gz_encode_kernel's: BGZF extra field, ONE final dynamic
//            block with the stream's shared code, stored when that is smaller.  One WAVE per member (a workgroup of 64): the text
//            (64 KB), the head table (2^13 x u16 = 16 KB) and the previous-position table ([pos & 0x7fff] x u16 = 64 KB) are in
//            LDS, 147 KB with the codes and the staging ring — one wave per CU.  The comparisons of the search are byte loads
//            at data-dependent addresses, thousands per window: from LDS they cost a few cycles each, from L2 hundreds.
//   THE RULE (what a position may link to; nothing in it depends on lane timing):
//            the member is walked in windows of 64 consecutive bytes, a lane per position.  Window w is INSERTED whole — in
//            position order: previous[p] = head[hash(p)], head[hash(p)] = p, for every p of the window with p + 2 < n — and
//            only then SEARCHED.  So the tables a position p of window w sees hold exactly the positions 0 .. 64 w + 63 of this
//            member, and the chain p walks is previous[p], previous[previous[p]], ...: the positions before p with p's hash
//            (or a colliding one), nearest first.  The wave builds the window's links with one ballot per distinct hash
//            (gzlz_insert_window) and gets the tables the sequential loop gets (gzlz_link, which the CPU program runs).
//   bounds   head and previous are filled with GZLZ_NIL for every member.  A walk ends after `depth` candidates, at GZLZ_NIL, at a
//            candidate that is not strictly smaller than the one before (previous[] is indexed modulo 32 KiB: an entry may have
//            been taken over by the position 32 KiB later — the chain then leads somewhere else or up, never round), at a
//            candidate >= the position, or at a distance > 32768.  The hash is taken only where p + 2 < n, a comparison never
//            goes past min(258, n - p) bytes, no position before the member's first byte exists in the tables.
//   tokens   per position the longest match (the nearest of equals; distance 1 is tried first, it has the cheapest code), taken
//            when its code is shorter than the literals' it replaces by the actual code lengths (gzlz_take).  No lazy step.
//   calls    from aqc_gzdev.hpp, shared with gz_encode_wave_kernel: gz_member_of / gz_sample_of, gz_load_code, gzw_open_block,
//            gzw_parse (the greedy parse over a window's token starts), gzw_token_bits (a token's bits and the lane scan of their
//            lengths), gzw_ring_put (the LDS ring and the coalesced word stores), gzw_close_block (end of block or stored),
//            gzw_crc<2>, gz_crc_short, gz_frame_member.  Its own: the tables, the search, and the stored test BEFORE a window is
//            written.  The length / distance symbols: aqc_deflate_sym.hpp.
//   sample   gz_hist_lz_kernel tokenises the same 16 pieces per stream as gz_hist_kernel, with this search and fixed thresholds
//            (no code exists yet), into the same hist layout.
//
// gzlz_hash / gzlz_link / gzlz_search / gzlz_take are __host__ __device__: tests/native/gzlz_selftest.cpp includes this header
// without HIP and deals them out by plain loops in the kernel's window order.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GZLZ_HD __host__ __device__ __forceinline__
#else
#define GZLZ_HD inline
#endif
#include "aqc_deflate_sym.hpp"

namespace aqc {

constexpr int GZLZ_HASH_BITS = 13;
constexpr int GZLZ_PREV = 32768;                 // entries of the previous-position table, indexed by position & (GZLZ_PREV - 1)
constexpr int GZLZ_NIL = 0xffff;                 // "no position" (a member has at most 0xff00 of them)
constexpr int GZLZ_MIN = 3, GZLZ_MAX = 258, GZLZ_FAR = 32768;
constexpr int GZLZ_WINDOW = 64;                  // positions inserted, then searched, together

// candidates a position tries on its chain
GZLZ_HD int gzlz_depth(int level) { return level <= 6 ? 8 : level == 7 ? 16 : level == 8 ? 32 : 64; }

// hash of the three bytes at p; the caller guarantees p + 2 < n
GZLZ_HD uint32_t gzlz_hash(const uint8_t* s, int p) {
    const uint32_t v = (uint32_t)s[p] | ((uint32_t)s[p + 1] << 8) | ((uint32_t)s[p + 2] << 16);
    return (v * 0x9E3779B1u) >> (32 - GZLZ_HASH_BITS);
}

// position p (hash h) enters the tables; positions enter in ascending order
GZLZ_HD void gzlz_link(uint16_t* head, uint16_t* prev, int p, uint32_t h) {
    prev[p & (GZLZ_PREV - 1)] = head[h];
    head[h] = (uint16_t)p;
}

// bytes that s[q ..] and s[p ..] share, at most lim (q < p, p + lim <= n)
GZLZ_HD int gzlz_extend(const uint8_t* s, int p, int q, int lim) {
    int m = 0;
    while (m < lim && s[q + m] == s[p + m]) ++m;
    return m;
}

struct GzlzMatch {
    int len, dist;       // len 0: none
};

// the longest match at position p of the member s[0, n), p already inserted: distance 1, then at most `depth` candidates of p's chain
GZLZ_HD GzlzMatch gzlz_search(const uint8_t* s, int n, int p, const uint16_t* prev, int depth) {
    GzlzMatch best{0, 0};
    const int lim = n - p < GZLZ_MAX ? n - p : GZLZ_MAX;
    if (lim < GZLZ_MIN) return best;
    if (p > 0 && s[p - 1] == s[p]) {
        const int m = gzlz_extend(s, p, p - 1, lim);
        if (m >= GZLZ_MIN) { best.len = m; best.dist = 1; }
    }
    int last = p, q = prev[p & (GZLZ_PREV - 1)];
    for (int step = 0; step < depth && best.len < lim; ++step) {
        if (q == GZLZ_NIL || q >= last || p - q > GZLZ_FAR) break;
        // (a longer match has to agree at the byte the best one ended on: most candidates fail here)
        if (s[q + best.len] == s[p + best.len]) {
            const int m = gzlz_extend(s, p, q, lim);
            if (m > best.len && m >= GZLZ_MIN) { best.len = m; best.dist = p - q; }
        }
        last = q;
        q = prev[q & (GZLZ_PREV - 1)];
    }
    return best;
}

// is the match worth a token?  EXACT: its code is shorter than the literals' it replaces, by the code lengths (lc / dc: bit-reversed
// code | length << 16); otherwise — the sampling pass, before a code exists — zlib's rule of thumb: not a length of 3 from far away
template <bool EXACT>
GZLZ_HD bool gzlz_take(const uint8_t* s, int p, GzlzMatch m, const uint32_t* lc, const uint32_t* dc) {
    if (m.len < GZLZ_MIN) return false;
    if (!EXACT) return m.len > GZLZ_MIN || m.dist <= 4096;
    const int ls = len_sym(m.len), ds = dist_sym(m.dist);
    const int cost = (int)(lc[257 + ls] >> 16) + len_extra(ls) + (int)(dc[ds] >> 16) + dist_extra(ds);
    int lit = 0;
    for (int i = 0; i < m.len && lit <= cost; ++i) lit += (int)(lc[s[p + i]] >> 16);
    return lit > cost;
}

}  // namespace aqc

#if defined(__HIPCC__)
#include "aqc_gzdev.hpp"

namespace aqc {

struct alignas(16) GzlzStage {
    uint8_t text[GZ_TEXT + 16];
    uint16_t head[1 << GZLZ_HASH_BITS];
    uint16_t prev[GZLZ_PREV];
    uint32_t lc[286], dc[30];
    uint32_t crc_tab[256];
    uint32_t ring[GZW_RING];
    uint32_t hist[320];
};
static_assert(sizeof(GzlzStage) <= 160 * 1024, "one member's state must fit a CU's LDS");

// the member's text into LDS, the tables emptied
__device__ __forceinline__ void gzlz_stage_member(GzlzStage& S, const uint8_t* src, int n, int lane) {
    for (int i = lane * 16; i < n; i += WAVE * 16) *reinterpret_cast<uint4*>(S.text + i) = load16u(src + i);      // (64 readable bytes follow a stream)
    uint32_t* const hw = reinterpret_cast<uint32_t*>(S.head);
    for (int i = lane; i < (1 << GZLZ_HASH_BITS) / 2; i += WAVE) hw[i] = 0xffffffffu;
    uint32_t* const pw = reinterpret_cast<uint32_t*>(S.prev);
    for (int i = lane; i < GZLZ_PREV / 2; i += WAVE) pw[i] = 0xffffffffu;
}

// window w enters the tables: what gzlz_link does position by position, a ballot per distinct hash.  A lane's predecessor is the
// nearest lane below it with its hash, else the head from before the window; the last lane of a hash becomes the head.
__device__ __forceinline__ void gzlz_insert_window(GzlzStage& S, int n, int w, int lane, unsigned long long lt) {
    const int p = GZLZ_WINDOW * w + lane;
    const bool valid = p + 2 < n;
    const uint32_t h = valid ? gzlz_hash(S.text, p) : 0u;
    const uint32_t old = valid ? S.head[h] : 0u;
    int pred = -1;
    bool last = false;
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int l = (int)__builtin_ctzll(todo);
        const uint32_t hl = (uint32_t)__builtin_amdgcn_readlane((int)h, l);
        const bool mine = valid && h == hl;
        const unsigned long long m = __ballot(mine);
        if (mine) {
            const unsigned long long below = m & lt;
            pred = below ? 63 - (int)__builtin_clzll(below) : -1;
            last = ((m >> lane) >> 1) == 0ull;
        }
        todo &= ~m;
    }
    if (valid) {
        S.prev[p & (GZLZ_PREV - 1)] = (uint16_t)(pred >= 0 ? (uint32_t)(GZLZ_WINDOW * w + pred) : old);
        if (last) S.head[h] = (uint16_t)p;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);              // lgkmcnt(0): the links are in LDS before the search reads them
}

// window w of the member: inserted, searched, parsed.  -> this lane's token (blen 1: a literal) and the mask of the lanes a token
// starts at; `skip` = bytes at the window's front that an earlier token covers, carried to the next call
template <bool EXACT>
__device__ __forceinline__ unsigned long long gzlz_window(GzlzStage& S, int n, int w, int lane, unsigned long long lt, int depth, int& skip, int& blen, int& dist) {
    gzlz_insert_window(S, n, w, lane, lt);
    blen = 1; dist = 0;
    if (skip >= GZLZ_WINDOW) { skip -= GZLZ_WINDOW; return 0ull; }
    const int p = GZLZ_WINDOW * w + lane;
    const bool valid = p < n;
    if (valid && lane >= skip) {
        const GzlzMatch m = gzlz_search(S.text, n, p, S.prev, depth);
        if (gzlz_take<EXACT>(S.text, p, m, S.lc, S.dc)) { blen = m.len; dist = m.dist; }
    }
    // (every lane takes part in the ballot: one behind the member's end keeps blen 1)
    return gzw_parse(__ballot(valid), __ballot(blen > 1) != 0ull, blen, skip);
}

// ---- sampling pass: symbol counts of some members of every stream, tokenised by the search ---------------------------------------
__global__ __launch_bounds__(WAVE) void gz_hist_lz_kernel(GzJob J, int depth) {
    __shared__ GzlzStage S;
    const int lane = (int)threadIdx.x;
    int q, n; uint64_t off;
    if (!gz_sample_of(J, q, off, n)) return;
    for (int i = lane; i < 320; i += WAVE) S.hist[i] = 0;
    gzlz_stage_member(S, J.text[q] + off, n, lane);
    __syncthreads();
    const unsigned long long lt = gzw_lanes_below(lane);
    const int n_win = (n + GZLZ_WINDOW - 1) / GZLZ_WINDOW;
    int skip = 0;
    for (int w = 0; w < n_win; ++w) {
        int blen, dist;
        const unsigned long long marks = gzlz_window<false>(S, n, w, lane, lt, depth, skip, blen, dist);
        if ((marks >> lane) & 1ull) {
            if (blen == 1) atomicAdd(&S.hist[S.text[GZLZ_WINDOW * w + lane]], 1u);
            else { atomicAdd(&S.hist[257 + len_sym(blen)], 1u); atomicAdd(&S.hist[286 + dist_sym(dist)], 1u); }
        }
    }
    __syncthreads();
    for (int i = lane; i < 320; i += WAVE)
        if (S.hist[i]) atomicAdd(&J.hist[q * 320 + i], S.hist[i]);
}

// ---- one gzip member per wave --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void gz_encode_lz_kernel(GzJob J, int depth) {
    __shared__ GzlzStage S;
    const int lane = (int)threadIdx.x;
    const uint32_t member = blockIdx.x;
    int q, n; uint64_t off;
    gz_member_of(J, member, GZ_TEXT, q, off, n);
    const GzCodebookDev& cb = J.code[q];
    gz_load_code<WAVE>(cb, J.crc->byte_table, S.lc, S.dc, S.crc_tab);
    gzlz_stage_member(S, J.text[q] + off, n, lane);
    __syncthreads();
    uint8_t* const mem = gz_member_slot(J, member, GZ_SLOT);
    uint32_t* const dwords = gz_member_data(mem);
    const unsigned long long lt = gzw_lanes_below(lane);
    uint32_t bitpos = gzw_open_block(cb, dwords, S.ring, lane);
    __syncthreads();
    // beyond this a stored block is smaller; tested BEFORE a window is written: the window that would cross the limit is not, so the
    // deflate data never passes n + 5 bytes (+ the end-of-block word) of the GZ_SLOT - 20 the slot has for data and trailer
    const uint32_t limit_bits = ((uint32_t)n + 5u) * 8u;
    bool stored = false;
    const int n_win = (n + GZLZ_WINDOW - 1) / GZLZ_WINDOW;
    int skip = 0;
    for (int w = 0; w < n_win && !stored; ++w) {
        int blen, dist;
        const unsigned long long marks = gzlz_window<true>(S, n, w, lane, lt, depth, skip, blen, dist);
        if (marks == 0ull) continue;
        const bool tok = (marks >> lane) & 1ull;
        const GzwBits t = gzw_token_bits(S.lc, S.dc, tok, S.text[GZLZ_WINDOW * w + lane], blen, dist, lane);
        if (bitpos + t.total > limit_bits) { stored = true; break; }
        gzw_ring_put(S.ring, dwords, bitpos, tok, t, lane);
    }
    const uint32_t dbytes = gzw_close_block(S.ring, S.lc, mem, S.text, bitpos, n, lane, stored);
    static_assert(GZ_TEXT == WAVE * 4 * GZ_SEG, "four segments of the CRC grid per lane");
    uint32_t c = gzw_crc<2>(S.text, n, S.crc_tab, *J.crc, lane);
    if (lane == 0) {
        if (n < 4) c = gz_crc_short(S.crc_tab, S.text, n);
        J.sizes[member] = gz_frame_member(mem, dbytes, ~c, n);
    }
}

}  // namespace aqc
#endif  // __HIPCC__
