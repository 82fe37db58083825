// aqc_adapter.hpp — trimming a given adapter from each read (--adapter_sequence / --adapter_sequence_r2): the pass that looks, for
// every mate of a batch, for the first place p of its trimmed and quality-cut SEQUENCE line at which the mate's adapter lies, and
// ends the mate's view there.  The rule is tests/adapter_rule.py (adapter_find): at p the k = min(m, n - p) bases the read still
// has are compared with the adapter's first k, p matches when at most k >> 3 of them differ, the smallest p wins; a match at the
// read's tail needs at least K bases of the adapter on the read (p <= n - K).
//
// The frame — lanes per read, the 16-byte load, the view word, the counts — is that of every view pass: aqc_viewpass.hpp.  Here:
//
//   line     the sequence line, its 16 bytes per lane stored into the LDS row of the group; the bytes behind the line, and the 80
//            bytes behind the row that a comparison at the tail reaches, are 0 — no base.  Where the line lies and how long it is
//            behind trim() and the view that comes in — the quality cut's when a cut is on, else VIEW_ALL — vp_line says.
//   adapter  both adapters travel in the kernel's by-value arguments, 16 dwords each.  The mate in turn has its 16 dwords in scalar
//            registers, fetched from the argument segment by one s_load_dwordx16 per mate and round: with both mates' 32 dwords
//            live at once the kernel spills 56 scalar registers.  There is no table in device memory.
//   search   pass j lets a lane test p = j * G + lane.  The lane walks the adapter a dword at a time: one aligned LDS read per
//            dword (the previous read's word is the low half), a byte-align, an XOR, a nonzero-byte mask, a popcount; the bytes
//            past k are masked out.  The walk ends for the whole wave once every lane's count is above its allowance, the passes
//            end once every group of the wave has its match or has run out of places.
//   out      the group's first lane composes the view (c0, c0 + p) — or leaves the one that came in — and counts.
//
// The per-read functions are __host__ __device__: tests/native/adapter_selftest.cpp includes this header without HIP, deals the
// lanes of a group out by plain loops and compares with vectors the model wrote.
#pragma once
#include <stdint.h>

#include "aqc_viewpass.hpp"

namespace aqc {

constexpr int ADP_NONE = 0x7fffffff;
constexpr int ADP_MIN_LEN = 4, ADP_MAX_LEN = 64, ADP_WORDS = ADP_MAX_LEN / 4;
// words behind the 16 * G bytes of a group's row: a lane at the row's last byte reads ADP_WORDS + 1 words from its word on
// (the row stays a multiple of 16 bytes, and neighbouring rows start 20 banks apart)
constexpr int ADP_ROW_TAIL = 20;

// the adapters as the kernel takes them: len 0 = that mate is not searched; the bytes little-endian in the dwords, zero behind them
struct AdapterOpts {
    int32_t len[2];
    int32_t min_overlap;
    uint32_t w[2][ADP_WORDS];
};

VP_HD bool adp_on(const AdapterOpts& a) { return a.len[0] > 0 || a.len[1] > 0; }
VP_HD bool adp_opts_ok(const AdapterOpts& a) {
    int shortest = ADP_MAX_LEN;
    for (int k = 0; k < 2; ++k) {
        if (a.len[k] == 0) continue;
        if (a.len[k] < ADP_MIN_LEN || a.len[k] > ADP_MAX_LEN) return false;
        shortest = vp_min(shortest, a.len[k]);
    }
    return !adp_on(a) || (a.min_overlap >= 1 && a.min_overlap <= shortest);
}

// how many of the four bytes of x are not zero
VP_HD int adp_mismatch4(uint32_t x) {
    const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(nz);
#else
    return __builtin_popcount(nz);
#endif
}

// the bytes of a dword that are still compared when `left` bytes of the comparison remain at its first byte
VP_HD uint32_t adp_tail_mask(int left) { return left >= 4 ? 0xffffffffu : left <= 0 ? 0u : (1u << (8 * left)) - 1u; }

// the four bytes that start `sh` (0 .. 3) bytes into the little-endian word pair lo, hi
VP_HD uint32_t adp_bytes_at(uint32_t lo, uint32_t hi, int sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | (uint64_t)lo) >> (8 * sh));
#endif
}

// a lane's 16 loaded bytes as they go into the row: the bytes from `nvalid` on are 0
VP_HD void adp_keep16(uint32_t d[4], int nvalid) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 4; ++j) d[j] &= adp_tail_mask(nvalid - 4 * j);
}

// the mismatches of the adapter's dword I against the read's four bytes at the comparison's byte 4 * I, of which k are compared in all
VP_HD int adp_dword(uint32_t lo, uint32_t hi, int sh, uint32_t a, int k, int I) {
    return adp_mismatch4((adp_bytes_at(lo, hi, sh) ^ a) & adp_tail_mask(k - 4 * I));
}

// A lane's walk along the adapter from dword I on, two dwords a step: `lo` is the row's word under the comparison's byte 4 * I, mm
// the mismatches so far.  It ends for the whole wave once no lane can still match.  A step's second dword may lie behind the adapter:
// its bytes are past k and masked out, and the row has the words.  (Written out step by step — a recursion the compiler flattens —
// so that A[I] names one scalar register: a loop that leaves on a wave-wide test is not unrolled, and would fetch A[i] from memory.)
template <int I>
VP_HD void adp_walk(const uint32_t* wp, uint32_t lo, int sh, const uint32_t (&A)[ADP_WORDS], int nd, int k, int allow, int& mm) {
    if constexpr (I < ADP_WORDS) {
        if (I >= nd || !vp_wave_any(mm <= allow)) return;
        const uint32_t mid = wp[I + 1], hi = wp[I + 2];
        mm += adp_dword(lo, mid, sh, A[I], k, I) + adp_dword(mid, hi, sh, A[I + 1], k, I + 1);
        adp_walk<I + 2>(wp, hi, sh, A, nd, k, allow, mm);
    }
}

// Lane g of a group of G lanes: the first p = j * G + g at which the adapter A (m bytes) matches the read of n bytes that stands
// in `row` (zero bytes behind it, ADP_ROW_TAIL words behind 16 * G bytes); ADP_NONE: nowhere.  Every lane of the wave runs it.
template <int G>
VP_HD int adp_lane_first(const uint32_t* row, int n, const uint32_t (&A)[ADP_WORDS], int m, int K, int g) {
    const int last = n - K;                          // the last place a match may start
    const int nd = (m + 3) >> 2;
    int best = ADP_NONE;
    bool open = true;                                // the lane's group has no match yet
    for (int p0 = 0; vp_wave_any(open && p0 <= last); p0 += G) {
        const int p = p0 + g;
        const bool active = open && p <= last;
        const int pp = active ? p : 0;               // (a lane with nothing to test reads the row's start)
        const int k = vp_min(m, n - pp), allow = k >> 3, sh = pp & 3;
        const uint32_t* const wp = row + (pp >> 2);
        int mm = active ? 0 : (1 << 20);
        adp_walk<0>(wp, wp[0], sh, A, nd, k, allow, mm);
        const bool hit = active && mm <= allow;
        if (hit) best = p;
        open = open && !vp_group_any<G>(hit, g);
    }
    return best;
}

}  // namespace aqc

#if defined(__HIPCC__)
#include "aqc_batch.hpp"

namespace aqc {

// what the pass takes of one mate: its line (ViewMate) and its adapter, side by side so that the mate in turn is one scalar base
struct AdapterMate {
    ViewMate v;
    int32_t alen, pad_;                        // adapter length, 0: the mate is not searched
    uint32_t w[ADP_WORDS];                     // AdapterOpts::w of the mate
};

struct AdapterArgs {
    AdapterMate m[2];
    uint64_t n;                                // records
    int32_t min_overlap;
    int32_t n_mates;                           // 1: read 1 only (single-end input, the function seam)
    const uint32_t* view_in;                   // the quality cut's views, laid out like `view` (may be `view` itself); NULL: no cut, (0, 0xffff)
    uint32_t* view;                            // c0 | c1 << 16 of mate k of record r at [r * n_mates + k]
    unsigned long long* stats;                 // [4] reads of R1 made shorter, bases removed from them, the same for R2; NULL: not counted
    uint64_t accum_limit;
    int* status;
};

static_assert(sizeof(((aqc_adapter_config*)nullptr)->seq1) == ADP_MAX_LEN, "an adapter of the C API fills the kernel's 16 dwords");

// the C API's adapters as the kernel takes them (NULL: off); false: a bad length, a letter that is no base, a bad min_overlap
inline bool adp_from_config(const aqc_adapter_config* cfg, AdapterOpts& a) {
    a = AdapterOpts{};
    if (!cfg) return true;
    a.len[0] = cfg->len1; a.len[1] = cfg->len2; a.min_overlap = cfg->min_overlap;
    if (!adp_opts_ok(a)) return false;
    for (int k = 0; k < 2; ++k) {
        const uint8_t* const s = k ? cfg->seq2 : cfg->seq1;
        for (int j = 0; j < a.len[k]; ++j) {
            if (s[j] != 'A' && s[j] != 'C' && s[j] != 'G' && s[j] != 'T') return false;
            a.w[k][j >> 2] |= (uint32_t)s[j] << (8 * (j & 3));
        }
    }
    return true;
}

template <int G>
__global__ __launch_bounds__(VP_THREADS) void adapter_cut_kernel(AdapterArgs K) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "a group is a power-of-two part of a wave");
    constexpr int CAP = vp_cap(G), GROUPS = vp_groups(G);
    constexpr int ROW = CAP / 4 + ADP_ROW_TAIL;     // words per group
    __shared__ __attribute__((aligned(16))) uint32_t lds[GROUPS * ROW];
    __shared__ unsigned long long tot[4];
    const int g = (int)threadIdx.x & (G - 1);
    const int grp = (int)threadIdx.x / G;
    uint32_t* const row = lds + grp * ROW;
    if (threadIdx.x < 4) tot[threadIdx.x] = 0ull;
    for (int j = g; j < ADP_ROW_TAIL; j += G) row[CAP / 4 + j] = 0u;      // (no load ever writes behind the row's CAP bytes)
    __syncthreads();
    const uint64_t n_rec = K.n;
    const int nm = K.n_mates;
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};             // (the group's first lane counts; a workgroup sees far fewer than 2^32 bases)
    for (uint64_t r0 = (uint64_t)blockIdx.x * GROUPS; r0 < n_rec; r0 += (uint64_t)gridDim.x * GROUPS) {
        const uint64_t rec = r0 + (uint64_t)grp;
        const bool have = rec < n_rec;
        bool r1_kept = true;                        // read 1 leaves the trim stage with 5 bases or more: read 2 is trimmed and cut too
        for (int k = 0; k < nm; ++k) {
            // ---- the read: where, how long behind trim() and the passes in front
            const AdapterMate& M = K.m[k];
            const uint32_t vi = (uint32_t)rec * (uint32_t)nm + (uint32_t)k;       // (a slot holds fewer than 2^31 records)
            const auto [too_long, vin, start, n] = vp_line<G>(M.v, rec, have, K.view_in, vi);
            const int m = M.alen;
            int p = ADP_NONE;
            if (m > 0) {                            // (wave-uniform)
                // ---- 16 bytes per lane into the group's row
                const int nvalid = vp_nvalid(n, g);
                const uint8_t* s = nullptr;
                if (nvalid > 0) s = M.v.seq + M.v.off[rec] + start;        // (no off[rec] behind the batch's last record)
                const uint4 v = vp_load16(s, nvalid, g);
                uint32_t d[4] = {v.x, v.y, v.z, v.w};
                adp_keep16(d, nvalid);
                *reinterpret_cast<uint4*>(row + 4 * g) = make_uint4(d[0], d[1], d[2], d[3]);
                vp_publish_row();
                // ---- the search
                p = vp_group_min<G>(adp_lane_first<G>(row, n, M.w, m, K.min_overlap, g));
                vp_release_row();                                                   // (the next read overwrites the row)
            }
            if (have && g == 0) {
                K.view[vi] = view_end(vin, p != ADP_NONE, p);
                if (too_long) vp_raise_too_long(K.status);
                const int kept = p == ADP_NONE ? n : p;
                vp_count(cnt, k, rec < K.accum_limit && r1_kept, n, kept);
                if (k == 0) r1_kept = vp_read1_kept(kept);
            }
        }
    }
    if (K.stats) vp_flush(cnt, tot, K.stats, g);
}

}  // namespace aqc
#endif
