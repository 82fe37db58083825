// aqc_polytail.hpp — cutting poly-G / poly-X tails from each read (--trim_poly_g / --trim_poly_x): the pass that looks, for every mate
// of a batch, at the tail of its trimmed, quality-cut and adapter-trimmed SEQUENCE line and ends the mate's view in front of a run of
// one letter.  The rule is tests/poly_rule.py (poly_end).  For a letter X with minimum length L and a line of n bytes:
//   mm(u)    the bytes among the last u that are not exactly X
//   fail(u)  mm(u) > 5, or u >= L and mm(u) > (u >> 3)
//   scanned  (the smallest u of 1 .. n with fail(u)) - 1; n where there is none
//   t        scanned < L: nothing; else the largest u <= scanned with s[n - u] == X — the line ends at n - t
// Every enabled letter is tried on the same line, the smallest end wins.
//
// The frame — lanes per read, the 16-byte load, the view word, the counts — is that of every view pass: aqc_viewpass.hpp.  Here:
//
//   line     the sequence line as vp_line forms it, behind trim() and the view that comes in — an earlier pass's, else VIEW_ALL.
//            No LDS row: a lane keeps its 16 bytes.
//   masks    per enabled letter 16 bits, one per byte of the lane that is not the letter; the bytes behind the line are no bytes.
//   scan     the lanes' mismatch counts, two letters to a dword (a wave holds at most 1024 a letter), go through one wave-wide
//            prefix sum; what a lane has BEHIND it in its group is the group's last sum minus its own.
//   decide   fail can first hold only at a mismatched byte or at u == L, and never in front of six mismatches: a lane walks at
//            most 6 - behind of its own mismatches from the tail on, and looks at the byte of u == L if it holds it.  A group
//            minimum gives scanned, a group maximum over the lanes' first X inside the scanned tail gives t.
//   leave    most reads have no tail.  In front of the scan the lane with the line's last byte counts, with its neighbour, the
//            mismatches among the last min(L, 16) bytes: more than min(5, L >> 3), or n < L, and the letter cannot pass; a wave
//            without a candidate leaves there.  Behind the scan, when no group of the wave has a letter with scanned >= L, the wave
//            skips the second half.
//   out      the group's first lane composes the view (c0, c0 + end) — or leaves the one that came in — and counts.
//
// The four L travel in the kernel's arguments; there is no table in device memory.  The per-read functions are __host__ __device__:
// tests/native/polytail_selftest.cpp includes this header without HIP, deals the lanes of a group out by plain loops and compares
// with vectors the model wrote.
#pragma once
#include <stdint.h>

#include "aqc_viewpass.hpp"

namespace aqc {

constexpr int POLY_NONE = 0x7fffffff;
constexpr int POLY_LETTERS = 4;                 // A, C, G, T: the order of aqc_poly_config::min_len
constexpr int POLY_MAX_MISMATCH = 5;            // more mismatches than this end the scan whatever its length
constexpr int POLY_MAX_MIN_LEN = 1000;          // (AQC_MAX_READ_LEN: a longer tail than a read does not exist)

// the minimum lengths as the kernel takes them: 0 = that letter is not tried
struct PolyOpts { int32_t min_len[POLY_LETTERS]; };

VP_HD uint8_t poly_letter(int x) { return (uint8_t)(x == 0 ? 'A' : x == 1 ? 'C' : x == 2 ? 'G' : 'T'); }
VP_HD bool poly_on(const PolyOpts& o) { return (o.min_len[0] | o.min_len[1] | o.min_len[2] | o.min_len[3]) != 0; }
VP_HD bool poly_opts_ok(const PolyOpts& o) {
    for (int x = 0; x < POLY_LETTERS; ++x)
        if (o.min_len[x] < 0 || o.min_len[x] > POLY_MAX_MIN_LEN) return false;
    return true;
}

VP_HD int poly_popc(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(m);
#else
    return __builtin_popcount(m);
#endif
}
VP_HD int poly_ffs16(uint32_t m) {              // lowest set bit, m != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)m) - 1;
#else
    return __builtin_ctz(m);
#endif
}
VP_HD int poly_fls16(uint32_t m) {              // highest set bit, m != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int)m);
#else
    return 31 - __builtin_clz(m);
#endif
}

// bit j: byte j of the little-endian dword is not zero
VP_HD uint32_t poly_nonzero4(uint32_t y) {
    const uint32_t nz = ((((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u) >> 7;      // bits 0, 8, 16, 24
    return (nz * 0x00204081u >> 21) & 0xfu;                                                 // ... moved next to each other (no two products meet)
}

// the lane's bytes that belong to the line, one bit each
VP_HD uint32_t poly_valid16(int nvalid) { return (1u << nvalid) - 1u; }

// bit j: byte j of the lane's 16 belongs to the line and is not exactly the letter
VP_HD uint32_t poly_mismatch16(const uint32_t d[4], uint8_t letter, int nvalid) {
    const uint32_t x4 = 0x01010101u * (uint32_t)letter;
    const uint32_t m = poly_nonzero4(d[0] ^ x4) | (poly_nonzero4(d[1] ^ x4) << 4) | (poly_nonzero4(d[2] ^ x4) << 8) | (poly_nonzero4(d[3] ^ x4) << 12);
    return m & poly_valid16(nvalid);
}

// A test in front of the scan.  scanned >= L needs n >= L and no fail(L): mm(L) <= min(5, L >> 3) — and the last w = min(L, 16) bytes
// of the line, which at most two neighbouring lanes hold, have no more mismatches than its last L.
VP_HD int poly_window(int L) { return vp_min(L, 16); }
// lane g's mismatches among the line's last w bytes
VP_HD int poly_window_count(uint32_t mm16, int n, int g, int w) {
    const int lo = vp_max(n - w - 16 * g, 0);
    return lo < vp_nvalid(n, g) ? poly_popc(mm16 >> lo) : 0;
}
VP_HD bool poly_candidate(int n, int L, int mm_w) { return n >= L && mm_w <= vp_min(POLY_MAX_MISMATCH, L >> 3); }

// Lane g of a line of n bytes, `behind` mismatches in the lanes behind it: the smallest u at which fail(u) holds among the places
// the lane decides — its mismatched bytes and the byte of u == L; POLY_NONE: none.  Byte j of the lane is u = n - 16 g - j.
VP_HD int poly_lane_fail(uint32_t mm16, int behind, int n, int g, int L) {
    const int top = n - 16 * g;
    int best = POLY_NONE;
    const int jl = top - L;
    if (jl >= 0 && jl < 16) {
        const int c = behind + poly_popc(mm16 >> jl);
        if (c > vp_min(POLY_MAX_MISMATCH, L >> 3)) best = L;
    }
    int c = behind;
    uint32_t m = mm16;
    while (m != 0u && c <= POLY_MAX_MISMATCH) {         // (in front of six mismatches nothing is left to decide)
        const int j = poly_fls16(m);
        m ^= 1u << j;
        ++c;
        const int u = top - j;
        if (c > POLY_MAX_MISMATCH || (u >= L && c > (u >> 3))) { best = vp_min(best, u); break; }
    }
    return best;
}

// the group's smallest failing u -> scanned
VP_HD int poly_scanned(int first_fail, int n) { return first_fail == POLY_NONE ? n : first_fail - 1; }

// Lane g: the largest u <= scanned at which the lane holds the letter (eq16: one bit per byte that is the letter); 0: none
VP_HD int poly_lane_last(uint32_t eq16, int n, int g, int scanned) {
    const int top = n - 16 * g;
    const int j0 = vp_max(top - scanned, 0);            // bytes in front of j0 lie outside the scanned tail
    if (j0 >= 16) return 0;
    const uint32_t m = (eq16 >> j0) << j0;
    return m ? top - poly_ffs16(m) : 0;
}

// where the letter ends the line: n - t, or n (nothing cut)
VP_HD int poly_end(int n, int L, int scanned, int t) { return (scanned >= L && t > 0) ? n - t : n; }

}  // namespace aqc

#if defined(__HIPCC__)
#include "aqc_batch.hpp"

namespace aqc {

struct PolyArgs {
    ViewMate m[2];
    uint64_t n;                                // records
    int32_t min_len[POLY_LETTERS];             // PolyOpts::min_len
    int32_t n_mates;                           // 1: read 1 only (single-end input, the function seam)
    const uint32_t* view_in;                   // the earlier passes' views, laid out like `view` (may be `view` itself); NULL: none ran, (0, 0xffff)
    uint32_t* view;                            // c0 | c1 << 16 of mate k of record r at [r * n_mates + k]
    unsigned long long* stats;                 // [4] reads of R1 made shorter, bases removed from them, the same for R2; NULL: not counted
    uint64_t accum_limit;
    int* status;
};

// the C API's lengths as the kernel takes them (NULL: off); false: a length outside 0 .. 1000
inline bool poly_from_config(const aqc_poly_config* cfg, PolyOpts& o) {
    o = PolyOpts{};
    if (!cfg) return true;
    for (int x = 0; x < POLY_LETTERS; ++x) o.min_len[x] = cfg->min_len[x];
    return poly_opts_ok(o);
}

template <int G>
__global__ __launch_bounds__(VP_THREADS) void poly_tail_kernel(PolyArgs K) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "a group is a power-of-two part of a wave");
    constexpr int GROUPS = vp_groups(G);
    __shared__ unsigned long long tot[4];
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int g = (int)threadIdx.x & (G - 1);
    const int grp = (int)threadIdx.x / G;
    if (threadIdx.x < 4) tot[threadIdx.x] = 0ull;
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
            const ViewMate& M = K.m[k];
            const uint32_t vi = (uint32_t)rec * (uint32_t)nm + (uint32_t)k;       // (a slot holds fewer than 2^31 records)
            const auto [too_long, vin, start, n] = vp_line<G>(M, rec, have, K.view_in, vi);
            // ---- 16 bytes per lane
            const int nvalid = vp_nvalid(n, g);
            const uint8_t* s = nullptr;
            if (nvalid > 0) s = M.seq + M.off[rec] + start;            // (no off[rec] behind the batch's last record)
            const uint4 v = vp_load16(s, nvalid, g);
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
            // ---- per letter: the mismatch mask, the mismatches behind the lane, scanned
            uint32_t mm[POLY_LETTERS] = {0u, 0u, 0u, 0u};
            int scanned[POLY_LETTERS] = {0, 0, 0, 0};
            bool open = false;                      // a letter of the lane's group has scanned >= L
#pragma unroll
            for (int x0 = 0; x0 < POLY_LETTERS; x0 += 2) {
                const int L0 = K.min_len[x0], L1 = K.min_len[x0 + 1];
                if ((L0 | L1) == 0) continue;       // (wave-uniform: the lengths are arguments)
                mm[x0] = L0 ? poly_mismatch16(d, poly_letter(x0), nvalid) : 0u;
                mm[x0 + 1] = L1 ? poly_mismatch16(d, poly_letter(x0 + 1), nvalid) : 0u;
                // (most reads have no tail: the lane that holds the line's last byte asks, with its neighbour's count, whether a letter
                //  can still pass; a wave without such a lane leaves before the scan)
                const int wc = poly_window_count(mm[x0], n, g, poly_window(L0)) | (poly_window_count(mm[x0 + 1], n, g, poly_window(L1)) << 16);
                const int up = __shfl_up(wc, 1, WAVE);                               // (every lane of the wave runs the exchange)
                const int wt = wc + (g > 0 ? up : 0);
                const bool cand = n > 0 && g == ((n - 1) >> 4) &&
                                  ((L0 && poly_candidate(n, L0, wt & 0xffff)) || (L1 && poly_candidate(n, L1, wt >> 16)));
                if (!vp_wave_any(cand)) continue;
                const int incl = wave_incl_sum(poly_popc(mm[x0]) | (poly_popc(mm[x0 + 1]) << 16), lane);
                const int behind = __shfl(incl, lane | (G - 1), WAVE) - incl;      // (every lane of the wave runs the exchange)
                if (L0) {
                    scanned[x0] = poly_scanned(vp_group_min<G>(poly_lane_fail(mm[x0], behind & 0xffff, n, g, L0)), n);
                    open = open || scanned[x0] >= L0;
                }
                if (L1) {
                    scanned[x0 + 1] = poly_scanned(vp_group_min<G>(poly_lane_fail(mm[x0 + 1], behind >> 16, n, g, L1)), n);
                    open = open || scanned[x0 + 1] >= L1;
                }
            }
            // ---- the leftmost letter inside the scanned tail, the smallest end
            int end = n;
            if (vp_wave_any(open)) {
                const uint32_t valid = poly_valid16(nvalid);
#pragma unroll
                for (int x = 0; x < POLY_LETTERS; ++x) {
                    const int L = K.min_len[x];
                    if (L == 0) continue;
                    const int t = vp_group_max<G>(scanned[x] >= L ? poly_lane_last(~mm[x] & valid, n, g, scanned[x]) : 0);
                    end = vp_min(end, poly_end(n, L, scanned[x], t));
                }
            }
            if (have && g == 0) {
                K.view[vi] = view_end(vin, end < n, end);
                if (too_long) vp_raise_too_long(K.status);
                vp_count(cnt, k, rec < K.accum_limit && r1_kept, n, end);
                if (k == 0) r1_kept = vp_read1_kept(end);
            }
        }
    }
    if (K.stats) vp_flush(cnt, tot, K.stats, g);
}

}  // namespace aqc
#endif
