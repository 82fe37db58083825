// aqc_adpcensus.hpp — the adapter census of pass 1 (--adapter_sequence auto): for every read of a range of a slot's records, which of
// up to 16 probes of 12 bases stand somewhere in its raw SEQUENCE line, and per probe the number of reads that hold it.  The rule is
// tests/detect_rule.py (holds): the 12 bytes byte for byte at any place 0 .. n - 12 of the line before -f / -t; an N or a lower-case
// letter is no match, a read under 12 bases holds nothing, a read that holds a probe twice counts once for it.
//
// The frame — lanes per read, the 16-byte load, the too-long line, the grid — is that of the view passes: aqc_viewpass.hpp.  No view
// is written: the census runs beside qc_stat on the pass-1 sample, before pass 2 is configured.  Here:
//
//   line     the sequence line, its 16 bytes per lane stored into the LDS row of the group; the bytes behind the line, and the four
//            words behind the row, are 0 — no base.  A probe is 12 letters of ACGT: a place whose 12 bytes reach behind the line
//            compares a 0 with a letter and cannot match, so no place is tested for lying in front of n - 12.
//   probes   travel in the kernel's by-value arguments, three dwords each: wave-uniform scalar registers, no
//            table in device memory.
//   search   a lane tests the 16 places that start in its own 16 bytes, from the seven row words that hold their 27 bytes.  One
//            dword per place is compared against one dword per probe.  That dword is not the place's first four bytes — of A C G T
//            text one place in 256 has a given first dword, so a wave's 1024 places would send it down the exact comparison for
//            nearly every read and probe — but a code of all twelve: bits 1 and 2 of a byte tell A, C, G and T apart (cen_code), and
//            the three dwords of a place, masked to those bits and shifted against each other, fill one dword.  Equal letters give
//            equal codes, so no match is lost; a place that is no match has the probe's code only where bytes outside A C G T
//            stand in for letters (an N has G's bits).  A lane whose code compare hit walks its places again, from the row, and
//            compares the three dwords themselves: that decides.
//   count    the probes a lane holds are a bit mask, OR-reduced over the group; the group's first lane counts reads looked at and
//            reads per probe in registers; vp_flush adds them through the workgroup's LDS words to the context's, one global
//            atomic per probe and workgroup.
//
// The per-read functions are __host__ __device__: tests/native/adpcensus_selftest.cpp includes this header without HIP, deals the
// lanes of a group out by plain loops and compares with vectors the model wrote.
#pragma once
#include <stdint.h>

#include "aqc_adapter.hpp"

namespace aqc {

constexpr int CEN_PROBE_LEN = 12, CEN_PROBE_WORDS = CEN_PROBE_LEN / 4, CEN_MAX_PROBES = 16;
// words behind the 16 * G bytes of a group's row: the row's last lane reads the three words behind its own four, and a place at the
// row's last byte one more as the high half of its last pair (the row stays a multiple of 16 bytes)
constexpr int CEN_ROW_TAIL = 4;
constexpr int CEN_COUNTS = 1 + CEN_MAX_PROBES;          // reads looked at, reads holding probe i at [1 + i]
constexpr uint32_t CEN_CODE_BITS = 0x06060606u;         // bits 1, 2 of a byte: A 00, C 01, T 10, G 11

// the probes as the kernel takes them: n of them, the bytes little-endian in the dwords
struct CensusProbes {
    int32_t n;
    uint32_t w[CEN_MAX_PROBES][CEN_PROBE_WORDS];
};

// the code of twelve bytes, from their three dwords masked to CEN_CODE_BITS: byte b of the code holds the letters b, b + 4, b + 8
VP_HD uint32_t cen_code(uint32_t m0, uint32_t m1, uint32_t m2) { return m0 | (m1 << 2) | (m2 << 4); }

// n probes of CEN_PROBE_LEN letters each; false: a bad n, a letter that is no base
inline bool cen_from_letters(int n, const uint8_t (*seq)[CEN_PROBE_LEN], CensusProbes& p) {
    p = CensusProbes{};
    if (n < 1 || n > CEN_MAX_PROBES) return false;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < CEN_PROBE_LEN; ++j) {
            const uint8_t b = seq[i][j];
            if (b != 'A' && b != 'C' && b != 'G' && b != 'T') return false;
            p.w[i][j >> 2] |= (uint32_t)b << (8 * (j & 3));
        }
    p.n = n;
    return true;
}

// the dword D (0 .. 2) of the 12 bytes at place p of the row
VP_HD uint32_t cen_dword_at(const uint32_t* row, int p, int D) {
    const uint32_t* const wp = row + (p >> 2) + D;
    return adp_bytes_at(wp[0], wp[1], p & 3);
}

// does the probe of dwords w stand at one of lane g's 16 places?  The bytes themselves, from the row (rare: behind a code hit)
VP_HD bool cen_exact(const uint32_t* row, const uint32_t (&w)[CEN_PROBE_WORDS], int g) {
    bool all = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int j = 0; j < 16 && !all; ++j) {
        const int p = 16 * g + j;
        all = cen_dword_at(row, p, 0) == w[0] && cen_dword_at(row, p, 1) == w[1] && cen_dword_at(row, p, 2) == w[2];
    }
    return all;
}

// Probe I and those behind it against the codes h of a lane's 16 places.  (Written out probe by probe — a recursion the compiler
// flattens — so that P.w[I] names three scalar registers; the test on P.n is wave-uniform.)
template <int I>
VP_HD void cen_probes(const uint32_t* row, const uint32_t (&h)[16], const CensusProbes& P, int g, uint32_t& held) {
    if constexpr (I < CEN_MAX_PROBES) {
        if (I >= P.n) return;
        const uint32_t c = cen_code(P.w[I][0] & CEN_CODE_BITS, P.w[I][1] & CEN_CODE_BITS, P.w[I][2] & CEN_CODE_BITS);      // (scalar arithmetic)
        bool any = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 16; ++j) any = any || h[j] == c;
        if (any && cen_exact(row, P.w[I], g)) held |= 1u << I;
        cen_probes<I + 1>(row, h, P, g, held);
    }
}

// Lane g of a group: the probes that stand at one of the 16 places 16 g .. 16 g + 15 of the read in `row` (zero bytes behind the
// line, CEN_ROW_TAIL zero words behind 16 * G bytes), bit i for probe i.
VP_HD uint32_t cen_lane_held(const uint32_t* row, const CensusProbes& P, int g) {
    const uint32_t* const wp = row + 4 * g;
    uint32_t m[7];                                   // the words under the lane's places, their code bits
    uint32_t y[24];                                  // ... byte-aligned: y[j] the first dword of place j, y[j + 4] its second, y[j + 8] its third
    uint32_t h[16];                                  // the code of each place
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 7; ++k) m[k] = wp[k] & CEN_CODE_BITS;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 24; ++j) y[j] = adp_bytes_at(m[j >> 2], m[(j >> 2) + 1], j & 3);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 16; ++j) h[j] = cen_code(y[j], y[j + 4], y[j + 8]);
    uint32_t held = 0u;
    cen_probes<0>(row, h, P, g, held);
    return held;
}

}  // namespace aqc

#if defined(__HIPCC__)
#include "aqc_batch.hpp"

namespace aqc {

struct CensusArgs {
    const uint8_t* seq;                        // the mate's sequence lines (raw: no trim, no view)
    const uint32_t *off, *len;
    uint64_t first, count;                     // records [first, first + count) of the slot
    unsigned long long* acc;                   // [CEN_COUNTS] of the context, per `which`
    int* status;
    CensusProbes probes;
};

template <int G>
__global__ __launch_bounds__(VP_THREADS) void adapter_census_kernel(CensusArgs K) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "a group is a power-of-two part of a wave");
    constexpr int CAP = vp_cap(G), GROUPS = vp_groups(G);
    constexpr int ROW = CAP / 4 + CEN_ROW_TAIL;     // words per group
    __shared__ __attribute__((aligned(16))) uint32_t lds[GROUPS * ROW];
    __shared__ unsigned long long tot[CEN_COUNTS];
    const int g = (int)threadIdx.x & (G - 1);
    const int grp = (int)threadIdx.x / G;
    uint32_t* const row = lds + grp * ROW;
    if (threadIdx.x < CEN_COUNTS) tot[threadIdx.x] = 0ull;
    if (g < CEN_ROW_TAIL) row[CAP / 4 + g] = 0u;                                  // (no load ever writes behind the row's CAP bytes)
    __syncthreads();
    const uint64_t n_rec = K.count;
    uint32_t cnt[CEN_COUNTS];                       // (the group's first lane counts; a workgroup sees fewer than 2^32 reads)
#pragma unroll
    for (int j = 0; j < CEN_COUNTS; ++j) cnt[j] = 0u;
    for (uint64_t r0 = (uint64_t)blockIdx.x * GROUPS; r0 < n_rec; r0 += (uint64_t)gridDim.x * GROUPS) {
        const uint64_t r = r0 + (uint64_t)grp;
        const bool have = r < n_rec;
        const uint64_t rec = K.first + r;
        // ---- the read: where, how long (raw: the line before -f / -t)
        int n = have ? (int)(K.len[rec] & LEN_MASK) : 0;
        const bool too_long = vp_too_long<G>(n);
        if (too_long) n = 0;
        // ---- 16 bytes per lane into the group's row
        const int nvalid = vp_nvalid(n, g);
        const uint8_t* s = nullptr;
        if (nvalid > 0) s = K.seq + K.off[rec];                                   // (no off[rec] behind the range's last record)
        const uint4 v = vp_load16(s, nvalid, g);
        uint32_t d[4] = {v.x, v.y, v.z, v.w};
        adp_keep16(d, nvalid);
        *reinterpret_cast<uint4*>(row + 4 * g) = make_uint4(d[0], d[1], d[2], d[3]);
        vp_publish_row();
        // ---- the search
        uint32_t held = cen_lane_held(row, K.probes, g);
        if (vp_wave_any(held != 0u)) held = vp_group_or<G>(held);
        vp_release_row();                                                         // (the next read overwrites the row)
        if (have && g == 0) {
            if (too_long) vp_raise_too_long(K.status);
            cnt[0] += 1u;
#pragma unroll
            for (int i = 0; i < CEN_MAX_PROBES; ++i) cnt[1 + i] += (held >> i) & 1u;
        }
    }
    vp_flush(cnt, tot, K.acc, g);
}

}  // namespace aqc
#endif
