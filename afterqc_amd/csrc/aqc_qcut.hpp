// aqc_qcut.hpp — per-read sliding-window quality cutting (--cut_front / --cut_tail / --cut_right): the pass that decides, for every
// mate of a batch, which part [c0, c1) of its TRIMMED quality line the cut keeps.  The rule is tests/cut_rule.py (cut_window):
// integers only, a window of w = min(W, n) bases is good when its sum of (byte - 33) is at least Q * w.
//
//   groups   G neighbouring lanes (8, 16, 32 or 64, by the slot's longest quality line) own one read; a workgroup of four waves
//            owns 256 / G consecutive records and takes read 1, then read 2 of each (read 2's counts need read 1's outcome).
//   load     one 16-byte load per lane, at the quality line's own alignment (the arenas are padded: aqc_batch), the bytes outside
//            the line count as nothing.  The length comes from the length word, or — a record marked LEN_IRR — from its
//            quality-length word: no address is ever formed from a word that carries the mark.
//   sums     W is a run-time value of up to AQC_MAX_READ_LEN, so no window sum is built directly: 16 running sums per lane, a
//            segmented scan of the lane totals over the group, and the prefix sums P[0 .. n] of the line stand in LDS.
//   windows  pass k tests the windows that start at i = k * G + lane: P[i + w] - P[i] >= Q * w, neighbouring lanes read neighbouring
//            words.  A lane keeps one bit per pass: 16 bits.
//   ends     first good and last good start by find-first-set / count-leading-zeros and a min / max over the group, then the
//            first bad start at or behind c0 the same way.
//   out      c0 | c1 << 16 per mate and record (the mates of a record side by side), relative to the trimmed quality line.  The verdict kernels apply it to every
//            string by the string's own length (qcut_apply): a record whose quality line is not as long as its sequence line
//            is sliced the python way, like upstream's trim().
//
// The per-read functions are __host__ __device__: tests/native/qcut_selftest.cpp includes this header without HIP, deals the
// lanes of a group out by plain loops and compares with vectors the model wrote.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QCUT_HD __host__ __device__ __forceinline__
#else
#define QCUT_HD inline
#endif

namespace aqc {

constexpr int QCUT_NONE = 0x7fffffff;
constexpr int QCUT_MAX_LEN = 1000;          // AQC_MAX_READ_LEN (afterqc_hip.h), restated: the self-test includes nothing else
constexpr int QCUT_MAX_QUALITY = 93;

// the option struct of the C API, as the kernels take it (aqc_cut_config has the same five words)
struct QcutOpts { int32_t front, tail, right, window, mean_quality; };

QCUT_HD int qcut_min(int a, int b) { return a < b ? a : b; }
QCUT_HD int qcut_max(int a, int b) { return a > b ? a : b; }

// trim() of preprocesser.py:19-28 on a string of `len` bytes -> (start, length)
QCUT_HD void qcut_trim(int len, int front, int tail, int& st, int& nl) {
    const int end = tail > 0 ? qcut_max(len - tail, 0) : len;
    st = qcut_min(front, len);
    nl = qcut_max(end - st, 0);
}

// s[c0:c1] of a string of `len` bytes, python slice semantics (0 <= c0 <= c1) -> (start, length)
QCUT_HD void qcut_slice(int len, int c0, int c1, int& st, int& nl) {
    st = qcut_min(c0, len);
    nl = qcut_max(qcut_min(c1, len) - st, 0);
}

// trim() and then the cut's view (c0 | c1 << 16) on a string of `len` bytes: moves (a, l), the view the caller holds of it
QCUT_HD void qcut_apply(int& a, int& l, int front, int tail, uint32_t view) {
    int st, nl, st2, nl2;
    qcut_trim(l, front, tail, st, nl);
    qcut_slice(nl, (int)(view & 0xffffu), (int)(view >> 16), st2, nl2);
    a += st + st2;
    l = nl2;
}

// the running sums of (byte - 33) over the first `nvalid` of 16 bytes (little-endian dwords); bytes behind them add nothing
QCUT_HD void qcut_sum16(uint32_t x, uint32_t y, uint32_t z, uint32_t w, int nvalid, int p[16]) {
    const uint32_t d[4] = {x, y, z, w};
    int run = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 16; ++k) {
        const int b = (int)((d[k >> 2] >> (8 * (k & 3))) & 0xffu);
        run += k < nvalid ? b - 33 : 0;
        p[k] = run;
    }
}

// Pass k of lane g in a group of G lanes: the window that starts at i = k * G + g.  Bit k of the low half: the window exists
// (i <= n - w); of the high half: it exists and is good.  P: the prefix sums P[0 .. n] of the line, thr = Q * w.
QCUT_HD uint32_t qcut_lane_bits(const int* P, int n, int w, int thr, int g, int G, int passes) {
    uint32_t bits = 0;
    for (int k = 0; k < passes; ++k) {
        const int i = k * G + g;
        if (i <= n - w) bits |= (1u | (P[i + w] - P[i] >= thr ? 0x10000u : 0u)) << k;
    }
    return bits;
}

QCUT_HD int qcut_ffs16(uint32_t m) {          // lowest set bit of a 16-bit mask, m != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)m) - 1;
#else
    int k = 0;
    while (!((m >> k) & 1u)) ++k;
    return k;
#endif
}
QCUT_HD int qcut_fls16(uint32_t m) {          // highest set bit, m != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int)m);
#else
    int k = 15;
    while (!((m >> k) & 1u)) --k;
    return k;
#endif
}

// the lane's first / last window start whose bit is set in the 16-bit mask m; `from`: only starts >= from count
QCUT_HD int qcut_lane_first(uint32_t m, int g, int G, int from) {
    const int k0 = from > g ? (from - g + G - 1) / G : 0;          // first pass whose start is >= from
    m = k0 >= 16 ? 0u : (m >> k0) << k0;
    return m ? qcut_ffs16(m) * G + g : QCUT_NONE;
}
QCUT_HD int qcut_lane_last(uint32_t m, int g, int G) { return m ? qcut_fls16(m) * G + g : -1; }

// what the group's reductions leave: c0 from the first good start (QCUT_NONE: no good window)
QCUT_HD int qcut_front(const QcutOpts& o, int first_good) { return o.front ? first_good : 0; }
// ... and the view: last good start (-1: none), first bad start at or behind c0 (QCUT_NONE: none)
QCUT_HD uint32_t qcut_view(const QcutOpts& o, int n, int w, int first_good, int last_good, int first_bad) {
    if (n == 0) return 0u;
    if ((o.front || o.tail) && first_good == QCUT_NONE) return 0u;
    const int c0 = qcut_front(o, first_good);
    int c1 = o.tail ? last_good + w : n;
    if (o.right && first_bad != QCUT_NONE) c1 = qcut_min(c1, first_bad);
    c1 = qcut_max(c1, c0);
    return (uint32_t)c0 | ((uint32_t)c1 << 16);
}

// the window and threshold of a line of n bytes
QCUT_HD int qcut_window(const QcutOpts& o, int n) { return qcut_min(o.window, n); }
QCUT_HD bool qcut_opts_ok(const QcutOpts& o) {
    return o.window >= 1 && o.window <= QCUT_MAX_LEN && o.mean_quality >= 0 && o.mean_quality <= QCUT_MAX_QUALITY;
}
QCUT_HD bool qcut_on(const QcutOpts& o) { return o.front || o.tail || o.right; }

}  // namespace aqc

#if defined(__HIPCC__)
#include "afterqc_hip.h"
#include "aqc_prim.hpp"
#include "aqc_batch.hpp"

namespace aqc {

static_assert(QCUT_MAX_LEN == AQC_MAX_READ_LEN, "the cut pass takes every read the verdict kernels take");

struct QcutArgs {
    DevBatch b;
    QcutOpts o;
    int32_t trim_front[2], trim_tail[2];       // per mate (aqc_config::trim_front / trim_front2, ...)
    int32_t n_mates;                           // 1: read 1 only (single-end input, the function seam)
    uint32_t* view;                            // c0 | c1 << 16 of mate k of record r at [r * n_mates + k]
    unsigned long long* stats;                 // [4] reads of R1 made shorter, bases removed from them, the same for R2; NULL: not counted
    uint64_t accum_limit;
    int* status;
};

constexpr int QCUT_THREADS = 256;

// min / max over the G lanes of a group (every lane of the wave runs it)
template <int G>
__device__ __forceinline__ int qcut_group_min(int v) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) v = min(v, __shfl_xor(v, d, WAVE));
    return v;
}
template <int G>
__device__ __forceinline__ int qcut_group_max(int v) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) v = max(v, __shfl_xor(v, d, WAVE));
    return v;
}

template <int G>
__global__ __launch_bounds__(QCUT_THREADS) void quality_cut_kernel(QcutArgs K) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "a group is a power-of-two part of a wave");
    constexpr int CAP = 16 * G;                     // longest line a group takes
    constexpr int GROUPS = QCUT_THREADS / G;        // records per workgroup and round
    constexpr int AREA = CAP + 4;                   // words per group: three unused, P[0], then P[1 ..] on a 16-byte boundary
    __shared__ __attribute__((aligned(16))) int lds[GROUPS * AREA];
    __shared__ unsigned long long tot[4];
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int g = (int)threadIdx.x & (G - 1);
    const int grp = (int)threadIdx.x / G;
    int* const area = lds + grp * AREA;
    int* const P = area + 3;
    if (threadIdx.x < 4) tot[threadIdx.x] = 0ull;
    if (g == 0) P[0] = 0;
    __syncthreads();
    const DevBatch& b = K.b;
    const uint64_t n_rec = b.n;
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};             // (the group's first lane counts; a workgroup sees far fewer than 2^32 bases)
    for (uint64_t r0 = (uint64_t)blockIdx.x * GROUPS; r0 < n_rec; r0 += (uint64_t)gridDim.x * GROUPS) {
        const uint64_t rec = r0 + (uint64_t)grp;
        const bool have = rec < n_rec;
        uint32_t lw[2] = {0u, 0u};
        bool irr = false;
        if (have) {
            lw[0] = b.len1[rec];
            if (K.n_mates == 2) lw[1] = b.len2[rec];
            irr = b.qlen1 != nullptr && ((lw[0] | lw[1]) & LEN_IRR) != 0u;
        }
        bool r1_kept = true;                        // read 1 leaves the trim stage with 5 bases or more: read 2 is trimmed and cut too
        for (int k = 0; k < K.n_mates; ++k) {
            // ---- the line: where, how long after trim()
            const int L = (int)(lw[k] & LEN_MASK);
            int n_line = L;
            if (irr) n_line = (int)((k ? b.qlen2[rec] : b.qlen1[rec]) & QLEN_MASK);
            bool too_long = n_line > CAP || n_line > AQC_MAX_READ_LEN;
            if (!have || too_long) n_line = 0;
            int q0 = 0, n = 0;
            qcut_trim(n_line, K.trim_front[k], K.trim_tail[k], q0, n);
            const uint8_t* q = nullptr;
            if (have && n > 0) {
                const uint32_t* const qo = k ? (b.qoff2 ? b.qoff2 : b.off2) : (b.qoff1 ? b.qoff1 : b.off1);
                q = (k ? b.qual2 : b.qual1) + qo[rec] + q0;
            }
            // ---- 16 bytes per lane, their running sums, the scan over the group
            const int nvalid = min(max(n - 16 * g, 0), 16);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (nvalid > 0) v = load16u(q + 16 * g);
            int p[16];
            qcut_sum16(v.x, v.y, v.z, v.w, nvalid, p);
            const int incl = wave_incl_sum(p[15], lane);
            int before = 0;
            if (G < WAVE) {
                const int first = lane & ~(G - 1);                                  // the group's first lane in the wave
                const int prev = __shfl(incl, max(first - 1, 0), WAVE);             // (every lane of the wave runs the exchange)
                before = first ? prev : 0;
            }
            const int base = incl - p[15] - before;
            int4* const S = reinterpret_cast<int4*>(area + 4 + 16 * g);            // P[16 g + 1 .. 16 g + 16]
            S[0] = make_int4(base + p[0], base + p[1], base + p[2], base + p[3]);
            S[1] = make_int4(base + p[4], base + p[5], base + p[6], base + p[7]);
            S[2] = make_int4(base + p[8], base + p[9], base + p[10], base + p[11]);
            S[3] = make_int4(base + p[12], base + p[13], base + p[14], base + p[15]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- the windows: one bit per pass and lane
            const int w = qcut_window(K.o, n);
            const int thr = K.o.mean_quality * w;
            const int starts = n > 0 ? n - w + 1 : 0;
            const int passes = (wave_max_i(starts) + G - 1) / G;                    // (wave-uniform, <= 16)
            const uint32_t bits = qcut_lane_bits(P, n, w, thr, g, G, passes);
            const uint32_t good = bits >> 16, bad = (bits & 0xffffu) & ~good;
            const int first_good = qcut_group_min<G>(qcut_lane_first(good, g, G, 0));
            const int last_good = qcut_group_max<G>(qcut_lane_last(good, g, G));
            const int c0 = first_good == QCUT_NONE ? 0 : qcut_front(K.o, first_good);
            const int first_bad = qcut_group_min<G>(qcut_lane_first(bad, g, G, c0));
            const uint32_t view = qcut_view(K.o, n, w, first_good, last_good, first_bad);
            __builtin_amdgcn_wave_barrier();                                        // (the next line's sums overwrite P)
            if (have && g == 0) {
                K.view[rec * (uint64_t)K.n_mates + (uint64_t)k] = view;
                if (too_long) atomicCAS(K.status, 0, AQC_ERR_READ_TOO_LONG);
                // what the cut takes from the SEQUENCE line (sliced by its own length, like the quality line)
                int st, tl, st2, kept;
                qcut_trim(L, K.trim_front[k], K.trim_tail[k], st, tl);
                qcut_slice(tl, (int)(view & 0xffffu), (int)(view >> 16), st2, kept);
                if (rec < K.accum_limit && r1_kept && kept < tl) { cnt[2 * k] += 1u; cnt[2 * k + 1] += (uint32_t)(tl - kept); }
                if (k == 0) r1_kept = kept >= 5;
            }
        }
    }
    if (K.stats) {
        if (g == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cnt[j]) atomicAdd(&tot[j], (unsigned long long)cnt[j]);
        }
        __syncthreads();
        if (threadIdx.x < 4 && tot[threadIdx.x]) atomicAdd(&K.stats[threadIdx.x], tot[threadIdx.x]);
    }
}

}  // namespace aqc
#endif
