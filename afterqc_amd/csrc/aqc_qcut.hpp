// aqc_qcut.hpp — per-read sliding-window quality cutting (--cut_front / --cut_tail / --cut_right): the pass that decides, for every
// mate of a batch, which part [c0, c1) of its TRIMMED quality line the cut keeps.  The rule is tests/cut_rule.py (cut_window):
// integers only, a window of w = min(W, n) bases is good when its sum of (byte - 33) is at least Q * w.
//
// The frame — lanes per read, the 16-byte load, the view word, the counts — is that of every view pass: aqc_viewpass.hpp.  Here:
//
//   line     the quality line.  Its length comes from the length word, or — a record marked LEN_IRR — from its quality-length
//            word: no address is ever formed from a word that carries the mark.  The bytes outside the line count as nothing.
//   sums     W is a run-time value of up to AQC_MAX_READ_LEN, so no window sum is built directly: 16 running sums per lane, a
//            segmented scan of the lane totals over the group, and the prefix sums P[0 .. n] of the line stand in LDS.
//   windows  pass k tests the windows that start at i = k * G + lane: P[i + w] - P[i] >= Q * w, neighbouring lanes read neighbouring
//            words.  A lane keeps one bit per pass: 16 bits.
//   ends     first good and last good start by find-first-set / count-leading-zeros and a min / max over the group, then the
//            first bad start at or behind c0 the same way.
//   out      the view (c0, c1), relative to the trimmed quality line; the counts are what it takes from the SEQUENCE line.
//
// The per-read functions are __host__ __device__: tests/native/qcut_selftest.cpp includes this header without HIP, deals the
// lanes of a group out by plain loops and compares with vectors the model wrote.
#pragma once
#include <stdint.h>

#include "aqc_viewpass.hpp"

namespace aqc {

constexpr int QCUT_NONE = 0x7fffffff;
constexpr int QCUT_MAX_QUALITY = 93;

// the option struct of the C API, as the kernels take it (aqc_cut_config has the same five words)
struct QcutOpts { int32_t front, tail, right, window, mean_quality; };

// the running sums of (byte - 33) over the first `nvalid` of 16 bytes (little-endian dwords); bytes behind them add nothing
VP_HD void qcut_sum16(uint32_t x, uint32_t y, uint32_t z, uint32_t w, int nvalid, int p[16]) {
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
VP_HD uint32_t qcut_lane_bits(const int* P, int n, int w, int thr, int g, int G, int passes) {
    uint32_t bits = 0;
    for (int k = 0; k < passes; ++k) {
        const int i = k * G + g;
        if (i <= n - w) bits |= (1u | (P[i + w] - P[i] >= thr ? 0x10000u : 0u)) << k;
    }
    return bits;
}

VP_HD int qcut_ffs16(uint32_t m) {          // lowest set bit of a 16-bit mask, m != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)m) - 1;
#else
    int k = 0;
    while (!((m >> k) & 1u)) ++k;
    return k;
#endif
}
VP_HD int qcut_fls16(uint32_t m) {          // highest set bit, m != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int)m);
#else
    int k = 15;
    while (!((m >> k) & 1u)) --k;
    return k;
#endif
}

// the lane's first / last window start whose bit is set in the 16-bit mask m; `from`: only starts >= from count
VP_HD int qcut_lane_first(uint32_t m, int g, int G, int from) {
    const int k0 = from > g ? (from - g + G - 1) / G : 0;          // first pass whose start is >= from
    m = k0 >= 16 ? 0u : (m >> k0) << k0;
    return m ? qcut_ffs16(m) * G + g : QCUT_NONE;
}
VP_HD int qcut_lane_last(uint32_t m, int g, int G) { return m ? qcut_fls16(m) * G + g : -1; }

// what the group's reductions leave: c0 from the first good start (QCUT_NONE: no good window)
VP_HD int qcut_front(const QcutOpts& o, int first_good) { return o.front ? first_good : 0; }
// ... and the view: last good start (-1: none), first bad start at or behind c0 (QCUT_NONE: none)
VP_HD uint32_t qcut_view(const QcutOpts& o, int n, int w, int first_good, int last_good, int first_bad) {
    if (n == 0) return 0u;
    if ((o.front || o.tail) && first_good == QCUT_NONE) return 0u;
    const int c0 = qcut_front(o, first_good);
    int c1 = o.tail ? last_good + w : n;
    if (o.right && first_bad != QCUT_NONE) c1 = vp_min(c1, first_bad);
    c1 = vp_max(c1, c0);
    return view_word(c0, c1);
}

// the window and threshold of a line of n bytes
VP_HD int qcut_window(const QcutOpts& o, int n) { return vp_min(o.window, n); }
VP_HD bool qcut_opts_ok(const QcutOpts& o) {
    return o.window >= 1 && o.window <= VP_MAX_LEN && o.mean_quality >= 0 && o.mean_quality <= QCUT_MAX_QUALITY;
}
VP_HD bool qcut_on(const QcutOpts& o) { return o.front || o.tail || o.right; }

}  // namespace aqc

#if defined(__HIPCC__)
#include "aqc_batch.hpp"

namespace aqc {

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

template <int G>
__global__ __launch_bounds__(VP_THREADS) void quality_cut_kernel(QcutArgs K) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "a group is a power-of-two part of a wave");
    constexpr int CAP = vp_cap(G), GROUPS = vp_groups(G);
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
            const bool too_long = vp_too_long<G>(n_line);
            if (!have || too_long) n_line = 0;
            int q0 = 0, n = 0;
            vp_trim(n_line, K.trim_front[k], K.trim_tail[k], q0, n);
            const uint8_t* q = nullptr;
            if (have && n > 0) {
                const uint32_t* const qo = k ? (b.qoff2 ? b.qoff2 : b.off2) : (b.qoff1 ? b.qoff1 : b.off1);
                q = (k ? b.qual2 : b.qual1) + qo[rec] + q0;
            }
            // ---- 16 bytes per lane, their running sums, the scan over the group
            const int nvalid = vp_nvalid(n, g);
            const uint4 v = vp_load16(q, nvalid, g);
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
            vp_publish_row();
            // ---- the windows: one bit per pass and lane
            const int w = qcut_window(K.o, n);
            const int thr = K.o.mean_quality * w;
            const int starts = n > 0 ? n - w + 1 : 0;
            const int passes = (wave_max_i(starts) + G - 1) / G;                    // (wave-uniform, <= 16)
            const uint32_t bits = qcut_lane_bits(P, n, w, thr, g, G, passes);
            const uint32_t good = bits >> 16, bad = (bits & 0xffffu) & ~good;
            const int first_good = vp_group_min<G>(qcut_lane_first(good, g, G, 0));
            const int last_good = vp_group_max<G>(qcut_lane_last(good, g, G));
            const int c0 = first_good == QCUT_NONE ? 0 : qcut_front(K.o, first_good);
            const int first_bad = vp_group_min<G>(qcut_lane_first(bad, g, G, c0));
            const uint32_t view = qcut_view(K.o, n, w, first_good, last_good, first_bad);
            vp_release_row();                                                       // (the next line's sums overwrite P)
            if (have && g == 0) {
                K.view[rec * (uint64_t)K.n_mates + (uint64_t)k] = view;
                if (too_long) vp_raise_too_long(K.status);
                // what the cut takes from the SEQUENCE line (sliced by its own length, like the quality line)
                int st, tl, st2, kept;
                vp_trim(L, K.trim_front[k], K.trim_tail[k], st, tl);
                view_slice(tl, view, st2, kept);
                vp_count(cnt, k, rec < K.accum_limit && r1_kept, tl, kept);
                if (k == 0) r1_kept = vp_read1_kept(kept);
            }
        }
    }
    if (K.stats) vp_flush(cnt, tot, K.stats, g);
}

}  // namespace aqc
#endif
