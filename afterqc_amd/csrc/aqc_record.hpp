// aqc_record.hpp — generation 1 ("wave per record") of the AfterQC hot path (wave64, LDS-staged): one 64-lane wavefront owns one read
// pair, stages the four byte strings of the pair in LDS and runs the whole per-read pipeline of preprocesser.py:436-631 on them with
// ballot / popcount reductions.  Every stage is an exact restatement of the reference arithmetic; comments cite the reference lines.
// Integer / byte work only — no MFMA, no floats except the f64 circle test of isInBubble.  The screens, process_record_wave and the
// two general verdict kernels built on it.  It defines kernels: aqc_capi_run.hip is the one unit that includes it (aqc_seams.hpp,
// of the same unit, builds on it; the complement table the statRead stage shares with it is in aqc_prim.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"
#include "aqc_prim.hpp"
#include "aqc_batch.hpp"
#include "aqc_viewpass.hpp"

namespace aqc {

constexpr int BLOCK = 256;
constexpr int WPB = BLOCK / WAVE;      // waves (= records in flight) per workgroup
constexpr int LSTR = 1024;             // LDS bytes per staged string (AQC_MAX_READ_LEN = 1000)

// ALL_BASES index A,T,C,G -> 0..3 (qualitycontrol.py:24), -1 otherwise
__device__ __forceinline__ int base_idx(uint8_t c) {
    return c == 'A' ? 0 : c == 'T' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : -1;
}

// the 9 symbols hasPolyX counts (preprocesser.py:35)
__device__ __forceinline__ bool poly_symbol(uint8_t c) { return comp_strict(c) != 0; }

// ------------------------------------------------------------------------------------------------
// util.overlap_hm (util.py:158-212) for one pair, executed by one wavefront.
//   r1  : LDS pointer to the current read 1 (len1 bytes)
//   c2  : LDS pointer to complement-or-N of the current read 2 in ORIGINAL orientation (len2 bytes)
//         -> reverse_r2[i] == c2[len2 - 1 - i]
// Candidates are enumerated in the reference's order (forward offsets 0..len1-31, then reverse
// 0,-1,..,-(len2-31)); 64 candidates per step, one per lane:
//   phase A  each lane counts mismatches over the first min(16, L) columns of its diagonal; a
//            diagonal with >= 3 of them can never be accepted (both accept branches of
//            util.py:183 need fewer than 3 mismatches among the first 50 columns);
//   phase B  survivors are verified in order by the whole wave: tot = mismatches over all L
//            columns, c50 = those at i < 50; accept iff tot < 3 or (c50 < 3 and L >= 52), which is
//            the loop of util.py:177-183 in closed form: the loop breaks at
//            the 3rd mismatch only if it falls at i < 50, otherwise it runs to i = L-1 and the
//            test `i > 50` needs L >= 52.  diff reported = tot.
// All lanes return the same (offset, overlap_len, diff).
// ------------------------------------------------------------------------------------------------
__device__ inline void overlap_hm_wave(const uint8_t* r1, int len1, const uint8_t* c2, int len2, int& o_offset,
                                       int& o_len, int& o_diff) {
    const int lane = lane_id();
    const int nf = len1 > 30 ? len1 - 30 : 0;   // forward offsets: offset < len1 - 30
    const int nr = len2 > 30 ? len2 - 30 : 0;   // reverse offsets: offset > -(len2 - 30)
    const int ncand = nf + nr;
    const uint8_t* rr2_last = c2 + len2 - 1;    // reverse_r2[i] = rr2_last[-i]
    for (int base = 0; base < ncand; base += WAVE) {
        const int c = base + lane;
        const bool valid = c < ncand;
        int p1 = 0, p2 = 0, L = 0;
        if (valid) {
            if (c < nf) { p1 = c; p2 = 0; L = min(len1 - c, len2); }
            else { p1 = 0; p2 = c - nf; L = min(len1, len2 - p2); }
        }
        int cnt = 0;
        const int P = min(16, L);
        for (int i = 0; i < P; i++) cnt += (r1[p1 + i] != rr2_last[-(p2 + i)]) ? 1 : 0;
        unsigned long long surv = __ballot(valid && cnt < 3);
        while (surv) {
            const int l = __ffsll((long long)surv) - 1;
            surv &= surv - 1;
            const int q1 = __shfl(p1, l, WAVE), q2 = __shfl(p2, l, WAVE), QL = __shfl(L, l, WAVE);
            int tot = 0, c50 = 0;
            for (int i0 = 0; i0 < QL; i0 += WAVE) {
                const int i = i0 + lane;
                const bool mm = i < QL && r1[q1 + i] != rr2_last[-(q2 + i)];
                const unsigned long long b = __ballot(mm);
                tot += __popcll(b);
                if (i0 == 0) c50 = __popcll(b & ((1ull << 50) - 1));
            }
            if (tot < 3 || (c50 < 3 && QL >= 52)) {
                const int cand = base + l;
                o_offset = cand < nf ? cand : -(cand - nf);
                o_len = QL;
                o_diff = tot;
                return;
            }
        }
    }
    o_offset = 0; o_len = 0; o_diff = 0;
}

// hasPolyX (preprocesser.py:30-51) by one wave: the byte that fires first, or 0 for None.
// Position x fires iff seq[x] occurs >= maxPoly - mismatch times in seq[max(0,x-maxPoly+1) .. x];
// scanning stops (with None) at the first byte outside the 9 symbols.
__device__ inline int has_polyx_wave(const uint8_t* s, int len, int maxPoly, int mismatch) {
    if (len < maxPoly) return 0;
    const int lane = lane_id();
    const int need = maxPoly - mismatch;
    // first invalid position (scan range is [0, vend))
    int vend = len;
    for (int x0 = 0; x0 < len; x0 += WAVE) {
        const int x = x0 + lane;
        const unsigned long long bad = __ballot(x < len && !poly_symbol(s[x]));
        if (bad) { vend = x0 + __ffsll((long long)bad) - 1; break; }
    }
    for (int x0 = 0; x0 < vend; x0 += WAVE) {
        const int x = x0 + lane;
        bool fire = false;
        if (x < vend) {
            const uint8_t f = s[x];
            const int lo = x - maxPoly + 1 > 0 ? x - maxPoly + 1 : 0;
            int cnt = 0;
            for (int j = lo; j <= x; j++) cnt += (s[j] == f) ? 1 : 0;
            fire = cnt >= need;
        }
        const unsigned long long b = __ballot(fire);
        if (b) return s[x0 + __ffsll((long long)b) - 1];
    }
    return 0;
}

// lowQualityNum (preprocesser.py:61-68): count of ord(q) < qual + 33
__device__ inline int low_quality_wave(const uint8_t* q, int len, int qual) {
    const int lane = lane_id();
    const int thr = qual + 33;
    int n = 0;
    for (int i0 = 0; i0 < len; i0 += WAVE) {
        const int i = i0 + lane;
        n += __popcll(__ballot(i < len && (int)q[i] < thr));
    }
    return n;
}

// nNumber (preprocesser.py:70-76)
__device__ inline int n_number_wave(const uint8_t* s, int len) {
    const int lane = lane_id();
    int n = 0;
    for (int i0 = 0; i0 < len; i0 += WAVE) {
        const int i = i0 + lane;
        n += __popcll(__ballot(i < len && s[i] == 'N'));
    }
    return n;
}

// Levenshtein distance of two short strings by ONE LANE, Myers/Hyyro bit-vector form (the
// algorithm of editdistance/_editdistance.cpp:29-60 for a single 64-bit block): A(i) is the pattern
// (la <= 64 bits), B(j) the text, both given as accessors so that views (reverse complements, LDS
// or global pointers) need no copy.  Equals the DP of util.py:72-83.
template <typename FA, typename FB>
__device__ __forceinline__ int edit_distance_lane(FA A, int la, FB B, int lb) {
    if (la == 0) return lb;
    if (lb == 0) return la;
    unsigned long long Pv = la >= 64 ? ~0ull : ((1ull << la) - 1), Mv = 0;
    const unsigned long long top = 1ull << (la - 1);
    int score = la;
    for (int j = 0; j < lb; j++) {
        const uint8_t ch = B(j);
        unsigned long long Eq = 0;
        for (int i = 0; i < la; i++) Eq |= (unsigned long long)(A(i) == ch) << i;
        const unsigned long long Xv = Eq | Mv;
        const unsigned long long Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        unsigned long long Ph = Mv | ~(Xh | Pv);
        unsigned long long Mh = Pv & Xh;
        if (Ph & top) score++;
        else if (Mh & top) score--;
        Ph = (Ph << 1) | 1ull;
        Mh <<= 1;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
    }
    return score;
}

// detectBarcode (barcodeprocesser.py:19-32) by one wave
__device__ inline int detect_barcode_wave(const uint8_t* s, int len, int bl, const uint8_t* verify, int vl) {
    if (len <= vl + bl + 1) return 0;
    const int lane = lane_id();
    const bool in = lane < vl;
    const uint8_t v = in ? verify[lane] : 0;
    const int dc = __popcll(__ballot(in && s[bl + lane] != v));
    if (dc <= 1) return bl;
    const int dl = __popcll(__ballot(in && s[bl - 1 + lane] != v));
    if (dl == 0) return bl - 1;
    const int dr = __popcll(__ballot(in && s[bl + 1 + lane] != v));
    if (dr == 0) return bl + 1;
    return 0;
}

// cleanBarcodeTail (barcodeprocesser.py:47-75): lane i evaluates iteration i of the loop
// (compLen = min(n1,n2) - i) with two Levenshtein distances; the first i that satisfies both
// thresholds wins.  rs1/rs2 = readStart strings (barcode + verify), r1/r2 = the moved reads.
__device__ inline int clean_barcode_tail_wave(const uint8_t* r1, int r1len, const uint8_t* r2, int r2len,
                                              const uint8_t* rs1, int n1, const uint8_t* rs2, int n2) {
    const int lane = lane_id();
    const int bsl = min(n1, n2);
    bool ok = false;
    int compLen = 0;
    if (lane < bsl) {
        compLen = bsl - lane;
        if (!(compLen >= r1len || compLen >= r2len)) {
            // reverse2[i:] = revcomp(readStart2)[i:], n2 - i chars; reverse1 likewise
            const int m2 = n2 - lane, m1 = n1 - lane;
            const uint8_t* t1p = r1 + r1len - compLen;
            const uint8_t* t2p = r2 + r2len - compLen;
            const int d1 = edit_distance_lane([&](int i) { return t1p[i]; }, compLen,
                                              [&](int k) { return comp_or_n(rs2[n2 - 1 - (lane + k)]); }, m2);
            const int d2 = edit_distance_lane([&](int i) { return t2p[i]; }, compLen,
                                              [&](int k) { return comp_or_n(rs1[n1 - 1 - (lane + k)]); }, m1);
            ok = (d1 * 5 <= compLen) && (d2 * 5 <= compLen);   // distance <= compLen/5
        }
    }
    const unsigned long long b = __ballot(ok);
    if (!b) return 0;
    return bsl - (__ffsll((long long)b) - 1);
}

// isInBubble's geometric half (preprocesser.py:193-204), IEEE double, no contraction
__device__ inline bool in_bubble_wave(int lane_no, int tile, int x, int y, const DevCircles& c) {
    const int lane = lane_id();
    bool hit = false;
    for (int i = lane; i < c.n; i += WAVE) {
        if (c.tile[i] == tile && c.lane[i] == lane_no) {
            const double dx = __dsub_rn(c.cx[i], (double)x), dy = __dsub_rn(c.cy[i], (double)y);
            const double lhs = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
            if (lhs < __dmul_rn(c.cr[i], c.cr[i])) hit = true;
        }
    }
    return __ballot(hit) != 0;
}

// stage `len` bytes from global memory into LDS (coalesced byte loads: lane i -> byte i)
__device__ __forceinline__ void stage(uint8_t* dst, const uint8_t* src, int len) {
    for (int i = lane_id(); i < len; i += WAVE) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------
// One record through preprocesser.py:436-631, executed by ONE wavefront on byte strings staged in
// LDS ("generation 1", fully general: any alphabet, any length <= AQC_MAX_READ_LEN, barcodes,
// bubbles).  Used by the generic kernel for every record and by the fast kernel (aqc_fast.hpp) for
// the records it defers.
// ------------------------------------------------------------------------------------------------
struct WaveLds {
    uint8_t *s1, *q1, *s2, *q2, *c2;   // 5 x LSTR bytes
    uint8_t *rs1, *rs2;                // 2 x 64 bytes (barcode readStart strings)
};

// CUT: the trim stage also applies the per-read views of the passes in front (aqc_viewpass.hpp: the quality cut, the adapter pass; the mates of a record side by side)
template <bool CUT = false, class Cfg>      // aqc_config, or aqc_config in the kernarg segment (address space 4: its fields are scalar loads where they are used)
__device__ __forceinline__ void process_record_wave(const DevBatch& b, uint64_t rec, const Cfg& cfg, const DevCircles& circ,
                                           const WaveLds& w, aqc_result* __restrict__ results, BlockAcc& acc,
                                           const DevStats& st, bool accum, const uint32_t* cut = nullptr) {
    const int lane = lane_id();
    uint8_t* s1 = w.s1;
    uint8_t* q1 = w.q1;
    uint8_t* s2 = w.s2;
    uint8_t* q2 = w.q2;
    uint8_t* c2 = w.c2;   // complement-or-N of s2, same orientation
    const bool paired = cfg.paired != 0;
    {
        const uint32_t l1w = b.len1[rec], l2w = paired ? b.len2[rec] : 0u;
        const int L1 = (int)(l1w & LEN_MASK);
        const int L2 = (int)(l2w & LEN_MASK);
        // a quality line that is not as long as its sequence line (either mate): every string keeps its own view
        const bool irr = b.qlen1 != nullptr && ((l1w | l2w) & LEN_IRR) != 0u;
        const int QL1 = irr ? (int)(b.qlen1[rec] & QLEN_MASK) : L1;
        const int QL2 = (irr && paired) ? (int)(b.qlen2[rec] & QLEN_MASK) : L2;
        if (L1 > AQC_MAX_READ_LEN || L2 > AQC_MAX_READ_LEN || QL1 > AQC_MAX_READ_LEN || QL2 > AQC_MAX_READ_LEN) {
            if (lane == 0) atomicCAS(st.status, 0, AQC_ERR_READ_TOO_LONG);
            return;
        }
        stage(s1, b.seq1 + b.off1[rec], L1);
        stage(q1, b.qual1 + (b.qoff1 ? b.qoff1[rec] : b.off1[rec]), QL1);
        if (paired) {
            stage(s2, b.seq2 + b.off2[rec], L2);
            stage(q2, b.qual2 + (b.qoff2 ? b.qoff2[rec] : b.off2[rec]), QL2);
            for (int i = lane; i < L2; i += WAVE) c2[i] = comp_or_n(b.seq2[b.off2[rec] + i]);
        }
        // (wave-private LDS region: no barrier needed, the compiler orders LDS ops of one wave)
        __builtin_amdgcn_wave_barrier();

        int a1 = 0, len1 = L1, a2 = 0, len2 = L2;     // current views: s1[a1 .. a1+len1), s2[a2 .. a2+len2)
        // ... and of the quality strings: q1[qa1 .. qa1+ql1), q2[qa2 .. qa2+ql2).  Every slice upstream is a python slice of
        // EACH string (preprocesser.py:19-28,521-524, barcodeprocesser.py:42-43,66-69): the same cut applied to a string of
        // another length.  For a regular record they stay equal to the sequence views.
        int qa1 = 0, ql1 = QL1, qa2 = 0, ql2 = QL2;
        auto cut_front = [](int& a, int& l, int k) { const int m = min(k, l); a += m; l -= m; };      // s[k:]
        auto cut_tail = [](int& l, int k) { if (k > 0) l = max(l - k, 0); };                          // s[:-k]  (k > 0)
        int flag = -1;
        int offset = 0, ovl = 0, dist = 0, n_edits = 0;
        uint8_t bcode = 0;
        // counters this record contributes (wave-uniform values, committed by lane 0)
        int c_adapter_base = 0, c_adapter_read = 0, c_overlapped = 0, c_corrected = 0, c_masked = 0, c_skipped = 0;
        int c_read_corrected = 0, ovl0 = -1, dist_final = -1;
        int em[3] = {-1, -1, -1};
        // (written through constant indices only, so that both arrays stay in registers: indexed by n_edits / handled they lived in
        //  20 bytes of scratch — round 5 review)
        unsigned long long ed0 = 0, ed1 = 0, ed2 = 0;      // o | kind << 16 | base << 24 | qual << 32
        auto put_edit = [&](int k, const aqc_edit& e) {
            const unsigned long long x = (unsigned long long)e.o | ((unsigned long long)e.kind << 16) | ((unsigned long long)e.base << 24) | ((unsigned long long)e.qual << 32);
            ed0 = k == 0 ? x : ed0; ed1 = k == 1 ? x : ed1; ed2 = k >= 2 ? x : ed2;
        };
        auto get_edit = [](unsigned long long x) { return aqc_edit{(uint16_t)(x & 0xffffu), (uint8_t)(x >> 16), (uint8_t)(x >> 24), (uint8_t)(x >> 32)}; };
        auto put_em = [&](int k, int val) { em[0] = k == 0 ? val : em[0]; em[1] = k == 1 ? val : em[1]; em[2] = k >= 2 ? val : em[2]; };

        // ---- barcode (preprocesser.py:436-452)
        if (cfg.barcode) {
            const int bl = cfg.barcode_length, vl = cfg.barcode_verify_len;
            const int b1 = detect_barcode_wave(s1, len1, bl, cfg.barcode_verify, vl);
            if (b1 == 0) flag = AQC_BADBCD1;
            else {
                bcode = (uint8_t)(b1 - bl + 2);
                if (!paired) {
                    const int rm = vl + bl;   // single-end moves the design length (preprocesser.py:444)
                    a1 += min(rm, len1); len1 = max(len1 - rm, 0);
                    cut_front(qa1, ql1, rm);
                } else {
                    const int b2 = detect_barcode_wave(s2, len2, bl, cfg.barcode_verify, vl);
                    if (b2 == 0) flag = AQC_BADBCD2;
                    else {
                        bcode |= (uint8_t)((b2 - bl + 2) << 4);
                        // readStart = seq[0:barcodeLen] + verify (barcodeprocesser.py:78-79)
                        uint8_t* rs1 = w.rs1;
                        uint8_t* rs2 = w.rs2;
                        if (lane < b1) rs1[lane] = s1[lane];
                        if (lane < vl) rs1[b1 + lane] = cfg.barcode_verify[lane];
                        if (lane < b2) rs2[lane] = s2[lane];
                        if (lane < vl) rs2[b2 + lane] = cfg.barcode_verify[lane];
                        __builtin_amdgcn_wave_barrier();
                        a1 += vl + b1; len1 -= vl + b1;
                        a2 += vl + b2; len2 -= vl + b2;
                        cut_front(qa1, ql1, vl + b1); cut_front(qa2, ql2, vl + b2);
                        const int cut = clean_barcode_tail_wave(s1 + a1, len1, s2 + a2, len2, rs1, b1 + vl, rs2, b2 + vl);
                        len1 -= cut; len2 -= cut;
                        cut_tail(ql1, cut); cut_tail(ql2, cut);
                    }
                }
            }
        }
        // ---- trim (preprocesser.py:455-466, python slice semantics of trim() :19-28)
        if (CUT) {
            // ... and the quality cut: every string is sliced by its own length, trim() first, then [c0:c1] of the cut pass
            if (flag < 0) {
                const uint32_t v1 = cut[paired ? 2 * rec : rec];
                view_apply(a1, len1, cfg.trim_front, cfg.trim_tail, v1);
                view_apply(qa1, ql1, cfg.trim_front, cfg.trim_tail, v1);
                if (len1 < 5) flag = AQC_BADTRIM1;
                else if (paired) {
                    const uint32_t v2 = cut[2 * rec + 1];
                    view_apply(a2, len2, cfg.trim_front2, cfg.trim_tail2, v2);
                    view_apply(qa2, ql2, cfg.trim_front2, cfg.trim_tail2, v2);
                    if (len2 < 5) flag = AQC_BADTRIM2;
                }
            }
        } else if (flag < 0 && (cfg.trim_front > 0 || cfg.trim_tail > 0)) {
            int end = cfg.trim_tail > 0 ? max(len1 - cfg.trim_tail, 0) : len1;
            int stt = min(cfg.trim_front, len1);
            int nl = max(end - stt, 0);
            a1 += stt; len1 = nl;
            {
                const int qend = cfg.trim_tail > 0 ? max(ql1 - cfg.trim_tail, 0) : ql1, qst = min(cfg.trim_front, ql1);
                qa1 += qst; ql1 = max(qend - qst, 0);
            }
            if (len1 < 5) flag = AQC_BADTRIM1;
            else if (paired) {
                end = cfg.trim_tail2 > 0 ? max(len2 - cfg.trim_tail2, 0) : len2;
                stt = min(cfg.trim_front2, len2);
                nl = max(end - stt, 0);
                a2 += stt; len2 = nl;
                const int qend = cfg.trim_tail2 > 0 ? max(ql2 - cfg.trim_tail2, 0) : ql2, qst = min(cfg.trim_front2, ql2);
                qa2 += qst; ql2 = max(qend - qst, 0);
                if (len2 < 5) flag = AQC_BADTRIM2;
            }
        }
        // ---- bubble (preprocesser.py:469-473)
        if (flag < 0 && cfg.debubble && b.aux_ok && b.aux_ok[rec]) {
            if (b.aux_ok[rec] == 2) { if (lane == 0) raise_at_record(st, rec, AQC_ERR_ARG); }     // int() raises upstream (preprocesser.py:187-192)
            else if (in_bubble_wave(b.aux_lane[rec], b.aux_tile[rec], b.aux_x[rec], b.aux_y[rec], circ)) flag = AQC_BADBBL;
        }
        // ---- length (preprocesser.py:476-479)
        if (flag < 0 && len1 < cfg.seq_len_req) flag = AQC_BADLEN;
        // ---- polyX (preprocesser.py:482-490)
        if (flag < 0 && cfg.poly_size_limit > 0) {
            int p = has_polyx_wave(s1 + a1, len1, cfg.poly_size_limit, cfg.allow_mismatch_in_poly);
            if (p == 0 && paired) p = has_polyx_wave(s2 + a2, len2, cfg.poly_size_limit, cfg.allow_mismatch_in_poly);
            if (p != 0) flag = AQC_BADPOL;
        }
        // ---- low quality: only read 1 is tested (preprocesser.py:498, upstream quirk)
        if (flag < 0 && cfg.unqualified_base_limit > 0) {
            if (low_quality_wave(q1 + qa1, ql1, cfg.qualified_quality_phred) > cfg.unqualified_base_limit) flag = AQC_BADLQC;      // (the QUALITY line is what is counted, :61-68)
        }
        // ---- N (preprocesser.py:504-512)
        if (flag < 0 && cfg.n_base_limit > 0) {
            const int n1 = n_number_wave(s1 + a1, len1);
            const int n2 = paired ? n_number_wave(s2 + a2, len2) : 0;
            if (n1 > cfg.n_base_limit || n2 > cfg.n_base_limit) flag = AQC_BADNCT;
        }
        // ---- overlap + correction (preprocesser.py:515-617)
        if (flag < 0 && paired && !cfg.no_overlap) {
            overlap_hm_wave(s1 + a1, len1, c2 + a2, len2, offset, ovl, dist);
            ovl0 = ovl;
            if (offset < 0 && ovl > 30) {
                len1 = ovl; len2 = ovl;                      // all four strings := [0:overlap_len]
                ql1 = min(ql1, ovl); ql2 = min(ql2, ovl);
                c_adapter_base = 2 * (-offset); c_adapter_read = 1;
                if (len1 < cfg.seq_len_req) { flag = AQC_BADLEN; offset = 0; ovl = 0; dist = 0; }   // record carries no overlap
                else overlap_hm_wave(s1 + a1, len1, c2 + a2, len2, offset, ovl, dist);
            }
            if (flag < 0) {
                dist_final = dist;
                if (dist > 3) flag = AQC_BADDIFF;
                else if (ovl > 30) {
                    c_overlapped = 1;
                    if (dist > 0 && irr) {
                        // The walk of preprocesser.py:563-598 for a record whose quality views differ from its sequence views,
                        // as upstream runs it: one position after the other, every string indexed from ITS OWN end
                        // (r1[3][len(r1[3]) - overlap_len + o] with python's wrap for a negative index, r2[3][-o-1]), the
                        // quality strings edited in place — a wrapped index can meet a position a later step reads again.
                        // An index outside a string is upstream's IndexError: the run ends at this record.  One lane; such
                        // records are rare.
                        int handled = 0, err = 0;
                        if (lane == 0) {
                            const uint8_t* S1 = s1 + a1;
                            const uint8_t* S2 = s2 + a2;
                            uint8_t* Q1 = q1 + qa1;
                            uint8_t* Q2 = q2 + qa2;
                            for (int o = 0; o < ovl && handled < dist; ++o) {
                                const uint8_t bA = S1[len1 - ovl + o];
                                const uint8_t r2o = S2[len2 - 1 - o];
                                const uint8_t bB = comp_strict(r2o);
                                if (bB == 0) { err = AQC_ERR_ALPHABET; break; }            // util.complement (:565)
                                int i1 = ql1 - ovl + o;
                                if (i1 < 0) i1 += ql1;                                      // python: a negative index counts from the end
                                const int i2 = ql2 - 1 - o;
                                if (i1 < 0 || i2 < 0) { err = AQC_ERR_INDEX; break; }      // IndexError (:566-567)
                                const int qa = Q1[i1], qb = Q2[i2];
                                if (bA == bB) continue;
                                bool fixed = false;
                                if (qa - 33 >= 30 && qb - 33 <= 14) {
                                    const uint8_t cA = comp_strict(bA);
                                    if (bA != 'N' && bB != 'N') {
                                        const int i0 = base_idx(cA), ix = base_idx(r2o);
                                        if (cA == 0 || i0 < 0 || ix < 0) { err = AQC_ERR_ALPHABET; break; }
                                        put_em(handled, i0 * 4 + ix);
                                    }
                                    if (!cfg.no_correction) {
                                        if (cA == 0) { err = AQC_ERR_ALPHABET; break; }
                                        put_edit(n_edits, aqc_edit{(uint16_t)o, AQC_EDIT_FIX_R2, cA, (uint8_t)qa});
                                        Q2[i2] = (uint8_t)qa;
                                        n_edits++; c_corrected++; fixed = true;
                                    }
                                } else if (qb - 33 >= 30 && qa - 33 <= 14) {
                                    if (bA != 'N' && bB != 'N') {
                                        const int i0 = base_idx(bB), ix = base_idx(bA);
                                        if (i0 < 0 || ix < 0) { err = AQC_ERR_ALPHABET; break; }
                                        put_em(handled, i0 * 4 + ix);
                                    }
                                    if (!cfg.no_correction) {
                                        put_edit(n_edits, aqc_edit{(uint16_t)o, AQC_EDIT_FIX_R1, bB, (uint8_t)qb});
                                        Q1[i1] = (uint8_t)qb;
                                        n_edits++; c_corrected++; fixed = true;
                                    }
                                }
                                if (!fixed) {
                                    if (cfg.mask_mismatch) {
                                        put_edit(n_edits, aqc_edit{(uint16_t)o, AQC_EDIT_MASK, 0, (uint8_t)'!'});
                                        Q2[i2] = (uint8_t)'!'; Q1[i1] = (uint8_t)'!';
                                        n_edits++; c_masked++;
                                    } else c_skipped++;
                                }
                                handled++;
                            }
                            if (err) raise_at_record(st, rec, err);
                        }
                        // (lane 0 writes the result record and the counters; the other lanes only need the verdict)
                        handled = __shfl(handled, 0, WAVE);
                        if (handled == dist) {
                            if (c_corrected > 0) c_read_corrected = 1;
                        } else {
                            flag = AQC_BADMISMATCH;
                            em[0] = em[1] = em[2] = -1;
                            c_corrected = c_masked = c_skipped = 0;
                        }
                    } else if (dist > 0) {
                        // the tail-anchored walk of preprocesser.py:563-598
                        int handled = 0;
                        bool bad_alpha = false;
                        const uint8_t* w1 = s1 + a1 + len1 - ovl;       // b1 = w1[o]
                        const uint8_t* x1 = q1 + a1 + len1 - ovl;       // q1 = x1[o]
                        const uint8_t* w2 = s2 + a2 + len2 - 1;         // r2[-o-1] = w2[-o]
                        const uint8_t* x2 = q2 + a2 + len2 - 1;
                        for (int o0 = 0; o0 < ovl && handled < dist; o0 += WAVE) {
                            const int o = o0 + lane;
                            const bool in = o < ovl;
                            const uint8_t r2b = in ? w2[-o] : (uint8_t)'A';
                            const uint8_t bb2 = comp_strict(r2b);
                            const unsigned long long inval = __ballot(in && bb2 == 0);
                            unsigned long long mm = __ballot(in && w1[o] != bb2);
                            int last = WAVE - 1;
                            while (mm && handled < dist) {
                                const int l = __ffsll((long long)mm) - 1;
                                mm &= mm - 1;
                                last = l;
                                const int oo = o0 + l;
                                const uint8_t bA = w1[oo];
                                const uint8_t r2o = w2[-oo];
                                const uint8_t bB = comp_strict(r2o);
                                const int qa = x1[oo], qb = x2[-oo];
                                bool fixed = false;
                                if (qa - 33 >= 30 && qb - 33 <= 14) {
                                    if (bA != 'N' && bB != 'N') {
                                        const uint8_t cA = comp_strict(bA);
                                        const int i0 = base_idx(cA), i1 = base_idx(r2o);
                                        if (cA == 0 || i0 < 0 || i1 < 0) bad_alpha = true;
                                        else put_em(handled, i0 * 4 + i1);          // err[comp(b1)][comp(b2)]
                                    }
                                    if (!cfg.no_correction) {
                                        const uint8_t cA = comp_strict(bA);
                                        if (cA == 0) bad_alpha = true;
                                        put_edit(n_edits, aqc_edit{(uint16_t)oo, AQC_EDIT_FIX_R2, cA, (uint8_t)qa});
                                        n_edits++; c_corrected++; fixed = true;
                                    }
                                } else if (qb - 33 >= 30 && qa - 33 <= 14) {
                                    if (bA != 'N' && bB != 'N') {
                                        const int i0 = base_idx(bB), i1 = base_idx(bA);
                                        if (i0 < 0 || i1 < 0) bad_alpha = true;
                                        else put_em(handled, i0 * 4 + i1);          // err[b2][b1]
                                    }
                                    if (!cfg.no_correction) {
                                        put_edit(n_edits, aqc_edit{(uint16_t)oo, AQC_EDIT_FIX_R1, bB, (uint8_t)qb});
                                        n_edits++; c_corrected++; fixed = true;
                                    }
                                }
                                if (!fixed) {
                                    if (cfg.mask_mismatch) {
                                        put_edit(n_edits, aqc_edit{(uint16_t)oo, AQC_EDIT_MASK, 0, (uint8_t)'!'});
                                        n_edits++; c_masked++;
                                    } else c_skipped++;
                                }
                                handled++;
                            }
                            // util.complement raises on every visited r2 byte outside COMP (preprocesser.py:565)
                            const unsigned long long visited = (handled >= dist) ? ((last == 63) ? ~0ull : ((2ull << last) - 1)) : ~0ull;
                            if (inval & visited) bad_alpha = true;
                        }
                        if (bad_alpha && lane == 0) raise_at_record(st, rec, AQC_ERR_ALPHABET);
                        if (handled == dist) {
                            if (c_corrected > 0) c_read_corrected = 1;
                        } else {
                            flag = AQC_BADMISMATCH;
                            em[0] = em[1] = em[2] = -1;
                            c_corrected = c_masked = c_skipped = 0;   // edits stay (written to bad/), counters do not
                        }
                    }
                }
            }
        }
        if (flag < 0) flag = AQC_GOOD;

        // ---- result record + counters (lane 0)
        if (lane == 0) {
            aqc_result r;
            r.flag = (uint8_t)flag; r.n_edits = (uint8_t)n_edits;
            r.start1 = (uint16_t)a1; r.len1 = (uint16_t)len1;
            r.start2 = (uint16_t)a2; r.len2 = (uint16_t)len2;
            r.offset = (int16_t)offset; r.overlap_len = (uint16_t)ovl; r.distance = (uint16_t)dist;
            r.edits[0] = get_edit(ed0); r.edits[1] = get_edit(ed1); r.edits[2] = get_edit(ed2);
            r.barcode = bcode;
            results[rec] = r;
            if (irr) {
                b.qview1[rec] = (uint32_t)qa1 | ((uint32_t)ql1 << 16);
                if (paired) b.qview2[rec] = (uint32_t)qa2 | ((uint32_t)ql2 << 16);
            }
            if (accum) {
                unsigned long long* C = acc.counters;
                atomicAdd(&C[AQC_C_TOTAL_READS], 1ull);
                atomicAdd(&C[AQC_C_TOTAL_BASES], (unsigned long long)(L1 + ((paired && cfg.count_r2_bases) ? L2 : 0)));
                atomicAdd(&C[AQC_C_FLAG0 + flag], 1ull);
                if (flag == AQC_GOOD) {
                    atomicAdd(&C[AQC_C_GOOD_READS], 1ull);
                    atomicAdd(&C[AQC_C_GOOD_BASES], (unsigned long long)(len1 + ((paired && cfg.count_r2_bases) ? len2 : 0)));
                }
                if (ovl0 >= 0) atomicAdd(&acc.ovl_hist[ovl0], 1u);
                if (dist_final >= 0) atomicAdd(&acc.dist_hist[min(dist_final, AQC_QC_COLS - 1)], 1u);
                if (c_adapter_read) {
                    atomicAdd(&C[AQC_C_TRIMMED_ADAPTER_BASE], (unsigned long long)c_adapter_base);
                    atomicAdd(&C[AQC_C_TRIMMED_ADAPTER_READ], 1ull);
                }
                if (c_overlapped) {
                    atomicAdd(&C[AQC_C_OVERLAPPED], 1ull);
                    atomicAdd(&C[AQC_C_OVERLAP_LEN_SUM], (unsigned long long)ovl);
                    atomicAdd(&C[AQC_C_OVERLAP_BASE_SUM], (unsigned long long)(2 * ovl));
                    atomicAdd(&C[AQC_C_OVERLAP_BASE_ERR], (unsigned long long)dist);
                    if (c_read_corrected) atomicAdd(&C[AQC_C_READ_CORRECTED], 1ull);
                    if (c_corrected) atomicAdd(&C[AQC_C_BASE_CORRECTED], (unsigned long long)c_corrected);
                    if (c_masked) atomicAdd(&C[AQC_C_BASE_ZERO_QUAL_MASKED], (unsigned long long)(2 * c_masked));
                    if (c_skipped) atomicAdd(&C[AQC_C_BASE_SKIPPED_CORRECTION], (unsigned long long)(2 * c_skipped));
                    for (int k = 0; k < 3; k++)
                        if (em[k] >= 0) atomicAdd(&C[AQC_C_ERR_MATRIX0 + em[k]], 1ull);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        }
}

// ------------------------------------------------------------------------------------------------
// Generic kernel: grid-stride over records, one wave per record, block-private counters flushed once.
// ------------------------------------------------------------------------------------------------
// the leading arguments of the two kernels below as they stand in the kernarg segment (each at its natural alignment)
struct FilterArgs {
    DevBatch b;
    aqc_config cfg;
    DevCircles circ;
    aqc_result* results;
    DevStats st;
    uint64_t accum_limit;
};

__global__ __launch_bounds__(BLOCK) void filter_overlap_kernel(DevBatch b, aqc_config cfg, DevCircles circ,
                                                               aqc_result* __restrict__ results, DevStats st,
                                                               uint64_t accum_limit) {
    __shared__ uint8_t lds[WPB][5][LSTR];
    __shared__ uint8_t rsbuf[WPB][2][64];
    __shared__ BlockAcc acc;
    const int wave = threadIdx.x / WAVE;
    for (int i = threadIdx.x; i < (int)(sizeof(BlockAcc) / 4); i += BLOCK) ((unsigned int*)&acc)[i] = 0;
    __syncthreads();
    const WaveLds w{lds[wave][0], lds[wave][1], lds[wave][2], lds[wave][3], lds[wave][4], rsbuf[wave][0], rsbuf[wave][1]};
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t n_rec = b.n;
    for (uint64_t rec = (uint64_t)blockIdx.x * WPB + wave; rec < n_rec; rec += nwaves) {
        // (the arguments — forty pointers and the configuration — are read from the kernarg segment where a record is worked on, not
        //  held in scalar registers across the loop: qc_stat_kernel's trick, round 5)
#if defined(__HIP_DEVICE_COMPILE__)
        const FilterArgs __attribute__((address_space(4)))* ka = (const FilterArgs __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const DevBatch bb = ka->b;
        const DevCircles ci = ka->circ;
        const DevStats ss = ka->st;
        // (the configuration is read in place: barcode_verify is indexed at run time, a copy would live in scratch)
        process_record_wave(bb, rec, ka->cfg, ci, w, ka->results, acc, ss, rec < ka->accum_limit);
#else
        process_record_wave(b, rec, cfg, circ, w, results, acc, st, rec < accum_limit);
#endif
    }
    __syncthreads();
    flush_block_acc(acc, st);
}

// The same pipeline over an explicit list of record indices (the pairs the lane-per-read kernel deferred);
// the list length lives in device memory, so the launch needs no host round trip.
__global__ __launch_bounds__(BLOCK) void filter_overlap_list_kernel(DevBatch b, aqc_config cfg, DevCircles circ,
                                                                    aqc_result* __restrict__ results, DevStats st,
                                                                    uint64_t accum_limit, const uint32_t* __restrict__ list,
                                                                    const unsigned int* __restrict__ n_list) {
    __shared__ uint8_t lds[WPB][5][LSTR];
    __shared__ uint8_t rsbuf[WPB][2][64];
    __shared__ BlockAcc acc;
    const unsigned int n = *n_list;
    if (n == 0) return;
    const int wave = threadIdx.x / WAVE;
    for (int i = threadIdx.x; i < (int)(sizeof(BlockAcc) / 4); i += BLOCK) ((unsigned int*)&acc)[i] = 0;
    __syncthreads();
    const WaveLds w{lds[wave][0], lds[wave][1], lds[wave][2], lds[wave][3], lds[wave][4], rsbuf[wave][0], rsbuf[wave][1]};
    const unsigned int nwaves = gridDim.x * WPB;
    for (unsigned int i = blockIdx.x * WPB + wave; i < n; i += nwaves) {
        const uint64_t rec = list[i];
#if defined(__HIP_DEVICE_COMPILE__)
        const FilterArgs __attribute__((address_space(4)))* ka = (const FilterArgs __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const DevBatch bb = ka->b;
        const DevCircles ci = ka->circ;
        const DevStats ss = ka->st;
        // (the configuration is read in place: barcode_verify is indexed at run time, a copy would live in scratch)
        process_record_wave(bb, rec, ka->cfg, ci, w, ka->results, acc, ss, rec < ka->accum_limit);
#else
        process_record_wave(b, rec, cfg, circ, w, results, acc, st, rec < accum_limit);
#endif
    }
    __syncthreads();
    flush_block_acc(acc, st);
}

// The two kernels above with the quality cut on (aqc_qcut.hpp): the same pipeline, the trim stage takes each mate's view from the
// slot's arrays.  LIST: over the records the lane-per-read kernel deferred.  Kernels of their own, so that the ones above take the
// arguments — and come out of the compiler — as they always did.
struct FilterCutArgs {
    FilterArgs a;
    const uint32_t* list;
    const unsigned int* n_list;
    const uint32_t* cut;
};

template <bool LIST>
__global__ __launch_bounds__(BLOCK) void filter_overlap_cut_kernel(FilterCutArgs A) {
    __shared__ uint8_t lds[WPB][5][LSTR];
    __shared__ uint8_t rsbuf[WPB][2][64];
    __shared__ BlockAcc acc;
    const uint64_t n = LIST ? (uint64_t)*A.n_list : A.a.b.n;
    if (n == 0) return;
    const int wave = threadIdx.x / WAVE;
    for (int i = threadIdx.x; i < (int)(sizeof(BlockAcc) / 4); i += BLOCK) ((unsigned int*)&acc)[i] = 0;
    __syncthreads();
    const WaveLds w{lds[wave][0], lds[wave][1], lds[wave][2], lds[wave][3], lds[wave][4], rsbuf[wave][0], rsbuf[wave][1]};
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB;
    for (uint64_t i = (uint64_t)blockIdx.x * WPB + wave; i < n; i += nwaves) {
#if defined(__HIP_DEVICE_COMPILE__)
        const FilterCutArgs __attribute__((address_space(4)))* ka = (const FilterCutArgs __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const uint64_t rec = LIST ? (uint64_t)ka->list[i] : i;
        const DevBatch bb = ka->a.b;
        const DevCircles ci = ka->a.circ;
        const DevStats ss = ka->a.st;
        process_record_wave<true>(bb, rec, ka->a.cfg, ci, w, ka->a.results, acc, ss, rec < ka->a.accum_limit, ka->cut);
#else
        const uint64_t rec = LIST ? (uint64_t)A.list[i] : i;
        process_record_wave<true>(A.a.b, rec, A.a.cfg, A.a.circ, w, A.a.results, acc, A.a.st, rec < A.a.accum_limit, A.cut);
#endif
    }
    __syncthreads();
    flush_block_acc(acc, A.a.st);
}

}  // namespace aqc
