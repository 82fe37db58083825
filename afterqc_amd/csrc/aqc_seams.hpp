// aqc_seams.hpp — function seams: the wave-per-record device functions behind kernels that give one result per input record, and the
// libed.so-compatible single-call kernels.  Test and compatibility entry points, not hot paths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"
#include "aqc_prim.hpp"
#include "aqc_batch.hpp"
#include "aqc_record.hpp"

namespace aqc {

// ------------------------------------------------------------------------------------------------
// function seams: the same device functions, one result per input record
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void overlap_seam_kernel(DevBatch b, int32_t* off, int32_t* ol, int32_t* df) {
    __shared__ uint8_t lds[WPB][2][LSTR];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const uint64_t rec = (uint64_t)blockIdx.x * WPB + wave;
    if (rec >= b.n) return;
    const int L1 = (int)(b.len1[rec] & LEN_MASK), L2 = (int)(b.len2[rec] & LEN_MASK);
    stage(lds[wave][0], b.seq1 + b.off1[rec], L1);
    for (int i = lane; i < L2; i += WAVE) lds[wave][1][i] = comp_or_n(b.seq2[b.off2[rec] + i]);
    __builtin_amdgcn_wave_barrier();
    int o, l, d;
    overlap_hm_wave(lds[wave][0], L1, lds[wave][1], L2, o, l, d);
    if (lane == 0) { off[rec] = o; ol[rec] = l; df[rec] = d; }
}

__global__ __launch_bounds__(BLOCK) void read_stats_seam_kernel(DevBatch b, int max_poly, int mismatch, int qual,
                                                                uint8_t* polyx, int32_t* lowq, int32_t* ncount) {
    __shared__ uint8_t lds[WPB][2][LSTR];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const uint64_t rec = (uint64_t)blockIdx.x * WPB + wave;
    if (rec >= b.n) return;
    const int L1 = (int)(b.len1[rec] & LEN_MASK);
    stage(lds[wave][0], b.seq1 + b.off1[rec], L1);
    stage(lds[wave][1], b.qual1 + (b.qoff1 ? b.qoff1[rec] : b.off1[rec]), L1);
    __builtin_amdgcn_wave_barrier();
    const int p = has_polyx_wave(lds[wave][0], L1, max_poly, mismatch);
    const int lq = low_quality_wave(lds[wave][1], L1, qual);
    const int nn = n_number_wave(lds[wave][0], L1);
    if (lane == 0) { polyx[rec] = (uint8_t)p; lowq[rec] = lq; ncount[rec] = nn; }
}

__global__ void edit_distance_seam_kernel(DevBatch b, int32_t* dist, int* status) {
    const uint64_t rec = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rec >= b.n) return;
    const int la = (int)(b.len1[rec] & LEN_MASK), lb = (int)(b.len2[rec] & LEN_MASK);
    const uint8_t* a = b.seq1 + b.off1[rec];
    const uint8_t* c = b.seq2 + b.off2[rec];
    // the bit-vector form needs the pattern in one 64-bit word; Levenshtein is symmetric
    auto fa = [&](int i) { return a[i]; };
    auto fc = [&](int i) { return c[i]; };
    if (la <= 64) dist[rec] = edit_distance_lane(fa, la, fc, lb);
    else if (lb <= 64) dist[rec] = edit_distance_lane(fc, lb, fa, la);
    else { dist[rec] = -1; atomicCAS(status, 0, AQC_ERR_UNSUPPORTED); }
}

// ---- libed.so-compatible seams (editdistance/_editdistance.h:16,23): one call = one tiny launch ----------------
// Levenshtein distance of two strings of any length: one workgroup, the DP row of util.py:72-83 in global scratch
// (`row`, lb + 1 ints), anti-dependencies resolved by walking the row in order on lane 0 — a compatibility seam, not a
// hot path (the hot path's Levenshtein is edit_distance_lane above).
__global__ void edit_distance_any_kernel(const uint8_t* a, int la, const uint8_t* b, int lb, int* row, int* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (la <= 64 || lb <= 64) {
        auto fa = [&](int i) { return a[i]; };
        auto fb = [&](int i) { return b[i]; };
        *out = la <= 64 ? edit_distance_lane(fa, la, fb, lb) : edit_distance_lane(fb, lb, fa, la);
        return;
    }
    for (int j = 0; j <= lb; ++j) row[j] = j;
    for (int i = 1; i <= la; ++i) {
        int diag = row[0];
        row[0] = i;
        const uint8_t ca = a[i - 1];
        for (int j = 1; j <= lb; ++j) {
            const int up = row[j];
            const int v = min(min(up + 1, row[j - 1] + 1), diag + (ca != b[j - 1] ? 1 : 0));
            diag = up;
            row[j] = v;
        }
    }
    *out = row[lb];
}

// seek_overlap(r1, len1, reverse_r2, len2, limit_distance, complete_compare_require, overlap_require) with the semantics of
// the LIVE scan util.overlap_hm (util.py:158-212), parameters made explicit: per offset the loop counts mismatches and
// breaks at the limit-th one if it falls at a column < complete_compare_require; the offset is accepted iff diff < limit,
// or the loop ran to the end (no break) and its last column L-1 is > complete_compare_require.  In closed form:
// tot < limit, or (mismatches among the first `ccr` columns < limit and L - 1 > ccr).  One candidate per lane, 64 per
// step, in the reference's order (forward offsets, then reverse).  Result (offset << 8) + diff, 0x7FFFFFFF for none
// (_editdistance.cpp:150,177,181).
__global__ void seek_overlap_kernel(const uint8_t* r1, int len1, const uint8_t* rr2, int len2, int limit, int ccr, int ovr, int* out) {
    const int lane = lane_id();
    const int nf = len1 > ovr ? len1 - ovr : 0;
    const int nr = len2 > ovr ? len2 - ovr : 0;
    for (int base = 0; base < nf + nr; base += WAVE) {
        const int c = base + lane;
        bool ok = false;
        int tot = 0;
        if (c < nf + nr) {
            const int p1 = c < nf ? c : 0, p2 = c < nf ? 0 : c - nf;
            const int L = c < nf ? min(len1 - c, len2) : min(len1, len2 - p2);
            int early = 0;
            for (int i = 0; i < L; ++i) {
                const int mm = r1[p1 + i] != rr2[p2 + i] ? 1 : 0;
                tot += mm;
                if (i < ccr) early += mm;
            }
            ok = tot < limit || (early < limit && L - 1 > ccr);
        }
        const unsigned long long b = __ballot(ok);
        if (b) {
            const int l = __ffsll((long long)b) - 1;
            const int cand = base + l;
            const int t = __shfl(tot, l, WAVE);
            if (lane == 0) *out = (int)((unsigned int)(cand < nf ? cand : -(cand - nf)) << 8) + t;
            return;
        }
    }
    if (lane == 0) *out = 0x7FFFFFFF;
}

}  // namespace aqc
