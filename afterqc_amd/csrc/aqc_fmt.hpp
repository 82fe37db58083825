// aqc_fmt.hpp — FASTQ text out, on the device: the writer's model of a record — what a record of each
// output stream is made of, how many bytes it takes, and where the streams' tiles start.  The kernels that write are in aqc_fmtcopy.hpp.
//
//   formatting seqFilter.writeReads (preprocesser.py:206-232) + fastq.Writer.writeLines (fastq.py:87-93):
//              name, bases, strand line, qualities, each followed by "\n"; a bad record's name becomes
//              "@" + FLAG + name[1:]; bases/qualities are the trimmed / adapter-cut slices with the <= 3 edits of
//              the correction walk applied.  Good and bad records of each file are compacted into their own
//              contiguous text streams in record order (sizes -> exclusive scan -> copy).
//
// All of it is byte shuffling bound by HBM bandwidth; no data-dependent host work remains per record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"      // aqc_result, the AQC_* flags and edit kinds, AQC_N_FLAGS
#include "aqc_prim.hpp"       // WAVE, lane_id, load16u, wave_sum_dpp, block_excl_scan
#include "aqc_batch.hpp"      // the marks in a framed chunk's length words: LEN_IRR, LEN_MASK, QLEN_MASK, QLEN_CONTIG
#include "aqc_textin.hpp"     // the text stage's workgroup size (TXT_BLOCK): the sizing and base passes run with it
#include "aqc_fmtwin.hpp"     // the piece list of a record (FmtPiece, FmtTask), piece_items: compiles without HIP, for the CPU selftest

namespace aqc {

// ---- formatting -----------------------------------------------------------------------------------------------------
__device__ __constant__ int FLAG_TEXT_LEN[AQC_N_FLAGS] = {4, 7, 7, 8, 8, 6, 6, 6, 6, 6, 7, 11};

struct TextFile {
    const uint8_t* text;
    const uint32_t *seq_off, *qual_off;
    const uint32_t *seq_len;      // bit 31 (LEN_IRR): the quality line has a length of its own -> qual_len / qview
    const uint32_t *name_off, *name_len, *plus_off, *plus_len;      // plus_len: bit 31 = LEN_IRR again
    const uint32_t *qual_len;     // bit 31: the quality line's '\n' follows it directly (frame_records_kernel)
    const uint32_t *qview;        // final quality view (start | length << 16) of the records marked LEN_IRR, left by the verdict kernels
};

// The slice of the QUALITY line that record r of this file writes, when that line is not as long as the sequence line (LEN_IRR):
// every slice upstream is a python slice of each string by its own length, the final view is what the verdict kernel left in
// qview; getOverlap (preprocesser.py:78-84) takes r[3][len(r[3]) - overlap_len:] — a NEGATIVE start counts from the end.
__device__ __forceinline__ void irregular_quality_slice(const TextFile& tf, uint64_t r, int plain, int overlap_pass, int ovl, int& qst, int& qlen) {
    if (plain) { qst = 0; qlen = (int)(tf.qual_len[r] & QLEN_MASK); return; }
    const uint32_t qv = tf.qview[r];
    const int vs = (int)(qv & 0xffffu), vl = (int)(qv >> 16);
    qst = vs; qlen = vl;
    if (overlap_pass) {
        const int k = vl - ovl;
        if (k >= 0) { qst = vs + k; qlen = ovl; }
        else if (-k <= vl) { qst = vs + vl + k; qlen = -k; }
    }
}

struct FormatView {
    TextFile f[2];
    const aqc_result* results;
    int paired;
    int barcode;          // options.barcode: moveBarcodeToName (barcodeprocesser.py:34-45) rewrites the names
    int barcode_length;
    int store_overlap;    // --store_overlap: third stream with the overlapped tails of good pairs (preprocesser.py:78-84,614-616);
                          // AQC_STORE_MERGED (--store_merged): the same pairs as merged reads in file 0's third stream, file 1's empty
    int plain;            // index files (-7 / -5): records are written whole (no trim, no edits, no barcode move); only
                          // the verdicts — of the read pairs in `results` — route them and rename the bad ones
    int verdict_paired;   // the verdicts belong to read PAIRS (overlap stream exists)
    int spans;            // aqc_format_spans: good records that go out as their own bytes are NOT copied (they already stand in the
                          // chunk the caller framed): stream 0 holds only the good records that had to be rebuilt, and every
                          // record that is not such a "whole" record leaves an event (SpanEvent) saying where it stood
    uint32_t consumed[2]; // bytes of each file's chunk that the framed records take (the end of the last record)
    uint64_t n_framed;    // records framed into the slot (>= the n being formatted)
    int fused;            // the verdict kernel placed every record itself and copied the whole good ones (aqc_fast.hpp, FUSE): fstate[file][r] =
                          // the record's offset inside its batch's share of its stream | bit 31: already written; fbatch[2 b], [2 b + 1] =
                          // the bytes of the good / bad streams up to and including batch b (2 bits of state | file 0: 31 bits | file 1: 31 bits)
    const uint32_t* fstate[2];
    const unsigned long long* fbatch;
    int fbatch_shift;     // records per batch = 1 << fbatch_shift
};
constexpr uint32_t FMT_FUSED_DONE = 0x80000000u, FMT_FUSED_PATCH = 0x40000000u, FMT_FUSED_OFF = 0xffffu;      // (bit 30: written, but for the walk's byte patches)

// event k of a file = the k-th record (in order) that is bad or had to be rebuilt: it stood at chunk bytes [in_start, in_start +
// in_len) and contributes out_len bytes to stream 0 (0: a bad record).  The good output of the file is, in order: the chunk's
// bytes up to event 0 | out_len bytes of stream 0 | the chunk's bytes behind event 0 up to event 1 | ... up to the end of record n - 1.
struct SpanEvent { uint32_t in_start, in_len, out_len; };

// A good record that is written as its own bytes: not trimmed, not renamed, no edit of the walk in this mate, and all four lines
// followed directly by their '\n' in the chunk (QLEN_CONTIG) — the bulk of a run without trimming.
__device__ __forceinline__ bool record_is_whole(const FormatView& v, const TextFile& t, uint64_t r, int file, const uint4& w0) {
    if (v.plain || v.barcode || (int)(w0.x & 0xffu) != AQC_GOOD) return false;
    const uint32_t slw = t.seq_len[r];
    const uint32_t st = file == 0 ? (w0.x >> 16) : (w0.y >> 16), len = file == 0 ? (w0.y & 0xffffu) : (w0.z & 0xffffu);
    if (st != 0u || len != slw) return false;                      // (a mate marked LEN_IRR never equals its length word)
    if (!(t.qual_len[r] & QLEN_CONTIG)) return false;
    const int n_edits = (int)((w0.x >> 8) & 0xffu);
    if (n_edits) {
        const uint4 w1 = *(reinterpret_cast<const uint4*>(v.results + r) + 1);
        const unsigned long long e_lo = ((unsigned long long)w1.y << 32) | w1.x, e_hi = ((unsigned long long)w1.w << 32) | w1.z;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if (e < n_edits) {
                const int bit = 40 * e + 16;                       // the edit's kind byte
                const unsigned int kind = (unsigned int)((bit < 64 ? e_lo >> bit : e_hi >> (bit - 64)) & 0xffu);
                if (kind == AQC_EDIT_MASK || (kind == AQC_EDIT_FIX_R1 && file == 0) || (kind == AQC_EDIT_FIX_R2 && file == 1)) return false;
            }
        }
    }
    return true;
}

// does record r go to the overlap stream?  paired, GOOD, overlap_len > 30 and every mismatch of the overlap was
// corrected (distance == 0 or distance == corrected bases, preprocesser.py:614)
__device__ __forceinline__ bool in_overlap_stream(const FormatView& v, const uint4& w0, const uint4& w1) {
    if (!v.store_overlap || !v.verdict_paired || (int)(w0.x & 0xffu) != AQC_GOOD) return false;
    const int ovl = (int)(w0.w & 0xffffu), dist = (int)(w0.w >> 16), n_edits = (int)((w0.x >> 8) & 0xffu);
    if (ovl <= 30) return false;
    const unsigned long long e_lo = ((unsigned long long)w1.y << 32) | w1.x, e_hi = ((unsigned long long)w1.w << 32) | w1.z;
    int corrected = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (e < n_edits) {
            const int bit = 40 * e + 16;                       // the edit's kind byte
            const unsigned int kind = (unsigned int)((bit < 64 ? e_lo >> bit : e_hi >> (bit - 64)) & 0xffu);
            corrected += (kind == AQC_EDIT_FIX_R1 || kind == AQC_EDIT_FIX_R2) ? 1 : 0;
        }
    }
    return dist == 0 || dist == corrected;
}

// ---- --store_merged (store_overlap == AQC_STORE_MERGED): the pairs of the overlap stream, each written ONCE ---------------------------
//     name 1 | s1 + reverseComplement(s2[0:p]) | strand line 1 | q1 + reversed(q2[0:p])          p = len(s2) - overlap_len
// with s, q as the good streams hold them.  The walk's edits all lie inside the overlap: s2[0:p] and q2[0:p] are raw text.
__device__ __forceinline__ uint32_t merged_tail_len(const uint4& w0) {
    const int p = (int)(w0.z & 0xffffu) - (int)(w0.w & 0xffffu);
    return (uint32_t)max(p, 0);
}
// read 2's quality line, as written to good, is as long as its sequence line (else the pair has no merged read: DESIGN §7)
__device__ __forceinline__ bool merged_mate2_regular(const TextFile& t2, uint64_t r, uint32_t len2) {
    if (!(t2.plus_len[r] & LEN_IRR)) return true;
    int qs_, ql_;
    irregular_quality_slice(t2, r, 0, 0, 0, qs_, ql_);
    return (uint32_t)ql_ == len2;
}


// moveBarcodeToName for one read: the name becomes '@' + bases[0:b] + name[first ':' :]; b is the detected barcode
// length for pairs (preprocesser.py:452), the design length for single-end input (:444).  Records flagged
// BADBCD1 / BADBCD2 keep their names.  Returns b (bases moved, clipped to the read) or -1 when the name stays.
__device__ __forceinline__ int moved_barcode_len(const FormatView& v, int file, int flag, uint32_t barcode_byte, uint32_t seq_len) {
    if (!v.barcode || flag == AQC_BADBCD1 || flag == AQC_BADBCD2) return -1;
    const int code = file == 0 ? (int)(barcode_byte & 15u) : (int)(barcode_byte >> 4);
    const int b = v.paired ? code - 2 + v.barcode_length : v.barcode_length;
    return min(max(b, 0), (int)seq_len);
}

// name.find(':') over a name of nlen bytes, 16 bytes per step (an unaligned 16-byte load, the exact zero-byte test on name ^ "::::"); nlen - 1
// when there is none — find() == -1 slices the last character (barcodeprocesser.py:41).  Reads up to 15 bytes behind the name: text.
// (rounds 2 - 5: a byte load per character — the sizing pass of a barcode run took 0.35 ms per 6 M records, six times the plain run's)
__device__ __forceinline__ uint32_t find_colon(const uint8_t* name, uint32_t nlen) {
    for (uint32_t i = 0; i < nlen; i += 16u) {
        const uint4 v = load16u(name + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        unsigned long long z[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t x0 = w[2 * h] ^ 0x3a3a3a3au, x1 = w[2 * h + 1] ^ 0x3a3a3a3au;
            const uint32_t z0 = ~(((x0 & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x0) & 0x80808080u, z1 = ~(((x1 & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x1) & 0x80808080u;
            z[h] = ((unsigned long long)z1 << 32) | z0;
        }
        const uint32_t at = z[0] ? (uint32_t)(__builtin_ctzll(z[0]) >> 3) : z[1] ? 8u + (uint32_t)(__builtin_ctzll(z[1]) >> 3) : 16u;
        if (at < 16u && i + at < nlen) return i + at;
    }
    return nlen - 1u;
}

// bytes of (file, stream) that record r contributes: the sizes of all three streams of one file at once
// (sz[0] good, sz[1] bad, sz[2] overlap); the name's first ':' is only searched when a barcode was moved
__device__ __forceinline__ void fmt_sizes(const FormatView& v, uint64_t r, int file, uint32_t sz[3], uint32_t& event) {
    const uint4 w0 = *reinterpret_cast<const uint4*>(v.results + r);
    const int flag = (int)(w0.x & 0xffu);
    const TextFile& t = v.f[file];
    event = 0u;
    bool whole = false;                                     // spans mode: the record stays where it is, stream 0 does not get it
    if (v.spans) {
        whole = record_is_whole(v, t, r, file, w0);
        event = whole ? 0u : 1u;
        if (whole && !v.store_overlap) { sz[0] = sz[1] = sz[2] = 0u; return; }
    }
    uint32_t len = file == 0 ? (w0.y & 0xffffu) : (w0.z & 0xffffu);
    const uint32_t plw = t.plus_len[r];
    // (the sequence line's own length only where it is needed: index records, the barcode move, a quality line of another length)
    const uint32_t slw = (v.plain || v.barcode || (plw & LEN_IRR)) ? t.seq_len[r] : 0u;
    if (v.plain) len = slw & LEN_MASK;                      // index records go out whole
    uint32_t nlen = t.name_len[r];
    if (v.barcode && !v.plain) {
        const uint32_t bc = reinterpret_cast<const uint8_t*>(v.results + r)[31];
        const int b = moved_barcode_len(v, file, flag, bc, slw & LEN_MASK);
        if (b >= 0) {
            // name[str.find(':'):] — find() == -1 slices the last character
            const uint32_t cpos = find_colon(t.text + t.name_off[r], nlen);
            nlen = 1u + (uint32_t)b + (nlen - cpos);
        }
    }
    const uint32_t body = nlen + (plw & LEN_MASK) + 4u;
    uint32_t qlen = len;                                    // the quality line written beside `len` bases
    if (slw & LEN_IRR) {
        int qs_, ql_;
        irregular_quality_slice(t, r, v.plain, 0, 0, qs_, ql_);
        qlen = (uint32_t)ql_;
    }
    sz[0] = (flag == AQC_GOOD && !whole) ? body + len + qlen : 0u;
    sz[1] = flag == AQC_GOOD ? 0u : body + (uint32_t)FLAG_TEXT_LEN[flag] + len + qlen;
    sz[2] = 0u;
    if (v.store_overlap) {
        const uint4 w1 = *(reinterpret_cast<const uint4*>(v.results + r) + 1);
        if (v.store_overlap == AQC_STORE_MERGED) {
            // the pair written once: read 1's good record with p = len2 - overlap_len bytes more in each of its two lines
            if (file == 0 && !v.plain && qlen == len && in_overlap_stream(v, w0, w1) && merged_mate2_regular(v.f[1], r, w0.z & 0xffffu))
                sz[2] = body + len + qlen + 2u * merged_tail_len(w0);
        } else if (in_overlap_stream(v, w0, w1)) {
            const uint32_t olen = v.plain ? len : (w0.w & 0xffffu);                                   // getOverlap: the last overlap_len bases
            uint32_t oq = v.plain ? qlen : olen;
            if ((slw & LEN_IRR) && !v.plain) {
                int qs_, ql_;
                irregular_quality_slice(t, r, 0, 1, (int)olen, qs_, ql_);
                oq = (uint32_t)ql_;
            }
            sz[2] = body + olen + oq;
        }
    }
}

constexpr int FMT_TILE = 128;           // records per workgroup of the plan pass (one thread per record)
constexpr int FMT_SUPER = 8;            // tiles per workgroup of the sizing pass = per entry of the second-level scan
constexpr int FMT_STREAMS = 8;          // file * 3 + {good, bad, overlap}, then (spans mode) the two files' event counts
constexpr int FMT_EVENT_STREAM = 6;

// Sizing pass (round 6: one workgroup per FMT_SUPER tiles, wave sums through DPP, no scans).  A wave takes the 64 records of half a
// tile; what it leaves behind, per stream q = file * 3 + stream:
//     tile_sum[q * n_tiles + tile]   the bytes of the tiles BEFORE this one inside its super-tile (a prefix the plan pass adds to ...)
//     super_sum[q * n_super + s]     ... the bytes of super-tile s, turned into the bytes before it by fmt_tile_bases_kernel
// (rounds 2 - 5: a workgroup of 128 threads per tile, four block scans of two barriers each to get four sums — 78 k workgroups and
//  0.26 ms per 10 M reads for 0.1 GB of input; the scan over all 78 k tile sums per stream, six workgroups, was another 0.11 ms)
__global__ __launch_bounds__(TXT_BLOCK) void fmt_tile_sums_kernel(FormatView v, uint64_t n, uint64_t n_tiles, uint64_t n_super,
                                                                  unsigned long long* __restrict__ tile_sum, unsigned long long* __restrict__ super_sum) {
    constexpr int HALVES = FMT_SUPER * FMT_TILE / WAVE;                   // waves' worth of records per super-tile
    constexpr int ROUNDS = FMT_SUPER * FMT_TILE / TXT_BLOCK;
    static_assert(FMT_TILE == 2 * WAVE && HALVES * WAVE == ROUNDS * TXT_BLOCK, "a tile is two waves' records");
    __shared__ uint32_t part[HALVES][FMT_STREAMS];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int nfiles = v.paired ? 2 : 1;
    for (int i = threadIdx.x; i < HALVES * FMT_STREAMS; i += TXT_BLOCK) (&part[0][0])[i] = 0u;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * (FMT_SUPER * FMT_TILE);
#pragma unroll 1
    for (int it = 0; it < ROUNDS; ++it) {
        const uint64_t r = r0 + (uint64_t)it * TXT_BLOCK + threadIdx.x;
        const int half = it * (TXT_BLOCK / WAVE) + wave;
        if (r0 + (uint64_t)half * WAVE >= n) break;                      // (wave-uniform: nothing of this wave's records exists)
        for (int file = 0; file < nfiles; ++file) {
            uint32_t sz[3] = {0, 0, 0}, ev = 0;
            if (r < n) fmt_sizes(v, r, file, sz, ev);
            // (a record is < 64 KiB, a wave's sum < 4 MiB: int arithmetic; all 64 lanes are here)
            const int g = wave_sum_dpp((int)sz[0]), b = wave_sum_dpp((int)sz[1]);
            if (lane == 0) { part[half][file * 3 + 0] = (uint32_t)g; part[half][file * 3 + 1] = (uint32_t)b; }
            if (v.store_overlap) {
                const int o = wave_sum_dpp((int)sz[2]);
                if (lane == 0) part[half][file * 3 + 2] = (uint32_t)o;
            }
            if (v.spans) {                                               // streams 6, 7: the files' event counts
                const int e = wave_sum_dpp((int)ev);
                if (lane == 0) part[half][FMT_EVENT_STREAM + file] = (uint32_t)e;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < FMT_STREAMS) {
        const int q = threadIdx.x;
        unsigned long long run = 0;
        for (int t = 0; t < FMT_SUPER; ++t) {
            const uint64_t tile = (uint64_t)blockIdx.x * FMT_SUPER + t;
            if (tile < n_tiles) tile_sum[(uint64_t)q * n_tiles + tile] = run;
            run += (unsigned long long)part[2 * t][q] + part[2 * t + 1][q];
        }
        super_sum[(uint64_t)q * n_super + blockIdx.x] = run;
    }
}

// exclusive scan of each stream's super-tile sums (workgroup q handles stream q, eight entries per thread per round); totals to total_out[q]
__global__ __launch_bounds__(TXT_BLOCK) void fmt_tile_bases_kernel(unsigned long long* __restrict__ tile_sum, uint64_t n_tiles,
                                                                   unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long lds[4];
    constexpr int PER = 8;
    unsigned long long* ts = tile_sum + (uint64_t)blockIdx.x * n_tiles;
    unsigned long long carry = 0;
    for (uint64_t t0 = 0; t0 < n_tiles; t0 += (uint64_t)TXT_BLOCK * PER) {
        const uint64_t t = t0 + (uint64_t)threadIdx.x * PER;
        unsigned long long val[PER], sum = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            val[k] = t + k < n_tiles ? ts[t + k] : 0ull;
            sum += val[k];
        }
        unsigned long long total;
        unsigned long long run = carry + block_excl_scan(sum, lds, total);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (t + k < n_tiles) ts[t + k] = run;
            run += val[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) total_out[blockIdx.x] = carry;
}

// ---- one record of one file, as the writer sees it --------------------------------------------------------------------
// The output record is a sequence of pieces
//     '@' FLAG | barcode bases | name tail | \n | bases | \n | strand line | \n | qualities | \n
// each copied from a source: the chunk's text, or a small table of literals ("@BADPOL", "\n", "@").  Neighbouring pieces
// that are neighbours in the text as well are merged while the list is built, so an untrimmed good record is ONE piece
// (the record's own bytes), a tail-trimmed one three, a renamed (bad) one two more.
// (FmtPiece, FmtTask, FMT_MAXP, FMT_LIT_BIT, GRID_MIN and piece_items — the work items of a piece — are in aqc_fmtwin.hpp)

// literals: row f < 12 = "@" + FLAG text, row 12 = "\n", row 13 = "@"
__device__ uint8_t FMT_LIT[16][16] = {"@GOOD", "@BADBCD1", "@BADBCD2", "@BADTRIM1", "@BADTRIM2", "@BADBBL", "@BADLEN", "@BADPOL", "@BADLQC",
                                      "@BADNCT", "@BADDIFF", "@BADMISMATCH", "\n", "@", "", ""};

__device__ __forceinline__ void fmt_add(FmtTask& t, int& o, int len, uint32_t src) {
    if (len <= 0) return;
    if (t.np > 0) {
        FmtPiece& q = t.p[t.np - 1];
        if (!((q.src | src) & FMT_LIT_BIT) && q.src + q.len == src && (int)q.len + len <= 0xffff) {       // neighbours in the text too
            q.len = (uint16_t)(q.len + len);
            o += len;
            return;
        }
    }
    if (t.np < FMT_MAXP) {
        t.p[t.np].src = src; t.p[t.np].dst = (uint16_t)o; t.p[t.np].len = (uint16_t)len;
        t.np++;
    }
    o += len;
}

// the piece list of record r of `file` for this pass (main: good / bad, overlap_pass: the overlap stream)
__device__ inline void fmt_build(const FormatView& v, uint64_t r, int file, int overlap_pass, FmtTask& t, int* status) {
    const uint4 w0 = *reinterpret_cast<const uint4*>(v.results + r);
    const uint4 w1 = *(reinterpret_cast<const uint4*>(v.results + r) + 1);
    const int flag = (int)(w0.x & 0xffu);
    const int n_edits = v.plain ? 0 : (int)((w0.x >> 8) & 0xffu);
    t.np = 0; t.n_patch = 0; t.pad_ = 0; t.items = 0; t.total = 0;
    if (overlap_pass) t.stream = in_overlap_stream(v, w0, w1) ? 2 : 0xff;
    else t.stream = flag == AQC_GOOD ? 0 : 1;
    if (t.stream == 0xff) return;
    const int len1 = (int)(w0.y & 0xffffu), len2 = (int)(w0.z & 0xffffu), ovl = (int)(w0.w & 0xffffu);
    const TextFile& tf = v.f[file];
    const uint32_t name_off = tf.name_off[r], seq_off = tf.seq_off[r], plus_off = tf.plus_off[r], qual_off = tf.qual_off[r];
    const uint32_t slw = tf.seq_len[r];
    const int nlen = (int)tf.name_len[r], plen = (int)(tf.plus_len[r] & LEN_MASK), slen = (int)(slw & LEN_MASK);
    // the slice of the original read that is written: the final read, or its last overlap_len bases (getOverlap)
    const int cut = v.plain ? 0 : (overlap_pass ? (file == 0 ? len1 : len2) - ovl : 0);
    const int st = v.plain ? 0 : (file == 0 ? (int)(w0.x >> 16) : (int)(w0.y >> 16)) + cut;
    const int len = v.plain ? slen : (overlap_pass ? ovl : (file == 0 ? len1 : len2));
    const int flen = t.stream == 1 ? FLAG_TEXT_LEN[flag] : 0;
    // barcode moved into the name: '@' + [FLAG] + bases[0:mb] + name[cpos:]  (name[str.find(':'):]; find() == -1 slices the last character)
    const int mb = (v.barcode && !v.plain) ? moved_barcode_len(v, file, flag, w1.w >> 24, (uint32_t)slen) : -1;
    const int cpos = mb >= 0 ? (int)find_colon(tf.text + name_off, (uint32_t)nlen) : nlen - 1;
    const uint32_t NL = FMT_LIT_BIT | (12 * 16);
    int o = 0;
    // "@" + FLAG + name[1:] for a bad record (preprocesser.py:213-219), the name itself for a good one
    const bool renamed = t.stream == 1 || mb >= 0;
    if (renamed) fmt_add(t, o, 1 + flen, FMT_LIT_BIT | (uint32_t)((t.stream == 1 ? flag : 13) * 16));
    if (mb >= 0) { fmt_add(t, o, mb, seq_off); fmt_add(t, o, nlen - cpos, name_off + (uint32_t)cpos); }
    else if (renamed) fmt_add(t, o, nlen - 1, name_off + 1);
    else fmt_add(t, o, nlen, name_off);
    // the newlines come from the text where the text has them right there (no stripped whitespace), else from the table
    fmt_add(t, o, 1, seq_off == name_off + (uint32_t)nlen + 1 ? name_off + (uint32_t)nlen : NL);
    const int seq_dst = o;
    fmt_add(t, o, len, seq_off + (uint32_t)st);
    fmt_add(t, o, 1, plus_off == seq_off + (uint32_t)slen + 1 ? seq_off + (uint32_t)slen : NL);
    fmt_add(t, o, plen, plus_off);
    fmt_add(t, o, 1, qual_off == plus_off + (uint32_t)plen + 1 ? plus_off + (uint32_t)plen : NL);
    const int qual_dst = o;
    // the quality line: the same slice as the bases, unless this record's quality line has a length of its own
    int qst = st, qlen = len, qline = slen;
    const bool irr = (slw & LEN_IRR) != 0u;
    if (irr) {
        qline = (int)(tf.qual_len[r] & QLEN_MASK);
        irregular_quality_slice(tf, r, v.plain, overlap_pass, ovl, qst, qlen);
    }
    fmt_add(t, o, qlen, qual_off + (uint32_t)qst);
    fmt_add(t, o, 1, (qst + qlen == qline && (tf.qual_len[r] >> 31)) ? qual_off + (uint32_t)qline : NL);
    if (o > 0xffff) { atomicCAS(status, 0, AQC_ERR_UNSUPPORTED); t.stream = 0xff; return; }      // (a 64 KiB FASTQ record)
    t.total = (uint16_t)o;
    int items = 0;
    for (int k = 0; k < t.np; ++k) items += (int)piece_items(t.p[k].len);
    t.items = (uint16_t)items;
    // the walk's edits in this mate's slice coordinates -> byte patches of the output record
    const unsigned long long e_lo = ((unsigned long long)w1.y << 32) | w1.x, e_hi = ((unsigned long long)w1.w << 32) | w1.z;
    for (int e = 0; e < n_edits && e < 3; ++e) {
        const int bit = 40 * e;
        unsigned long long x = bit < 64 ? e_lo >> bit : 0ull;
        if (bit + 40 > 64) x |= bit < 64 ? e_hi << (64 - bit) : e_hi >> (bit - 64);
        const int oo = (int)(x & 0xffffu);
        const uint32_t kind = (uint32_t)(x >> 16) & 0xffu, base = (uint32_t)(x >> 24) & 0xffu, qual = (uint32_t)(x >> 32) & 0xffu;
        const int pp = (file == 0 ? len1 - ovl + oo : len2 - 1 - oo) - cut;
        if (irr) {
            // each string was edited at its OWN index (preprocesser.py:575-576,583-584,591-592): the bases at pp, the quality
            // view (start vs, length vl) at vl - overlap_len + o (a negative index wraps) resp. vl - 1 - o; two edits may meet
            // in one quality character — the later one stands
            const uint32_t qv = tf.qview[r];
            const int vs = (int)(qv & 0xffffu), vl = (int)(qv >> 16);
            int iq = file == 0 ? vl - ovl + oo : vl - 1 - oo;
            if (iq < 0) iq += vl;
            const int qp = vs + iq - qst;                    // in the slice that is written
            const bool mine = (kind == AQC_EDIT_FIX_R1 && file == 0) || (kind == AQC_EDIT_FIX_R2 && file == 1);
            if (mine && base && pp >= 0 && pp < len) t.patch[t.n_patch++] = (uint32_t)(seq_dst + pp) | (base << 16);
            if ((mine || kind == AQC_EDIT_MASK) && iq >= 0 && qp >= 0 && qp < qlen) {
                const uint32_t at = (uint32_t)(qual_dst + qp), val = kind == AQC_EDIT_MASK ? (uint32_t)'!' : qual;
                bool merged = false;
                for (int k = 0; k < (int)t.n_patch; ++k)
                    if ((t.patch[k] & 0xffffu) == at) { t.patch[k] = at | (val << 16); merged = true; }
                if (!merged) t.patch[t.n_patch++] = at | (val << 16);
            }
            continue;
        }
        if (pp < 0 || pp >= len) continue;
        if (kind == AQC_EDIT_MASK) t.patch[t.n_patch++] = (uint32_t)(qual_dst + pp) | ((uint32_t)'!' << 16);
        else if ((kind == AQC_EDIT_FIX_R1 && file == 0) || (kind == AQC_EDIT_FIX_R2 && file == 1)) {
            if (base) t.patch[t.n_patch++] = (uint32_t)(seq_dst + pp) | (base << 16);
            t.patch[t.n_patch++] = (uint32_t)(qual_dst + pp) | (qual << 16);
        }
    }
}

struct FormatOut {
    uint8_t* p[6];        // [file * 3 + stream]
};

}  // namespace aqc
