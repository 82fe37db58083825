// aqc_qcstat.hpp — the statRead stage (qualitycontrol.py:73-122): the read descriptors of the sampling kernels, the per-cycle
// accumulators, and qc_stat_kernel / kmer_count_kernel / kmer_reduce_kernel / the two compact kernels.  The k-mer table they fill
// (KmerTable) is a member of the context and sits with the other descriptors in aqc_batch.hpp; comp_or_n comes from aqc_prim.hpp.
// It defines kernels: aqc_capi_qc.hip is the one unit that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"
#include "aqc_prim.hpp"
#include "aqc_batch.hpp"      // DevBatch, KmerTable and the sizes of its dense tables

namespace aqc {

// ------------------------------------------------------------------------------------------------
// QualityControl.statRead (qualitycontrol.py:73-122): one wave per read, lane = cycle.
// Block-private u32 accumulators in LDS, flushed with 64-bit global atomics at the end.
// k-mers go to an open-addressing table in HBM keyed by the k raw bytes (k <= 8).
// ------------------------------------------------------------------------------------------------
constexpr int KRED_BLOCK = 256;

// id of the XCD this wave runs on (HW_REG_XCC_ID, bits 3:0)
__device__ __forceinline__ uint32_t xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & (N_XCD - 1); }

// reverse complement of a dense k-mer index: complement flips the code's high bit, the order of bases reverses
__device__ __host__ inline uint32_t dense_rc(uint32_t idx, int k) {
    // reverse the order of the 2-bit codes and complement each (A0 <-> T2, C1 <-> G3: code ^ 2)
    uint32_t r = 0;
    for (int j = 0; j < k; ++j) r |= (((idx >> (2 * j)) & 3u) ^ 2u) << (2 * (k - 1 - j));
    return r;
}

__device__ __forceinline__ uint64_t hash64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

// Key 0 marks an empty slot, and it is also the key of the k-mer of k NUL bytes (a zero-filled block of a damaged
// file): that k-mer gets the dedicated entry mask + 1 of counts / order, and never claims a slot.  (No spare key
// value exists to remap it to: for k = 8 every 64-bit value is some k-mer's key.)
__device__ inline long long kmer_slot(const KmerTable& t, unsigned long long key) {
    if (key == 0) return (long long)(t.mask + 1);
    uint64_t h = hash64(key) & t.mask;
    for (uint64_t probe = 0; probe <= t.mask; probe++) {
        unsigned long long cur = t.keys[h];
        if (cur == key) return (long long)h;
        if (cur == 0) {
            unsigned long long prev = atomicCAS(&t.keys[h], 0ull, key);
            if (prev == 0 || prev == key) return (long long)h;
        }
        h = (h + 1) & t.mask;
    }
    return -1;
}

// both slots of a k-mer and its reverse complement: the two first probes travel together (the common case, both
// keys already present, costs ONE memory round trip)
__device__ __forceinline__ void kmer_slot2(const KmerTable& t, unsigned long long key, unsigned long long rkey,
                                           long long& h, long long& hr) {
    const uint64_t a = hash64(key) & t.mask, b = hash64(rkey) & t.mask;
    const unsigned long long ka = t.keys[a], kb = t.keys[b];
    h = ka == key && key != 0 ? (long long)a : kmer_slot(t, key);
    hr = kb == rkey && rkey != 0 ? (long long)b : kmer_slot(t, rkey);
}

// ------------------------------------------------------------------------------------------------
// Read descriptors for the sampling kernels.  A wavefront that walks its reads one by one pays the chain
// len/offset -> verdict record -> bases -> table probe as four DEPENDENT memory round trips per read (~6 us on
// this chip), which is what bounded both sampling kernels.  Instead lane j fetches the descriptor of the
// wave's j-th read (64 descriptors per two round trips), the loop broadcasts one descriptor per iteration with
// v_readlane, and the bases of read j+1 are loaded into registers while read j is being accumulated.
//   len  < 0 : not part of the sample (verdict not GOOD / beyond the range)
//   e[k]     : the walk's k-th edit as it applies to THIS mate in final-read coordinates,
//              pos << 16 | new base << 8 | new quality   (base 0 = keep the base: a mask edit; pos 0xffff = none)
// ------------------------------------------------------------------------------------------------
struct ReadDesc {
    unsigned long long s, q;
    int len;
    int qlen;                // length of the quality view (== len unless the record's quality line has a length of its own)
    unsigned int e[3];
};

__device__ __forceinline__ ReadDesc lane_desc(const DevBatch& b, int mate, uint64_t rec, bool valid, int post,
                                              const aqc_result* __restrict__ results) {
    ReadDesc d;
    d.s = d.q = 0ull;
    d.len = -1;
    d.qlen = -1;
    d.e[0] = d.e[1] = d.e[2] = 0xffff0000u;
    if (!valid) return d;
    int len, st = 0;
    uint32_t lw;
    if (mate == 0) {
        lw = b.len1[rec];
        const uint64_t o = b.off1[rec];
        d.s = (unsigned long long)(b.seq1 + o);
        d.q = (unsigned long long)(b.qual1 + (b.qoff1 ? b.qoff1[rec] : o));
    } else {
        lw = b.len2[rec];
        const uint64_t o = b.off2[rec];
        d.s = (unsigned long long)(b.seq2 + o);
        d.q = (unsigned long long)(b.qual2 + (b.qoff2 ? b.qoff2[rec] : o));
    }
    len = (int)(lw & LEN_MASK);
    // this mate's quality line has a length of its own: its view comes from qlen (raw read) / qview (final read)
    const bool irr = (lw & LEN_IRR) != 0u && b.qlen1 != nullptr;
    int qst = 0, qlen = irr ? (int)((mate == 0 ? b.qlen1[rec] : b.qlen2[rec]) & QLEN_MASK) : len;
    if (post) {
        // the 32-byte verdict record as two 16-byte loads; fields by shifts (aqc_result is packed, see the header)
        const uint4* rp = reinterpret_cast<const uint4*>(results + rec);
        const uint4 w0 = rp[0], w1 = rp[1];
        if ((w0.x & 0xffu) != (unsigned int)AQC_GOOD) return d;   // only good records reach preprocesser.py:624-627
        const int n_edits = (int)((w0.x >> 8) & 0xffu);
        const int len1 = (int)(w0.y & 0xffffu), len2 = (int)(w0.z & 0xffffu), ovl = (int)(w0.w & 0xffffu);
        st = mate == 0 ? (int)(w0.x >> 16) : (int)(w0.y >> 16);
        len = mate == 0 ? len1 : len2;
        qst = st; qlen = len;
        if (irr) {
            const uint32_t qv = mate == 0 ? b.qview1[rec] : b.qview2[rec];
            qst = (int)(qv & 0xffffu); qlen = (int)(qv >> 16);
        }
        const unsigned long long e_lo = ((unsigned long long)w1.y << 32) | w1.x, e_hi = ((unsigned long long)w1.w << 32) | w1.z;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if (e < n_edits) {
                // edit e = 5 bytes at byte 5e of the 16: o (u16), kind, base, qual
                const int bit = 40 * e;
                unsigned long long v = bit < 64 ? e_lo >> bit : 0ull;
                if (bit + 40 > 64) v |= bit < 64 ? e_hi << (64 - bit) : e_hi >> (bit - 64);
                const int o = (int)(v & 0xffffu);
                const unsigned int kind = (unsigned int)(v >> 16) & 0xffu, base = (unsigned int)(v >> 24) & 0xffu, qual = (unsigned int)(v >> 32) & 0xffu;
                const unsigned int pos = mate == 0 ? (unsigned int)(len1 - ovl + o) : (unsigned int)(len2 - 1 - o);
                if (kind == AQC_EDIT_MASK) d.e[e] = (pos << 16) | (unsigned int)'!';
                else if ((kind == AQC_EDIT_FIX_R1 && mate == 0) || (kind == AQC_EDIT_FIX_R2 && mate == 1))
                    d.e[e] = (pos << 16) | (base << 8) | qual;
            }
        }
    }
    d.s += (unsigned int)st;
    d.q += (unsigned int)(post ? qst : 0);
    d.len = len;
    d.qlen = qlen;
    return d;
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int j) {
    const unsigned int lo = __builtin_amdgcn_readlane((int)(unsigned int)v, j);
    const unsigned int hi = __builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ ReadDesc bcast_desc(const ReadDesc& d, int j) {
    ReadDesc o;
    o.s = readlane64(d.s, j);
    o.q = readlane64(d.q, j);
    o.len = __builtin_amdgcn_readlane(d.len, j);
    o.qlen = __builtin_amdgcn_readlane(d.qlen, j);
    o.e[0] = (unsigned int)__builtin_amdgcn_readlane((int)d.e[0], j);
    o.e[1] = (unsigned int)__builtin_amdgcn_readlane((int)d.e[1], j);
    o.e[2] = (unsigned int)__builtin_amdgcn_readlane((int)d.e[2], j);
    return o;
}

// four consecutive bytes of a read starting at byte x; bytes at or beyond `len` read as the (byte-uniform) `pad`.
// Branch-free so that a prefetch stays asynchronous: ONE unaligned dword load from an address clamped into the
// read (len >= 4), then a funnel shift brings the pad in from the top.
__device__ __forceinline__ uint32_t load4(const uint8_t* p, int x, int len, uint32_t pad) {
    const int xa = min(x, len - 4);
    uint32_t dw = pad;
    if (x < len) dw = gload_u32(p + xa);      // (global_load: the pointer came through v_readlane and would otherwise be a flat_load)
    return __builtin_amdgcn_alignbit(pad, dw, (unsigned)(8 * (x - xa)) & 31u);
}

// the walk's edits that fall into the dword at byte offset x (d is wave-uniform, so the outer tests are scalar)
// (IRR: the caller may meet reads whose quality view has a length of its own — qc_stat_kernel; the fused k-mer kernel, which runs at
//  its register limit, leaves such reads' per-cycle statistics to that kernel and only ever needs the bases here)
template <bool IRR>
__device__ __forceinline__ void apply_edits(const ReadDesc& d, int x, uint32_t& ws, uint32_t& wq) {
    if (IRR && d.qlen != d.len) {
        // a quality view of its own length: the walk indexed it from ITS end (preprocesser.py:566-567) — position + (qlen - len),
        // a negative index wrapped the python way; edits in order, a later one wins (d is wave-uniform: scalar branches)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const unsigned int ed = d.e[e];
            if ((ed >> 16) != 0xffffu) {
                const unsigned int rel = (ed >> 16) - (unsigned int)x;
                if (rel < 4u && ((ed >> 8) & 0xffu)) ws = (ws & ~(0xffu << (8u * rel))) | (((ed >> 8) & 0xffu) << (8u * rel));
                int qp = (int)(ed >> 16) + d.qlen - d.len;
                if (qp < 0) qp += d.qlen;
                const unsigned int relq = (unsigned int)(qp - x);
                if (qp >= 0 && relq < 4u) wq = (wq & ~(0xffu << (8u * relq))) | ((ed & 0xffu) << (8u * relq));
            }
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const unsigned int ed = d.e[e];
        if ((ed >> 16) != 0xffffu) {
            const unsigned int rel = (ed >> 16) - (unsigned int)x;
            if (rel < 4u) {
                const unsigned int sh = 8u * rel;
                if ((ed >> 8) & 0xffu) ws = (ws & ~(0xffu << sh)) | (((ed >> 8) & 0xffu) << sh);
                wq = (wq & ~(0xffu << sh)) | ((ed & 0xffu) << sh);
            }
        }
    }
}

// 0x80 in every byte of x that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
    return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

constexpr uint32_t CODE_TO_BASE = 0x47544341u;   // 2-bit code (c >> 1) & 3 -> 'A' 'C' 'T' 'G'

// ------------------------------------------------------------------------------------------------
// Per-cycle accumulators of statRead (qualitycontrol.py:73-111).  A lane owns FOUR consecutive cycles of the
// read: one unaligned dword of bases and one of qualities live in registers (no LDS staging), the neighbours'
// dwords come over the wave for the 5-wide discontinuity window, and a base's count and quality sum travel in
// ONE LDS atomic (count << 20 | sum of the RAW quality bytes; at most 4095 reads per workgroup, 4095 * 255 < 2^20).
// The flush subtracts 33 per count: qualNum is ord(q) - 33 for any byte (util.py:39-40), so a control byte or a
// space inside a quality line is a negative quality upstream, and a per-byte "q - '!'" would borrow from the next
// field.  total_num / total_qual are column sums of the five rows (A T C G other), formed when the workgroup flushes.
// ------------------------------------------------------------------------------------------------
constexpr int QC_BLOCK = 1024;
constexpr int QC_WPB = QC_BLOCK / WAVE;
constexpr int QC_LDS_ROWS = 6;            // A T C G other | discontinuity   (+ gc histogram)
constexpr int QC_MAX_READS_PER_BLOCK = 4095;

struct QcLds {
    unsigned int* accs;          // [QC_LDS_ROWS][cols], columns permuted (see qc_accumulate_read)
    unsigned int* gch;           // [cols] GC histogram
    unsigned long long* scal;    // [0] totalKmer, [1] reads
    int cols;
};

// statRead's per-cycle part for ONE read (wave-wide).  ws / wq: the lane's dword of bases / qualities of pass 0
// (bytes 4*lane .. 4*lane+3, zero beyond the read), without the walk's edits.
// Column i lives at word (i & 3) * (cols / 4) + (i >> 2): the four cycles a lane owns are cols/4 words apart and
// neighbouring lanes hit neighbouring banks (the natural layout would be a 4-way bank conflict on every add).
template <bool IRR>
__device__ __forceinline__ void qc_accumulate_read(const ReadDesc& cur, uint32_t ws, uint32_t wq, const QcLds& L, int kmer_len) {
    const int lane = lane_id();
    const int len = cur.len;
    const int qlen = IRR ? cur.qlen : cur.len;               // (the pass-0 dword of qualities was loaded against it)
    const int cols = L.cols, cq = L.cols >> 2;
    unsigned int* const accs = L.accs;
    unsigned int* const gch = L.gch;
    unsigned long long* const scal = L.scal;
    const uint8_t* gs = reinterpret_cast<const uint8_t*>(cur.s);
    const uint8_t* gq = reinterpret_cast<const uint8_t*>(cur.q);
    int gc = 0;
    unsigned int d_head = 0, d_tail = 0;      // discontinuity of cycle 2 / cycle len-3: the clamped windows
    for (int base0 = 0; base0 < len; base0 += 4 * WAVE) {
        const int x = base0 + 4 * lane;
        if (base0 > 0) { ws = load4(gs, x, len, 0); wq = load4(gq, x, qlen, 0); }
        apply_edits<IRR>(cur, x, ws, wq);
        uint32_t prev = __shfl_up(ws, 1), next = __shfl_down(ws, 1);
        if (base0 > 0 && lane == 0) { uint32_t dq = 0; prev = load4(gs, x - 4, len, 0); apply_edits<false>(cur, x - 4, prev, dq); }
        if (base0 + 4 * WAVE < len && lane == WAVE - 1) { uint32_t dq = 0; next = load4(gs, x + 4, len, 0); apply_edits<false>(cur, x + 4, next, dq); }
        // bytes x-2 .. x+5 ; byte k of (v ^ v >> 8) is non-zero iff bases x-2+k and x-1+k differ
        const uint32_t vlo = __builtin_amdgcn_alignbit(ws, prev, 16), vhi = __builtin_amdgcn_alignbit(next, ws, 16);
        const uint32_t tlo = nonzero_bytes(vlo ^ __builtin_amdgcn_alignbit(vhi, vlo, 8));
        const uint32_t thi = nonzero_bytes(vhi ^ (vhi >> 8));
        unsigned int dpk = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) dpk |= (unsigned int)__popc(__builtin_amdgcn_alignbit(thi, tlo, 8 * j)) << (3 * j);
        if (base0 == 0) d_head = ((unsigned int)__builtin_amdgcn_readlane((int)dpk, 0) >> 6) & 7u;
        const int tl = len - 3 - base0;                 // cycle len-3 relative to this pass (uniform)
        if (tl >= 0 && tl < 4 * WAVE)
            d_tail = ((unsigned int)__builtin_amdgcn_readlane((int)dpk, tl >> 2) >> (3 * (tl & 3))) & 7u;
        // the lane's four cycles at once: accumulator row per base (A T C G = 0..3, anything else 4), raw quality byte
        // per cycle, the clamped discontinuity windows patched into the packed fields; then per cycle only two field
        // extractions, one multiply-add for the address and the atomics remain
        if (base0 == 0 && lane == 0) dpk = (dpk & ~0x3fu) | d_head | (d_head << 3);     // cycles 0, 1: window [0, 5)
        {
            const int over = min(max(x + 3 - (len - 3), 0), 4);                         // cycles beyond len-3: window [len-5, len)
            const unsigned int m = over ? (0xfffu << (3 * (4 - over))) & 0xfffu : 0u;
            dpk = (dpk & ~m) | ((d_tail * 0x249u) & m);
        }
        if (IRR && qlen < len) {
            // A quality line shorter than the read (qualitycontrol.py:81-88): totalNum[i] is counted, then qual[i] raises and the
            // rest of the position is skipped — no quality sum, no base count, no G/C, no discontinuity.  In these accumulators
            // that is a "foreign" base (byte 0: row 4, which only feeds the total_num / total_qual column sums) of quality '!' = 0
            // whose discontinuity is dropped; the discontinuities of the cycles before it were formed from the real bases above.
            // (Edited in place: the kernels that inline this run at their register limit.)
            const int qin = min(max(qlen - x, 0), 4);
            const uint32_t qm = qin >= 4 ? 0xffffffffu : ((1u << (8 * qin)) - 1u);
            ws &= qm;
            wq = (wq & qm) | (0x21212121u & ~qm);
            dpk &= qin >= 4 ? 0xfffu : ((1u << (3 * qin)) - 1u);
        }
        const uint32_t codes = (ws >> 1) & 0x03030303u;
        const uint32_t bad = __builtin_amdgcn_perm(0u, CODE_TO_BASE, codes) ^ ws;       // 0 where the byte is A/C/G/T
        const uint32_t nz = nonzero_bytes(bad);                                         // 0x80 per foreign byte
        const uint32_t foreign = nz | (nz - (nz >> 7));                                 // 0xff per foreign byte
        // code (A0 C1 T2 G3) -> row (A0 T1 C2 G3); foreign -> 4
        const uint32_t rows4 = (__builtin_amdgcn_perm(0u, 0x03010200u, codes) & ~foreign) | (0x04040404u & foreign);
        const int nin = min(max(len - x, 0), 4);                                        // cycles of this lane inside the read
        const unsigned int col0 = (unsigned int)lane + (unsigned int)(base0 >> 2);
        // G / C among the lane's cycles inside the read (C = code 1, G = code 3: low code bit), not foreign
        const uint32_t gcm = codes & 0x01010101u & ~foreign & (nin >= 4 ? 0x01010101u : ((1u << (8 * nin)) - 1u));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < nin) {
                const unsigned int row = (rows4 >> (8 * j)) & 0xffu;
                atomicAdd(&accs[row * (unsigned int)cols + (unsigned int)(j * cq) + col0], (1u << 20) + ((wq >> (8 * j)) & 0xffu));
                // discontinuity over the 5-wide window clamped to the read (qualitycontrol.py:97-109)
                const unsigned int d = (dpk >> (3 * j)) & 7u;
                if (d) atomicAdd(&accs[5u * (unsigned int)cols + (unsigned int)(j * cq) + col0], d);
            }
            gc += __popcll(__ballot((gcm >> (8 * j)) & 1u));
        }
    }
    if (lane == 0) {
        atomicAdd(&gch[gc], 1u);
        atomicAdd(&scal[1], 1ull);
        if (len > kmer_len) atomicAdd(&scal[0], (unsigned long long)(len - kmer_len));
    }
}

__global__ __launch_bounds__(QC_BLOCK) void qc_stat_kernel(DevBatch b, int mate, uint64_t first, uint64_t count, int post,
                                                           const aqc_result* __restrict__ results, int kmer_len,
                                                           unsigned long long* __restrict__ qc /* [QC_ROWS*QC_COLS] */,
                                                           int* status, int cols, int only_irr) {
    // (only_irr: the reads whose quality view has a length of its own, and nothing else — the fused k-mer kernel has left exactly
    //  those reads' per-cycle statistics to this one)
    // dynamic LDS, sized by the longest read of the batch (cols = multiple of 64 <= 1024)
    extern __shared__ __attribute__((aligned(16))) unsigned int qc_smem[];
    unsigned int* const accs = qc_smem;                               // accs[row * cols + i]
    unsigned int* const gch = qc_smem + QC_LDS_ROWS * cols;
    unsigned long long* const scal = reinterpret_cast<unsigned long long*>(gch + cols);
    const int lane = lane_id();
    const int wave = threadIdx.x / WAVE;
    for (int i = threadIdx.x; i < (QC_LDS_ROWS + 1) * cols; i += QC_BLOCK) qc_smem[i] = 0;
    if (threadIdx.x < 2) scal[threadIdx.x] = 0;
    __syncthreads();
    const int cq = cols >> 2;
    const uint64_t nwaves = (uint64_t)gridDim.x * QC_WPB;
    if ((count + nwaves - 1) / nwaves * QC_WPB > (uint64_t)QC_MAX_READS_PER_BLOCK) {      // host sizes the grid; never silently overflow
        if (threadIdx.x == 0) atomicCAS(status, 0, AQC_ERR_STATE);
        return;
    }
    auto usable = [&](const ReadDesc& d) { return d.len >= 5 && d.len <= AQC_MAX_READ_LEN && d.len <= cols && (!only_irr || d.qlen != d.len); };
    for (uint64_t kb = (uint64_t)blockIdx.x * QC_WPB + wave; kb < count; kb += nwaves * WAVE) {
        const uint64_t myk = kb + (uint64_t)lane * nwaves;
#if defined(__HIP_DEVICE_COMPILE__)
        const DevBatch __attribute__((address_space(4)))* kb_args = (const DevBatch __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kb_args));          // (read where it is used, not held across the loop: see kmer_count_kernel)
        const DevBatch bb = *kb_args;              // (the batch descriptor is the kernel's first argument)
#else
        const DevBatch bb = b;
#endif
        const ReadDesc mine = lane_desc(bb, mate, first + myk, myk < count, post, results);
        const int nr = (int)min((uint64_t)WAVE, (count - kb + nwaves - 1) / nwaves);
        ReadDesc cur = bcast_desc(mine, 0);
        uint32_t pre_s = 0, pre_q = 0;
        if (usable(cur)) {
            pre_s = load4(reinterpret_cast<const uint8_t*>(cur.s), 4 * lane, cur.len, 0);
            pre_q = load4(reinterpret_cast<const uint8_t*>(cur.q), 4 * lane, cur.qlen, 0);
        }
        for (int r = 0; r < nr; ++r) {
            uint32_t ws = pre_s, wq = pre_q;
            ReadDesc nxt = cur;
            if (r + 1 < nr) {
                nxt = bcast_desc(mine, r + 1);
                if (usable(nxt)) {
                    pre_s = load4(reinterpret_cast<const uint8_t*>(nxt.s), 4 * lane, nxt.len, 0);
                    pre_q = load4(reinterpret_cast<const uint8_t*>(nxt.q), 4 * lane, nxt.qlen, 0);
                }
            }
            const int len = cur.len;
            if (only_irr) { }                                                                    // (the fused kernel has reported these)
            else if (len > AQC_MAX_READ_LEN || len > cols) { if (lane == 0) atomicCAS(status, 0, AQC_ERR_READ_TOO_LONG); }
            else if (len < 5 && len > 0) { if (lane == 0) atomicCAS(status, 0, AQC_ERR_ARG); }   // IndexError upstream (:106-107)
            if (usable(cur)) qc_accumulate_read<true>(cur, ws, wq, QcLds{accs, gch, scal, cols}, kmer_len);
            cur = nxt;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cols; i += QC_BLOCK) {
        const int ci = (i & 3) * cq + (i >> 2);
        unsigned long long tn = 0, tq = 0;
#pragma unroll
        for (int row = 0; row < 5; ++row) {
            const unsigned int v = accs[row * cols + ci];
            const unsigned long long cnt = v >> 20, qs = (v & 0xfffffu) - 33ull * cnt;   // raw byte sum -> sum of qualNum (mod 2^64)
            if (row < 4 && v) {
                atomicAdd(&qc[(AQC_QC_BASE_COUNT_A + row) * AQC_QC_COLS + i], cnt);
                atomicAdd(&qc[(AQC_QC_BASE_QUAL_A + row) * AQC_QC_COLS + i], qs);
            }
            tn += cnt; tq += qs;
        }
        if (tn) {
            atomicAdd(&qc[AQC_QC_TOTAL_NUM * AQC_QC_COLS + i], tn);
            atomicAdd(&qc[AQC_QC_TOTAL_QUAL * AQC_QC_COLS + i], tq);
        }
        const unsigned int dv = accs[5 * cols + ci];
        if (dv) atomicAdd(&qc[AQC_QC_DISCONTINUITY * AQC_QC_COLS + i], (unsigned long long)dv);
        if (gch[i]) atomicAdd(&qc[AQC_QC_GC_HIST * AQC_QC_COLS + i], (unsigned long long)gch[i]);
    }
    if (threadIdx.x < 2 && scal[threadIdx.x]) atomicAdd(&qc[AQC_QC_SCALARS * AQC_QC_COLS + threadIdx.x], scal[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// k-mer dictionary of statRead (qualitycontrol.py:113-122), counting part.
// Global atomics top out near 3e10 /s on this chip — 28 M k-mers of a 200 k-read sample would cost ~0.9 ms —
// so the 4^k counters live in LDS: one 1024-thread workgroup per CU keeps a private table of 65536 u16 counters
// (128 KiB) and works in ROUNDS of at most 65535 k-mers (no counter can overflow), then streams the table to
// its own slice of `partial` with plain coalesced stores; kmer_reduce_kernel adds the slices up.  No global
// atomic is issued for a pure A/C/G/T k-mer except the (rare, load-guarded) first-seen minimum.
// A lane owns four consecutive k-mer start positions: its dword of bases is packed to 4 x 2-bit codes, two
// wave shifts assemble the codes of 16 consecutive bases, and the dense index of position j is
// (window >> 2j) & (4^k - 1) — base q of the k-mer at bits 2q..2q+1, code (c >> 1) & 3 = A0 C1 T2 G3.
// K-mers containing anything else go to the open-addressing table (byte keys).
// Descriptors are fetched lane-parallel and the bases of the next read are prefetched (see ReadDesc).
// ------------------------------------------------------------------------------------------------
#ifdef AQC_PROFILE
__device__ unsigned long long g_kprof[16];
#define KPROF_DECL unsigned long long kp_t[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long kp_last = __builtin_amdgcn_s_memtime();
#define KPROF(k) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); kp_t[k] += now_ - kp_last; kp_last = now_; } while (0)
#define KPROF_FLUSH do { if (lane == 0) for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&g_kprof[k_], kp_t[k_]); } while (0)
#else
#define KPROF_DECL
#define KPROF(k)
#define KPROF_FLUSH
#endif

constexpr int KMER_BLOCK = 1024;                // (round 6: 512 threads at <= 128 registers, to leave room for the writer's kernels beside it, measured slower —
                                                //  the step 3.90 - 3.95 -> 4.10 - 4.22 ms, the k-mer launches 0.265 -> 0.35 ms: profiles/r06_copy_window_grid.txt)
constexpr int KMER_WPB = KMER_BLOCK / WAVE;
constexpr int KMER_EXQ = 1536;                  // LDS queue of k-mers bound for the open-addressing table (24 KiB)
constexpr size_t KMER_LDS_BYTES = DENSE_ENTRIES * 2 + (size_t)KMER_EXQ * 16 + 16;
constexpr int KMER_FUSED_MAX_COLS = 256;         // widest QC accumulator block that still fits behind the table (160 KiB LDS)
constexpr size_t KMER_FUSED_LDS_BYTES = KMER_LDS_BYTES + sizeof(unsigned int) * (QC_LDS_ROWS + 1) * KMER_FUSED_MAX_COLS + 16;
constexpr int KMER_PASS_LANES = WAVE - 2;        // the last two lanes of a pass only supply bases to their neighbours

__global__ __launch_bounds__(KMER_BLOCK) void kmer_count_kernel(DevBatch b, int mate, uint64_t first, uint64_t count, int post,
                                                                const aqc_result* __restrict__ results, int kmer_len,
                                                                KmerTable kt, unsigned long long order_base,
                                                                uint16_t* __restrict__ partial, uint32_t reads_per_round,
                                                                uint32_t n_rounds, int* status,
                                                                unsigned long long* __restrict__ qc /* [QC_ROWS*QC_COLS] or null */,
                                                                int cols) {
    extern __shared__ __attribute__((aligned(16))) unsigned int ktab[];     // 32768 words = 65536 u16 counters
    unsigned long long* const exq_key = reinterpret_cast<unsigned long long*>(ktab + DENSE_ENTRIES / 2);   // parked exotic k-mers
    unsigned long long* const exq_t = exq_key + KMER_EXQ;
    unsigned int* const exq_n = reinterpret_cast<unsigned int*>(exq_t + KMER_EXQ);
    // fused mode (qc != null, reads <= 256 bases): the per-cycle accumulators of statRead ride along — same descriptor,
    // same dword of bases — in the LDS left over behind the k-mer table, and fill the issue slots this kernel idles in
    const bool fused = qc != nullptr;
    unsigned int* const q_accs = exq_n + 4;
    unsigned int* const q_gch = q_accs + QC_LDS_ROWS * cols;
    unsigned long long* const q_scal = reinterpret_cast<unsigned long long*>(q_gch + cols);
    const QcLds qlds{q_accs, q_gch, q_scal, cols};
    const int lane = lane_id();
    const int wave = threadIdx.x / WAVE;
    if (fused) {
        for (int i = threadIdx.x; i < (QC_LDS_ROWS + 1) * cols; i += KMER_BLOCK) q_accs[i] = 0;
        if (threadIdx.x < 2) q_scal[threadIdx.x] = 0;
    }
    const unsigned long long kmask = kmer_len >= 8 ? ~0ull : (1ull << (8 * kmer_len)) - 1ull;
    // k-mer with a symbol outside A/C/G/T -> open-addressing table, keyed by its bytes (first seen at time t)
    auto exotic_insert = [&](unsigned long long key, unsigned long long t) {
        unsigned long long rkey = 0;
        for (int qq = 0; qq < kmer_len; qq++)
            rkey |= (unsigned long long)comp_or_n((uint8_t)(key >> (8 * (kmer_len - 1 - qq)))) << (8 * qq);
        long long h, hr;
        kmer_slot2(kt, key, rkey, h, hr);
        if (h < 0 || hr < 0) atomicCAS(status, 0, AQC_ERR_UNSUPPORTED);
        else {
            // (the minima are load-guarded: after its first occurrence a k-mer costs one atomic, not three)
            const unsigned long long oa = kt.order[h], ob = kt.order[hr];
            atomicAdd(&kt.counts[h], 1ull);
            if (oa > 2 * t) atomicMin(&kt.order[h], 2 * t);
            if (ob > 2 * t + 1) atomicMin(&kt.order[hr], 2 * t + 1);
        }
    };
    const uint32_t imask = (1u << (2 * kmer_len)) - 1u, kbits = (1u << kmer_len) - 1u;
    unsigned long long* const my_first = kt.dense_first + (size_t)xcc_id() * DENSE_ENTRIES;
    auto usable = [&](const ReadDesc& d) { return d.len >= 5 && d.len <= AQC_MAX_READ_LEN && d.len > kmer_len; };
    // (a read whose quality view has a length of its own is left to qc_stat_kernel's only_irr pass: its per-cycle statistics, not its k-mers)
    auto qc_usable = [&](const ReadDesc& d) { return fused && d.len >= 5 && d.len <= AQC_MAX_READ_LEN && d.len <= cols && d.qlen == d.len; };
    KPROF_DECL
    // every dense k-mer already has a first-seen time from an earlier launch: nothing this launch sees can be earlier
    const bool complete = __syncthreads_and(threadIdx.x < (int)(DENSE_ENTRIES / KRED_ENTRIES) ? (int)kt.complete[threadIdx.x] : 1) != 0;
    constexpr uint32_t PAD = 0x41414141u;      // 'AAAA': bases beyond the read never reach a counted k-mer
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        for (int i = threadIdx.x; i < (int)(DENSE_ENTRIES / 2); i += KMER_BLOCK) ktab[i] = 0;
        if (threadIdx.x == 0) *exq_n = 0;
        __syncthreads();
        KPROF(0);
        const uint64_t r_lo = (uint64_t)round * reads_per_round;
        const uint64_t r_hi = min(r_lo + reads_per_round, count);
        for (uint64_t kb = r_lo + wave; kb < r_hi; kb += (uint64_t)KMER_WPB * WAVE) {
            const uint64_t myk = kb + (uint64_t)lane * KMER_WPB;
            // (the batch descriptor — twenty pointers — is read from the kernarg segment where it is used, once per 64 reads: held in
            //  scalar registers across the loop it was most of this kernel's SGPR spills)
#if defined(__HIP_DEVICE_COMPILE__)
            const DevBatch __attribute__((address_space(4)))* kb_args = (const DevBatch __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(kb_args));
            const DevBatch bb = *kb_args;              // (the batch descriptor is the kernel's first argument)
#else
            const DevBatch bb = b;
#endif
            const ReadDesc mine = lane_desc(bb, mate, first + myk, myk < r_hi, post, results);
            const int nr = (int)min((uint64_t)WAVE, (r_hi - kb + KMER_WPB - 1) / KMER_WPB);
            ReadDesc cur = bcast_desc(mine, 0);
            uint32_t pre = PAD, pre_q = 0;
            if (qc_usable(cur) || usable(cur)) {
                pre = load4(reinterpret_cast<const uint8_t*>(cur.s), 4 * lane, cur.len, PAD);
                if (fused) pre_q = load4(reinterpret_cast<const uint8_t*>(cur.q), 4 * lane, cur.qlen, 0);
            }
            KPROF(1);
            for (int r = 0; r < nr; ++r) {
                uint32_t ws = pre;
                const uint32_t wq0 = pre_q;
                ReadDesc nxt = cur;
                if (r + 1 < nr) {
                    nxt = bcast_desc(mine, r + 1);
                    if (qc_usable(nxt) || usable(nxt)) {
                        pre = load4(reinterpret_cast<const uint8_t*>(nxt.s), 4 * lane, nxt.len, PAD);
                        if (fused) pre_q = load4(reinterpret_cast<const uint8_t*>(nxt.q), 4 * lane, nxt.qlen, 0);
                    }
                }
                if (fused) {
                    const int len = cur.len;
                    if (len > AQC_MAX_READ_LEN || len > cols) { if (lane == 0) atomicCAS(status, 0, AQC_ERR_READ_TOO_LONG); }
                    else if (len < 5 && len > 0) { if (lane == 0) atomicCAS(status, 0, AQC_ERR_ARG); }   // IndexError upstream (:106-107)
                    if (qc_usable(cur)) {
                        // (the bases beyond the read are 'A' here, 0 in qc_stat_kernel: neither is ever looked at)
                        qc_accumulate_read<false>(cur, ws, wq0, qlds, kmer_len);
                    }
                }
                if (usable(cur)) {
                    const int len = cur.len;
                    const int nk = len - kmer_len;
                    const uint64_t k = kb + (uint64_t)r * KMER_WPB;
                    const unsigned long long t0 = (order_base + k) * (unsigned long long)AQC_QC_COLS;
                    for (int base0 = 0; base0 < nk; base0 += 4 * KMER_PASS_LANES) {
                        const int x = base0 + 4 * lane;
                        if (base0 > 0) ws = load4(reinterpret_cast<const uint8_t*>(cur.s), x, len, PAD);
                        uint32_t dq = 0;
                        apply_edits<false>(cur, x, ws, dq);                                           // (only the bases matter here)
                        const uint32_t codes = (ws >> 1) & 0x03030303u;
                        const uint32_t bad = __builtin_amdgcn_perm(0u, CODE_TO_BASE, codes) ^ ws;    // 0 where the byte is A/C/G/T
                        const uint32_t c8 = (codes | (codes >> 6) | (codes >> 12) | (codes >> 18)) & 0xffu;
                        const uint32_t c16 = c8 | ((uint32_t)__shfl_down(c8, 1) << 8);
                        const uint32_t win = c16 | ((uint32_t)__shfl_down(c16, 2) << 16);           // codes of bases x .. x+15
                        uint32_t badwin = 0;                                                         // bit q: base x+q is not A/C/G/T
                        if (__ballot(bad != 0u)) {
                            const uint32_t nz = nonzero_bytes(bad);
                            const uint32_t b4 = ((nz >> 7) | (nz >> 14) | (nz >> 21) | (nz >> 28)) & 0xfu;
                            const uint32_t b8 = b4 | ((uint32_t)__shfl_down(b4, 1) << 4);
                            badwin = b8 | ((uint32_t)__shfl_down(b8, 2) << 8);
                        }
                        KPROF(2);
                        uint32_t idx[4];
                        bool dense[4], exotic[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool act = lane < KMER_PASS_LANES && x + j < nk;
                            idx[j] = (win >> (2 * j)) & imask;
                            exotic[j] = act && ((badwin >> j) & kbits) != 0u;
                            dense[j] = act && !exotic[j];
                            if (dense[j]) atomicAdd(&ktab[idx[j] >> 1], 1u << (16 * (idx[j] & 1)));
                        }
                        KPROF(3);
                        if (!complete) {
                            unsigned long long seen[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) seen[j] = dense[j] ? my_first[idx[j]] : 0ull;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const unsigned long long t = t0 + (unsigned long long)(x + j);
                                if (dense[j] && seen[j] > t) __hip_atomic_fetch_min(&my_first[idx[j]], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                        KPROF(4);
                        if (__ballot(badwin != 0u)) {
                            // byte keys straight from registers: bases x .. x+11 = own dword + the next two lanes'.
                            // The table insert is a chain of global round trips, so it is not done here: the
                            // k-mer is parked in the workgroup's LDS queue and inserted when the round ends.
                            const uint32_t w1 = (uint32_t)__shfl_down(ws, 1), w2 = (uint32_t)__shfl_down(ws, 2);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                if (exotic[j]) {
                                    const uint32_t lo = __builtin_amdgcn_alignbit(w1, ws, 8 * j), hi = __builtin_amdgcn_alignbit(w2, w1, 8 * j);
                                    const unsigned long long key = (((unsigned long long)hi << 32) | lo) & kmask;
                                    const unsigned long long t = t0 + (unsigned long long)(x + j);
                                    const unsigned int slot = atomicAdd(exq_n, 1u);
                                    if (slot < (unsigned int)KMER_EXQ) { exq_key[slot] = key; exq_t[slot] = t; }
                                    else exotic_insert(key, t);                       // queue full: insert in place
                                }
                            }
                        }
                    }
                }
                KPROF(5);
                cur = nxt;
            }
        }
        __syncthreads();
        KPROF(6);
        {
            const unsigned int nq = min(*exq_n, (unsigned int)KMER_EXQ);
            for (unsigned int e = threadIdx.x; e < nq; e += KMER_BLOCK) exotic_insert(exq_key[e], exq_t[e]);
        }
        KPROF(5);
        uint4* dst = reinterpret_cast<uint4*>(partial + (size_t)round * DENSE_ENTRIES);
        const uint4* srcv = reinterpret_cast<const uint4*>(ktab);
        for (int i = threadIdx.x; i < (int)(DENSE_ENTRIES * 2 / 16); i += KMER_BLOCK) dst[i] = srcv[i];
        // the table and the queue may be reused once every wave has READ them out of LDS: wait for the LDS reads
        // only (lgkmcnt), not for the slice stores and table atomics still in flight — they drain under the next round
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_s_barrier();
        KPROF(7);
    }
    if (fused) {
        __syncthreads();
        const int cq = cols >> 2;
        for (int i = threadIdx.x; i < cols; i += KMER_BLOCK) {
            const int ci = (i & 3) * cq + (i >> 2);
            unsigned long long tn = 0, tq = 0;
#pragma unroll
            for (int row = 0; row < 5; ++row) {
                const unsigned int v = q_accs[row * cols + ci];
                const unsigned long long cnt = v >> 20, qs = (v & 0xfffffu) - 33ull * cnt;   // raw byte sum -> sum of qualNum (mod 2^64)
                if (row < 4 && v) {
                    atomicAdd(&qc[(AQC_QC_BASE_COUNT_A + row) * AQC_QC_COLS + i], cnt);
                    atomicAdd(&qc[(AQC_QC_BASE_QUAL_A + row) * AQC_QC_COLS + i], qs);
                }
                tn += cnt; tq += qs;
            }
            if (tn) {
                atomicAdd(&qc[AQC_QC_TOTAL_NUM * AQC_QC_COLS + i], tn);
                atomicAdd(&qc[AQC_QC_TOTAL_QUAL * AQC_QC_COLS + i], tq);
            }
            const unsigned int dv = q_accs[5 * cols + ci];
            if (dv) atomicAdd(&qc[AQC_QC_DISCONTINUITY * AQC_QC_COLS + i], (unsigned long long)dv);
            if (q_gch[i]) atomicAdd(&qc[AQC_QC_GC_HIST * AQC_QC_COLS + i], (unsigned long long)q_gch[i]);
        }
        if (threadIdx.x < 2 && q_scal[threadIdx.x]) atomicAdd(&qc[AQC_QC_SCALARS * AQC_QC_COLS + threadIdx.x], q_scal[threadIdx.x]);
    }
    KPROF_FLUSH;
}

// dense_count[XCD 0 copy][idx] += sum over rounds of partial[round][idx]
// A workgroup owns 256 adjacent entries; its four waves take every fourth round each, a lane adds four entries
// (one 8-byte load per round, 512 contiguous bytes per wave) and the four partial sums meet in LDS.
__global__ __launch_bounds__(KRED_BLOCK) void kmer_reduce_kernel(const uint16_t* __restrict__ partial, uint32_t n_rounds,
                                                                 KmerTable kt, int kmer_len) {
    __shared__ unsigned int part[4][KRED_ENTRIES];
    const int quad = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const uint32_t e0 = blockIdx.x * KRED_ENTRIES + 4 * quad;
    unsigned int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll 8
    for (uint32_t r = grp; r < n_rounds; r += 4) {
        const uint2 v = *reinterpret_cast<const uint2*>(partial + (size_t)r * DENSE_ENTRIES + e0);
        s0 += v.x & 0xffffu; s1 += v.x >> 16; s2 += v.y & 0xffffu; s3 += v.y >> 16;
    }
    part[grp][4 * quad + 0] = s0; part[grp][4 * quad + 1] = s1; part[grp][4 * quad + 2] = s2; part[grp][4 * quad + 3] = s3;
    __syncthreads();
    const int i = threadIdx.x;
    const uint32_t idx = blockIdx.x * KRED_ENTRIES + i;
    kt.dense_count[idx] += part[0][i] + part[1][i] + part[2][i] + part[3][i];
    // does every entry of this workgroup have a first-seen time by now (in any XCD's copy)?
    bool seen = idx >= (1u << (2 * kmer_len));
    if (!kt.complete[blockIdx.x]) {
        for (int x = 0; x < N_XCD && !seen; ++x) seen = kt.dense_first[(size_t)x * DENSE_ENTRIES + idx] != ~0ull;
        const int all = __syncthreads_and(seen ? 1 : 0);
        if (threadIdx.x == 0 && all) kt.complete[blockIdx.x] = 1u;
    }
}

// compact the occupied k-mer slots into dense arrays (i = mask + 1: the all-NUL k-mer's entry, present once its order is set)
__global__ void kmer_compact_kernel(KmerTable kt, unsigned long long* keys, unsigned long long* counts,
                                    unsigned long long* order, unsigned long long cap, unsigned long long* n_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > kt.mask + 1) return;
    const unsigned long long key = i > kt.mask ? 0ull : kt.keys[i];
    if (i > kt.mask ? kt.order[i] == ~0ull : key == 0) return;
    const unsigned long long w = atomicAdd(n_out, 1ull);
    if (w < cap) { keys[w] = key; counts[w] = kt.counts[i]; order[w] = kt.order[i]; }
}

// ... and the dense A/C/G/T table: k-mer X is in the dictionary iff X or its reverse complement was scanned;
// its insertion rank is min(2 * first(X), 2 * first(rc X) + 1) (qualitycontrol.py:116-122)
__global__ void kmer_compact_dense_kernel(KmerTable kt, int k, unsigned long long* keys, unsigned long long* counts,
                                          unsigned long long* order, unsigned long long cap, unsigned long long* n_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << (2 * k))) return;
    const unsigned long long never = ~0ull;
    unsigned long long f = never, fr = never, cnt = 0;
    const uint32_t ir = dense_rc(i, k);
    for (int x = 0; x < N_XCD; ++x) {
        const unsigned long long a = kt.dense_first[(size_t)x * DENSE_ENTRIES + i], b = kt.dense_first[(size_t)x * DENSE_ENTRIES + ir];
        f = a < f ? a : f;
        fr = b < fr ? b : fr;
        cnt += kt.dense_count[(size_t)x * DENSE_ENTRIES + i];
    }
    if (f == never && fr == never) return;
    unsigned long long ord = never;
    if (f != never) ord = 2 * f;
    if (fr != never && 2 * fr + 1 < ord) ord = 2 * fr + 1;
    unsigned long long key = 0;
    for (int j = 0; j < k; ++j) {
        const uint32_t code = (i >> (2 * j)) & 3u;
        key |= (unsigned long long)((CODE_TO_BASE >> (8 * code)) & 0xffu) << (8 * j);
    }
    const unsigned long long w = atomicAdd(n_out, 1ull);
    if (w < cap) { keys[w] = key; counts[w] = cnt; order[w] = ord; }
}

}  // namespace aqc
