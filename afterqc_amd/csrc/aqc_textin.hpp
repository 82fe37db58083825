// aqc_textin.hpp — FASTQ text in, on the device: the line index, record framing, Illumina name parsing.
//
//   framing    fastq.Reader.nextRead (fastq.py:37-49): a record is 4 lines, each `readline().rstrip()`; a line
//              that is empty after stripping ends the file.  The raw text chunk is the byte arena; the kernels
//              here find the newlines, strip trailing whitespace and emit (offset, length) per line.
//
// All of it is byte shuffling bound by HBM bandwidth; no data-dependent host work remains per record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aqc_prim.hpp"       // WAVE, lane_id, the DPP wave sum and lane scan of the index pass
#include "aqc_batch.hpp"      // the marks in a framed chunk's length words: LEN_IRR, LEN_MASK, QLEN_MASK, QLEN_TAILNL, QLEN_CONTIG

namespace aqc {

constexpr int TXT_BLOCK = 256;

// ---- line index of a text chunk in ONE pass over the bytes ----------------------------------------------------------
// line_end[i] = byte position of the i-th '\n' (bit 31: the byte before it is a blank or control character, i.e. the
// line MAY end in whitespace that readline().rstrip() removes — the framing kernel looks at the text only then).
// Tiles of 32 KiB are claimed in arrival order (ticket) and chained with a decoupled look-back: a tile publishes its
// newline count (flag A), adds up its predecessors' counts until it meets one that already knows its inclusive prefix
// (flag P), publishes its own prefix and emits.  The text is read once; the old count / scan / emit trio read it twice
// and needed three launches per file.
constexpr int IDX_K = 8;                              // 16-byte pieces a lane loads at a time (one sub-tile)
constexpr int IDX_SUB = 4;                            // sub-tiles per tile
constexpr int IDX_P = IDX_K * IDX_SUB;                // pieces per lane per tile
constexpr int IDX_TILE = TXT_BLOCK * 16 * IDX_P;      // 128 KiB: one ticket and one look-back per tile (same-address atomics
                                                      // serialise in L2 at ~8 ns each, so 32 KiB tiles capped the kernel near 4 TB/s)
constexpr unsigned long long IDX_FLAG_A = 1ull << 62, IDX_FLAG_P = 2ull << 62, IDX_VAL = (1ull << 62) - 1ull;
constexpr uint32_t LINE_WS = 0x80000000u, LINE_POS = 0x7fffffffu;

struct IndexFile {
    const uint8_t* text;
    uint64_t bytes;
    uint32_t* line_end;
    uint64_t cap;              // entries line_end can take (more are counted, not written)
    unsigned long long* total; // out: number of '\n' in the chunk
    uint32_t tile0, tiles;     // this file's tiles are [tile0, tile0 + tiles) of the launch
};

// newline flags and "< 0x21" flags of the 16 bytes of v, one bit per byte
__device__ __forceinline__ void piece_masks(const uint4 v, uint32_t& nl16, uint32_t& bl16) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t zb[4], zn[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t t = (w[d] & 0x7f7f7f7fu) + 0x5f5f5f5fu;                            // bit 7 where the low 7 bits are >= 0x21
        zb[d] = ~(t | w[d]) & 0x80808080u;                                                 // 0x80 where the byte is < 0x21
        // '\n' is one of those bytes, and they all have bit 7 clear: byte ^ 0x0a is zero iff adding 0x7f does not reach bit 7
        const uint32_t x = w[d] ^ 0x0a0a0a0au;
        zn[d] = ~((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) & zb[d];                          // 0x80 where the byte is '\n'
    }
    // gather the bit 7s: dot products with weights 1, 2, 4, ... (0x80 * mask), two words per chain
    const uint32_t n_lo = __builtin_amdgcn_udot4(zn[1], 0x80402010u, __builtin_amdgcn_udot4(zn[0], 0x08040201u, 0u, false), false);
    const uint32_t n_hi = __builtin_amdgcn_udot4(zn[3], 0x80402010u, __builtin_amdgcn_udot4(zn[2], 0x08040201u, 0u, false), false);
    const uint32_t b_lo = __builtin_amdgcn_udot4(zb[1], 0x80402010u, __builtin_amdgcn_udot4(zb[0], 0x08040201u, 0u, false), false);
    const uint32_t b_hi = __builtin_amdgcn_udot4(zb[3], 0x80402010u, __builtin_amdgcn_udot4(zb[2], 0x08040201u, 0u, false), false);
    nl16 = (n_lo >> 7) | (n_hi << 1);
    bl16 = (b_lo >> 7) | (b_hi << 1);
}

// Layout inside a tile: a wave owns IDX_SUB * 8 KiB; its lane i reads the 16-byte pieces at  wave base + p * 1024 + i * 16,
// p = 0..IDX_P-1, eight at a time — every load instruction of the wave is one contiguous KiB (the earlier "contiguous bytes
// per thread" made each instruction touch 64 different cache lines and ran at 2.3 TB/s whatever the arithmetic cost).  The
// text order of the pieces is (p, lane), so the rank of a piece's first newline is  tile prefix + waves before + pieces
// (p' < p) + lanes before within p.  Between the load and the emit only the 16-bit newline / blank masks of a piece are
// kept, in LDS (32 KiB per workgroup); the emit pass rebuilds the lane ranks from them with one packed lane scan per two
// pieces.  Both passes are rolled loops: fully unrolled, the compiler kept the whole tile's state live (300 registers).
__global__ __launch_bounds__(TXT_BLOCK) void text_index_kernel(IndexFile f0, IndexFile f1, unsigned long long* __restrict__ state,
                                                               unsigned int* __restrict__ ticket) {
    __shared__ unsigned int s_tile;
    __shared__ unsigned int s_wave_tot[TXT_BLOCK / WAVE];
    __shared__ unsigned long long s_base;
    __shared__ uint32_t s_nl[IDX_P / 2][TXT_BLOCK], s_ws[IDX_P / 2][TXT_BLOCK];     // two pieces per word
    if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const IndexFile& f = tile >= f1.tile0 && f1.tiles ? f1 : f0;
    const uint32_t lt = tile - f.tile0;                                   // tile within the file
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const uint64_t wbase = (uint64_t)lt * IDX_TILE + (uint64_t)wave * (WAVE * 16 * IDX_P);
    const uint64_t lbase = wbase + (uint64_t)lane * 16;
    // (the buffer is zero-filled for more than a tile behind the text; loads are still bounded by the text's end)
    // (round 6: a wave whose 32 KiB lie inside the text — all but a file's last — loads and masks without looking at the text's end;
    //  "the byte before is blank" comes from a ballot of the lanes' last bytes instead of a lane shift through LDS; the lane scans
    //  of the emit pass are DPP scans: 146 -> ~115 instructions per 16 bytes of an instruction-bound kernel)
    const bool full = wbase + (uint64_t)(WAVE * 16 * IDX_P) <= f.bytes;          // (wave-uniform)
    uint32_t carry_in = (wbase > 0 && wbase <= f.bytes) ? (f.text[wbase - 1] < 0x21 ? 1u : 0u) : 0u;      // (wave-uniform too)
    uint32_t mine = 0;                            // newlines in this lane's pieces
    uint4 v[IDX_K];
    auto load_piece = [&](int p) -> uint4 {
        const uint64_t q = lbase + (uint64_t)p * (WAVE * 16);
        if (full) return *reinterpret_cast<const uint4*>(f.text + q);
        return q < f.bytes ? *reinterpret_cast<const uint4*>(f.text + q) : make_uint4(0, 0, 0, 0);
    };
#pragma unroll
    for (int k = 0; k < IDX_K; ++k) v[k] = load_piece(k);
#pragma unroll 1
    for (int sub = 0; sub < IDX_SUB; ++sub) {
        uint4 nx[IDX_K];
#pragma unroll
        for (int k = 0; k < IDX_K; ++k)          // the next sub-tile is on its way while this one is worked on
            nx[k] = sub + 1 < IDX_SUB ? load_piece((sub + 1) * IDX_K + k) : make_uint4(0, 0, 0, 0);
        uint32_t nlp = 0, wsp = 0;
#pragma unroll
        for (int k = 0; k < IDX_K; ++k) {
            const int p = sub * IDX_K + k;
            uint32_t nl, bl;
            piece_masks(v[k], nl, bl);
            // mask the bytes behind the end of the text (the last piece may be partial)
            if (!full) {
                const uint64_t q = lbase + (uint64_t)p * (WAVE * 16);
                if (q + 16 > f.bytes) { const uint32_t keep = q >= f.bytes ? 0u : ((1u << (f.bytes - q)) - 1u); nl &= keep; }
            }
            // "the byte before is blank": this piece's flags moved up one byte; the byte before the piece is the last byte
            // of the piece of the lane before (same p), for lane 0 of the last lane's piece of p - 1
            const unsigned long long tops = __ballot((bl >> 15) != 0u);
            const uint32_t prev = (uint32_t)((((tops << 1) | carry_in) >> lane) & 1ull);
            carry_in = (uint32_t)(tops >> (WAVE - 1));
            const uint32_t ws = ((bl << 1) | prev) & 0xffffu;
            mine += (uint32_t)__popc(nl);
            if (k & 1) {
                s_nl[p / 2][threadIdx.x] = nlp | (nl << 16);
                s_ws[p / 2][threadIdx.x] = wsp | (ws << 16);
            } else { nlp = nl; wsp = ws; }
        }
#pragma unroll
        for (int k = 0; k < IDX_K; ++k) v[k] = nx[k];
    }
    const uint32_t wtot = (uint32_t)wave_sum_dpp((int)mine);
    if (lane == 0) s_wave_tot[wave] = wtot;
    __syncthreads();
    unsigned long long total = 0, wave_off = 0;
#pragma unroll
    for (int w = 0; w < TXT_BLOCK / WAVE; ++w) {
        if (w < wave) wave_off += s_wave_tot[w];
        total += s_wave_tot[w];
    }
    if (threadIdx.x < WAVE) {
        unsigned long long base = 0;
        if (lt == 0) {
            if (lane == 0) __hip_atomic_store(&state[tile], IDX_FLAG_P | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(&state[tile], IDX_FLAG_A | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            long long j = (long long)tile - 1;                            // look back from the predecessor
            const long long first = (long long)f.tile0;
            while (true) {
                const long long idx = j - lane;
                unsigned long long sv = IDX_FLAG_P;                       // before the file's first tile: prefix 0
                if (idx >= first) sv = __hip_atomic_load(&state[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned int flag = (unsigned int)(sv >> 62);
                const unsigned long long pend = __ballot(flag == 0), pfx = __ballot(flag == 2);
                if (pfx) {
                    const int fp = __ffsll((long long)pfx) - 1;
                    const unsigned long long upto = fp == 63 ? ~0ull : ((2ull << fp) - 1ull);
                    if (pend & upto) { __builtin_amdgcn_s_sleep(1); continue; }
                    unsigned long long part = lane <= fp ? (sv & IDX_VAL) : 0ull;
#pragma unroll
                    for (int sft = 32; sft > 0; sft >>= 1) part += __shfl_xor(part, sft, WAVE);
                    base += part;
                    break;
                }
                if (pend) { __builtin_amdgcn_s_sleep(1); continue; }
                unsigned long long part = sv & IDX_VAL;
#pragma unroll
                for (int sft = 32; sft > 0; sft >>= 1) part += __shfl_xor(part, sft, WAVE);
                base += part;
                j -= WAVE;
            }
            if (lane == 0) __hip_atomic_store(&state[tile], IDX_FLAG_P | (base + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            s_base = base;
            if (lt + 1 == f.tiles) *f.total = base + total;
        }
    }
    __syncthreads();
    unsigned long long run = s_base + wave_off;      // rank of the first newline of the wave's pieces in row p (wave-uniform)
#pragma unroll 2
    for (int j = 0; j < IDX_P / 2; ++j) {
        const uint32_t nlp = s_nl[j][threadIdx.x], wsp = s_ws[j][threadIdx.x];
        const uint32_t own = (uint32_t)__popc(nlp & 0xffffu) | ((uint32_t)__popc(nlp >> 16) << 16);
        const uint32_t c = (uint32_t)wave_incl_sum((int)own, lane);      // inclusive lane scan, two rows at once (each < 2^11)
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)c, WAVE - 1);
        const uint32_t ex = c - own;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t m = h ? (nlp >> 16) : (nlp & 0xffffu);
            const uint32_t ws = h ? (wsp >> 16) : (wsp & 0xffffu);
            unsigned long long i = run + (h ? (ex >> 16) : (ex & 0xffffu));
            const uint32_t q = (uint32_t)lbase + (uint32_t)(2 * j + h) * (WAVE * 16);      // (chunks are < 2 GiB)
            // (a lane's 16 bytes hold at most two line ends but for one-base lines: two predicated stores, then the loop for the rest)
            if (m) {
                const int bit = __builtin_ctz(m);
                if (i < f.cap) f.line_end[i] = (q + (uint32_t)bit) | (((ws >> bit) & 1u) ? LINE_WS : 0u);
                m &= m - 1;
                if (m) {
                    const int bit2 = __builtin_ctz(m);
                    if (i + 1 < f.cap) f.line_end[i + 1] = (q + (uint32_t)bit2) | (((ws >> bit2) & 1u) ? LINE_WS : 0u);
                    m &= m - 1;
                }
                i += 2;
            }
            if (__ballot(m != 0u)) {
                while (m) {
                    const int bit = __builtin_ctz(m);
                    if (i < f.cap) f.line_end[i] = (q + (uint32_t)bit) | (((ws >> bit) & 1u) ? LINE_WS : 0u);
                    ++i;
                    m &= m - 1;
                }
            }
            run += h ? (last >> 16) : (last & 0xffffu);
        }
    }
}

// the whitespace bytes.rstrip() removes: space, \t \n \v \f \r
__device__ __forceinline__ bool is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

struct FrameMeta {
    unsigned int first_empty;   // first record with an empty line (0xffffffff = none)
    unsigned int max_len;       // longest sequence line
    unsigned int first_mismatch; // first record whose quality line is not as long as its sequence line
    unsigned int pad_;
};

// the four lines of every complete group of the chunk (fastq.py:37-49); thread per record
struct FramedFile {
    uint32_t* seq_off;
    uint32_t* qual_off;
    uint32_t* seq_len;
    uint32_t* name_off;
    uint32_t* name_len;
    uint32_t* plus_off;
    uint32_t* plus_len;
    uint32_t* qual_len;      // QLEN_TAILNL: the byte behind the (stripped) quality line is its '\n'; QLEN_CONTIG: that holds for all four lines
};

// (the number of lines comes from the index pass's device-side total: nothing of it goes through the host first.  virt_end != 0:
//  the file's unterminated last line ends at this virtual line end — readline() returns it — which is line number *d_total)
__global__ __launch_bounds__(TXT_BLOCK) void frame_records_kernel(const uint8_t* __restrict__ text,
                                                                  const uint32_t* __restrict__ line_end, const unsigned long long* __restrict__ d_total,
                                                                  uint32_t virt_end, FramedFile out, FrameMeta* __restrict__ meta, uint64_t cap) {
    // (`cap`: entries the line table holds.  The index pass COUNTS every line and writes the first `cap`: when a chunk of very
    //  short lines overflows the table the host indexes it again with the exact size — until then nothing beyond the table may
    //  be read, and no record beyond it written: the output arrays are sized for cap / 4 records — round-4 advisory)
    const uint64_t real = *d_total < cap ? *d_total : cap;
    const uint64_t n_rec = (real + ((virt_end && *d_total <= cap) ? 1u : 0u)) / 4;
    if ((uint64_t)blockIdx.x * TXT_BLOCK >= n_rec) return;          // (the grid is sized for the most lines the chunk could hold)
    const uint64_t r = (uint64_t)blockIdx.x * TXT_BLOCK + threadIdx.x;
    const bool in = r < n_rec;
    const int lane = lane_id();
    // the record's four line ends in one 16-byte load; the end of the line before it is the neighbour lane's fourth
    uint4 le4 = make_uint4(0, 0, 0, 0);
    if (in) {
        le4 = reinterpret_cast<const uint4*>(line_end)[r];
        if (virt_end && 4 * r + 3 == real && *d_total <= cap) le4.w = virt_end;         // (a virtual line can only be the last line of the last record)
    }
    uint32_t before = (uint32_t)__shfl_up((int)le4.w, 1, WAVE);
    if (lane == 0) before = (in && r > 0) ? line_end[4 * r - 1] : 0u;
    const uint32_t le[4] = {le4.x, le4.y, le4.z, le4.w};
    uint32_t s[4] = {0, 0, 0, 0}, l[4] = {1, 1, 1, 1};
    uint32_t tail_nl = 0;                                   // the quality line ends right at its '\n' (nothing stripped)
    bool all_nl = true;                                     // ... and so do the other three lines
    if (in) {
        uint32_t b = r == 0 ? 0u : (before & LINE_POS) + 1u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t e = le[k] & LINE_POS;
            const uint32_t nl_at = e;
            bool at_nl = true;
            if (le[k] & LINE_WS) {                          // only lines that may end in whitespace touch the text
                while (e > b && is_space(text[e - 1])) --e;
                at_nl = e == nl_at && text[nl_at] == '\n';   // (the file's unterminated last line ends at a virtual '\n')
            }
            s[k] = b;
            l[k] = e - b;
            all_nl = all_nl && at_nl;
            if (k == 3) tail_nl = at_nl ? QLEN_TAILNL : 0u;
            b = nl_at + 1u;
        }
        out.name_off[r] = s[0]; out.name_len[r] = l[0];
        // a quality line of another length than its sequence line: the reference does not mind (fastq.py:37-49 hands the lines
        // over as they are) — the record is marked, every later stage keeps a view per string (aqc_batch.hpp, LEN_IRR)
        out.seq_off[r] = s[1];  out.seq_len[r] = l[1] | (l[1] != l[3] ? LEN_IRR : 0u);
        out.plus_off[r] = s[2]; out.plus_len[r] = l[2] | (l[1] != l[3] ? LEN_IRR : 0u);      // (the mark once more, where the writer's sizing pass reads anyway)
        out.qual_off[r] = s[3]; out.qual_len[r] = min(l[3], QLEN_MASK) | tail_nl | (all_nl ? QLEN_CONTIG : 0u);
    }
    // chunk-wide reductions: at most one atomic per workgroup and only when it has something to say.  (Same-address
    // atomics serialise in L2 at ~8 ns each; the running maximum is read with an L2-coherent load — a plain load is served
    // from the CU's L1, which kept saying 0 for most of the kernel and let nearly every wave through to the atomic.)
    __shared__ unsigned int s_mx[TXT_BLOCK / WAVE];
    const bool empty = in && (l[0] == 0 || l[1] == 0 || l[2] == 0 || l[3] == 0);
    const bool mism = in && !empty && l[1] != l[3];
    const unsigned long long be = __ballot(empty), bm = __ballot(mism);
    unsigned int mx = in ? l[1] : 0u;
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, sft, WAVE));
    if (lane == 0) {
        const uint64_t rw = r;                                     // first record of this wave
        if (be) atomicMin(&meta->first_empty, (unsigned int)(rw + (uint64_t)__builtin_ctzll(be)));
        if (bm) atomicMin(&meta->first_mismatch, (unsigned int)(rw + (uint64_t)__builtin_ctzll(bm)));
        s_mx[threadIdx.x / WAVE] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TXT_BLOCK / WAVE; ++w) mx = max(mx, s_mx[w]);
        if (mx > __hip_atomic_load(&meta->max_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&meta->max_len, mx);
    }
}

// What aqc_frame reports, worked out on the device behind the framing kernels (one thread): the lock-step record count of
// preprocesser.py:412-429, the bytes the n records take, R1's next sequence length.  The host reads it with ONE copy and ONE wait
// per chunk (rounds 1 - 3: three round trips — line totals, frame meta, tail values).
struct FrameOut {
    unsigned long long n, avail[2], lines[2], consumed[2];
    unsigned int eof[2], first_mismatch[2], max_len, next_len1;
};

__global__ void frame_finish_kernel(const unsigned long long* __restrict__ d_total, const FrameMeta* __restrict__ meta, const uint32_t* __restrict__ line_end0,
                                    const uint32_t* __restrict__ line_end1, const uint32_t* __restrict__ seq_len0, uint32_t virt0, uint32_t virt1,
                                    unsigned long long bytes0, unsigned long long bytes1, int nf, unsigned long long max_records, FrameOut* __restrict__ out,
                                    unsigned long long cap0, unsigned long long cap1) {
    const unsigned long long cap[2] = {cap0, cap1};
    const uint32_t* const le[2] = {line_end0, line_end1};
    const uint32_t virt[2] = {virt0, virt1};
    const unsigned long long bytes[2] = {bytes0, bytes1};
    FrameOut o{};
    unsigned long long nrec[2] = {0, 0};
    for (int k = 0; k < nf; ++k) {
        o.lines[k] = d_total[k] + (virt[k] ? 1u : 0u);
        // (a table that overflowed: the host sees lines > cap and frames the chunk again; what is reported until then stays inside it)
        nrec[k] = (d_total[k] <= cap[k] ? o.lines[k] : cap[k]) / 4;
        o.avail[k] = meta[k].first_empty < nrec[k] ? meta[k].first_empty : nrec[k];
        o.eof[k] = meta[k].first_empty < nrec[k] ? 1u : 0u;
        o.first_mismatch[k] = meta[k].first_mismatch;
        o.max_len = meta[k].max_len > o.max_len ? meta[k].max_len : o.max_len;
    }
    unsigned long long n = o.avail[0];
    if (nf == 2 && o.avail[1] < n) n = o.avail[1];
    if (max_records < n) n = max_records;
    o.n = n;
    for (int k = 0; k < nf; ++k) {
        if (!n) continue;
        const unsigned long long i = 4 * n - 1;
        const uint32_t e = (virt[k] && i == d_total[k]) ? virt[k] : le[k][i];
        const unsigned long long end = (unsigned long long)(e & LINE_POS) + 1;
        o.consumed[k] = end < bytes[k] ? end : bytes[k];
    }
    o.next_len1 = o.avail[0] > n ? (seq_len0[n] & LEN_MASK) : 0u;
    *out = o;
}

// ---- Illumina read names for the bubble filter (preprocesser.py:155,176-192) ---------------------------------------
// re.search(r'\S+\:\d+\:\S+\:\d+\:\d+\:\d+\:\d+', name), then items = match.split(':'), lane = int(items[3]),
// tile = int(items[4][1:]), x = int(items[5]), y = int(items[6]).  The search is reproduced with the regex engine's
// own order: leftmost start; first \S+ greedy (longest first, backing off to the previous ':'); \d+ runs are maximal
// (a shorter run is followed by a digit, never by ':'); second \S+ greedy.  ok = 0 no match, 1 parsed, 2 the
// reference would raise (a non-numeric items[k], e.g. more than seven fields, or an empty items[4][1:]) — the
// kernels turn 2 into AQC_ERR_ARG only if the record actually reaches the bubble stage, like the exception upstream.
__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// int() of name[a:b) as CPython 3 — the interpreter the golden vectors were recorded with — reads a field that holds no blanks: an
// optional sign, then digits with single underscores between them ("+5", "-5", "1_0", "007"); returns false for anything else;
// values beyond int32 saturate and set `big` (such a coordinate is outside every circle; such a lane or tile is no circle's, but
// its saturated value may be one's: the caller must not compare it)
__device__ __forceinline__ bool parse_int(const uint8_t* name, int a, int b, int32_t& out, bool& big) {
    if (b <= a) return false;
    const bool neg = name[a] == '-';
    if (neg || name[a] == '+') ++a;
    unsigned long long v = 0;
    bool after_digit = false;                         // an underscore stands between two digits
    for (int i = a; i < b; ++i) {
        if (name[i] == '_' && after_digit) { after_digit = false; continue; }
        if (!is_digit(name[i])) return false;
        after_digit = true;
        v = v * 10ull + (unsigned long long)(name[i] - '0');
        if (v > 0x7fffffffull) { v = 0x7fffffffull; big = true; }
    }
    if (!after_digit) return false;                   // nothing behind the sign, or an underscore at the end
    out = neg ? -(int32_t)v : (int32_t)v;
    return true;
}

__global__ __launch_bounds__(TXT_BLOCK) void parse_names_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ name_off,
                                                                const uint32_t* __restrict__ name_len, const unsigned long long* __restrict__ n_dev,
                                                                int32_t* __restrict__ lane_out, int32_t* __restrict__ tile_out,
                                                                int32_t* __restrict__ x_out, int32_t* __restrict__ y_out,
                                                                uint8_t* __restrict__ ok_out) {
    const uint64_t r = (uint64_t)blockIdx.x * TXT_BLOCK + threadIdx.x;
    if (r >= *n_dev) return;                              // (FrameOut::n: the grid is sized for the most records the chunk could hold)
    const uint8_t* name = text + name_off[r];
    const int len = (int)name_len[r];
    int m_s = -1, m_e = -1;
    for (int s = 0; s < len && m_s < 0; ++s) {
        if (is_space(name[s])) continue;
        int E = s;
        while (E < len && !is_space(name[E])) ++E;           // the match stays inside this blank-delimited token
        for (int e1 = E - 1; e1 > s && m_s < 0; --e1) {
            if (name[e1] != ':') continue;
            int p = e1 + 1;
            while (p < E && is_digit(name[p])) ++p;
            if (p == e1 + 1 || p >= E || name[p] != ':') continue;
            const int s3 = p + 1;
            for (int e3 = E - 1; e3 > s3 && m_s < 0; --e3) {
                if (name[e3] != ':') continue;
                int q = e3 + 1;
                bool good = true;
                for (int g = 0; g < 3 && good; ++g) {
                    const int a = q;
                    while (q < E && is_digit(name[q])) ++q;
                    if (q == a || q >= E || name[q] != ':') good = false;
                    else ++q;
                }
                if (good) {
                    const int a = q;
                    while (q < E && is_digit(name[q])) ++q;
                    if (q > a) { m_s = s; m_e = q; }
                }
            }
        }
    }
    int32_t lane = 0, tile = 0, x = 0, y = 0;
    uint8_t ok = 0;
    if (m_s >= 0) {
        // items = match.split(':') : the 4th..7th field from the LEFT
        int fs[8], fe[8], nf = 0, a = m_s;
        for (int i = m_s; i <= m_e && nf < 8; ++i) {
            if (i == m_e || name[i] == ':') { fs[nf] = a; fe[nf] = i; ++nf; a = i + 1; }
        }
        // (all four fields are converted before any is used: one that int() rejects raises whatever the others hold)
        bool big_id = false, big_xy = false;
        const bool p3 = parse_int(name, fs[3], fe[3], lane, big_id), p4 = parse_int(name, fs[4] + 1, fe[4], tile, big_id);
        const bool p5 = parse_int(name, fs[5], fe[5], x, big_xy), p6 = parse_int(name, fs[6], fe[6], y, big_xy);      // (saturated: outside)
        ok = !(p3 && p4 && p5 && p6) ? 2 : big_id ? 0 : 1;          // a lane or tile beyond int32 is in no circle: as good as no match
    }
    lane_out[r] = lane; tile_out[r] = tile; x_out[r] = x; y_out[r] = y; ok_out[r] = ok;
}

}  // namespace aqc
