// aqc_fmtcopy.hpp — FASTQ text out, on the device: the writers.  They place every record of a chunk in its
// output stream and copy its pieces there; what a record is made of and how big it is comes from aqc_fmt.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"      // AQC_GOOD and the edit kinds of the correction walk
#include "aqc_prim.hpp"       // WAVE, lane_id, gload_* / gstore_*, load16u / store16u, wave_incl_sum, block_excl_scan
#include "aqc_batch.hpp"      // the marks in a framed chunk's length words: LEN_IRR, LEN_MASK, QLEN_CONTIG
#include "aqc_fmt.hpp"        // the format model: FormatView, fmt_sizes, FmtTask, fmt_build, FormatOut, the FMT_* tile sizes
#include "aqc_fmtwin.hpp"     // the forward copies' arithmetic: plan_words, the plan decode and the window rules (FMTW_*)
#include "aqc_revcopy.hpp"    // the reversed 16-byte windows of the merged-read pass

namespace aqc {

// ---- the writer: plan, then copy ------------------------------------------------------------------------------------------
// fmt_plan_kernel (thread = record, workgroup = tile of FMT_TILE records): the record's offset in its stream (block scans
// over the sizes, tile bases from fmt_tile_bases_kernel) and its piece list, written as a PLAN of six 16-byte words per
// (record, file):
//     q0  offset in the stream | stream, piece count, patch count | source of piece 0 | lengths of pieces 0, 1
//     q1  sources of pieces 1..4          q2  sources of pieces 5..7 | lengths of pieces 2, 3
//     q3  lengths of pieces 4..7 | cumulative work items of pieces 0..7 (a byte each)
//     q4  output offsets of pieces 1..7 (16 bits each) | total work items      q5  up to four byte patches (position | byte << 16)
// The search a copy lane would otherwise repeat (which piece is my work item in, where does that piece start in the
// output) is done here once per record.  Records with more than eight pieces / four patches / 32 work items keep their
// full FmtTask in an overflow array (q0.y bit 31).  A record that goes out as ONE piece — its own bytes — needs q0 only.
// fmt_copy_whole_kernel takes those, fmt_copy_kernel everything else (listed by the plan kernel).
constexpr unsigned int GEN_LISTS = 256;      // lists of "general" records (capacity gen_cap each), see fmt_plan_kernel
// (PLAN_SKIP, PLAN_OVER, PLAN_Q, PLAN_MAXP, GEN_PASSES, plan_is_whole — the plans fmt_copy_whole_kernel takes — and plan_words, which
//  packs a piece list into the six words, are in aqc_fmtwin.hpp)

// exclusive prefixes of two values per thread over the FMT_TILE threads of a plan workgroup (two waves): DPP lane scans, the other
// wave's totals through LDS (`lds`: 2 x 2 words of its own per call site — one barrier, none for reuse)
__device__ __forceinline__ void tile_excl_scan2(uint32_t a, uint32_t b, uint32_t (*lds)[2], uint32_t& ea, uint32_t& eb) {
    static_assert(FMT_TILE == 2 * WAVE, "two waves per plan workgroup");
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const int ia = wave_incl_sum((int)a, lane), ib = wave_incl_sum((int)b, lane);
    if (lane == WAVE - 1) { lds[wave][0] = (uint32_t)ia; lds[wave][1] = (uint32_t)ib; }
    __syncthreads();
    ea = (uint32_t)ia - a + (wave ? lds[0][0] : 0u);
    eb = (uint32_t)ib - b + (wave ? lds[0][1] : 0u);
}

__global__ __launch_bounds__(FMT_TILE) void fmt_plan_kernel(FormatView v, uint64_t n, uint64_t n_tiles, uint64_t n_super,
                                                            const unsigned long long* __restrict__ tile_base, const unsigned long long* __restrict__ super_base, int overlap_pass,
                                                            int* __restrict__ status, uint4* __restrict__ plan0, uint4* __restrict__ plan_patch, uint4* __restrict__ plan_gen,
                                                            FmtTask* __restrict__ over, uint32_t* __restrict__ gen_list,
                                                            unsigned int* __restrict__ n_gen, uint64_t gen_cap,
                                                            uint4* __restrict__ whole_plan, unsigned int* __restrict__ n_whole, uint8_t* __restrict__ good0, uint8_t* __restrict__ good1,
                                                            SpanEvent* __restrict__ events0, SpanEvent* __restrict__ events1) {
    __shared__ unsigned long long lds[4];
    __shared__ uint32_t lds2[2][2][2];          // [file][wave][good, bad]: tile_excl_scan2
    __shared__ FmtTask tasks[FMT_TILE];
    const int nfiles = v.paired ? 2 : 1;
    const uint64_t r = (uint64_t)blockIdx.x * FMT_TILE + threadIdx.x;
    // bytes of stream q before this tile: the super-tiles before (fmt_tile_bases_kernel) + the tiles before inside the super-tile
    auto base_of = [&](int q) -> unsigned long long {
        return super_base[(uint64_t)q * n_super + blockIdx.x / FMT_SUPER] + tile_base[(uint64_t)q * n_tiles + blockIdx.x];
    };
    for (int file = 0; file < nfiles; ++file) {
        FmtTask& t = tasks[threadIdx.x];
        t.stream = 0xff;
        t.total = 0;
        uint32_t sz[3] = {0, 0, 0};
        uint32_t event = 0;                     // spans mode, main pass: this record is not one that stays where it is
        if (r < n) {
            // (spans mode: a whole record needs no piece list — it is not copied — except for the overlap stream's slice of it)
            const uint32_t fs = v.fused ? v.fstate[file][r] : 0u;
            const bool whole = v.fused ? (fs & (FMT_FUSED_DONE | FMT_FUSED_PATCH)) == FMT_FUSED_DONE
                                       : v.spans && !overlap_pass && record_is_whole(v, v.f[file], r, file, *reinterpret_cast<const uint4*>(v.results + r));
            if (!whole) fmt_build(v, r, file, overlap_pass, t, status);
            event = (v.spans && !overlap_pass && !whole) ? 1u : 0u;
            if (!overlap_pass) sz[t.stream == 1 ? 1 : 0] = t.stream == 0xff ? 0u : (uint32_t)t.total;
            else sz[2] = t.stream == 2 ? (uint32_t)t.total : 0u;
        }
        if (v.spans && !overlap_pass) {
            // the event list of the file, in record order: where the record stood in the chunk, what it gives to stream 0
            unsigned long long te;
            const unsigned long long ee = block_excl_scan((unsigned long long)event, lds, te);
            if (event) {
                const TextFile& tf = v.f[file];
                const uint32_t a = tf.name_off[r];
                const uint32_t b = r + 1 < v.n_framed ? tf.name_off[r + 1] : v.consumed[file];
                SpanEvent* const ev = file == 0 ? events0 : events1;
                ev[base_of(FMT_EVENT_STREAM + file) + ee] = SpanEvent{a, b - a, t.stream == 0 ? (uint32_t)t.total : 0u};
            }
        }
        unsigned int pos;
        bool general = false, listed_whole = false;
        const uint4 zero4 = make_uint4(0, 0, 0, 0);
        uint4 q0 = zero4, q1 = zero4, q2 = zero4, q3 = zero4, q4 = zero4, q5 = zero4;      // (named, not an array: an array of them ended up in scratch)
        if (v.fused) {
            // (placed by the verdict kernel: no scans, no tile bases)
            pos = 0u;
            if (r < n && t.stream != 0xff) {
                const uint64_t b = r >> v.fbatch_shift;
                const unsigned long long w = b ? v.fbatch[2 * (b - 1) + (t.stream == 1 ? 1 : 0)] : 0ull;
                pos = (unsigned int)((file == 0 ? (w >> 31) : w) & 0x7fffffffull) + (v.fstate[file][r] & FMT_FUSED_OFF);
                if (v.fstate[file][r] & FMT_FUSED_DONE) {
                    // the verdict kernel wrote the record's own bytes; the walk's edits go on top (its launch is long complete)
                    uint8_t* const rec_out = (file == 0 ? good0 : good1) + pos;
                    for (int e = 0; e < (int)t.n_patch; ++e) rec_out[t.patch[e] & 0xffffu] = (uint8_t)(t.patch[e] >> 16);
                    t.stream = 0xff;
                }
            }
        } else if (!overlap_pass) {
            // good and bad records interleave: two scans, each record keeps the offset of the stream it goes to
            uint32_t eg, eb;
            tile_excl_scan2(sz[0], sz[1], lds2[file], eg, eb);
            pos = sz[1] ? (unsigned int)(base_of(file * 3 + 1) + eb) : (unsigned int)(base_of(file * 3 + 0) + eg);      // (offsets inside a chunk's stream fit 32 bits)
        } else {
            unsigned long long to;
            const unsigned long long eo = block_excl_scan((unsigned long long)sz[2], lds, to);
            pos = (unsigned int)(base_of(file * 3 + 2) + eo);
        }
        if (r < n) {
            const uint64_t ti = r * nfiles + file;
            q0 = make_uint4(pos, PLAN_SKIP, 0, 0);
            if (t.stream != 0xff) {
                t.pos = pos;
                const PlanWords pw = plan_words(t, pos);
                q0 = pw.q0; q1 = pw.q1; q2 = pw.q2; q3 = pw.q3; q4 = pw.q4; q5 = pw.q5;
                if (!pw.inline_ok) over[ti] = t;
            }
            // (spans / fused mode: the records that stay where they are / that the verdict kernel copied have no plan: PLAN_SKIP)
            // Text mode: nearly every record is one piece — fmt_copy_whole_kernel walks the dense plan0.  Spans / fused mode: few
            // are left (the pairs the walk edited) — their plans are LISTED (q0 with the file in bit 24 | the patches) and
            // fmt_copy_whole_list_kernel walks the lists (a dense walk over 10 M mostly empty plans cost 0.8 ms).
            // (a barcode run has no one-piece record — every good name is rewritten, every bad one flagged: no dense plans, and the
            //  host does not launch the kernel that would walk them: 0.33 ms per 6 M records of config 5 for nothing; should a plan
            //  be one piece after all it goes the general way)
            const bool no_dense = v.barcode && !v.plain;
            const bool whole = plan_is_whole(q0) && !no_dense;
            const bool sparse = v.spans || v.fused;
            if (!sparse && !no_dense) {
                plan0[ti] = q0;
                if (whole && (q0.y & 0x00ff0000u)) plan_patch[ti] = q5;        // (written and read for the patched records only)
            }
            general = q0.y != PLAN_SKIP && !whole;
            listed_whole = sparse && whole;
        }
        // the records fmt_copy_whole_kernel does not take are listed (one atomic per wave) for the general copy kernel
        {
            const unsigned long long gm = __ballot(general);
            if (gm) {
                unsigned int base = 0;
                // (GEN_LISTS separate lists, tile t appends to list t % GEN_LISTS: one shared counter would serialise
                //  ~10^5 same-address atomics in L2 — that alone cost 1.3 ms)
                const unsigned int lj = blockIdx.x % GEN_LISTS;
                if (lane_id() == 0) base = atomicAdd(&n_gen[lj], (unsigned int)__popcll(gm));
                base = (unsigned int)__shfl((int)base, 0, WAVE);
                if (general) {
                    // the general kernel reads its plans in list order: all six words go where the record is listed
                    const uint64_t slot = (uint64_t)lj * gen_cap + base + (unsigned int)__popcll(gm & ((1ull << lane_id()) - 1ull));
                    gen_list[slot] = (uint32_t)(r * nfiles + file);
                    uint4* const pg = plan_gen + slot * PLAN_Q;
                    pg[0] = q0; pg[1] = q1; pg[2] = q2; pg[3] = q3; pg[4] = q4; pg[5] = q5;
                }
            }
        }
        {
            const unsigned long long wm = __ballot(listed_whole);
            if (wm) {
                unsigned int base = 0;
                const unsigned int lj = blockIdx.x % GEN_LISTS;
                if (lane_id() == 0) base = atomicAdd(&n_whole[lj], (unsigned int)__popcll(wm));
                base = (unsigned int)__shfl((int)base, 0, WAVE);
                if (listed_whole) {
                    const uint64_t slot = (uint64_t)lj * gen_cap + base + (unsigned int)__popcll(wm & ((1ull << lane_id()) - 1ull));
                    whole_plan[2 * slot] = make_uint4(q0.x, q0.y | ((uint32_t)file << 24), q0.z, q0.w);
                    whole_plan[2 * slot + 1] = q5;
                }
            }
        }
        __syncthreads();            // (tasks[] is reused for the second file)
    }
}

constexpr int FMT_UNROLL = 4;
constexpr int COPY_BLOCK = 256;

// Records that are ONE piece (untrimmed, unedited, not renamed: the bulk of a -f 0 -t 0 run): 32 lanes, window
// min(16 * lane, len - 16), load, store — as lean as a copy gets (tools/ubench/copy_rate.hip: this shape moves 6.9 GB in
// 1.4 ms without the plan read, 1.6 ms with it).
// pa[u]: the plan's first word (PLAN_SKIP: nothing), file[u]: its file, pq[u]: where its patch word stands
template <int NU>
__device__ __forceinline__ void copy_whole_tasks(const FormatView& v, const uint4 (&pa)[NU], const int (&file_of)[NU], const uint4* const (&pq)[NU],
                                                 const FormatOut& outs, int lane32) {
    uint4 val[NU];
    uint8_t* dptr[NU];
    bool on[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int file = file_of[u];
        const int len = (int)(pa[u].w & 0xffffu);
        uint8_t* const d0 = outs.p[file * 3 + (int)(pa[u].y & 0xffu)] + pa[u].x;
        const uint8_t* const s0 = v.f[file].text + pa[u].z;
        // the windows: head window + the source's 16-byte grid, the last one end-aligned (the rule's text: aqc_fmtwin.hpp)
        FMTW_WHOLE_WINDOW_GRID(len, s0, lane32, nw, off)
        on[u] = plan_is_whole(pa[u]) && lane32 < nw;
        FMTW_WHOLE_WINDOW_END(len, off)
        dptr[u] = d0 + off;
        if (on[u]) val[u] = load16u(s0 + off);
    }
    // the correction walk's edits: byte patches applied in registers (windows that overlap carry the same patch)
    // (a wave-level test per record in flight and per patch: 8 % of a 2 x 150 run's records carry one or two, and half the rounds of a wave
    //  — eight records — met one: all 16 patch slots were worked through for them)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const uint32_t np = on[u] ? (pa[u].y >> 16) & 0xffu : 0u;
        if (__ballot(np != 0)) {
            if (np) {
                const uint4 q5 = *pq[u];
                const uint32_t pt[4] = {q5.x, q5.y, q5.z, q5.w};
                const uint32_t wpos = (uint32_t)(dptr[u] - (outs.p[file_of[u] * 3 + (int)(pa[u].y & 0xffu)] + pa[u].x));      // (the window's place in the record)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e > 0 && __ballot((uint32_t)e < np) == 0) break;
                    const uint32_t i = (pt[e] & 0xffffu) - wpos;
                    const bool hit = (uint32_t)e < np && i < 16u;
                    const uint32_t sh = (i & 3u) * 8u, m = hit ? 0xffu << sh : 0u, cb = hit ? ((pt[e] >> 16) & 0xffu) << sh : 0u;
                    const uint32_t wd = i >> 2;
                    val[u].x = wd == 0 ? (val[u].x & ~m) | cb : val[u].x;
                    val[u].y = wd == 1 ? (val[u].y & ~m) | cb : val[u].y;
                    val[u].z = wd == 2 ? (val[u].z & ~m) | cb : val[u].z;
                    val[u].w = wd == 3 ? (val[u].w & ~m) | cb : val[u].w;
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u)
        if (on[u]) store16u(dptr[u], val[u]);      // (non-temporal loads / stores here: 3.95 -> 4.23 ms per step either way — measured, left out)
}

__global__ __launch_bounds__(COPY_BLOCK) void fmt_copy_whole_kernel(FormatView v, uint64_t n_tasks, const uint4* __restrict__ plan,
                                                                   const uint4* __restrict__ plan_patch, FormatOut outs) {
    const int nfiles = v.paired ? 2 : 1;
    const int lane32 = threadIdx.x & 31;
    // (grid-strided: the host launches one workgroup per 32 records)
    const uint64_t n_hw = ((uint64_t)gridDim.x * COPY_BLOCK) >> 5;
    for (uint64_t hw = ((uint64_t)blockIdx.x * COPY_BLOCK + threadIdx.x) >> 5; hw * FMT_UNROLL < n_tasks; hw += n_hw) {
        uint4 pa[FMT_UNROLL];
        int file_of[FMT_UNROLL];
        const uint4* pq[FMT_UNROLL];
#pragma unroll
        for (int u = 0; u < FMT_UNROLL; ++u) {
            const uint64_t ti = hw * FMT_UNROLL + u;
            pa[u] = make_uint4(0, PLAN_SKIP, 0, 0);
            if (ti < n_tasks) pa[u] = plan[ti];
            file_of[u] = nfiles == 2 ? (int)(ti & 1) : 0;
            pq[u] = plan_patch + ti;
        }
        copy_whole_tasks(v, pa, file_of, pq, outs, lane32);
    }
}

// ... the same for the LISTED one-piece records of a spans / fused format (fmt_plan_kernel): workgroup b walks list b % GEN_LISTS, whose
// plans stand in list order (two 16-byte words each: one coalesced load per round, then the text)
__global__ __launch_bounds__(COPY_BLOCK) void fmt_copy_whole_list_kernel(FormatView v, const uint4* __restrict__ whole_plans, FormatOut outs,
                                                                        const unsigned int* __restrict__ n_whole, uint64_t gen_cap) {
    const int lane32 = threadIdx.x & 31, hwi = threadIdx.x >> 5;
    const unsigned int lj = blockIdx.x % GEN_LISTS;
    const uint4* wp = whole_plans + 2 * (uint64_t)lj * gen_cap;
    const uint32_t n_list = n_whole[lj];
    constexpr uint32_t PER_WG = (COPY_BLOCK / 32) * FMT_UNROLL;
    const uint32_t stride = (gridDim.x / GEN_LISTS) * PER_WG;
    for (uint32_t r0 = (blockIdx.x / GEN_LISTS) * PER_WG; r0 < n_list; r0 += stride) {
        uint4 pa[FMT_UNROLL];
        int file_of[FMT_UNROLL];
        const uint4* pq[FMT_UNROLL];
#pragma unroll
        for (int u = 0; u < FMT_UNROLL; ++u) {
            const uint32_t idx = r0 + (uint32_t)(hwi * FMT_UNROLL + u);
            pa[u] = make_uint4(0, PLAN_SKIP, 0, 0);
            if (idx < n_list) pa[u] = wp[2 * (uint64_t)idx];
            file_of[u] = (int)((pa[u].y >> 24) & 1u);
            if (pa[u].y != PLAN_SKIP) pa[u].y &= ~(1u << 24);
            pq[u] = wp + 2 * (uint64_t)min(idx, n_list - 1u) + 1;
        }
        copy_whole_tasks(v, pa, file_of, pq, outs, lane32);
    }
}

// Everything else, from the plan kernel's lists: 32 lanes per plan, two plans in flight per half-wave, a lane owns one work
// item — a 16-byte window of a long piece (16-byte load + 16-byte store at any alignment, the piece's last window
// end-aligned) or a whole short piece.  Stages (list, plans, decode, loads, patches, stores) run over both plans so that
// each stage's memory operations travel together.
constexpr int GEN_U = 2;                                   // plans per half-wave per round
constexpr int GEN_ROUND = (COPY_BLOCK / 32) * GEN_U;       // plans per workgroup per round
static_assert(GEN_ROUND * PLAN_Q <= COPY_BLOCK, "one 16-byte word per thread stages a round's plans");

// Everything that is not "one piece": the plans arrive in list order (fmt_plan_kernel), so a workgroup stages the 16 plans
// of a round with ONE coalesced load into LDS (1.5 KB) and its eight half-waves take two plans each: per lane up to four
// 16-byte windows in flight (32 lanes x 2 work items per plan), held as 32-bit offsets — the earlier version kept the
// plans in registers (48 of them), had two records in flight per half-wave and three dependent memory round trips per
// iteration (list -> plan -> data): 1.6 TB/s.
__global__ __launch_bounds__(COPY_BLOCK) void fmt_copy_kernel(FormatView v, const uint4* __restrict__ plan_gen, const FmtTask* __restrict__ over,
                                                             FormatOut outs, const uint32_t* __restrict__ gen_lists,
                                                             const unsigned int* __restrict__ n_gen, uint64_t gen_cap) {
    __shared__ uint4 s_plan[GEN_ROUND * PLAN_Q];
    __shared__ uint32_t s_ti[GEN_ROUND];
    __shared__ const uint8_t* s_ptr[8];                       // [0..5] output streams (file * 3 + stream), [6..7] the files' texts
    const int nfiles = v.paired ? 2 : 1;
    const int lane32 = threadIdx.x & 31, hwi = threadIdx.x >> 5;
    if (threadIdx.x < 6) s_ptr[threadIdx.x] = outs.p[threadIdx.x];
    if (threadIdx.x >= 6 && threadIdx.x < 8) s_ptr[threadIdx.x] = v.f[threadIdx.x - 6].text;
    // workgroup b works on list b % GEN_LISTS together with the other workgroups of that list
    const unsigned int lj = blockIdx.x % GEN_LISTS;
    const uint32_t* gen_list = gen_lists + (uint64_t)lj * gen_cap;
    const uint4* pg = plan_gen + (uint64_t)lj * gen_cap * PLAN_Q;
    const uint32_t n_list = n_gen[lj];
    const uint32_t stride = (gridDim.x / GEN_LISTS) * GEN_ROUND;
    for (uint32_t r0 = (blockIdx.x / GEN_LISTS) * GEN_ROUND; r0 < n_list; r0 += stride) {
        const uint32_t cnt = min((uint32_t)GEN_ROUND, n_list - r0);
        __syncthreads();                                     // (the previous round's plans are no longer read)
        if (threadIdx.x < cnt * PLAN_Q) s_plan[threadIdx.x] = pg[(uint64_t)r0 * PLAN_Q + threadIdx.x];
        if (threadIdx.x < cnt) s_ti[threadIdx.x] = gen_list[r0 + threadIdx.x];
        __syncthreads();
        // (round 6, measured twice and left out: the next round's plans prefetched into registers while this round is worked on — with the
        //  79-register kernel a wave less per SIMD, config 5 2.32 -> 2.41 ms; with this one 4.82 -> 4.80 ms per step: not what a round waits for)
        constexpr int NWIN = GEN_U * GEN_PASSES;          // windows in flight per lane: plan u, pass j -> slot u * GEN_PASSES + j
        uint4 val[NWIN];
        uint32_t so[NWIN], dof[NWIN], mw[NWIN];           // source offset (FMT_LIT_BIT: literal table), offset in the output stream,
                                                          // mode | position in the record << 5 | file * 3 + stream << 21 | file << 24
                                                          // (mode: 0 nothing, 16 a window, 1..15 a short piece of that many bytes)
        uint32_t more = 0;                                // bit u: plan u lives in the overflow array
        const uint8_t* const tp0 = s_ptr[6];
        const uint8_t* const tp1 = s_ptr[7];
        // (straight-line on purpose: with a branch per plan / window the instruction stream was one saveexec - branch - nop
        //  sequence after the other and the kernel spent its time on instruction latency)
#pragma unroll
        for (int u = 0; u < GEN_U; ++u) {
            const uint32_t idx = (uint32_t)(hwi * GEN_U + u);
            const bool live = idx < cnt;
            const uint4* P = s_plan + (live ? idx : 0u) * PLAN_Q;
            // (round 6) the fields of my piece are READ from the plan in LDS at an address worked out from k — a 32-bit source, two 16-bit
            // reads — and k itself is a packed byte compare: the eight-way selects and seven compares per window they replace were a
            // third of this kernel's vector instructions
            const uint8_t* const pb = reinterpret_cast<const uint8_t*>(P);
            const uint4 q0 = P[0];
            FMTW_PLAN_HEAD(pb, cumw, q4w)                                                                // q3.z, q3.w: cumulative items, a byte per piece | q4.w
            const bool ovf = live && (q0.y & PLAN_OVER) != 0;
            more |= ovf ? 1u << u : 0u;
            const uint32_t file = nfiles == 2 ? (s_ti[live ? idx : 0u] & 1u) : 0u;
            const uint32_t fs = file * 3u + (q0.y & 0xffu);
            const uint32_t items = (live && !ovf) ? q4w >> 16 : 0u;
            const unsigned long long cum = ((unsigned long long)cumw.y << 32) | cumw.x;
#pragma unroll
            for (int j = 0; j < GEN_PASSES; ++j) {
                const int w = u * GEN_PASSES + j;
                const uint32_t item = (uint32_t)lane32 + 32u * j;
                const bool on = item < items;
                // my piece, read from the plan in LDS at an address worked out from its number k ...
                FMTW_PLAN_PIECE(pb, cumw, cum, item, on, k, first_item, lk, dst_off, sk)
                // ... and my window of it: a long piece's 16-byte window, the last one aligned to the piece's end; a short piece: all of it
                FMTW_GEN_WINDOW(lk, (uint32_t)(uintptr_t)(file ? tp1 : tp0), sk, (int)item - first_item, off)
                so[w] = sk + (uint32_t)off;
                dof[w] = q0.x + (uint32_t)(dst_off + off);
                mw[w] = on ? ((uint32_t)min(lk, 16) | ((uint32_t)(dst_off + off) << 5) | (fs << 21) | (file << 24)) : 0u;
            }
        }
        const uint8_t* const lit = &FMT_LIT[0][0];
        auto src_of = [&](int w) -> const uint8_t* {
            const uint8_t* base = ((mw[w] >> 24) & 1u) ? tp1 : tp0;
            base = (so[w] & FMT_LIT_BIT) ? lit : base;
            return base + (so[w] & ~FMT_LIT_BIT);
        };
        auto dst_of = [&](int w) -> uint8_t* { return const_cast<uint8_t*>(s_ptr[(mw[w] >> 21) & 7u]) + dof[w]; };
        // every lane loads (a lane without a window reads the first bytes of the text: harmless, and no branch)
        uint32_t any_small = 0;
#pragma unroll
        for (int w = 0; w < NWIN; ++w) {
            const uint32_t md = mw[w] & 31u;
            val[w] = gload_u128(md ? src_of(w) : tp0);       // (a short piece's 16 bytes too: the text is padded, a literal is a 16-byte row)
            any_small |= (md - 1u) < 15u ? 1u : 0u;
        }
        // the correction walk's edits: byte patches applied in registers (windows that overlap carry the same patch)
        {
            uint32_t np_[GEN_U];
            uint32_t any_patch = 0;
#pragma unroll
            for (int u = 0; u < GEN_U; ++u) {
                const uint32_t idx = (uint32_t)(hwi * GEN_U + u);
                np_[u] = (idx < cnt && !((more >> u) & 1u)) ? (s_plan[idx * PLAN_Q].y >> 16) & 0xffu : 0u;
                any_patch |= np_[u];
            }
            if (__ballot(any_patch != 0)) {
#pragma unroll
                for (int u = 0; u < GEN_U; ++u) {
                    // (a wave-level test per plan and per patch: a record carries two patches or none, and few records any)
                    if (__ballot(np_[u] != 0) == 0) continue;
                    const uint32_t idx = min((uint32_t)(hwi * GEN_U + u), cnt - 1u);
                    const uint4 q5 = s_plan[idx * PLAN_Q + 5];
                    const uint32_t pt[4] = {q5.x, q5.y, q5.z, q5.w};
#pragma unroll
                    for (int j = 0; j < GEN_PASSES; ++j) {
                        const int w = u * GEN_PASSES + j;
                        const bool win = (mw[w] & 31u) == 16u;
                        const uint32_t wpos = (mw[w] >> 5) & 0xffffu;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (e > 0 && __ballot((uint32_t)e < np_[u]) == 0) break;
                            const uint32_t i = (pt[e] & 0xffffu) - wpos;
                            const bool hit = win && (uint32_t)e < np_[u] && i < 16u;
                            const uint32_t sh = (i & 3u) * 8u, m = hit ? 0xffu << sh : 0u, cb = hit ? ((pt[e] >> 16) & 0xffu) << sh : 0u;
                            const uint32_t wd = i >> 2;
                            val[w].x = wd == 0 ? (val[w].x & ~m) | cb : val[w].x;
                            val[w].y = wd == 1 ? (val[w].y & ~m) | cb : val[w].y;
                            val[w].z = wd == 2 ? (val[w].z & ~m) | cb : val[w].z;
                            val[w].w = wd == 3 ? (val[w].w & ~m) | cb : val[w].w;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int w = 0; w < NWIN; ++w)
            if ((mw[w] & 31u) == 16u) gstore_u128(dst_of(w), val[w]);
        // pieces of 1..15 bytes — a literal '@', a moved barcode, a stray newline: their bytes came with the windows' loads; 8 + 4 + 2 + 1
        // bytes stored as the length's bits say.  (Rounds 2 - 5 copied them behind the windows, a branch per size class with its own
        // load -> store round trip: two or three memory latencies per round of a barcode run, where every record has two of them.)
        if (__ballot(any_small != 0)) {
#pragma unroll
            for (int w = 0; w < NWIN; ++w) {
                const uint32_t md = mw[w] & 31u;
                const bool sm = (md - 1u) < 15u;
                uint8_t* const d = dst_of(w);
                const uint32_t i2 = (md >> 2) & 3u;
                uint32_t vx = val[w].x, vy = val[w].y, vz = val[w].z, vw = val[w].w;
                asm volatile("" : "+v"(vx), "+v"(vy), "+v"(vz), "+v"(vw));      // (values, not addresses: a select of loads would put val[] into scratch)
                const uint32_t pick = i2 == 0u ? vx : i2 == 1u ? vy : i2 == 2u ? vz : vw;      // the word of byte (md & 12)
                if (sm && (md & 8u)) gstore_u64(d, vx, vy);
                if (sm && (md & 4u)) gstore_u32(d + (md & 8u), (md & 8u) ? vz : vx);
                if (sm && (md & 2u)) gstore_u16(d + (md & 12u), (uint16_t)pick);
                if (sm && (md & 1u)) gstore_u8(d + (md & 14u), (uint8_t)(pick >> ((md & 2u) * 8u)));
            }
        }
        // ---- overflow records: any number of pieces / work items, piece by piece (records of more than 1 KiB, more than
        //      eight pieces or four patches)
        if (more) {
            for (int u = 0; u < GEN_U; ++u) {
                if (!((more >> u) & 1u)) continue;
                const uint64_t ti = s_ti[hwi * GEN_U + u];
                const FmtTask& t = over[ti];
                const int file = nfiles == 2 ? (int)(ti & 1) : 0;
                uint8_t* out0 = outs.p[file * 3 + (int)t.stream] + t.pos;
                const int np = (int)t.np;
                for (int k = 0; k < np; ++k) {
                    const uint32_t sk = t.p[k].src;
                    const int lk = (int)t.p[k].len;
                    const uint8_t* src = (sk & FMT_LIT_BIT) ? &FMT_LIT[0][0] + (sk & ~FMT_LIT_BIT) : v.f[file].text + sk;
                    uint8_t* dst = out0 + t.p[k].dst;
                    if (lk >= 16) {
                        for (int w0 = 16 * lane32; w0 < lk; w0 += 16 * 32) {
                            const int off = min(w0, lk - 16);
                            store16u(dst + off, load16u(src + off));
                        }
                    } else if (lane32 < lk) dst[lane32] = src[lane32];
                }
                if (t.n_patch) {
                    // byte patches on top of the copies (the copies of this wave are complete first)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_s_waitcnt(0);
                    if (lane32 < (int)t.n_patch) {
                        const uint32_t pt = t.patch[lane32];
                        out0[pt & 0xffffu] = (uint8_t)(pt >> 16);
                    }
                }
            }
        }
    }
}

// ---- round 6: the text mode's default writer — place + copy in one kernel, piece lists only for the records that need them ------
// (rounds 2 - 5: fmt_plan_kernel built the piece list of EVERY record — fmt_build, a 116-byte task in LDS, six plan words — wrote a
//  16-byte plan per record and file to HBM, and fmt_copy_whole_kernel read it back: 0.31 + 2.06 ms and 0.64 GB of plan traffic per
//  10 M reads, although 97 % of the records of a run without trimming go out as their own bytes.)
// A workgroup takes a tile of FMT_TILE records, thread = (record, file):
//   1. the record's bytes in its streams (fmt_sizes — the sizing pass's routine, so the two agree by construction), two DPP scans
//      per file, the tile's bases -> the record's place;
//   2. a good record that is its own bytes (record_is_whole's conditions, but edits of the walk in this mate become <= 4 byte
//      patches): its plan word (+ patch word) stays in LDS;  every other record is LISTED for fmt_plan_listed_kernel with its place;
//   3. the workgroup copies its own-bytes records: 32 lanes per record, four records in flight per half-wave (copy_whole_tasks).
// fmt_plan_listed_kernel then builds the piece lists / plans of the listed records only (thread = list entry), fmt_copy_kernel
// copies them as before.  Barcode runs (every name rewritten), index files, the overlap pass, spans and fused formats keep
// fmt_plan_kernel.
__device__ __forceinline__ int own_bytes_patches(const uint4& w0, const uint4& w1, int file, int len, int seq_dst, int qual_dst, uint32_t (&patch)[6]) {
    // fmt_build's edit loop for a record whose quality line is as long as its sequence line, written from base 0 (cut == 0)
    const int n_edits = (int)((w0.x >> 8) & 0xffu);
    const int len1 = (int)(w0.y & 0xffffu), len2 = (int)(w0.z & 0xffffu), ovl = (int)(w0.w & 0xffffu);
    const unsigned long long e_lo = ((unsigned long long)w1.y << 32) | w1.x, e_hi = ((unsigned long long)w1.w << 32) | w1.z;
    int np = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (e >= n_edits) break;
        const int bit = 40 * e;
        unsigned long long x = bit < 64 ? e_lo >> bit : 0ull;
        if (bit + 40 > 64) x |= bit < 64 ? e_hi << (64 - bit) : e_hi >> (bit - 64);
        const int oo = (int)(x & 0xffffu);
        const uint32_t kind = (uint32_t)(x >> 16) & 0xffu, base = (uint32_t)(x >> 24) & 0xffu, qual = (uint32_t)(x >> 32) & 0xffu;
        const int pp = file == 0 ? len1 - ovl + oo : len2 - 1 - oo;
        if (pp < 0 || pp >= len) continue;
        if (kind == AQC_EDIT_MASK) patch[np++] = (uint32_t)(qual_dst + pp) | ((uint32_t)'!' << 16);
        else if ((kind == AQC_EDIT_FIX_R1 && file == 0) || (kind == AQC_EDIT_FIX_R2 && file == 1)) {
            if (base) patch[np++] = (uint32_t)(seq_dst + pp) | (base << 16);
            patch[np++] = (uint32_t)(qual_dst + pp) | (qual << 16);
        }
    }
    return np;
}

constexpr int PC_BLOCK = 2 * FMT_TILE;       // thread = (record of the tile, file)
constexpr int PC_UNROLL = 4;                 // records in flight per half-wave in the copy phase
static_assert(PC_BLOCK == COPY_BLOCK, "the copy phase is fmt_copy_whole_kernel's");

__global__ __launch_bounds__(PC_BLOCK, 1) void fmt_place_copy_kernel(FormatView v, uint64_t n, uint64_t n_tiles, uint64_t n_super,
                                                                   const unsigned long long* __restrict__ tile_base, const unsigned long long* __restrict__ super_base,
                                                                   uint4* __restrict__ plan_gen, uint32_t* __restrict__ gen_list, unsigned int* __restrict__ n_gen,
                                                                   uint64_t gen_cap, FormatOut outs) {
    __shared__ uint4 s_q0[PC_BLOCK], s_q5[PC_BLOCK];
    __shared__ uint32_t s_tot[PC_BLOCK / WAVE][2];
    const int nfiles = v.paired ? 2 : 1;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const int file = wave >> 1;                                           // waves 0, 1: the tile's records of file 0; waves 2, 3: of file 1
    const uint64_t r = (uint64_t)blockIdx.x * FMT_TILE + (threadIdx.x & (FMT_TILE - 1));
    const bool have = file < nfiles && r < n;
    uint32_t sz[3] = {0, 0, 0}, ev = 0;
    uint4 q0 = make_uint4(0, PLAN_SKIP, 0, 0), q5 = make_uint4(0, 0, 0, 0);
    bool own = false;
    uint32_t own_src = 0, n_patch = 0;
    if (have) {
        fmt_sizes(v, r, file, sz, ev);
        const TextFile& tf = v.f[file];
        const uint4 w0 = *reinterpret_cast<const uint4*>(v.results + r);
        const uint32_t slw = tf.seq_len[r];
        const uint32_t st = file == 0 ? (w0.x >> 16) : (w0.y >> 16), len = file == 0 ? (w0.y & 0xffffu) : (w0.z & 0xffffu);
        // its own bytes: good, the whole read (a mate marked LEN_IRR never equals its length word), every line followed directly by
        // its '\n' — then sz[0] = name + bases + strand line + qualities + 4 is the distance from its name to behind its last '\n'
        if ((int)(w0.x & 0xffu) == AQC_GOOD && st == 0u && len == slw && (tf.qual_len[r] & QLEN_CONTIG) && sz[0] >= 16u && sz[0] <= 512u) {
            own = true;
            own_src = tf.name_off[r];
            if ((w0.x >> 8) & 0xffu) {
                const uint4 w1 = *(reinterpret_cast<const uint4*>(v.results + r) + 1);
                const int nlen = (int)tf.name_len[r], plen = (int)(tf.plus_len[r] & LEN_MASK);
                uint32_t patch[6] = {0, 0, 0, 0, 0, 0};
                n_patch = (uint32_t)own_bytes_patches(w0, w1, file, (int)len, nlen + 1, nlen + 1 + (int)len + 1 + plen + 1, patch);
                q5 = make_uint4(patch[0], patch[1], patch[2], patch[3]);
                own = n_patch <= 4u;                                      // (three corrections in one mate: the general kernel's overflow path)
            }
        }
    }
    // the record's place: exclusive prefixes over the tile's records of this file (two waves), good and bad apart
    const int ig = wave_incl_sum((int)sz[0], lane), ib = wave_incl_sum((int)sz[1], lane);
    if (lane == WAVE - 1) { s_tot[wave][0] = (uint32_t)ig; s_tot[wave][1] = (uint32_t)ib; }
    __syncthreads();
    uint32_t pos = 0;
    if (have) {
        const int q = file * 3 + (sz[1] ? 1 : 0);
        const unsigned long long base = super_base[(uint64_t)q * n_super + blockIdx.x / FMT_SUPER] + tile_base[(uint64_t)q * n_tiles + blockIdx.x];
        const uint32_t ex = sz[1] ? (uint32_t)ib - sz[1] + ((wave & 1) ? s_tot[wave - 1][1] : 0u) : (uint32_t)ig - sz[0] + ((wave & 1) ? s_tot[wave - 1][0] : 0u);
        pos = (uint32_t)(base + ex);                                      // (offsets inside a chunk's stream fit 32 bits)
        if (own) q0 = make_uint4(pos, 0x100u | (n_patch << 16), own_src, sz[0]);      // stream 0, one piece: what fmt_build + plan_words make of it
    }
    s_q0[threadIdx.x] = q0;
    s_q5[threadIdx.x] = q5;
    // everything else is listed for fmt_plan_listed_kernel, with its place (one atomic per wave; the lists: see fmt_plan_kernel)
    {
        const bool general = have && !own;
        const unsigned long long gm = __ballot(general);
        if (gm) {
            unsigned int b0 = 0;
            const unsigned int lj = blockIdx.x % GEN_LISTS;
            if (lane == 0) b0 = atomicAdd(&n_gen[lj], (unsigned int)__popcll(gm));
            b0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)b0);
            if (general) {
                const uint64_t slot = (uint64_t)lj * gen_cap + b0 + (unsigned int)__popcll(gm & ((1ull << lane) - 1ull));
                gen_list[slot] = (uint32_t)(r * nfiles + file);
                plan_gen[slot * PLAN_Q] = make_uint4(pos, PLAN_SKIP, 0, 0);
            }
        }
    }
    __syncthreads();
    // the copy: a half-wave per record, FMT_UNROLL records in flight, plans and patch words from LDS
    const int lane32 = threadIdx.x & 31, hwi = threadIdx.x >> 5;
    const int n_plans = nfiles * FMT_TILE;
    constexpr int PER_ROUND = (PC_BLOCK / 32) * PC_UNROLL;
#pragma unroll 1
    for (int p0 = 0; p0 < n_plans; p0 += PER_ROUND) {
        uint4 pa[PC_UNROLL];
        int file_of[PC_UNROLL];
        const uint4* pq[PC_UNROLL];
#pragma unroll
        for (int u = 0; u < PC_UNROLL; ++u) {
            const int p = p0 + hwi * PC_UNROLL + u;                       // (< PC_BLOCK: a single-end tile's upper half says PLAN_SKIP)
            pa[u] = s_q0[p];
            file_of[u] = p / FMT_TILE;
            pq[u] = &s_q5[p];
        }
        copy_whole_tasks(v, pa, file_of, pq, outs, lane32);
    }
}

// the piece lists and plans of the records fmt_place_copy_kernel listed: workgroup b works on list b % GEN_LISTS, thread = entry
__global__ __launch_bounds__(FMT_TILE) void fmt_plan_listed_kernel(FormatView v, uint4* __restrict__ plan_gen, FmtTask* __restrict__ over,
                                                                   const uint32_t* __restrict__ gen_lists, const unsigned int* __restrict__ n_gen,
                                                                   uint64_t gen_cap, int* __restrict__ status) {
    __shared__ FmtTask tasks[FMT_TILE];
    const int nfiles = v.paired ? 2 : 1;
    const unsigned int lj = blockIdx.x % GEN_LISTS;
    const uint32_t n_list = n_gen[lj];
    const uint32_t stride = (gridDim.x / GEN_LISTS) * FMT_TILE;
    FmtTask& t = tasks[threadIdx.x];
    for (uint32_t i = (blockIdx.x / GEN_LISTS) * FMT_TILE + threadIdx.x; i < n_list; i += stride) {
        const uint64_t slot = (uint64_t)lj * gen_cap + i;
        const uint64_t ti = gen_lists[slot];
        const uint32_t pos = plan_gen[slot * PLAN_Q].x;
        const uint64_t r = nfiles == 2 ? ti >> 1 : ti;
        const int file = nfiles == 2 ? (int)(ti & 1) : 0;
        fmt_build(v, r, file, 0, t, status);
        const uint4 zero4 = make_uint4(0, 0, 0, 0);
        uint4 q0 = make_uint4(pos, PLAN_SKIP, 0, 0), q1 = zero4, q2 = zero4, q3 = zero4, q4 = zero4, q5 = zero4;
        if (t.stream != 0xff) {
            t.pos = pos;
            const PlanWords pw = plan_words(t, pos);
            q0 = pw.q0; q1 = pw.q1; q2 = pw.q2; q3 = pw.q3; q4 = pw.q4; q5 = pw.q5;
            if (!pw.inline_ok) over[ti] = t;
        }
        uint4* const pg = plan_gen + slot * PLAN_Q;
        pg[0] = q0; pg[1] = q1; pg[2] = q2; pg[3] = q3; pg[4] = q4; pg[5] = q5;
    }
}

// ---- --store_merged: the second pass of a format in mode AQC_STORE_MERGED, a kernel of its own ---------------------------------------
// The merged read of a pair is read 1's GOOD record G (fmt_build's piece list of the main pass, the walk's patches included) with
// p bytes put in behind its bases (at G's offset i1) and p behind its qualities (at i2):
//     G[0:i1] | reverseComplement(s2[0:p]) | G[i1:i2] | reversed(q2[0:p]) | G[i2:]
// A workgroup takes a tile of FMT_TILE records.  Thread = record: its bytes (fmt_sizes — the sizing pass's routine), its place (one
// block scan + the tile's base), read 1's piece list into LDS.  Then a half-wave per merged record: every piece of G is cut at i1
// and i2 and copied 16 bytes per lane (the pieces' last windows end-aligned, pieces of < 16 bytes a byte per lane), the two tails
// go out through the reversed windows of aqc_revcopy.hpp — seq and quality windows side by side in one round of the 32 lanes
// up to p = 240 —, the walk's patches go on top, moved by p where they lie in G's quality line.
struct MergedRec {
    uint32_t pos;          // offset of the merged read in stream [0][2]; the record has none: total == 0
    uint32_t total;        // bytes of G
    uint32_t i1, i2, p;
    uint32_t src_s2, src_q2;      // text offsets (file 1) of s2[0], q2[0]
};

__device__ __forceinline__ void merged_store_low(uint8_t* d, const RevWin& v, uint32_t n) {      // the low n < 16 bytes of v: 8 + 4 + 2 + 1
    uint32_t vx = v.x, vy = v.y, vz = v.z, vw = v.w;
    asm volatile("" : "+v"(vx), "+v"(vy), "+v"(vz), "+v"(vw));      // (values, not addresses: a select of loads would put v into scratch)
    const uint32_t i2 = (n >> 2) & 3u;
    const uint32_t pick = i2 == 0u ? vx : i2 == 1u ? vy : i2 == 2u ? vz : vw;                     // the word of byte (n & 12)
    if (n & 8u) gstore_u64(d, vx, vy);
    if (n & 4u) gstore_u32(d + (n & 8u), (n & 8u) ? vz : vx);
    if (n & 2u) gstore_u16(d + (n & 12u), (uint16_t)pick);
    if (n & 1u) gstore_u8(d + (n & 14u), (uint8_t)(pick >> ((n & 2u) * 8u)));
}

__global__ __launch_bounds__(FMT_TILE) void fmt_merged_kernel(FormatView v, uint64_t n, uint64_t n_tiles, uint64_t n_super,
                                                              const unsigned long long* __restrict__ tile_base, const unsigned long long* __restrict__ super_base,
                                                              int* __restrict__ status, uint8_t* __restrict__ out) {
    __shared__ unsigned long long lds[4];
    __shared__ FmtTask tasks[FMT_TILE];
    __shared__ MergedRec recs[FMT_TILE];
    const uint64_t r = (uint64_t)blockIdx.x * FMT_TILE + threadIdx.x;
    uint32_t sz[3] = {0, 0, 0}, ev = 0;
    MergedRec m{0, 0, 0, 0, 0, 0, 0};
    if (r < n) {
        fmt_sizes(v, r, 0, sz, ev);
        if (sz[2]) {
            FmtTask& t = tasks[threadIdx.x];
            fmt_build(v, r, 0, 0, t, status);
            const uint4 w0 = *reinterpret_cast<const uint4*>(v.results + r);
            const uint32_t len1 = w0.y & 0xffffu;
            m.p = merged_tail_len(w0);
            m.total = t.stream == 0 ? (uint32_t)t.total : 0u;                      // (0xff: a 64 KiB record, the status says so)
            // G = name | \n | bases | \n | strand line | \n | qualities | \n, bases and qualities len1 bytes each (a regular pair)
            m.i2 = m.total - 1u;
            m.i1 = m.total - 1u - len1 - 1u - (v.f[0].plus_len[r] & LEN_MASK) - 1u;
            const TextFile& t2 = v.f[1];
            const uint32_t st2 = w0.y >> 16;
            int qst = (int)st2, ql_ = 0;
            if (t2.plus_len[r] & LEN_IRR) irregular_quality_slice(t2, r, 0, 0, 0, qst, ql_);
            m.src_s2 = t2.seq_off[r] + st2;
            m.src_q2 = t2.qual_off[r] + (uint32_t)qst;
            if (!m.total) sz[2] = 0u;
        }
    }
    unsigned long long to;
    const unsigned long long eo = block_excl_scan((unsigned long long)sz[2], lds, to);
    m.pos = (uint32_t)(super_base[(uint64_t)2 * n_super + blockIdx.x / FMT_SUPER] + tile_base[(uint64_t)2 * n_tiles + blockIdx.x] + eo);
    recs[threadIdx.x] = m;
    __syncthreads();
    const uint32_t lane32 = threadIdx.x & 31u, hwi = threadIdx.x >> 5;
    const uint8_t* const text1 = v.f[0].text;
    const uint8_t* const text2 = v.f[1].text;
#pragma unroll 1
    for (int i = (int)hwi; i < FMT_TILE; i += FMT_TILE / 32) {
        const MergedRec& mr = recs[i];
        if (!mr.total) continue;
        const FmtTask& t = tasks[i];
        uint8_t* const out0 = out + mr.pos;
        const uint32_t p = mr.p;
        // read 1's record, cut at i1 and i2: part g goes out g * p bytes further on
        const int np = (int)t.np;
        for (int k = 0; k < np; ++k) {
            const uint32_t sk = t.p[k].src, d0 = t.p[k].dst, d1 = d0 + t.p[k].len;
            const uint8_t* const src = (sk & FMT_LIT_BIT) ? &FMT_LIT[0][0] + (sk & ~FMT_LIT_BIT) : text1 + sk;
            auto part = [&](uint32_t from, uint32_t to, uint32_t shift) {
                const uint32_t lo = max(d0, from), hi = min(d1, to);
                if (hi <= lo) return;
                const uint32_t len = hi - lo;
                const uint8_t* const s = src + (lo - d0);
                uint8_t* const d = out0 + lo + shift;
                if (len >= 16u) {
                    for (uint32_t w0 = 16u * lane32; w0 < len; w0 += 16u * 32u) {
                        const uint32_t off = min(w0, len - 16u);
                        store16u(d + off, load16u(s + off));
                    }
                } else if (lane32 < len) d[lane32] = s[lane32];
            };
            part(0u, mr.i1, 0u);
            part(mr.i1, mr.i2, p);
            part(mr.i2, mr.total, 2u * p);
        }
        // the two tails: work items [0, ni) the bases, [ni, 2 ni) the qualities
        if (p) {
            const uint32_t a_s = (0u - (uint32_t)(uintptr_t)(text2 + mr.src_s2)) & 15u, a_q = (0u - (uint32_t)(uintptr_t)(text2 + mr.src_q2)) & 15u;
            const uint32_t ni_s = revc_items(p, a_s), ni_q = revc_items(p, a_q);
            for (uint32_t it = lane32; it < ni_s + ni_q; it += 32u) {
                const bool qual = it >= ni_s;
                const int off = revc_src_off(p, qual ? a_q : a_s, qual ? it - ni_s : it);
                const uint4 ld = load16u(text2 + (qual ? mr.src_q2 : mr.src_s2) + off);
                RevWin wv = revc_reverse(RevWin{ld.x, ld.y, ld.z, ld.w});
                const RevWin cv = revc_comp16(wv);
                if (!qual) wv = cv;
                uint8_t* const d = out0 + (qual ? mr.i2 + p : mr.i1) + revc_dst_off(p, off);
                if (p >= 16u) store16u(d, make_uint4(wv.x, wv.y, wv.z, wv.w));
                else merged_store_low(d, wv, p);
            }
        }
        if (t.n_patch) {
            // byte patches on top of the copies (the copies of this wave are complete first)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);
            if (lane32 < (uint32_t)t.n_patch) {
                const uint32_t pt = t.patch[lane32], at = pt & 0xffffu;
                out0[at + (at >= mr.i1 ? p : 0u)] = (uint8_t)(pt >> 16);
            }
        }
    }
}

}  // namespace aqc
