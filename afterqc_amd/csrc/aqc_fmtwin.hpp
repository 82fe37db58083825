// aqc_fmtwin.hpp — the arithmetic of the forward copies of the text writer (aqc_fmtcopy.hpp), apart from the kernels that use it:
//
//   pieces   what a record's piece list is (FmtPiece, FmtTask) and how many work items a piece takes (piece_items);
//   plans    the six 16-byte words a piece list is packed into (plan_words) and what a lane of the general copy kernel reads
//            back from them for its work item (a packed byte compare, then reads at byte offsets worked out from the piece's number);
//   windows  where the 16-byte window of a lane stands — in a record that goes out as its own bytes (the rule of copy_whole_tasks)
//            and in a piece of the general copy kernel.
//
// Everything here is __host__ __device__ and needs no HIP: tests/native/fmtcopy_selftest.cpp includes this header with the
// host compiler and deals the windows out by plain loops, over every length and source alignment.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMTW_HD __host__ __device__ __forceinline__
#else
#define FMTW_HD inline
#endif

namespace aqc {

#if !defined(__HIPCC__)
// (the vector types of HIP, for the host compiler: little-endian dwords)
struct uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
#endif

// ---- pieces ------------------------------------------------------------------------------------------------------------------
constexpr int FMT_MAXP = 10;
constexpr uint32_t GRID_MIN = 48;      // the general copy kernel's pieces of >= GRID_MIN bytes: windows on the source's grid, one work item more per piece
// work items of a piece of `len` bytes in the general copy kernel: a short piece is one, a long one a 16-byte window per item —
// on the source's grid (head window + aligned windows, the last one end-aligned) that is one more than len / 16 rounded up
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr uint32_t piece_items(uint32_t len) {
    return len >= 16u ? ((len + 15u) >> 4) + (len >= GRID_MIN ? 1u : 0u) : (len > 0u ? 1u : 0u);
}
constexpr uint32_t FMT_LIT_BIT = 0x80000000u;
struct FmtPiece {
    uint32_t src;          // byte offset from the file's text base; FMT_LIT_BIT: offset into FMT_LIT instead
    uint16_t dst, len;     // position in the output record, bytes
};
struct FmtTask {
    uint32_t pos;          // offset of the record in its output stream
    uint8_t stream;        // 0 good / 1 bad / 2 overlap, 0xff: not written in this pass
    uint8_t np, n_patch, pad_;
    uint16_t total, items; // bytes of the output record; work items (16-byte windows + short pieces)
    uint32_t patch[6];     // the walk's edits: output position | new byte << 16
    FmtPiece p[FMT_MAXP];
};

// ---- plans: see the layout at fmt_plan_kernel (aqc_fmtcopy.hpp) ---------------------------------------------------------------
constexpr uint32_t PLAN_SKIP = 0xffffffffu, PLAN_OVER = 0x80000000u;
constexpr int PLAN_Q = 6;                    // 16-byte words per plan
constexpr int PLAN_MAXP = 8;
constexpr int GEN_PASSES = 2;                // work items per lane of the general copy kernel (32 lanes per record)

// the plans fmt_copy_whole_kernel takes: one piece of 16..512 bytes from the text — the record's own bytes — with up to four
// byte patches (a pair the correction walk edited is still its own bytes but for those: ~8 % of the records of a 2 x 150 run,
// which used to go through the general kernel, 0.7 of the text step's 4.6 ms)
FMTW_HD bool plan_is_whole(const uint4& q0) {
    return (q0.y & 0xff00ff00u) == 0x100u && ((q0.y >> 16) & 0xffu) <= 4u && !(q0.z & FMT_LIT_BIT) && (q0.w & 0xffffu) >= 16u && (q0.w & 0xffffu) <= 512u;
}

// the six plan words of a record's piece list `t` placed at `pos` of its stream (layout: above); false: the record does not fit a
// plan — more than eight pieces, four patches or 64 work items, or a patch inside a piece of < 16 bytes — q[0] then says PLAN_OVER
// and the caller keeps the full FmtTask in the overflow array
struct PlanWords { uint4 q0, q1, q2, q3, q4, q5; bool inline_ok; };
FMTW_HD PlanWords plan_words(const FmtTask& t, uint32_t pos) {
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    uint4 q0 = zero4, q1 = zero4, q2 = zero4, q3 = zero4, q4 = zero4, q5 = zero4;
    // inline: up to eight pieces, four byte patches (each inside a piece of >= 16 bytes), 64 work items (1 KiB)
    bool inline_ok = t.np <= PLAN_MAXP && t.n_patch <= 4 && t.items <= 32 * GEN_PASSES;
    for (int e = 0; e < (int)t.n_patch && inline_ok; ++e) {
        const int pp = (int)(t.patch[e] & 0xffffu);
        int o = 0;
        for (int k = 0; k < (int)t.np; ++k) {
            if (pp >= o && pp < o + (int)t.p[k].len && t.p[k].len < 16) inline_ok = false;
            o += t.p[k].len;
        }
    }
    if (inline_ok) {
        uint32_t src[PLAN_MAXP], len[PLAN_MAXP], cum[PLAN_MAXP], off[PLAN_MAXP];
        uint32_t ci = 0, doff = 0;
        for (int k = 0; k < PLAN_MAXP; ++k) {
            const bool in = k < (int)t.np;
            src[k] = in ? t.p[k].src : 0u;
            len[k] = in ? (uint32_t)t.p[k].len : 0u;
            off[k] = doff;
            ci += piece_items(len[k]);
            cum[k] = ci;
            doff += len[k];
        }
        q0 = make_uint4(pos, (uint32_t)t.stream | ((uint32_t)t.np << 8) | ((uint32_t)t.n_patch << 16), src[0], len[0] | (len[1] << 16));
        q1 = make_uint4(src[1], src[2], src[3], src[4]);
        q2 = make_uint4(src[5], src[6], src[7], len[2] | (len[3] << 16));
        q3 = make_uint4(len[4] | (len[5] << 16), len[6] | (len[7] << 16), cum[0] | (cum[1] << 8) | (cum[2] << 16) | (cum[3] << 24),
                          cum[4] | (cum[5] << 8) | (cum[6] << 16) | (cum[7] << 24));
        q4 = make_uint4(off[1] | (off[2] << 16), off[3] | (off[4] << 16), off[5] | (off[6] << 16), off[7] | (ci << 16));
        q5 = make_uint4(t.n_patch > 0 ? t.patch[0] : 0u, t.n_patch > 1 ? t.patch[1] : 0u, t.n_patch > 2 ? t.patch[2] : 0u,
                          t.n_patch > 3 ? t.patch[3] : 0u);
    } else q0 = make_uint4(pos, PLAN_OVER | (uint32_t)t.stream, 0, 0);
    return PlanWords{q0, q1, q2, q3, q4, q5, inline_ok};
}

// ---- the rules the copy kernels compute per lane -----------------------------------------------------------------------------------
// Each rule's TEXT stands here once, as a macro: the kernels of aqc_fmtcopy.hpp expand it in place, the functions below wrap the
// same text for the CPU selftest.  (They were tried as functions the kernels call.  Inlined, they give the same instructions in
// another order, and the compiler then schedules and allocates the copy kernels differently; a change for testability alone must
// leave the kernels' instruction streams as they were — tools/isa_identity.py — and text expanded in place does.)
// A macro's arguments are plain names or, where its comment says so, expressions.  Each macro DECLARES variables in the scope it is
// expanded in: the ones named by its arguments and, for some, helpers of fixed names — its comment lists both ("declares: ...").
#if defined(__HIPCC__)
#define FMTW_MIN(a, b) min(a, b)
#define FMTW_MAX(a, b) max(a, b)
#define FMTW_POPC(x) __popc(x)
#else
#define FMTW_MIN(a, b) fmtw_min(a, b)
#define FMTW_MAX(a, b) fmtw_max(a, b)
#define FMTW_POPC(x) __builtin_popcount(x)
inline int fmtw_min(int a, int b) { return a < b ? a : b; }
inline int fmtw_max(int a, int b) { return a > b ? a : b; }
#endif

// A record that goes out as its own bytes (copy_whole_tasks): `len` = 16..512 bytes at source address `s0`, 32 lanes.
// in: len, s0, lane32.  declares: int nw — the number of windows; int off — lane32's offset into the record (lanes >= nw have no
// window).  (a, nwa, grid live in a block of their own.)
// round 6: the windows stand on the 16-byte grid of the SOURCE (on the destination's they measured slower than with no
// grid at all — profiles/r06_copy_window_grid.txt): lane 0 takes the record's first 16 bytes wherever they stand, lane k >= 1 the
// k-th aligned window behind them, the last window end-aligned as before.  A wave's load instruction then touches every 64-byte
// line once (off the grid each quad of lanes straddles two).  A record of > 496 bytes off the grid would take 33 windows: it
// keeps the plain ones
#define FMTW_WHOLE_WINDOW_GRID(len, s0, lane32, nw, off)                                  \
    int nw = (len + 15) >> 4;                                                             \
    int off = 16 * lane32;                                                                \
    {                                                                                     \
        const int a = (16 - (int)((uintptr_t)s0 & 15u)) & 15;                             \
        const int nwa = 1 + ((len - a + 15) >> 4);                                        \
        const bool grid = a != 0 && nwa <= 32;                                            \
        nw = grid ? nwa : nw;                                                             \
        off = grid && lane32 ? a + 16 * (lane32 - 1) : off;                               \
    }
// ... and the last window (every lane behind it, too) aligned to the record's end.  in: len; changes: off; declares nothing
#define FMTW_WHOLE_WINDOW_END(len, off) off = FMTW_MIN(off, len - 16);

// What a lane of the general copy kernel reads from the plan at `pb` (the six words, 96 bytes, 16-byte aligned).
// in: pb.  declares: const uint2 cumw — the cumulative work items of pieces 0..7, a byte each (q3.z, q3.w); const uint32_t q4w —
// q4.w: the record's work items in its upper half
#define FMTW_PLAN_HEAD(pb, cumw, q4w)                                                     \
    const uint2 cumw = *reinterpret_cast<const uint2*>(pb + 56);                          \
    const uint32_t q4w = *reinterpret_cast<const uint32_t*>(pb + 76);
// ... and the piece work item `item` lies in.
// in: pb, cumw (FMTW_PLAN_HEAD's), cum — cumw as ONE 64-bit value, ((unsigned long long)cumw.y << 32) | cumw.x, built by the caller
// once per plan —, item, on (the item exists; else piece 0).
// declares: int k — the piece's number; const int first_item — the work item it starts with; const int lk — its length; const int
// dst_off — its offset in the output record; const uint32_t sk — its source; and two helpers of fixed names: const uint32_t rep (the
// item's number in every byte) and const int dst_rd (the offset as read, before piece 0's is chosen) — once per scope, therefore.
// my piece: the pieces whose cumulative item count I am at or beyond (bytes 0..6; counts and items are < 128)
#define FMTW_PLAN_PIECE(pb, cumw, cum, item, on, k, first_item, lk, dst_off, sk)                                                       \
    const uint32_t rep = (item * 0x01010101u) | 0x80808080u;                                                                           \
    int k = FMTW_POPC((rep - cumw.x) & 0x80808080u) + FMTW_POPC((rep - cumw.y) & 0x00808080u);                                         \
    k = on ? k : 0;                                                                                                                    \
    const int first_item = (int)(((cum << 8) >> (8 * k)) & 0xffu);                                                                     \
    const int lk = (int)*reinterpret_cast<const uint16_t*>(pb + (k < 2 ? 12 : 40) + 2 * k);      /* lengths: q0.w | q2.w, q3.x, q3.y */ \
    const int dst_rd = (int)*reinterpret_cast<const uint16_t*>(pb + 62 + 2 * FMTW_MAX(k, 1));    /* output offsets of pieces 1..7: q4 */ \
    const int dst_off = k == 0 ? 0 : dst_rd;                                                     /* (read, then chosen: no branch around the read) */ \
    const uint32_t sk = *reinterpret_cast<const uint32_t*>(pb + (k == 0 ? 8 : 12 + 4 * k));      /* sources: q0.z | q1, q2.xyz */

// A piece of the general copy kernel: `lk` bytes from source `sk` (FMT_LIT_BIT: a literal) of a text whose base address is `tbase`
// (its low 32 bits, an expression), `d` (an expression): the work item's number within the piece.
// in: lk, tbase, sk, d.  declares: int off — the offset into the piece of that work item's window.  (tb, a, grid live in a block of
// their own.)  A long piece: its 16-byte window, the last one aligned to the piece's end; a short piece (< 16 bytes): all of it, offset 0.
// (round 6) a piece of >= GRID_MIN bytes has one item more (piece_items): its first window where the piece starts, the
// others on the 16-byte grid of the SOURCE, so that a load instruction touches each 64-byte line once
#define FMTW_GEN_WINDOW(lk, tbase, sk, d, off)                                                                     \
    int off = 16 * (d);                                                                                            \
    {                                                                                                              \
        const uint32_t tb = tbase;                                                                                 \
        const int a = (int)((0u - (tb + sk)) & 15u);                                                               \
        const bool grid = lk >= (int)GRID_MIN && !(sk & FMT_LIT_BIT) && off;                                       \
        off += (a - 16) & -(int)grid;                /* (arithmetic, not a branch around eight instructions) */   \
    }                                                                                                              \
    off = lk >= 16 ? FMTW_MIN(off, lk - 16) : 0;

// the same rules as functions
struct WholeWin { int nw, off; };
FMTW_HD WholeWin whole_window(int len, const uint8_t* s0, int lane32) {
    FMTW_WHOLE_WINDOW_GRID(len, s0, lane32, nw, off)
    FMTW_WHOLE_WINDOW_END(len, off)
    return WholeWin{nw, off};
}
FMTW_HD int gen_window_off(int lk, uint32_t tbase, uint32_t sk, int d) {
    FMTW_GEN_WINDOW(lk, tbase, sk, d, off)
    return off;
}
struct PlanPiece { int k, first_item, lk, dst_off; uint32_t sk, items; };
FMTW_HD PlanPiece plan_piece_of(const uint8_t* pb, uint32_t item) {
    FMTW_PLAN_HEAD(pb, cumw, q4w)
    const uint32_t items = q4w >> 16;
    const unsigned long long cum = ((unsigned long long)cumw.y << 32) | cumw.x;
    const bool on = item < items;
    FMTW_PLAN_PIECE(pb, cumw, cum, item, on, k, first_item, lk, dst_off, sk)
    return PlanPiece{k, first_item, lk, dst_off, sk, items};
}

}  // namespace aqc
