// aqc_fast_args.hpp — what the host sees of the lane-per-read verdict kernel (aqc_fast.hpp): the layout of a wave's LDS rows (the
// batch size PPW comes from it) and the kernel's argument structs.  No device code: a translation unit that only sizes a launch or a
// fused placement by PPW includes this header and not the kernel.
#pragma once
#include <stdint.h>

#include "afterqc_hip.h"
#include "aqc_batch.hpp"

namespace aqc {

template <int NW, bool PAIRED, bool FUSE = false>
struct FastWaveLds {
    static constexpr int PPW = PAIRED ? 32 : 64;               // records per wave batch
    static constexpr int GUARD = (PAIRED ? 4 : 2) * NW;        // 5 zero words behind the planes
    static constexpr int LQ0 = GUARD + 5;                      // read 1's low-quality bit plane: 16 bits per chunk
    // the record's descriptor lives in its row too: one row address serves the planes and these (immediate offsets)
    static constexpr int D_O1 = LQ0 + (NW + 1) / 2, D_L1 = D_O1 + 1, D_Q1 = D_O1 + 2, D_O2 = D_O1 + 3, D_L2 = D_O1 + 4, D_Q2 = D_O1 + 5;
    static constexpr int D_EXO = D_O1 + 6, D_LQ = D_O1 + 7;    // alphabet verdict (non-zero: defer), read 1's low-quality count
    // FUSE (the kernel also places every record and copies the whole ones): where each mate's record starts in its text
    // (bit 31: all four lines end right at their '\n')
    static constexpr int D_N1 = D_O1 + 8, D_N2 = D_O1 + 9;
    static constexpr int STRIDE = (D_O1 + (FUSE ? 10 : 8)) | 1;   // odd: conflict-free lane-strided access
    uint32_t planes[PPW][STRIDE];
    uint8_t stage[16 * NW + 16];
    // FUSE: the batch whose records are copied one batch later (by then its predecessors have long published their sums): per
    // record and file the first byte in the text | copied here << 31, and its length | offset inside the batch's bytes << 16
    uint32_t pend[FUSE ? 2 : 1][FUSE ? 4 * PPW : 1];
};

// The kernel's arguments, one struct.  The hot loop keeps what it uses in every batch in scalar registers (K.field); what
// only rare branches need — the bubble circles and name fields, the trim amounts, the deferral queue, the device status
// word, the statistics arrays — is read from the kernarg segment where it is used (R->field, an s_load): held in SGPRs
// across the loop those ~40 values pushed the kernel past the 102 it has, and the spill code (v_writelane / v_readlane
// + hazard nops) was ~6 % of all vector instructions issued.
// FUSE: what the verdict kernel needs to place every record of the chunk in its output stream and to copy the good records that
// go out as their own bytes itself.  Batches are committed in index order: a batch publishes the bytes it adds to
// the four streams (good / bad of either file) and looks back over its predecessors' (decoupled look-back, as text_index_kernel).
struct FuseArgs {
    const uint32_t *name_off1, *name_off2;       // where each record starts in its file's text
    uint8_t *out1, *out2;                        // the good streams
    uint32_t *fstate1, *fstate2;                 // per record and file: offset inside its batch's share of its stream (16 bits) | FUSE_WHOLE (its own
                                                 // bytes, written here) | FUSE_PATCH (... but for the walk's byte patches, which the plan pass stores)
    unsigned long long* state;                   // [2 * batches]: flag (2 bits) | good1 (31) | good2 (31), flag | bad1 | bad2: the batch's sums (A), then
                                                 // — final — the streams' bytes up to and including the batch (P): the plan pass reads those
    unsigned int* ticket;                        // rounds handed out (a round = WPBT consecutive batches)
    int* abort;                                  // != 0: this placement is void — a deferred pair, a record that is not contiguous text, a
                                                 // look-back that ran out of patience: the host formats the chunk the other way
    unsigned long long* totals;                  // [4] bytes of good1, good2, bad1, bad2
};
constexpr uint32_t FUSE_WHOLE = 0x80000000u, FUSE_POS = 0x7fffffffu, FUSE_PATCH = 0x40000000u;
constexpr unsigned long long FUSE_FLAG_A = 1ull << 62, FUSE_FLAG_P = 2ull << 62;

struct FastArgs {
    DevBatch fb;
    aqc_config cfg;
    DevCircles circ;
    aqc_result* results;
    DevStats st;
    uint64_t accum_limit;
    uint32_t* deferred;
    unsigned int* n_deferred;
    FuseArgs fz;
};
typedef const FastArgs __attribute__((address_space(4))) * FastArgsRare;

// CUT: the quality cut is on (aqc_qcut.hpp): the kernel's arguments continue with the view array of the cut pass (the mates of a record side by side), and the trim
// stage slices every read by its own view after the fixed trim.  Only those instances take the longer argument struct: the others
// take what they always took and come out of the compiler with the same instructions (profiles/r16_qcut.txt).
struct FastCutArgs : FastArgs {
    const uint32_t* cut;                       // c0 | c1 << 16 of the trimmed reads: [2 r], [2 r + 1] for read 1 / 2 of pair r, [r] single-end
};
typedef const FastCutArgs __attribute__((address_space(4))) * FastCutArgsRare;

}  // namespace aqc
