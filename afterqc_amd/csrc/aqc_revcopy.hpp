// aqc_revcopy.hpp — the reversed copy of the merged-read writer (--store_merged, fmt_merged_kernel in aqc_fmtcopy.hpp): p bytes
// of read 2 go out back to front, the bases complemented (util.reverseComplement: COMP, anything else -> 'N'), the qualities
// as they are.
//
//   windows  as the forward copy kernels: 16 bytes per work item.  A piece of p >= 16 bytes has its first window where the
//            piece starts, the others on the 16-byte grid of the SOURCE (a wave's load touches each 64-byte line once), the last
//            one end-aligned; windows that overlap write the same bytes.  A piece of 1 .. 15 bytes is ONE window that ENDS with
//            the piece (source offset p - 16 < 0: it reads up to 15 bytes in front of the piece — text, or the buffer's front
//            pad), so that after the reversal the piece's bytes are the LOW p bytes of the window and go out as 8 + 4 + 2 + 1.
//   place    the window at source offset o lands, reversed, at destination offset p - 16 - o.
//   bytes    a dword is reversed by one v_perm (selector 0x00010203), the four dwords swap places.  The complement works on
//            four bytes at once: the 3-bit code (c >> 1) & 7 is A0 C1 T2 G3 N7 for either case, one v_perm looks the
//            complement up, a second one the letter the code stands for — a byte that is not that letter (or is 'n', which
//            COMP does not hold) becomes 'N'; the case bit 0x20 is carried over.
//
// Everything here is __host__ __device__: tests/native/revcopy_selftest.cpp includes this header without HIP and deals the
// windows out by plain loops, over every source and destination alignment.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define REVC_HD __host__ __device__ __forceinline__
#else
#define REVC_HD inline
#endif

namespace aqc {

struct RevWin { uint32_t x, y, z, w; };      // 16 bytes, little-endian dwords (uint4 without HIP)

// v_perm_b32 for selectors 0 .. 7: result byte i = byte sel[i] of {hi : lo} (0 .. 3 from lo, 4 .. 7 from hi)
REVC_HD uint32_t revc_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7u))) & 0xffu) << (8 * i);
    return r;
#endif
}

REVC_HD uint32_t revc_bswap(uint32_t d) { return revc_perm(0u, d, 0x00010203u); }

// the 16 bytes back to front
REVC_HD RevWin revc_reverse(const RevWin& v) { return RevWin{revc_bswap(v.w), revc_bswap(v.z), revc_bswap(v.y), revc_bswap(v.x)}; }

// comp_or_n (aqc_prim.hpp) of four bytes
REVC_HD uint32_t revc_comp4(uint32_t d) {
    const uint32_t code = (d >> 1) & 0x07070707u;
    const uint32_t comp = revc_perm(0x4e000000u, 0x43414754u, code);                 // T G A C . . . N
    const uint32_t canon = revc_perm(0x4e000000u, 0x47544341u, code);                // A C T G . . . N
    const uint32_t is_n = code & (code >> 1) & (code >> 2) & 0x01010101u;            // code 7
    const uint32_t lower = d & 0x20202020u & ~(is_n << 5);                           // ('n' is not in COMP: no case bit for it)
    const uint32_t x = d ^ (canon | lower);                                          // 0 where the byte is in COMP
    const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;       // 0x80 per foreign byte
    const uint32_t foreign = nz | (nz - (nz >> 7));                                  // 0xff per foreign byte
    return ((comp | lower) & ~foreign) | (0x4e4e4e4eu & foreign);
}

REVC_HD RevWin revc_comp16(const RevWin& v) { return RevWin{revc_comp4(v.x), revc_comp4(v.y), revc_comp4(v.z), revc_comp4(v.w)}; }

// work items of a reversed piece of p bytes whose source starts `a` bytes before a 16-byte boundary (a = -address & 15)
REVC_HD uint32_t revc_items(uint32_t p, uint32_t a) {
    if (p < 16u) return p ? 1u : 0u;
    return a ? 1u + ((p - a + 15u) >> 4) : (p + 15u) >> 4;
}

// source offset of work item `item` (< revc_items): in [0, p - 16], or p - 16 < 0 for the one window of a short piece
REVC_HD int revc_src_off(uint32_t p, uint32_t a, uint32_t item) {
    if (p < 16u) return (int)p - 16;
    const uint32_t off = (a && item) ? a + 16u * (item - 1u) : 16u * item;
    return (int)(off < p - 16u ? off : p - 16u);
}

// destination offset of the window read at source offset `off`: 0 for a short piece, whose low p bytes are the piece
REVC_HD int revc_dst_off(uint32_t p, int off) { return (int)p - 16 - off; }

}  // namespace aqc
