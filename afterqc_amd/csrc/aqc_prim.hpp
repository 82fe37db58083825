// aqc_prim.hpp — what more than one stage of the gfx950 device code uses, one copy of each: the wave size and lane id, loads / stores
// that name their address space, the 16-byte unaligned load / store, the wave-wide reductions and scans, and the complement of a base.
// It depends on no other header of the project and defines no kernel; every stage header (aqc_record / aqc_qcstat / aqc_seams /
// aqc_fast / aqc_textin / aqc_fmt / aqc_fmtcopy / aqc_census / aqc_gzdev) includes it for these and includes another stage's header
// only for what is that stage's own — and only where both belong to the same C-API unit (aqc_ctx.hpp): a header that defines a
// non-template kernel is included by one unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aqc {

constexpr int WAVE = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }

// ---- loads / stores that SAY the pointer is global memory ---------------------------------------------------------------------------
// A pointer that reached a lane through LDS, v_readlane or a select between arrays is "generic" to the compiler: it emits flat_load /
// flat_store, which count on lgkmcnt as well as vmcnt — every wait for an LDS read behind one then waits for the memory round trip
// too (the general copy kernel's four window loads and the k-mer kernel's prefetch were serialised that way, rounds 1 - 5).  These
// helpers cast to address space 1 first: global_load / global_store at any alignment, vmcnt only.
#define AQC_GLOBAL_AS __attribute__((address_space(1)))
typedef uint32_t aqc_u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t aqc_u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t aqc_u32_u __attribute__((aligned(1)));
typedef uint16_t aqc_u16_u __attribute__((aligned(1)));
__device__ __forceinline__ uint4 gload_u128(const uint8_t* p) {
    const aqc_u32x4_u t = *(const AQC_GLOBAL_AS aqc_u32x4_u*)p;
    return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ uint32_t gload_u32(const uint8_t* p) { return *(const AQC_GLOBAL_AS aqc_u32_u*)p; }
__device__ __forceinline__ void gstore_u128(uint8_t* p, uint4 v) {
    aqc_u32x4_u t;
    t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    *(AQC_GLOBAL_AS aqc_u32x4_u*)p = t;
}
__device__ __forceinline__ void gstore_u64(uint8_t* p, uint32_t a, uint32_t b) {
    aqc_u32x2_u t;
    t.x = a; t.y = b;
    *(AQC_GLOBAL_AS aqc_u32x2_u*)p = t;
}
__device__ __forceinline__ void gstore_u32(uint8_t* p, uint32_t a) { *(AQC_GLOBAL_AS aqc_u32_u*)p = a; }
__device__ __forceinline__ void gstore_u16(uint8_t* p, uint16_t a) { *(AQC_GLOBAL_AS aqc_u16_u*)p = a; }
__device__ __forceinline__ void gstore_u8(uint8_t* p, uint8_t a) { *(AQC_GLOBAL_AS uint8_t*)p = a; }

// 16 bytes from / to an arbitrarily aligned address (generic pointer): one dwordx4 load / store
__device__ __forceinline__ uint4 load16u(const uint8_t* p) {
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void store16u(uint8_t* p, uint4 v) { __builtin_memcpy(p, &v, 16); }

// ---- wave-wide sum ---------------------------------------------------------------------------------------------------------------------
// wave_sum_dpp  is right in UNIFORM control flow only (all 64 lanes active) and returns a wave-uniform result: four DPP steps inside
//               the rows of 16 lanes (lane ^ 1, lane ^ 2, half-row mirror, row mirror), then the four row results through v_readlane
//               and scalar arithmetic.  Code that runs under a lane mask sums with __shfl_xor at its own site instead: six ds_bpermute
//               round trips through the LDS crossbar, and six lane-address registers alive for the whole kernel.
template <int CTRL>
__device__ __forceinline__ int dpp_move(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
__device__ __forceinline__ int wave_sum_dpp(int v) {
    v += dpp_move<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_move<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_move<0x141>(v);      // row_half_mirror
    v += dpp_move<0x140>(v);      // row_mirror
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) + (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
// wave-wide max, the DPP form (uniform control flow, wave-uniform result)
__device__ __forceinline__ int wave_max_i(int v) {
    v = max(v, dpp_move<0xB1>(v));
    v = max(v, dpp_move<0x4E>(v));
    v = max(v, dpp_move<0x141>(v));
    v = max(v, dpp_move<0x140>(v));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// Inclusive prefix sum / running maximum over the 64 lanes, in uniform control flow: four DPP row_shr steps scan the rows of 16
// lanes (lanes shifted in from outside a row read 0), the three row totals come through v_readlane.
template <int CTRL>
__device__ __forceinline__ int dpp_shr0(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int wave_incl_sum(int v, int lane) {
    v += dpp_shr0<0x111>(v);
    v += dpp_shr0<0x112>(v);
    v += dpp_shr0<0x114>(v);
    v += dpp_shr0<0x118>(v);
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
    const int row = lane >> 4;
    return v + (row >= 1 ? t0 : 0) + (row >= 2 ? t1 : 0) + (row >= 3 ? t2 : 0);
}
__device__ __forceinline__ int wave_incl_max(int v, int lane) {      // (values >= 0)
    v = max(v, dpp_shr0<0x111>(v));
    v = max(v, dpp_shr0<0x112>(v));
    v = max(v, dpp_shr0<0x114>(v));
    v = max(v, dpp_shr0<0x118>(v));
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
    const int row = lane >> 4;
    return max(max(v, row >= 1 ? t0 : 0), max(row >= 2 ? t1 : 0, row >= 3 ? t2 : 0));
}

// exchange a value with the partner lane (lane ^ 1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ int xchg(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }

// Inclusive prefix sum over the 64 lanes by __shfl_up (six ds_bpermute steps), for the values the DPP scan above does not take: 64-bit
// ones, and sums of the gzip / census stages that were written this way and whose instruction streams stay as they are.  It replaced
// the hand-written loops of block_excl_scan, poly_census_kernel, gz_block_excl_scan and gz_encode_wave_kernel with identical
// instructions (profiles/r09_isa_identity.txt); the two loops in aqc_gunzip_dev.hpp stay written out: that header stands alone.
template <class T>
__device__ __forceinline__ T wave_incl_sum_shfl(T v, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T o = __shfl_up(v, d, WAVE);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive prefix of one value per thread over a workgroup of 64 .. 256 threads; `total` = sum over the workgroup
constexpr int BLOCK_SCAN_WAVES = 4;
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* lds /* [4] */,
                                                              unsigned long long& total) {
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const unsigned long long inc = wave_incl_sum_shfl(v, lane);
    __syncthreads();                       // lds may still be read by the previous call
    if (lane == WAVE - 1) lds[wave] = inc;
    __syncthreads();
    unsigned long long base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK_SCAN_WAVES; ++w) {
        if (w >= (int)(blockDim.x / WAVE)) break;
        const unsigned long long t = lds[w];
        if (w < wave) base += t;
        total += t;
    }
    return base + inc - v;
}

// ---- the complement of a base (the verdict kernels, the seams and the k-mer kernel's reverse complement) ------------------------------
// util.py:27 COMP; returns 0 for bytes outside the table (KeyError upstream)
__device__ __forceinline__ uint8_t comp_strict(uint8_t c) {
    switch (c) {
        case 'A': return 'T';
        case 'T': return 'A';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'a': return 't';
        case 't': return 'a';
        case 'c': return 'g';
        case 'g': return 'c';
        case 'N': return 'N';
        default: return 0;
    }
}

// util.py:47-50 reverseComplement's per-base rule: unknown -> 'N'
__device__ __forceinline__ uint8_t comp_or_n(uint8_t c) {
    uint8_t r = comp_strict(c);
    return r ? r : (uint8_t)'N';
}

}  // namespace aqc
