// aqc_viewpass.hpp — what a view pass is: a kernel in front of the verdict kernel that decides, for every mate of a batch, which
// part [c0, c1) of its trimmed line the verdict kernels see, and leaves that as one word per mate and record in Slot::cut.  Three
// passes exist, the quality cut (aqc_qcut.hpp), the adapter pass (aqc_adapter.hpp) and the poly-tail pass (aqc_polytail.hpp); a later
// one takes the views of the earlier ones and narrows them.  The adapter census (aqc_adpcensus.hpp) writes no view but is a group-per-read
// kernel over the same lines.  What all are made of stands here once, each pass's header holds its own middle.
//
//   view     c0 | c1 << 16, relative to the line behind trim(); VIEW_ALL (0, 0xffff) is the view of a mate nothing has cut.  The
//            mates of a record lie side by side: mate k of record r at [r * n_mates + k].  The verdict kernels apply it to every
//            string by the string's own length (view_apply): a record whose quality line is not as long as its sequence line is
//            sliced the python way, like upstream's trim().
//   groups   G neighbouring lanes (8, 16, 32 or 64, by the slot's longest line) own one read of up to 16 * G bytes; a workgroup of
//            four waves owns 256 / G consecutive records and takes read 1, then read 2 of each (read 2's counts need read 1's
//            outcome).  The grid strides over the records.
//   load     one 16-byte load per lane at the line's own alignment (the arenas are padded: aqc_batch), of which vp_nvalid bytes
//            belong to the line.  The line's address is formed only where there is a line: never for a record behind the batch's
//            last, never from a length word that carries the LEN_IRR mark.
//   line     the passes that read the SEQUENCE line (adapter, poly-tail) take a mate as a ViewMate; vp_line gives where the line lies
//            and how long it is behind trim() and the view that comes in, view_end the view the mate leaves with.  The quality cut
//            reads quality lines through aqc_batch and keeps its own arguments.
//   row     what the lanes wrote into the group's LDS row the whole group reads after vp_publish_row (a group is part of one wave).
//   out      the group's first lane writes the view, raises AQC_ERR_READ_TOO_LONG for a line no group of G lanes takes, and counts
//            "reads made shorter, bases removed" per mate (vp_count: read 2 only while read 1 keeps 5 bases or more, and only records
//            in front of accum_limit); vp_flush<N> adds the workgroup's counts to the context's — four of a view pass, 17 of the census.
//
// The record loop and the mate loop themselves stand in each kernel: as a function that takes the kernel's middle as a callable
// the counters leave the registers, as they do in a struct — the closure holds them by reference: 32 bytes of scratch in the cut
// kernel, 4 KiB more LDS in the adapter kernel (profiles/r18_viewpass.txt).  A kernel reads: frame (rows, counters, the two loops), its own middle, frame (view out, too long,
// counts, flush).
//
// Host-includable without HIP: tests/native/qcut_selftest.cpp, adapter_selftest.cpp and polytail_selftest.cpp take the per-read functions from here with a
// plain C++ compiler and deal the lanes of a group out by loops.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VP_HD __host__ __device__ __forceinline__
#else
#define VP_HD inline
#endif

namespace aqc {

constexpr int VP_MAX_LEN = 1000;            // AQC_MAX_READ_LEN (afterqc_hip.h), restated: the self-tests include nothing else
constexpr int VP_THREADS = 256;             // a workgroup of a view pass: four waves
constexpr int vp_cap(int G) { return 16 * G; }                  // longest line a group of G lanes takes
constexpr int vp_groups(int G) { return VP_THREADS / G; }       // records per workgroup and round

VP_HD int vp_min(int a, int b) { return a < b ? a : b; }
VP_HD int vp_max(int a, int b) { return a > b ? a : b; }

// ---- the view word
constexpr uint32_t VIEW_ALL = 0xffff0000u;
VP_HD uint32_t view_word(int c0, int c1) { return (uint32_t)c0 | ((uint32_t)c1 << 16); }
VP_HD int view_c0(uint32_t view) { return (int)(view & 0xffffu); }
VP_HD int view_c1(uint32_t view) { return (int)(view >> 16); }

// trim() of preprocesser.py:19-28 on a string of `len` bytes -> (start, length)
VP_HD void vp_trim(int len, int front, int tail, int& st, int& nl) {
    const int end = tail > 0 ? vp_max(len - tail, 0) : len;
    st = vp_min(front, len);
    nl = vp_max(end - st, 0);
}

// s[c0:c1] of a string of `len` bytes, python slice semantics (0 <= c0 <= c1) -> (start, length)
VP_HD void vp_slice(int len, int c0, int c1, int& st, int& nl) {
    st = vp_min(c0, len);
    nl = vp_max(vp_min(c1, len) - st, 0);
}
VP_HD void view_slice(int len, uint32_t view, int& st, int& nl) { vp_slice(len, view_c0(view), view_c1(view), st, nl); }

// trim() and then the view on a string of `len` bytes: moves (a, l), the view the caller holds of it
VP_HD void view_apply(int& a, int& l, int front, int tail, uint32_t view) {
    int st, nl, st2, nl2;
    vp_trim(l, front, tail, st, nl);
    view_slice(nl, view, st2, nl2);
    a += st + st2;
    l = nl2;
}

// The view a mate leaves a sequence-line pass with: the one it came with — or, where the pass cut, that one ended at `kept` bytes
// of the line.  The pass says whether it cut (the adapter pass: it has a match; the poly-tail pass: end < n) instead of handing n in:
// as view_end(view_in, n, kept) testing `kept >= n` the adapter kernel's select compares kept with n where it compared p with
// ADP_NONE, and six instructions of all four instances change places (profiles/r21_viewpass_frame.txt).
VP_HD uint32_t view_end(uint32_t view_in, bool cut, int kept) {
    if (!cut) return view_in;
    const int c0 = view_c0(view_in);
    return view_word(c0, c0 + kept);
}

// how many of lane g's 16 bytes belong to a line of n bytes
VP_HD int vp_nvalid(int n, int g) { return vp_min(vp_max(n - 16 * g, 0), 16); }

// true when the condition holds in any lane of the wave / of the lane's group of G (the self-tests' single lane: in the lane)
VP_HD bool vp_wave_any(bool c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(c) != 0ull;
#else
    return c;
#endif
}
template <int G>
VP_HD bool vp_group_any(bool c, int g) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long b = __ballot(c);
    if (G == 64) return b != 0ull;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    return ((b >> (lane - g)) & ((1ull << (G & 63)) - 1ull)) != 0ull;
#else
    (void)g;
    return c;
#endif
}

}  // namespace aqc

#if defined(__HIPCC__)
#include <type_traits>

#include "afterqc_hip.h"
#include "aqc_batch.hpp"
#include "aqc_prim.hpp"

namespace aqc {

static_assert(VP_MAX_LEN == AQC_MAX_READ_LEN, "a view pass takes every read the verdict kernels take");

// min / max / OR over the G lanes of a group (every lane of the wave runs it)
template <int G>
__device__ __forceinline__ int vp_group_min(int v) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) v = min(v, __shfl_xor(v, d, WAVE));
    return v;
}
template <int G>
__device__ __forceinline__ int vp_group_max(int v) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) v = max(v, __shfl_xor(v, d, WAVE));
    return v;
}

template <int G>
__device__ __forceinline__ uint32_t vp_group_or(uint32_t v) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) v |= (uint32_t)__shfl_xor((int)v, d, WAVE);
    return v;
}

// lane g's 16 bytes of the line at `line`; nothing is read, and `line` may be NULL, where none of them belongs to the line
__device__ __forceinline__ uint4 vp_load16(const uint8_t* line, int nvalid, int g) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (nvalid > 0) v = load16u(line + 16 * g);
    return v;
}

// what the group's lanes wrote into its LDS row, readable by all of them
__device__ __forceinline__ void vp_publish_row() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// ... and every lane is done reading it: the next line may overwrite it
__device__ __forceinline__ void vp_release_row() { __builtin_amdgcn_wave_barrier(); }

// a line no group of G lanes takes: the pass leaves it alone, and its first lane raises the error
template <int G>
__device__ __forceinline__ bool vp_too_long(int n) { return n > vp_cap(G) || n > AQC_MAX_READ_LEN; }
__device__ __forceinline__ void vp_raise_too_long(int* status) { atomicCAS(status, 0, AQC_ERR_READ_TOO_LONG); }

// what a sequence-line pass takes of one mate: its sequence lines and its fixed trim (aqc_config::trim_front / trim_front2, ...)
struct ViewMate {
    const uint8_t* seq;
    const uint32_t *off, *len;
    int32_t trim_front, trim_tail;
};
// The line of mate M of record `rec`: n bytes from `start` of its sequence line, behind trim() and the view vin that comes in
// (view_in[vi]; NULL: VIEW_ALL).  Nothing is left of a record behind the batch's last (!have) and of a line no group of G lanes takes.
// The length is the length word's, its LEN_IRR mark taken off; the address, M.seq + M.off[rec] + start, the kernel forms where a lane holds bytes.
struct ViewLine { bool too_long; uint32_t vin; int start, n; };
template <int G>
__device__ __forceinline__ ViewLine vp_line(const ViewMate& M, uint64_t rec, bool have, const uint32_t* view_in, uint32_t vi) {
    int len = have ? (int)(M.len[rec] & LEN_MASK) : 0;
    const bool too_long = vp_too_long<G>(len);
    if (!have || too_long) len = 0;
    uint32_t vin = VIEW_ALL;
    if (have && view_in) vin = view_in[vi];
    int t0, tl, s0, n;
    vp_trim(len, M.trim_front, M.trim_tail, t0, tl);
    view_slice(tl, vin, s0, n);
    return ViewLine{too_long, vin, t0 + s0, n};
}

// The group's first lane, mate k left with `kept` of `before` bases: reads made shorter and bases removed, [2 k] and [2 k + 1].
// counted: the record lies in front of accum_limit, and — for read 2 — read 1 left the trim stage with 5 bases or more
// (vp_read1_kept: read 2 is trimmed and cut only then, else the pair is gone).  A kernel's mate loop reads
//     vp_count(cnt, k, rec < K.accum_limit && r1_kept, before, kept);
//     if (k == 0) r1_kept = vp_read1_kept(kept);
// cnt is a plain local array of the kernel and these are free functions: in a struct the counts leave the registers.  The flag's
// update stays in the kernel: taken into vp_count, by reference or as its result, two scalar moves in front of the record loop
// change places in all eight instances (profiles/r18_viewpass.txt).
__device__ __forceinline__ void vp_count(uint32_t (&cnt)[4], int k, bool counted, int before, int kept) {
    if (counted && kept < before) { cnt[2 * k] += 1u; cnt[2 * k + 1] += (uint32_t)(before - kept); }
}
__device__ __forceinline__ bool vp_read1_kept(int kept) { return kept >= 5; }

// the N counts of the groups' first lanes -> the workgroup's (tot: zeroed by the kernel before its first barrier) -> stats: four of a
// view pass, the census's 17.  The caller asks `if (K.stats)`: with the test in here the compiler inverts the branch around the flush.
template <int N>
__device__ __forceinline__ void vp_flush(const uint32_t (&cnt)[N], unsigned long long (&tot)[N], unsigned long long* stats, int g) {
    if (g == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (cnt[j]) atomicAdd(&tot[j], (unsigned long long)cnt[j]);
    }
    __syncthreads();
    if (threadIdx.x < N && tot[threadIdx.x]) atomicAdd(&stats[threadIdx.x], tot[threadIdx.x]);
}

// Host side: the grid of a pass over n records (at most 16 workgroups per CU, the rest by the stride) and the <G> instance for G
// lanes per read.  launch(std::integral_constant<int, G>, grid, block) names the kernel.
template <class Launch>
inline void vp_dispatch(int G, uint64_t n, int n_cu, Launch&& launch) {
    uint64_t blocks = (n + vp_groups(G) - 1) / vp_groups(G);
    const uint64_t cap = (uint64_t)n_cu * 16;
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(VP_THREADS);
    if (G == 8) launch(std::integral_constant<int, 8>{}, grid, block);
    else if (G == 16) launch(std::integral_constant<int, 16>{}, grid, block);
    else if (G == 32) launch(std::integral_constant<int, 32>{}, grid, block);
    else launch(std::integral_constant<int, 64>{}, grid, block);
}

}  // namespace aqc
#endif
