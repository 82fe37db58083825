// polyX flowcell census of the debubble pre-pass (bubbleprocesser.py:348-397): per framed read countPoly, and for the
// reads it finds the Illumina name fields of statFileFastq.  Lane per record; the hits leave compacted (one atomic per
// workgroup), in no particular order: the host restores record order from aqc_census_hit::index.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"
#include "aqc_prim.hpp"
#include "aqc_batch.hpp"      // LEN_MASK: the length words of a framed chunk
#include "aqc_textin.hpp"     // the text-in stage's own: its workgroup size (TXT_BLOCK) and the character classes of framing (is_space, is_digit)

namespace aqc {

// countPoly (bubbleprocesser.py:385-397): A, T, C, G in that order, the first base p with p * K in the read; count is the
// length of the first run of p that is at least K long.  Every maximal run of equal bytes is seen once, where it ends; the
// first run of >= K of each base is kept, and A / T / C / G decide at the end.  16 bytes per step from aligned loads: per
// dword x = w ^ (w shifted by one byte) has a zero byte exactly where base i equals base i + 1; the pairs outside
// [first, last) of the read are forced unequal, so nothing before or behind the read joins a run.  With K >= 5 only the
// run that ends at the dword's first unequal pair can be long enough (a run that starts and ends inside 4 bytes has at
// most 3 bases): ctz / clz of x carry the run across dwords.  K < 5 walks each unequal pair of the dword.
struct PolyRuns {
    int cA = 0, cT = 0, cC = 0, cG = 0;
    __device__ __forceinline__ void note(uint32_t c, int len) {
        if (c == 'A' && !cA) cA = len;
        else if (c == 'T' && !cT) cT = len;
        else if (c == 'C' && !cC) cC = len;
        else if (c == 'G' && !cG) cG = len;
    }
};

__device__ __forceinline__ uint32_t census_mask_bytes(int64_t k) {       // bytes [0, k) of a dword, k clamped to 0..4
    const int c = k < 0 ? 0 : (k > 4 ? 4 : (int)k);
    return (uint32_t)((1ull << (8 * c)) - 1ull);
}

__device__ __forceinline__ void count_poly(const uint8_t* __restrict__ seq, int len, int K, uint8_t& base, int& count) {
    base = 0;
    count = 0;
    if (len <= 0) return;
    const uintptr_t lo = (uintptr_t)seq, hi = lo + (uintptr_t)len - 1;   // pairs (i, i + 1) count for lo <= i < hi
    uintptr_t a = lo & ~(uintptr_t)15;
    // two blocks in registers and the third on its way: the load of a step is not waited for in that step
    uint4 cur = *reinterpret_cast<const uint4*>(a);
    uint4 nxt = *reinterpret_cast<const uint4*>(a + 16);
    PolyRuns f;
    int run = 0;                                                          // equal pairs in a row in front of the dword
    for (; a <= hi && !f.cA; a += 16) {
        const uint4 ahead = *reinterpret_cast<const uint4*>(a + 32);
        const uint32_t w[5] = {cur.x, cur.y, cur.z, cur.w, nxt.x};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uintptr_t at = a + 4 * k;
            uint32_t x = w[k] ^ ((w[k] >> 8) | (w[k + 1] << 24));
            x |= census_mask_bytes((int64_t)(lo - at)) | ~census_mask_bytes((int64_t)(hi - at));
            if (x == 0) { run += 4; continue; }
            if (K >= 5) {
                const int t0 = __builtin_ctz(x) >> 3;
                if (run + t0 >= K - 1) f.note((w[k] >> (8 * t0)) & 0xffu, run + t0 + 1);
                run = __builtin_clz(x) >> 3;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((x >> (8 * j)) & 0xffu) {
                        if (run >= K - 1 && at + j >= lo && at + j <= hi) f.note((w[k] >> (8 * j)) & 0xffu, run + 1);
                        run = 0;
                    } else {
                        ++run;
                    }
                }
            }
        }
        cur = nxt;
        nxt = ahead;
    }
    if (f.cA) { base = 'A'; count = f.cA; }
    else if (f.cT) { base = 'T'; count = f.cT; }
    else if (f.cC) { base = 'C'; count = f.cC; }
    else if (f.cG) { base = 'G'; count = f.cG; }
}

// int() of name[a:b) as Python takes it: an optional sign, then at least one digit and nothing else.  More than 18 digits:
// `wide` (the host finishes the field from the name bytes)
__device__ __forceinline__ bool census_int(const uint8_t* name, int a, int b, long long& out, uint8_t& wide) {
    out = 0;
    const bool neg = a < b && name[a] == '-';
    if (a < b && (name[a] == '+' || name[a] == '-')) ++a;
    if (b <= a) return false;
    long long v = 0;
    for (int i = a; i < b; ++i) {
        if (!is_digit(name[i])) return false;
        v = v * 10 + (long long)(name[i] - '0');
    }
    if (b - a > 18) { wide = 1; v = 0; }
    out = neg ? -v : v;
    return true;
}

// statFileFastq's name handling (bubbleprocesser.py:361-381): re.search(r'\S+\:\d+\:\S+\:\d+\:\d+\:\d+\:\d+', name) with the
// regex engine's own order (leftmost start; first \S+ greedy, backing off to the previous ':'; \d+ runs maximal; second \S+
// greedy), items = match.split(':'), lane = items[3], tile_no = items[4] (surface / swath / camera its first three
// characters, tile the rest), x = items[5], y = items[6], each through int().  The same walk as parse_names_kernel, kept
// apart: the census keeps tile_no whole and all four digit groups.
__device__ inline uint8_t census_name(const uint8_t* __restrict__ name, int len, aqc_census_hit& h) {
    int m_s = -1, m_e = -1;
    for (int s = 0; s < len && m_s < 0; ++s) {
        if (is_space(name[s]) || (s > 0 && !is_space(name[s - 1]))) continue;   // a match that starts inside a token also starts at its head
        int E = s;
        while (E < len && !is_space(name[E])) ++E;
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
    if (m_s < 0) return AQC_CENSUS_NO_NAME;
    int fs[7], fe[7], nf = 0, a = m_s;
    for (int i = m_s; i <= m_e && nf < 7; ++i) {
        if (i == m_e || name[i] == ':') { fs[nf] = a; fe[nf] = i; ++nf; a = i + 1; }
    }
    // tile_no: surface = int(tile_no[0]), swath, camera, tile = int(tile_no[3:]), int(tile_no): all digits, at least 4
    const int t0 = fs[4], t1 = fe[4];
    if (t1 - t0 < 4) return AQC_CENSUS_RAISE;
    for (int i = t0; i < t1; ++i)
        if (!is_digit(name[i])) return AQC_CENSUS_RAISE;
    h.surface = (uint8_t)(name[t0] - '0');
    h.swath = (uint8_t)(name[t0 + 1] - '0');
    h.camera = (uint8_t)(name[t0 + 2] - '0');
    long long v;
    if (!census_int(name, fs[3], fe[3], v, h.wide)) return AQC_CENSUS_RAISE;
    h.lane = v;
    census_int(name, t0, t1, v, h.wide);
    h.tile_no = v;
    census_int(name, t0 + 3, t1, v, h.wide);
    h.tile = v;
    if (!census_int(name, fs[5], fe[5], v, h.wide)) return AQC_CENSUS_RAISE;
    h.x = v;
    if (!census_int(name, fs[6], fe[6], v, h.wide)) return AQC_CENSUS_RAISE;
    h.y = v;
    return AQC_CENSUS_OK;
}

// CENSUS_PER_THREAD records per thread (rows of TXT_BLOCK records): countPoly, then each polyX read compacted into `out` (room
// for n) behind the counter *n_out with its index, base, count and name line; census_names_kernel fills in the name fields.
// ONE atomic per workgroup of TXT_BLOCK * CENSUS_PER_THREAD records: same-address atomics serialise in L2 (~8 ns each), and one
// per wave of 64 records cost 2.9 ms for 10 M reads with 3 % polyX reads against 1.1 ms with none (round 7's first version).
constexpr int CENSUS_PER_THREAD = 8;

__global__ __launch_bounds__(TXT_BLOCK) void poly_census_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ seq_off,
                                                                const uint32_t* __restrict__ seq_len, const uint32_t* __restrict__ name_off,
                                                                const uint32_t* __restrict__ name_len, uint64_t n, int K, uint64_t first_index,
                                                                aqc_census_hit* __restrict__ out, unsigned long long* __restrict__ n_out,
                                                                int* __restrict__ status) {
    __shared__ unsigned int s_wave[TXT_BLOCK / WAVE];
    __shared__ unsigned long long s_base;
    const uint64_t r0 = (uint64_t)blockIdx.x * TXT_BLOCK * CENSUS_PER_THREAD + threadIdx.x;
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    uint32_t found[CENSUS_PER_THREAD];                    // per record: count << 8 | base (0: no polyX)
    unsigned int mine = 0;
#pragma unroll
    for (int j = 0; j < CENSUS_PER_THREAD; ++j) {
        const uint64_t r = r0 + (uint64_t)j * TXT_BLOCK;
        uint8_t base = 0;
        int count = 0;
        if (r < n) {
            const int len = (int)(seq_len[r] & LEN_MASK);
            if (len > AQC_MAX_READ_LEN) atomicCAS(status, 0, AQC_ERR_READ_TOO_LONG);
            else count_poly(text + seq_off[r], len, K, base, count);
        }
        found[j] = ((uint32_t)count << 8) | base;
        mine += base != 0;
    }
    // exclusive prefix of the hits over the workgroup: in the wave by shuffles, across the waves through LDS
    const unsigned int incl = wave_incl_sum_shfl(mine, lane);
    if (lane == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    unsigned int before = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < TXT_BLOCK / WAVE; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    if (total == 0) return;                               // (uniform over the workgroup)
    if (threadIdx.x == 0) s_base = atomicAdd(n_out, (unsigned long long)total);
    __syncthreads();
    unsigned long long at = s_base + before;
#pragma unroll
    for (int j = 0; j < CENSUS_PER_THREAD; ++j) {
        if (!(found[j] & 0xffu)) continue;
        const uint64_t r = r0 + (uint64_t)j * TXT_BLOCK;
        aqc_census_hit h{};
        h.index = first_index + r;
        h.name_off = name_off[r];
        h.name_len = name_len[r];
        h.base = (uint8_t)(found[j] & 0xffu);
        h.count = (int32_t)(found[j] >> 8);
        out[at++] = h;
    }
}

// thread per hit, grid-strided: the name walk runs with every lane of a wave on a name of its own (in poly_census_kernel only
// the few polyX lanes of a wave would walk while the others wait)
__global__ __launch_bounds__(TXT_BLOCK) void census_names_kernel(const uint8_t* __restrict__ text, aqc_census_hit* __restrict__ hits,
                                                                 const unsigned long long* __restrict__ n_hits) {
    const uint64_t m = *n_hits;
    for (uint64_t i = (uint64_t)blockIdx.x * TXT_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * TXT_BLOCK) {
        aqc_census_hit h = hits[i];
        h.status = census_name(text + h.name_off, (int)h.name_len, h);
        hits[i] = h;
    }
}

}  // namespace aqc
