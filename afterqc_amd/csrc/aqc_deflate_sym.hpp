// aqc_deflate_sym.hpp — the length and distance symbols of DEFLATE (RFC 1951 3.2.5) in closed form, once, for the device gzip
// encoders (aqc_gzdev.hpp, aqc_gzlz.hpp) and the CPU program that runs their logic (tests/native/gzlz_selftest.cpp checks every
// length 3..258 and every distance 1..32768 against base and extra bits).  No tables: a table in constant memory indexed per
// lane is a vector load from memory per token (measured on the inflate side, aqc_gunzip_dev.hpp).  Needs no HIP.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DEFLATE_HD __host__ __device__ __forceinline__
#else
#define DEFLATE_HD inline
#endif

namespace aqc {

// length 3..258 -> length symbol - 257; distance 1..32768 -> distance symbol
DEFLATE_HD int len_sym(int len) {
    if (len == 258) return 28;
    if (len < 11) return len - 3;
    const int v = len - 3;                                          // 8 .. 254
    const int e = 31 - __builtin_clz((unsigned)v) - 2;              // extra bits: v in [8,16) -> 1, [16,32) -> 2, ...
    return 4 + 4 * e + ((v >> e) & 3);
}
DEFLATE_HD int dist_sym(int d) {
    if (d < 5) return d - 1;
    const int v = d - 1;                                            // >= 4
    const int e = 31 - __builtin_clz((unsigned)v) - 1;              // extra bits
    return 2 + 2 * e + ((v >> e) & 1);
}
// number of extra bits and base value of length symbol 257 + i / distance symbol i
DEFLATE_HD int len_extra(int i) { return (i < 8 || i == 28) ? 0 : (i - 4) >> 2; }
DEFLATE_HD int len_base(int i) { return i == 28 ? 258 : i < 8 ? 3 + i : 3 + ((4 + (i & 3)) << ((i - 4) >> 2)); }
DEFLATE_HD int dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }
DEFLATE_HD int dist_base(int i) { return i < 4 ? 1 + i : 1 + ((2 + (i & 1)) << ((i - 2) >> 1)); }

}  // namespace aqc
