// aqc_upload.hpp — the small kernels around an uploaded batch: the two that bring it into the device form (mark_irregular_kernel,
// narrow_offsets_kernel) and the one behind aqc_fetch_quality_views (quality_views_kernel).  It defines kernels: aqc_capi_run.hip is
// the one unit that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"
#include "aqc_batch.hpp"      // DevBatch, LEN_IRR

namespace aqc {

// an uploaded batch whose quality strings have lengths of their own (aqc_batch::qlen*): mark the mates that differ
__global__ void mark_irregular_kernel(uint32_t* __restrict__ len, const uint32_t* __restrict__ qlen, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && qlen[i] != len[i]) len[i] |= LEN_IRR;
}

// aqc_fetch_quality_views: the slice of the quality string that goes with the final read of every record
__global__ void quality_views_kernel(DevBatch b, const aqc_result* __restrict__ results, int mate, uint32_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t lw = mate == 0 ? b.len1[i] : b.len2[i];
    if ((lw & LEN_IRR) && b.qlen1) { out[i] = mate == 0 ? b.qview1[i] : b.qview2[i]; return; }
    const aqc_result r = results[i];
    out[i] = mate == 0 ? ((uint32_t)r.start1 | ((uint32_t)r.len1 << 16)) : ((uint32_t)r.start2 | ((uint32_t)r.len2 << 16));
}

// the caller's 64-bit byte offsets (struct aqc_batch) -> the 32-bit device form
__global__ void narrow_offsets_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)in[i];
}

}  // namespace aqc
