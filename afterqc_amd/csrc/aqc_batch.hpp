// aqc_batch.hpp — a batch as it sits in HBM and what every stage shares about it: the batch / circle / statistics descriptors, how a
// device error is raised at a record, the workgroup-private counters and their flush, and the small kernels that bring an uploaded
// batch into the device form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afterqc_hip.h"

namespace aqc {

struct DevBatch {
    const uint8_t *seq1, *qual1, *seq2, *qual2;
    const uint32_t *off1, *qoff1, *off2, *qoff2;   // byte offsets into the arenas (a chunk / batch arena is < 4 GiB); qoff NULL = off
    const uint32_t *len1, *len2;
    const int32_t *aux_lane, *aux_tile, *aux_x, *aux_y;
    const uint8_t* aux_ok;
    uint64_t n;
    uint64_t first_index;
    // Records whose QUALITY line is not as long as their SEQUENCE line (the reference never compares the two: fastq.py:37-49
    // hands the lines over as they are, preprocesser.py:19-28 slices each string by its own length, :565-568 index each quality
    // string from its own end).  Such a mate carries LEN_IRR in its len word; qlen holds the quality line's length (low 31
    // bits; NULL: the batch has no such record) and the general kernel leaves the FINAL quality view of both mates of such a
    // record in qview (start | length << 16, relative to the quality line) for the writer and the post-filter statRead.
    const uint32_t *qlen1, *qlen2;
    uint32_t *qview1, *qview2;
};
constexpr uint32_t LEN_IRR = 0x80000000u, LEN_MASK = 0x7fffffffu;
// the quality-length words of a framed chunk (frame_records_kernel) carry two flags above the length: the quality line ends right
// at its '\n' (nothing stripped), and ALL FOUR lines of the record do — the record stands in the chunk exactly as a writer would
// write it
constexpr uint32_t QLEN_TAILNL = 0x80000000u, QLEN_CONTIG = 0x40000000u, QLEN_MASK = 0x3fffffffu;

struct DevCircles {
    const double *cx, *cy, *cr;
    const int32_t *lane, *tile;
    int32_t n;
};

struct DevStats {
    unsigned long long* counters;   // [AQC_N_COUNTERS]
    unsigned long long* ovl_hist;   // [AQC_QC_COLS]
    unsigned long long* dist_hist;  // [AQC_QC_COLS]
    int* status;                    // first error code raised on the device (0 = ok)
    // errors that END THE RUN AT A RECORD upstream (an exception inside the loop of preprocesser.py:411-631: KeyError of
    // util.complement / the error matrix, IndexError of a quality string too short for the walk, int() of a name field):
    // min over (record << 8 | -code), so that the host learns the EARLIEST such record — everything before it was written
    // upstream when the exception flew (~0 = none)
    unsigned long long* err_key;
};
__device__ __forceinline__ void raise_at_record(const DevStats& st, uint64_t rec, int code) {
    atomicCAS(st.status, 0, code);
    atomicMin(st.err_key, ((unsigned long long)rec << 8) | (unsigned long long)(unsigned int)(-code));
}

struct BlockAcc {
    unsigned long long counters[AQC_N_COUNTERS];
    unsigned int ovl_hist[AQC_QC_COLS];
    unsigned int dist_hist[AQC_QC_COLS];
};

// block-private counters -> the device's, once per workgroup
__device__ inline void flush_block_acc(BlockAcc& acc, const DevStats& st, int tid = -1) {
    if (tid < 0) tid = (int)threadIdx.x;
    for (int i = tid; i < AQC_N_COUNTERS; i += blockDim.x)
        if (acc.counters[i]) atomicAdd(&st.counters[i], acc.counters[i]);
    for (int i = tid; i < AQC_QC_COLS; i += blockDim.x) {
        if (acc.ovl_hist[i]) atomicAdd(&st.ovl_hist[i], (unsigned long long)acc.ovl_hist[i]);
        if (acc.dist_hist[i]) atomicAdd(&st.dist_hist[i], (unsigned long long)acc.dist_hist[i]);
    }
}

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
